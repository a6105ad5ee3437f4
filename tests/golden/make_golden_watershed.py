"""Golden vectors for tests/test_watershed.py, recorded from the REAL reference program (oracle/_ref/filter_mrc_ref, built
by `make -C oracle`): for every case of watershed_cases.golden_cases() the image that `-watershed` wrote to -out (whole
numbers, stored as int32), with the input volumes, masks and marker images."""
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import volgen  # noqa: E402
import watershed_cases as WC  # noqa: E402

REF_CLI = os.path.join(os.path.dirname(os.path.dirname(HERE)), "oracle", "_ref", "filter_mrc_ref")


def reference_flags(case):
    """The program's flags for a case; the threshold comes after -watershed, which would otherwise reset it."""
    vol, masked, kind, c, show, thr, mk, lb, und = case
    args = ["-watershed", "minima" if kind == "min" else "maxima", "-neighbor-connectivity", str(c),
            "-watershed-show-boundaries" if show else "-watershed-hide-boundaries"]
    if thr:
        args += ["-watershed-threshold", repr(WC.THRESHOLDS[vol][0 if kind == "min" else 1])]
    if lb:
        args += ["-watershed-boundary", str(lb)]
    if und != "max":
        args += ["-undefined-out", str(und)]
    return args


def run_reference(src, mask, markers, case, workdir):
    volgen.write_mrc(os.path.join(workdir, "in.rec"), src, voxel_width=1.0)
    args = [REF_CLI, "-in", "in.rec", "-w", "1", "-out", "out.rec"] + reference_flags(case)
    if case[1]:
        volgen.write_mrc(os.path.join(workdir, "mask.rec"), mask, voxel_width=1.0)
        args += ["-mask", "mask.rec"]
    if markers is not None:
        volgen.write_mrc(os.path.join(workdir, "markers.rec"), markers, voxel_width=1.0)
        args += ["-markers", "markers.rec"]
    if os.path.exists(os.path.join(workdir, "out.rec")):
        os.remove(os.path.join(workdir, "out.rec"))
    r = subprocess.run(args, cwd=workdir, capture_output=True, text=True)
    assert r.returncode == 0, (args, r.stderr[-2000:])
    out = volgen.read_mrc(os.path.join(workdir, "out.rec"))
    lab = out.astype(np.int32)
    assert np.array_equal(lab.astype(np.float32), out)
    return lab


def main():
    vols, masks = WC.golden_volumes()
    out = {}
    for k in vols:
        out["vol/" + k] = vols[k]
        out["mask/" + k] = masks[k]
    with tempfile.TemporaryDirectory() as d:
        for case in WC.golden_cases():
            vol, mk = case[0], case[6]
            markers = None
            if mk:
                markers = WC.marker_volume(mk, vols[vol].shape, masks[vol])
                out["markers/%s/%s" % (mk, vol)] = markers
            out[WC.case_name(case) + "/out"] = run_reference(vols[vol], masks[vol], markers, case, d)
    path = os.path.join(HERE, "watershed.npz")
    np.savez_compressed(path, **out)
    print("wrote watershed.npz: %d cases, %d bytes" % (len(WC.golden_cases()), os.path.getsize(path)))


if __name__ == "__main__":
    main()
