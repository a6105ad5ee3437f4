"""Golden vectors for tests/test_extrema.py, recorded from the REAL reference program (oracle/_ref/filter_mrc_ref, built
by `make -C oracle`): for every case of extrema_cases.golden_cases() the two text files of -find-minima / -find-maxima
(byte for byte; empty where the program wrote none) and the label image of -out, with the input volumes and masks."""
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import extrema_cases as EC  # noqa: E402
import volgen  # noqa: E402

REF_CLI = os.path.join(os.path.dirname(os.path.dirname(HERE)), "oracle", "_ref", "filter_mrc_ref")


def run_reference(src, mask, case, workdir):
    vol, masked, kind, c, borders, thr = case
    volgen.write_mrc(os.path.join(workdir, "in.rec"), src, voxel_width=1.0)
    args = [REF_CLI, "-in", "in.rec", "-w", "1", "-out", "out.rec", "-neighbor-connectivity", str(c),
            "-boundary-extrema" if borders else "-ignore-boundary-extrema"]
    if masked:
        volgen.write_mrc(os.path.join(workdir, "mask.rec"), mask, voxel_width=1.0)
        args += ["-mask", "mask.rec"]
    if EC.KINDS[kind][0]:
        args += ["-find-minima", "min.txt"]
    if EC.KINDS[kind][1]:
        args += ["-find-maxima", "max.txt"]
    if thr:
        lo, hi = EC.THRESHOLDS[vol]
        args += ["-minima-threshold", repr(lo), "-maxima-threshold", repr(hi)]
    for f in ("min.txt", "max.txt", "out.rec"):
        if os.path.exists(os.path.join(workdir, f)):
            os.remove(os.path.join(workdir, f))
    r = subprocess.run(args, cwd=workdir, capture_output=True, text=True)
    assert r.returncode == 0, (args, r.stderr[-2000:])
    txt = []
    for f in ("min.txt", "max.txt"):
        p = os.path.join(workdir, f)
        txt.append(open(p, "rb").read() if os.path.exists(p) else b"")
    out = volgen.read_mrc(os.path.join(workdir, "out.rec"))
    lab = out.astype(np.int32)
    assert np.array_equal(lab.astype(np.float32), out)
    return txt[0], txt[1], lab


def main():
    vols, masks = EC.golden_volumes()
    out = {}
    for k in vols:
        out["vol/" + k] = vols[k]
        out["mask/" + k] = masks[k]
    with tempfile.TemporaryDirectory() as d:
        for case in EC.golden_cases():
            name = EC.case_name(case)
            mn, mx, lab = run_reference(vols[case[0]], masks[case[0]], case, d)
            out[name + "/min_txt"] = np.frombuffer(mn, np.uint8)
            out[name + "/max_txt"] = np.frombuffer(mx, np.uint8)
            out[name + "/labels"] = lab
    path = os.path.join(HERE, "extrema.npz")
    np.savez_compressed(path, **out)
    print("wrote extrema.npz: %d cases, %d bytes" % (len(EC.golden_cases()), os.path.getsize(path)))


if __name__ == "__main__":
    main()
