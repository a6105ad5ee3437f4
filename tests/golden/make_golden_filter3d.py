"""Golden vectors for tests/test_filter3d*.py, recorded from the REAL reference program (oracle/_ref/filter_mrc_ref, built
by `make -C oracle ref_cli`): for every case of filter3d_cases.CASES the image of -out and the A (and B) coefficients the
program prints on stderr.  Inputs are not stored: filter3d_cases.inputs rebuilds them from seeds.  A case whose reference
run does not exit 0 is left out and named."""
import os
import re
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import filter3d_cases as FC  # noqa: E402
import volgen  # noqa: E402

REF_CLI = os.path.join(os.path.dirname(os.path.dirname(HERE)), "oracle", "_ref", "filter_mrc_ref")


def run_reference(name, workdir):
    src, mask = FC.inputs(name)
    volgen.write_mrc(os.path.join(workdir, "in.rec"), src, voxel_width=1.0)
    args = [REF_CLI, "-in", "in.rec", "-w", "1", "-out", "out.rec"] + FC.CASES[name][2]
    if mask is not None:
        volgen.write_mrc(os.path.join(workdir, "mask.rec"), mask, voxel_width=1.0)
        args += ["-mask", "mask.rec"]
    if os.path.exists(os.path.join(workdir, "out.rec")):
        os.remove(os.path.join(workdir, "out.rec"))
    r = subprocess.run(args, cwd=workdir, capture_output=True, text=True)
    if r.returncode != 0:
        return None
    coeff = [float("nan"), float("nan")]
    for k, letter in enumerate("AB"):
        m = re.search(r"\b%s = (\S+)" % letter, r.stderr)
        if m:
            coeff[k] = float(m.group(1))
    return volgen.read_mrc(os.path.join(workdir, "out.rec")), np.array(coeff, np.float64)


def main():
    out = {}
    left_out = []
    with tempfile.TemporaryDirectory() as d:
        for name in sorted(FC.CASES):
            res = run_reference(name, d)
            if res is None:
                left_out.append(name)
                continue
            out[name + "/out"], out[name + "/AB"] = res
    path = os.path.join(HERE, "filter3d.npz")
    np.savez_compressed(path, **out)
    print("wrote filter3d.npz: %d cases, %d bytes; left out (reference did not exit 0): %s"
          % (len(out) // 2, os.path.getsize(path), left_out or "none"))


if __name__ == "__main__":
    main()
