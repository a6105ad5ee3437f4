"""Golden vectors for tests/test_distance.py and tests/test_distance_gpu.py, recorded from the REAL reference program
(oracle/_ref/filter_mrc_ref, built by `make -C oracle ref_cli`): for every case of tests/distance_cases.py what the program
wrote to -out, the dmin, dmax, dmean of that file's header and, for -distance-to-voxels, the text of the distance file.
Inputs, masks, point files (as text) and outputs only."""
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import distance_cases as dc  # noqa: E402
import volgen  # noqa: E402

REF_CLI = os.path.join(os.path.dirname(os.path.dirname(HERE)), "oracle", "_ref", "filter_mrc_ref")


def header_stats(path):
    with open(path, "rb") as f:
        return np.frombuffer(f.read(1024), "<f4")[19:22].copy()


def text(s):
    return np.frombuffer(s.encode() if isinstance(s, str) else s, np.uint8).copy()


def main():
    out = {}
    for name, (vol, mask) in dc.inputs().items():
        out["in/" + name] = vol
        out["mask/" + name] = mask
    for name, body in dc.POINT_FILES.items():
        out["points/" + name] = text(body)
    env = dict(os.environ, OMP_NUM_THREADS="1")
    with tempfile.TemporaryDirectory() as d:
        for name, body in dc.POINT_FILES.items():
            with open(os.path.join(d, name), "w") as f:
                f.write(body)
        for name, case in dc.CASES.items():
            vol, mask = dc.inputs()[case["input"]]
            volgen.write_mrc(os.path.join(d, "in.rec"), vol, voxel_width=case["w"])
            volgen.write_mrc(os.path.join(d, "mask.rec"), mask, voxel_width=case["w"])
            args = dc.command(case, REF_CLI, "in.rec", "mask.rec", "out.rec")
            p = subprocess.run(args, cwd=d, capture_output=True, text=True, timeout=120, env=env)
            assert p.returncode == 0, (args, p.stderr[-2000:])
            out["out/" + name] = volgen.read_mrc(os.path.join(d, "out.rec"))
            out["header/" + name] = header_stats(os.path.join(d, "out.rec"))
            os.remove(os.path.join(d, "out.rec"))
            if dc.writes_distances(case):
                with open(os.path.join(d, dc.DIST), "rb") as f:
                    out["dist/" + name] = text(f.read())
                os.remove(os.path.join(d, dc.DIST))
    path = os.path.join(HERE, "distance.npz")
    np.savez_compressed(path, **out)
    print("wrote distance.npz: %d bytes, %d arrays" % (os.path.getsize(path), len(out)))


if __name__ == "__main__":
    main()
