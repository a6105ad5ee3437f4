"""Golden vectors for tests/test_median_gpu.py, recorded from the REAL reference program (oracle/_ref/filter_mrc_ref, built
by `make -C oracle ref_cli`).  The reference's median loop does not end once a neighbour is skipped, so only footprints of
the centre voxel alone complete: `-median 0` and `-median 0.5`, here with a mask, on the seeded 12^3 volume of volume().
The file holds the seed, the volume and mask built from it, and what the program wrote to -out for both radii."""
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import volgen  # noqa: E402

REF_CLI = os.path.join(os.path.dirname(os.path.dirname(HERE)), "oracle", "_ref", "filter_mrc_ref")
SEED = 20251
RADII = (0.0, 0.5)


def volume(seed=SEED):
    """-> (src, mask): 12^3 noise with a block of zeros of both signs, and a mask with about a quarter zeros."""
    rng = np.random.default_rng(seed)
    src = rng.normal(0.0, 10.0, (12, 12, 12)).astype(np.float32)
    src[:3, :4, :5] = 0.0
    src[:3, :4, 5:9] = -0.0
    mask = (rng.random((12, 12, 12)) > 0.25).astype(np.float32)
    return src, mask


def main():
    src, mask = volume()
    out = {"seed": np.int64(SEED), "src": src, "mask": mask}
    with tempfile.TemporaryDirectory() as d:
        volgen.write_mrc(os.path.join(d, "in.rec"), src, voxel_width=1.0)
        volgen.write_mrc(os.path.join(d, "mask.rec"), mask, voxel_width=1.0)
        for r in RADII:
            args = [REF_CLI, "-in", "in.rec", "-w", "1", "-mask", "mask.rec", "-median", repr(r), "-out", "out.rec"]
            env = dict(os.environ, OMP_NUM_THREADS="1")
            p = subprocess.run(args, cwd=d, capture_output=True, text=True, timeout=60, env=env)
            assert p.returncode == 0, (args, p.stderr[-2000:])
            out["out/%g" % r] = volgen.read_mrc(os.path.join(d, "out.rec"))
            os.remove(os.path.join(d, "out.rec"))
    path = os.path.join(HERE, "median.npz")
    np.savez_compressed(path, **out)
    print("wrote median.npz: %d bytes" % os.path.getsize(path))


if __name__ == "__main__":
    main()
