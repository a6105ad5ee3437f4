"""The inputs, point files and command lines of the distance-map tests (tests/test_distance.py, tests/test_distance_gpu.py)
and of the recorder of their goldens (tests/golden/make_golden_distance.py)."""
import numpy as np

SHAPE = (9, 8, 7)   # nz, ny, nx: a 7 x 8 x 9 volume; cap = 24^2 = 576


def volume(seed=9101):
    """Integers 0..9 as floats and a mask with about 70 % ones."""
    rng = np.random.default_rng(seed)
    v = rng.integers(0, 10, SHAPE).astype(np.float32)
    mask = (rng.random(SHAPE) < 0.7).astype(np.float32)
    return v, mask


def nan_volume():
    """The same volume with NaN voxels among the selected ones: next to and between voxels of the interval [3, 6]."""
    v, mask = volume()
    v = v.copy()
    v[4, 3:5, 2:5] = np.nan
    v[0, 0, 0] = np.nan
    return v, mask


def inputs():
    """name -> (volume, mask)"""
    return {"vol": volume(), "nanvol": nan_volume()}


# Coordinate files as text.  Physical units unless a line carries parentheses (IMOD's notation: 1-based voxels, and then
# the whole file is in voxels).  "phys" has a point outside the image and one farther away than cap at every voxel width
# used; rounding cases sit at .5 voxel boundaries for the widths 1, 1.3 and 2.5.
POINT_FILES = {
    "phys.txt": "# x y z in physical units\n"
                "5.0 7.5 2.5\n"
                "12.4 3.1 9.9\n"
                "3.25 16.25 1.3\n"
                "-6.0 10 5\n"
                "900 0 0\n",
    "imod.txt": "(3, 4, 5)\n"
                "Pixel (7, 1, 9) = 63\n"
                "(1 8 2)\n"
                "(0, 4, 12)\n",
    "outside.txt": "-7.6 5.2 2.6\n"
                   "10.4 30.0 11.7\n",
    "far.txt": "900 900 900\n",
    "empty.txt": "# no points at all\n",
    "queries.txt": "5.0 7.5 2.5\n"
                   "0 0 0\n"
                   "15.0 17.5 20.0\n"
                   "-6.0 10 5\n"
                   "40 3 3\n"
                   "900 0 0\n",
}

DIST = "dist.txt"   # the text file -distance-to-voxels writes

# name -> dict(input, mask, w, flags).  Flags name the point files above and DIST.
CASES = {
    "w1": dict(input="vol", mask=False, w=1.0, flags=["-distance-points", "phys.txt"]),
    "w2p5": dict(input="vol", mask=False, w=2.5, flags=["-distance-points", "phys.txt"]),
    "w1p3": dict(input="vol", mask=False, w=1.3, flags=["-distance-points", "phys.txt"]),
    "imod": dict(input="vol", mask=False, w=2.5, flags=["-distance-points", "imod.txt"]),
    "two_files": dict(input="vol", mask=False, w=2.5, flags=["-distance-points", "phys.txt", "-distance-points", "imod.txt"]),
    "outside": dict(input="vol", mask=False, w=2.6, flags=["-distance-points", "outside.txt"]),
    "far": dict(input="vol", mask=False, w=2.5, flags=["-distance-points", "far.txt"]),
    "no_points": dict(input="vol", mask=False, w=2.5, flags=["-distance-points", "empty.txt"]),
    "mask": dict(input="vol", mask=True, w=2.5, flags=["-distance-points", "phys.txt"]),
    "mask_out": dict(input="vol", mask=True, w=1.3, flags=["-distance-points", "imod.txt", "-mask-out", "-2"]),
    "bin2": dict(input="vol", mask=False, w=1.3, flags=["-bin", "2", "-distance-points", "phys.txt"]),
    "bin2_mask": dict(input="vol", mask=True, w=1.3, flags=["-bin", "2", "-distance-points", "imod.txt"]),
    "rescale": dict(input="vol", mask=False, w=1.3, flags=["-distance-points", "phys.txt", "-rescale", "0.5", "3"]),
    "mask_rescale_min_max": dict(input="vol", mask=True, w=2.5,
                                 flags=["-distance-points", "phys.txt", "-rescale-min-max", "0", "1"]),
    "voxels": dict(input="vol", mask=False, w=2.5, flags=["-distance-to-voxels", "queries.txt", DIST, "3", "6"]),
    "voxels_w1p3": dict(input="vol", mask=False, w=1.3, flags=["-distance-to-voxels", "queries.txt", DIST, "9", "9"]),
    "voxels_mask": dict(input="vol", mask=True, w=2.5, flags=["-distance-to-voxels", "queries.txt", DIST, "8.5", "20"]),
    "voxels_imod": dict(input="vol", mask=True, w=2.5, flags=["-distance-to-voxels", "imod.txt", DIST, "0", "0"]),
    "voxels_empty": dict(input="vol", mask=False, w=2.5, flags=["-distance-to-voxels", "queries.txt", DIST, "100", "200"]),
    "voxels_nan": dict(input="nanvol", mask=False, w=2.5, flags=["-distance-to-voxels", "queries.txt", DIST, "3", "6"]),
    "voxels_nan_mask": dict(input="nanvol", mask=True, w=1.0, flags=["-distance-to-voxels", "queries.txt", DIST, "-1", "0.5"]),
    "voxels_bin2": dict(input="vol", mask=False, w=1.3, flags=["-bin", "2", "-distance-to-voxels", "queries.txt", DIST, "4", "5"]),
}


def writes_distances(case):
    return "-distance-to-voxels" in case["flags"]


def command(case, exe, in_path, mask_path, out_path):
    args = [exe, "-in", in_path, "-w", repr(case["w"]), "-out", out_path]
    if case["mask"]:
        args += ["-mask", mask_path]
    return args + list(case["flags"])
