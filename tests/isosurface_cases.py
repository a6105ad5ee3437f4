"""The volumes of the isosurface tests.  Shapes are (nz, ny, nx); every case is meshed on both sides of its
level.  CASES: small enough for the Python restatement and the Python voxeliser.  DEVICE_CASES: compared between the device
and the host walk only -- rows past a wave and past a workgroup, the densest output, degenerate axes."""
import numpy as np

SIDES = ("below", "above")


class Case(object):
    def __init__(self, name, vol, iso):
        self.name = name
        self.vol = np.ascontiguousarray(vol, np.float32)
        self.iso = float(iso)
        assert self.vol.ndim == 3


def _noise(shape, seed):
    return np.random.RandomState(seed).standard_normal(shape).astype(np.float32)


def _special():
    """4 x 5 x 6 noise with NaN, +inf, -inf and adjacent +-inf voxels, some of them on the image's faces"""
    v = _noise((4, 5, 6), 11)
    inf, nan = np.inf, np.nan
    v[1, 2, 2] = nan
    v[1, 2, 3] = -1.0       # an inside node (below) next to a NaN
    v[2, 1, 1] = inf
    v[2, 1, 2] = -inf       # adjacent along x
    v[2, 2, 2] = inf        # ... and along y
    v[3, 3, 3] = -inf
    v[2, 3, 2] = inf        # ... and along the diagonal (1, 0, 1)
    v[0, 0, 0] = -inf       # a corner of the image
    v[0, 0, 1] = inf
    v[3, 4, 5] = nan
    v[3, 4, 4] = nan        # two NaNs side by side
    v[1, 4, 0] = inf        # on a face
    return v


def _sphere(n, radius, offset):
    z, y, x = np.meshgrid(*[np.arange(n, dtype=np.float64)] * 3, indexing="ij")
    c = (n - 1) / 2.0
    d = np.sqrt((x - c - offset[0]) ** 2 + (y - c - offset[1]) ** 2 + (z - c - offset[2]) ** 2)
    return (d - radius).astype(np.float32)


def build():
    c = []
    c.append(Case("one", np.zeros((1, 1, 1)), 0.5))                      # inside below: 14 vertices, 24 triangles
    v = np.ones((3, 3, 3))
    v[1, 1, 1] = -1.0
    c.append(Case("single", v, 0.0))                                     # one inside node (below)
    c.append(Case("all_in", np.zeros((2, 3, 4)), 0.5))                   # below: caps only; above: nothing
    c.append(Case("all_out", np.ones((2, 3, 4)), 0.5))                   # below: nothing; above: caps only
    c.append(Case("noise345", _noise((3, 4, 5), 1), 0.0))
    c.append(Case("noise547", _noise((5, 4, 7), 2), 0.0))
    c.append(Case("integers", np.random.RandomState(3).randint(0, 3, (5, 5, 5)), 1.0))   # a third of the voxels equal the level
    c.append(Case("special", _special(), 0.0))
    v = np.ones((4, 4, 4))
    v[1:3, 1:3, 1:3] = -1e-6
    c.append(Case("clamp", v, 0.0))                                      # t = 1e-6 and 1 - 1e-6 before the clamp
    c.append(Case("sphere", _sphere(12, 4.3, (0.3, -0.2, 0.1)), 0.0))
    return c


def build_device():
    c = []
    c.append(Case("row65", _noise((2, 3, 65), 21), 0.0))       # nx = 65: a row past one wave
    c.append(Case("row257", _noise((3, 5, 257), 22), 0.0))     # a row past a 256-lane workgroup
    c.append(Case("dense", _noise((9, 16, 17), 23), 0.0))      # about half inside: the densest output
    c.append(Case("line_x", _noise((1, 1, 300), 24), 0.0))
    c.append(Case("line_z", _noise((300, 1, 1), 25), 0.0))
    return c


CASES = build()
DEVICE_CASES = build_device()
