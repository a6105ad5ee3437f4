"""The point clouds of the close_surface tests: seeded samples of a sphere, about 1.5 per unit area, with
unit outward normals and the centre off the lattice by (0.3, -0.2, 0.1); some with their polar caps removed (the missing
wedge), one on a thin box, one tiny, one with points that must be skipped, one empty.  Everything is float32, (x, y, z)."""
import numpy as np

OFFSET = (0.3, -0.2, 0.1)
DENSITY = 1.5


class Case(object):
    def __init__(self, name, shape, points, normals, pad=0, orientation="outward", center=None, radius=None, cap=None,
                 n_used=None, n_skipped=0):
        self.name = name
        self.shape = tuple(shape)          # (nz, ny, nx)
        self.points = np.ascontiguousarray(points, np.float32).reshape(-1, 3)
        self.normals = np.ascontiguousarray(normals, np.float32).reshape(-1, 3)
        self.pad = pad
        self.orientation = orientation
        self.center, self.radius, self.cap = center, radius, cap    # the sphere behind the cloud (None: no geometry checks)
        self.n_used = len(self.points) if n_used is None else n_used
        self.n_skipped = n_skipped


def sphere_cloud(shape, r, cap, seed):
    """-> points, normals, centre (x, y, z): samples with |z - cz| / r <= cap (cap None: all)"""
    nz, ny, nx = shape
    c = np.array([(nx - 1) / 2.0 + OFFSET[0], (ny - 1) / 2.0 + OFFSET[1], (nz - 1) / 2.0 + OFFSET[2]])
    rng = np.random.RandomState(seed)
    n = int(round(DENSITY * 4.0 * np.pi * r * r))
    d = rng.standard_normal((n, 3))
    d /= np.linalg.norm(d, axis=1)[:, None]
    if cap is not None:
        d = d[np.abs(d[:, 2]) <= cap]
    return (c + r * d).astype(np.float32), d.astype(np.float32), tuple(c)


def _sphere_case(name, shape, r, cap, seed, **kw):
    p, n, c = sphere_cloud(shape, r, cap, seed)
    return Case(name, shape, p, n, center=c, radius=r, cap=1.0 if cap is None else cap, **kw)


def _ring(shape, r, seed):
    nz, ny, nx = shape
    c = np.array([(nx - 1) / 2.0 + OFFSET[0], (ny - 1) / 2.0 + OFFSET[1], (nz - 1) / 2.0 + OFFSET[2]])
    rng = np.random.RandomState(seed)
    a = rng.uniform(0.0, 2.0 * np.pi, int(round(DENSITY * 2.0 * np.pi * r)))
    d = np.stack([np.cos(a), np.sin(a), np.zeros_like(a)], 1)
    return (c + r * d).astype(np.float32), d.astype(np.float32)


def _junk(base):
    """caps75 plus points that must be counted as skipped"""
    nz, ny, nx = base.shape
    inf, nan = np.inf, np.nan
    bad_p = [(nan, 10, 10), (10, inf, 10), (10, 10, -inf), (10, 10, 10), (10, 10, 10), (10, 10, 10),
             (-0.5, 10, 10), (10, -3.0, 10), (10, 10, nz + 5.0), (1e30, 10, 10), (-1e30, 10, 10),
             (nx - 0.75, 10, 10), (10, ny - 0.5, 10), (10, 10, nz - 0.25), (nx - 1.0, 10, 10), (10, ny - 1.0, 10)]
    bad_n = [(1, 0, 0)] * 3 + [(nan, 0, 0), (0, inf, 0), (0, 0, -inf)] + [(0, 1, 0)] * 10
    good_p = [(0.0, 0.0, 0.0), (nx - 1.5, ny - 1.25, nz - 2.0)]        # the first and the last cell: used
    good_n = [(0, 0, 0), (0, 0, 0)]                                    # with null normals: they move the level only
    k = len(base.points) // 2
    p = np.concatenate([base.points[:k], np.array(bad_p, np.float32), base.points[k:], np.array(good_p, np.float32)])
    n = np.concatenate([base.normals[:k], np.array(bad_n, np.float32), base.normals[k:], np.array(good_n, np.float32)])
    return Case("junk", base.shape, p, n, n_used=len(base.points) + len(good_p), n_skipped=len(bad_p))


def build():
    c = {}
    c["full"] = _sphere_case("full", (48, 48, 48), 14.3, None, 1)
    c["caps75"] = _sphere_case("caps75", (48, 48, 48), 14.3, 0.75, 1)
    c["caps60"] = _sphere_case("caps60", (48, 48, 48), 14.3, 0.6, 1)
    c["odd"] = _sphere_case("odd", (44, 36, 40), 9.0, 0.75, 2)
    p, n = _ring((3, 33, 37), 10.0, 3)
    c["thin"] = Case("thin", (3, 33, 37), p, n)
    c["tiny"] = Case("tiny", (3, 4, 5), [(1.25, 1.5, 0.75), (2.5, 1.75, 1.0)], [(-1, 0, 0), (1, 0, 0)])
    c["padded"] = _sphere_case("padded", (44, 36, 40), 9.0, 0.75, 2, pad=5)
    b = c["caps75"]
    c["inward"] = Case("inward", b.shape, b.points, -b.normals, orientation="inward", center=b.center, radius=b.radius,
                       cap=b.cap)
    c["junk"] = _junk(b)
    c["empty"] = Case("empty", (5, 6, 7), np.zeros((0, 3)), np.zeros((0, 3)), n_used=0)
    return c


CASES = build()
SPHERE_CASES = ("full", "caps75", "caps60", "odd", "padded")
