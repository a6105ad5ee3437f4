"""Meshes for the voxeliser's tests: vertices float32 (n, 3) as x, y, z in voxels, triangles int32 (m, 3).  Every closed
case exists at two image shapes: 20 x 17 x 13 and 70 x 9 x 7 (three toggle words per row, nx no multiple of 32, a carry
across words)."""
import numpy as np

SHAPES = {"s20": (13, 17, 20), "s70": (7, 9, 70)}   # (nz, ny, nx)


def _mesh(v, t):
    return np.asarray(v, np.float32).reshape(-1, 3), np.asarray(t, np.int32).reshape(-1, 3)


BOX_QUADS = [(0, 2, 6, 4), (1, 5, 7, 3), (0, 4, 5, 1), (2, 3, 7, 6), (0, 1, 3, 2), (4, 6, 7, 5)]   # x-, x+, y-, y+, z-, z+


def box_vertices(lo, hi):
    return [(hi[0] if i & 1 else lo[0], hi[1] if i & 2 else lo[1], hi[2] if i & 4 else lo[2]) for i in range(8)]


def box(lo, hi):
    """12 triangles; triangles 0-3 are the two faces across x"""
    t = []
    for a, b, c, d in BOX_QUADS:
        t += [(a, b, c), (a, c, d)]
    return _mesh(box_vertices(lo, hi), t)


def icosphere(center, radii, subdivisions):
    g = (1.0 + 5.0 ** 0.5) / 2.0
    v = [(-1, g, 0), (1, g, 0), (-1, -g, 0), (1, -g, 0), (0, -1, g), (0, 1, g), (0, -1, -g), (0, 1, -g), (g, 0, -1), (g, 0, 1),
         (-g, 0, -1), (-g, 0, 1)]
    v = [tuple(np.array(p, np.float64) / np.linalg.norm(p)) for p in v]
    t = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8),
         (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    for _ in range(subdivisions):
        mid, t2 = {}, []

        def midpoint(a, b):
            k = (min(a, b), max(a, b))
            if k not in mid:
                p = (np.array(v[a]) + np.array(v[b])) / 2.0
                v.append(tuple(p / np.linalg.norm(p)))
                mid[k] = len(v) - 1
            return mid[k]
        for a, b, c in t:
            ab, bc, ca = midpoint(a, b), midpoint(b, c), midpoint(c, a)
            t2 += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        t = t2
    return _mesh(np.array(v) * np.array(radii, np.float64) + np.array(center, np.float64), t)


def torus(center, R, r, nu, nv, scale=(1.0, 1.0, 1.0)):
    v, t = [], []
    for i in range(nu):
        a = 2.0 * np.pi * i / nu
        for j in range(nv):
            b = 2.0 * np.pi * j / nv
            v.append(((R + r * np.cos(b)) * np.cos(a), (R + r * np.cos(b)) * np.sin(a), r * np.sin(b)))
    for i in range(nu):
        for j in range(nv):
            p, q = i * nv + j, i * nv + (j + 1) % nv
            s, u = ((i + 1) % nu) * nv + j, ((i + 1) % nu) * nv + (j + 1) % nv
            t += [(p, s, u), (p, u, q)]
    return _mesh(np.array(v) * np.array(scale, np.float64) + np.array(center, np.float64), t)


def octahedron(center, radii):
    c, r = np.array(center, np.float64), np.array(radii, np.float64)
    v = [c + (r[0], 0, 0), c - (r[0], 0, 0), c + (0, r[1], 0), c - (0, r[1], 0), c + (0, 0, r[2]), c - (0, 0, r[2])]
    t = [(0, 2, 4), (2, 1, 4), (1, 3, 4), (3, 0, 4), (2, 0, 5), (1, 2, 5), (3, 1, 5), (0, 3, 5)]
    return _mesh(v, t)


# name -> shape key -> () -> (vertices, triangles); the five off-grid meshes have no sample exactly on their surface
OFF_GRID = {
    "box_off_grid": {"s20": lambda: box((2.3, 1.7, 3.1), (15.6, 14.2, 9.9)),
                     "s70": lambda: box((2.3, 1.7, 1.1), (65.6, 7.2, 5.9))},
    "box_beyond_image": {"s20": lambda: box((-5.5, -3.25, 2.5), (40.5, 30.25, 7.75)),
                         "s70": lambda: box((-5.5, -3.25, 1.5), (90.5, 30.25, 4.75))},
    "icosphere_coarse": {"s20": lambda: icosphere((9.21, 8.13, 6.4), (5.37, 5.37, 5.37), 2),
                         "s70": lambda: icosphere((34.21, 4.13, 3.4), (30.37, 3.37, 2.87), 2)},
    "torus": {"s20": lambda: torus((9.6, 8.4, 6.3), 5.5, 2.2, 24, 12),
              "s70": lambda: torus((35.6, 4.4, 3.3), 1.0, 0.4, 24, 12, (22.0, 2.2, 5.5))},
    "icosphere_fine": {"s20": lambda: icosphere((7.77, 6.31, 5.55), (3.3, 3.3, 3.3), 4),
                       "s70": lambda: icosphere((33.77, 4.31, 3.55), (20.3, 3.3, 2.8), 4)},
}
ON_GRID = {
    "box_on_samples": {"s20": lambda: box((3, 2, 2), (15, 12, 9)), "s70": lambda: box((4, 1, 1), (66, 7, 5))},
    "octahedron_on_samples": {"s20": lambda: octahedron((10, 8, 6), (5, 5, 5)),
                              "s70": lambda: octahedron((35, 4, 3), (30, 3, 2))},
}
# octahedra of about 10^5 voxels' radius whose +x faces pass through samples of the image: cross products beyond 2^53,
# plane functions beyond 2^64, every crossing exactly on a sample
HUGE = {
    "octahedron_huge": {"s20": lambda: octahedron((-99990, 8, 6), (100003, 100003, 100003)),
                        "s70": lambda: octahedron((-99960, 4, 3), (100003, 100001, 99999))},
}
CLOSED = dict(OFF_GRID)
CLOSED.update(ON_GRID)
CLOSED.update(HUGE)

# the figures of a Python-integer prototype of the rule at 20 x 17 x 13: inside samples of the off-grid meshes
PROTOTYPE_INSIDE = {"box_off_grid": 1014, "box_beyond_image": 1700, "icosphere_coarse": 625, "torus": 491, "icosphere_fine": 153}


def box_open():
    """the off-grid box without its x+ face: 4 boundary edges; rows through the hole have one crossing"""
    v, t = box((2.3, 1.7, 3.1), (15.6, 14.2, 9.9))
    return v, np.ascontiguousarray(np.delete(t, [2, 3], axis=0))


def box_duplicated():
    """the off-grid box with the first triangle of its x- face listed twice: its 3 edges are used three times"""
    v, t = box((2.3, 1.7, 3.1), (15.6, 14.2, 9.9))
    return v, np.ascontiguousarray(np.concatenate([t, t[:1]]))


def box_with_sliver():
    """the box with one edge of its x- face split at its midpoint and the gap closed by a triangle of three collinear
    vertices: closed and manifold, one triangle of area zero next to the eight whose projection along x is a segment"""
    lo, hi = (2.5, 1.5, 3.0), (15.5, 14.5, 9.0)
    v, t = box(lo, hi)
    t = t.tolist()
    a, b, c = t[0]                         # (0, 2, 6): the edge 0-2 runs along y and is shared with the z- face
    m = len(v)
    v = np.concatenate([v, ((v[a] + v[b]) / 2)[None, :]]).astype(np.float32)
    t = [(a, m, c), (m, b, c)] + t[1:] + [(b, a, m)]
    return _mesh(v, t)


def box_quads():
    """the off-grid box as six quadrilaterals (for the PLY reader's fans)"""
    return np.asarray(box_vertices((2.3, 1.7, 3.1), (15.6, 14.2, 9.9)), np.float32), [list(q) for q in BOX_QUADS]
