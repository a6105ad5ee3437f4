"""The isosurface definition (include/visfd_hip.h) restated in plain Python and numpy: marching tetrahedra
on the Kuhn split of every cell of the image with one layer of outside border nodes.  Written from the text of the definition:
vertices live in a dictionary keyed by (lower node, direction), polygons are oriented by the cross product of the edge
midpoints each time a tet is met.  Slow on purpose; the tests use it on small volumes only."""
import itertools

import numpy as np

BELOW, ABOVE = 0, 1
DIRS = ((1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 0), (0, 1, 1), (1, 0, 1), (1, 1, 1))
PERMS = tuple(itertools.permutations((0, 1, 2)))   # lexicographic: xyz, xzy, yxz, yzx, zxy, zyx
T_LO, T_HI = np.float64(1.0) / np.float64(64.0), np.float64(63.0) / np.float64(64.0)


def tet_corners(perm):
    """the 4 corner offsets (x, y, z) of the tet 0, e_a, e_a + e_b, e_a + e_b + e_c"""
    c = [(0, 0, 0)]
    for axis in perm:
        o = list(c[-1])
        o[axis] += 1
        c.append(tuple(o))
    return c


def inside_set(vol, iso, side):
    """bool [nz, ny, nx]: the inside image nodes"""
    v = np.asarray(vol, np.float32).astype(np.float64)
    with np.errstate(invalid="ignore"):
        return (v < np.float64(iso)) if side == BELOW else (v > np.float64(iso))


def isosurface(vol, iso, side):
    """-> (vertices float32 (n, 3) x y z, triangles int32 (m, 3))"""
    vol = np.asarray(vol, np.float32)
    nz, ny, nx = vol.shape
    size = (nx, ny, nz)
    iso = np.float64(iso)
    ins = inside_set(vol, iso, side)

    def is_image(p):
        return all(0 <= p[d] < size[d] for d in range(3))

    def inside(p):
        return is_image(p) and bool(ins[p[2], p[1], p[0]])

    def key(a):
        return ((a[2] + 1) * (ny + 1) + (a[1] + 1)) * (nx + 1) + (a[0] + 1)

    def vertex(a, cls):
        d = DIRS[cls]
        b = (a[0] + d[0], a[1] + d[1], a[2] + d[2])
        t = np.float64(0.5)
        if is_image(a) and is_image(b):
            va, vb = np.float64(vol[a[2], a[1], a[0]]), np.float64(vol[b[2], b[1], b[0]])
            with np.errstate(all="ignore"):
                t = (iso - va) / (vb - va)
            if not np.isfinite(t):
                t = np.float64(0.5)
            t = min(max(t, T_LO), T_HI)
        return [np.float32(np.float64(a[k]) + t) if d[k] else np.float32(a[k]) for k in range(3)]

    found = {}      # key(a) * 7 + class -> (a, class)
    polygons = []   # lists of such numbers, in order (cell key, tet index)
    for az in range(-1, nz):
        for ay in range(-1, ny):
            for ax in range(-1, nx):
                for perm in PERMS:
                    corners = [(ax + o[0], ay + o[1], az + o[2]) for o in tet_corners(perm)]
                    flags = [inside(c) for c in corners]
                    I = [k for k in range(4) if flags[k]]
                    O = [k for k in range(4) if not flags[k]]
                    if not I or not O:
                        continue
                    if len(I) == 1:
                        pairs = [(I[0], o) for o in O]
                    elif len(I) == 3:
                        pairs = [(i, O[0]) for i in I]
                    else:
                        pairs = [(I[0], O[0]), (I[0], O[1]), (I[1], O[1]), (I[1], O[0])]
                    mid = [(np.array(corners[i], np.float64) + np.array(corners[o], np.float64)) / 2 for i, o in pairs]
                    normal = np.cross(mid[1] - mid[0], mid[2] - mid[0])
                    to_inside = (np.mean([corners[i] for i in I], axis=0) - np.mean([corners[o] for o in O], axis=0))
                    if np.dot(normal, to_inside) > 0:
                        pairs = pairs[::-1]
                    poly = []
                    for i, o in pairs:
                        lo, hi = min(i, o), max(i, o)   # later tet corners are the upper ends
                        a = corners[lo]
                        cls = DIRS.index(tuple(corners[hi][k] - a[k] for k in range(3)))
                        number = key(a) * 7 + cls
                        found[number] = (a, cls)
                        poly.append(number)
                    polygons.append(poly)
    order = sorted(found)
    index = {number: k for k, number in enumerate(order)}
    vertices = np.array([vertex(*found[number]) for number in order], np.float32).reshape(-1, 3)
    tris = []
    for poly in polygons:
        p = [index[number] for number in poly]
        tris.append((p[0], p[1], p[2]))
        if len(p) == 4:
            tris.append((p[0], p[2], p[3]))
    return vertices, np.array(tris, np.int32).reshape(-1, 3)


def signed_volume(vertices, triangles):
    """the mesh's volume by the divergence theorem, positive for outward normals (float64)"""
    v = np.asarray(vertices, np.float64)
    t = np.asarray(triangles, np.int64).reshape(-1, 3)
    if not len(t):
        return 0.0
    a, b, c = v[t[:, 0]], v[t[:, 1]], v[t[:, 2]]
    return float(np.einsum("ij,ij->i", a, np.cross(b, c)).sum() / 6.0)


def scale_vertices(vertices, width):
    """voxel coordinates to physical units as the command line does it: the product in double, rounded to float"""
    return (np.asarray(vertices, np.float32).astype(np.float64) * np.float64(width)).astype(np.float32)
