"""The voxeliser's rule (include/visfd_hip.h) restated in Python integers: the quantisation in numpy
float64, the cover test, the exact crossing, the parity fill and the edge census.  Also an exact on-surface test and a
ray-axis parameter, which only the oracle's own checks use (the product's rays run along x)."""
import numpy as np

Q = 1024
QMAX = 1 << 29


class Refused(Exception):
    pass


def quantize(vertices, voxel_width=1.0, origin=(0.0, 0.0, 0.0)):
    """nearbyint(((double)v / w - origin) * 1024), ties to even -> int64 array (n, 3) of values within +-2^29."""
    w = float(voxel_width)
    if w == 0.0 or not np.isfinite(w):
        raise Refused("voxel width")
    v = np.asarray(vertices, np.float32).reshape(-1, 3)
    if not np.isfinite(v).all():
        raise Refused("vertex not finite")
    with np.errstate(all="ignore"):
        t = v.astype(np.float64) / np.float64(w)
        t = t - np.asarray(origin, np.float64)[None, :]
        t = t * np.float64(1024.0)
        r = np.rint(t)
    if not (np.abs(r) <= float(QMAX)).all():
        raise Refused("vertex out of range")
    return r.astype(np.int64)


def edges(triangles, n_vertices):
    """(boundary edges, non-manifold edges): undirected edges used by exactly one triangle, and by more than two."""
    t = np.asarray(triangles, np.int64).reshape(-1, 3)
    if t.size and (t.min() < 0 or t.max() >= n_vertices):
        raise Refused("index out of range")
    count = {}
    for a, b, c in t.tolist():
        for e in ((a, b), (b, c), (c, a)):
            k = (min(e), max(e))
            count[k] = count.get(k, 0) + 1
    return sum(1 for n in count.values() if n == 1), sum(1 for n in count.values() if n > 2)


def _sgn(v):
    return (v > 0) - (v < 0)


def _side(a, b, pu, pv):
    du, dv = b[0] - a[0], b[1] - a[1]
    E = du * (pv - a[1]) - dv * (pu - a[0])
    if E:
        return _sgn(E)
    if dv:
        return -_sgn(dv)
    return _sgn(du)


def _ceil_div(a, b):
    return -((-a) // b)


_PERM = {0: (0, 1, 2), 1: (1, 2, 0), 2: (2, 0, 1)}


def voxelize_q(q, triangles, shape, axis=0):
    """The rule on quantised vertices q (n, 3) and an image of shape (nz, ny, nx), rays along `axis` (0: x, the product's).
    -> (image float32 [nz, ny, nx], crossings, skipped triangles, odd rows)."""
    nz, ny, nx = shape
    size = (nx, ny, nz)
    p = _PERM[axis]
    n0, n1, n2 = size[p[0]], size[p[1]], size[p[2]]   # ray axis, u axis, v axis
    pts = [tuple(int(row[k]) for k in p) for row in np.asarray(q).tolist()]
    toggles = np.zeros((n2, n1, n0 + 1), np.uint8)
    crossings = skipped = 0
    for ia, ib, ic in np.asarray(triangles, np.int64).reshape(-1, 3).tolist():
        A, B, C = pts[ia], pts[ib], pts[ic]
        bx, by, bz = B[0] - A[0], B[1] - A[1], B[2] - A[2]
        cx, cy, cz = C[0] - A[0], C[1] - A[1], C[2] - A[2]
        Nx, Ny, Nz = by * cz - bz * cy, bz * cx - bx * cz, bx * cy - by * cx
        if Nx == 0:
            skipped += 1
            continue
        s = _sgn(Nx)
        u0 = max(_ceil_div(min(A[1], B[1], C[1]), Q), 0)
        u1 = min(max(A[1], B[1], C[1]) // Q, n1 - 1)
        v0 = max(_ceil_div(min(A[2], B[2], C[2]), Q), 0)
        v1 = min(max(A[2], B[2], C[2]) // Q, n2 - 1)
        a2, b2, c2 = A[1:], B[1:], C[1:]
        for iv in range(v0, v1 + 1):
            for iu in range(u0, u1 + 1):
                pu, pv = Q * iu, Q * iv
                if _side(a2, b2, pu, pv) != s or _side(b2, c2, pu, pv) != s or _side(c2, a2, pu, pv) != s:
                    continue
                num = A[0] * Nx - Ny * (pu - A[1]) - Nz * (pv - A[2])   # x_c = num / Nx
                k = num // (Q * Nx) + 1                               # Python's // is the floor for either sign
                k = min(max(k, 0), n0)
                toggles[iv, iu, k] ^= 1
                crossings += 1
    par = np.bitwise_xor.accumulate(toggles, axis=2)
    odd_rows = int(par[:, :, n0].sum())
    inside = par[:, :, :n0]                      # indexed [i2][i1][i0]
    # back to [iz][iy][ix]: axis j of the image is position p.index(j) of (i0, i1, i2)
    src_axes = {p[0]: 2, p[1]: 1, p[2]: 0}      # image axis (0: x, 1: y, 2: z) -> axis of `inside`
    img = np.transpose(inside, (src_axes[2], src_axes[1], src_axes[0]))
    return np.ascontiguousarray(img).astype(np.float32), crossings, skipped, odd_rows


def voxelize(vertices, triangles, shape, voxel_width=1.0, origin=(0.0, 0.0, 0.0), axis=0):
    return voxelize_q(quantize(vertices, voxel_width, origin), triangles, shape, axis)


def on_surface(q, triangles, shape):
    """bool [nz, ny, nx]: the samples 1024 (ix, iy, iz) that lie exactly on a triangle (its edges and corners included), in
    exact integers."""
    nz, ny, nx = shape
    size = (nx, ny, nz)
    out = np.zeros(shape, bool)
    pts = [tuple(int(x) for x in row) for row in np.asarray(q).tolist()]

    def sub(a, b):
        return (a[0] - b[0], a[1] - b[1], a[2] - b[2])

    def cross(a, b):
        return (a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0])

    def dot(a, b):
        return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]

    def on_segment(P, A, B):
        d, e = sub(B, A), sub(P, A)
        return cross(d, e) == (0, 0, 0) and 0 <= dot(d, e) <= dot(d, d)

    for ia, ib, ic in np.asarray(triangles, np.int64).reshape(-1, 3).tolist():
        A, B, C = pts[ia], pts[ib], pts[ic]
        N = cross(sub(B, A), sub(C, A))
        lo = [max(_ceil_div(min(A[d], B[d], C[d]), Q), 0) for d in range(3)]
        hi = [min(max(A[d], B[d], C[d]) // Q, size[d] - 1) for d in range(3)]
        for iz in range(lo[2], hi[2] + 1):
            for iy in range(lo[1], hi[1] + 1):
                for ix in range(lo[0], hi[0] + 1):
                    P = (Q * ix, Q * iy, Q * iz)
                    if N == (0, 0, 0):
                        hit = on_segment(P, A, B) or on_segment(P, B, C) or on_segment(P, C, A)
                    elif dot(N, sub(P, A)) != 0:
                        hit = False
                    else:   # in the plane: inside or on the border iff no edge sees it on the outer side
                        w = [dot(N, cross(sub(Y, X), sub(P, X))) for X, Y in ((A, B), (B, C), (C, A))]
                        hit = all(x >= 0 for x in w)
                    if hit:
                        out[iz, iy, ix] = True
    return out
