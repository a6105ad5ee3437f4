"""close_surface as include/visfd_hip.h and DESIGN.md 4.17 define it, in numpy: the splat in Python integers, the right-hand
side in float32 in the stated order, the Poisson solve in float64 by the sine transform (exact up to rounding: the yardstick
of the device's float32 multigrid), the level and the mask; and the checkers the tests share.  Arrays are [z, y, x]."""
import numpy as np

SCALE = 2.0 ** 24
NORMAL_MAX = 2.0 ** 30


def used_mask(points, normals, shape, pad):
    """which points are used: six finite floats, |n_d| <= 2^30, and the cell floor(p) .. floor(p) + 1 inside the padded box"""
    nz, ny, nx = shape
    p = np.asarray(points, np.float32).astype(np.float64).reshape(-1, 3)
    n = np.asarray(normals, np.float32).astype(np.float64).reshape(-1, 3)
    ok = np.isfinite(p).all(1) & np.isfinite(n).all(1)
    ok &= (np.abs(np.where(np.isfinite(n), n, 0.0)) <= NORMAL_MAX).all(1)
    with np.errstate(invalid="ignore"):
        fl = np.floor(np.where(np.isfinite(p), p, 0.0))
    for d, size in enumerate((nx, ny, nz)):
        ok &= (fl[:, d] >= -pad) & (fl[:, d] + 1 <= size - 1 + pad)
    return ok


def splat_int(points, normals, shape, pad, drop=None):
    """-> acc: a [3][Nz][Ny][Nx] nested array of Python integers as an object ndarray, n_used, n_skipped.
    drop = k: the k-th contribution is left out (a mutant for the tests)."""
    nz, ny, nx = shape
    N = (nz + 2 * pad, ny + 2 * pad, nx + 2 * pad)
    acc = np.zeros((3,) + N, object)
    acc[...] = 0
    ok = used_mask(points, normals, shape, pad)
    P = np.asarray(points, np.float32).reshape(-1, 3)
    Nn = np.asarray(normals, np.float32).reshape(-1, 3)
    count = 0
    for i in np.nonzero(ok)[0]:
        p = [float(v) for v in P[i]]
        n = [float(v) for v in Nn[i]]
        base = [int(np.floor(v)) for v in p]
        f = [v - np.floor(v) for v in p]
        for cz in (0, 1):
            wz = f[2] if cz else 1.0 - f[2]
            for cy in (0, 1):
                wy = f[1] if cy else 1.0 - f[1]
                for cx in (0, 1):
                    wx = f[0] if cx else 1.0 - f[0]
                    w = (wx * wy) * wz
                    for d in range(3):
                        if drop is not None and count == drop:
                            count += 1
                            continue
                        count += 1
                        acc[d, base[2] + cz + pad, base[1] + cy + pad, base[0] + cx + pad] += int(round((w * n[d]) * SCALE))
    return acc, int(ok.sum()), int((~ok).sum())


def acc_to_int64(acc):
    return np.array(acc, np.int64)


def field_from_acc(acc):
    """V_d = (float)((double)acc_d * 2^-24)"""
    return (np.array(acc, np.int64).astype(np.float64) * (1.0 / SCALE)).astype(np.float32)


def rhs(V):
    """b in float32, in the stated order; V = 0 outside the box"""
    Vp = np.pad(V, ((0, 0), (1, 1), (1, 1), (1, 1)))
    h = np.float32(0.5)
    dx = h * (Vp[0, 1:-1, 1:-1, 2:] - Vp[0, 1:-1, 1:-1, :-2])
    dy = h * (Vp[1, 1:-1, 2:, 1:-1] - Vp[1, 1:-1, :-2, 1:-1])
    dz = h * (Vp[2, 2:, 1:-1, 1:-1] - Vp[2, :-2, 1:-1, 1:-1])
    out = (dx + dy) + dz
    assert out.dtype == np.float32
    return out


def _sine(n):
    k = np.arange(1, n + 1, dtype=np.float64)
    S = np.sin(np.pi * np.outer(k, k) / (n + 1)) * np.sqrt(2.0 / (n + 1))
    lam = 2.0 * np.cos(np.pi * k / (n + 1)) - 2.0
    return S, lam


def laplacian(u):
    up = np.pad(u, 1)
    return (up[2:, 1:-1, 1:-1] + up[:-2, 1:-1, 1:-1] + up[1:-1, 2:, 1:-1] + up[1:-1, :-2, 1:-1] + up[1:-1, 1:-1, 2:] +
            up[1:-1, 1:-1, :-2]) - 6.0 * u


def solve64(b):
    """chi with laplacian(chi) = b, chi = 0 outside the box, in float64"""
    b = np.asarray(b, np.float64)
    Sz, lz = _sine(b.shape[0])
    Sy, ly = _sine(b.shape[1])
    Sx, lx = _sine(b.shape[2])
    t = np.einsum("az,zyx->ayx", Sz, b)
    t = np.einsum("by,ayx->abx", Sy, t)
    t = np.einsum("cx,abx->abc", Sx, t)
    t /= lz[:, None, None] + ly[None, :, None] + lx[None, None, :]
    t = np.einsum("az,abc->zbc", Sz, t)
    t = np.einsum("by,zbc->zyc", Sy, t)
    return np.einsum("cx,zyc->zyx", Sx, t)


def residual_ratio(chi, b):
    b = np.asarray(b, np.float64)
    nb = np.sqrt((b * b).sum())
    r = b - laplacian(np.asarray(chi, np.float64))
    return float(np.sqrt((r * r).sum()) / nb) if nb > 0 else 0.0


def sample(chi, points, normals, shape, pad):
    """the mean over the used points of chi interpolated trilinearly (double): the level"""
    ok = used_mask(points, normals, shape, pad)
    if not ok.any():
        return 0.0
    p = np.asarray(points, np.float32).reshape(-1, 3)[ok].astype(np.float64)
    fl = np.floor(p)
    f = p - fl
    i = fl.astype(np.int64) + pad
    c = np.asarray(chi, np.float64)
    tot = np.zeros(len(p))
    for cz in (0, 1):
        wz = f[:, 2] if cz else 1.0 - f[:, 2]
        for cy in (0, 1):
            wy = f[:, 1] if cy else 1.0 - f[:, 1]
            for cx in (0, 1):
                wx = f[:, 0] if cx else 1.0 - f[:, 0]
                tot += ((wx * wy) * wz) * c[i[:, 2] + cz, i[:, 1] + cy, i[:, 0] + cx]
    return float(tot.sum() / len(p))


def face_counts(chi, iso):
    """nodes on the six faces of the padded box with chi < iso, and with chi > iso"""
    f = np.zeros(chi.shape, bool)
    f[0], f[-1], f[:, 0], f[:, -1], f[:, :, 0], f[:, :, -1] = True, True, True, True, True, True
    c = np.asarray(chi, np.float64)
    return int((f & (c < iso)).sum()), int((f & (c > iso)).sum())


def cut(chi, iso, pad, orientation):
    """-> mask float32 over the image, the orientation taken"""
    if orientation == "auto":
        lo, hi = face_counts(chi, iso)
        orientation = "outward" if lo <= hi else "inward"
    c = np.asarray(chi, np.float64)
    if pad:
        c = c[pad:-pad, pad:-pad, pad:-pad]
    m = (c < iso) if orientation == "outward" else (c > iso)
    return m.astype(np.float32), orientation


class Result(object):
    pass


def close_surface(points, normals, shape, pad=0, orientation="outward"):
    r = Result()
    r.pad = pad
    acc, r.n_used, r.n_skipped = splat_int(points, normals, shape, pad)
    r.acc = acc_to_int64(acc)
    r.b = rhs(field_from_acc(acc))
    if r.n_used == 0:
        r.chi = np.zeros(r.b.shape)
        r.iso = 0.0
        r.mask, r.orientation = np.zeros(shape, np.float32), orientation
        r.range = 0.0
        return r
    r.chi = solve64(r.b)
    r.iso = sample(r.chi, points, normals, shape, pad)
    r.mask, r.orientation = cut(r.chi, r.iso, pad, orientation)
    r.range = float(r.chi.max() - r.chi.min())
    return r


_REFERENCE = {}


def reference(case):
    """close_surface of a case of close_surface_cases, computed once per process and shared read-only"""
    if case.name not in _REFERENCE:
        r = close_surface(case.points, case.normals, case.shape, case.pad, case.orientation)
        for a in (r.acc, r.b, r.chi, r.mask):
            a.setflags(write=False)
        _REFERENCE[case.name] = r
    return _REFERENCE[case.name]


def image_of(chi, pad):
    return chi[pad:-pad, pad:-pad, pad:-pad] if pad else chi


# ---- the checkers --------------------------------------------------------------------------------------------------------

def touches_face(mask):
    m = np.asarray(mask) != 0
    return bool(m[0].any() or m[-1].any() or m[:, 0].any() or m[:, -1].any() or m[:, :, 0].any() or m[:, :, -1].any())


def n_solids(mask):
    """the number of 6-connected components of the mask"""
    todo = np.asarray(mask) != 0
    n = 0
    while todo.any():
        n += 1
        seed = np.zeros_like(todo)
        seed[tuple(np.argwhere(todo)[0])] = True
        while True:
            g = seed.copy()
            g[1:] |= seed[:-1]
            g[:-1] |= seed[1:]
            g[:, 1:] |= seed[:, :-1]
            g[:, :-1] |= seed[:, 1:]
            g[:, :, 1:] |= seed[:, :, :-1]
            g[:, :, :-1] |= seed[:, :, 1:]
            g &= todo
            if (g == seed).all():
                break
            seed = g
        todo &= ~seed
    return n


def ball(shape, center, radius):
    """-> the exact ball's voxels, and each voxel's distance from the centre"""
    z, y, x = np.meshgrid(*[np.arange(s, dtype=np.float64) for s in shape], indexing="ij")
    d = np.sqrt((x - center[0]) ** 2 + (y - center[1]) ** 2 + (z - center[2]) ** 2)
    return d < radius, d


def geometry(mask, case):
    """-> dict: touches, solids, worst (the largest | |v - c| - r | over the voxels of the sampled latitudes where mask and
    ball differ; 0 when none does), fraction (mask voxels / ball voxels)"""
    m = np.asarray(mask) != 0
    b, d = ball(m.shape, case.center, case.radius)
    z = np.arange(m.shape[0], dtype=np.float64)[:, None, None]
    lat = np.abs(z - case.center[2]) <= case.cap * case.radius
    diff = (m != b) & lat
    return {"touches": touches_face(m), "solids": n_solids(m),
            "worst": float(np.abs(d[diff] - case.radius).max()) if diff.any() else 0.0,
            "fraction": float(m.sum()) / float(b.sum())}


def check_geometry(mask, case):
    """the geometric conditions of DESIGN.md 4.17; raises AssertionError with the figures"""
    g = geometry(mask, case)
    assert not g["touches"], (case.name, "the mask touches a face", g)
    assert g["solids"] == 1, (case.name, "the mask is not one solid", g)
    assert g["worst"] <= 0.5, (case.name, "mask and ball differ away from the sphere", g)
    assert 0.85 <= g["fraction"] <= 1.01, (case.name, "volume", g)
    return g


def band(chi64, iso64, rng, width=1e-3):
    """the voxels where |chi - iso| <= width * range"""
    return np.abs(np.asarray(chi64, np.float64) - iso64) <= width * rng


def check_mask_against(mask, ref, what=""):
    """the device mask may differ from the restatement's only inside the band, and the band holds at most 1 % of the
    restatement's mask; -> (differing voxels, band voxels, mask voxels)"""
    chi = image_of(ref.chi, ref.pad)
    bd = band(chi, ref.iso, ref.range)
    diff = np.asarray(mask) != ref.mask
    nm = int((ref.mask != 0).sum())
    assert not (diff & ~bd).any(), "%s: %d voxels differ outside the band" % (what, int((diff & ~bd).sum()))
    assert int(bd.sum()) <= 0.01 * nm, "%s: the band holds %d voxels, the mask %d" % (what, int(bd.sum()), nm)
    return int(diff.sum()), int(bd.sum()), nm
