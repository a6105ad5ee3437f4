"""numpy restatement of the reference's general 3-D filter, the yardstick of tests/test_filter3d*.py:

  the table makers GenFilterGenGauss3D (lib/visfd/filter3d.hpp:546-638) and GenFilterDogg3D
  (bin/filter_mrc/filter3d_variants.hpp:270-482) in float32 with the reference's type rules, and
  Filter3D::Apply (filter3d.hpp:81-198, :403-458) as one float32 array operation per tap, in tap order, every skip done
  with np.where -- exact by construction.

exp and pow go through the C library's float functions (what std::exp / std::pow of floats call); numpy's own float32
exp is a vector routine with different last bits."""
import ctypes
import ctypes.util
import math

import numpy as np

F = np.float32

_libm = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6")
for _name in ("expf", "powf", "logf"):
    getattr(_libm, _name).restype = ctypes.c_float
    getattr(_libm, _name).argtypes = [ctypes.c_float] * (2 if _name == "powf" else 1)


def expf(x):
    return F(_libm.expf(float(x)))


def powf(x, y):
    return F(_libm.powf(float(x), float(y)))


def logf(x):
    return F(_libm.logf(float(x)))


def halfwidths(width, m_exp, ratio=-1.0, threshold=0.03):
    """floor(width_d * ratio) in float; a negative ratio is first replaced by pow(-log(threshold), 1.0 / m): float log,
    double pow, stored to float (filter3d_variants.hpp:99-103, filter3d.hpp:631-633)."""
    ratio = F(ratio)
    if ratio < 0:
        ratio = F(math.pow(float(-logf(F(threshold))), 1.0 / float(F(m_exp))))
    return tuple(int(math.floor(F(F(w) * ratio))) for w in width)


def gengauss3d_table(width, m_exp, hw):
    """-> (table float32 [jz][jy][jx], A)"""
    width = [F(w) for w in width]
    m = F(m_exp)
    cut = F(1.0)
    for d in range(3):
        if width[d] > 0:
            e = expf(-powf(F(hw[d]) / width[d], m))
            if e < cut:
                cut = e
    t = np.zeros((2 * hw[2] + 1, 2 * hw[1] + 1, 2 * hw[0] + 1), F)
    total = F(0.0)
    with np.errstate(divide="ignore", invalid="ignore"):
        for iz in range(-hw[2], hw[2] + 1):
            z = F(0.0) if (width[2] == 0 and iz == 0) else F(iz) / width[2]
            for iy in range(-hw[1], hw[1] + 1):
                y = F(0.0) if (width[1] == 0 and iy == 0) else F(iy) / width[1]
                for ix in range(-hw[0], hw[0] + 1):
                    x = F(0.0) if (width[0] == 0 and ix == 0) else F(ix) / width[0]
                    r = np.sqrt(F(F(F(x * x) + F(y * y)) + F(z * z)))
                    v = expf(-powf(r, m)) if r > 0 else F(1.0)
                    if abs(v) < cut:
                        v = F(0.0)
                    t[iz + hw[2], iy + hw[1], ix + hw[0]] = v
                    total = F(total + v)
    t = (t / total).astype(F)
    return t, t[hw[2], hw[1], hw[0]]


def dogg3d_table(width_a, width_b, m_exp, n_exp, ratio=-1.0, threshold=0.03):
    """-> (table, (hx, hy, hz), A, B): each Gaussian in its own window, entries 0 + A_entry - B_entry."""
    ha = halfwidths(width_a, m_exp, ratio, threshold)
    hb = halfwidths(width_b, n_exp, ratio, threshold)
    fa, A = gengauss3d_table(width_a, m_exp, ha)
    fb, B = gengauss3d_table(width_b, n_exp, hb)
    hw = tuple(max(a, b) for a, b in zip(ha, hb))
    t = np.zeros((2 * hw[2] + 1, 2 * hw[1] + 1, 2 * hw[0] + 1), F)

    def window(h):
        return tuple(slice(hw[d] - h[d], hw[d] + h[d] + 1) for d in (2, 1, 0))
    t[window(ha)] = (t[window(ha)] + fa).astype(F)
    t[window(hb)] = (t[window(hb)] - fb).astype(F)
    return t, hw, A, B


def apply(src, table, hw=None, mask=None, normalize=False, want_den=False):
    """Filter3D::Apply.  table[jz + hz][jy + hy][jx + hx]; hw = (hx, hy, hz) (default: from the table's shape).  Voxels with
    mask == 0 get dst = 0 and den = 0 (the project's definition where the reference has none)."""
    src = np.asarray(src, F)
    table = np.asarray(table, F)
    if hw is None:
        hw = ((table.shape[2] - 1) // 2, (table.shape[1] - 1) // 2, (table.shape[0] - 1) // 2)
    hx, hy, hz = hw
    nz, ny, nx = src.shape
    pad = ((hz, hz), (hy, hy), (hx, hx))
    ps = np.pad(src, pad)
    pm = np.pad(np.ones_like(src) if mask is None else np.asarray(mask, F), pad)   # 0 outside the image
    valid = pm != 0
    g = np.zeros(src.shape, F)
    den = np.zeros(src.shape, F)
    with np.errstate(all="ignore"):
        for jz in range(-hz, hz + 1):
            for jy in range(-hy, hy + 1):
                for jx in range(-hx, hx + 1):
                    sl = (slice(hz - jz, hz - jz + nz), slice(hy - jy, hy - jy + ny), slice(hx - jx, hx - jx + nx))
                    h = table[jz + hz, jy + hy, jx + hx]
                    fv = np.full(src.shape, h, F) if mask is None else (h * pm[sl]).astype(F)
                    dg = (fv * ps[sl]).astype(F)
                    ok = valid[sl]
                    g = np.where(ok, (g + dg).astype(F), g)
                    den = np.where(ok, (den + fv).astype(F), den)
        if mask is not None:
            off = np.asarray(mask, F) == 0
            g[off] = 0
            den[off] = 0
        out = g
        if normalize:
            out = np.where(den > 0, (g / np.where(den > 0, den, F(1))).astype(F), g)
    return (out, den) if want_den else out


def local_fluctuations(src, sigma, exponent, ratio, mask=None, normalize=True):
    """LocalFluctuations with the dense window (filter3d.hpp:1713-1847; exponent != 2)."""
    src = np.asarray(src, F)
    hw = halfwidths(sigma, exponent, ratio)
    w, wpeak = gengauss3d_table(sigma, exponent, hw)
    w = (w * F(1.0 / float(wpeak))).astype(F)
    avg = apply(src, w, hw, mask, normalize)
    p = (src - avg).astype(F)
    p = (p * p).astype(F)
    var = (apply(p, w, hw, mask, normalize) * wpeak).astype(F)
    var = np.where(var < 0, F(0), var)
    return np.sqrt(var).astype(F)
