"""numpy restatement of DrawSpheres and DrawRegions (reference lib/visfd/draw.hpp:90-457) and of the filter_mrc handlers
that call them (bin/filter_mrc/handlers.cpp:712-780, settings.cpp:2306-2577, filter_mrc.cpp:220-336): the yardstick of the
GPU tests, itself checked bit for bit against outputs of the real reference program (golden/draw.npz).

Every shape is drawn in list order, vectorised over its clipped bounding box, with the reference's own conversions:
float -> int truncation of the centres, the int r^2 compared as a float32, float32 products, the double
1.0 / n rounded to float32.  The background statistics are plain serial loops with np.float32 accumulators (AverageArr and
StdDevArr, visfd_utils.hpp:685-790): no pairwise or vectorised sum gives their bits."""
import math

import numpy as np

F = np.float32
MAX_RS = 26754          # 3 Rs^2 < 2^31
RECT, SPHERE = 0, 1


class Refused(ValueError):
    """An input the library refuses with VISFD_HIP_EINVAL (the reference has undefined behaviour there)."""


def average_stddev(h, w=None):
    """(AverageArr, StdDevArr): float32 accumulators in raster order, w as weights."""
    hs = [F(x) for x in h.ravel()]
    ws = [F(x) for x in w.ravel()] if w is not None else None
    one = F(1.0)

    def wsum(vals):
        total, denom = F(0.0), F(0.0)
        for k, v in enumerate(vals):
            if ws is not None:
                v = F(v * ws[k])
                denom = F(denom + ws[k])
            else:
                denom = F(denom + one)
            total = F(total + v)
        return total, denom

    with np.errstate(all="ignore"):
        total, denom = wsum(hs)
        ave = F(total / denom)
        dev = []
        for v in hs:
            d = F(v - ave)
            dev.append(F(d * d))
        total, denom = wsum(dev)
        return ave, F(np.sqrt(F(total / denom)))


def sphere_geometry(d, th):
    """(Rs, rmin2, rmax2) of draw.hpp:375-381 for float32 d and th."""
    d, th = F(d), F(th)
    if not np.isfinite(d):
        raise Refused("diameter not finite")
    half = F(d / F(2))
    rs = math.ceil(float(half) - 0.5)
    if rs > MAX_RS:
        raise Refused("diameter too large")
    rs = max(rs, 0)
    rmax2 = F(half * half)
    rmin2 = F(0.0)
    with np.errstate(all="ignore"):
        inner = F(half - th)
    if th > 0 and inner > 0:
        rmin2 = F(inner * inner)
    return rs, rmin2, rmax2


def _clip(c, r, n):
    return max(c - r, 0), min(c + r, n - 1)


def draw_spheres(background, centers, diameters=None, shell_thicknesses=None, foreground=None, mask=None,
                 background_offset=0.0, background_rescale=1.0, background_normalize=False, foreground_normalize=False):
    """-> (image, any_center_outside).  background (nz, ny, nx) float32; centers (n, 3) as x, y, z."""
    if background is None:
        raise Refused("null background")
    bg = np.asarray(background, F)
    nz, ny, nx = bg.shape
    c = np.asarray(centers, F).reshape(-1, 3)
    n = c.shape[0]
    d = np.zeros(n, F) if diameters is None else np.asarray(diameters, F)
    th = (d / F(2)).astype(F) if shell_thicknesses is None else np.asarray(shell_thicknesses, F)
    fg = np.ones(n, F) if foreground is None else np.asarray(foreground, F)
    if not (np.isfinite(c).all() and (c >= F(-2147483648.0)).all() and (c < F(2147483648.0)).all()):
        raise Refused("centre not finite or not an int")
    geo = [sphere_geometry(d[i], th[i]) for i in range(n)]
    rescale, offset = F(background_rescale), F(background_offset)

    with np.errstate(all="ignore"):
        if not background_normalize:
            out = (bg * rescale).astype(F)
        else:
            ave, stddev = average_stddev(bg, mask)
            rms = 0.0
            for f in fg:                      # the square in float32, the sum in double (draw.hpp:306-309)
                rms += float(F(f * f))
            if n > 0:                         # draw.hpp:308-310: the rms of an empty list stays 0
                rms = math.sqrt(rms / n)
            if stddev > 0:
                q = ((bg - ave) / stddev).astype(F)
                out = (q.astype(np.float64) * rms * float(rescale)).astype(F)
            else:
                out = np.zeros_like(bg)
        out = (out + offset).astype(F)

    unmasked = np.ones(bg.shape, bool) if mask is None else (np.asarray(mask) != 0)
    outside = False
    for i in range(n):
        ix, iy, iz = (int(v) for v in c[i])          # truncation toward zero (draw.hpp:365-367)
        outside = outside or not (0 <= ix < nx and 0 <= iy < ny and 0 <= iz < nz)
        rs, rmin2, rmax2 = geo[i]
        (x0, x1), (y0, y1), (z0, z1) = _clip(ix, rs, nx), _clip(iy, rs, ny), _clip(iz, rs, nz)
        if x0 > x1 or y0 > y1 or z0 > z1:
            continue
        jz = (np.arange(z0, z1 + 1, dtype=np.int64) - iz)[:, None, None]
        jy = (np.arange(y0, y1 + 1, dtype=np.int64) - iy)[None, :, None]
        jx = (np.arange(x0, x1 + 1, dtype=np.int64) - ix)[None, None, :]
        r2 = (jx * jx + jy * jy + jz * jz).astype(np.int32).astype(F)    # the int rsqr, compared as a float
        shell = (rmin2 <= r2) & (r2 <= rmax2) & unmasked[z0:z1 + 1, y0:y1 + 1, x0:x1 + 1]
        mult = F(1.0)
        if foreground_normalize:
            cnt = int(shell.sum())
            if cnt > 0:
                mult = F(1.0 / cnt)
        with np.errstate(all="ignore"):
            out[z0:z1 + 1, y0:y1 + 1, x0:x1 + 1][shell] = F(fg[i] * mult)
    return out, outside


def _put(dst, sel, unmasked, value, subtract):
    sel = sel & unmasked
    if value < 0:                       # NaN is not negative: it is written (draw.hpp:165-173)
        if subtract:
            dst[sel & (dst > 0)] = F(0.0)
    else:
        dst[sel] = F(value)


def _rect_axis(fmin, fmax, n):
    """int range of draw.hpp:190-198 with the bounds held in float32; None: empty."""
    lo = F(math.floor(float(F(fmin)) + 0.5)) if np.isfinite(fmin) else F(fmin)
    hi = F(math.floor(float(F(fmax)) + 0.5)) if np.isfinite(fmax) else F(fmax)
    lo = lo if not (lo < F(0)) else F(0)            # std::max<float>(lo, 0)
    hi = F(n - 1) if (F(n - 1) < hi) else hi        # std::min<float>(hi, n - 1)
    if not (lo <= hi):
        return None
    return int(lo), min(int(hi), n - 1)


def draw_regions(image, regions, mask=None, negative_means_subtract=False):
    """regions: [(RECT, (xmin, xmax, ymin, ymax, zmin, zmax), value) | (SPHERE, (x0, y0, z0, r), value)] -> new image."""
    dst = np.array(image, F, copy=True)
    nz, ny, nx = dst.shape
    unmasked = np.ones(dst.shape, bool) if mask is None else (np.asarray(mask) != 0)
    for t, c, v in regions:
        if t == SPHERE:
            cc = [F(x) for x in c[:4]]
            if not np.isfinite(cc).all() or math.ceil(float(cc[3]) - 0.5) > 32767 or \
                    any(abs(math.floor(float(x) + 0.5)) >= 2 ** 31 for x in cc[:3]):
                raise Refused("sphere region")
        elif t != RECT:
            raise Refused("region type")
    if negative_means_subtract and len(regions) > 0 and F(regions[0][2]) < 0:
        if not (dst[unmasked] != 0).any():
            dst[unmasked] = F(1.0)
    for t, c, v in regions:
        v = F(v)
        if t == RECT:
            ax = [_rect_axis(F(c[2 * k]), F(c[2 * k + 1]), (nx, ny, nz)[k]) for k in range(3)]
            if any(a is None or a[0] > a[1] for a in ax):
                continue
            sel = np.zeros(dst.shape, bool)
            sel[ax[2][0]:ax[2][1] + 1, ax[1][0]:ax[1][1] + 1, ax[0][0]:ax[0][1] + 1] = True
            _put(dst, sel, unmasked, v, negative_means_subtract)
        else:
            R = F(c[3])
            Ri = math.ceil(float(R) - 0.5)
            ix, iy, iz = (math.floor(float(F(x)) + 0.5) for x in c[:3])
            (x0, x1), (y0, y1), (z0, z1) = _clip(ix, Ri, nx), _clip(iy, Ri, ny), _clip(iz, Ri, nz)
            if x0 > x1 or y0 > y1 or z0 > z1:
                continue
            jz = (np.arange(z0, z1 + 1, dtype=np.int64) - iz)[:, None, None]
            jy = (np.arange(y0, y1 + 1, dtype=np.int64) - iy)[None, :, None]
            jx = (np.arange(x0, x1 + 1, dtype=np.int64) - ix)[None, None, :]
            with np.errstate(all="ignore"):
                descr = (F(R * R) - (jy * jy + jz * jz).astype(np.int32).astype(F)).astype(F)   # draw.hpp:148
                xrange = np.floor(np.sqrt(descr))                                               # float32 sqrt, :151
            inside = (descr >= 0) & (np.abs(jx) <= np.where(descr >= 0, xrange, -1))
            sel = np.zeros(dst.shape, bool)
            sel[z0:z1 + 1, y0:y1 + 1, x0:x1 + 1] = inside
            _put(dst, sel, unmasked, v, negative_means_subtract)
    return dst


# ---- the filter_mrc handlers around the two functions ---------------------------------------------------------------------
DEFAULTS = dict(diameter=-1.0, diameter_in_voxels=False, scale=1.0, thickness=1.0, thickness_is_ratio=True, thickness_min=1.0,
                use_score=True, foreground=1.0, background=0.0, background_scale=1.0, background_norm=False,
                foreground_norm=False)


def shell_thickness(opts, diameter):
    """handlers.cpp:751-758 (and :957-964): below the minimum a ratio's thickness becomes 1.0, not the minimum."""
    th = F(opts["thickness"])
    if opts["thickness_is_ratio"]:
        th = F(th * F(diameter))
        if th < F(opts["thickness_min"]):
            th = F(1.0)
    return th


def read_blob_rows(rows, w, opts):
    """ReadBlobCoordsFile and the unit conversions of HandleBlobsNonmaxSuppression (file_io.hpp:413-493,
    handlers.cpp:443-508) for rows of 3 to 5 numbers in physical units -> (crds, diameters, scores) in voxels."""
    w = F(w)
    crds, dia, sc = [], [], []
    for r in rows:
        r = [F(x) for x in r]
        d = r[3] if len(r) > 3 else F(-1.0)
        if d < 0:
            d = F(-1.0)
        d = F(d * F(opts["scale"]))
        c = [F(math.floor(float(F(x / w)) + 0.5)) for x in r[:3]]
        if d != F(-1.0):
            d = F(d / w)
        if opts["diameter"] >= 0:
            d = F(opts["diameter"])
            if not opts["diameter_in_voxels"]:
                d = F(d / w)
        crds.append(c)
        dia.append(d)
        sc.append(r[4] if len(r) > 4 else F(opts["foreground"]))
    return np.array(crds, F).reshape(-1, 3), np.array(dia, F), np.array(sc, F)


def handle_draw_spheres(image, mask, rows, w, **options):
    """HandleDrawSpheres (handlers.cpp:712-780) and the masking that ends every run (filter_mrc.cpp:765-776)."""
    opts = dict(DEFAULTS, **options)
    if not opts["thickness_is_ratio"]:
        opts["thickness"] = F(F(opts["thickness"]) / F(w))          # filter_mrc.cpp:333-334
    crds, dia, sc = read_blob_rows(rows, w, opts)
    if not opts["use_score"]:
        sc = np.full(len(sc), opts["foreground"], F)
    th = np.array([shell_thickness(opts, d) for d in dia], F)
    out, _ = draw_spheres(image, crds[::-1], dia[::-1], th[::-1], sc[::-1], mask, opts["background"],
                          opts["background_scale"], opts["background_norm"], opts["foreground_norm"])
    if mask is not None:
        out[np.asarray(mask) == 0] = F(0.0)
    return out


def handle_blob_display(image, mask, minima, maxima, w, **options):
    """The picture that ends HandleBlobDetector (handlers.cpp:933-978).  minima, maxima: (voxel crds in detection order,
    physical diameters, scores -- the last two sorted as their list file is, or in detection order where none is written)."""
    opts = dict(DEFAULTS, **options)
    w = F(w)
    crds = np.concatenate([np.asarray(minima[0], F).reshape(-1, 3), np.asarray(maxima[0], F).reshape(-1, 3)[::-1]])
    dia = np.concatenate([np.asarray(minima[1], F), np.asarray(maxima[1], F)[::-1]])
    sc = np.concatenate([np.asarray(minima[2], F), np.asarray(maxima[2], F)[::-1]])
    dia = (dia / w).astype(F)
    th = np.full(len(dia), opts["thickness"], F)
    if opts["thickness_is_ratio"]:
        th = (th * dia).astype(F)
    dia = (dia * F(opts["scale"])).astype(F)
    th[th < F(opts["thickness_min"])] = F(1.0)
    out, _ = draw_spheres(image, crds, dia, th, sc, mask, opts["background"], opts["background_scale"],
                          opts["background_norm"], False)
    if mask is not None:
        out[np.asarray(mask) == 0] = F(0.0)
    return out


def handle_mask_regions(shape, regions, mask=None):
    """filter_mrc.cpp:220-286 without binning: the mask starts as zeros (or as the file's), then DrawRegions(..., true)."""
    m = np.zeros(shape, F) if mask is None else mask
    return draw_regions(m, regions, None, True)
