"""A from-scratch numpy restatement of the reference's grayscale morphology (lib/visfd/morphology.hpp:134-597): the
sphere structuring element and Dilate / Erode with an arbitrary element, for the morphology tests."""
import numpy as np

f32 = np.float32


def sphere_structure(radius, radius_max=0.0, bmax=0.0):
    """(dxyz (n, 3) int32, b (n,) float32) of DilateSphere / ErodeSphere: dz outermost, then dy, then dx; integer squares,
    double sqrt stored to float, float compares and float b arithmetic."""
    radius, radius_max, bmax = f32(radius), f32(radius_max), f32(bmax)
    Ri = int(np.ceil(max(radius, radius_max)))
    d, bs = [], []
    corners = [(jx - 0.5, jy - 0.5, jz - 0.5) for jz in (0, 1) for jy in (0, 1) for jx in (0, 1)]
    with np.errstate(all="ignore"):
        for iz in range(-Ri, Ri + 1):
            for iy in range(-Ri, Ri + 1):
                for ix in range(-Ri, Ri + 1):
                    add, b = False, f32(0.0)
                    r = f32(np.sqrt(np.float64(ix * ix + iy * iy + iz * iz)))
                    if bmax == 0:
                        add = r <= radius
                    elif radius_max > radius:
                        if r <= radius:
                            add = True
                        elif r <= radius_max:
                            add = True
                            b = f32(-(r - radius)) / f32(radius_max - radius)
                            b = f32(b * bmax)
                    else:
                        rs = [f32(np.sqrt((ix + cx) ** 2 + (iy + cy) ** 2 + (iz + cz) ** 2)) for cx, cy, cz in corners]
                        r_min, r_max = min(rs), max(rs)
                        if r_max < radius:
                            add = True
                        elif r_min > radius:
                            add = False
                        else:
                            add = True
                            b = f32(-(r_max - radius)) / f32(r_max - r_min)
                            b = f32(b * bmax)
                    if add:
                        d.append((ix, iy, iz))
                        bs.append(f32(b))
    return np.array(d, np.int32).reshape(-1, 3), np.array(bs, np.float32)


def _shifted(a, dx, dy, dz, fill):
    """out[z, y, x] = a[z + dz, y + dy, x + dx] where that lies inside, else fill."""
    nz, ny, nx = a.shape
    out = np.full(a.shape, fill, a.dtype)
    zs, ys, xs = [(max(0, -d), min(n, n - d)) for d, n in ((dz, nz), (dy, ny), (dx, nx))]
    if zs[0] < zs[1] and ys[0] < ys[1] and xs[0] < xs[1]:
        out[zs[0]:zs[1], ys[0]:ys[1], xs[0]:xs[1]] = a[zs[0] + dz:zs[1] + dz, ys[0] + dy:ys[1] + dy, xs[0] + dx:xs[1] + dx]
    return out


def dilate_erode(src, dxyz, b, dilate, mask=None, dst=None):
    """Dilate / Erode (morphology.hpp:134-229): the element walked in order, skipped neighbours (outside, mask == 0), the
    running value kept with std::max / std::min (cur = where(cur < c, c, cur)); voxels with mask == 0 keep dst."""
    src = np.asarray(src, np.float32)
    valid_src = np.ones(src.shape, bool) if mask is None else (mask != 0)
    cur = np.full(src.shape, -np.inf if dilate else np.inf, np.float32)
    with np.errstate(all="ignore"):
        for (dx, dy, dz), bb in zip(dxyz.tolist(), b):
            f = _shifted(src, dx, dy, dz, 0.0)
            ok = _shifted(valid_src, dx, dy, dz, False)
            c = (f + bb) if dilate else (f - bb)
            take = ok & ((cur < c) if dilate else (c < cur))
            cur = np.where(take, c, cur).astype(np.float32)
    out = np.array(src if dst is None else dst, np.float32, copy=True)
    write = valid_src if mask is not None else np.ones(src.shape, bool)
    out[write] = cur[write]
    return out


def sphere_op(op, src, radius, radius_max=0.0, bmax=0.0, mask=None, dst=None):
    """op 0..5: dilate, erode, open, close, white top-hat (dst - open(src)), black top-hat (close(src) - dst); masked
    voxels of dst untouched."""
    d, b = sphere_structure(radius, radius_max, bmax)
    dst = np.array(src if dst is None else dst, np.float32, copy=True)
    if op in (0, 1):
        return dilate_erode(src, d, b, op == 0, mask, dst)
    first_dilate = op in (3, 5)
    tmp = dilate_erode(src, d, b, first_dilate, mask)
    res = dilate_erode(tmp, d, b, not first_dilate, mask)
    write = np.ones(src.shape, bool) if mask is None else (mask != 0)
    with np.errstate(all="ignore"):
        if op in (2, 3):
            dst[write] = res[write]
        elif op == 4:
            dst[write] = (dst - res)[write]
        else:
            dst[write] = (res - dst)[write]
    return dst
