"""A numpy restatement of filter_mrc's tail (include/visfd_hip.h, section m1c): the scalar maps with Number = float, one
float32 operation per step, and the whole tail of a command line in the reference's order (invert, one map, mask fill,
-rescale-min-max) with its serial sums."""
import numpy as np

f32 = np.float32
f64 = np.float64
MAP_NONE, MAP_STEP, MAP_THRESH2, MAP_THRESH4, MAP_RANGE, MAP_GAUSS, MAP_RESCALE = range(7)


def _a(x):
    return np.asarray(x, f32)


def is_between(x, a, b):
    return ((a <= x) & (x < b)) | ((b < x) & (x <= a))


def ramp(I, a, b):
    I, a, b = _a(I), f32(a), f32(b)
    with np.errstate(all="ignore"):
        inside = (I - a) / (b - a)
        beyond = np.where((I - a) * (b - a) > 0, f32(1), f32(0))
    return np.where(is_between(I, a, b), inside, beyond).astype(f32)


def stretch(g, out_a, out_b):
    out_a, out_b = f32(out_a), f32(out_b)
    with np.errstate(all="ignore"):
        return (out_a + _a(g) * (out_b - out_a)).astype(f32)


def step(I, t, out_a, out_b):
    return np.where(_a(I) > f32(t), f32(out_b), f32(out_a)).astype(f32)


def threshold2(I, a, b, out_a=0.0, out_b=1.0):
    return stretch(ramp(I, a, b), out_a, out_b)


def threshold4(I, a, b, c, d, out_a=0.0, out_b=1.0):
    I = _a(I)
    a, b, c, d = f32(a), f32(b), f32(c), f32(d)
    g0 = threshold2(I, a, b)
    if b == c and b == d:
        return g0
    one, zero = np.ones_like(I), np.zeros_like(I)
    if b <= c:
        rest = np.where(is_between(I, b, c), one, zero)
    elif d <= a:
        rest = np.where(is_between(I, d, a), zero, one)
    else:
        rest = g0
    g = np.where(is_between(I, a, b), threshold2(I, a, b), np.where(is_between(I, c, d), threshold2(I, c, d), rest))
    return stretch(g.astype(f32), out_a, out_b)


def select_range(I, a, b):
    I, a, b = _a(I), f32(a), f32(b)
    if a < b:
        return np.where(is_between(I, a, b), f32(1), f32(0)).astype(f32)
    return np.where(is_between(I, b, a), f32(0), f32(1)).astype(f32)


def gauss(I, x0, sigma, out_a=0.0, out_b=1.0):
    with np.errstate(all="ignore"):
        xr = ((_a(I) - f32(x0)) / f32(sigma)).astype(f32).astype(f64)
        span = f64(f32(out_b) - f32(out_a))
        return (f64(f32(out_a)) + span * np.exp((-0.5 * xr) * xr)).astype(f32)


def rescale(v, factor, offset):
    with np.errstate(all="ignore"):
        return ((_a(v) * f32(factor)).astype(f32) + f32(offset)).astype(f32)


def invert(v, ave):
    return (2.0 * f64(ave) - _a(v).astype(f64)).astype(f32)


def rescale01(v, out_a, out_b, dmin, dmax):
    out_a, out_b, dmin, dmax = f32(out_a), f32(out_b), f32(dmin), f32(dmax)
    with np.errstate(all="ignore"):
        num = ((out_b - out_a) * (_a(v) - dmin)).astype(f32)
        return (out_a + (num / (dmax - dmin)).astype(f32)).astype(f32)


def apply(out, src=None, mask=None, map=MAP_NONE, t=(), out_a=0.0, out_b=1.0, invert_ave=None, masked_value=None,
          rescale01_args=None):
    """The stages of one visfd_hip_intensity pass, as api.intensity(...) names them -> the new image."""
    v = _a(out).copy()
    inm = np.ones(v.shape, bool) if mask is None else (mask != 0)
    if invert_ave is not None:
        v = np.where(inm, invert(v, invert_ave), v)
    if map == MAP_STEP:
        v = step(src, t[0], out_a, out_b)
    elif map == MAP_THRESH2:
        v = threshold2(src, t[0], t[1], out_a, out_b)
    elif map == MAP_THRESH4:
        v = threshold4(src, t[0], t[1], t[2], t[3], out_a, out_b)
    elif map == MAP_RANGE:
        v = select_range(src, t[0], t[1])
    elif map == MAP_GAUSS:
        v = gauss(src, t[0], t[1], out_a, out_b)
    elif map == MAP_RESCALE:
        v = rescale(v, t[0], t[1])
    if masked_value is not None:
        v = np.where(inm, v, f32(masked_value))
    if rescale01_args is not None:
        v = rescale01(v, rescale01_args[2], rescale01_args[3], rescale01_args[0], rescale01_args[1])
    return v.astype(f32)


# ---- a whole command line ---------------------------------------------------------------------------------------------
def serial_sum64(x):
    """sum in double, in scan order"""
    x = np.asarray(x, f64).reshape(-1)
    return f64(np.add.accumulate(x)[-1]) if x.size else f64(0.0)


def serial_sum32(x):
    """sum in float, in scan order"""
    x = np.asarray(x, f32).reshape(-1)
    return f32(np.add.accumulate(x, dtype=f32)[-1]) if x.size else f32(0.0)


def parse(flags):
    """The tail's settings from a flag list, as bin/filter_mrc/settings.cpp leaves them (flags of filters are skipped)."""
    s = dict(map=None, a=f32(0), b=f32(0), c=f32(0), d=f32(0), dual=False, clip=False, clip_sigma=False, gauss=False,
             x0=f32(0), sigma=f32(1), mult=None, off=f32(0), out_a=f32(0), out_b=f32(1), invert=False, rmm=None,
             mask_out=f32(0), mask_select=None)
    i = 0
    num = lambda k: f32(float(flags[i + k]))
    while i < len(flags):
        f = flags[i]
        if f in ("-thresh", "-thresh-out"):
            s.update(map="thresh", dual=False, a=num(1), b=num(1)); i += 2
        elif f in ("-thresh2", "-thresh2-out"):
            s.update(map="thresh", dual=False, a=num(1), b=num(2), clip=False); i += 3
        elif f in ("-clip", "-cl"):
            s.update(map="thresh", dual=False, a=num(1), b=num(2), clip=True, clip_sigma=(f == "-cl")); i += 3
        elif f in ("-thresh4", "-thresh4-out"):
            s.update(map="thresh", dual=True, a=num(1), b=num(2), c=num(3), d=num(4)); i += 5
        elif f in ("-thresh-interval", "-thresh-interval-out"):
            s.update(map="thresh", dual=True, a=num(1), b=num(1), c=num(2), d=num(2)); i += 3
        elif f in ("-thresh-gauss", "-thresh-gauss-out"):
            s.update(map="thresh", gauss=True, x0=num(1), sigma=num(2)); i += 3
        elif f in ("-thresh-range", "-thresh-range-out"):
            s.update(out_a=num(1), out_b=num(2)); i += 3
        elif f == "-rescale":
            s.update(map="thresh", mult=num(1), off=num(2)); i += 3
        elif f == "-fill":
            s.update(map="thresh", mult=f32(0), off=num(1)); i += 2
        elif f == "-rescale-min-max":
            s["rmm"] = (num(1), num(2)); i += 3   # the first number is stored as the maximum
        elif f in ("-no-rescale", "-norescale"):
            s.update(rmm=None, a=f32(1), b=f32(1)); i += 1
        elif f in ("-invert", "-inv"):
            s["invert"] = True; i += 1
        elif f == "-mask-out":
            s["mask_out"] = num(1); i += 2
        elif f == "-mask-select":
            s["mask_select"] = int(flags[i + 1]); i += 2
        elif f == "-gauss":
            i += 2
        else:
            raise ValueError(f)
    return s


def cl_thresholds(tomo_in, mask, a, b):
    """-cl: AverageArr and StdDevArr in float, weighted by the mask's values, in scan order (visfd_utils.hpp:685-790)."""
    h = _a(tomo_in).reshape(-1)
    if mask is None:
        w = np.ones_like(h)
    else:
        w = _a(mask).reshape(-1)
    ave = f32(serial_sum32(h * w) / serial_sum32(w))
    dev = (h - ave).astype(f32)
    dev = (dev * dev).astype(f32)
    sd = f32(np.sqrt(f32(serial_sum32((dev * w).astype(f32)) / serial_sum32(w))))
    return f32(ave + f32(a * sd)), f32(ave + f32(b * sd))


def tail(tomo_in, filtered, mask, flags):
    """What the reference writes for `flags` when its filter has left `filtered` in the output image; mask as loaded from the
    file (or None).  -> (image, True when -invert's mean is the serial double sum of values whose order matters)"""
    s = parse(flags)
    if mask is not None and s["mask_select"] is not None:
        mask = np.where(mask == f32(s["mask_select"]), f32(1), f32(0)).astype(f32)
    inm = np.ones(tomo_in.shape, bool) if mask is None else (mask != 0)
    out = _a(filtered).copy()
    if s["invert"]:
        ave = serial_sum64(out[inm]) / f64(int(inm.sum()))
        out = np.where(inm, invert(out, ave), out)
    if s["map"]:
        if s["mult"] is not None:
            out = rescale(out, s["mult"], s["off"])
        elif s["gauss"]:
            out = gauss(tomo_in, s["x0"], s["sigma"], s["out_a"], s["out_b"])
        elif not s["dual"]:
            a, b = s["a"], s["b"]
            if s["clip_sigma"]:
                a, b = cl_thresholds(tomo_in, mask, a, b)
            if a == b:
                out = step(tomo_in, a, s["out_a"], s["out_b"])
            else:
                out = threshold2(tomo_in, a, b, a if s["clip"] else s["out_a"], b if s["clip"] else s["out_b"])
        else:
            out = threshold4(tomo_in, s["a"], s["b"], s["c"], s["d"], s["out_a"], s["out_b"])
    if mask is not None:
        out = np.where(inm, out, s["mask_out"]).astype(f32)
    if s["rmm"] is not None:
        sel = out[inm]
        out = rescale01(out, s["rmm"][1], s["rmm"][0], sel.min(), sel.max())
    return out.astype(f32)


def ulp_distance(a, b):
    """distance in float32 ulps between two arrays of finite values (0 where the bits agree)"""
    def key(x):
        u = np.ascontiguousarray(x, f32).view(np.uint32).astype(np.int64)
        return np.where(u & 0x80000000, -(u & 0x7fffffff), u)
    return np.abs(key(a) - key(b))
