"""Flat-ball morphology of images with at most two levels, restated in numpy from its definition (include/visfd_hip.h,
visfd_hip_morph_sphere; csrc/morph_levels.hip): the flat ball of DilateSphere is {d^2 <= t_max(radius)}, so a dilation
writes the higher level where a voxel of it lies within the ball and an erosion the lower one.  Squared distances are
integers, minimised by brute force over every position of each axis in turn.  Also the images the tests of that path
share."""
import numpy as np

f32 = np.float32

# (lo, hi); a single entry: a one-level image
LEVEL_SETS = [(0.0, 1.0), (-0.0, 1.0), (-1.0, 0.0), (-np.inf, 3.0), (2.0, np.inf), (5.0,)]
PATTERNS = ["sparse", "half", "block", "corner"]
OPS = ["dilate", "erode", "open", "close", "white", "black"]


def t_max(radius):
    """The largest integer n with float32(sqrt(float64(n))) <= radius: the rule of DilateSphere's flat ball
    (morphology.hpp:253-263) in terms of the squared length of an offset."""
    radius = f32(radius)
    assert np.isfinite(radius) and radius >= 0

    def inside(n):
        return f32(np.sqrt(np.float64(n))) <= radius
    n = int(np.floor(np.float64(radius) ** 2))
    while not inside(n):
        n -= 1
    while inside(n + 1):
        n += 1
    return n


def nearest_dsq(seeds):
    """int64 squared distance from every voxel to the nearest True voxel of `seeds` (a value above every distance in the
    image where there is none), one axis at a time: min over every position of the axis, by brute force."""
    big = np.int64(1) << 40
    g = np.where(seeds, np.int64(0), big)
    for axis in (2, 1, 0):
        n = g.shape[axis]
        pos = np.arange(n, dtype=np.int64)
        best = np.full(g.shape, big, np.int64)
        for j in range(n):
            sl = [slice(None)] * 3
            sl[axis] = slice(j, j + 1)
            shape = [1, 1, 1]
            shape[axis] = n
            best = np.minimum(best, g[tuple(sl)] + ((pos - j) ** 2).reshape(shape))
        g = best
    return g


def _levels(src, valid):
    v = src[valid]
    pats = np.unique(v.view(np.uint32))
    assert len(pats) <= 2 and not np.isnan(v).any(), "not an image of at most two levels"
    if len(pats) == 0:
        return f32(0), f32(0)
    vals = np.sort(pats.view(np.float32))
    assert len(vals) == 1 or vals[0] < vals[1]
    return vals[0], vals[-1]


def _step(img, valid, dilate, lo, hi, t):
    """One Dilate / Erode of an image holding lo <= hi at the valid voxels; returns (image, lo, hi of the result)."""
    zero = f32(0.0)
    if dilate:
        near, far, seeds = f32(hi + zero), f32(lo + zero), valid & (img == hi)
    else:
        near, far, seeds = lo, hi, valid & (img == lo)
    out = np.where(nearest_dsq(seeds) <= t, near, far).astype(np.float32)
    return (out, f32(lo + zero), f32(hi + zero)) if dilate else (out, lo, hi)


def levels_op(op, src, radius, mask=None, dst=None):
    """op 0..5 as morph_np.sphere_op (dilate, erode, open, close, white top-hat dst - open(src), black top-hat
    close(src) - dst) with the flat ball of `radius` on a source of at most two levels; voxels with mask == 0 keep dst."""
    src = np.asarray(src, np.float32)
    valid = np.ones(src.shape, bool) if mask is None else (mask != 0)
    dst = np.array(src if dst is None else dst, np.float32, copy=True)
    t = t_max(radius)
    lo, hi = _levels(src, valid)
    if op in (0, 1):
        res, _, _ = _step(src, valid, op == 0, lo, hi, t)
    else:
        first_dilate = op in (3, 5)
        tmp, lo, hi = _step(src, valid, first_dilate, lo, hi, t)
        res, _, _ = _step(tmp, valid, not first_dilate, lo, hi, t)
    with np.errstate(all="ignore"):
        if op == 4:
            res = dst - res
        elif op == 5:
            res = res - dst
    dst[valid] = res[valid]
    return dst


def seeds(shape, pattern, seed):
    """Where the second level of a test image goes: 0.3 % or 50 % of the voxels at random, a solid block that touches two
    faces, or the single voxel of a corner."""
    rng = np.random.default_rng(seed)
    nz, ny, nx = shape
    s = np.zeros(shape, bool)
    if pattern == "sparse":
        s = rng.random(shape) < 0.003
        s.reshape(-1)[rng.integers(s.size)] = True
    elif pattern == "half":
        s = rng.random(shape) < 0.5
    elif pattern == "block":
        s[: max(1, nz // 2), max(0, ny // 3): max(1, (2 * ny) // 3), max(0, nx - max(1, nx // 4)):] = True
    elif pattern == "corner":
        s[nz - 1, 0, nx - 1] = True
    else:
        raise ValueError(pattern)
    return s


def level_image(shape, levels, pattern, seed):
    """float32 image: levels[-1] at seeds(...), levels[0] elsewhere (a one-level image ignores the pattern)."""
    a = np.full(shape, levels[0], np.float32)
    a[seeds(shape, pattern, seed)] = levels[-1]
    return a


def mask_with_garbage(src, seed):
    """(mask, source): 80 % of the voxels valid; the source holds noise and NaN under the zeros of the mask."""
    rng = np.random.default_rng(seed)
    mask = (rng.random(src.shape) > 0.2).astype(np.float32)
    junk = rng.normal(0.0, 10.0, src.shape).astype(np.float32)
    junk[rng.random(src.shape) < 0.3] = np.nan
    return mask, np.where(mask != 0, src, junk).astype(np.float32)
