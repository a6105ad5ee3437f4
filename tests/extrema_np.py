"""A from-scratch numpy restatement of the reference's plateau-aware extrema search (_FindExtrema, lib/visfd/
morphology_implementation.hpp:57-515), for the extrema tests.  It states the result, not the reference's breadth-first
search: plateaus are labelled by a union-find over the pairs of equal neighbours."""
import numpy as np

f32 = np.float32
INF = float("inf")


def neighbours(connectivity):
    """(dz, dy, dx) with 0 < dx^2 + dy^2 + dz^2 <= connectivity inside the cube of half-width floor(sqrt(connectivity))."""
    r = int(np.floor(np.sqrt(connectivity)))
    rng = range(-r, r + 1)
    return [(dz, dy, dx) for dz in rng for dy in rng for dx in rng
            if (dz, dy, dx) != (0, 0, 0) and dx * dx + dy * dy + dz * dz <= connectivity]


def _pair(shape, off):
    """Slices of the voxels whose neighbour at `off` lies inside the image, and of those neighbours."""
    cs, ns = [], []
    for n, d in zip(shape, off):
        lo, hi = max(0, -d), min(n, n - d)
        if hi <= lo:
            return None
        cs.append(slice(lo, hi))
        ns.append(slice(lo + d, hi + d))
    return tuple(cs), tuple(ns)


def find_extrema(src, mask=None, find_minima=True, find_maxima=True, minima_threshold=INF, maxima_threshold=-INF,
                 connectivity=3, allow_borders=True, labels=None):
    """-> dict(min=(index int64, score float32, nvoxels int64), max=(...), labels=int32 volume).  src (nz, ny, nx).
    `labels`: the volume the label image is written into (voxels with mask == 0 keep its values); default zeros."""
    src = np.asarray(src, f32)
    shape = src.shape
    N = src.size
    exist = np.ones(shape, bool) if mask is None else (np.asarray(mask) != 0)
    lower = np.zeros(shape, bool)
    higher = np.zeros(shape, bool)
    missing = np.zeros(shape, bool)
    equal = []
    with np.errstate(invalid="ignore"):
        for off in neighbours(connectivity):
            gone = np.ones(shape, bool)   # the neighbour is outside the image or masked out
            p = _pair(shape, off)
            if p is not None:
                cs, ns = p
                gone[cs] = ~exist[ns]
                both = exist[cs] & exist[ns]
                a, b = src[cs], src[ns]
                lower[cs] |= both & (b < a)
                higher[cs] |= both & (b > a)
                equal.append((cs, ns, both & (a == b)))
            missing |= gone & exist
    # plateaus: every voxel ends with the smallest linear index of its plateau, the root.  Union-find over the pairs of
    # equal neighbours: the larger of two roots is hooked under the smaller, then every voxel jumps to its root.
    index = np.arange(N, dtype=np.int64).reshape(shape)
    A = np.concatenate([index[cs][e] for cs, ns, e in equal]) if equal else np.zeros(0, np.int64)
    B = np.concatenate([index[ns][e] for cs, ns, e in equal]) if equal else np.zeros(0, np.int64)
    lab = np.arange(N, dtype=np.int64)
    while True:
        ra, rb = lab[A], lab[B]
        hi, lo = np.maximum(ra, rb), np.minimum(ra, rb)
        apart = hi != lo
        if not apart.any():
            break
        np.minimum.at(lab, hi[apart], lo[apart])
        while True:
            nxt = lab[lab]
            if np.array_equal(nxt, lab):
                break
            lab = nxt
    flat = lab.reshape(-1)
    ex = exist.reshape(-1)
    members = flat[ex]
    nvox = np.bincount(members, minlength=N)
    any_lower = np.bincount(members, weights=lower.reshape(-1)[ex], minlength=N) > 0
    any_higher = np.bincount(members, weights=higher.reshape(-1)[ex], minlength=N) > 0
    any_missing = np.bincount(members, weights=missing.reshape(-1)[ex], minlength=N) > 0
    roots = np.nonzero(ex & (flat == np.arange(N)))[0]   # raster order
    barred = any_missing[roots] & (not allow_borders)
    is_min = ~any_lower[roots] & ~barred
    is_max = ~any_higher[roots] & ~barred
    val = src.reshape(-1)[roots]
    with np.errstate(invalid="ignore"):
        listed_min = is_min & (val <= f32(minima_threshold)) & bool(find_minima)
        listed_max = is_max & (val >= f32(maxima_threshold)) & bool(find_maxima)

    def ordered(listed, descending):
        sel = np.nonzero(listed)[0]
        order = np.lexsort((np.arange(len(sel)), val[sel]))   # ascending (score, raster position); -0 == +0
        if descending:
            order = order[::-1]                                # the exact reverse of ascending
        rank = np.empty(len(sel), np.int64)
        rank[order] = np.arange(1, len(sel) + 1)               # raster position -> 1-based position in the list
        pick = sel[order]
        return (roots[pick].astype(np.int64), val[pick].copy(), nvox[roots[pick]].astype(np.int64)), rank

    mins, rank_min = ordered(listed_min, False)
    maxs, rank_max = ordered(listed_max, True)
    # numbering: the count of listed entries up to and including this root, then that entry's place in the sorted list
    kmin, kmax = np.cumsum(listed_min), np.cumsum(listed_max)
    rank_min = np.concatenate(([0], rank_min))
    rank_max = np.concatenate(([0], rank_max))
    plateau = np.where(is_max, rank_max[kmax], np.where(is_min, -rank_min[kmin], 0))
    if not (find_minima and find_maxima):
        plateau = np.abs(plateau)
    by_root = np.zeros(N, np.int64)
    by_root[roots] = plateau
    out = np.zeros(shape, np.int32) if labels is None else np.array(labels, np.int32).reshape(shape)
    out.reshape(-1)[ex] = by_root[members]
    return {"min": mins, "max": maxs, "labels": out}


def find_minima(src, mask=None, threshold=INF, connectivity=3, allow_borders=True, labels=None):
    return find_extrema(src, mask, True, False, threshold, -INF, connectivity, allow_borders, labels)


def find_maxima(src, mask=None, threshold=INF, connectivity=3, allow_borders=True, labels=None):
    """The single-kind wrappers turn a threshold of +inf into -inf (morphology_implementation.hpp:573-574, :775-776)."""
    if threshold == INF:
        threshold = -INF
    return find_extrema(src, mask, False, True, INF, threshold, connectivity, allow_borders, labels)
