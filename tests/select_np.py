"""The top-fraction saliency cut (reference bin/filter_mrc/handlers.cpp:1751-1797) in plain numpy, for the select tests:
collect the voxels whose mask is not zero, sort them in descending order, read entry floor(n * fraction) with the product
taken in float32 (the reference multiplies a size_t by a float), and zero every voxel of the field -- masked or not -- that
is below it.  The reference reads past its array when that entry does not exist; here that is an error."""
import numpy as np

f32 = np.float32


def rank_k(n, fraction):
    """floor(float32(n) * float32(fraction))."""
    return int(np.floor(f32(n) * f32(fraction)))


def included(values, mask):
    v = np.asarray(values, f32).reshape(-1)
    return v if mask is None else v[np.asarray(mask).reshape(-1) != 0]


def threshold_fraction(values, mask, fraction):
    """-> (threshold, thresholded field)."""
    s = included(values, mask)
    n = s.size
    k = rank_k(n, fraction)
    if n == 0 or k >= n:
        raise ValueError("threshold fraction selects no voxel")
    thr = np.sort(s)[::-1][k]
    return thr, np.where(values < thr, f32(0), values)


def order_key(values):
    """The select's 32-bit key: unsigned order of the keys = numeric order of the floats (-0 just below +0)."""
    u = np.ascontiguousarray(values, f32).reshape(-1).view(np.uint32)
    return np.where(u >> 31, ~u, u | np.uint32(0x80000000)).astype(np.uint32)


def round_histogram(values, mask, rnd, prefix):
    """The 2048 counters of radix round `rnd` (digits of 11, 11 and 10 bits from the top) among the keys whose higher
    digits equal `prefix`."""
    key = order_key(values)
    if mask is not None:
        key = key[np.asarray(mask).reshape(-1) != 0]
    shift, width, pshift = ((21, 11, 32), (10, 11, 21), (0, 10, 10))[rnd]
    if rnd > 0:
        key = key[(key.astype(np.uint64) >> np.uint64(pshift)) == np.uint64(prefix)]
    digit = (key >> np.uint32(shift)) & np.uint32((1 << width) - 1)
    return np.bincount(digit, minlength=2048).astype(np.uint64)


def round_prefix(thr, rnd):
    """The higher digits of thr's key that round `rnd` is given."""
    key = int(order_key(np.array([thr], f32))[0])
    return (0, key >> 21, key >> 10)[rnd]
