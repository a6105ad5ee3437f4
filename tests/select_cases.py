"""Inputs for the top-fraction saliency cut (csrc/select.hip and its three host walks), numpy only: signed fields, ties,
keys that share their leading radix digits, masks that hide hostile values, every fraction edge and the sizes at which
the kernel changes its path.  A case is (name, values float32[n], mask float32[n] or None, fraction); the first component
of the name ("field/...") is the group the tests are parametrised by.

No case holds a NaN in an included voxel: the reference's std::sort on NaN is undefined, so there is nothing to compare
with ("The top-fraction cut").

What the builders assert about their own cases is pure CPU arithmetic and runs at import."""
import collections

import numpy as np

from select_np import included, order_key, rank_k

f32 = np.float32
Case = collections.namedtuple("Case", "name values mask fraction")

SIZES = (5, 7, 8, 315, 4096, 70001)     # around the float4 / scalar-tail boundaries of the histogram kernel
N0 = 4099                               # the size of the field cases: odd, so a three-float tail follows the float4 part
BELOW_ONE = float(np.nextafter(f32(1), f32(0)))     # 1 - 2^-24
BIG = ((1 << 24) + 1, (1 << 24) + 3)    # float32(n) != n: 2^24 + 1 -> 2^24, 2^24 + 3 -> 2^24 + 4


def _bits(u):
    return np.ascontiguousarray(u, np.uint32).view(f32)


def _rng(*seed):
    return np.random.default_rng(list(seed))


# ---- fields: f(n, rng) -> float32[n] ---------------------------------------------------------------------------------
def normals(n, rng):
    return rng.standard_normal(n).astype(f32)


def negatives(n, rng):
    return -(np.abs(rng.standard_normal(n)) + 0.25).astype(f32)


def zeros_mix(n, rng):
    """Signed normals with a fifth of the voxels +0 and a fifth -0 (at least one of each)."""
    v = normals(n, rng)
    r = rng.permutation(n)
    v[r[:max(1, n // 5)]] = f32(0.0)
    v[r[max(1, n // 5):max(2, 2 * (n // 5))]] = f32(-0.0)
    return v


def infinities(n, rng):
    v = normals(n, rng)
    r = rng.permutation(n)
    m = max(1, n // 30)
    v[r[:m]] = np.inf
    v[r[m:2 * m]] = -np.inf
    return v


def denormals(n, rng):
    return _bits(rng.integers(1, 1 << 23, n).astype(np.uint32) | (rng.integers(0, 2, n).astype(np.uint32) << 31))


def wide(n, rng):
    """Magnitudes from 1e-38 to 1e38, both signs."""
    return (rng.choice([-1.0, 1.0], n) * 10.0 ** rng.uniform(-38, 38, n)).astype(f32)


def all_equal(n, rng):
    return np.full(n, -1.5, f32)


def majority(n, rng):
    """One value in 60 % of the voxels."""
    v = normals(n, rng)
    v[rng.permutation(n)[:(3 * n) // 5]] = f32(0.375)
    return v


def _ulps(base, span, sign=None):
    def f(n, rng):
        s = rng.integers(0, 2, n) if sign is None else np.full(n, sign)
        return _bits((s.astype(np.uint32) << 31) | np.uint32(base) + rng.integers(0, span, n).astype(np.uint32))
    return f


def _shares_top_bits(v, nbits):
    k = order_key(v) >> np.uint32(32 - nbits)
    return bool((k == k[0]).all())


FIELDS = collections.OrderedDict([
    ("normals", normals), ("negatives", negatives), ("zeros", zeros_mix), ("infinities", infinities),
    ("denormals", denormals), ("wide", wide), ("all_equal", all_equal), ("majority", majority),
    # base + j ulps: every key agrees in its top 11 bits (round 0 has one bin, rounds 1 and 2 do the work) ...
    ("prefix11_pos", _ulps(0x3F800000, 1 << 21, 0)), ("prefix11_neg", _ulps(0x3F800000, 1 << 21, 1)),
    # ... or in its top 22 (only round 2 separates them; with 1024 values in 4099 voxels every value is a tie)
    ("prefix22_pos", _ulps(0x3F800000, 1 << 10, 0)), ("prefix22_neg", _ulps(0x3F800000, 1 << 10, 1)),
])
# +-(base + j ulps) with both signs: the two halves sit in the two key bins either side of the sign change
STRADDLES = collections.OrderedDict([("straddle_denormal", _ulps(1, 512)), ("straddle_normal", _ulps(0x00800000, 512))])


# ---- fractions -------------------------------------------------------------------------------------------------------
def fraction_for_k(n, k):
    f = float(f32((k + 0.5) / n))
    assert rank_k(n, f) == k, (n, k, f)
    return f


def top_fraction(n):
    """The largest float32 fraction below 1 that still selects a voxel, and its k.  k is n - 1 wherever a fraction can give
    that: float32(n) * f reaches at most float32(n) * (1 - 2^-24), which for n = 2^24 + 1 (float32(n) = 2^24) is n - 2."""
    f = f32(BELOW_ONE)
    while rank_k(n, f) >= n:
        f = np.nextafter(f, f32(0))
    k = rank_k(n, f)
    assert k == n - 1 or float(f32(n)) * (1.0 - 2.0 ** -24) < n - 1, (n, float(f), k)
    return float(f)


def fractions(n):
    out = []
    for f in (0.0, 1.0 / n, 0.05, 0.25, 0.5, (n - 1.0) / n, top_fraction(n)):
        f = float(f32(f))
        if f not in out and rank_k(n, f) < n:
            out.append(f)
    return out


# ---- masks -----------------------------------------------------------------------------------------------------------
def random_mask(n, rng, keep=0.8):
    m = (rng.random(n) < keep).astype(f32)
    m[rng.integers(0, n)] = 1
    m[m != 0] = rng.choice(np.array([1.0, 0.5, -2.0], f32), int((m != 0).sum()))     # any non-zero value means "exists"
    return m


def single_mask(n, rng):
    m = np.zeros(n, f32)
    m[rng.integers(0, n)] = 1
    return m


def hostile(v, rng):
    """-> (values, mask): the excluded voxels hold NaN (both signs), +inf and values above every included one."""
    n = v.size
    m = random_mask(n, rng, 0.7)
    out = np.flatnonzero(m == 0)
    v = v.copy()
    top = np.abs(v).max()
    fill = np.array([np.nan, np.inf, top * 8, -np.nan, top + 1], f32)
    v[out] = fill[np.arange(out.size) % fill.size]
    assert not np.isnan(included(v, m)).any()
    return v, m


# ---- the table -------------------------------------------------------------------------------------------------------
def _add(cases, name, v, m, f):
    v = np.ascontiguousarray(v, f32)
    assert not np.isnan(included(v, m)).any(), name
    assert rank_k(included(v, m).size, f) < included(v, m).size, name
    cases.append(Case("%s/%s/f=%.9g" % (name, "nomask" if m is None else "mask", f), v, m, float(f)))


def _three_values(cases):
    """3 in a quarter of the voxels, 0.5 in half, -2 in the rest: the cut inside the middle run and at both its ends, and on
    the last 3 and the first -2."""
    n = N0
    a, b = n // 4, n // 2
    v = np.concatenate([np.full(a, 3.0), np.full(b, 0.5), np.full(n - a - b, -2.0)]).astype(f32)
    v = v[_rng(7, 0).permutation(n)]
    for k in (a - 1, a, a + b // 2, a + b - 1, a + b, 0, n - 1):
        _add(cases, "three_values/k=%d" % k, v, None, fraction_for_k(n, k))
    m = random_mask(n, _rng(7, 1))
    s = np.sort(included(v, m))[::-1]
    first, last = int(np.argmax(s == 0.5)), int(s.size - 1 - np.argmax(s[::-1] == 0.5))
    for k in (first, (first + last) // 2, last):
        _add(cases, "three_values/k=%d" % k, v, m, fraction_for_k(s.size, k))


def _straddles(cases):
    for i, (name, gen) in enumerate(STRADDLES.items()):
        v = gen(N0, _rng(8, i))
        npos = int((v > 0).sum())
        assert 0 < npos < N0 and not (v == 0).any()
        key = order_key(v) >> np.uint32(21)
        bins = sorted(set(key.tolist()))                      # two round-0 bins, one either side of the sign change
        assert len(bins) == 2 and bins[0] < 0x400 <= bins[1] and (i > 0 or bins == [0x3FF, 0x400])
        for k in (npos - 1, npos):                            # the smallest positive value, the largest negative one
            _add(cases, "%s/k=%d" % (name, k), v, None, fraction_for_k(N0, k))
        for f in fractions(N0):
            _add(cases, name, v, None, f)
        m = random_mask(N0, _rng(8, i, 1))
        s = included(v, m)
        for k in (int((s > 0).sum()) - 1, int((s > 0).sum())):
            _add(cases, "%s/k=%d" % (name, k), v, m, fraction_for_k(s.size, k))


def _build():
    cases = []
    for i, (name, gen) in enumerate(FIELDS.items()):
        v = gen(N0, _rng(1, i))
        if name.startswith("prefix"):
            nb = int(name[6:8])
            assert _shares_top_bits(v, nb) and not _shares_top_bits(v, 32), name
        for f in fractions(N0):
            _add(cases, name, v, None, f)
    _three_values(cases)
    _straddles(cases)
    # masks: random, one voxel left, and hostile values behind the mask
    for i, name in enumerate(("normals", "zeros", "infinities", "majority", "prefix22_neg")):
        v = FIELDS[name](N0, _rng(2, i))
        m = random_mask(N0, _rng(3, i))
        for f in fractions(int((m != 0).sum())):
            _add(cases, name, v, m, f)
        m = single_mask(N0, _rng(4, i))
        for f in (0.0, 0.5, BELOW_ONE):
            _add(cases, name + "/single", v, m, f)
    for i, name in enumerate(("normals", "negatives", "zeros")):
        v, m = hostile(FIELDS[name](N0, _rng(5, i)), _rng(6, i))
        for f in fractions(int((m != 0).sum())):
            _add(cases, "hostile_" + name, v, m, f)
    # sizes around the kernel's boundaries: signed values with ties
    for n in SIZES:
        v = zeros_mix(n, _rng(9, n))
        v[_rng(10, n).permutation(n)[:max(1, n // 10)]] = f32(-0.75)
        for f in fractions(n):
            _add(cases, "size_%d" % n, v, None, f)
        m = random_mask(n, _rng(11, n))
        for f in (0.0, 0.25, top_fraction(int((m != 0).sum()))):
            _add(cases, "size_%d" % n, v, m, f)
    return cases


CASES = _build()
GROUPS = list(collections.OrderedDict((c.name.split("/")[0], 1) for c in CASES))


def cases_of(group):
    return [c for c in CASES if c.name.split("/")[0] == group]


# ---- refusals: the entry floor(n * fraction) does not exist ------------------------------------------------------------
def _refusals():
    v = normals(315, _rng(12))
    out = [Case("fraction=1", v, None, 1.0), Case("fraction=1.5", v, None, 1.5),
           Case("fraction=1/masked", v, random_mask(315, _rng(13)), 1.0),
           Case("all_masked", v, np.zeros(315, f32), 0.25), Case("all_masked/f=0", v, np.zeros(315, f32), 0.0),
           Case("empty", np.zeros(0, f32), None, 0.25)]
    return out


REFUSALS = _refusals()


# ---- sizes above 2^24, where float32(n) != n --------------------------------------------------------------------------
def _exact_k(n, f):
    """floor(n * f) with f the float32 fraction, in exact (integer) arithmetic."""
    num, den = float(f32(f)).as_integer_ratio()
    return n * num // den


# n = 2^24 + 3: float32(n) = n + 1, so the float32 product and the exact one part company already at 0.5.
# n = 2^24 + 1: float32(n) = 2^24, and 2^24 * f is exact for every float32 f; with f = m * 2^-(24+e) < 2^-e the exact
# product is m * 2^-e + f, whose fractional part stays below 1: no fraction separates the two floors there.  The case
# keeps the size (float32(n) rounds) with an ordinary fraction.
BIG_FRACTIONS = {BIG[0]: (0.25, BELOW_ONE), BIG[1]: (0.5, BELOW_ONE)}
assert float(f32(BIG[0])) == BIG[0] - 1 and float(f32(BIG[1])) == BIG[1] + 1
assert rank_k(BIG[1], 0.5) == _exact_k(BIG[1], 0.5) + 1
assert all(rank_k(BIG[0], f) == _exact_k(BIG[0], f) for f in (0.05, 0.25, 0.3, 0.5, 0.7, BELOW_ONE))
assert rank_k(BIG[0], BELOW_ONE) == BIG[0] - 2 and rank_k(BIG[1], BELOW_ONE) == BIG[1] - 1


def big_field(n):
    """Signed normals; 64 MB, so built on demand."""
    return _rng(15, n).standard_normal(n, dtype=f32)


def with_ties_at_cut(v, fraction, seed, share=0.1):
    """A tenth of the voxels set to the value at the cut of v, which puts the cut inside that run of ties."""
    n = v.size
    k = rank_k(n, fraction)
    thr = np.partition(v, n - 1 - k)[n - 1 - k]
    v = v.copy()
    v[_rng(16, seed).random(n) < share] = thr
    assert int((v > thr).sum()) < k < int((v >= thr).sum()) - 1
    return v, thr


def device_sized_n(cus):
    """-> (n, step) for a device of `cus` compute units: the histogram's grid is capped at cus * 32 workgroups of 256
    threads, n / 4 float4 loads are 2.5 grid-wide steps and a bit, and three floats are left for the scalar tail."""
    step = cus * 32 * 256
    return 4 * (2 * step + step // 2 + 37) + 3, step
