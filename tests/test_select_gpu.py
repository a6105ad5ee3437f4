"""The top-fraction saliency cut on the GPU (csrc/select.hip) against the numpy reference (tests/select_np.py, which
tests/test_select.py holds to the oracle and the compiled reference), on every case of tests/select_cases.py: through the
host face, through the device face with the pointer 0, 1, 2 and 3 floats past a 16-byte boundary, and through the Python
walk of visfd_amd/slab.py over the device histograms.  Every result must give select_np's threshold, select_np's field
bit for bit, and pass a rank certificate that involves neither: with k = floor(float32(n) * float32(fraction)), among the
included voxels count(v > thr) <= k < count(v >= thr).

The sizes that decide which path the histogram kernel takes come from the device: above (compute units * 32 * 256) float4
loads the grid is capped and the two-loads-in-flight loop runs."""
import types

import numpy as np
import pytest

import select_cases as SC
import select_np
from conftest import assert_bits_equal

pytestmark = pytest.mark.gpu

f32 = np.float32
WORLD1 = types.SimpleNamespace(world=1)
GUARD = 8      # floats of NaN either side of a device field: counted if read, found changed if written


@pytest.fixture(scope="module")
def ctx():
    """A context on a stream of its own that is also torch's current stream, as visfd_amd/slab.py requires."""
    import torch
    from visfd_amd import api
    before = torch.cuda.current_stream()
    st = torch.cuda.Stream()
    torch.cuda.set_stream(st)
    c = api.Context(0, st.cuda_stream)
    yield c
    c.close()
    torch.cuda.set_stream(before)


def on_device(values, offset=0):
    """-> (buffer, view): the values `offset` floats past a 16-byte boundary, NaN around them."""
    import torch
    n = values.size
    buf = torch.full((n + 2 * GUARD,), float("nan"), device="cuda")
    assert buf.data_ptr() % 16 == 0
    view = buf[GUARD + offset:GUARD + offset + n]
    assert view.data_ptr() % 16 == 4 * offset
    view.copy_(torch.from_numpy(values))
    return buf, view


def guards_intact(buf, view):
    import torch
    outside = torch.ones(buf.numel(), dtype=torch.bool, device=buf.device)
    first = (view.data_ptr() - buf.data_ptr()) // 4
    outside[first:first + view.numel()] = False
    return bool(torch.isnan(buf[outside]).all())


def certificate(pre, mask, thr, fraction, what):
    """pre, mask: torch tensors of the field before the call.  No sort, no oracle, no code under test."""
    inc = pre if mask is None else pre[mask != 0]
    k = select_np.rank_k(inc.numel(), fraction)
    above, at_least = int((inc > thr).sum()), int((inc >= thr).sum())
    assert above <= k < at_least, "%s: thr %r is not entry %d of the descending order (%d above it, %d not below it)" % (
        what, thr, k, above, at_least)


def check(ctx, case, offsets=(0, 1, 2, 3), host=True, walk=True):
    import torch
    from visfd_amd import slab
    name, values, mask, fraction = case
    thr, want = select_np.threshold_fraction(values, mask, fraction)
    if host:
        got = values.copy()
        t = ctx.threshold_fraction(got, fraction, mask)
        assert f32(t) == thr, (name, "host face", t, thr)
        assert_bits_equal(got, want, name + " host face")
        certificate(torch.from_numpy(values), None if mask is None else torch.from_numpy(mask), t, fraction, name + " host face")
    dm = None if mask is None else torch.from_numpy(mask).cuda()
    for off in offsets:
        what = "%s device face, offset %d" % (name, off)
        buf, sal = on_device(values, off)
        pre = sal.clone()
        t = ctx.threshold_fraction_dev(sal, fraction, dm)
        ctx.synchronize()
        assert f32(t) == thr, (what, t, thr)
        certificate(pre, dm, t, fraction, what)
        assert_bits_equal(sal.cpu().numpy(), want, what)
        assert guards_intact(buf, sal), what
        if walk and off == offsets[-1]:     # the Python walk over the device histograms of the untouched field
            assert f32(slab.distributed_threshold_fraction(ctx, pre, fraction, WORLD1, dm)) == thr, what + " (Python walk)"


@pytest.mark.parametrize("group", SC.GROUPS)
def test_case_table(ctx, group):
    for case in SC.cases_of(group):
        check(ctx, case)


@pytest.mark.parametrize("n", SC.BIG)
def test_above_2_24(ctx, n):
    """float32(n) != n: k comes from the float product of the reference, in the kernel's capped-grid regime."""
    v = SC.big_field(n)
    f0, f1 = SC.BIG_FRACTIONS[n]
    check(ctx, SC.Case("n=%d/f=%.9g" % (n, f0), v, None, f0), offsets=(0, 1))
    check(ctx, SC.Case("n=%d/f=%.9g" % (n, f1), v, None, f1), offsets=(0,), host=False)
    ties, _ = SC.with_ties_at_cut(v, f0, n)
    check(ctx, SC.Case("n=%d/ties/f=%.9g" % (n, f0), ties, None, f0), offsets=(0, 1), host=False)
    m = SC.random_mask(n, np.random.default_rng(n))
    nm = int((m != 0).sum())
    check(ctx, SC.Case("n=%d/mask/f=%.9g" % (n, f0), v, m, f0), offsets=(0,))
    assert nm < (1 << 24)      # (the masked count is below 2^24 again: the product is exact there)


def test_device_sized(ctx):
    """The capped grid, the two-loads-in-flight float4 loop, its one-load remainder in some threads only, and a scalar
    tail, all in one call: n is built from the device's compute-unit count."""
    import torch
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    n, step = SC.device_sized_n(cus)
    n4 = n // 4
    assert n4 > step                                      # the loop `j + step < n4` runs (and the grid is capped at step / 256)
    assert 0 < n4 % step < step and (n4 // step) % 2 == 0   # after the loop some threads have one load left, some none
    assert n % 4 == 3                                     # and three floats go to the scalar tail
    fraction = 0.25
    v, tie = SC.with_ties_at_cut(np.random.default_rng(cus).standard_normal(n, dtype=f32), fraction, cus)
    thr, _ = select_np.threshold_fraction(v, None, fraction)
    assert thr == tie
    check(ctx, SC.Case("device-sized n=%d" % n, v, None, fraction), offsets=(0, 1))
    m = SC.random_mask(n, np.random.default_rng(cus + 1))
    check(ctx, SC.Case("device-sized n=%d/mask" % n, v, m, fraction), offsets=(0,), host=False)
    # the histogram faces at this size, whole and as three uneven shards that start 0, 1 and 2 floats past a boundary
    buf, sal = on_device(v, 0)
    a, b = n // 8 * 4 + 1, (n // 2 + step) // 4 * 4 + 2
    assert a % 4 == 1 and b % 4 == 2 and a < b < n and a // 4 > step      # the aligned first shard runs the loop too
    for rnd in range(3):
        histogram_faces(ctx, v, sal, None, rnd, select_np.round_prefix(thr, rnd), (0, a, b, n))


def histogram_faces(ctx, values, sal, dm, rnd, prefix, cuts):
    """Both faces return the numpy histogram of the order key; the shards' counters sum to the whole volume's."""
    import torch
    mask = None if dm is None else dm.cpu().numpy()
    want = select_np.round_histogram(values, mask, rnd, prefix)

    def both(s, m):
        h, count = ctx.select_histogram_dev(s, rnd, prefix, m)
        hdev = torch.full((2048,), -1, dtype=torch.int64, device="cuda")
        ctx.select_histogram_todev(s, rnd, prefix, hdev, m)
        ctx.synchronize()
        assert np.array_equal(hdev.cpu().numpy().astype(np.uint64), h), "the two histogram faces differ"
        assert count == int(h.sum())
        return h

    whole = both(sal, dm)
    assert np.array_equal(whole, want), ("round %d" % rnd, np.flatnonzero(whole != want)[:4])
    if rnd == 0:
        assert int(whole.sum()) == select_np.included(values, mask).size
    total = np.zeros(2048, np.uint64)
    for lo, hi in zip(cuts[:-1], cuts[1:]):
        total += both(sal[lo:hi], None if dm is None else dm[lo:hi])
    assert np.array_equal(total, whole), "shards do not sum to the whole"


@pytest.mark.parametrize("group", ["normals", "zeros", "prefix11_neg", "prefix22_pos", "straddle_denormal", "hostile_zeros",
                                   "size_70001"])
def test_histogram_faces(ctx, group):
    import torch
    case = SC.cases_of(group)[3]
    n = case.values.size
    thr, _ = select_np.threshold_fraction(case.values, case.mask, case.fraction)
    a = n // 5 - (n // 5) % 4 + 1
    b = (2 * n) // 3 - ((2 * n) // 3) % 4 + 2
    assert 0 < a < b < n and a % 4 == 1 and b % 4 == 2
    buf, sal = on_device(case.values, 0)
    for dm in [None] + ([] if case.mask is None else [torch.from_numpy(case.mask).cuda()]):
        for rnd in range(3):
            histogram_faces(ctx, case.values, sal, dm, rnd, select_np.round_prefix(thr, rnd), (0, a, b, n))
            histogram_faces(ctx, case.values, sal, dm, rnd, 0x155 if rnd else 0, (0, a, b, n))     # a prefix nothing has


@pytest.mark.parametrize("n", [SC.N0, 70001])
def test_apply_threshold(ctx, n):
    """v < thr -> 0 and nothing else: NaN (both signs), -0 and +0 and the infinities survive where the comparison is
    false, whatever the threshold."""
    rng = np.random.default_rng(n)
    v = SC.zeros_mix(n, rng)
    r = rng.permutation(n)
    m = n // 20
    for i, x in enumerate([np.nan, -np.nan, np.inf, -np.inf, 1e-45, -1e-45, 1e-39, -1e-39]):
        v[r[i * m:(i + 1) * m]] = f32(x)
    for thr in (-np.inf, -0.0, 0.0, 0.5, -0.5, np.inf, np.nan, 1e-45, -1e-45, float(np.finfo(f32).tiny)):
        with np.errstate(invalid="ignore"):
            want = np.where(v < f32(thr), f32(0), v)
        assert np.isnan(want).sum() == 2 * m and (thr != 0 or np.signbit(want[v == 0]).any())     # -0 survives thr = 0
        for off in (0, 1):
            buf, sal = on_device(v, off)
            ctx.apply_threshold_dev(sal, thr)
            ctx.synchronize()
            assert_bits_equal(sal.cpu().numpy(), want, "apply_threshold thr=%r offset %d" % (thr, off))
            assert guards_intact(buf, sal)


@pytest.mark.parametrize("case", SC.REFUSALS, ids=[c.name for c in SC.REFUSALS])
def test_refusals(ctx, case):
    """A fraction that selects no voxel is an error from every face; the field is left alone and the context goes on."""
    import torch
    from visfd_amd import api, slab
    name, values, mask, fraction = case
    good = SC.cases_of("size_315")[3]
    got = values.copy()
    with pytest.raises(api.VisfdHipError):
        ctx.threshold_fraction(got, fraction, mask)
    assert got.tobytes() == values.tobytes()
    check(ctx, good, offsets=(1,), walk=False)
    dm = None if mask is None else torch.from_numpy(mask).cuda()
    if values.size:
        buf, sal = on_device(values, 0)
    else:
        buf = sal = torch.empty(0, device="cuda")
    with pytest.raises(api.VisfdHipError):
        ctx.threshold_fraction_dev(sal, fraction, dm)
    ctx.synchronize()
    assert sal.cpu().numpy().tobytes() == values.tobytes()
    check(ctx, good, offsets=(0,), host=False, walk=False)
    with pytest.raises((ValueError, api.VisfdHipError)):
        slab.distributed_threshold_fraction(ctx, sal, fraction, WORLD1, dm)
    assert sal.cpu().numpy().tobytes() == values.tobytes()
    check(ctx, good, offsets=(2,), host=False)
