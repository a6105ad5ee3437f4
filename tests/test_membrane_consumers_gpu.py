"""The two consumers of the saliency cut on their own: ridge_directions_kernel and the sender lists of tensor voting
(csrc/ridge.hip, csrc/tv_list.hip) given the threshold in device memory and a volume that has NOT been cut, against the same
kernels on the copy that apply_threshold has cut.  The predicate !(s < thr) && s != 0 must pick the voxels the cut followed by
s != 0 leaves: scores equal to the threshold, +inf and NaN stay, zeros of either sign and everything below go; a threshold
of +0, -0 or below zero (negative scores present) behaves like the cut."""
import numpy as np
import pytest

from conftest import assert_bits_equal

pytestmark = pytest.mark.gpu

FILL = 7.0
SIGMA = 1.5
SHAPES = [(5, 7, 70), (4, 300, 40), (3, 3, 3)]   # rows no multiple of 64, rows past 256, the smallest volume


@pytest.fixture(scope="module")
def ctx():
    from visfd_amd import api
    c = api.Context(0)
    yield c
    c.close()


def _dev(a):
    import torch
    t = torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")
    torch.cuda.synchronize()
    return t


def _host(ctx, t):
    ctx.synchronize()
    return t.cpu().numpy()


def _scores(shape, seed, negative):
    """Scores with ties at the cut, exact zeros of both signs, and +inf and NaN above it."""
    rng = np.random.default_rng(seed)
    s = rng.integers(1, 40, size=shape).astype(np.float32) / np.float32(8.0)   # many equal values
    if negative:
        s -= np.float32(2.5)
    flat = s.reshape(-1)
    idx = rng.permutation(flat.size)
    q = max(flat.size // 9, 1)
    flat[idx[:q]] = 0.0
    flat[idx[q:2 * q]] = -0.0
    flat[idx[2 * q]] = np.inf
    if flat.size > 2 * q + 1:
        flat[idx[2 * q + 1]] = np.nan
    return s


def _thresholds(s):
    vals = np.unique(s[np.isfinite(s)])
    return [np.float32(vals[len(vals) // 2]), np.float32(0.0), np.float32(-0.0), np.float32(vals[-1]), np.float32(np.inf),
            np.float32(vals[0])]


def _cut_copy(ctx, s, thr):
    t = _dev(s)
    ctx.apply_threshold_dev(t, float(thr))
    return t


@pytest.mark.parametrize("negative", [False, True], ids=["positive", "signed"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_directions_cut_for_themselves(ctx, shape, negative):
    from visfd_amd import api
    rng = np.random.default_rng(3)
    smoothed = _dev(rng.standard_normal(shape).astype(np.float32))
    s = _scores(shape, 11, negative)
    for mode in ({}, {"eig_f32": 1}):
        for thr in _thresholds(s):
            cut = _cut_copy(ctx, s, thr)
            want, got = _dev(np.full((3,) + shape, FILL, np.float32)), _dev(np.full((3,) + shape, FILL, np.float32))
            with ctx.options(**mode):
                ctx.ridge_directions_dev(smoothed, cut, want, SIGMA, api.DECREASING_EIVALS)
                ctx.debug_ridge_directions_thr_dev(smoothed, _dev(s), got, SIGMA, api.DECREASING_EIVALS, _dev(np.array([thr], np.float32)))
            w, g = _host(ctx, want), _host(ctx, got)
            assert_bits_equal(g, w, "directions, thr %r" % thr)
            kept = _host(ctx, cut) != 0
            assert np.array_equal(kept, w[0] != FILL)
            assert kept[np.isposinf(s)].all() and kept[np.isnan(s)].all()   # +inf and NaN pass every cut
            assert not kept[s == 0].any()                                    # zeros of either sign pass none


def _lists_equal(a, b, ny, what):
    rows_a, ent_a, pos_a, flags_a = a
    rows_b, ent_b, pos_b, flags_b = b
    assert flags_a == flags_b and len(pos_a) == len(pos_b), (what, flags_a, flags_b, len(pos_a), len(pos_b))
    # where a list lies in the entry arrays differs from run to run: compare offsets inside each list, and the lists' contents
    assert np.array_equal(rows_a - rows_a[:, ny:ny + 1, :], rows_b - rows_b[:, ny:ny + 1, :]), what
    nz, _, ntx = rows_a.shape
    for z in range(nz):
        for tx in range(ntx):
            sa = slice(int(rows_a[z, ny, tx]), int(rows_a[z, 0, tx]))
            sb = slice(int(rows_b[z, ny, tx]), int(rows_b[z, 0, tx]))
            assert_bits_equal(ent_a[sa], ent_b[sb], "%s: entries of list (%d, %d)" % (what, z, tx))
            assert np.array_equal(pos_a[sa], pos_b[sb]), "%s: positions of list (%d, %d)" % (what, z, tx)


@pytest.mark.parametrize("negative", [False, True], ids=["positive", "signed"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_sender_lists_cut_for_themselves(ctx, shape, negative):
    rng = np.random.default_rng(4)
    d = rng.standard_normal((3,) + shape).astype(np.float32)
    dirs = _dev(d / np.sqrt((d * d).sum(0, keepdims=True)))
    s = _scores(shape, 12, negative)
    total_seen = 0
    for h, mode in ((4, 0), (12, 1), (2, 2)):   # windows clipped on both sides of the short rows
        for thr in _thresholds(s):
            want = ctx.debug_tv_lists_dev(_cut_copy(ctx, s, thr), dirs, h, mode)
            got = ctx.debug_tv_lists_dev(_dev(s), dirs, h, mode, thr_dev=_dev(np.array([thr], np.float32)))
            _lists_equal(got, want, shape[1], "h %d mode %d thr %r" % (h, mode, thr))
            total_seen += len(want[2])
    assert total_seen > 0


def test_folded_lists_cut_for_themselves(ctx):
    """Positive, finite scores: the folded records (tolerance vote, exponent 4) through both forms."""
    shape = (5, 7, 70)
    rng = np.random.default_rng(6)
    d = rng.standard_normal((3,) + shape).astype(np.float32)
    dirs = _dev(d / np.sqrt((d * d).sum(0, keepdims=True)))
    s = rng.integers(0, 30, size=shape).astype(np.float32) / np.float32(4.0)
    thr = np.float32(3.5)
    want = ctx.debug_tv_lists_dev(_cut_copy(ctx, s, thr), dirs, 4, 0, fold=True)
    got = ctx.debug_tv_lists_dev(_dev(s), dirs, 4, 0, fold=True, thr_dev=_dev(np.array([thr], np.float32)))
    assert want[3] == 0 and len(want[2]) > 100
    _lists_equal(got, want, shape[1], "folded")
