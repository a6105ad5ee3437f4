"""The membrane stage queued in one go (option membrane_queue = 1: digits of the select picked on the device, no threshold pass,
one wait per stage; csrc/api.hip: membrane_stage) against the sequence it replaces (membrane_queue = 0) on the same context
and input: the threshold as a number, `sal` and `ten` bit for bit, `dirs` bit for bit where the old path's cut `sal` is
non-zero (and, both runs starting from the same fill, everywhere else too: neither may write a voxel the other leaves).
Both arithmetic modes (tv_fma / eig_f32 / gauss_fma on and off).  Volumes: rows that are no multiple of 16 or 64 with list
windows clipped on both sides, the smallest volume the ridge stage takes, rows past 256 (the y << 8 of tv_list.hip), a run of
exact zeros that holds the cut, and tied scores at the cut."""
import numpy as np
import pytest

import volgen
from conftest import assert_bits_equal

pytestmark = pytest.mark.gpu

SIGMA, TV_RATIO = 1.5, 2.0      # vote windows of half-width floor(3 sqrt 2) = 4
MODES = [pytest.param({}, id="exact"), pytest.param(dict(tv_fma=1, eig_f32=1, gauss_fma=1), id="tolerance")]
FILL = 7.0                      # what dirs and ten hold before a run
EINVAL = 1


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


def _full(shape, v=FILL):
    import torch
    t = torch.full(tuple(shape), float(v), device="cuda:0")
    torch.cuda.synchronize()
    return t


def _host(ctx, t):
    ctx.synchronize()
    return t.cpu().numpy()


def _stage(ctx, src, queue, fraction, modes, mask=None, sigma_background=0.0):
    from visfd_amd import pipeline
    s, m = _dev(src), (None if mask is None else _dev(mask))
    sal, scratch, dirs, ten = _full(src.shape), _full(src.shape), _full((3,) + src.shape), _full((6,) + src.shape)
    with ctx.options(membrane_queue=queue, **modes):
        thr = pipeline.membrane_detect(ctx, s, sal, dirs, ten, SIGMA, TV_RATIO, 4, fraction, mask=m, scratch=scratch,
                                       sigma_background=sigma_background)
    return np.float32(thr), _host(ctx, sal), _host(ctx, dirs), _host(ctx, ten)


def _cut_scores(ctx, src, fraction, modes, mask=None, sigma_background=0.0):
    """(scores as ridge_scores leaves them, the same after the old path's cut)"""
    from visfd_amd import api
    ratio = api.ratio_from_threshold(0.03)
    s, m = _dev(src), (None if mask is None else _dev(mask))
    sal, scratch, bg = _full(src.shape), _full(src.shape), None
    with ctx.options(membrane_queue=0, **modes):
        if sigma_background > 0:
            bg = _full(src.shape)
            ctx.peak_background_dev(s, bg, sigma_background, ratio, m)
        ctx.ridge_scores_dev(s, sal, scratch, SIGMA, ratio, api.DECREASING_EIVALS, m, bg)
        raw = _host(ctx, sal)
        try:
            ctx.threshold_fraction_dev(sal, fraction, m)
        except api.VisfdHipError:
            return raw, None
    return raw, _host(ctx, sal)


def _compare(ctx, src, fraction, modes, what, **kw):
    raw, cut = _cut_scores(ctx, src, fraction, modes, **kw)
    old = _stage(ctx, src, 0, fraction, modes, **kw)
    new = _stage(ctx, src, 1, fraction, modes, **kw)
    assert old[0] == new[0] or (np.isnan(old[0]) and np.isnan(new[0])), (what, old[0], new[0])
    assert_bits_equal(new[1], old[1], what + ": sal")
    assert_bits_equal(new[3], old[3], what + ": ten")
    keep = cut != 0
    assert_bits_equal(new[2][:, keep], old[2][:, keep], what + ": dirs of the survivors")
    assert not np.any(old[2][:, keep] == FILL), what + ": a survivor without a direction"
    assert_bits_equal(new[2], old[2], what + ": dirs everywhere (both runs started from the same fill)")
    return raw, cut, old


def _zero_run_volume():
    """A block of zeros with one thin plane: most scores are exact zeros, and the run of zeros holds the cut."""
    src = np.zeros((30, 6, 9), np.float32)
    src[15] = 1.0
    return src


def _tied_volume():
    """A periodic pattern: its interior repeats the same scores, so the cut falls among ties."""
    z, y, x = np.meshgrid(np.arange(12), np.arange(20), np.arange(40), indexing="ij")
    return (((x % 4) == 0) * 1.0 + ((y % 5) == 0) * 0.5).astype(np.float32)


SHAPES = [(5, 7, 70), (17, 33, 65), (3, 3, 3), (9, 300, 40)]


@pytest.mark.parametrize("modes", MODES)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_queued_stage_has_the_bits_of_the_sequence(ctx, shape, modes):
    src = volgen.membrane_volume(shape, seed=5)
    n = src.size
    for fraction in (0.05, 0.5, 0.0):   # 0: the smallest fraction, k = 0 -- the cut is the largest score
        raw, cut, old = _compare(ctx, src, fraction, modes, "%s fraction %g" % (shape, fraction))
        k = int(np.floor(np.float32(n) * np.float32(fraction)))
        assert old[0] == np.sort(raw.ravel())[::-1][k], "the threshold is the k-th largest score"
        assert np.count_nonzero(cut) >= 1


@pytest.mark.parametrize("modes", MODES)
def test_cut_inside_a_run_of_zeros(ctx, modes):
    src = _zero_run_volume()
    raw, cut, old = _compare(ctx, src, 0.7, modes, "zero run")
    assert old[0] == 0.0 and np.count_nonzero(raw == 0) > 0.3 * raw.size   # a threshold of +0 or -0
    assert np.count_nonzero(cut) == np.count_nonzero(raw) > 0              # every non-zero score survives, no zero does


@pytest.mark.parametrize("modes", MODES)
def test_ties_at_the_cut(ctx, modes):
    src = _tied_volume()
    raw, cut, old = _compare(ctx, src, 0.05, modes, "ties")
    k = int(np.floor(np.float32(src.size) * np.float32(0.05)))
    assert np.count_nonzero(raw == old[0]) > 1 and np.count_nonzero(cut) > k + 1   # more survivors than k


@pytest.mark.parametrize("modes", MODES)
def test_fraction_that_selects_no_voxel(ctx, modes):
    """k >= n: VISFD_HIP_EINVAL with the same message from both, and sal as ridge_scores wrote it."""
    from visfd_amd import api
    src = volgen.membrane_volume((6, 9, 21), seed=2)
    raw, cut = _cut_scores(ctx, src, 1.0, modes)
    assert cut is None
    said = []
    for queue in (0, 1):
        from visfd_amd import pipeline
        s = _dev(src)
        sal, scratch, dirs, ten = _full(src.shape), _full(src.shape), _full((3,) + src.shape), _full((6,) + src.shape)
        with ctx.options(membrane_queue=queue, **modes):
            with pytest.raises(api.VisfdHipError) as e:
                pipeline.membrane_detect(ctx, s, sal, dirs, ten, SIGMA, TV_RATIO, 4, 1.0, scratch=scratch)
        assert e.value.code == EINVAL
        said.append(str(e.value))
        assert_bits_equal(_host(ctx, sal), raw, "sal after the refused cut, membrane_queue=%d" % queue)
        assert np.all(_host(ctx, ten) == FILL)
    assert said[0] == said[1] and "selects no voxel" in said[0]


@pytest.mark.parametrize("modes", MODES)
def test_masked_and_background_calls_agree(ctx, modes):
    shape = (10, 21, 37)
    src = volgen.membrane_volume(shape, seed=9)
    mask = np.ones(shape, np.float32)
    mask[:, :6, :] = 0.0
    mask[3:5, :, 30:] = 0.0
    _compare(ctx, src, 0.2, modes, "masked", mask=mask)
    _compare(ctx, src, 0.2, modes, "background", sigma_background=4.0)


def test_stage_between_the_halves_of_a_blob_job(ctx):
    """A blob job begun before the stage and ended after it (as bench.py runs them): the lists of the same job with nothing
    in between, and the stage's results as without a job."""
    sig = np.array([1.2, 1.5, 1.9, 2.4, 3.0, 3.7], np.float32)   # (the job of tests/test_context_state_gpu.py)
    bsrc = _dev(volgen.blob_volume((40, 44, 48), seed=31, nblobs=60))
    src = volgen.membrane_volume((17, 33, 65), seed=5)
    modes = dict(tv_fma=1, eig_f32=1, gauss_fma=1)
    alone = _stage(ctx, src, 1, 0.05, modes)
    job = ctx.blob_dog_begin_dev(bsrc, sig, None, None, 0.02, 2.5)
    want = ctx.blob_dog_end(job)
    assert len(want[0]) + len(want[1]) > 10
    job = ctx.blob_dog_begin_dev(bsrc, sig, None, None, 0.02, 2.5)
    try:
        between = _stage(ctx, src, 1, 0.05, modes)
    except BaseException:
        ctx.blob_dog_abort(job)
        raise
    got = ctx.blob_dog_end(job)
    assert_bits_equal(volgen.sort_blobs(got[0], True), volgen.sort_blobs(want[0], True), "minima")
    assert_bits_equal(volgen.sort_blobs(got[1], False), volgen.sort_blobs(want[1], False), "maxima")
    assert between[0] == alone[0]
    for a, b, name in zip(between[1:], alone[1:], ("sal", "dirs", "ten")):
        assert_bits_equal(a, b, name + " with a blob job pending")
