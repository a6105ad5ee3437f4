"""The tolerance-mode voting kernel's square-root table (exponent 4, folded saliencies: the 17-instruction vote) against the
CPU oracle, at the smallest shapes at which the vote and the hit lists of a half can go wrong -- a sender reaches both
4 x 4 x 2 sub-patches of an 8-column half, only the left one or only the right one, and sits in one hit list or in two: a
single sender walked across sub-patch, half and tile edges, hit lists of one to four senders, chunks of 64 hits of one
kind, random fields at three window sizes, the vote forms that keep the plain table, and saliencies of very small and very
large magnitude.

Bounds and helpers are those of tests/test_tolerance_modes.py: within 1e-5 of the field's scale, and at most 0.5 % of the
significant voxels off by more than 1e-5 of their own value.  A tile is 16 x 32 receivers, a wave owns four rows of it."""
import numpy as np
import pytest

from conftest import assert_close_rel

pytestmark = pytest.mark.gpu

TOL = 1e-5
PV = 0.005
CUT = 2.0 ** 0.5
SIGMA_OF_H = {3: 2.2, 4: 3.0, 5: 3.6, 7: 5.0, 12: 8.66}   # sigma_tv whose window half-width at cutoff sqrt(2) is h
TILT = np.array([0.48, -0.6, 0.64], np.float32)            # a unit normal tilted against every axis


@pytest.fixture(scope="module")
def ctx():
    from visfd_amd import api
    c = api.Context(0)
    yield c
    c.close()


def _check(ctx, oracle, sal, dirs, h, what, exponent=4, **opts):
    sigma = SIGMA_OF_H[h]
    assert oracle.tv_tables(sigma, CUT)[0] == h
    want = oracle.tv_dense_stick(sal, dirs, sigma, exponent, CUT)
    with ctx.options(tv_fma=1, tv_poison=1, **opts):
        got = ctx.tv_dense_stick(sal, dirs, sigma, exponent, CUT)
    assert np.any(want), what
    assert_close_rel(got, want, TOL, what, pervoxel=PV)


def _random_dirs(shape, rng):
    d = rng.standard_normal(shape + (3,)).astype(np.float32)
    d /= np.linalg.norm(d, axis=-1, keepdims=True).astype(np.float32)
    return np.ascontiguousarray(d)


def _sparse_field(shape, seed, frac=0.05):
    rng = np.random.default_rng(seed)
    sal = rng.random(shape, dtype=np.float32)
    sal[rng.random(shape) > frac] = 0.0
    return sal, _random_dirs(shape, rng)


def _senders(shape, where, sal=(1.5,)):
    s = np.zeros(shape, np.float32)
    d = np.zeros(shape + (3,), np.float32)
    for i, (z, y, x) in enumerate(where):
        s[z, y, x] = sal[i % len(sal)]
        d[z, y, x] = TILT
    return s, d


@pytest.mark.parametrize("y", [17, 20])   # inside a wave's four rows (16..19), and the first row of the next wave's
def test_single_sender_sweep(ctx, oracle, y):
    """one sender at every x from 10 to 26: across a sub-patch edge (12), the half edge inside a tile (8 + h reaches back over
    it), the tile edge at 16 and the next tile's sub-patch edge at 20 -- at each position the sender reaches both sub-patches
    of a half for some waves and planes and only the left or only the right one for others"""
    shape = (8, 40, 48)
    for x in range(10, 27):
        sal, dirs = _senders(shape, [(3, y, x)])
        _check(ctx, oracle, sal, dirs, 5, "single sender at y=%d x=%d" % (y, x))


@pytest.mark.parametrize("n", [1, 2, 3, 4])
def test_odd_and_even_list_lengths(ctx, oracle, n):
    """n senders in one row: inside one half (x 1, 2, ...: every wave's lists have n entries or none) and
    straddling the half edge at x = 8 (the two sub-patches' lists split the n senders between them)"""
    shape = (8, 40, 48)
    for x0, what in ((1, "inside a half"), (8 - (n + 1) // 2, "straddling the half edge"), (16 - n // 2, "straddling the tile edge")):
        sal, dirs = _senders(shape, [(3, 18, x0 + i) for i in range(n)], sal=(1.5, 0.25, 3.0, 0.75))
        _check(ctx, oracle, sal, dirs, 5, "%d senders %s" % (n, what))


def test_full_chunks(ctx, oracle):
    """every voxel a sender: chunks of 64 tested senders that all reach both sub-patches; a slab of senders in the columns 4..7,
    which reach the sub-patch x 8..11 of the tile's second half and never the sub-patch x 12..15 (five columns away, h = 4):
    chunks of hits of the left sub-patch only; and its mirror image, the columns 16..19 against the same half"""
    shape = (6, 20, 24)
    rng = np.random.default_rng(21)
    dirs = _random_dirs(shape, rng)
    full = (rng.random(shape, dtype=np.float32) + 0.1).astype(np.float32)
    _check(ctx, oracle, full, dirs, 4, "every voxel a sender")
    for lo, what in ((4, "slab x 4..7 (left sub-patch only)"), (16, "slab x 16..19 (right sub-patch only)")):
        slab = np.zeros(shape, np.float32)
        slab[:, :, lo:lo + 4] = full[:, :, lo:lo + 4]
        _check(ctx, oracle, slab, dirs, 4, what)


@pytest.mark.parametrize("shape", [(9, 37, 50), (4, 33, 17)])
@pytest.mark.parametrize("h", [3, 7, 12])
def test_random_senders(ctx, oracle, shape, h):
    sal, dirs = _sparse_field(shape, seed=100 * h + shape[0])
    sigma = SIGMA_OF_H[h]
    assert oracle.tv_tables(sigma, CUT)[0] == h
    want = oracle.tv_dense_stick(sal, dirs, sigma, 4, CUT)
    for opts in ({}, {"tv_max_wg": 1}, {"tv_max_wg": 3, "tv_zrun": 3}):
        with ctx.options(tv_fma=1, tv_poison=1, **opts):
            got = ctx.tv_dense_stick(sal, dirs, sigma, 4, CUT)
        assert_close_rel(got, want, TOL, "random senders %s h=%d %s" % (shape, h, opts), pervoxel=PV)


def test_paths_that_keep_the_plain_table(ctx, oracle):
    """the unfolded 19-instruction vote (option tv_no_fold; one saliency that is not positive) and exponent 2 read the table
    of w, not of sqrt(w)"""
    shape = (9, 37, 50)
    sal, dirs = _sparse_field(shape, seed=5)
    _check(ctx, oracle, sal, dirs, 5, "tv_no_fold", tv_no_fold=1)
    neg = sal.copy()
    zz, yy, xx = np.nonzero(neg)
    neg[zz[7], yy[7], xx[7]] *= -1.0
    _check(ctx, oracle, neg, dirs, 5, "one negative saliency")
    _check(ctx, oracle, sal, dirs, 5, "exponent 2", exponent=2)


@pytest.mark.parametrize("scale", [1e-12, 1e12])
def test_magnitudes(ctx, oracle, scale):
    """the vote's vector g = sqrt(w) q' m' is of the order of the square root of the saliency (the product b = w q'^2 m' it
    replaces was s^(5/6)): saliencies of real tomograms span many orders of magnitude"""
    sal, dirs = _sparse_field((9, 37, 50), seed=77)
    _check(ctx, oracle, (sal * np.float32(scale)).astype(np.float32), dirs, 5, "saliency scale %g" % scale)
