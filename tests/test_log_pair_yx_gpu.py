"""The second launch of the pair route (csrc/gauss_pair.hip: pair_yx_kernel) at the seams of its structure: the rounds in which a
turn's X tasks are dealt, the turn itself, y-chunk seams, x tiles whose last waves have nothing to march and whose tasks are
dealt over fewer quads, and the two ways it treats the normaliser (skipped where it is 1, divided by elsewhere).  Every case compares log_pair = 2 bit for bit with the oracle and with the route it replaces
(log_pair = 0).

Geometry (YxCfg): 256 columns per workgroup with the X halo, TX = 244 / 240 / 236 outputs at H = 6 / 7 / 10; a turn is 2H + 1
rows, whose X tasks are dealt in rounds of 256, four to five rows each."""
import numpy as np
import pytest

import volgen
from conftest import assert_bits_equal

pytestmark = pytest.mark.gpu

DELTA = 0.02
HS = [6, 7, 10]
ROUND_ROWS = (4, 5)   # rows a round of 256 tasks spans (61, 60 or 59 tasks per row)


def _tx(h):
    return 256 + 4 - 4 * ((2 * h + 4 + 3) // 4)


@pytest.fixture(scope="module")
def ctx():
    from visfd_amd import api
    c = api.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def ratio(oracle):
    return oracle.ratio_from_threshold(0.03)


def _halfwidth(ratio, sigma):
    """The LoG half-width as api.hip's log plan derives it: floor(ratio * max(sa, sb)), the sigmas rounded to float first."""
    sb = np.float32(float(np.float32(sigma)) * (1.0 + 0.5 * DELTA))
    return int(np.floor(np.float32(ratio) * sb))


def _log_sigma(ratio, h):
    s = (h + 0.5) / (ratio * (1 + 0.5 * DELTA))
    assert _halfwidth(ratio, s) == h
    return s


def _same_field(a, b, what):
    """Bit for bit, except that a NaN equals any NaN: which payload a sum of several NaN terms keeps depends on the operand
    order the compiler gave each add, which is not part of the contract (tests/test_gpu_parity.py: _same_float_field)."""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    na, nb = np.isnan(a), np.isnan(b)
    assert np.array_equal(na, nb), "%s: NaN patterns differ (%d vs %d NaNs)" % (what, na.sum(), nb.sum())
    assert_bits_equal(np.where(na, np.float32(0), a), np.where(nb, np.float32(0), b), what)


def _check(ctx, oracle, ratio, src, sigma, what, **opts):
    s3 = (sigma,) * 3
    with ctx.options(log_pair=2, **opts):
        new = ctx.log(src, s3, DELTA, ratio)[0]
    with ctx.options(log_pair=0):
        old = ctx.log(src, s3, DELTA, ratio)[0]
    assert_bits_equal(new, oracle.log(src, s3, DELTA, ratio)[0], what + ": against the oracle")
    _same_field(new, old, what + ": against log_pair = 0")


@pytest.mark.parametrize("h", HS)
def test_rows_around_the_task_rounds_and_the_turn(ctx, oracle, ratio, h):
    sigma = _log_sigma(ratio, h)
    g_lo, g_hi = ROUND_ROWS
    for ny in sorted({1, g_lo - 1, g_lo, g_hi, g_hi + 1, 2 * h, 2 * h + 1, 2 * (2 * h + 1) + 3}):
        src = volgen.noise_volume((5, ny, 45), seed=700 + ny)
        _check(ctx, oracle, ratio, src, sigma, "h=%d ny=%d" % (h, ny))


@pytest.mark.parametrize("h", HS)
def test_y_chunk_seams_inside_a_round(ctx, oracle, ratio, h):
    """log_pair_chunk cuts y (and z) into marches of that length: seams inside a round's rows and inside a turn, last chunks of
    3 rows (47 = 2 * 22 + 3), of 2 (47 = 5 * 9 + 2) and of 1 (47 = 23 * 2 + 1)."""
    sigma = _log_sigma(ratio, h)
    src = volgen.noise_volume((6, 47, 50), seed=720 + h)
    for chunk in (22, 9, 2):
        _check(ctx, oracle, ratio, src, sigma, "h=%d chunk=%d" % (h, chunk), log_pair_chunk=chunk)


@pytest.mark.parametrize("h", HS)
def test_row_ends_and_waves_with_nothing_to_march(ctx, oracle, ratio, h):
    """nx below one quad; one whole tile; one column, 10 and 70 columns into the second tile, whose last three and last two
    waves lie outside the image."""
    sigma = _log_sigma(ratio, h)
    tx = _tx(h)
    assert tx == {6: 244, 7: 240, 10: 236}[h]
    for nx in (3, tx, tx + 1, tx + 10, tx + 70):
        src = volgen.noise_volume((4, 9, nx), seed=740 + h)
        _check(ctx, oracle, ratio, src, sigma, "h=%d nx=%d" % (h, nx))


def _interior_norm(sigma, h):
    """(Dx*Dy)*Dz of a voxel away from the faces, for the two Gaussians of the LoG at sigma: the float sum of the taps in tap
    order on each axis, as the kernels form it."""
    from visfd_amd import api
    out = []
    s32 = float(np.float32(sigma))   # (the library takes sigma as a float)
    for s in (np.float32(s32 * (1.0 - 0.5 * DELTA)), np.float32(s32 * (1.0 + 0.5 * DELTA))):
        acc = np.float32(0)
        for t in api.gauss_taps(float(s), h):
            acc = np.float32(acc + np.float32(t * np.float32(1)))
        out.append(np.float32(np.float32(acc * acc) * acc))
    return out


def _sigma_of_kind(ratio, h, kind):
    """A sigma of half-width h whose two interior normalisers are both exactly 1 ("ones"), both not ("neither"), or one of
    each ("mixed"); the first such on a fixed grid over h's interval."""
    for s in np.linspace((h + 0.05) / (ratio * (1 + 0.5 * DELTA)), (h + 0.95) / (ratio * (1 + 0.5 * DELTA)), 200):
        s = float(s)
        if _halfwidth(ratio, s) != h:
            continue
        n_one = sum(1 for d in _interior_norm(s, h) if d == np.float32(1))
        if {"ones": 2, "mixed": 1, "neither": 0}[kind] == n_one:
            return s
    raise AssertionError("no sigma of kind %r at h=%d" % (kind, h))


@pytest.mark.parametrize("kind", ["ones", "neither", "mixed"])
def test_both_division_paths(ctx, oracle, ratio, kind):
    h = 8
    sigma = _sigma_of_kind(ratio, h, kind)
    da, db = _interior_norm(sigma, h)
    assert {"ones": da == 1 and db == 1, "neither": da != 1 and db != 1, "mixed": (da == 1) != (db == 1)}[kind], (da, db)
    faces = volgen.noise_volume((2 * h, 21, 40), seed=760)         # no voxel is H away from both z faces
    inner = volgen.noise_volume((2 * h + 6, 2 * h + 9, 2 * h + 40), seed=761)
    _check(ctx, oracle, ratio, faces, sigma, "%s, faces" % kind)
    _check(ctx, oracle, ratio, inner, sigma, "%s, interior" % kind)


def test_numerators_outside_the_guard(ctx, oracle, ratio):
    """The numerators a reciprocal-based division (csrc/exact_div.hpp, as the single sweeps of log_pair = 0 use it) has to turn
    away: magnitudes near 1e-30 and 1e+30 (the guard's bounds are 2^-100 and 2^100), planes of exact zeros, non-finite voxels
    and denormals, at a sigma whose normalisers are not 1, in a volume with an interior.  The two routes give the same fields."""
    h = 8
    sigma = _sigma_of_kind(ratio, h, "neither")
    shape = (2 * h + 6, 2 * h + 9, 2 * h + 40)
    noise = volgen.noise_volume(shape, seed=770)
    with np.errstate(over="ignore", under="ignore"):
        tiny, huge = (noise * np.float32(1e-30)).astype(np.float32), (noise * np.float32(1e+30)).astype(np.float32)
    planes = noise.copy()
    planes[:, :, 20:30] = 0.0
    planes[:, 10:14, :] = -0.0
    planes[3:7] = 0.0
    wild = noise.copy()
    wild[2, 3, 4] = np.nan
    wild[11, 12, 30] = np.inf
    wild[12, 20, 50] = -np.inf
    wild[shape[0] - 1, shape[1] - 1, shape[2] - 1] = np.nan
    rng = np.random.default_rng(771)
    wild[14:18, 5:15, 10:30] = np.float32(1e-41) * rng.integers(1, 1000, (4, 10, 20)).astype(np.float32)   # denormals
    s3 = (sigma,) * 3
    for name, src in (("1e-30", tiny), ("1e+30", huge), ("zero planes", planes), ("non-finite and denormal", wild)):
        with ctx.options(log_pair=0):
            old = ctx.log(src, s3, DELTA, ratio)[0]
        with ctx.options(log_pair=2):
            new = ctx.log(src, s3, DELTA, ratio)[0]
        _same_field(new, old, name)
    for name, src in (("1e-30", tiny), ("zero planes", planes)):   # (finite fields: the oracle's bits as well)
        with ctx.options(log_pair=2):
            assert_bits_equal(ctx.log(src, s3, DELTA, ratio)[0], oracle.log(src, s3, DELTA, ratio)[0], name + ": against the oracle")


def _ladder(ratio, h_lo, h_hi, n=12):
    """n sigmas in geometric steps from the LoG half-width h_lo to h_hi, and the half-width of each, as the kernels derive it
    (tests/test_log_pair_gpu.py: _ladder)."""
    sig = np.geomspace((h_lo + 0.2) / (ratio * (1 + 0.5 * DELTA)), (h_hi + 0.8) / (ratio * (1 + 0.5 * DELTA)), n).astype(np.float32)
    hs = [int(np.floor(np.float32(ratio) * np.float32(np.float32(s) * np.float32(1 + 0.5 * DELTA)))) for s in sig]
    return sig, hs


def test_blob_lists_over_every_half_width(ctx, ratio):
    import torch
    from visfd_amd import pipeline
    sig, hs = _ladder(ratio, 6, 10)
    assert set(hs) == {6, 7, 8, 9, 10}
    src = volgen.noise_volume((48, 56, 300), seed=780)
    dsrc = torch.from_numpy(src).to("cuda:0")
    lists = {}
    for mode in (0, 1, 2):
        with ctx.options(log_pair=mode):
            got = pipeline.blob_detect(ctx, dsrc, sig)
        lists[mode] = (volgen.sort_blobs(got[0], True), volgen.sort_blobs(got[1], False))
    assert len(lists[0][0]) > 0 and len(lists[0][1]) > 0
    for mode in (1, 2):
        for k in (0, 1):
            assert_bits_equal(lists[mode][k], lists[0][k], "blob list %d, log_pair=%d against 0" % (k, mode))
