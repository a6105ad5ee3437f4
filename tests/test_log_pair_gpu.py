"""The pair route of DoG / LoG (csrc/gauss_pair.hip): both Gaussians of a scale in two shared launches, bit for bit the
oracle's and the previous route's field.  Option log_pair: 0 never, 1 by the route's table, 2 wherever it applies;
log_pair_chunk puts the seams of its marches into small volumes.

Tile width of the second launch: 256 columns with the X halo, 244 / 240 / 236 / 236 outputs at H = 6 / 8 / 9 / 10, so the
shapes with nx = 376 and 401 cross a tile edge at every H (with whole 16-byte store groups, and with a ragged row end)."""
import numpy as np
import pytest

import volgen
from conftest import assert_bits_equal

pytestmark = pytest.mark.gpu

DELTA = 0.02
HS = [6, 8, 9, 10]
# (shape, options)
SHAPES = [((36, 41, 75), {}),                          # odd nx, below one x tile
          ((7, 9, 200), {}),                           # every axis but x narrower than the window
          ((20, 45, 401), {}),                         # nx crosses an x-tile edge with a ragged end
          ((6, 8, 376), {}),                           # the same with rows of whole store groups
          ((40, 50, 70), {"log_pair_chunk": 16})]      # chunk seams in z and y, the last y chunk shorter than H


@pytest.fixture(scope="module")
def ctx():
    from visfd_amd import api
    c = api.Context(0)
    yield c
    c.close()


def _log_sigma(oracle, h):
    """A sigma whose LoG half-width floor(ratio * sigma * (1 + delta / 2)) is h, from the middle of h's interval."""
    r = oracle.ratio_from_threshold(0.03)
    s = (h + 0.5) / (r * (1 + 0.5 * DELTA))
    assert int(np.floor(np.float32(r) * np.float32(s * (1 + 0.5 * DELTA)))) == h
    return s


def _ladder(oracle, h_lo, h_hi, n=12):
    """n sigmas in geometric steps from the LoG half-width h_lo to h_hi -- steps fine enough for scale-space extrema to exist in
    noise (a ladder of one sigma per half-width finds none) -- and the half-width of each, as the kernels derive it."""
    r = oracle.ratio_from_threshold(0.03)
    sig = np.geomspace((h_lo + 0.2) / (r * (1 + 0.5 * DELTA)), (h_hi + 0.8) / (r * (1 + 0.5 * DELTA)), n).astype(np.float32)
    hs = [int(np.floor(np.float32(r) * np.float32(np.float32(s) * np.float32(1 + 0.5 * DELTA)))) for s in sig]
    return sig, hs


def _dog_args(h):
    return ((h / 3.1,) * 3, (h / 2.6,) * 3, (h, h, h))


def _same_field(a, b, what):
    """Bit for bit, except that a NaN equals any NaN: which payload a sum of several NaN terms keeps depends on the operand
    order the compiler gave each add, which is not part of the contract (tests/test_gpu_parity.py: _same_float_field)."""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    na, nb = np.isnan(a), np.isnan(b)
    assert np.array_equal(na, nb), "%s: NaN patterns differ (%d vs %d NaNs)" % (what, na.sum(), nb.sum())
    assert_bits_equal(np.where(na, np.float32(0), a), np.where(nb, np.float32(0), b), what)


@pytest.mark.parametrize("h", HS)
def test_pair_route_against_the_oracle(ctx, oracle, h):
    r = oracle.ratio_from_threshold(0.03)
    s3 = (_log_sigma(oracle, h),) * 3
    for shape, opts in SHAPES:
        src = volgen.noise_volume(shape, seed=500 + h)
        with ctx.options(log_pair=2, **opts):
            got_dog = ctx.dog(src, *_dog_args(h))
            got_log = ctx.log(src, s3, DELTA, r)
        want_dog = oracle.dog(src, *_dog_args(h))
        want_log = oracle.log(src, s3, DELTA, r)
        what = "h=%d shape=%s %s" % (h, shape, opts)
        assert_bits_equal(got_dog[0], want_dog[0], "dog " + what)
        assert_bits_equal(got_log[0], want_log[0], "log " + what)
        assert_bits_equal(np.array(got_dog[1:], np.float32), np.array(want_dog[1:], np.float32), "dog A, B " + what)
        assert_bits_equal(np.array(got_log[1:], np.float32), np.array(want_log[1:], np.float32), "log A, B " + what)


def _input_classes(h):
    rng = np.random.default_rng(60 + h)
    shape = (24, 36, 72)
    n = int(np.prod(shape))
    zeros = np.full(shape, -0.0, np.float32)            # regions of -0.0 alone, next to +0.0, next to data
    zeros[:, :, 36:] = 0.0
    zeros[8:12, 10:20, 20:50] = rng.standard_normal((4, 10, 30)).astype(np.float32)
    zeros[rng.random(shape) < 0.02] = np.float32(-3.5)
    wild = (rng.standard_normal(shape) * 100 + 1000).astype(np.float32)
    wild[:, :, 20:45] = 0.0
    wild[3, 4, 5] = np.nan
    wild[20, 30, 40] = np.inf
    wild[12, 12, 12] = -np.inf
    wild[23, 35, 71] = np.nan
    wild[5:9, 20:30, 50:70] = np.float32(1e-41) * rng.integers(1, 1000, (4, 10, 20)).astype(np.float32)   # denormals
    with np.errstate(over="ignore", under="ignore"):
        mags = (rng.choice([-1.0, 1.0], n) * 10.0 ** rng.choice([-30.0, 30.0], n) * rng.uniform(1.0, 9.0, n)).astype(np.float32)
    face = np.zeros(shape, np.float32)
    face[0, 17, 33] = np.float32(7.25)
    return {"signed zeros": zeros, "non-finite and denormal": wild, "magnitudes 1e+-30": mags.reshape(shape),
            "all zero": np.zeros(shape, np.float32), "one voxel on a face": face}


@pytest.mark.parametrize("h", HS)
def test_pair_route_against_the_current_route(ctx, oracle, h):
    r = oracle.ratio_from_threshold(0.03)
    s3 = (_log_sigma(oracle, h),) * 3
    for name, src in _input_classes(h).items():
        with ctx.options(log_pair=0):
            old_dog, old_log = ctx.dog(src, *_dog_args(h))[0], ctx.log(src, s3, DELTA, r)[0]
        with ctx.options(log_pair=2):
            new_dog, new_log = ctx.dog(src, *_dog_args(h))[0], ctx.log(src, s3, DELTA, r)[0]
        _same_field(new_dog, old_dog, "dog h=%d %s" % (h, name))
        _same_field(new_log, old_log, "log h=%d %s" % (h, name))
    assert np.signbit(_input_classes(h)["signed zeros"]).any()


def _held_after_log_dev(ctx, dsrc, ddst, sigma, r, mask=None):
    ctx.synchronize()
    ctx.trim()
    ctx.log_dev(dsrc, ddst, sigma, DELTA, r, mask)
    ctx.synchronize()
    return ctx.workspace_bytes()


def test_pair_route_in_place_and_workspace(ctx, oracle):
    """log_dev with dst = src equals the out-of-place field (the first launch has read src before the second one writes).
    Workspace: the route holds the two Z-filtered volumes and the normaliser lines, nothing else -- at H = 6, too, where
    the single sweeps it replaces hold no volume at all, which shows that log_pair = 2 took the route."""
    import torch
    r = oracle.ratio_from_threshold(0.03)
    shape = (30, 37, 52)
    n = int(np.prod(shape))
    src = volgen.noise_volume(shape, seed=78)
    dev = torch.device("cuda:0")
    for h in (6, 9):
        s3 = (_log_sigma(oracle, h),) * 3
        want = oracle.log(src, s3, DELTA, r)[0]
        dsrc = torch.from_numpy(src).to(dev)
        dst = torch.empty_like(dsrc)
        with ctx.options(log_pair=2):
            held = _held_after_log_dev(ctx, dsrc, dst, s3, r)
            assert_bits_equal(dst.cpu().numpy(), want, "log_dev h=%d" % h)
            assert 2 * 4 * n <= held < 3 * 4 * n, "workspace after log_dev on the pair route: %d bytes, volume %d bytes" % (held, 4 * n)
            ctx.log_dev(dsrc, dsrc, s3, DELTA, r)
            ctx.synchronize()
            assert_bits_equal(dsrc.cpu().numpy(), want, "log_dev in place h=%d" % h)
        if h == 6:
            dsrc = torch.from_numpy(src).to(dev)
            with ctx.options(log_pair=0):
                assert _held_after_log_dev(ctx, dsrc, dst, s3, r) < 4 * n
            with ctx.options(log_pair=1):   # the table's choice, whichever it is, changes no bit
                ctx.log_dev(dsrc, dst, s3, DELTA, r)
                ctx.synchronize()
                assert_bits_equal(dst.cpu().numpy(), want, "log_dev h=6 by the table")


def test_blob_lists_on_every_setting(ctx, oracle):
    import torch
    from visfd_amd import pipeline
    r = oracle.ratio_from_threshold(0.03)
    sig, hs = _ladder(oracle, 8, 10)
    assert hs.count(8) >= 2 and hs.count(9) >= 2 and hs.count(10) >= 2 and set(hs) == {8, 9, 10}
    src = volgen.noise_volume((40, 50, 70), seed=79)
    want = oracle.blob_dog(src, sig, None, None, DELTA, r)
    assert len(want[0]) > 0 and len(want[1]) > 0
    dsrc = torch.from_numpy(src).to("cuda:0")
    for mode in (0, 1, 2):
        with ctx.options(log_pair=mode):
            got = pipeline.blob_detect(ctx, dsrc, sig)
        for g, w, asc in ((got[0], want[0], True), (got[1], want[1], False)):
            assert_bits_equal(volgen.sort_blobs(g, asc), volgen.sort_blobs(w, asc), "blob list log_pair=%d" % mode)


def test_blob_lists_of_two_z_partitions(ctx, oracle):
    """One blob run cut into two Z slabs with their ghost planes (visfd_amd.slab.SlabLayout), each run on its own on this
    GPU; the owned candidates of the two, moved to global planes, are the whole volume's lists."""
    import torch
    from visfd_amd import api, slab
    r = oracle.ratio_from_threshold(0.03)
    sig, hs = _ladder(oracle, 7, 9)
    assert hs.count(9) >= 2 and set(hs) == {7, 8, 9}
    nz = 64
    src = volgen.noise_volume((nz, 30, 40), seed=80)
    depth = api.blob_halo_depth(sig, DELTA, r)
    assert depth == 10
    want = oracle.blob_dog(src, sig, None, None, DELTA, r)
    with ctx.options(log_pair=2):
        whole = ctx.blob_dog_dev(torch.from_numpy(src).to("cuda:0"), sig, None, None, DELTA, r)
        parts = ([], [])
        for rank in (0, 1):
            L = slab.SlabLayout(nz, rank, 2, depth)
            local = torch.from_numpy(np.ascontiguousarray(src[L.lo:L.hi])).to("cuda:0")
            for k, rows in enumerate(ctx.blob_dog_dev(local, sig, None, None, DELTA, r)):
                rows = rows[(rows[:, 2] >= L.own0) & (rows[:, 2] < L.own1)].copy()
                rows[:, 2] += np.float32(L.lo)
                parts[k].append(rows)
    for k, asc in ((0, True), (1, False)):
        both = np.concatenate(parts[k], 0)
        assert len(both) > 0
        assert_bits_equal(volgen.sort_blobs(both, asc), volgen.sort_blobs(whole[k], asc), "two slabs against the whole volume")
        assert_bits_equal(volgen.sort_blobs(whole[k], asc), volgen.sort_blobs(want[k], asc), "whole volume against the oracle")


def test_requests_the_route_declines(ctx, oracle):
    """Masked, unequal half-widths, H = 12 and unnormalised requests run as before under log_pair = 2: the oracle's field,
    and (device-pointer LoG) the workspace the previous route leaves."""
    import torch
    r = oracle.ratio_from_threshold(0.03)
    shape = (30, 37, 52)
    src = volgen.noise_volume(shape, seed=81)
    mask = volgen.block_mask(shape, seed=9)
    s9, s12 = (_log_sigma(oracle, 9),) * 3, (_log_sigma(oracle, 12),) * 3
    aniso = (_log_sigma(oracle, 9), _log_sigma(oracle, 9), _log_sigma(oracle, 8))
    with ctx.options(log_pair=2):
        assert_bits_equal(ctx.log(src, s9, DELTA, r, mask)[0], oracle.log(src, s9, DELTA, r, mask)[0], "masked LoG")
        assert_bits_equal(ctx.dog(src, *_dog_args(9), mask)[0], oracle.dog(src, *_dog_args(9), mask)[0], "masked DoG")
        assert_bits_equal(ctx.log(src, aniso, DELTA, r)[0], oracle.log(src, aniso, DELTA, r)[0], "LoG, half-widths 9, 9, 8")
        sa, sb, _ = _dog_args(9)
        assert_bits_equal(ctx.dog(src, sa, sb, (9, 8, 9))[0], oracle.dog(src, sa, sb, (9, 8, 9))[0], "DoG, half-widths 9, 8, 9")
        assert_bits_equal(ctx.log(src, s12, DELTA, r)[0], oracle.log(src, s12, DELTA, r)[0], "LoG h=12")
        assert_bits_equal(ctx.gauss_hw(src, (9 / 2.6,) * 3, (9, 9, 9), None, False)[0],
                          oracle.gauss_hw(src, (9 / 2.6,) * 3, (9, 9, 9), None, False)[0], "unnormalised Gaussian h=9")
    dsrc = torch.from_numpy(src).to("cuda:0")
    dmask = torch.from_numpy(mask).to("cuda:0")
    dst = torch.empty_like(dsrc)
    for sigma, m in ((s9, dmask), (s12, None), (aniso, None)):
        held = []
        for mode in (0, 2):
            with ctx.options(log_pair=mode):
                held.append(_held_after_log_dev(ctx, dsrc, dst, sigma, r, m))
        assert held[0] == held[1], (sigma, m is not None, held)
