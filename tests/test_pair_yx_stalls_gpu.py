"""pair_yx_kernel (csrc/gauss_pair.hip) after its X pass was given a raised issue priority and a divide-by-one test per filter:
one LoG scale through log_pair = 2 at EVERY half-width H = 6..10, bit for bit against the oracle, at the row ends, tile ends,
chunk seams and alignments at which the X tasks take another path, and with normalisers that are exactly 1 in the interior
for both filters, for neither, and for one of the two (the case in which only one filter divides).

Geometry (YxCfg): 256 columns per workgroup with the X halo; TX = 256 + 4 - 4 * ceil((2H + 4) / 4) output columns per tile; a
task is four adjacent outputs; a turn is 2H + 1 rows."""
import numpy as np
import pytest

import volgen
from conftest import assert_bits_equal

pytestmark = pytest.mark.gpu

DELTA = 0.02
HS = [6, 7, 8, 9, 10]
KINDS = ("ones", "neither", "mixed")


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


def _interior_norm(sigma, h):
    """(Dx*Dy)*Dz of a voxel away from the faces, for the two Gaussians of the LoG at sigma: the float sum of the taps in tap
    order on each axis, as the kernels form it (tests/test_log_pair_yx_gpu.py)."""
    from visfd_amd import api
    out = []
    s32 = float(np.float32(sigma))
    for s in (np.float32(s32 * (1.0 - 0.5 * DELTA)), np.float32(s32 * (1.0 + 0.5 * DELTA))):
        acc = np.float32(0)
        for t in api.gauss_taps(float(s), h):
            acc = np.float32(acc + np.float32(t * np.float32(1)))
        out.append(np.float32(np.float32(acc * acc) * acc))
    return out


@pytest.fixture(scope="module")
def sigmas(ratio):
    """{h: {kind: sigma}}: for every half-width the first sigma of each kind on a fixed grid over h's interval.  Which kinds
    exist depends on the taps' rounding; on this grid every h has all three."""
    out = {}
    for h in HS:
        kinds = {}
        for s in np.linspace((h + 0.05) / (ratio * (1 + 0.5 * DELTA)), (h + 0.95) / (ratio * (1 + 0.5 * DELTA)), 200):
            s = float(s)
            if _halfwidth(ratio, s) != h:
                continue
            n_one = sum(1 for d in _interior_norm(s, h) if d == np.float32(1))
            kinds.setdefault({2: "ones", 1: "mixed", 0: "neither"}[n_one], s)
        out[h] = kinds
    return out


def test_every_kind_of_normaliser_is_covered(sigmas):
    for h in HS:
        assert set(sigmas[h]) == set(KINDS), (h, sigmas[h])


def _check_host(ctx, oracle, ratio, src, sigma, what, **opts):
    s3 = (sigma,) * 3
    with ctx.options(log_pair=2, **opts):
        new = ctx.log(src, s3, DELTA, ratio)[0]
    assert_bits_equal(new, oracle.log(src, s3, DELTA, ratio)[0], what)


@pytest.mark.parametrize("h", HS)
def test_row_ends_tile_ends_and_short_volumes(ctx, oracle, ratio, sigmas, h):
    """nx: below a window, around one wave, around one tile (the second tile then has three idle waves), and 13 columns into the
    second tile (a partial quad at the row's end); ny in {3, 2H, 2H+1} and nz in {1, 3, 2H+1} rotate through; so do the kinds
    of sigma this half-width has."""
    tx = _tx(h)
    kinds = sorted(sigmas[h])
    nxs = (h + 1, 63, 64, 65, tx - 1, tx, tx + 1, tx + 4 * 3 + 1)
    nys, nzs = (3, 2 * h, 2 * h + 1), (1, 3, 2 * h + 1)
    for i, nx in enumerate(nxs):
        ny, nz, kind = nys[i % 3], nzs[(i // 3 + i) % 3], kinds[(i + h) % len(kinds)]
        src = volgen.noise_volume((nz, ny, nx), seed=1000 + i)
        _check_host(ctx, oracle, ratio, src, sigmas[h][kind], "h=%d %s %dx%dx%d" % (h, kind, nz, ny, nx))


@pytest.mark.parametrize("h", HS)
def test_interior_of_every_kind(ctx, oracle, ratio, sigmas, h):
    """A volume with voxels H away from every face (there the interior normalisers apply and a filter whose normaliser is 1
    does not divide), nx one quad and one column into the second tile."""
    for kind, sigma in sorted(sigmas[h].items()):
        src = volgen.noise_volume((2 * h + 3, 2 * h + 8, _tx(h) + 5), seed=1100 + h)
        _check_host(ctx, oracle, ratio, src, sigma, "h=%d %s interior" % (h, kind))


@pytest.mark.parametrize("h", HS)
def test_two_y_chunks(ctx, oracle, ratio, sigmas, h):
    kinds = sorted(sigmas[h])
    for i, chunk in enumerate((8, 16)):
        for ny in (chunk + 1, 2 * chunk - 3, 2 * chunk):
            src = volgen.noise_volume((3, ny, 65), seed=1200 + ny)
            _check_host(ctx, oracle, ratio, src, sigmas[h][kinds[i % len(kinds)]], "h=%d chunk=%d ny=%d" % (h, chunk, ny),
                        log_pair_chunk=chunk)


@pytest.mark.parametrize("h", HS)
def test_in_place_and_unaligned_destinations(ctx, oracle, ratio, sigmas, h):
    """log_dev on device tensors: dst == src; a dst one, two and three floats off a 16-byte boundary with nx % 4 == 0 (the
    vector store must not be taken) and with nx % 4 != 0."""
    import torch
    kinds = sorted(sigmas[h])
    for i, nx in enumerate((_tx(h) + 8, 67, 2 * h + 6)):
        sigma = sigmas[h][kinds[i % len(kinds)]]
        shape = (3, 2 * h + 2, nx)
        src = volgen.noise_volume(shape, seed=1300 + nx)
        want = oracle.log(src, (sigma,) * 3, DELTA, ratio)[0]
        n = src.size
        dsrc = torch.from_numpy(src).to("cuda:0")
        with ctx.options(log_pair=2):
            for off in (0, 1, 2, 3):
                buf = torch.zeros(n + 8, device="cuda:0")
                dst = buf[off:off + n].view(shape)
                assert dst.data_ptr() % 16 == 4 * off
                torch.cuda.synchronize()   # the context has a stream of its own: torch's fills first, then the call, then the reads
                ctx.log_dev(dsrc, dst, (sigma,) * 3, DELTA, ratio)
                ctx.synchronize()
                assert_bits_equal(dst.cpu().numpy(), want, "h=%d nx=%d dst %d floats off" % (h, nx, off))
                assert float(buf[:off].abs().sum()) == 0.0 and float(buf[off + n:].abs().sum()) == 0.0, "wrote outside dst"
            both = dsrc.clone()
            torch.cuda.synchronize()
            ctx.log_dev(both, both, (sigma,) * 3, DELTA, ratio)
            ctx.synchronize()
            assert_bits_equal(both.cpu().numpy(), want, "h=%d nx=%d in place" % (h, nx))
