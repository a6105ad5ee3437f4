"""The candidate sweep of the blob scan (csrc/blob.hip: blob_candidates_kernel) at the seams of its structure, through the
whole blob_dog_dev: every list bit for bit against the oracle.

Geometry of the sweep: a wave owns 62 interior columns (x = 62 k + 1 .. 62 k + 62) by 4 interior rows, eight waves of a
workgroup are stacked in y (32 rows: y = 32 k + 1 .. 32 k + 32), a march is a chunk of at least 16 planes taken three planes
per turn of its request queue.  The sizes below hold the seams of that geometry (nx - 2, ny - 2 one below, at and one above
62 / 124, 4, 32; nz around 16, 18 and 33) and those of the tiled form it replaced (64-wide tiles, steps of four planes)."""
import numpy as np
import pytest

import volgen
from conftest import assert_bits_equal

pytestmark = pytest.mark.gpu

SIG = np.array([0.6, 0.7, 0.8], np.float32)     # fine scales: in noise about one voxel in 150 is a blob
SPIKE_SIG = np.array([0.5, 0.6, 0.72], np.float32)   # a single voxel on a zero background is a blob of the middle scale
NXY = (3, 63, 64, 65, 66, 129, 126, 127)
NY_MORE = (6, 7, 34, 35)
NZ = (3, 15, 16, 17, 33, 18, 19, 34)


@pytest.fixture(scope="module")
def ctx():
    from visfd_amd import api
    c = api.Context(0)
    yield c
    c.close()


def _dev(a):
    import torch
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


def _same_lists(got, want, what):
    for k, asc in ((0, True), (1, False)):
        assert_bits_equal(volgen.sort_blobs(got[k], asc), volgen.sort_blobs(want[k], asc), "%s, list %d" % (what, k))


def _check(ctx, oracle, src, what, mask=None, sig=SIG, **kw):
    want = oracle.blob_dog(src, sig, mask, None, 0.02, 2.5, **kw)
    got = ctx.blob_dog_dev(_dev(src), sig, _dev(mask), None, 0.02, 2.5, **kw)
    _same_lists(got, want, what)
    nz, ny, nx = src.shape
    for rows in got:   # a face voxel has no 26 neighbours inside the image: never a blob
        if len(rows):
            x, y, z = rows[:, 0], rows[:, 1], rows[:, 2]
            assert x.min() >= 1 and x.max() <= nx - 2 and y.min() >= 1 and y.max() <= ny - 2 and z.min() >= 1 and z.max() <= nz - 2, what
    return want


def _shapes():
    """Every nx, every ny and every nz of the lists above at least once, the other two sizes rotating through theirs."""
    nys = NXY + NY_MORE
    n = max(len(NXY), len(nys), len(NZ))
    out = []
    for i in range(n):
        out.append((NZ[i % len(NZ)], nys[(i * 5 + 2) % len(nys)], NXY[i % len(NXY)]))
        out.append((NZ[(i * 3 + 1) % len(NZ)], nys[i % len(nys)], NXY[(i * 3 + 4) % len(NXY)]))
    assert {s[0] for s in out} == set(NZ) and {s[1] for s in out} == set(nys) and {s[2] for s in out} == set(NXY)
    return sorted(set(out))


def _spike_field(shape, seed, density=0.01):
    """Single voxels of either sign and random height on a zero background, one voxel in a hundred, faces included: the
    isolated ones are blobs, and between them lie plateaus of equal values."""
    rng = np.random.default_rng(seed)
    src = np.zeros(shape, np.float32)
    hit = rng.random(shape) < density
    src[hit] = (rng.choice([-1.0, 1.0], int(hit.sum())) * rng.uniform(500, 1500, int(hit.sum()))).astype(np.float32)
    return src


@pytest.mark.parametrize("shape", _shapes(), ids=lambda s: "%dx%dx%d" % s)
def test_volumes_at_the_seams(ctx, oracle, shape):
    seed = 900 + shape[0] + 7 * shape[1] + 31 * shape[2]
    noise = _check(ctx, oracle, volgen.noise_volume(shape, seed=seed), "noise %s" % (shape,))
    spikes = _check(ctx, oracle, _spike_field(shape, seed + 1), "spike field %s" % (shape,), sig=SPIKE_SIG)
    if min(shape) >= 15:
        assert len(noise[0]) > 5 and len(noise[1]) > 5 and len(spikes[0]) > 20 and len(spikes[1]) > 20, shape


def _spike_volume(shape, sites, amp):
    src = np.zeros(shape, np.float32)
    for i, (z, y, x) in enumerate(sites):
        src[z, y, x] = amp * (1.0 + 0.01 * i) * (1 if i % 2 == 0 else -1)   # both signs, no two scores equal
    return src


def test_extrema_on_the_seams_and_faces(ctx, oracle):
    """Single bright and dark voxels on a zero background (a plateau of equal values everywhere else): each is a strict
    extremum of the finest scale where it has 26 neighbours, and nothing where it lies on a face."""
    shape = (35, 67, 129)
    nz, ny, nx = shape
    inner = [(z, y, x) for z in (1, 16, nz - 2) for y, x in ((1, 1), (4, 62), (5, 63), (32, 64), (33, 124), (ny - 2, nx - 2),
                                                             (33, 1), (1, 125), (36, 65))]
    inner += [(8, 20, 30), (15, 32, 62), (17, 33, 63), (18, 5, 124), (19, 4, 125), (32, 28, 93)]
    faces = [(0, 10, 10), (nz - 1, 40, 100), (9, 0, 50), (9, ny - 1, 77), (20, 20, 0), (20, 50, nx - 1), (0, 0, 0)]
    # (sites are at least three voxels apart wherever they share a neighbourhood at these scales)
    src = _spike_volume(shape, inner + faces, 1000.0)
    want = _check(ctx, oracle, src, "spikes", sig=SPIKE_SIG)
    found = {(int(r[2]), int(r[1]), int(r[0])) for rows in want for r in rows}
    assert set(inner) <= found, sorted(set(inner) - found)
    assert not (set(faces) & found)
    assert len(want[0]) > 10 and len(want[1]) > 10   # both signs


def test_plateaus_report_nothing(ctx, oracle):
    flat = np.full((17, 34, 66), 3.5, np.float32)
    want = _check(ctx, oracle, flat, "constant volume")
    assert len(want[0]) == 0 and len(want[1]) == 0
    # constant blocks: the LoG volumes are piecewise equal, with equal values across the seams of the sweep
    blocks = np.zeros((19, 35, 127), np.float32)
    blocks[:, :, 62:] = 8.0
    blocks[:, 5:, :] += 4.0
    blocks[16:, :, :] -= 2.0
    _check(ctx, oracle, blocks, "constant blocks")
    # two equal neighbours: neither is a STRICT extremum of the other
    pair = np.zeros((9, 9, 130), np.float32)
    pair[4, 4, 62] = pair[4, 4, 63] = 100.0
    pair[4, 4, 100] = -100.0
    want = _check(ctx, oracle, pair, "equal neighbours", sig=SPIKE_SIG)
    found = {(int(r[2]), int(r[1]), int(r[0])) for rows in want for r in rows}
    assert (4, 4, 100) in found and (4, 4, 62) not in found and (4, 4, 63) not in found


@pytest.mark.parametrize("shape", [(17, 35, 127), (33, 66, 65)], ids=lambda s: "%dx%dx%d" % s)
def test_masks_and_thresholds(ctx, oracle, shape):
    src = volgen.noise_volume(shape, seed=950 + shape[2])
    mask = volgen.block_mask(shape, seed=951 + shape[2])
    full = oracle.blob_dog(src, SIG, None, None, 0.02, 2.5)
    lo = float(np.median(full[0][:, 4])) if len(full[0]) else -1.0
    hi = float(np.median(full[1][:, 4])) if len(full[1]) else 1.0
    assert lo < 0 < hi
    modes = {"none": dict(), "abs": dict(minima_threshold=lo, maxima_threshold=hi, use_ratios=False),
             "ratio": dict(minima_threshold=0.5, maxima_threshold=0.5, use_ratios=True),
             "min_only": dict(minima_threshold=lo, maxima_threshold=np.inf, use_ratios=False),
             "max_only": dict(minima_threshold=-np.inf, maxima_threshold=hi, use_ratios=False)}
    for name, kw in modes.items():
        for m in (None, mask):
            _check(ctx, oracle, src, "%s, mask %s" % (name, m is not None), mask=m, **kw)
    want = oracle.blob_dog(src, SIG, None, None, 0.02, 2.5, **modes["abs"])
    assert 0 < len(want[0]) < len(full[0]) and 0 < len(want[1]) < len(full[1])


@pytest.mark.parametrize("cap", [8, 40])
def test_overflow_and_redo(ctx, oracle, cap):
    """blob_test_cap cuts the buffers of the pipelined scan to `cap` entries: the sweep's waves flush past the end of the
    candidate buffer (nothing may be written there), the scale is redone with buffers that fit."""
    shape = (34, 35, 129)
    src = volgen.noise_volume(shape, seed=960)
    want = oracle.blob_dog(src, SIG, None, None, 0.02, 2.5)
    assert len(want[0]) > 40 and len(want[1]) > 40
    with ctx.options(blob_test_cap=cap):
        got = ctx.blob_dog_dev(_dev(src), SIG, None, None, 0.02, 2.5)
    _same_lists(got, want, "cap %d" % cap)
    got = ctx.blob_dog_dev(_dev(src), SIG, None, None, 0.02, 2.5)
    _same_lists(got, want, "afterwards, without the cap")
