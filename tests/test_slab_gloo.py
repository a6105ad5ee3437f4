"""The N>1 (Z-slab) path on CPU: world sizes 2, 3 and 4 over gloo, oracle arithmetic plugged in for the
kernels (tests/oracle_ops.py).  Slab results must equal the single-volume oracle results bit-for-bit:
halo exchange, ghost handling at true vs interior faces, the distributed exact radix select and the
blob-list merge are what is being tested -- over even and uneven splits, slabs exactly `ghost` thick and
ghosts with slack.  Also here: the host arithmetic of the blob halo depth, the planes next to a seam of
every LoG scale with that depth, and the "slab too thin" refusal being the same on every rank."""
import os
import tempfile

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import volgen
from conftest import assert_bits_equal

XY = (18, 20)
SIGMA = 1.2
TV_RATIO = 2.0
FRACTION = 0.15
BLOB_SIGMAS = np.array([1.0, 1.25, 1.55, 1.9], np.float32)


def _worker(rank, world, store_path, out_dir, nz, ghost):
    import sys
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    from oracle_ops import OracleOps
    from visfd_amd import slab
    dist.init_process_group("gloo", init_method="file://" + store_path, rank=rank, world_size=world)
    try:
        ops = OracleOps()
        full = torch.from_numpy(volgen.membrane_volume((nz,) + XY, seed=55))
        L = slab.SlabLayout(nz, rank, world, ghost=ghost)
        shape = (L.nz_local,) + XY
        src = torch.full(shape, float("nan"))          # ghosts must come from the exchange, not from here
        L.owned(src).copy_(full[L.z0:L.z1])
        sal = torch.zeros(shape)
        dirs = torch.zeros((3,) + shape)
        ten = torch.zeros((6,) + shape)
        thr = slab.membrane_detect_slab(ops, L, src, sal, dirs, ten, SIGMA, TV_RATIO, 4, FRACTION, 0.03, 2.0 ** 0.5)
        src2 = torch.full(shape, float("nan"))
        L.owned(src2).copy_(full[L.z0:L.z1])
        mins, maxs = slab.blob_detect_slab(ops, L, src2, BLOB_SIGMAS, 0.03, 0.02, -5.0, 5.0, False)
        rmins, rmaxs = slab.blob_detect_slab(ops, L, src2, BLOB_SIGMAS, 0.03, 0.02, 0.5, 0.5, True)
        np.savez(os.path.join(out_dir, "rank%d.npz" % rank), z0=L.z0, z1=L.z1, thr=np.float32(thr),
                 sal=L.owned(sal).numpy(), ten=L.owned(ten).numpy(), mins=mins, maxs=maxs, rmins=rmins, rmaxs=rmaxs)
    finally:
        dist.destroy_process_group()


# The deepest window of this stage is the blob halo (6 planes for sigma 1.9); the ridge stage needs floor(1.2 * ratio) + 1 = 4
# and the vote h_tv = 3.  (nz, world, ghost):
GEOMETRIES = [
    (30, 2, 6), (30, 3, 6),     # even splits
    (31, 2, 6), (31, 3, 6),     # uneven: nz % world != 0
    (31, 4, 6),                 # uneven, 7 or 8 planes per rank
    (47, 4, 6),                 # uneven, rem 3
    (24, 4, 6),                 # every slab exactly `ghost` thick: the middle ranks vote without an interior band
    (47, 3, 9),                 # a ghost with slack: stored planes beyond every exchanged halo stay NaN
]


@pytest.mark.parametrize("nz,world,ghost", GEOMETRIES)
def test_slab_pipeline_equals_single_volume(oracle, nz, world, ghost):
    from oracle import pyoracle as po
    from visfd_amd import slab
    assert [slab.SlabLayout(nz, r, world, ghost).z1 for r in range(world)][-1] == nz
    with tempfile.TemporaryDirectory() as tmp:
        store = os.path.join(tmp, "store")
        mp.spawn(_worker, args=(world, store, tmp, nz, ghost), nprocs=world, join=True)
        parts = [np.load(os.path.join(tmp, "rank%d.npz" % r)) for r in range(world)]
    assert [int(p["z1"]) - int(p["z0"]) for p in parts] == [nz // world + (r < nz % world) for r in range(world)]
    # single-volume oracle
    full = volgen.membrane_volume((nz,) + XY, seed=55)
    ratio = oracle.ratio_from_threshold(0.03)
    _, hess = oracle.calc_hessian(full, SIGMA, ratio, None, want_grad=False)
    sal, dirs = oracle.hessian_saliency(hess, po.ORDER_DECREASING)
    thr = oracle.threshold_fraction(sal, FRACTION)
    sigma_tv = float(np.float32(TV_RATIO) * np.float32(SIGMA))
    ten = oracle.tv_dense_stick(sal, dirs, sigma_tv, 4, 2.0 ** 0.5)
    oracle.tensor_saliency(ten, po.ORDER_DECREASING, sal)
    assert np.abs(ten).max() > 0
    for p in parts:
        assert np.float32(p["thr"]) == np.float32(thr)
        z0, z1 = int(p["z0"]), int(p["z1"])
        assert_bits_equal(p["sal"], sal[z0:z1], "post-voting saliency of planes %d..%d" % (z0, z1))
        assert_bits_equal(p["ten"], np.ascontiguousarray(np.moveaxis(ten, -1, 0))[:, z0:z1], "vote tensor")
    a, b = oracle.blob_dog(full, BLOB_SIGMAS, None, None, 0.02, ratio, -5.0, 5.0, False)
    ra, rb = oracle.blob_dog(full, BLOB_SIGMAS, None, None, 0.02, ratio, 0.5, 0.5, True)
    assert len(a) + len(b) > 4
    for p in parts:  # every rank holds the merged lists
        assert_bits_equal(volgen.sort_blobs(p["mins"], True), volgen.sort_blobs(a, True), "minima")
        assert_bits_equal(volgen.sort_blobs(p["maxs"], False), volgen.sort_blobs(b, False), "maxima")
        assert_bits_equal(volgen.sort_blobs(p["rmins"], True), volgen.sort_blobs(ra, True), "ratio minima")
        assert_bits_equal(volgen.sort_blobs(p["rmaxs"], False), volgen.sort_blobs(rb, False), "ratio maxima")


def test_layout_covers_volume():
    from visfd_amd import slab
    for nz, world, ghost in ((30, 2, 5), (31, 3, 4), (1024, 8, 12), (17, 1, 3)):
        seen = np.zeros(nz, int)
        for r in range(world):
            L = slab.SlabLayout(nz, r, world, ghost)
            seen[L.z0:L.z1] += 1
            assert L.lo == max(0, L.z0 - ghost) and L.hi == min(nz, L.z1 + ghost)
            assert L.own1 - L.own0 == L.z1 - L.z0
        assert (seen == 1).all()


# sigma_max values (float32) at which floor(ratio * sigma * (1 + delta/2)) in double precision is one less than the LoG
# kernels' float window (delta 0.02, truncate 0.03): a halo depth restated in double was one plane short for these
SEAM_SIGMAS = (1.4954885, 0.74774426, 1.8693607, 2.990977, 3.7387214)


def _plan_log_hw_f32(sigma, delta, ratio):
    """plan_log (csrc/api.hip, declared in common.hpp) restated in float32 numpy: sigma_a/b = (float)(sigma * (1 -/+ delta/2)) with the factor in
    double, the half-width floor(ratio * max(sigma_a, sigma_b)) as a float32 product."""
    s, d = float(np.float32(sigma)), float(np.float32(delta))
    sa = np.float32(s * (1.0 - 0.5 * d))
    sb = np.float32(s * (1.0 + 0.5 * d))
    return int(np.floor(np.float32(np.float32(ratio) * max(sa, sb))))


def test_blob_halo_depth_is_the_kernels_float_window():
    from visfd_amd import api
    rng = np.random.default_rng(7)
    for thr in (0.03, 0.01, 0.1):
        ratio = api.ratio_from_threshold(thr)
        for delta in (0.02, 0.05, 0.1):
            # sigmas whose float window lies just below / on / just above every integer half-width 0..24
            for h in range(0, 25):
                s0 = np.float32(h / (np.float32(ratio) * (1.0 + 0.5 * delta)))
                for k in range(-3, 4):
                    s = np.float32(s0 + np.float32(k) * np.spacing(s0)) if s0 > 0 else np.float32(1e-3 * (k + 4))
                    want = _plan_log_hw_f32(s, delta, ratio) + 1
                    assert api.blob_halo_depth([s], delta, ratio) == want, (thr, delta, float(s))
            # several scales: the widest window decides
            for _ in range(20):
                sig = np.sort(rng.uniform(0.3, 6.0, 5).astype(np.float32))
                want = max(_plan_log_hw_f32(x, delta, ratio) for x in sig) + 1
                assert api.blob_halo_depth(sig, delta, ratio) == want
    ratio = api.ratio_from_threshold(0.03)
    for s in SEAM_SIGMAS:
        assert api.blob_halo_depth([s], 0.02, ratio) == _plan_log_hw_f32(s, 0.02, ratio) + 1
    assert api.blob_halo_depth([1.4954885], 0.02, ratio) == 5


@pytest.mark.parametrize("smax", SEAM_SIGMAS)
def test_blob_halo_depth_covers_the_planes_next_to_a_seam(oracle, smax):
    """With the ghost planes exchanged as deep as the library says (the rest NaN, as if never received), the LoG of every
    scale on the local array equals the full-volume LoG bit for bit on planes [own0-1, own1+1): the owned planes and the
    one plane on each side that the 26-neighbour scan of the first/last owned plane reads."""
    from visfd_amd import api, slab
    delta, ratio = 0.02, api.ratio_from_threshold(0.03)
    sigmas = np.array([smax * 0.62, smax * 0.8, smax], np.float32)
    sigmas[-1] = np.float32(smax)
    depth = api.blob_halo_depth(sigmas, delta, ratio)
    assert depth == _plan_log_hw_f32(smax, delta, ratio) + 1
    world, ghost = 3, depth + 2
    nz = world * ghost + 2
    full = volgen.blob_volume((nz, 12, 14), seed=21)
    logs = [oracle.log(full, (s, s, s), delta, ratio)[0] for s in sigmas]
    for r in range(world):
        L = slab.SlabLayout(nz, r, world, ghost)
        loc = np.full((L.nz_local, 12, 14), np.nan, np.float32)
        a, b = max(0, L.own0 - depth), min(L.nz_local, L.own1 + depth)
        loc[a:b] = full[L.lo + a:L.lo + b]
        za, zb = max(0, L.own0 - 1), min(L.nz_local, L.own1 + 1)
        for s, want in zip(sigmas, logs):
            got = oracle.log(loc, (s, s, s), delta, ratio)[0]
            assert_bits_equal(got[za:zb], want[L.lo + za:L.lo + zb],
                              "LoG sigma %r, rank %d, planes %d..%d" % (float(s), r, L.lo + za, L.lo + zb))


@pytest.mark.parametrize("nz,world,ghost", [(25, 4, 7), (100, 8, 13), (31, 3, 11), (31, 3, 10), (24, 4, 6), (47, 4, 11),
                                            (48, 8, 6), (49, 8, 6), (17, 2, 9), (18, 2, 9)])
def test_too_thin_refusal_is_the_same_on_every_rank(nz, world, ghost):
    """A rank that accepted a geometry another refused would wait for ever in the first halo exchange."""
    from visfd_amd import slab
    verdict = []
    for r in range(world):
        try:
            slab.SlabLayout(nz, r, world, ghost)
            verdict.append(True)
        except ValueError as e:
            assert "thinner than the ghost depth" in str(e)
            verdict.append(False)
    assert len(set(verdict)) == 1, verdict
    assert verdict[0] == (nz // world >= ghost)
