"""Slab entry points that one process can check on its own GPU: the slab Gaussian (visfd_hip_apply_gauss_slab_dev) on
arrays that hold planes [z_lo, z_lo + nz_local) of a taller volume, against the oracle Gaussian of the whole volume; and the
layout / "slab too thin" verdict of the library's slab handle (csrc/slab.hip) against visfd_amd.slab.SlabLayout on every
rank.  (The multi-rank runs are tests/test_00_slab_gpu.py.)"""
import numpy as np
import pytest

import volgen
from conftest import assert_bits_equal, assert_close_rel

pytestmark = pytest.mark.gpu

NZ = 64
# (sigma, halfwidth): equal half-widths 1..8 on every axis take the single-sweep (fused) route; hz = 12 and anisotropic
# windows take the three-pass route whatever gauss_3pass says
WINDOWS = [((0.6, 0.6, 0.6), (1, 1, 1)), ((1.3, 1.3, 1.3), (3, 3, 3)), ((2.2, 2.2, 2.2), (6, 6, 6)),
           ((4.4, 4.4, 4.4), (12, 12, 12)), ((1.0, 1.6, 2.4), (2, 4, 6)), ((2.5, 1.1, 4.3), (6, 3, 12))]


@pytest.fixture(scope="module")
def ctx():
    from visfd_amd import api
    c = api.Context(0)
    yield c
    c.close()


def _slabs(hz):
    """(z_lo, nz_local) touching the bottom face, the top face, both, and neither."""
    n = 2 * hz + 9
    return [(0, n), (NZ - n, n), (0, NZ), ((NZ - n) // 2, n)]


def _valid(z_lo, nzl, hz):
    """Global planes whose Z window lies inside the slab or ends at a true face of the volume."""
    z = np.arange(z_lo, z_lo + nzl)
    ok = ((z - hz >= z_lo) | (z_lo == 0)) & ((z + hz < z_lo + nzl) | (z_lo + nzl == NZ))
    return z[ok]


@pytest.mark.parametrize("nx", [24, 21])
@pytest.mark.parametrize("three_pass", [0, 1])
def test_gauss_slab_dev_with_z_offset_equals_whole_volume(ctx, oracle, nx, three_pass):
    import torch
    full = volgen.noise_volume((NZ, 18, nx), seed=17)
    full[NZ // 2:] += 400.0   # a step inside the volume: a slab's offset into the normaliser shows in every plane
    dev = torch.device("cuda", 0)
    with ctx.options(gauss_3pass=three_pass, gauss_fma=0):
        for sigma, hw in WINDOWS:
            for normalize in (1, 0):
                want, A_want = oracle.gauss_hw(full, sigma, hw, None, bool(normalize))
                for z_lo, nzl in _slabs(hw[2]):
                    src = torch.from_numpy(np.ascontiguousarray(full[z_lo:z_lo + nzl])).to(dev)
                    dst = torch.full_like(src, float("nan"))
                    A = ctx.gauss_slab_dev(src, dst, z_lo, NZ, sigma, hw, normalize)
                    ctx.synchronize()
                    z = _valid(z_lo, nzl, hw[2])
                    assert len(z) >= 9
                    what = "slab gauss sigma %s hw %s normalize %d slab [%d, %d) nx %d 3pass %d" % (
                        sigma, hw, normalize, z_lo, z_lo + nzl, nx, three_pass)
                    assert_bits_equal(dst.cpu().numpy()[z - z_lo], want[z], what)
                    assert np.float32(A) == np.float32(A_want), what


def test_gauss_slab_dev_tolerance_mode(ctx, oracle):
    import torch
    full = volgen.noise_volume((NZ, 18, 24), seed=18)
    dev = torch.device("cuda", 0)
    with ctx.options(gauss_fma=1):
        for sigma, hw in WINDOWS:
            for normalize in (1, 0):
                want, _ = oracle.gauss_hw(full, sigma, hw, None, bool(normalize))
                for z_lo, nzl in _slabs(hw[2]):
                    src = torch.from_numpy(np.ascontiguousarray(full[z_lo:z_lo + nzl])).to(dev)
                    dst = torch.empty_like(src)
                    ctx.gauss_slab_dev(src, dst, z_lo, NZ, sigma, hw, normalize)
                    ctx.synchronize()
                    z = _valid(z_lo, nzl, hw[2])
                    assert_close_rel(dst.cpu().numpy()[z - z_lo], want[z], 1e-5,
                                     "fma slab gauss sigma %s hw %s normalize %d slab [%d, %d)" % (sigma, hw, normalize, z_lo,
                                                                                                 z_lo + nzl))


def test_gauss_slab_dev_refuses_a_slab_outside_the_volume(ctx):
    import torch
    from visfd_amd import api
    src = torch.zeros((10, 8, 8), device="cuda:0")
    dst = torch.empty_like(src)
    for z_lo, nz_global in ((-1, 64), (55, 64), (0, 9)):
        with pytest.raises(api.VisfdHipError, match="outside the volume"):
            ctx.gauss_slab_dev(src, dst, z_lo, nz_global, (1.0, 1.0, 1.0), (2, 2, 2), 1)
    ctx.gauss_slab_dev(src, dst, 54, 64, (1.0, 1.0, 1.0), (2, 2, 2), 1)   # the last valid offset
    ctx.synchronize()


def test_slab_handle_layout_and_refusals_agree_with_slablayout(ctx):
    """The handle's layout (visfd_hip_slab_layout) equals SlabLayout's on every rank, and both refuse the same geometries on
    every rank.  Creating a handle with the callback transport does not communicate, so all ranks of a world can be made
    here, one after the other."""
    from visfd_amd import api, slab
    geoms = [(nz, world, ghost) for world in (2, 3, 4, 5, 8) for nz in (world * 6 - 1, world * 6, world * 6 + 1, 31, 47, 100)
             for ghost in (0, 3, 6, 7, 13) if nz >= world]
    geoms += [(25, 4, 7), (100, 8, 13), (31, 3, 11), (31, 3, 10)]
    refused_any = accepted_any = 0
    for nz, world, ghost in geoms:
        verdict = []
        for r in range(world):
            try:
                L = slab.SlabLayout(nz, r, world, ghost)
            except ValueError:
                L = None
            try:
                h = api.Slab(ctx, r, world, nz, ghost, transport="torch")
            except api.VisfdHipError as e:
                assert "thinner than the ghost depth" in str(e)
                h = None
            assert (L is None) == (h is None), (nz, world, ghost, r)
            if h is not None:
                assert (h.z0, h.z1, h.lo, h.hi, h.own0, h.own1, h.nz_local) == (L.z0, L.z1, L.lo, L.hi, L.own0, L.own1, L.nz_local), \
                    (nz, world, ghost, r)
                h.close()
            verdict.append(h is not None)
        assert len(set(verdict)) == 1, (nz, world, ghost, verdict)
        refused_any += not verdict[0]
        accepted_any += verdict[0]
    assert refused_any >= 5 and accepted_any >= 20
