"""The median filter, CPU side: the footprint of MedianSphere (host arithmetic of visfd_hip_median_footprint) against the
numpy restatement (tests/median_np.py), and the restatement against a voxel-by-voxel loop and against what the reference
program wrote for the one kind of footprint it completes (tests/golden/median.npz)."""
import ctypes as C
import sys

import numpy as np
import pytest

import median_np
from conftest import GOLDEN, assert_bits_equal, golden

F = np.float32
SQRT2 = F(np.sqrt(2.0))
RADII = [0.0, 0.5, 1.0, float(SQRT2), float(np.nextafter(SQRT2, F(0))), float(F(np.sqrt(3.0))), 2.5, 3.0, 16.0]


@pytest.mark.parametrize("radius", RADII)
def test_footprint_matches_restatement(radius):
    from visfd_amd import api
    d = api.median_footprint(radius)
    assert d.dtype == np.int32 and np.array_equal(d, median_np.footprint(radius)), radius


def test_footprint_known_counts():
    from visfd_amd import api
    assert [len(api.median_footprint(r)) for r in (1, 1.5, 2, 2.5, 3, 4, 5, 8)] == [7, 19, 33, 81, 123, 257, 515, 2109]
    # sqrt(2) as a float takes the 12 edge neighbours, the float just below it does not
    assert len(api.median_footprint(float(SQRT2))) == 19 and len(api.median_footprint(float(np.nextafter(SQRT2, F(0))))) == 7


def test_footprint_capacity_and_limits():
    from visfd_amd import api
    L = api.load_library()
    n = C.c_int64()
    assert L.visfd_hip_median_footprint(2.0, None, 0, C.byref(n)) == 0 and n.value == 33       # count only
    d = np.full((4, 3), 99, np.int32)
    rc = L.visfd_hip_median_footprint(2.0, d.ctypes.data_as(api._ip), 4, C.byref(n))
    assert rc == 4 and n.value == 33                                   # VISFD_HIP_ECAPACITY, count still returned,
    assert np.array_equal(d, median_np.footprint(2.0)[:4])             # and the first `cap` entries written
    assert L.visfd_hip_median_footprint(-1.0, None, 0, C.byref(n)) == 1     # VISFD_HIP_EINVAL
    assert L.visfd_hip_median_footprint(16.5, None, 0, C.byref(n)) == 1
    assert L.visfd_hip_median_footprint(float("nan"), None, 0, C.byref(n)) == 1
    assert L.visfd_hip_median_footprint(16.0, None, 0, C.byref(n)) == 0 and n.value == len(median_np.footprint(16.0))


def test_key_order_and_inverse():
    bits = np.array([0xffffffff, 0xffc00123, 0xff800000, 0xc1200000, 0x80400000, 0x80000000, 0x00000000, 0x00000005,
                     0x41200000, 0x7f800000, 0x7f800001, 0x7fffffff], np.uint32)   # ascending in the filter's order
    k = median_np.keys(bits.view(F))
    assert np.all(np.diff(k.astype(np.int64)) > 0)
    assert k[0] == 0 and k[-1] == 0xffffffff                          # the extreme keys
    assert np.array_equal(median_np.unkeys(k).view(np.uint32), bits)
    finite = bits.view(F)[2:10]                                        # -inf .. +inf: operator< (zeros of both signs tie there)
    assert np.all(np.diff(finite.astype(np.float64)) >= 0)


def test_restatement_matches_brute_force():
    rng = np.random.default_rng(3)
    a = rng.normal(0, 1, (6, 7, 9)).astype(F)
    a[0, 0, :4] = 0.0
    a[0, 0, 4:8] = -0.0          # -0 and +0 side by side: -0 sorts first
    a[1, :2, :] = 0.0
    a[1, 2:4, :] = -0.0
    a[2, 3, 4] = np.nan
    mask = (rng.random(a.shape) > 0.25).astype(F)
    dst0 = np.full(a.shape, 7.5, F)
    even = 0
    for radius in (1.0, 2.5):
        fp = median_np.footprint(radius)
        for m in (None, mask):
            assert_bits_equal(median_np.median_table(a, fp, mask=m, dst=dst0), median_np.median_brute(a, fp, mask=m, dst=dst0),
                              "radius %g mask=%s" % (radius, m is not None))
    no_centre = np.array([(1, 0, 0), (1, 0, 0), (0, 2, -1)], np.int32)   # a duplicate, no centre: some voxels collect nothing
    got = median_np.median_table(a, no_centre, mask=mask, dst=dst0)
    assert_bits_equal(got, median_np.median_brute(a, no_centre, mask=mask, dst=dst0), "no centre")
    zeros = (got.view(np.uint32) == 0) & (mask != 0)
    assert zeros.any() and np.array_equal(got[mask == 0], dst0[mask == 0])
    z = median_np.median_sphere(a, 1.0)
    assert np.signbit(z[z == 0]).any() and (~np.signbit(z[z == 0])).any()


def test_restatement_matches_reference_program_golden():
    """What the reference's own program wrote for the footprints it completes (radius 0 and 0.5: the centre voxel)."""
    sys.path.insert(0, GOLDEN)
    import make_golden_median as G
    g = golden("median")
    src, mask = G.volume(int(g["seed"]))
    assert_bits_equal(src, g["src"], "volume rebuilt from its seed")
    assert_bits_equal(mask, g["mask"], "mask rebuilt from its seed")
    for r in G.RADII:
        want = median_np.median_sphere(src, r, mask=mask)
        want[mask == 0] = 0.0          # the program's -mask-out default
        assert_bits_equal(want, g["out/%g" % r], "radius %g" % r)
