"""Grayscale morphology, CPU side: the sphere structuring element (host arithmetic of visfd_hip_sphere_structure) against
a numpy restatement of morphology.hpp:254-316, and the filter_mrc morphology flags' argument errors."""
import os
import subprocess

import numpy as np
import pytest

import morph_np
from conftest import GOLDEN, ROOT

CLI = os.path.join(ROOT, "visfd_amd", "cli", "filter_mrc")

F = np.float32
FLAT_RADII = [0.0, 0.5, 0.866, 1.0, float(F(np.sqrt(2.0))), 2.0, float(F(np.sqrt(5.0))), 2.5, 3.0, 4.7]
SOFT_CASES = [
    (2.0, 3.5, 50.0),     # linear rim: radius_max > radius
    (3.0, 5.0, -7.0),     # linear rim, negative bmax
    (2.5, 0.0, 1.0),      # corner rule (radius_max <= radius)
    (2.0, 0.0, 1.0),      # corner rule
    (float(F(np.sqrt(2.75))), 0.0, 1.0),   # corner rule with r_max == radius at (1, 0, 0): b = -0.0f
    (3.2, 1.0, -20.0),    # corner rule, negative bmax
    (1.0, 1.0, 3.0),      # corner rule, radius_max == radius
]


def _lib_structure(radius, radius_max=0.0, bmax=0.0):
    from visfd_amd import api
    return api.sphere_structure(radius, radius_max, bmax)


@pytest.mark.parametrize("radius", FLAT_RADII)
def test_flat_sphere_element_matches_restatement(radius):
    d, b = _lib_structure(radius)
    dw, bw = morph_np.sphere_structure(radius)
    assert np.array_equal(d, dw), radius
    assert np.array_equal(b.view(np.uint32), bw.view(np.uint32)), radius
    assert not np.any(b.view(np.uint32))   # every b is +0.0f


@pytest.mark.parametrize("radius,radius_max,bmax", SOFT_CASES)
def test_soft_sphere_element_matches_restatement(radius, radius_max, bmax):
    d, b = _lib_structure(radius, radius_max, bmax)
    dw, bw = morph_np.sphere_structure(radius, radius_max, bmax)
    assert np.array_equal(d, dw)
    assert np.array_equal(b.view(np.uint32), bw.view(np.uint32))


def test_sphere_element_known_counts_and_negative_zero():
    assert len(_lib_structure(10.0)[0]) == 4169                     # the R = 10 ball
    assert [len(_lib_structure(r)[0]) for r in (0, 1, 2)] == [1, 7, 33]
    d, b = _lib_structure(float(F(np.sqrt(2.75))), 0.0, 1.0)
    neg_zero = (b == 0) & np.signbit(b)
    assert neg_zero.any()                                              # the corner rule's b = -0.0f is kept
    d, b = _lib_structure(2.0, 3.5, 50.0)
    assert (b <= 0).all() and b.min() >= F(-50.0) and (b < 0).any()


def test_sphere_element_capacity_and_limits():
    import ctypes as C
    from visfd_amd import api
    L = api.load_library()
    n = C.c_int64()
    assert L.visfd_hip_sphere_structure(2.0, 0.0, 0.0, None, None, 0, C.byref(n)) == 0 and n.value == 33
    d = np.zeros((4, 3), np.int32)
    b = np.zeros(4, np.float32)
    rc = L.visfd_hip_sphere_structure(2.0, 0.0, 0.0, d.ctypes.data_as(api._ip), b.ctypes.data_as(api._fp), 4, C.byref(n))
    assert rc == 4 and n.value == 33                                   # VISFD_HIP_ECAPACITY, count still returned
    assert L.visfd_hip_sphere_structure(200.0, 0.0, 0.0, None, None, 0, C.byref(n)) == 1
    assert L.visfd_hip_sphere_structure(float("nan"), 0.0, 0.0, None, None, 0, C.byref(n)) == 1


@pytest.fixture(scope="module")
def cli():
    if not os.path.exists(CLI):
        from visfd_amd import build
        build.build(verbose=False)
    return CLI


SINGLE = ["-dilate", "-dilation", "-erode", "-erosion", "-open", "-opening", "-close", "-closing", "-top-hat-white",
          "-top-hat-black"]
SOFT = ["-dilate-binary-soft", "-dilation-binary-soft", "-erode-binary-soft", "-erosion-binary-soft"]


@pytest.mark.parametrize("flag", SINGLE)
@pytest.mark.parametrize("tail", [[], ["-3"], ["-w", "1"], ["abc"]])
def test_cli_morphology_flag_needs_a_number(cli, flag, tail):
    r = subprocess.run([cli, "-in", os.path.join(GOLDEN, "test_blob_detect.rec"), flag] + tail, capture_output=True,
                       text=True)
    assert r.returncode == 1, r.stderr
    assert "Error: The %s argument must be followed by a nonnegative number" % flag in r.stderr, r.stderr
    assert "Unrecognized" not in r.stderr


@pytest.mark.parametrize("flag", SOFT)
@pytest.mark.parametrize("tail", [["2", "3"], ["2"], [], ["2", "-3", "4"], ["2", "3", "-w", "1"], ["2", "3", "x"]])
def test_cli_soft_morphology_flag_needs_three_numbers(cli, flag, tail):
    r = subprocess.run([cli, "-in", os.path.join(GOLDEN, "test_blob_detect.rec"), flag] + tail, capture_output=True,
                       text=True)
    assert r.returncode == 1, r.stderr
    assert "Error: The %s argument must be followed by nonnegative numbers" % flag in r.stderr, r.stderr
    assert "Unrecognized" not in r.stderr


def test_cli_morphology_refused_under_slab(cli):
    r = subprocess.run([cli, "-in", os.path.join(GOLDEN, "test_blob_detect.rec"), "-dilate", "2", "-w", "1", "-slab", "0",
                        "1", "-"], capture_output=True, text=True)
    assert r.returncode == 1 and "-slab runs with" in r.stderr, r.stderr
