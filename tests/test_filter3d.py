"""The general 3-D filter, CPU side: the table makers (host arithmetic of visfd_hip_gengauss3d_table / _dogg3d_table /
_gengauss3d_halfwidths) against the numpy restatement tests/filter3d_np.py, bits included; the restatement itself -- the
yardstick of the GPU tests -- against golden outputs of the real reference program (golden/filter3d.npz, recorded by
golden/make_golden_filter3d.py); and the filter_mrc flags' argument errors."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import filter3d_cases as FC
import filter3d_np as FN
from conftest import GOLDEN, ROOT, assert_bits_equal

CLI = os.path.join(ROOT, "visfd_amd", "cli", "filter_mrc")
GOLD = os.path.join(GOLDEN, "filter3d.npz")

EXPONENTS = [1.0, 1.5, 2.0, 3.0, 6.0]
# (width (x, y, z), half-widths (x, y, z))
TABLE_CASES = [
    ((1.6, 1.6, 1.6), (3, 3, 3)),
    ((2.2, 1.1, 0.6), (4, 2, 1)),        # anisotropic
    ((1.5, 0.0, 2.0), (3, 0, 4)),        # a width of 0 with a half-width of 0
    ((0.0, 1.2, 1.2), (1, 2, 2)),        # a width of 0 with a window: x / 0 = inf off the centre plane
    ((3.0, 3.0, 3.0), (2, 5, 1)),        # the cut comes from the narrowest axis
]


def _api():
    from visfd_amd import api
    return api


@pytest.mark.parametrize("m", EXPONENTS)
@pytest.mark.parametrize("width,hw", TABLE_CASES)
def test_gengauss3d_table_matches_restatement(width, hw, m):
    t, A = _api().gengauss3d_table(width, m, hw)
    tw, Aw = FN.gengauss3d_table(width, m, hw)
    assert t.shape == (2 * hw[2] + 1, 2 * hw[1] + 1, 2 * hw[0] + 1)
    assert_bits_equal(t, tw, "generalised Gaussian table %s %s m=%g" % (width, hw, m))
    assert np.float32(A).view(np.uint32) == np.float32(Aw).view(np.uint32)
    assert np.float32(A) == t[hw[2], hw[1], hw[0]]


@pytest.mark.parametrize("m", EXPONENTS)
@pytest.mark.parametrize("ratio,thr", [(2.5, 0.03), (2.0, -1.0), (-1.0, 0.03), (-1.0, 0.01), (-1.0, 0.5)])
def test_gengauss3d_halfwidths_from_ratio_and_threshold(m, ratio, thr):
    for width in [(1.6, 1.6, 1.6), (2.2, 1.1, 0.6), (0.0, 4.0, 7.3)]:
        assert _api().gengauss3d_halfwidths(width, m, ratio, thr) == FN.halfwidths(width, m, ratio, thr)


def test_gengauss3d_threshold_window_known_values():
    # pow(-log(0.03), 1 / m): m = 2 -> 1.8725..., m = 6 -> 1.2325...
    assert _api().gengauss3d_halfwidths((2.0, 2.0, 2.0), 2.0, -1.0, 0.03) == (3, 3, 3)
    assert _api().gengauss3d_halfwidths((2.0, 3.0, 10.0), 6.0, -1.0, 0.03) == (2, 3, 12)
    assert _api().gengauss3d_halfwidths((2.0, 3.0, 10.0), 6.0, 1.5, 0.03) == (3, 4, 15)


@pytest.mark.parametrize("wa,wb,m,n,ratio,thr", [
    ((1.2, 1.2, 1.2), (2.0, 2.0, 2.0), 2.0, 4.0, 2.5, 0.03),
    ((1.2, 1.2, 1.2), (2.0, 2.0, 2.0), 2.0, 4.0, -1.0, 0.03),       # each window from the threshold and its own exponent
    ((1.0, 1.5, 0.8), (2.0, 1.2, 1.6), 3.0, 1.5, 2.0, 0.03),        # neither window holds the other
    ((2.0, 2.0, 2.0), (1.0, 1.0, 1.0), 6.0, 1.0, -1.0, 0.01),
    ((1.5, 0.0, 1.5), (2.5, 0.0, 1.0), 1.5, 3.0, 2.0, 0.03),        # a flat axis
])
def test_dogg3d_table_matches_restatement(wa, wb, m, n, ratio, thr):
    t, A, B = _api().dogg3d_table(wa, wb, m, n, ratio, thr)
    tw, hw, Aw, Bw = FN.dogg3d_table(wa, wb, m, n, ratio, thr)
    assert t.shape == tw.shape
    assert_bits_equal(t, tw, "DoGG table")
    assert np.float32(A).view(np.uint32) == np.float32(Aw).view(np.uint32)
    assert np.float32(B).view(np.uint32) == np.float32(Bw).view(np.uint32)


def test_table_capacity_and_refusals():
    api = _api()
    L = api.load_library()
    n = C.c_int64()
    w = api._f3((1.6, 1.6, 1.6))
    assert L.visfd_hip_gengauss3d_table(w, 3.0, api._i3((2, 3, 4)), None, 0, C.byref(n), None) == 0
    assert n.value == 5 * 7 * 9
    small = np.zeros(10, np.float32)
    rc = L.visfd_hip_gengauss3d_table(w, 3.0, api._i3((2, 3, 4)), small.ctypes.data_as(api._fp), 10, C.byref(n), None)
    assert rc == 4 and n.value == 5 * 7 * 9 and not small.any()          # VISFD_HIP_ECAPACITY, nothing written
    assert L.visfd_hip_gengauss3d_table(w, 3.0, api._i3((2, -1, 4)), None, 0, C.byref(n), None) == 1   # negative half-width
    hw = (C.c_int * 3)()
    rc = L.visfd_hip_dogg3d_table(w, w, 2.0, 4.0, 2.5, 0.03, hw, small.ctypes.data_as(api._fp), 10, C.byref(n), None, None)
    assert rc == 4 and n.value == 9 ** 3 and tuple(hw) == (4, 4, 4)
    assert L.visfd_hip_dogg3d_table(w, w, 2.0, 4.0, 2.5, 0.03, hw, None, 0, C.byref(n), None, None) == 0
    # a negative width gives a negative window
    assert L.visfd_hip_dogg3d_table(api._f3((-1.0, 1.0, 1.0)), w, 2.0, 4.0, 2.5, 0.03, hw, None, 0, C.byref(n), None, None) == 1


def _restated(name):
    """The restatement's output for a golden case, and its A (and B)."""
    src, mask = FC.inputs(name)
    p = FC.CASES[name][3]
    if p[0] == "ggauss":
        _, width, m, ratio, norm = p
        hw = FN.halfwidths(width, m, ratio)
        t, A = FN.gengauss3d_table(width, m, hw)
        return FN.apply(src, t, hw, mask, norm), (A,)
    if p[0] == "dogg":
        _, wa, wb, m, n, ratio = p
        t, hw, A, B = FN.dogg3d_table(wa, wb, m, n, ratio)
        return FN.apply(src, t, hw, mask, False), (A, B)
    _, radius, exponent, ratio, norm = p
    sg, r = _api().fluctuation_sigmas(radius, exponent, ratio, 0.03)
    return FN.local_fluctuations(src, sg, exponent, r, mask, norm), ()


@pytest.mark.parametrize("name", sorted(FC.CASES))
def test_restatement_matches_reference_golden(name):
    """Validates the yardstick: one float32 array operation per tap equals the reference program's output bit for bit,
    and the A / B the program printed (six significant digits) are the tables' centre values."""
    g = np.load(GOLD)
    out, coeff = _restated(name)
    assert_bits_equal(out, g[name + "/out"], name)
    for k, c in enumerate(coeff):
        assert float("%.6g" % c) == g[name + "/AB"][k], (name, "AB"[k], c)


@pytest.mark.parametrize("name", [n for n in sorted(FC.CASES) if FC.CASES[n][3][0] != "fluct"])
def test_library_coefficients_match_reference_golden(name):
    api = _api()
    g = np.load(GOLD)
    p = FC.CASES[name][3]
    if p[0] == "ggauss":
        _, width, m, ratio, norm = p
        coeff = (api.gengauss3d_table(width, m, api.gengauss3d_halfwidths(width, m, ratio))[1],)
    else:
        _, wa, wb, m, n, ratio = p
        coeff = api.dogg3d_table(wa, wb, m, n, ratio)[1:]
    for k, c in enumerate(coeff):
        assert float("%.6g" % c) == g[name + "/AB"][k], (name, "AB"[k], c)


def test_vote_table_shares_the_entry_loop(oracle):
    """host_tv_tables runs the general table maker's entry loop with the literal exponent 2 of TV3D::Resize, which
    compilers evaluate as a product: at wide windows that differs in the last bit from powf(r, 2), the run-time
    exponent's path, so the two tables agree only where no entry hits such an r.  The vote table stays the oracle's."""
    api = _api()
    for sigma, c in ((2.3, 2.0 ** 0.5), (19.2, 2.0 ** 0.5)):
        h, w, rhat = api.tv_tables(sigma, c)
        ho, wo, ro = oracle.tv_tables(sigma, c)
        assert h == ho
        assert_bits_equal(w, wo, "vote weights, sigma %g" % sigma)
        assert_bits_equal(rhat, ro, "unit vectors, sigma %g" % sigma)
    h, w, rhat = api.tv_tables(2.3, 2.0 ** 0.5)
    assert_bits_equal(w, api.gengauss3d_table((2.3, 2.3, 2.3), 2.0, (h, h, h))[0], "narrow window: the same table")


@pytest.fixture(scope="module")
def cli():
    if not os.path.exists(CLI):
        from visfd_amd import build
        build.build(verbose=False)
    return CLI


NEW_FLAGS = {"-ggauss": 1, "-ggauss-aniso": 3, "-dogg": 2, "-dogg-aniso": 6, "-exponent": 1, "-gauss-exponent": 1,
             "-exponents": 2, "-gdog-exponents": 2}


@pytest.mark.parametrize("flag", sorted(NEW_FLAGS))
@pytest.mark.parametrize("tail", ["short", "dash", "word"])
def test_cli_filter3d_flag_needs_its_numbers(cli, flag, tail):
    k = NEW_FLAGS[flag]
    args = ["1.5"] * (k - 1) + {"short": [], "dash": ["-w"], "word": ["abc"]}[tail]
    r = subprocess.run([cli, "-in", os.path.join(GOLDEN, "test_blob_detect.rec"), flag] + args, capture_output=True,
                       text=True)
    assert r.returncode == 1, r.stderr
    assert "Error: The %s argument must be followed by" % flag in r.stderr, r.stderr
    assert "Unrecognized" not in r.stderr


def test_cli_unknown_flag_still_rejected(cli):
    for flag in ("-median", "-doggxy", "-ggauss-iso"):
        r = subprocess.run([cli, "-in", os.path.join(GOLDEN, "test_blob_detect.rec"), flag, "2"], capture_output=True,
                           text=True)
        assert r.returncode == 1 and "Unrecognized" in r.stderr, r.stderr


def test_cli_filter3d_refused_under_slab(cli):
    r = subprocess.run([cli, "-in", os.path.join(GOLDEN, "test_blob_detect.rec"), "-ggauss", "2", "-w", "1", "-slab", "0",
                        "1", "-"], capture_output=True, text=True)
    assert r.returncode == 1 and "-slab runs with" in r.stderr, r.stderr
