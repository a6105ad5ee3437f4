"""Intensity maps and image statistics without a GPU: the numpy restatement (tests/intensity_np.py) against what the
reference program wrote (tests/golden/intensity.npz), csrc/intensity.hpp compiled for the host against the restatement,
the exact sum of visfd_hip_image_stats_host against math.fsum, and filter_mrc's parser.

Equality is bit for bit everywhere but for -thresh-gauss, which gets one float ulp: its only operation outside IEEE's
correctly rounded set is a double exp, whose last bit may differ between libraries, and a last-bit difference of a double
moves its rounding to float by at most one ulp."""
import math
import os
import struct
import subprocess

import numpy as np
import pytest

import intensity_cases as ic
import intensity_np as inp
from conftest import ROOT, assert_bits_equal, golden

CLI = os.path.join(ROOT, "visfd_amd", "cli", "filter_mrc")


@pytest.fixture(scope="module")
def api():
    from visfd_amd import api as a
    a.load_library()
    return a


@pytest.fixture(scope="module")
def gold():
    return golden("intensity")


@pytest.fixture(scope="module")
def inputs():
    return ic.inputs()


def assert_within_one_ulp(got, want, what):
    d = inp.ulp_distance(got, want)
    print("%s: %d of %d values differ by one ulp" % (what, int((d > 0).sum()), d.size))
    assert d.max() <= 1, "%s: %d ulps apart" % (what, int(d.max()))


def test_golden_inputs_are_the_generated_ones(gold, inputs):
    for name in ("dyadic", "dyadic_sel", "wide"):
        assert_bits_equal(gold["in/" + name], inputs[name][0], name)
        if inputs[name][1] is not None:
            assert_bits_equal(gold["mask/" + name], inputs[name][1], name + " mask")


@pytest.mark.parametrize("case", ic.CASES, ids=[c[0] for c in ic.CASES])
def test_restatement_equals_reference(case, gold, inputs):
    name, input_name, use_mask, flags = case
    vol, mask = inputs[input_name]
    filtered = gold["filtered/" + name] if "filtered/" + name in gold.files else vol
    got = inp.tail(vol, filtered, mask if use_mask else None, flags)
    if name in ic.GAUSS_ULP_CASES:
        assert_within_one_ulp(got, gold["out/" + name], name)
    else:
        assert_bits_equal(got, gold["out/" + name], name)


def test_reference_behaviours_the_goldens_pin(gold):
    """The threshold family maps the input image: a filter or an inversion before it leaves no trace; -rescale keeps both."""
    assert_bits_equal(gold["out/gauss_thresh2"], gold["out/thresh2"], "-gauss 2 -thresh2 == -thresh2")
    assert_bits_equal(gold["out/invert_thresh2"], gold["out/thresh2"], "-invert -thresh2 == -thresh2")
    assert not np.array_equal(gold["out/inv_rescale"], gold["out/rescale"])
    assert not np.array_equal(gold["out/gauss_rescale"], gold["out/rescale"])
    # clipping is Threshold2 with the thresholds as outputs: min(max(I, a), b) has other bits at some voxels
    lo, hi = np.float32(-100.125), np.float32(75.5)
    assert not np.array_equal(gold["out/clip"].view(np.uint32), np.clip(gold["in/dyadic"], lo, hi).view(np.uint32))
    # mask fill comes before -rescale-min-max: voxels outside the mask hold the rescaled image of the fill value
    out, mask = gold["out/mask_rescale_min_max"], gold["mask/dyadic"]
    sel = gold["in/dyadic"][mask != 0]
    want = inp.rescale01(np.float32(300.0), 1.0, 0.0, sel.min(), sel.max())
    assert np.all(out[mask == 0] == want)


def shim(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("shim_intensity") / "shim_intensity_check")
    from visfd_amd import api as a
    libdir = os.path.dirname(a.LIB_PATH)
    cmd = ["g++", "-std=c++11", "-O2", "-ffp-contract=off", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
           os.path.join(ROOT, "tests", "shim_intensity_check.cpp"), "-L" + libdir, "-lvisfd_hip", "-Wl,-rpath," + libdir,
           "-Wl,-rpath,/opt/rocm/lib", "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return exe


@pytest.fixture(scope="module")
def shim_exe(tmp_path_factory):
    return shim(tmp_path_factory)


def run_shim(exe, mode, tmp_path, p, src, out, mask):
    nz, ny, nx = out.shape
    fin, fout = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(fin, "wb") as f:
        f.write(struct.pack("<4i", nx, ny, nz, int(mask is not None)))
        f.write(bytes(p))
        f.write(src.tobytes())
        f.write(out.tobytes())
        if mask is not None:
            f.write(mask.tobytes())
    r = subprocess.run([exe, mode, fin, fout], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    raw = open(fout, "rb").read()
    return np.frombuffer(raw[:4 * out.size], np.float32).reshape(out.shape), raw[4 * out.size:]


@pytest.mark.parametrize("name", sorted(ic.MAP_CASES))
@pytest.mark.parametrize("with_mask", [False, True])
def test_host_header_equals_restatement(name, with_mask, api, shim_exe, tmp_path):
    """csrc/intensity.hpp as g++ compiles it: through the reference names of include/visfd_hip.hpp (the shim) and through
    visfd_hip_intensity_map_host."""
    kw = ic.MAP_CASES[name]
    src, out, mask = ic.map_volume((5, 6, 7))
    mask = mask if with_mask else None
    want = inp.apply(out, src, mask, **kw)
    p = ic.map_params(api, kw)
    got, _ = run_shim(shim_exe, "host", tmp_path, p, src, out, mask)
    lib = out.copy()
    api.intensity_map_host(p, lib, src, mask)
    for g, what in ((got, "shim"), (lib, "library")):
        if name in ic.MAP_GAUSS_CASES:
            assert_within_one_ulp(g, want, name + " " + what)
        else:
            assert_bits_equal(g, want, name + " " + what)


def fsum(values):
    return math.fsum(float(x) for x in np.asarray(values).reshape(-1))


@pytest.mark.parametrize("name", sorted(ic.stats_inputs()))
def test_host_stats_sum_is_exact(name, api):
    v = ic.stats_inputs()[name]
    st = api.image_stats_host(v)
    assert st["sum"] == fsum(v) and st["count"] == v.size and st["n_nonfinite"] == 0
    assert st["min"] == v.min() and st["max"] == v.max()
    rng = np.random.default_rng(5)
    mask = (rng.random(v.size) < 0.5).astype(np.float32)
    st = api.image_stats_host(v, mask)
    assert st["sum"] == fsum(v[mask != 0]) and st["count"] == int((mask != 0).sum())
    # the sum does not depend on the order of the values
    assert api.image_stats_host(np.ascontiguousarray(v[rng.permutation(v.size)]))["sum"] == fsum(v)


def test_host_stats_edges(api, inputs):
    v = np.array([1.5, 2.0, -7.0], np.float32)
    st = api.image_stats_host(v, np.zeros(3, np.float32))   # everything masked
    assert st["count"] == 0 and st["sum"] == 0.0 and st["order_free"] == 1 and st["n_nonfinite"] == 0
    st = api.image_stats_host(np.array([1.0, np.nan, np.inf, -np.inf, 2.0], np.float32))
    assert st["count"] == 5 and st["n_nonfinite"] == 3
    st = api.image_stats_host(np.array([1.0, np.nan], np.float32), np.array([1.0, 0.0], np.float32))
    assert st["count"] == 1 and st["n_nonfinite"] == 0 and st["sum"] == 1.0
    zeros = api.image_stats_host(np.array([0.0, -0.0], np.float32))
    assert zeros["sum"] == 0.0 and zeros["order_free"] == 1
    # order_free: proven for the fixtures and the dyadic volume, not for the wide one
    for name, (vol, mask) in inputs.items():
        st = api.image_stats_host(vol, mask)
        sel = vol[mask != 0] if mask is not None else vol
        assert st["sum"] == fsum(sel), name
        assert st["order_free"] == (0 if name == "wide" else 1), name
        if st["order_free"]:   # then the serial double sum is the exact one, and so is every other order's
            assert float(inp.serial_sum64(sel)) == st["sum"]
            assert float(np.sum(sel.astype(np.float64))) == st["sum"]
    wide = inputs["wide"][0]
    assert float(inp.serial_sum64(wide)) != fsum(wide)   # what the proof is for: here the order matters
    # the boundary of the proof: 2^53 ones' worth of magnitude at q = 0
    assert api.image_stats_host(np.array([2.0 ** 52, 2.0 ** 52 - 2.0 ** 29, 1.0], np.float32))["order_free"] == 1
    assert api.image_stats_host(np.array([2.0 ** 52, 2.0 ** 52, 1.0], np.float32))["order_free"] == 0


def cli(*args):
    return subprocess.run([CLI] + list(args), capture_output=True, text=True, timeout=60)


TOO_FEW = [
    ("-thresh", [], "1 number."), ("-thresh", ["x"], "1 number."), ("-thresh-out", [], "1 number."),
    ("-thresh2", ["1"], "2 numbers."), ("-thresh2-out", ["1", "x"], "2 numbers."),
    ("-thresh4", ["1", "2", "3"], "4 numbers"), ("-thresh4-out", ["1", "2", "x", "4"], "4 numbers"),
    ("-thresh-interval", ["1"], "4 numbers."), ("-thresh-interval-out", ["x", "1"], "4 numbers."),
    ("-thresh-gauss", ["1"], "4 numbers."), ("-thresh-gauss-out", ["1", "x"], "4 numbers."),
    ("-thresh-range", ["1"], "2 numbers:"), ("-thresh-range-out", ["x", "2"], "2 numbers:"),
    ("-clip", ["1"], "2 numbers."), ("-cl", ["x", "y"], "2 numbers."),
    ("-rescale", ["2"], "2 numbers:"), ("-rescale", ["x", "1"], "2 numbers:"),
    ("-fill", [], "a number."), ("-fill", ["x"], "a number."),
    ("-rescale-min-max", ["0"], "2 numbers:"), ("-rescale-min-max", ["0", "x"], "2 numbers:"),
    ("-mask-select", [], "an integer."), ("-mask-select", ["x"], "an integer."),
]


@pytest.mark.parametrize("flag,words,what", TOO_FEW, ids=["%s-%d" % (t[0], i) for i, t in enumerate(TOO_FEW)])
def test_parser_wants_its_numbers(flag, words, what):
    r = cli("-in", "nothing.rec", flag, *words)
    assert r.returncode == 1
    assert "Error: The %s argument must be followed by %s" % (flag, what) in r.stderr, r.stderr
    assert "Unrecognized" not in r.stderr


def test_parser_thresh4_order_and_refusals():
    for nums in (["1", "2", "3", "2"], ["4", "3", "5", "1"]):
        r = cli("-in", "nothing.rec", "-thresh4", *nums)
        assert r.returncode == 1 and "These numbers must be either in increasing or decreasing order" in r.stderr
    for tail in (["-invert"], ["-thresh2", "1", "2"], ["-rescale-min-max", "0", "1"], ["-fill", "1"], ["-mask-select", "1"]):
        r = cli("-in", "nothing.rec", "-gauss", "1", "-slab", "0", "1", "-", *tail)
        assert r.returncode == 1 and "-slab runs with" in r.stderr and tail[0] in r.stderr, r.stderr
    for tail in (["-thresh", "1"], ["-thresh2", "1", "2"], ["-clip", "1", "2"], ["-cl", "1", "2"], ["-thresh4", "1", "2", "3", "4"],
                 ["-thresh-interval", "1", "2"], ["-thresh-gauss", "1", "2"]):
        r = cli("-in", "nothing.rec", "-membrane", "minima", "30", *tail)
        assert r.returncode == 1 and (tail[0] + " does not combine with -membrane") in r.stderr, r.stderr
    # the maps that act on the output pass the parser on that path (the run then fails on the missing file)
    for tail in (["-rescale", "2", "1"], ["-fill", "1"], ["-invert"], ["-rescale-min-max", "0", "1"], ["-no-rescale"]):
        r = cli("-in", "nothing.rec", "-membrane", "minima", "30", *tail)
        assert r.returncode == 1 and "nothing.rec" in r.stderr and "combine" not in r.stderr, r.stderr
