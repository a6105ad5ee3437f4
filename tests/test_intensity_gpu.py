"""Image statistics and intensity maps on the GPU (csrc/intensity.hip): the exact sum against math.fsum, every map against
the numpy restatement (tests/intensity_np.py), the torch and C++ faces, and filter_mrc's tail against what the reference
program wrote (tests/golden/intensity.npz).

Equality is bit for bit everywhere but for the Gaussian map (-thresh-gauss), which gets one float ulp: its only operation
that is not the reference's own is the device's double exp; a last-bit difference of that double moves the rounded float
by at most one ulp.  The number of voxels that differ is printed."""
import math
import os
import struct
import subprocess

import numpy as np
import pytest

import intensity_cases as ic
import intensity_np as inp
import volgen
from conftest import ROOT, assert_bits_equal, golden
from test_intensity import assert_within_one_ulp, fsum, run_shim, shim

pytestmark = pytest.mark.gpu

CLI = os.path.join(ROOT, "visfd_amd", "cli", "filter_mrc")
REF_CLI = os.path.join(ROOT, "oracle", "_ref", "filter_mrc_ref")
HOST_SUM_LINE = "-invert: summing on the host in scan order"
SIZES = (1, 63, 64, 65, 257, 4 * 64 * 1024 + 3)   # the last: several workgroups and a ragged tail
SHAPES = ((1, 1, 1), (1, 1, 65), (7, 9, 11), (5, 33, 67))


@pytest.fixture(scope="module")
def api():
    from visfd_amd import api as a
    return a


@pytest.fixture(scope="module")
def ctx(api):
    c = api.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def torch():
    import torch as t
    return t


@pytest.fixture(scope="module")
def shim_exe(tmp_path_factory):
    return shim(tmp_path_factory)


_stats_cache = {}


def stats_case(kind, n):
    """values, mask and the expected statistics with and without the mask, computed once"""
    if (kind, n) not in _stats_cache:
        base = ic.stats_inputs()[kind]
        v = np.ascontiguousarray(np.resize(base, n))
        mask = (np.random.default_rng(n).random(n) < 0.6).astype(np.float32)
        mask[0] = 1.0
        want = {}
        for key, sel in (("all", v), ("mask", v[mask != 0])):
            want[key] = dict(count=sel.size, n_nonfinite=0, sum=fsum(sel), min=sel.min(), max=sel.max())
        _stats_cache[(kind, n)] = (v, mask, want)
    return _stats_cache[(kind, n)]


def check_stats(st, want, what):
    for k, x in want.items():
        assert st[k] == x, (what, k, st[k], x)


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("kind", ["dyadic", "wide", "cancel_wide", "denormal"])
def test_stats_are_exact(kind, n, api, ctx, torch):
    v, mask, want = stats_case(kind, n)
    host = api.image_stats_host(v)
    dv, dm = torch.from_numpy(v).cuda(), torch.from_numpy(mask).cuda()
    for blocks in (0, 1, 5):   # the result must not depend on the grid
        with ctx.options(stats_blocks=blocks):
            st = ctx.image_stats(v)
            check_stats(st, want["all"], "numpy face, %d blocks" % blocks)
            assert st == host, (st, host)
            check_stats(ctx.image_stats(v, mask), want["mask"], "numpy face, mask, %d blocks" % blocks)
            check_stats(ctx.image_stats(dv), want["all"], "torch face, %d blocks" % blocks)
            check_stats(ctx.image_stats(dv, dm), want["mask"], "torch face, mask, %d blocks" % blocks)
    ctx.debug_poison_workspace()
    check_stats(ctx.image_stats(dv, dm), want["mask"], "after the workspace was poisoned")
    check_stats(ctx.image_stats(v), want["all"], "after the workspace was poisoned")


def test_stats_edges(api, ctx):
    v = np.array([1.0, np.nan, np.inf, -np.inf, 2.0, 0.0, -0.0], np.float32)
    st = ctx.image_stats(v)
    assert st["count"] == 7 and st["n_nonfinite"] == 3
    st = ctx.image_stats(v, np.array([1, 0, 0, 0, 1, 1, 1], np.float32))
    assert st == api.image_stats_host(v, np.array([1, 0, 0, 0, 1, 1, 1], np.float32))
    assert st["n_nonfinite"] == 0 and st["sum"] == 3.0 and st["min"] == 0.0 and st["max"] == 2.0 and st["order_free"] == 1
    st = ctx.image_stats(v, np.zeros(7, np.float32))
    assert st["count"] == 0 and st["sum"] == 0.0 and st["order_free"] == 1
    for name, (vol, mask) in ic.inputs().items():
        st = ctx.image_stats(vol, mask)
        assert st == api.image_stats_host(vol, mask), name
        assert st["order_free"] == (0 if name == "wide" else 1), name
    # unaligned arrays: the scalar head and tail, and the all-scalar path when the two addresses disagree modulo 16
    big = np.resize(ic.stats_inputs()["wide"], 3000).astype(np.float32)
    mbuf = (np.random.default_rng(3).random(3010) < 0.5).astype(np.float32)
    for off_v in (0, 1, 2, 3):
        for off_m in (0, 1):
            n = 2990
            vv, mm = big[off_v:off_v + n], mbuf[off_m:off_m + n]
            st = ctx.image_stats(np.ascontiguousarray(vv), np.ascontiguousarray(mm))
            assert st["sum"] == fsum(vv[mm != 0]) and st["count"] == int((mm != 0).sum())


def dev_view(torch, a, offset):
    """a device copy of `a` that starts `offset` floats behind a 16-byte boundary"""
    buf = torch.zeros(a.size + 8, dtype=torch.float32, device="cuda")
    view = buf[offset:offset + a.size].view(a.shape)
    view.copy_(torch.from_numpy(a))
    assert view.data_ptr() % 16 == 4 * (offset % 4) and view.is_contiguous()
    return view


@pytest.mark.parametrize("shape", SHAPES, ids=["x".join(map(str, s)) for s in SHAPES])
@pytest.mark.parametrize("name", sorted(ic.MAP_CASES))
def test_maps_equal_restatement(name, shape, api, ctx, torch):
    kw = ic.MAP_CASES[name]
    nz_ny_nx = shape[::-1]
    src, out, mask = ic.map_volume(nz_ny_nx)
    uses_mask = "invert_ave" in kw or "masked_value" in kw
    compare = assert_within_one_ulp if name in ic.MAP_GAUSS_CASES else assert_bits_equal
    reads_src = kw.get("map", 0) in (1, 2, 3, 4, 5)
    for m in ((None, mask) if uses_mask else (None,)):
        p = ic.map_params(api, kw, stats_mask=m is not None)
        # out of place, and in place (the map's input is the output array itself)
        want = inp.apply(out, src, m, **kw)
        want_in_place = inp.apply(src, src, m, **kw)
        got = out.copy()
        st = ctx.intensity_map(p, got, src if reads_src else None, m, want_stats=True)
        compare(got, want, name + " numpy face")
        assert st == api.image_stats_host(got, m), "stats_out is not the statistics of what was written"
        assert st == ctx.image_stats(got, m)
        got = src.copy()
        ctx.intensity_map(p, got, got, m)
        compare(got, want_in_place, name + " numpy face, in place")
        # the torch face; (0, 0, 0): vectors from the first element, (1, 1, 1): a scalar head, (1, 2, 0): addresses
        # that disagree modulo 16, everything scalar
        for offs in ((0, 0, 0), (1, 1, 1), (1, 2, 0)):
            ds, do = dev_view(torch, src, offs[0]), dev_view(torch, out, offs[1])
            dm = None if m is None else dev_view(torch, m, offs[2])
            st = ctx.intensity_map(p, do, ds if reads_src else None, dm, want_stats=True)
            compare(do.cpu().numpy(), want, "%s torch face, offsets %s" % (name, offs))
            assert st == api.image_stats_host(do.cpu().numpy(), m)
            ctx.intensity_map(p, ds, ds, dm)
            ctx.synchronize()   # without stats_out the call only queues the kernel
            compare(ds.cpu().numpy(), want_in_place, "%s torch face, in place, offsets %s" % (name, offs))
    ctx.synchronize()


def test_invert_leaves_masked_voxels_alone(api, ctx, torch):
    """With invert and no mask fill, voxels with mask == 0 are not written: a poison pattern there survives bit for bit."""
    src, out, mask = ic.map_volume((11, 9, 7))
    poison = np.array([0xFFC0DEAD], np.uint32).view(np.float32)[0]
    out = np.where(mask == 0, poison, out).astype(np.float32)
    ave = api.image_stats_host(out, mask)
    p = api.intensity(invert_ave=ave["sum"] / ave["count"])
    want = inp.apply(out, None, mask, invert_ave=ave["sum"] / ave["count"])
    for off in (0, 1):
        do, dm = dev_view(torch, out, off), dev_view(torch, mask, off)
        ctx.intensity_map(p, do, None, dm)
        ctx.synchronize()
        got = do.cpu().numpy()
        assert_bits_equal(got, want, "invert under a mask")
        assert np.all(got.view(np.uint32)[mask == 0] == 0xFFC0DEAD)


def test_map_refuses_overlap(api, ctx, torch):
    buf = torch.zeros(200, dtype=torch.float32, device="cuda")
    p = api.intensity(api.MAP_THRESH2, (0.0, 1.0))
    with pytest.raises(api.VisfdHipError):
        ctx.intensity_map(p, buf[4:104].view(1, 10, 10), buf[0:100].view(1, 10, 10))
    with pytest.raises(api.VisfdHipError):
        ctx.intensity_map(p, buf[0:100].view(1, 10, 10), buf[100:200].view(1, 10, 10), buf[50:150].view(1, 10, 10))
    with pytest.raises(api.VisfdHipError):
        ctx.intensity_map(p, buf[0:100].view(1, 10, 10), None)   # a threshold map without its input


@pytest.mark.parametrize("name", ["thresh4", "everything", "gauss"])
def test_cpp_drop_in(name, api, shim_exe, tmp_path):
    """visfd::IntensityMap and visfd::ImageStats of include/visfd_hip.hpp, in a process of their own."""
    exe = shim_exe
    kw = ic.MAP_CASES[name]
    src, out, mask = ic.map_volume((5, 6, 7))
    p = ic.map_params(api, kw, stats_mask=True)
    got, tail = run_shim(exe, "gpu", tmp_path, p, src, out, mask)
    want = inp.apply(out, src, mask, **kw)
    (assert_within_one_ulp if name in ic.MAP_GAUSS_CASES else assert_bits_equal)(got, want, name)
    st = api.Stats.from_buffer_copy(tail[:40]).as_dict()
    st2 = api.Stats.from_buffer_copy(tail[40:80]).as_dict()
    assert st == st2 == api.image_stats_host(np.ascontiguousarray(got), mask)


# ---- filter_mrc -------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def files(tmp_path_factory):
    d = tmp_path_factory.mktemp("intensity_cli")
    for name, (vol, mask) in ic.inputs().items():
        volgen.write_mrc(str(d / (name + ".rec")), vol, voxel_width=ic.voxel_width(name))
        if mask is not None:
            volgen.write_mrc(str(d / (name + "_mask.rec")), mask, voxel_width=ic.voxel_width(name))
    return d


def header_stats(path):
    with open(path, "rb") as f:
        return np.frombuffer(f.read(1024), "<f4")[19:22].copy()


def run_cli(exe, case, d, out_name):
    name, input_name, use_mask, flags = case
    args = ic.command(case, exe, input_name + ".rec", input_name + "_mask.rec", out_name)
    r = subprocess.run(args, cwd=str(d), capture_output=True, text=True, timeout=120, env=dict(os.environ, OMP_NUM_THREADS="1"))
    assert r.returncode == 0, (args, r.stderr[-2000:])
    return volgen.read_mrc(str(d / out_name)), header_stats(str(d / out_name)), r.stderr


@pytest.mark.parametrize("case", ic.CASES, ids=[c[0] for c in ic.CASES])
def test_cli_reproduces_the_reference(case, files):
    name, input_name = case[0], case[1]
    gold = golden("intensity")
    got, header, err = run_cli(CLI, case, files, "out_%s.rec" % name)
    want, want_header = gold["out/" + name], gold["header/" + name]
    if name in ic.GAUSS_ULP_CASES:
        assert_within_one_ulp(got, want, name)
        if np.array_equal(got.view(np.uint32), want.view(np.uint32)):
            assert_bits_equal(header, want_header, name + " header")
    else:
        assert_bits_equal(got, want, name)
        assert_bits_equal(header, want_header, name + " header (dmin, dmax, dmean)")
    # the host sum is announced exactly where the proof of order-freedom fails
    if "-invert" in case[3] or "-inv" in case[3]:
        if input_name == "wide":
            assert HOST_SUM_LINE in err, err
        elif "-gauss" not in case[3]:   # (a filtered image may or may not pass the proof)
            assert HOST_SUM_LINE not in err, err
    else:
        assert HOST_SUM_LINE not in err
    if any(f.startswith("-gauss") for f in case[3]) and any(f.startswith(("-thresh", "-cl")) and "range" not in f for f in case[3]):
        assert "maps the INPUT image" in err


LIVE = [
    ("live_invert", "blob", False, ["-invert"]),
    ("live_gauss_cl", "blob", False, ["-gauss", "120", "-cl", "-1", "1.5"]),
    ("live_rescale_min_max", "blob", True, ["-rescale-min-max", "0", "1"]),
]


@pytest.mark.parametrize("case", LIVE, ids=[c[0] for c in LIVE])
def test_cli_against_a_live_reference_run(case, files):
    if not os.path.exists(REF_CLI):
        pytest.skip("oracle/_ref/filter_mrc_ref is not built")
    got, header, _ = run_cli(CLI, case, files, "got_%s.rec" % case[0])
    want, want_header, _ = run_cli(REF_CLI, case, files, "want_%s.rec" % case[0])
    assert_bits_equal(got, want, case[0])
    assert_bits_equal(header, want_header, case[0] + " header")


def test_pipeline_tail(api, ctx, torch):
    """pipeline.gauss(..., tail=...) and pipeline.intensity_tail on device tensors: the reference's order of stages."""
    from visfd_amd import pipeline
    src, _, mask = ic.map_volume((11, 9, 7))
    ds, dm = torch.from_numpy(src).cuda(), torch.from_numpy(mask).cuda()
    dst = torch.empty_like(ds)
    pipeline.gauss(ctx, ds, dst, 1.5, mask=dm)
    ctx.synchronize()
    filtered = dst.cpu().numpy()
    pipeline.gauss(ctx, ds, dst, 1.5, mask=dm, tail=dict(invert=True, map=api.MAP_RESCALE, t=(2.0, 1.0), masked_value=5.0,
                                                          rescale_min_max=(1.0, 0.0)))
    ctx.synchronize()
    flags = ["-invert", "-rescale", "2", "1", "-mask-out", "5", "-rescale-min-max", "1", "0"]
    st = api.image_stats_host(filtered, mask)
    want = inp.tail(src, filtered, mask, flags)
    if st["order_free"]:   # (else the serial sum of the restatement and the exact one may differ in the last bit)
        assert_bits_equal(dst.cpu().numpy(), want, "gauss with a tail")
    out = ds.clone()
    pipeline.intensity_tail(ctx, ds, out, None, map=api.MAP_THRESH2, t=(-100.0, 150.25), out_a=3.0, out_b=-2.5)
    ctx.synchronize()
    assert_bits_equal(out.cpu().numpy(), inp.tail(src, src, None, ["-thresh2", "-100", "150.25", "-thresh-range", "3", "-2.5"]),
                      "thresh2 tail")
    with pytest.raises(ValueError):
        wide = torch.from_numpy(ic.wide_volume()).cuda()
        pipeline.intensity_tail(ctx, wide, wide.clone(), None, invert=True)
