"""The surface points on the GPU (csrc/surface_points.hip): Context.surface_points and surface_points_dev against the host
entry visfd_hip_surface_points (which tests/test_surface_points.py pins to the numpy restatement) on every case of
tests/surface_points_cases.py.  Every comparison is bitwise, in count and in order."""
import os
import subprocess

import numpy as np
import pytest

import surface_points_cases as SC
from conftest import GOLDEN, ROOT, assert_bits_equal

pytestmark = pytest.mark.gpu

CLI = os.path.join(ROOT, "visfd_amd", "cli", "filter_mrc")
ECAPACITY = 4


@pytest.fixture(scope="module")
def ctx():
    from visfd_amd import api
    c = api.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def torch():
    import torch
    return torch


_HOST = {}


def host(name):
    if name not in _HOST:
        from visfd_amd import api
        c = SC.get(name)
        _HOST[name] = api.surface_points_host(c["saliency"], c["direction"], **SC.call_args(c))
        for a in _HOST[name]:
            a.setflags(write=False)
    return _HOST[name]


def selected(c):
    sel = np.ones(c["saliency"].shape, bool) if c["mask"] is None else c["mask"] != 0
    if c["cluster"] is not None:
        sel &= c["cluster"] == np.float32(c["select_cluster"])
    return int(sel.sum())


def dev_args(torch, c):
    up = lambda a: None if a is None else torch.from_numpy(np.array(a, order="C")).cuda()   # (the cases' arrays are read-only)
    planar = np.ascontiguousarray(np.moveaxis(c["direction"], 3, 0))
    kw = SC.call_args(c)
    kw["voxel2cluster"], kw["mask"] = up(c["cluster"]), up(c["mask"])
    return (up(c["saliency"]), up(planar)), kw


def check(got, want, what):
    assert_bits_equal(got[0], want[0], what + " crds")
    assert_bits_equal(got[1], want[1], what + " norms")


@pytest.mark.parametrize("name", sorted(SC.CASES))
def test_both_faces_equal_the_host_entry_on_the_device_path(ctx, torch, name):
    from visfd_amd import api
    c = SC.get(name)
    want = host(name)
    got = ctx.surface_points(c["saliency"], c["direction"], **SC.call_args(c))
    last = ctx.surface_points_last()
    print(name, "host face:", last)
    check(got, want, name + " host face")
    assert last[:4] == (api.SURFACE_POINTS_PATH_DEVICE, 0, selected(c), len(want[0])), last
    assert last[4] < 60
    a, kw = dev_args(torch, c)
    got = ctx.surface_points_dev(*a, **kw)
    last = ctx.surface_points_last()
    check(got, want, name + " device face")
    assert last[:4] == (api.SURFACE_POINTS_PATH_DEVICE, 0, selected(c), len(want[0])), last


def test_device_face_writes_device_arrays(ctx, torch):
    c = SC.get("sheet")
    want = host("sheet")
    a, kw = dev_args(torch, c)
    cap = len(want[0]) + 5
    crds = torch.full((cap, 3), float("nan"), device="cuda")
    norms = torch.full((cap, 3), float("nan"), device="cuda")
    n = ctx.surface_points_dev(*a, crds=crds, norms=norms, **kw)
    assert n == len(want[0])
    check((crds[:n].cpu().numpy(), norms[:n].cpu().numpy()), want, "device arrays")
    assert bool(torch.isnan(crds[n:]).all()) and bool(torch.isnan(norms[n:]).all())   # nothing past the count


def test_unaligned_images_take_the_scalar_select(ctx, torch):
    """label and mask images that start 4 bytes past a 16-byte boundary"""
    c = SC.get("mask_cut_no_ridge")
    want = host("mask_cut_no_ridge")
    (s, v), kw = dev_args(torch, c)
    shift = lambda t: torch.cat([t.new_zeros(1), t.reshape(-1)])[1:].reshape(t.shape)
    kw["voxel2cluster"], kw["mask"] = shift(kw["voxel2cluster"]), shift(kw["mask"])
    assert kw["mask"].data_ptr() % 16 == 4 and kw["mask"].is_contiguous()
    check(ctx.surface_points_dev(s, v, **kw), want, "unaligned")


def test_steps_cap_hands_the_call_over_and_the_points_stay(ctx, torch):
    from visfd_amd import api
    c = SC.get("sheet")
    want = host("sheet")
    with ctx.options(surface_steps_cap=8):
        got = ctx.surface_points(c["saliency"], c["direction"], **SC.call_args(c))
        last = ctx.surface_points_last()
        check(got, want, "capped host face")
        assert last[0] == api.SURFACE_POINTS_PATH_HANDED_OVER and last[1] == api.SURFACE_POINTS_REASON_STEPS, last
        assert last[2] == selected(c) and last[3] == len(want[0])
        a, kw = dev_args(torch, c)
        got = ctx.surface_points_dev(*a, **kw)
        last = ctx.surface_points_last()
        check(got, want, "capped device face")
        assert last[0] == api.SURFACE_POINTS_PATH_HANDED_OVER and last[1] == api.SURFACE_POINTS_REASON_STEPS, last
    assert ctx.get_option("surface_steps_cap") == 256


def test_zero_length_directions_end_their_walks(ctx, torch):
    """Outside the bit contract (the host's (int)round(NaN) is undefined): the call returns, and no selected voxel gives
    more than one point."""
    c = SC.ZERO_DIRECTION()
    for ridge in (True, False):
        kw = dict(SC.call_args(c), find_ridge=ridge)
        got = ctx.surface_points(c["saliency"], c["direction"], **kw)   # raises unless VISFD_HIP_OK
        assert len(got[0]) <= selected(c)
        a, dkw = dev_args(torch, c)
        got = ctx.surface_points_dev(*a, **dict(dkw, find_ridge=ridge))
        assert len(got[0]) <= selected(c)


@pytest.mark.parametrize("name", ["sheet", "no_ridge", "no_cluster_masked"])
def test_too_small_a_capacity_reports_the_count(ctx, torch, name):
    from visfd_amd import api
    c = SC.get(name)
    want = host(name)
    a, kw = dev_args(torch, c)
    for call in (lambda **k: ctx.surface_points(c["saliency"], c["direction"], **dict(SC.call_args(c), **k)),
                 lambda **k: ctx.surface_points_dev(*a, **dict(kw, **k))):
        with pytest.raises(api.VisfdHipError) as e:
            call(capacity=len(want[0]) - 1)
        assert e.value.code == ECAPACITY and e.value.needed == len(want[0])
        check(call(capacity=e.value.needed), want, name + " at the reported capacity")


def test_two_calls_in_a_row_give_the_same_bytes(ctx, torch):
    c = SC.get("tilted")
    a, kw = dev_args(torch, c)
    first = ctx.surface_points_dev(*a, **kw)
    other = SC.get("no_ridge")                      # another call in between, on the same workspace
    ctx.surface_points(other["saliency"], other["direction"], **SC.call_args(other))
    second = ctx.surface_points_dev(*a, **kw)
    assert first[0].tobytes() == second[0].tobytes() and first[1].tobytes() == second[1].tobytes()
    check(first, host("tilted"), "tilted")


def test_count_only_call(ctx, torch):
    import ctypes as C
    from visfd_amd import api
    for name in ("sheet", "no_ridge"):
        c = SC.get(name)
        nz, ny, nx = c["saliency"].shape
        n = C.c_int64(-1)
        kw = SC.call_args(c)
        rc = ctx._L.visfd_hip_surface_points_ctx(ctx._h, c["saliency"].ctypes.data, c["cluster"].ctypes.data,
                                                c["direction"].ctypes.data, None, nx, ny, nz, kw["select_cluster"],
                                                api._f3(kw["voxel_width"]), kw["curve_ds"], int(kw["find_ridge"]),
                                                kw["max_distance_to_feature"], None, None, 0, C.byref(n))
        assert rc == 0 and n.value == len(host(name)[0])


def test_program_writes_the_reference_programs_ply(tmp_path):
    """The scenario of tests/golden/make_golden_surface_points.py: this project's program on the recorded input and tensor
    files, with a device, against the PLY text the reference program wrote."""
    import sys
    sys.path.insert(0, GOLDEN)
    import make_golden_surface_points as MG
    g = np.load(os.path.join(GOLDEN, "surface_points.npz"))
    assert MG.write_files(str(tmp_path)) == int(g["crc"]), "the scenario's files are not the ones the golden text was made from"
    args = [str(x) for x in g["args"]]
    assert args == SC.PROGRAM_ARGS
    r = subprocess.run([CLI] + args, cwd=str(tmp_path), capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    got = (tmp_path / "n.ply").read_text()
    want = g["ply"].tobytes().decode()
    assert got.count("\n") > 200
    assert got == want
