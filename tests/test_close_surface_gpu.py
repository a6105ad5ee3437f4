"""close_surface on the GPU (csrc/close_surface.hip) against the numpy restatement (tests/close_surface_np.py,
held to its own conditions in test_close_surface.py): the integer splat bit for bit, the mask up to the voxels whose float64
value lies within 1e-3 of the field's range of the level, the level against the restatement's sampling of the device's own
field, the same bits on every run, and the geometric conditions on the device mask itself.

The band of 1e-3 of the range holds at most 1 % of the restatement's mask on every case (0.07 to 0.48 % on the spheres, none
of the 3 voxels of `tiny`) but `thin`: three planes between two Dirichlet faces, where the float64 field itself is so flat that
18 of its 585 mask voxels (3.1 %) lie in the band.  There the cap says nothing about the device and only the rule itself
(differences inside the band only) is asserted.

The small cases fit one plane per workgroup; `test_marching_sweeps_on_a_larger_box` runs a box on which the sweeps and the
restriction march over several planes per workgroup, as they do at real sizes."""
import os
import subprocess
import sys

import numpy as np
import pytest

import close_surface_np as R
import volgen
from close_surface_cases import CASES, SPHERE_CASES
from conftest import ROOT, assert_bits_equal

pytestmark = pytest.mark.gpu

EINVAL = 1
SOLVED = sorted(set(CASES) - {"empty"})
CAPPED = set(SOLVED) - {"thin"}


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


_DEVICE = {}


def device(ctx, name):
    """(mask, chi, last) of the host face on a case, computed once"""
    if name not in _DEVICE:
        c = CASES[name]
        mask, chi = ctx.close_surface(c.points, c.normals, c.shape, c.pad, c.orientation, want_chi=True)
        for a in (mask, chi):
            a.setflags(write=False)
        _DEVICE[name] = (mask, chi, ctx.close_surface_last())
    return _DEVICE[name]


@pytest.mark.parametrize("name", sorted(CASES))
def test_splat_equals_the_python_integer_splat_on_both_faces(ctx, torch, name):
    c = CASES[name]
    ref = R.reference(c)
    acc, used, skipped = ctx.close_surface_splat(c.points, c.normals, c.shape, c.pad)
    assert (used, skipped) == (ref.n_used, ref.n_skipped)
    assert_bits_equal(acc, ref.acc, name + ", host face")
    d = torch.full(ref.acc.shape, -7, dtype=torch.int64, device="cuda")
    p, n = torch.from_numpy(c.points).cuda(), torch.from_numpy(c.normals).cuda()
    assert ctx.close_surface_splat_dev(d, p, n, c.shape, c.pad) == (ref.n_used, ref.n_skipped)
    assert_bits_equal(d.cpu().numpy(), ref.acc, name + ", device face")


@pytest.mark.parametrize("name", sorted(CASES))
def test_mask_differs_from_the_restatement_only_in_the_band(ctx, name):
    c = CASES[name]
    ref = R.reference(c)
    mask, chi, last = device(ctx, name)
    assert mask.dtype == np.float32 and set(np.unique(mask)) <= {0.0, 1.0}
    if name == "empty":
        assert not mask.any() and not chi.any() and last["n_used"] == 0
        return
    err = float(np.abs(chi - R.image_of(ref.chi, c.pad)).max())
    bd = R.band(R.image_of(ref.chi, c.pad), ref.iso, ref.range)
    diff = mask != ref.mask
    print("%s: max|chi - chi64| = %.3g of the range, iso %.9g vs %.9g, %d voxels differ, band %d, mask %d" % (
        name, err / ref.range, last["iso"], ref.iso, int(diff.sum()), int(bd.sum()), int(ref.mask.sum())))
    assert not (diff & ~bd).any(), "%d voxels differ outside the band" % int((diff & ~bd).sum())
    if name in CAPPED:
        assert int(bd.sum()) <= 0.01 * ref.mask.sum()
    assert err <= 1e-4 * ref.range, "the solver's error is to stay a tenth of the band"


@pytest.mark.parametrize("name", SOLVED)
def test_level_is_the_sampling_of_the_device_field(ctx, name):
    """iso against the restatement's sampling of the device's own chi_out (every used point of every case lies in a cell of
    the image, so the image's part of the field is all the sampling reads)"""
    c = CASES[name]
    ref = R.reference(c)
    mask, chi, last = device(ctx, name)
    assert R.used_mask(c.points, c.normals, c.shape, 0).sum() == c.n_used
    want = R.sample(chi, c.points, c.normals, c.shape, 0)
    print("%s: iso %.12g, sampled %.12g, range %.6g" % (name, last["iso"], want, ref.range))
    assert abs(last["iso"] - want) <= 1e-6 * ref.range


@pytest.mark.parametrize("name", ["caps60", "padded", "thin", "junk"])
def test_same_bits_on_every_run_and_on_a_fresh_context(ctx, name):
    from visfd_amd import api
    c = CASES[name]
    mask, chi, last = device(ctx, name)
    m2, chi2 = ctx.close_surface(c.points, c.normals, c.shape, c.pad, c.orientation, want_chi=True)
    assert_bits_equal(m2, mask, "second call: mask")
    assert_bits_equal(chi2, chi, "second call: chi")
    assert ctx.close_surface_last() == last
    fresh = api.Context(0)
    try:
        m3, chi3 = fresh.close_surface(c.points, c.normals, c.shape, c.pad, c.orientation, want_chi=True)
        assert_bits_equal(m3, mask, "fresh context: mask")
        assert_bits_equal(chi3, chi, "fresh context: chi")
        assert fresh.close_surface_last() == last
    finally:
        fresh.close()


@pytest.mark.parametrize("name", SPHERE_CASES + ("inward",))
def test_device_mask_meets_the_geometric_conditions(ctx, name):
    g = R.check_geometry(device(ctx, name)[0], CASES[name])
    print(name, g)


def test_last_reports(ctx):
    from visfd_amd import api
    cap = ctx.get_option("close_surface_max_cycles")
    rtol = 10.0 ** -ctx.get_option("close_surface_rtol_exp")
    for name in SOLVED:
        last = device(ctx, name)[2]
        print(name, last)
        assert last["stop"] == api.CLOSE_STOP_RTOL and 0 < last["cycles"] < cap and 0.0 <= last["ratio"] <= rtol, (name, last)
        assert (last["n_used"], last["n_skipped"]) == (CASES[name].n_used, CASES[name].n_skipped)
        if name in SPHERE_CASES + ("inward", "junk"):
            assert last["touches_face"] == 0
    assert device(ctx, "thin")[2]["touches_face"] == 1      # three planes: every voxel lies on a face
    e = device(ctx, "empty")[2]
    assert (e["n_used"], e["n_skipped"], e["cycles"], e["stop"], e["touches_face"]) == (0, 0, 0, api.CLOSE_STOP_NONE, 0)
    j = device(ctx, "junk")[2]
    assert (j["n_used"], j["n_skipped"]) == (2943, 16)
    assert device(ctx, "inward")[2]["orientation"] == "inward"
    # the residual the call reports is that of the field it returns
    c = CASES["odd"]
    mask, chi, last = device(ctx, "odd")
    assert abs(R.residual_ratio(chi, R.reference(c).b) - last["ratio"]) <= 0.05 * last["ratio"] + 1e-9


def test_marching_sweeps_on_a_larger_box(ctx):
    """138 x 135 x 401: the sweeps march over 7 planes per workgroup and the fused restriction over 3 coarse planes (the last
    workgroup over 2), with rows that are no multiple of 4 and an odd number of planes.  The ratio the call reports is the
    residual of the field it returns, recomputed here in float64 from chi_out and the restatement's right-hand side (from
    the host splat, which test_close_surface.py pins to the Python integers); the call stops by rtol; a second call gives
    the same bits; the mask fills the ball."""
    from visfd_amd import api
    from close_surface_cases import sphere_cloud
    shape = (401, 135, 138)
    r = 55.0
    p, n, center = sphere_cloud(shape, r, 0.75, 11)
    mask, chi = ctx.close_surface(p, n, shape, 0, "outward", want_chi=True)
    last = ctx.close_surface_last()
    acc, used, skipped = api.close_surface_splat_host(p, n, shape, 0)
    assert (last["n_used"], last["n_skipped"]) == (used, skipped) == (len(p), 0)
    b = R.rhs(R.field_from_acc(acc))
    del acc
    true = R.residual_ratio(chi, b)
    print("larger box: reported %.6e, recomputed %.6e, %d cycles" % (last["ratio"], true, last["cycles"]))
    assert abs(true - last["ratio"]) <= 0.05 * last["ratio"]
    assert last["stop"] == api.CLOSE_STOP_RTOL and last["ratio"] <= 1e-5 and true <= 1.05e-5
    assert 0 < last["cycles"] < ctx.get_option("close_surface_max_cycles")
    m2, chi2 = ctx.close_surface(p, n, shape, 0, "outward", want_chi=True)
    assert_bits_equal(chi2, chi, "second call: chi")
    assert_bits_equal(m2, mask, "second call: mask")
    assert ctx.close_surface_last() == last
    inside, d = R.ball(shape, center, r)
    assert not R.touches_face(mask) and last["touches_face"] == 0
    assert 0.85 <= mask.sum() / inside.sum() <= 1.01
    z = np.arange(shape[0], dtype=np.float64)[:, None, None]
    diff = ((mask != 0) != inside) & (np.abs(z - center[2]) <= 0.75 * r)
    assert not diff.any() or np.abs(d[diff] - r).max() <= 0.5


def test_device_face_refuses_overlapping_arrays(ctx, torch):
    c = CASES["tiny"]
    nvox = c.shape[0] * c.shape[1] * c.shape[2]
    buf = torch.zeros(2 * nvox + 64, device="cuda")
    p, n = torch.from_numpy(c.points).cuda(), torch.from_numpy(c.normals).cuda()
    mask, chi = buf[:nvox].view(c.shape), buf[nvox:2 * nvox].view(c.shape)
    ctx.close_surface_dev(mask, p, n, c.pad, c.orientation, chi=chi)
    assert_bits_equal(mask.cpu().numpy(), device(ctx, "tiny")[0], "disjoint views of one buffer")
    lists = buf[nvox - 3:nvox + 3].view(2, 3)      # the last voxel of mask, the first of chi
    from visfd_amd import api
    for call in (lambda: ctx.close_surface_dev(mask, p, n, c.pad, c.orientation, chi=buf[1:nvox + 1].view(c.shape)),
                 lambda: ctx.close_surface_dev(mask, lists, n, c.pad, c.orientation),
                 lambda: ctx.close_surface_dev(mask, p, lists, c.pad, c.orientation),
                 lambda: ctx.close_surface_dev(buf[nvox + 32:2 * nvox + 32].view(c.shape), p, lists, c.pad, c.orientation,
                                               chi=chi)):
        with pytest.raises(api.VisfdHipError) as e:
            call()
        assert e.value.code == EINVAL
    ctx.close_surface_dev(mask, p, n, c.pad, c.orientation)
    assert_bits_equal(mask.cpu().numpy(), device(ctx, "tiny")[0], "after the refusals")


def test_cycle_cap_is_reported_and_the_mask_still_returned(ctx):
    from visfd_amd import api
    c = CASES["caps75"]
    with ctx.options(close_surface_max_cycles=1):
        mask = ctx.close_surface(c.points, c.normals, c.shape, c.pad, c.orientation)
        last = ctx.close_surface_last()
    assert last["stop"] == api.CLOSE_STOP_CAP and last["cycles"] == 1 and last["ratio"] > 1e-5
    assert mask.shape == c.shape and set(np.unique(mask)) <= {0.0, 1.0} and mask.any()
    with ctx.options(close_surface_rtol_exp=3):
        ctx.close_surface(c.points, c.normals, c.shape, c.pad, c.orientation)
        loose = ctx.close_surface_last()
    assert loose["stop"] == api.CLOSE_STOP_RTOL and loose["cycles"] < device(ctx, "caps75")[2]["cycles"]
    assert 1e-5 < loose["ratio"] <= 1e-3


def test_orientation_auto(ctx):
    for name, taken in (("inward", "inward"), ("caps75", "outward")):
        c = CASES[name]
        mask = ctx.close_surface(c.points, c.normals, c.shape, c.pad, "auto")
        assert ctx.close_surface_last()["orientation"] == taken
        assert_bits_equal(mask, device(ctx, name)[0], name + ", auto")
    assert_bits_equal(device(ctx, "inward")[0], device(ctx, "caps75")[0], "negated normals cut from the other side")


@pytest.mark.parametrize("name", ["odd", "padded", "tiny", "empty"])
def test_device_face_equals_host_face(ctx, torch, name):
    c = CASES[name]
    mask, chi, last = device(ctx, name)
    p, n = torch.from_numpy(c.points).cuda(), torch.from_numpy(c.normals).cuda()
    dm = torch.full(c.shape, float("nan"), device="cuda")
    dc = torch.full(c.shape, float("nan"), device="cuda")
    ctx.close_surface_dev(dm, p, n, c.pad, c.orientation, chi=dc)
    assert_bits_equal(dm.cpu().numpy(), mask, "mask")
    assert_bits_equal(dc.cpu().numpy(), chi, "chi")
    assert ctx.close_surface_last() == last
    dm.fill_(float("nan"))
    ctx.close_surface_dev(dm, p, n, c.pad, c.orientation)
    assert_bits_equal(dm.cpu().numpy(), mask, "mask without chi")


def test_refusals_leave_the_context_usable(ctx):
    from visfd_amd import api
    c = CASES["tiny"]
    L = ctx._L
    p, n = c.points, c.normals
    mask = np.zeros(c.shape, np.float32)
    held = ctx.workspace_bytes()
    bad = [(ctx._h, p.ctypes.data, n.ctypes.data, 2, 5, 4, 2, 0, 0, mask.ctypes.data, None),
           (ctx._h, p.ctypes.data, n.ctypes.data, 2, 2, 4, 3, 0, 0, mask.ctypes.data, None),
           (ctx._h, p.ctypes.data, n.ctypes.data, 2, 5, 4, 3, -1, 0, mask.ctypes.data, None),
           (ctx._h, p.ctypes.data, n.ctypes.data, -1, 5, 4, 3, 0, 0, mask.ctypes.data, None),
           (ctx._h, None, n.ctypes.data, 2, 5, 4, 3, 0, 0, mask.ctypes.data, None),
           (ctx._h, p.ctypes.data, None, 2, 5, 4, 3, 0, 0, mask.ctypes.data, None),
           (ctx._h, p.ctypes.data, n.ctypes.data, 2, 5, 4, 3, 0, 0, None, None),
           (None, p.ctypes.data, n.ctypes.data, 2, 5, 4, 3, 0, 0, mask.ctypes.data, None),
           (ctx._h, p.ctypes.data, n.ctypes.data, 2, 5, 4, 3, 0, 3, mask.ctypes.data, None),
           (ctx._h, p.ctypes.data, n.ctypes.data, 2, 5, 4, 3, 40000, 0, mask.ctypes.data, None)]
    for args in bad:
        assert L.visfd_hip_close_surface(*args) == EINVAL, args[3:9]
        assert L.visfd_hip_close_surface_dev(*args) == EINVAL, args[3:9]
    assert ctx.workspace_bytes() == held, "a refused call allocates nothing"
    with pytest.raises(api.VisfdHipError) as e:
        ctx.close_surface(p, n, (2, 4, 5))
    assert e.value.code == EINVAL
    assert_bits_equal(ctx.close_surface(p, n, c.shape), device(ctx, "tiny")[0], "after the refusals")


def test_phase_times(ctx):
    c = CASES["odd"]
    assert ctx.get_option("close_surface_time") == 0
    with ctx.options(close_surface_time=1):
        assert_bits_equal(ctx.close_surface(c.points, c.normals, c.shape, c.pad), device(ctx, "odd")[0], "timed call")
        ms = ctx.close_surface_last_times()
    assert len(ms) == 3 and all(0.0 <= x < 10000.0 for x in ms), ms


def test_program_end_to_end(ctx, tmp_path):
    from visfd_amd import voxelize_mesh as P
    d = str(tmp_path)
    c = CASES["caps75"]
    w = 12.5
    phys = (c.points.astype(np.float64) * w).astype(np.float32)
    pts = (phys.astype(np.float64) / w).astype(np.float32)      # the tool's division: the points up to a float ulp
    assert np.abs(pts - c.points).max() < 1e-5
    with open(os.path.join(d, "cloud.ply"), "w") as f:
        f.write("ply\nformat ascii 1.0\ncomment  created by visfd\nelement vertex %d\nproperty float x\nproperty float y\n"
                "property float z\nproperty float nx\nproperty float ny\nproperty float nz\nend_header\n" % len(phys))
        for a, b in zip(phys, c.normals):
            f.write(" ".join("%.9g" % v for v in list(a) + list(b)) + "\n")
    volgen.write_mrc(os.path.join(d, "orig.rec"), volgen.noise_volume(c.shape, seed=5), voxel_width=w)
    r = subprocess.run([sys.executable, "-m", "visfd_amd.close_surface", "-p", "cloud.ply", "-o", "mask.rec", "-i", "orig.rec",
                        "--orientation", "auto", "--chi", "chi.rec"], cwd=d, capture_output=True, text=True,
                       env=dict(os.environ, PYTHONPATH=ROOT), timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "2941 points used, 0 skipped" in r.stderr and "normals point outward" in r.stderr
    hdr = P.read_mrc_header(os.path.join(d, "mask.rec"))
    assert hdr["n"] == c.shape[::-1] and abs(hdr["cella"][0] - w * c.shape[2]) < 1e-3
    mask, chi = ctx.close_surface(pts, c.normals, c.shape, 0, "auto", want_chi=True)
    assert not (mask != device(ctx, "caps75")[0]).sum() > 5
    assert_bits_equal(volgen.read_mrc(os.path.join(d, "mask.rec")), mask, "the program's mask")
    assert_bits_equal(volgen.read_mrc(os.path.join(d, "chi.rec")), chi, "the program's chi")
    r = subprocess.run([sys.executable, "-m", "visfd_amd.close_surface", "-p", "orig.rec", "-o", "m2.rec", "-i", "orig.rec"],
                       cwd=d, capture_output=True, text=True, env=dict(os.environ, PYTHONPATH=ROOT), timeout=300)
    assert r.returncode == 1 and "not a PLY file" in r.stderr


def test_cpp_face(ctx, tmp_path):
    """include/visfd_hip.hpp: CloseSurface under g++ -std=c++11 -Wall -Werror gives the library call's mask"""
    from visfd_amd import api
    c = CASES["tiny"]
    src = tmp_path / "shim_close.cpp"
    src.write_text('''#include "visfd_hip.hpp"
#include <cstdio>
int main() {
  int size[3] = {5, 4, 3};
  float*** img = visfd::Alloc3D<float>(size);
  float* flat = &img[0][0][0];
  std::vector<std::array<float, 3> > p(2), n(2);
  p[0] = {{1.25f, 1.5f, 0.75f}}; p[1] = {{2.5f, 1.75f, 1.0f}};
  n[0] = {{-1.0f, 0.0f, 0.0f}}; n[1] = {{1.0f, 0.0f, 0.0f}};
  visfd::CloseSurface(nullptr, size, p, n, img);
  for (int i = 0; i < 60; i++) std::printf("%d", (int)flat[i]);
  std::printf("\\n");
  return 0;
}
''')
    exe = str(tmp_path / "shim_close")
    libdir = os.path.dirname(api.LIB_PATH)
    subprocess.check_call(["g++", "-std=c++11", "-O1", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), str(src),
                           "-L" + libdir, "-lvisfd_hip", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib", "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert r.stdout.strip() == "".join("%d" % v for v in device(ctx, "tiny")[0].ravel())
