"""The isosurface kernels (csrc/isosurface.hip) against the serial host walk, bit for bit, on both faces; the
caps protocol and the overlap refusals of the device face; and the round trip the mesh exists for: the field and the level of
close_surface, meshed and voxelised again on the device, give close_surface's mask back voxel for voxel.

The host walk itself is held to the Python restatement and to the definition's promises in test_isosurface.py."""
import os
import subprocess
import sys

import numpy as np
import pytest

from close_surface_cases import CASES as CLOUDS
from conftest import ROOT, assert_bits_equal
from isosurface_cases import CASES, DEVICE_CASES, SIDES

pytestmark = pytest.mark.gpu

EINVAL, ECAPACITY = 1, 4
ALL = {c.name: c for c in CASES + DEVICE_CASES}
PAIRS = [(name, s) for name in ALL for s in SIDES]
ROUND_TRIP = ("tiny", "thin", "odd", "padded")


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


def host(name, side):
    """the host walk's mesh of a case, computed once and frozen"""
    from visfd_amd import api
    if (name, side) not in _HOST:
        v, t = api.isosurface_host(ALL[name].vol, ALL[name].iso, side)
        v.setflags(write=False)
        t.setflags(write=False)
        _HOST[(name, side)] = (v, t)
    return _HOST[(name, side)]


@pytest.mark.parametrize("name,side", PAIRS)
def test_both_faces_equal_the_host_walk(ctx, torch, name, side):
    c = ALL[name]
    hv, ht = host(name, side)
    v, t = ctx.isosurface(c.vol, c.iso, side)
    assert (len(v), len(t)) == (len(hv), len(ht)), "counts, host face"
    assert_bits_equal(v, hv, "vertices, host face")
    assert_bits_equal(t, ht, "triangles, host face")
    last = ctx.isosurface_last()
    vol = np.asarray(c.vol, np.float64)
    with np.errstate(invalid="ignore"):
        inside = (vol < c.iso) if side == "below" else (vol > c.iso)
    faces = np.zeros(c.vol.shape, bool)
    for axis in range(3):
        idx = [slice(None)] * 3
        for k in (0, -1):
            idx[axis] = k
            faces[tuple(idx)] = True
    assert last == {"n_vertices": len(hv), "n_triangles": len(ht), "n_inside": int(inside.sum()),
                    "capped": int((inside & faces).any())}
    dv, dt = ctx.isosurface_dev(torch.from_numpy(c.vol).cuda(), c.iso, side)
    assert dv.dtype == torch.float32 and dt.dtype == torch.int32
    assert_bits_equal(dv.cpu().numpy(), hv, "vertices, device face")
    assert_bits_equal(dt.cpu().numpy(), ht, "triangles, device face")


def test_two_calls_write_the_same_bytes(ctx, torch):
    c = ALL["dense"]
    vol = torch.from_numpy(c.vol).cuda()
    a = ctx.isosurface_dev(vol, c.iso, "below")
    ctx.isosurface(ALL["sphere"].vol, 0.0, "above")   # another shape between the two: the workspace is reused
    b = ctx.isosurface_dev(vol, c.iso, "below")
    assert torch.equal(a[0].view(torch.int32), b[0].view(torch.int32)) and torch.equal(a[1], b[1])
    # 7 edges start at every lower node and one in two crosses where half the nodes are inside: 3.5 vertices per node
    assert len(a[0]) > 3 * c.vol.size, "the dense case"


def test_small_capacities_leave_the_arrays_alone_and_report_the_counts(ctx, torch):
    from visfd_amd import api
    c = ALL["noise547"]
    hv, ht = host("noise547", "above")
    n, m = len(hv), len(ht)
    vol = torch.from_numpy(c.vol).cuda()

    def fresh(rows_v, rows_t):
        return (torch.full((rows_v, 3), -3.0, dtype=torch.float32, device="cuda"),
                torch.full((rows_t, 3), -3, dtype=torch.int32, device="cuda"))

    v, t = fresh(n - 1, m)
    with pytest.raises(api.VisfdHipError) as e:
        ctx.isosurface_dev(vol, c.iso, "above", vertices=v, triangles=t)
    assert e.value.code == ECAPACITY and e.value.counts == (n, m)
    assert bool((v == -3.0).all()), "the short vertex array was written to"
    assert_bits_equal(t.cpu().numpy(), ht, "triangles beside a short vertex array")
    v, t = fresh(n, m - 1)
    with pytest.raises(api.VisfdHipError) as e:
        ctx.isosurface_dev(vol, c.iso, "above", vertices=v, triangles=t)
    assert e.value.code == ECAPACITY and e.value.counts == (n, m)
    assert bool((t == -3).all()), "the short triangle array was written to"
    assert_bits_equal(v.cpu().numpy(), hv, "vertices beside a short triangle array")
    v, t = fresh(n + 3, m + 3)
    assert ctx.isosurface_dev(vol, c.iso, "above", vertices=v, triangles=t) == (n, m)
    assert_bits_equal(v[:n].cpu().numpy(), hv, "vertices")
    assert_bits_equal(t[:m].cpu().numpy(), ht, "triangles")
    assert bool((v[n:] == -3.0).all()) and bool((t[m:] == -3).all()), "nothing past the counts"
    # the host face
    hv_small, ht_full = np.full((n - 1, 3), -3.0, np.float32), np.full((m, 3), -3, np.int32)
    with pytest.raises(api.VisfdHipError) as e:
        ctx.isosurface(c.vol, c.iso, "above", vertices=hv_small, triangles=ht_full)
    assert e.value.code == ECAPACITY and e.value.counts == (n, m) and (hv_small == -3.0).all()
    assert_bits_equal(ht_full, ht, "host face: triangles beside a short vertex array")


def test_device_face_refuses_overlapping_arrays(ctx, torch):
    from visfd_amd import api
    c = ALL["noise547"]
    hv, ht = host("noise547", "below")
    n, m = len(hv), len(ht)
    pool = torch.full((3 * (n + m) + c.vol.size + 64,), -3.0, dtype=torch.float32, device="cuda")
    vol = pool[:c.vol.size].view(c.vol.shape)
    vol.copy_(torch.from_numpy(c.vol))
    before = pool.clone()
    tail = pool[c.vol.size - 3:]            # starts on the volume's last three floats
    apart_v = pool[c.vol.size:c.vol.size + 3 * n].view(n, 3)
    apart_t = pool[c.vol.size + 3 * n:c.vol.size + 3 * (n + m)].view(torch.int32).view(m, 3)
    for v, t, what in ((tail[:3 * n].view(n, 3), apart_t, "overlaps the volume"),
                       (apart_v, tail[:3 * m].view(torch.int32).view(m, 3), "overlaps the volume"),
                       (apart_v, pool[c.vol.size + 3 * n - 3:c.vol.size + 3 * (n + m) - 3].view(torch.int32).view(m, 3),
                        "outputs overlap")):
        with pytest.raises(api.VisfdHipError) as e:
            ctx.isosurface_dev(vol, c.iso, "below", vertices=v, triangles=t)
        assert e.value.code == EINVAL and what in str(e.value) and e.value.counts is None
        assert torch.equal(pool.view(torch.int32), before.view(torch.int32)), "a refused call wrote something"
    # side by side in one allocation: accepted
    assert ctx.isosurface_dev(vol, c.iso, "below", vertices=apart_v, triangles=apart_t) == (n, m)
    assert_bits_equal(apart_v.cpu().numpy(), hv, "vertices")
    assert_bits_equal(apart_t.cpu().numpy(), ht, "triangles")


def test_refusals_leave_the_context_usable(ctx, torch):
    from visfd_amd import api
    c = ALL["single"]
    for bad in (float("nan"), float("inf")):
        with pytest.raises(api.VisfdHipError) as e:
            ctx.isosurface(c.vol, bad, "below")
        assert e.value.code == EINVAL
    with pytest.raises(api.VisfdHipError) as e:
        ctx.isosurface(c.vol, 0.0, 7)
    assert e.value.code == EINVAL
    v, t = ctx.isosurface(c.vol, c.iso, "below")
    assert_bits_equal(v, host("single", "below")[0], "after the refusals")


def test_phase_times(ctx):
    c = ALL["dense"]
    assert ctx.get_option("isosurface_time") == 0
    with ctx.options(isosurface_time=1):
        v, _t = ctx.isosurface(c.vol, c.iso, "below")
        ms = ctx.isosurface_last_times()
    assert_bits_equal(v, host("dense", "below")[0], "timed call")
    assert len(ms) == 4 and all(0.0 <= x < 10000.0 for x in ms), ms


@pytest.mark.parametrize("name", ROUND_TRIP)
def test_mesh_of_close_surface_voxelises_to_its_mask(ctx, torch, name):
    c = CLOUDS[name]
    mask = torch.empty(c.shape, dtype=torch.float32, device="cuda")
    chi = torch.empty(c.shape, dtype=torch.float32, device="cuda")
    ctx.close_surface_dev(mask, torch.from_numpy(c.points).cuda(), torch.from_numpy(c.normals).cuda(), c.pad, c.orientation,
                          chi=chi)
    last = ctx.close_surface_last()
    assert bool(mask.any()), "the case closes something"
    v, t = ctx.isosurface_dev(chi, last["iso"], "below" if last["orientation"] == "outward" else "above")
    assert ctx.isosurface_last()["n_inside"] == int(mask.sum().item())
    back = torch.full(c.shape, -1.0, dtype=torch.float32, device="cuda")
    ctx.voxelize_mesh_dev(back, v.cpu().numpy(), t.cpu().numpy(), 1.0, (0, 0, 0), check_closed=True)
    assert ctx.voxelize_last()[2] == 0, "odd rows"
    assert torch.equal(back, mask), "%d voxels differ" % int((back != mask).sum().item())


def test_program_writes_the_mesh(ctx, tmp_path):
    from visfd_amd import close_surface as P
    from visfd_amd import ply
    import volgen
    d = str(tmp_path)
    c = CLOUDS["tiny"]
    w = 1.7
    phys = (c.points.astype(np.float64) * w).astype(np.float32)
    pts = (phys.astype(np.float64) / w).astype(np.float32)      # the tool's division
    with open(os.path.join(d, "cloud.ply"), "w") as f:
        f.write("ply\nformat ascii 1.0\nelement vertex %d\nproperty float x\nproperty float y\nproperty float z\n"
                "property float nx\nproperty float ny\nproperty float nz\nend_header\n" % len(phys))
        for a, b in zip(phys, c.normals):
            f.write(" ".join("%.9g" % x for x in list(a) + list(b)) + "\n")
    nz, ny, nx = c.shape
    r = subprocess.run([sys.executable, "-m", "visfd_amd.close_surface", "-p", "cloud.ply", "-o", "mask.rec", "-w", repr(w),
                        "--image-size", str(nx), str(ny), str(nz), "--orientation", c.orientation, "--mesh", "mesh.ply"],
                       cwd=d, capture_output=True, text=True, env=dict(os.environ, PYTHONPATH=ROOT), timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    mask, _chi, _last, (v, t, level, _capped) = P.close_and_mesh(ctx, pts, c.normals, c.shape, c.pad, c.orientation)
    assert mask.any() and len(t) > 0
    assert "mesh of %d vertices and %d triangles" % (len(v), len(t)) in r.stderr
    rv, rt = ply.read_ply(os.path.join(d, "mesh.ply"))
    assert_bits_equal(rv, (v.astype(np.float64) * np.float64(w)).astype(np.float32), "the program's vertices")
    assert_bits_equal(rt, t, "the program's triangles")
    assert_bits_equal(volgen.read_mrc(os.path.join(d, "mask.rec")), mask, "the program's mask")
    # what the file is for: voxelised at the same width it is the mask
    assert_bits_equal(ctx.voxelize_mesh(rv, rt, c.shape, w), mask, "the mesh file voxelised")
    r = subprocess.run([sys.executable, "-m", "visfd_amd.close_surface", "-p", "cloud.ply", "-o", "m2.rec", "-w", repr(w),
                        "--image-size", str(nx), str(ny), str(nz), "--mesh-level", "0.5"],
                       cwd=d, capture_output=True, text=True, env=dict(os.environ, PYTHONPATH=ROOT), timeout=300)
    assert r.returncode == 1 and "--mesh-level needs --mesh" in r.stderr


def test_cpp_face(ctx, tmp_path):
    """include/visfd_hip.hpp: IsoSurface under g++ -std=c++11 -Wall -Werror gives the library call's mesh"""
    from visfd_amd import api
    src = tmp_path / "shim_iso.cpp"
    src.write_text('''#include "visfd_hip.hpp"
#include <cstdio>
int main() {
  int size[3] = {3, 3, 3};
  float*** img = visfd::Alloc3D<float>(size);
  float* flat = &img[0][0][0];
  for (int i = 0; i < 27; i++) flat[i] = 1.0f;
  flat[13] = -1.0f;
  std::vector<std::array<float, 3> > v;
  std::vector<std::array<int, 3> > t;
  size_t n = visfd::IsoSurface(nullptr, size, img, 0.0, VISFD_HIP_ISO_BELOW, v, t);
  std::printf("%d %d %d\\n", (int)v.size(), (int)t.size(), (int)n);
  for (size_t i = 0; i < v.size(); i++) std::printf("%.9g %.9g %.9g\\n", v[i][0], v[i][1], v[i][2]);
  for (size_t i = 0; i < t.size(); i++) std::printf("%d %d %d\\n", t[i][0], t[i][1], t[i][2]);
  return 0;
}
''')
    exe = str(tmp_path / "shim_iso")
    libdir = os.path.dirname(api.LIB_PATH)
    subprocess.check_call(["g++", "-std=c++11", "-O1", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), str(src),
                           "-L" + libdir, "-lvisfd_hip", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib", "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    hv, ht = host("single", "below")
    lines = r.stdout.split("\n")
    assert lines[0] == "%d %d %d" % (len(hv), len(ht), len(ht))
    got_v = np.array([[float(x) for x in l.split()] for l in lines[1:1 + len(hv)]], np.float32)
    got_t = np.array([[int(x) for x in l.split()] for l in lines[1 + len(hv):1 + len(hv) + len(ht)]], np.int32)
    assert_bits_equal(got_v, hv, "C++ vertices")
    assert_bits_equal(got_t, ht, "C++ triangles")
