"""VoxelizeMesh on the GPU (csrc/voxelize.hip) against the Python-integer restatement of its rule (tests/voxelize_np.py, checked
against itself in test_voxelize.py).  Every comparison is bitwise."""
import os
import subprocess
import sys

import numpy as np
import pytest

import volgen
import voxelize_cases as VC
import voxelize_np as VN
from conftest import ROOT, assert_bits_equal

pytestmark = pytest.mark.gpu

CLI = os.path.join(ROOT, "visfd_amd", "cli", "filter_mrc")
EINVAL = 1


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


_ORACLE = {}


def oracle(name, key):
    if (name, key) not in _ORACLE:
        v, t = VC.CLOSED[name][key]()
        _ORACLE[name, key] = VN.voxelize(v, t, VC.SHAPES[key])
        _ORACLE[name, key][0].setflags(write=False)
    return _ORACLE[name, key]


def check_stats(ctx, want, what):
    img, crossings, skipped, odd = want
    assert ctx.voxelize_last() == (crossings, skipped, odd, int(img.sum())), what


@pytest.mark.parametrize("key", sorted(VC.SHAPES))
@pytest.mark.parametrize("name", sorted(VC.CLOSED))
def test_closed_meshes_match_the_rule_on_both_faces(ctx, torch, name, key):
    v, t = VC.CLOSED[name][key]()
    want = oracle(name, key)
    assert want[3] == 0
    got = ctx.voxelize_mesh(v, t, VC.SHAPES[key])
    assert_bits_equal(got, want[0], "%s %s" % (name, key))
    check_stats(ctx, want, "host face")
    d = torch.full(VC.SHAPES[key], float("nan"), device="cuda")
    torch.cuda.synchronize()   # the context runs on a stream of its own
    ctx.voxelize_mesh_dev(d, v, t)
    assert_bits_equal(d.cpu().numpy(), want[0], "%s %s (device face)" % (name, key))
    check_stats(ctx, want, "device face")


@pytest.mark.parametrize("name", ["box_beyond_image", "icosphere_fine", "octahedron_on_samples", "octahedron_huge"])
def test_bisected_crossings_give_the_same_image(ctx, name):
    """option voxelize_bisect: the sample behind every crossing from the exact sign alone (the path the double estimate
    falls back to) -- the tiled path, the one-lane path, crossings exactly on samples, and 90-bit plane functions"""
    v, t = VC.CLOSED[name]["s70"]()
    want = oracle(name, "s70")
    with ctx.options(voxelize_bisect=1):
        assert_bits_equal(ctx.voxelize_mesh(v, t, VC.SHAPES["s70"]), want[0], name + " bisected")
        check_stats(ctx, want, name + " bisected")


@pytest.mark.parametrize("nx", [2100, 2102])
def test_rows_longer_than_one_chunk_of_toggle_words(ctx, nx):
    """More than 64 toggle words per row: the fill carries the parity from one chunk of 2048 samples into the next; with
    16-byte stores (nx = 2100) and without.  Two disjoint boxes: one across the chunk seam, one past it."""
    shape = (2, 3, nx)
    va, ta = VC.box((100.3, 0.4, 0.3), (2090.6, 2.2, 1.7))
    vb, tb = VC.box((2092.5, -1.0, -1.0), (2098.5, 1.5, 0.5))
    v, t = np.concatenate([va, vb]), np.concatenate([ta, tb + len(va)])
    want = VN.voxelize(v, t, shape)
    assert want[3] == 0 and want[0][1, 1, 2047:2050].tolist() == [1, 1, 1] and want[0].sum() == 1990 * 2 + 6 * 2
    assert_bits_equal(ctx.voxelize_mesh(v, t, shape), want[0], "nx = %d" % nx)
    check_stats(ctx, want, "nx = %d" % nx)


def test_device_face_with_an_unaligned_destination(ctx, torch):
    """nx a multiple of 4 but dst only 4-byte aligned: the fill must not use its 16-byte stores"""
    v, t = VC.CLOSED["torus"]["s20"]()
    shape = VC.SHAPES["s20"]
    n = int(np.prod(shape))
    buf = torch.full((n + 1,), float("nan"), device="cuda")
    torch.cuda.synchronize()
    ctx.voxelize_mesh_dev(buf[1:].view(shape), v, t)
    assert_bits_equal(buf[1:].cpu().numpy().reshape(shape), oracle("torus", "s20")[0], "dst 4 bytes past a 16-byte boundary")
    assert np.isnan(buf[:1].cpu().numpy()).all()


def test_same_call_twice_gives_the_same_bits(ctx):
    v, t = VC.CLOSED["icosphere_fine"]["s70"]()
    first = ctx.voxelize_mesh(v, t, VC.SHAPES["s70"])
    for _ in range(2):
        assert_bits_equal(ctx.voxelize_mesh(v, t, VC.SHAPES["s70"]), first, "repeat")


def test_voxel_width_and_origin(ctx):
    w, origin = 19.6, (1.5, -2.25, 0.5)
    v, t = VC.CLOSED["torus"]["s20"]()
    phys = ((v.astype(np.float64) + np.array(origin)) * w).astype(np.float32)
    want = VN.voxelize(phys, t, VC.SHAPES["s20"], w, origin)
    assert want[3] == 0 and 400 < want[0].sum() < 600
    assert_bits_equal(ctx.voxelize_mesh(phys, t, VC.SHAPES["s20"], w, origin), want[0], "w = 19.6 with an origin")
    check_stats(ctx, want, "w = 19.6 with an origin")


@pytest.mark.parametrize("make,open_", [(VC.box_open, True), (VC.box_duplicated, False)])
def test_open_and_duplicated_meshes(ctx, make, open_):
    from visfd_amd import api
    v, t = make()
    shape = VC.SHAPES["s20"]
    with pytest.raises(api.VisfdHipError) as e:
        ctx.voxelize_mesh(v, t, shape, check_closed=True)
    nb, nn = VN.edges(t, len(v))
    assert e.value.code == EINVAL and ("%d boundary" % nb) in str(e.value) and ("%d non-manifold" % nn) in str(e.value)
    want = VN.voxelize(v, t, shape)
    assert_bits_equal(ctx.voxelize_mesh(v, t, shape, check_closed=False), want[0], "unchecked")
    check_stats(ctx, want, "unchecked")
    if open_:
        assert ctx.voxelize_last()[2] > 0


def test_zero_area_triangle_is_skipped(ctx):
    v, t = VC.box_with_sliver()
    want = VN.voxelize(v, t, VC.SHAPES["s20"])
    assert want[2] == 9
    assert_bits_equal(ctx.voxelize_mesh(v, t, VC.SHAPES["s20"]), want[0], "sliver")
    check_stats(ctx, want, "sliver")


def _raw(ctx, v, t, shape, w=1.0, n_vertices=None, dst=None):
    from visfd_amd import api
    import ctypes as C
    nz, ny, nx = shape
    v = np.ascontiguousarray(v, np.float32)
    t = np.ascontiguousarray(t, np.int32)
    return ctx._L.visfd_hip_voxelize_mesh(ctx._h, v.ctypes.data, len(v) if n_vertices is None else n_vertices, t.ctypes.data,
                                          len(t), float(w), (C.c_double * 3)(0, 0, 0), nx, ny, nz, 1,
                                          None if dst is None else api._np(dst))


def test_refusals_leave_dst_alone(ctx):
    v, t = VC.CLOSED["box_off_grid"]["s20"]()
    shape = VC.SHAPES["s20"]
    dst = np.full(shape, 123.0, np.float32)
    for bad in (np.nan, np.inf, -np.inf):
        vb = v.copy()
        vb[3, 1] = bad
        assert _raw(ctx, vb, t, shape, dst=dst) == EINVAL
    tb = t.copy()
    tb[5, 2] = 8
    assert _raw(ctx, v, tb, shape, dst=dst) == EINVAL
    tb[5, 2] = -1
    assert _raw(ctx, v, tb, shape, dst=dst) == EINVAL
    assert _raw(ctx, v, t, shape, w=0.0, dst=dst) == EINVAL
    assert _raw(ctx, v, t, shape, w=float("nan"), dst=dst) == EINVAL
    vb = v.copy()
    vb[0, 0] = 6e5                                                    # beyond 2^29 / 1024 voxels
    assert _raw(ctx, vb, t, shape, dst=dst) == EINVAL
    assert _raw(ctx, v, t, (1, 1, 2 ** 19), dst=dst) == EINVAL        # nx >= 2^19 (refused before dst is looked at)
    assert _raw(ctx, v, t, (2 ** 11, 2 ** 10, 2 ** 10), dst=dst) == EINVAL   # 2^31 voxels
    assert _raw(ctx, v, t, (0, 17, 20), dst=dst) == EINVAL
    assert _raw(ctx, v, t, shape, dst=None) == EINVAL
    assert (dst == 123.0).all(), "a refused call wrote to dst"


def test_empty_mesh_gives_an_empty_image(ctx):
    got = ctx.voxelize_mesh(np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32), (3, 4, 5))
    assert got.shape == (3, 4, 5) and (got == 0).all()
    assert ctx.voxelize_last() == (0, 0, 0, 0)


def test_voxelize_between_two_gaussians(ctx):
    """workspace reuse: the Gaussian before and after is the same, also across a trim and a poisoned workspace"""
    src = volgen.noise_volume((12, 14, 16), seed=78)
    first, _ = ctx.gauss_ratio(src, (1.5, 1.5, 1.5), 2.5)
    v, t = VC.CLOSED["box_beyond_image"]["s70"]()
    want = oracle("box_beyond_image", "s70")[0]
    assert_bits_equal(ctx.voxelize_mesh(v, t, VC.SHAPES["s70"]), want, "between Gaussians")
    again, _ = ctx.gauss_ratio(src, (1.5, 1.5, 1.5), 2.5)
    assert_bits_equal(again, first, "Gaussian after a voxelisation")
    ctx.trim()
    assert ctx.workspace_bytes() == 0
    assert_bits_equal(ctx.voxelize_mesh(v, t, VC.SHAPES["s70"]), want, "after trim")
    ctx.debug_poison_workspace()
    assert_bits_equal(ctx.voxelize_mesh(v, t, VC.SHAPES["s70"]), want, "after poisoning the workspace")


def test_voxelize_time_option_reports_three_phases(ctx):
    v, t = VC.CLOSED["torus"]["s70"]()
    assert ctx.get_option("voxelize_time") == 0
    with ctx.options(voxelize_time=1):
        assert_bits_equal(ctx.voxelize_mesh(v, t, VC.SHAPES["s70"]), oracle("torus", "s70")[0], "timed call")
        ms = ctx.voxelize_last_times()
    assert len(ms) == 3 and all(0.0 <= x < 1000.0 for x in ms), ms


# ---- the program ---------------------------------------------------------------------------------------------------------------
def _program(args, cwd):
    return subprocess.run([sys.executable, "-m", "visfd_amd.voxelize_mesh"] + args, cwd=cwd, capture_output=True, text=True,
                          env=dict(os.environ, PYTHONPATH=ROOT), timeout=300)


def test_program_end_to_end(tmp_path):
    from visfd_amd import ply, voxelize_mesh as P
    d = str(tmp_path)
    w = 19.6
    shape = VC.SHAPES["s20"]
    v, t = VC.CLOSED["torus"]["s20"]()
    phys = (v.astype(np.float64) * w).astype(np.float32)
    ply.write_ply(os.path.join(d, "bin.ply"), phys, t.tolist(), "binary_little_endian")
    ply.write_ply(os.path.join(d, "asc.ply"), phys, t.tolist(), "ascii")
    image = volgen.noise_volume(shape, seed=79)
    volgen.write_mrc(os.path.join(d, "orig.rec"), image, voxel_width=w)

    # -i: the size and the voxel width of the original image
    hdr = P.read_mrc_header(os.path.join(d, "orig.rec"))
    wi, _b, n, origin, _ = P.plan(hdr)
    r = _program(["-m", "bin.ply", "-o", "mask_i.rec", "-i", "orig.rec"], d)
    assert r.returncode == 0, r.stderr[-2000:]
    got = volgen.read_mrc(os.path.join(d, "mask_i.rec"))
    want = VN.voxelize(phys, t, (n[2], n[1], n[0]), wi, origin)[0]
    assert n == (20, 17, 13) and 400 < want.sum() < 600
    assert_bits_equal(got, want, "-i")
    assert P.read_mrc_header(os.path.join(d, "mask_i.rec"))["cella"] == hdr["cella"]

    # ascii mesh, -w, -c and -s
    crop = (2, 17, 1, 15, 3, 10)
    wc, _b, n, origin, _ = P.plan(None, w, crop, None, (0.5, 0.5, 0.5))
    r = _program(["-m", "asc.ply", "-o", "mask_c.rec", "-w", repr(w), "-s", "0.5", "0.5", "0.5", "-c"] + [str(c) for c in crop], d)
    assert r.returncode == 0, r.stderr[-2000:]
    got_c = volgen.read_mrc(os.path.join(d, "mask_c.rec"))
    want_c = VN.voxelize(phys, t, (n[2], n[1], n[0]), wc, origin)[0]
    assert n == (16, 15, 8) and want_c.sum() > 100
    assert_bits_equal(got_c, want_c, "-c with -s")
    assert not np.array_equal(want_c, want[3:11, 1:16, 2:18]), "the half-voxel shift must show"

    # refusals, in the reference's wording where it has one
    r = _program(["-m", "bin.ply", "-o", "orig.rec", "-i", "orig.rec"], d)
    assert r.returncode != 0 and "Input and output image files cannot have the same name" in r.stderr
    r = _program(["-m", "bin.ply", "-o", "x.rec", "-i", "orig.rec", "-w", "0"], d)
    assert r.returncode != 0 and "voxel width cannot be non-zero" in r.stderr
    vo, to = VC.box_open()
    ply.write_ply(os.path.join(d, "open.ply"), vo, to.tolist())
    r = _program(["-m", "open.ply", "-o", "x.rec", "-b", "0", "20", "0", "17", "0", "13"], d)
    assert r.returncode != 0 and "not closed" in r.stderr and not os.path.exists(os.path.join(d, "x.rec"))

    # the image is a mask filter_mrc accepts: the masked Gaussian is the one the same mask gives as a float image, and
    # not the unmasked one
    volgen.write_mrc(os.path.join(d, "mask_float.rec"), want, voxel_width=w)
    g = {}
    for name, mask in (("bytes", ["-mask", "mask_i.rec"]), ("floats", ["-mask", "mask_float.rec"]), ("none", [])):
        r = subprocess.run([CLI, "-in", "orig.rec", "-out", name + ".rec", "-w", repr(w), "-gauss", repr(2 * w)] + mask,
                           cwd=d, capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-2000:]
        g[name] = volgen.read_mrc(os.path.join(d, name + ".rec"))
    assert_bits_equal(g["bytes"], g["floats"], "-mask with the program's image")
    assert not np.array_equal(g["bytes"], g["none"])


def test_shim_program_runs(tmp_path):
    exe = str(tmp_path / "shim_voxelize_check")
    libdir = os.path.join(ROOT, "visfd_amd")
    subprocess.check_call(["g++", "-std=c++11", "-O1", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "shim_voxelize_check.cpp"), "-o", exe, "-L" + libdir, "-lvisfd_hip",
                           "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "shim voxelize check ok" in r.stdout, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
    assert "inside 1014\n" in r.stdout and "shifted inside 1014 first 1\n" in r.stdout and "open odd rows 78\n" in r.stdout
