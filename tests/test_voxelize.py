"""The voxeliser without a GPU: the Python-integer restatement of its rule (tests/voxelize_np.py) against itself across the
three ray axes and against the analytic sphere; the host entries (quantisation, edge census) against numpy; the PLY reader;
the program's bounds arithmetic and MRC writer; the C++ face under -Wall -Werror."""
import os
import subprocess

import numpy as np
import pytest

import volgen
import voxelize_cases as VC
import voxelize_np as VN
from conftest import ROOT, assert_bits_equal


@pytest.fixture(scope="module")
def api():
    from visfd_amd import api
    api.load_library()
    return api


_ORACLE = {}


def oracle(name, key, axis=0):
    """one evaluation per (mesh, shape, axis), shared and never modified"""
    k = (name, key, axis)
    if k not in _ORACLE:
        v, t = VC.CLOSED[name][key]()
        _ORACLE[k] = VN.voxelize(v, t, VC.SHAPES[key], axis=axis)
        _ORACLE[k][0].setflags(write=False)
    return _ORACLE[k]


# ---- the rule against itself ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", sorted(VC.SHAPES))
@pytest.mark.parametrize("name", sorted(VC.OFF_GRID))
def test_off_grid_meshes_agree_across_ray_axes(name, key):
    """No sample of these meshes lies exactly on the surface, so rays along x, y and z must give the same image bit for bit."""
    v, t = VC.OFF_GRID[name][key]()
    assert not VN.on_surface(VN.quantize(v), t, VC.SHAPES[key]).any()
    x, crossings, _skipped, odd = oracle(name, key, 0)
    assert crossings > 0 and odd == 0 and 0 < x.sum() < x.size
    for axis in (1, 2):
        y, _c, _s, odd = oracle(name, key, axis)
        assert odd == 0
        assert_bits_equal(y, x, "%s %s axis %d" % (name, key, axis))


@pytest.mark.parametrize("key", sorted(VC.SHAPES))
@pytest.mark.parametrize("name", sorted(VC.ON_GRID))
def test_on_grid_meshes_differ_across_ray_axes_on_the_surface_only(name, key):
    """Corners on samples: the three ray axes may disagree, but only on samples that lie exactly on the surface, and the set
    left out of the comparison is exactly that set."""
    v, t = VC.ON_GRID[name][key]()
    surf = VN.on_surface(VN.quantize(v), t, VC.SHAPES[key])
    assert surf.sum() > 0
    imgs = [oracle(name, key, axis)[0] for axis in (0, 1, 2)]
    for axis in (1, 2):
        differ = imgs[axis] != imgs[0]
        assert not (differ & ~surf).any(), "axes %d and 0 differ off the surface" % axis
    # the on-surface set is exact: the closed box's / octahedron's own description gives the same samples
    nz, ny, nx = VC.SHAPES[key]
    iz, iy, ix = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    lo, hi = v.min(0), v.max(0)
    if name == "box_on_samples":
        inside = (ix >= lo[0]) & (ix <= hi[0]) & (iy >= lo[1]) & (iy <= hi[1]) & (iz >= lo[2]) & (iz <= hi[2])
        strictly = (ix > lo[0]) & (ix < hi[0]) & (iy > lo[1]) & (iy < hi[1]) & (iz > lo[2]) & (iz < hi[2])
        want = inside & ~strictly
    else:
        c, r = (lo + hi) / 2, (hi - lo) / 2
        # |x|/rx + |y|/ry + |z|/rz == 1 in integers: multiply by rx ry rz
        R = [int(x) for x in r]
        lhs = np.abs(ix - int(c[0])) * R[1] * R[2] + np.abs(iy - int(c[1])) * R[0] * R[2] + np.abs(iz - int(c[2])) * R[0] * R[1]
        want = lhs == R[0] * R[1] * R[2]
    assert np.array_equal(surf, want)
    off = ~surf
    assert_bits_equal(imgs[1][off], imgs[0][off], "off-surface samples")
    assert_bits_equal(imgs[2][off], imgs[0][off], "off-surface samples")


def test_prototype_figures():
    for name, n in VC.PROTOTYPE_INSIDE.items():
        assert int(oracle(name, "s20")[0].sum()) == n


def test_coarse_icosphere_against_the_analytic_sphere():
    """An icosphere lies inside its sphere and, at two subdivisions, outside 0.97 of it."""
    img = oracle("icosphere_coarse", "s20")[0]
    nz, ny, nx = VC.SHAPES["s20"]
    iz, iy, ix = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    d = np.sqrt((ix - 9.21) ** 2 + (iy - 8.13) ** 2 + (iz - 6.4) ** 2)
    assert (img[d < 0.97 * 5.37] == 1).all()
    assert (img[d > 5.37] == 0).all()
    assert 0 < img.sum()


def test_special_meshes_in_the_oracle():
    shape = VC.SHAPES["s20"]
    v, t = VC.box_open()
    img, _c, skipped, odd = VN.voxelize(v, t, shape)
    assert odd == 13 * 6 and skipped == 8
    v, t = VC.box_with_sliver()
    q = VN.quantize(v)
    img, _c, skipped, odd = VN.voxelize_q(q, t, shape)
    assert skipped == 9 and odd == 0 and img.sum() == 13 * 13 * 6
    assert VN.edges(t, len(v)) == (0, 0)


# ---- host entries -------------------------------------------------------------------------------------------------------------
def test_quantiser_matches_numpy_bit_for_bit(api):
    rng = np.random.default_rng(5)
    v = (rng.standard_normal((4000, 3)) * 300).astype(np.float32)
    # ties: multiples of 1/2048 quantise to .5 exactly; negative ones too
    ties = (np.arange(-60, 60, dtype=np.float64)[:, None] * 2 + 1) / 2048.0 + np.array([0.0, 7.0, -3.0])
    v = np.concatenate([v, ties.astype(np.float32)]).astype(np.float32)
    for w, origin in ((1.0, (0, 0, 0)), (19.6, (1.5, -2.25, 0.5)), (0.37, (-100.125, 3.0, 1e-3)), (-2.0, (0, 0, 0))):
        want = VN.quantize(v, w, origin)
        got = api.voxelize_quantize_host(v, w, origin)
        assert got.dtype == np.int32 and np.array_equal(got.astype(np.int64), want), (w, origin)
    q = api.voxelize_quantize_host(ties.astype(np.float32)[:, :1].repeat(3, 1))
    assert (q % 2 == 0).all(), "ties go to even"
    assert (q < 0).any() and (q > 0).any()


@pytest.mark.parametrize("bad", [
    dict(v=[[524288.0625, 0, 0]]), dict(v=[[0, -524289.0, 0]]), dict(v=[[np.nan, 0, 0]]), dict(v=[[0, np.inf, 0]]),
    dict(v=[[1, 1, 1]], w=0.0), dict(v=[[1, 1, 1]], w=np.inf), dict(v=[[1, 1, 1]], w=np.nan), dict(v=[[1, 1, 1]], w=1e-6),
    dict(v=[[1, 1, 1]], origin=(0, np.nan, 0))])
def test_quantiser_refusals(api, bad):
    v, w, origin = np.asarray(bad["v"], np.float32), bad.get("w", 1.0), bad.get("origin", (0, 0, 0))
    with pytest.raises(VN.Refused):
        VN.quantize(v, w, origin)
    with pytest.raises(api.VisfdHipError) as e:
        api.voxelize_quantize_host(v, w, origin)
    assert e.value.code == 1


def test_quantiser_accepts_the_limit(api):
    v = np.array([[524288.0, -524288.0, 0.0]], np.float32)
    assert api.voxelize_quantize_host(v).tolist() == [[2 ** 29, -2 ** 29, 0]]


def test_edge_census(api):
    for make, want in ((VC.OFF_GRID["box_off_grid"]["s20"], (0, 0)), (VC.OFF_GRID["torus"]["s20"], (0, 0)),
                       (VC.OFF_GRID["icosphere_fine"]["s20"], (0, 0)), (VC.box_with_sliver, (0, 0)), (VC.box_open, (4, 0)),
                       (VC.box_duplicated, (0, 3))):
        v, t = make()
        assert VN.edges(t, len(v)) == want
        assert api.mesh_edges_host(t, len(v)) == want
    v, t = VC.box_open()
    t2 = np.concatenate([t, t[:1], t[:1]])      # open and non-manifold at once
    assert api.mesh_edges_host(t2, len(v)) == VN.edges(t2, len(v)) == (4, 3)
    for bad in ([[0, 1, 8]], [[0, -1, 2]]):
        with pytest.raises(api.VisfdHipError):
            api.mesh_edges_host(np.array(bad, np.int32), 8)
    assert api.mesh_edges_host(np.zeros((0, 3), np.int32), 0) == (0, 0)


# ---- PLY ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", ["ascii", "binary_little_endian", "binary_big_endian"])
def test_ply_round_trips(fmt, tmp_path):
    from visfd_amd import ply
    v, t = VC.OFF_GRID["icosphere_coarse"]["s20"]()
    p = str(tmp_path / "a.ply")
    ply.write_ply(p, v, t.tolist(), fmt)
    v2, t2 = ply.read_ply(p)
    assert v2.dtype == np.float32 and t2.dtype == np.int32
    assert_bits_equal(v2, v, fmt)
    assert np.array_equal(t2, t)
    # extra vertex properties of several widths, the other list name, other integer types, quadrilaterals
    vq, quads = VC.box_quads()
    extra = [("nx", "float", np.arange(8) * 0.5), ("red", "uchar", np.arange(8) * 30), ("quality", "double", np.arange(8) / 7.0),
             ("flags", "short", -np.arange(8))]
    ply.write_ply(p, vq, quads, fmt, extra, index_name="vertex_index", count_type="ushort", index_type="uint")
    v3, t3 = ply.read_ply(p)
    assert_bits_equal(v3, vq, fmt + " quads")
    assert np.array_equal(t3, VC.box((2.3, 1.7, 3.1), (15.6, 14.2, 9.9))[1]), "fans from corner 0"
    # mixed polygons: a triangle, a quad and a pentagon
    ply.write_ply(p, vq, [[0, 1, 2], [0, 2, 6, 4], [0, 1, 3, 7, 5]], fmt)
    assert ply.read_ply(p)[1].tolist() == [[0, 1, 2], [0, 2, 6], [0, 6, 4], [0, 1, 3], [0, 3, 7], [0, 7, 5]]


def test_ply_refuses_what_it_cannot_read(tmp_path):
    from visfd_amd import ply
    p = tmp_path / "bad.ply"
    p.write_bytes(b"plx\n")
    with pytest.raises(ply.PlyError):
        ply.read_ply(str(p))
    p.write_bytes(b"ply\nformat binary_little_endian 1.0\nelement vertex 2\nproperty float x\nproperty float y\n"
                  b"property float z\nend_header\n\0\0\0\0")
    with pytest.raises(ply.PlyError):
        ply.read_ply(str(p))


# ---- the program's arithmetic -----------------------------------------------------------------------------------------------------
def test_program_bounds_arithmetic():
    from visfd_amd import voxelize_mesh as P
    hdr = {"n": (20, 17, 13), "m": (20, 17, 13), "cella": (392.0, 333.2, 254.8), "cellb": (90.0, 90.0, 90.0), "origin": (0.0, 0.0, 0.0)}
    w, b, n, origin, from_file = P.plan(hdr)
    assert from_file and w == 392.0 / 20 and n == (20, 17, 13) and origin == (0.0, 0.0, 0.0)
    assert n == tuple(len(np.arange(b[2 * d], b[2 * d + 1], w)) for d in range(3))
    # -w beats the header's width; -s moves the mesh, so voxel 0 sits at -s
    w, b, n, origin, from_file = P.plan(hdr, width=10.0, shift=(0.5, 0.5, 0.5))
    assert not from_file and w == 10.0 and n == (20, 17, 13) and origin == (-0.5, -0.5, -0.5)
    # -c: (c_min w, (c_max + 0.99) w), as the script computes it (its documentation's example is one voxel off)
    w, b, n, origin, _ = P.plan(hdr, width=2.0, crop=(3, 10, 0, 4, 2, 2))
    assert b == (6.0, 10.99 * 2.0, 0.0, 4.99 * 2.0, 4.0, 2.99 * 2.0)
    assert n == tuple(len(np.arange(b[2 * d], b[2 * d + 1], w)) for d in range(3)) == (8, 5, 1)
    assert origin == (3.0, 0.0, 2.0)
    # -b as given, overriding -i; without any width, 1
    w, b, n, origin, _ = P.plan(None, bounds=(0.5, 7.25, -2, 2, 0, 3))
    assert w == 1.0 and n == (7, 4, 3) and origin == (0.5, -2.0, 0.0)
    w, b, n, origin, _ = P.plan(hdr, bounds=(0, 40, 0, 40, 0, 40))
    assert n == tuple(len(np.arange(0, 40, w)) for _ in range(3))
    for kw in (dict(width=0.0), dict()):
        with pytest.raises(P.InputError):
            P.plan(None, **kw)
    with pytest.raises(P.InputError) as e:
        P.plan(hdr, width=0.0)
    assert "voxel width" in str(e.value)


def test_program_mrc_round_trip(tmp_path):
    from visfd_amd import voxelize_mesh as P
    vol = oracle("torus", "s20")[0]
    p = str(tmp_path / "mask.rec")
    P.write_mrc_bytes(p, vol, (39.2, 33.32, 25.48), origin=(1.0, 2.0, 3.0))
    assert os.path.getsize(p) == 1024 + vol.size
    assert_bits_equal(volgen.read_mrc(p), np.ascontiguousarray(vol), "mode-0 round trip")
    h = P.read_mrc_header(p)
    assert h["n"] == (20, 17, 13) and h["origin"] == (1.0, 2.0, 3.0)
    assert np.allclose(h["cella"], (39.2, 33.32, 25.48), rtol=1e-6)
    src = str(tmp_path / "src.mrc")
    volgen.write_mrc(src, np.zeros((13, 17, 20), np.float32), voxel_width=19.6)
    h = P.read_mrc_header(src)
    assert h["n"] == h["m"] == (20, 17, 13) and abs(h["cella"][0] / h["m"][0] - 19.6) < 1e-5


def test_program_refuses_before_touching_the_device(tmp_path):
    from visfd_amd import voxelize_mesh as P, ply
    v, t = VC.box_open()
    mesh = str(tmp_path / "open.ply")
    ply.write_ply(mesh, v, t.tolist())
    assert P.main(["-m", mesh, "-o", "same.rec", "-i", "same.rec"]) == 1
    assert P.main(["-m", mesh, "-o", str(tmp_path / "o.rec"), "-w", "0", "-b", "0", "9", "0", "9", "0", "9"]) == 1
    assert P.main(["-m", mesh, "-o", str(tmp_path / "o.rec"), "-b", "0", "20", "0", "17", "0", "13"]) == 1   # open mesh
    assert not os.path.exists(str(tmp_path / "o.rec"))


# ---- the C++ face ---------------------------------------------------------------------------------------------------------------
def test_cpp_shim_compiles(api, tmp_path):
    exe = str(tmp_path / "shim_voxelize_check")
    libdir = os.path.dirname(api.LIB_PATH)
    r = subprocess.run(["g++", "-std=c++11", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                        os.path.join(ROOT, "tests", "shim_voxelize_check.cpp"), "-L" + libdir, "-lvisfd_hip",
                        "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib", "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
