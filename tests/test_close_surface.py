"""close_surface without a GPU: the exact part of the definition (the integer splat) pinned through the
host entry, the numpy restatement held to the geometric conditions it is the yardstick for, the PLY reader and the
command line's arithmetic, and each checker shown to trip on a mutant."""
import os

import numpy as np
import pytest

import close_surface_np as R
from close_surface_cases import CASES, SPHERE_CASES
from conftest import assert_bits_equal

EINVAL = 1


@pytest.fixture(scope="module")
def api():
    from visfd_amd import api
    return api


@pytest.mark.parametrize("name", sorted(CASES))
def test_splat_host_equals_the_python_integer_splat(api, name):
    c = CASES[name]
    ref = R.reference(c)
    acc, used, skipped = api.close_surface_splat_host(c.points, c.normals, c.shape, c.pad)
    assert (used, skipped) == (ref.n_used, ref.n_skipped) == (c.n_used, c.n_skipped)
    assert_bits_equal(acc, ref.acc, name)
    if name != "empty":
        assert np.abs(acc).sum() > 0


def test_splat_host_refusals(api):
    p, n = CASES["tiny"].points, CASES["tiny"].normals
    L = api.load_library()
    acc = np.zeros((3, 3, 4, 5), np.int64)
    for args in ((p.ctypes.data, n.ctypes.data, 2, 5, 4, 2, 0), (p.ctypes.data, n.ctypes.data, 2, 5, 4, 3, -1),
                 (p.ctypes.data, n.ctypes.data, -1, 5, 4, 3, 0), (None, n.ctypes.data, 2, 5, 4, 3, 0),
                 (p.ctypes.data, None, 2, 5, 4, 3, 0)):
        assert L.visfd_hip_close_surface_splat_host(*(args + (acc.ctypes.data, None))) == EINVAL
    assert L.visfd_hip_close_surface_splat_host(p.ctypes.data, n.ctypes.data, 2, 5, 4, 3, 0, None, None) == EINVAL
    assert L.visfd_hip_close_surface_splat_host(None, None, 0, 5, 4, 3, 0, acc.ctypes.data, None) == 0


@pytest.mark.parametrize("name", SPHERE_CASES)
def test_restatement_meets_the_geometric_conditions(name):
    c = CASES[name]
    g = R.check_geometry(R.reference(c).mask, c)
    print(name, g)


@pytest.mark.parametrize("name", sorted(set(CASES) - {"empty"}))
def test_restatement_solves_its_equation(name):
    ref = R.reference(CASES[name])
    assert R.residual_ratio(ref.chi, ref.b) < 1e-12


@pytest.mark.parametrize("name", SPHERE_CASES + ("inward", "junk"))
def test_restatement_band_is_a_small_part_of_its_mask(name):
    """the voxels within 1e-3 of the range of the level: the only ones on which a float32 solve may cut differently"""
    ref = R.reference(CASES[name])
    nb = int(R.band(R.image_of(ref.chi, ref.pad), ref.iso, ref.range).sum())
    assert nb <= 0.01 * ref.mask.sum(), (nb, ref.mask.sum())


def test_orientation_auto_and_inward():
    c = CASES["inward"]
    ref = R.reference(c)
    assert_bits_equal(ref.mask, R.reference(CASES["caps75"]).mask, "negated normals, inward")
    m, taken = R.cut(ref.chi, ref.iso, c.pad, "auto")
    assert taken == "inward"
    assert_bits_equal(m, ref.mask, "auto")
    assert R.cut(R.reference(CASES["caps75"]).chi, R.reference(CASES["caps75"]).iso, 0, "auto")[1] == "outward"


def test_junk_moves_nothing_but_the_counts():
    a, b = R.reference(CASES["junk"]), R.reference(CASES["caps75"])
    assert_bits_equal(a.acc, b.acc, "skipped points and null normals add nothing")
    assert (a.n_used, a.n_skipped) == (b.n_used + 2, 16)


# ---- the PLY reader and the command line ------------------------------------------------------------------------------------
def _write_normals_file(path, p, n):
    """what filter_mrc -normals-file writes (cli/filter_mrc.cpp: write_normals_file)"""
    with open(path, "w") as f:
        f.write("ply\nformat ascii 1.0\ncomment  created by visfd\nelement vertex %d\nproperty float x\nproperty float y\n"
                "property float z\nproperty float nx\nproperty float ny\nproperty float nz\nend_header\n" % len(p))
        for a, b in zip(p, n):
            f.write(" ".join("%.9g" % v for v in list(a) + list(b)) + "\n")


def test_read_ply_points(tmp_path):
    from visfd_amd import ply
    c = CASES["odd"]
    _write_normals_file(str(tmp_path / "a.ply"), c.points, c.normals)
    p, n = ply.read_ply_points(str(tmp_path / "a.ply"))
    assert_bits_equal(p, c.points, "ascii points")
    assert_bits_equal(n, c.normals, "ascii normals")
    extra = [("quality", "uchar", np.arange(len(c.points)) % 256)] + [(k, "float", c.normals[:, d]) for d, k in
                                                                      enumerate(("nx", "ny", "nz"))]
    for fmt in ("binary_little_endian", "binary_big_endian", "ascii"):
        path = str(tmp_path / (fmt + ".ply"))
        ply.write_ply(path, c.points, [[0, 1, 2]], fmt, extra=extra)
        p, n = ply.read_ply_points(path)
        assert_bits_equal(p, c.points, fmt)
        assert_bits_equal(n, c.normals, fmt)
    ply.write_ply(str(tmp_path / "mesh.ply"), c.points, [[0, 1, 2]], "binary_little_endian")
    with pytest.raises(ply.PlyError):
        ply.read_ply_points(str(tmp_path / "mesh.ply"))
    ply.write_ply(str(tmp_path / "mesh_a.ply"), c.points, [[0, 1, 2]], "ascii", extra=extra[:3])
    with pytest.raises(ply.PlyError):
        ply.read_ply_points(str(tmp_path / "mesh_a.ply"))
    _write_normals_file(str(tmp_path / "none.ply"), c.points[:0], c.normals[:0])
    p, n = ply.read_ply_points(str(tmp_path / "none.ply"))
    assert p.shape == n.shape == (0, 3)


def test_command_line_arithmetic_agrees_with_voxelize_mesh():
    from visfd_amd import close_surface as T, voxelize_mesh as P
    for n, w in (((40, 36, 44), 12.0), ((37, 33, 3), 19.6), ((48, 48, 48), 0.1), ((101, 7, 13), 3.3)):
        hdr = {"n": n, "m": n, "cella": tuple(np.float32(w) * np.float32(k) for k in n), "cellb": (90.0, 90.0, 90.0),
               "origin": (0.0, 0.0, 0.0)}
        for width in (None, 2.5, w):
            pw, _b, pn, _o, _f = P.plan(hdr, width)
            assert T.plan_cloud(hdr, width) == (pw, pn)
            assert T.plan_cloud(hdr, width, (5, 6, 7)) == (pw, (5, 6, 7))
    assert T.plan_cloud(None, None, (5, 6, 7)) == (1.0, (5, 6, 7))
    assert T.plan_cloud(None, 4.0, (5, 6, 7)) == (4.0, (5, 6, 7))
    with pytest.raises(P.InputError):
        T.plan_cloud(None, None, None)
    with pytest.raises(P.InputError):
        T.plan_cloud(None, 0.0, (5, 6, 7))


# ---- the checkers trip on mutants ---------------------------------------------------------------------------------------------
def test_checkers_trip_on_mutants():
    c = CASES["caps75"]
    ref = R.reference(c)
    R.check_geometry(ref.mask, c)
    R.check_mask_against(ref.mask, ref, "itself")
    shifted = np.roll(ref.mask, 1, axis=2)
    with pytest.raises(AssertionError):
        R.check_geometry(shifted, c)
    with pytest.raises(AssertionError):
        R.check_mask_against(shifted, ref, "shifted")
    flipped = R.cut(ref.chi, ref.iso, c.pad, "inward")[0]
    with pytest.raises(AssertionError):
        R.check_geometry(flipped, c)
    with pytest.raises(AssertionError):
        R.check_mask_against(flipped, ref, "flipped")
    t = CASES["thin"]
    dropped = R.acc_to_int64(R.splat_int(t.points, t.normals, t.shape, t.pad, drop=100)[0])
    with pytest.raises(AssertionError):
        assert_bits_equal(dropped, R.reference(t).acc, "one contribution dropped")
    assert int((dropped != R.reference(t).acc).sum()) == 1
