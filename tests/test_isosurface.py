"""The isosurface's host walk (visfd_hip_isosurface_host, csrc/isosurface.hip) against the Python restatement of the
definition (tests/isosurface_np.py), bit for bit, and both against what the definition promises: a closed, edge-manifold
mesh with outward normals whose voxelisation (tests/voxelize_np.py, the exact rule of the product's voxeliser) is the inside
set, voxel for voxel, at voxel widths 1 and 1.7.  No GPU needed.

The voxeliser's `skipped` count is not looked at: a triangle parallel to x has no projected area and is skipped by rule."""
import ctypes as C

import numpy as np
import pytest

import isosurface_np as R
import voxelize_np as V
from conftest import assert_bits_equal
from isosurface_cases import CASES, SIDES

EINVAL, ECAPACITY = 1, 4
WIDTHS = (1.0, 1.7)
SIDE_CODE = {"below": R.BELOW, "above": R.ABOVE}
PAIRS = [(c.name, s) for c in CASES for s in SIDES]
BY_NAME = {c.name: c for c in CASES}

_REF = {}


def reference(name, side):
    """the Python restatement's mesh of a case, computed once and frozen"""
    if (name, side) not in _REF:
        c = BY_NAME[name]
        v, t = R.isosurface(c.vol, c.iso, SIDE_CODE[side])
        v.setflags(write=False)
        t.setflags(write=False)
        _REF[(name, side)] = (v, t)
    return _REF[(name, side)]


@pytest.fixture(scope="module")
def api():
    from visfd_amd import api
    return api


@pytest.mark.parametrize("name,side", PAIRS)
def test_host_walk_equals_the_python_restatement(api, name, side):
    c = BY_NAME[name]
    rv, rt = reference(name, side)
    v, t = api.isosurface_host(c.vol, c.iso, side)
    assert (len(v), len(t)) == (len(rv), len(rt)), "counts"
    assert v.dtype == np.float32 and t.dtype == np.int32
    assert_bits_equal(v, rv, "%s %s vertices" % (name, side))
    assert_bits_equal(t, rt, "%s %s triangles" % (name, side))


def test_the_counts_the_definition_names(api):
    v, t = api.isosurface_host(BY_NAME["one"].vol, 0.5, "below")
    assert (len(v), len(t)) == (14, 24)
    # the node's 14 edges: 7 classes upwards and 7 downwards, every one at a border node, so every t is 0.5
    assert sorted(set(np.abs(v).ravel().tolist())) == [0.0, 0.5]
    for name, side in (("all_out", "below"), ("all_in", "above"), ("one", "above")):
        v, t = api.isosurface_host(BY_NAME[name].vol, BY_NAME[name].iso, side)
        assert (len(v), len(t)) == (0, 0), (name, side)
    v, t = api.isosurface_host(BY_NAME["all_in"].vol, 0.5, "below")
    assert len(v) > 0 and set(np.unique(v - np.floor(v)).tolist()) <= {0.0, 0.5}, "caps only: every vertex halfway to the border"


@pytest.mark.parametrize("name,side", PAIRS)
def test_mesh_is_closed_outward_and_voxelises_to_the_inside_set(name, side):
    c = BY_NAME[name]
    v, t = reference(name, side)
    inside = R.inside_set(c.vol, c.iso, SIDE_CODE[side])
    assert V.edges(t, len(v)) == (0, 0), "boundary / non-manifold edges"
    if inside.any():
        assert R.signed_volume(v, t) > 0.0
    else:
        assert len(v) == 0 and len(t) == 0
    for w in WIDTHS:
        img, _crossings, _skipped, odd_rows = V.voxelize(R.scale_vertices(v, w), t, c.vol.shape, voxel_width=w)
        assert odd_rows == 0, w
        assert np.array_equal(img != 0, inside), "width %g: %d voxels differ" % (w, int(((img != 0) != inside).sum()))


def test_the_clamp_keeps_vertices_off_the_nodes(api):
    c = BY_NAME["clamp"]
    v, _t = api.isosurface_host(c.vol, c.iso, "below")
    frac = (v - np.floor(v)).astype(np.float64)
    moved = frac[frac != 0.0]
    assert moved.min() == 1.0 / 64.0 and moved.max() == 63.0 / 64.0
    assert set(moved.tolist()) == {1.0 / 64.0, 63.0 / 64.0}, "no border edge in this case: every t was clamped"


def test_nan_and_infinite_neighbours_put_the_vertex_halfway(api):
    c = BY_NAME["special"]
    v, _t = reference("special", "below")
    # node (x 3, y 2, z 1) is inside and its x neighbour (2, 2, 1) is NaN: the vertex on that edge sits at x = 2.5
    assert any((row == np.array([2.5, 2.0, 1.0], np.float32)).all() for row in v)
    # (2, 1, 2) = -inf against (1, 1, 2) = +inf: inf / inf is not finite
    assert any((row == np.array([1.5, 1.0, 2.0], np.float32)).all() for row in v)
    assert np.isfinite(v).all()
    assert np.isnan(c.vol).sum() == 3 and np.isinf(c.vol).sum() == 8


def _raw(api, vol, iso, side, v, vcap, t, tcap, nv=True, nt=True):
    """the C entry itself -> (return code, n_vertices, n_triangles)"""
    L = api.load_library()
    a, b = C.c_int64(-5), C.c_int64(-5)
    nz, ny, nx = vol.shape if vol is not None else (1, 1, 1)
    rc = L.visfd_hip_isosurface_host(vol.ctypes.data if vol is not None else None, nx, ny, nz, iso, side,
                                     v.ctypes.data if v is not None else None, vcap,
                                     t.ctypes.data if t is not None else None, tcap,
                                     C.byref(a) if nv else None, C.byref(b) if nt else None)
    return rc, a.value, b.value


def test_caps_protocol(api):
    c = BY_NAME["noise345"]
    rv, rt = reference("noise345", "below")
    n, m = len(rv), len(rt)
    assert _raw(api, c.vol, c.iso, 0, None, 0, None, 0) == (0, n, m), "the count query"
    big_v, big_t = np.full((n + 2, 3), -3.0, np.float32), np.full((m + 2, 3), -3, np.int32)
    assert _raw(api, c.vol, c.iso, 0, big_v, n + 2, big_t, m + 2) == (0, n, m)
    assert_bits_equal(big_v[:n], rv, "vertices")
    assert_bits_equal(big_t[:m], rt, "triangles")
    assert (big_v[n:] == -3.0).all() and (big_t[m:] == -3).all(), "nothing past the counts"
    # too few vertices: they stay as they were, the triangles are still written, the counts are reported
    small_v, full_t = np.full((n - 1, 3), -3.0, np.float32), np.full((m, 3), -3, np.int32)
    assert _raw(api, c.vol, c.iso, 0, small_v, n - 1, full_t, m) == (ECAPACITY, n, m)
    assert (small_v == -3.0).all()
    assert_bits_equal(full_t, rt, "triangles beside a short vertex array")
    full_v, small_t = np.full((n, 3), -3.0, np.float32), np.full((m - 1, 3), -3, np.int32)
    assert _raw(api, c.vol, c.iso, 0, full_v, n, small_t, m - 1) == (ECAPACITY, n, m)
    assert (small_t == -3).all()
    assert_bits_equal(full_v, rv, "vertices beside a short triangle array")
    # one array alone
    only_v = np.full((n, 3), -3.0, np.float32)
    assert _raw(api, c.vol, c.iso, 0, only_v, n, None, 0) == (0, n, m)
    assert_bits_equal(only_v, rv, "vertices alone")
    # the Python face: the error carries the counts
    with pytest.raises(api.VisfdHipError) as e:
        api.isosurface_host(c.vol, c.iso, "below", vertices=small_v, triangles=full_t)
    assert e.value.code == ECAPACITY and e.value.counts == (n, m)
    assert api.isosurface_host(c.vol, c.iso, "below", vertices=big_v, triangles=big_t) == (n, m)
    assert api.isosurface_host(c.vol, c.iso, "below", count_only=True) == (n, m)


def test_refusals(api):
    vol = BY_NAME["noise345"].vol
    v, t = np.full((400, 3), -3.0, np.float32), np.full((800, 3), -3, np.int32)

    def refused(*a, **k):
        rc, nv, nt = _raw(api, *a, **k)
        assert rc == EINVAL and (nv, nt) == (-5, -5), (rc, nv, nt)
        assert (v == -3.0).all() and (t == -3).all()
        assert b"isosurface" in api.load_library().visfd_hip_last_error()

    refused(None, 0.0, 0, v, 400, t, 800)                                 # null volume
    refused(vol, 0.0, 0, v, 400, t, 800, nv=False)                        # null count pointers
    refused(vol, 0.0, 0, v, 400, t, 800, nt=False)
    refused(vol, 0.0, 2, v, 400, t, 800)                                  # unknown side
    refused(vol, 0.0, -1, v, 400, t, 800)
    for bad in (float("nan"), float("inf"), -float("inf")):               # non-finite level
        refused(vol, bad, 0, v, 400, t, 800)
    refused(vol, 0.0, 0, v, -1, t, 800)                                   # negative capacity
    L = api.load_library()
    a, b = C.c_int64(-5), C.c_int64(-5)
    for dims in ((0, 4, 3), (5, 0, 3), (5, 4, 0), (-1, 4, 3)):            # a dimension below 1
        rc = L.visfd_hip_isosurface_host(vol.ctypes.data, dims[0], dims[1], dims[2], 0.0, 0, v.ctypes.data, 400, t.ctypes.data,
                                         800, C.byref(a), C.byref(b))
        assert rc == EINVAL and (a.value, b.value) == (-5, -5) and (v == -3.0).all() and (t == -3).all()
    with pytest.raises(ValueError):
        api.isosurface_host(vol, 0.0, "sideways")


def test_context_entries_refuse_a_null_context(api):
    L = api.load_library()
    vol = BY_NAME["one"].vol
    a, b = C.c_int64(-5), C.c_int64(-5)
    s, ms = (C.c_int64 * 4)(), (C.c_float * 4)()
    for fn in (L.visfd_hip_isosurface, L.visfd_hip_isosurface_dev):
        assert fn(None, vol.ctypes.data, 1, 1, 1, 0.5, 0, None, 0, None, 0, C.byref(a), C.byref(b)) == EINVAL
        assert (a.value, b.value) == (-5, -5)
    assert L.visfd_hip_isosurface_last(None, s) == EINVAL
    assert L.visfd_hip_isosurface_last_times(None, ms) == EINVAL
