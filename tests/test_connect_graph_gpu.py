"""LabelConnected as a graph problem on the device (csrc/connect_graph.hip) through both faces -- host arrays
(visfd_hip_label_connected_graph) and device arrays (visfd_hip_label_connected_graph_dev) -- against the flood
(api.label_connected), by the contract of tests/connect_graph_contract.py: the flood's labels, lists and labelled
directions, the input's directions everywhere else.  Wherever the restatement (connect_graph_np.py) reports no reason other
than HALO the call must have taken the device path; the other calls must agree through the fall-back.

The kernels work on four voxels per thread and 256 threads per workgroup over the flat image, and one listed voxel per
thread afterwards, so there are no 3-D tiles of their own; the seed search they call has 64 x 8 x 8 tiles.  The shapes
cross both: 70 in x, y and z, images thinner than a tile, sizes that are no multiple of four (27, 1050 voxels).  Every
test is a comparison; none repeats a run."""
import numpy as np
import pytest

import connect_graph_contract as cc
import connect_graph_np as cg
import test_connect as tc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def api():
    from visfd_amd import api
    return api


@pytest.fixture(scope="module")
def ctx(api):
    c = api.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def tv(oracle):
    return tc.tv_outputs(oracle)


def _dev_face(api, ctx, sal, ten, direction, case):
    import torch
    kw, mask, d_in, t = cc.split(sal, ten, direction, case)
    up = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()
    labels = torch.empty(sal.shape, dtype=torch.int64, device="cuda")
    d = up(d_in)
    if "voxel_weights" in kw:
        kw["voxel_weights"] = up(kw["voxel_weights"])
    k, cm, cs, csal = ctx.label_connected_graph_dev(up(sal), labels, mask=up(mask), direction=d, tensor=up(t), **kw)
    return labels.cpu().numpy(), k, cm, cs, csal, None if d is None else d.cpu().numpy()


def both_faces(api, ctx, name, sal, ten, direction, case, want_path=None):
    """one call through both faces, the contract checked on each -> (flood result, path, reasons, valid, candidates)"""
    flood, want, want_valid, want_candidates = cc.reference(name, sal, ten, direction, case)
    last = None
    for face in ("host arrays", "device arrays"):
        if face == "host arrays":
            kw, mask, d_in, t = cc.split(sal, ten, direction, case)
            d = None if d_in is None else d_in.copy()
            got = ctx.label_connected_graph(sal, mask=mask, direction=d, tensor=t, **kw) + (d,)
        else:
            got = _dev_face(api, ctx, sal, ten, direction, case)
        path, reasons, n_valid, n_undecided = ctx.label_connected_graph_last()
        _check(name, face, got, sal, ten, direction, case)
        if want_path is not None:
            assert path == want_path, (name, face, path, cg.reason_names(reasons))
        elif want == 0:
            assert path == api.CONNECT_GRAPH_DEVICE and reasons == 0, (name, face, path, cg.reason_names(reasons))
        else:
            assert path == api.CONNECT_GRAPH_FLOOD and reasons != 0, (name, face, path)
        if path == api.CONNECT_GRAPH_DEVICE:
            assert n_valid == want_valid, (name, face, n_valid, want_valid)
            assert n_undecided == want_candidates, (name, face, n_undecided, want_candidates)
            assert ("v" in case.get("use", "")) or n_undecided == 0, (name, face)
        elif n_undecided >= 0:      # handed over after the device had counted
            assert n_undecided == want_candidates, (name, face, n_undecided, want_candidates)
        assert last is None or last == (path, reasons, n_valid, n_undecided), (name, "the two faces disagree")
        last = (path, reasons, n_valid, n_undecided)
    return (flood,) + last


def _check(name, face, got, sal, ten, direction, case):
    # the reference is kept under the call's name; the face only labels the message
    try:
        cc.check(name, got, sal, ten, direction, case)
    except AssertionError as e:
        raise AssertionError("%s: %s" % (face, e))


def test_tensor_voting_outputs_every_case(api, ctx, tv):
    """test_connect.py's calls, its must-link and voxel-weight calls, and the 34 calls of test_connect_graph.py, all of
    which must take the device path"""
    jobs = cc.tv_jobs(*tv)
    found = 0
    for k, job in enumerate(jobs):
        want = api.CONNECT_GRAPH_DEVICE if k >= len(jobs) - cc.N_TG else None
        found += both_faces(api, ctx, *job, want_path=want)[0][1]
    assert found > 100


@pytest.mark.parametrize("conn", [1, 2, 3])
@pytest.mark.parametrize("shape", cc.SHAPES, ids=lambda s: "%dx%dx%d" % (s[2], s[1], s[0]))
def test_small_and_edge_crossing_images(api, ctx, shape, conn):
    for job in cc.shape_jobs(shape, conn):
        both_faces(api, ctx, *job)


def _sheet(shape=(10, 24, 70), seed=5, levels=True):
    """one sheet at z = 4 whose normals fan out from a point far below it, each with a random sign"""
    rng = np.random.default_rng(seed)
    nz, ny, nx = shape
    sal = np.zeros(shape, np.float32)
    v = rng.random((ny, nx)).astype(np.float32)
    sal[4] = 1 + (np.floor(v * 5) / 5 if levels else v)
    z, y, x = np.meshgrid(np.arange(nz) + 40.0, np.arange(ny) - ny / 2 + 0.3, np.arange(nx) - nx / 2 + 0.3, indexing="ij")
    d = np.stack([x, y, z], -1)
    d /= np.linalg.norm(d, axis=-1, keepdims=True)
    d *= np.where(rng.random(shape) < 0.5, -1.0, 1.0)[..., None]
    ten = np.zeros(shape + (6,), np.float32)
    ten[..., :3] = 1
    return sal, ten, np.ascontiguousarray(d.astype(np.float32))


_SHEET_CASE = dict(threshold_saliency=0.5, use="vt", threshold_vector_saliency=-2.0, threshold_vector_neighbor=0.5,
                   consider_dot_product_sign=False, standardize_directions=True, connectivity=1)


def test_two_sheets_joined_through_one_voxel(api, ctx):
    sal = np.zeros((16, 20, 70), np.float32)
    rng = np.random.default_rng(5)
    sal[4] = 1 + rng.random((20, 70)).astype(np.float32)
    sal[6] = 1 + rng.random((20, 70)).astype(np.float32)
    case = dict(threshold_saliency=0.5, connectivity=1)
    assert both_faces(api, ctx, "two sheets", sal, None, None, case, api.CONNECT_GRAPH_DEVICE)[0][1] == 2
    sal = sal.copy()
    sal[5, 9, 66] = 1.5
    assert both_faces(api, ctx, "two sheets bridged", sal, None, None, case, api.CONNECT_GRAPH_DEVICE)[0][1] == 1


def test_many_seeds_facing_against_their_anchor(api, ctx):
    """the case that used to be HALO: one component, many seeds, raw directions of either sign"""
    sal, ten, d = _sheet()
    g = cg.label_connected_graph(sal, direction=d.copy(), tensor=ten, **{k: v for k, v in _SHEET_CASE.items() if k != "use"})
    assert g["reasons"] == cg.HALO and g["detail"]["seeds_against_anchor"] > 20 and g["n_clusters"] == 1
    flood = both_faces(api, ctx, "opposing seeds", sal, ten, d, _SHEET_CASE, api.CONNECT_GRAPH_DEVICE)[0]
    assert flood[1] == 1 and flood[3][0] == 24 * 70


def test_component_without_a_valid_seed_stays_unlabelled(api, ctx):
    """a ramp: the one seed is the plateau at the high end; the low half faces across and is its own component, which
    holds no seed"""
    sal = np.broadcast_to(1 + np.arange(70, dtype=np.float32) / 70, (6, 8, 70)).copy()
    z, y, x = np.meshgrid(np.arange(6) + 200.0, np.arange(8) - 3.7, np.arange(70) - 49.7, indexing="ij")
    d = np.stack([x, y, z], -1)      # the high part fans out from a point far below (its outward sum is far from zero)
    d = np.ascontiguousarray((d / np.linalg.norm(d, axis=-1, keepdims=True)).astype(np.float32))
    d[:, :, :30] = (1.0, 0.0, 0.0)
    ten = np.zeros((6, 8, 70, 6), np.float32)
    ten[..., :3] = 1
    flood, path, reasons, n_valid, _ = both_faces(api, ctx, "ramp", sal, ten, d, dict(_SHEET_CASE, connectivity=3))
    assert flood[1] == 1 and flood[3][0] == 6 * 8 * 40 and n_valid == sal.size and path == api.CONNECT_GRAPH_DEVICE


def test_discarded_seed_all_candidates_failing_and_no_candidate(api, ctx, tv):
    post, ten, direction = tv
    case = dict(tc.cases(post)[3], threshold_vector_saliency=0.97)      # strict: some maxima fail and seed nothing
    flood, path, _, n_valid, n_undecided = both_faces(api, ctx, "discarded seeds", post, ten, direction, case)
    assert 0 < flood[1] and path == api.CONNECT_GRAPH_DEVICE and 0 < n_valid < n_undecided
    case = dict(tc.cases(post)[3], threshold_vector_saliency=1.5)       # no cosine reaches 1.5
    flood, path, _, n_valid, n_undecided = both_faces(api, ctx, "all fail", post, ten, direction, case, api.CONNECT_GRAPH_DEVICE)
    assert flood[1] == 0 and n_valid == 0 and n_undecided > 1000
    case = dict(tc.cases(post)[2], threshold_saliency=float(post.max()) * 2)
    flood, path, _, n_valid, n_undecided = both_faces(api, ctx, "no candidate", post, ten, direction, case, api.CONNECT_GRAPH_DEVICE)
    assert flood[1] == 0 and n_valid == 0 and n_undecided == 0
    # without directions nothing is undecided
    _, path, _, n_valid, n_undecided = both_faces(api, ctx, "no directions", post, ten, direction, dict(tc.cases(post)[0], use="t"))
    assert path == api.CONNECT_GRAPH_DEVICE and n_valid > 1000 and n_undecided == 0


def test_one_long_component(api, ctx):
    """some 10^5 voxels; a corridor that doubles back every four rows makes one component some thousand voxels long:
    deep trees and roots that many lanes hook at once"""
    shape = (8, 112, 112)
    sal, ten, d = _sheet(shape, seed=7)
    y, x = np.meshgrid(np.arange(112), np.arange(112), indexing="ij")
    wall = (y % 4 == 3) & np.where((y // 4) % 2 == 0, x < 108, x >= 4)
    sal[4][wall] = 0
    flood, path, reasons, n_valid, _ = both_faces(api, ctx, "corridor", sal, ten, d, _SHEET_CASE, api.CONNECT_GRAPH_DEVICE)
    assert flood[1] == 1 and flood[3][0] == n_valid == int((~wall).sum())


def test_refusals_and_fall_backs_leave_the_context_usable(api, ctx):
    sal, ten, d = _sheet()
    good = lambda tag: both_faces(api, ctx, "opposing seeds", sal, ten, d, _SHEET_CASE, api.CONNECT_GRAPH_DEVICE)
    good("before")
    before = ctx.label_connected_graph_last()
    with pytest.raises(api.VisfdHipError):
        ctx.label_connected_graph(np.zeros((2, 8, 8), np.float32), 0.0)
    with pytest.raises(api.VisfdHipError):
        ctx.label_connected_graph(np.zeros((8, 8, 8), np.float32), 0.0, connectivity=0)
    assert ctx.label_connected_graph_last() == before        # a refused call leaves the record alone
    good("after a refusal")
    import test_connect_graph as tg
    band, band_d = tg._twisted_band()
    case = dict(threshold_saliency=float(np.exp(-0.5)), connectivity=3, consider_dot_product_sign=False, use="v",
                standardize_directions=True, threshold_vector_saliency=-2.0)
    _, path, reasons, _, _ = both_faces(api, ctx, "band", band, None, band_d, case)
    assert path == api.CONNECT_GRAPH_FLOOD and reasons & api.CONNECT_REASON_UNBALANCED
    good("after a fall-back")
    w = np.random.default_rng(2).uniform(0.5, 2, band.shape).astype(np.float32)
    _, path, reasons, _, _ = both_faces(api, ctx, "band weights", band, None, band_d, dict(case, voxel_weights=w))
    assert path == api.CONNECT_GRAPH_FLOOD and reasons == api.CONNECT_REASON_WEIGHTS
    _, path, reasons, _, _ = both_faces(api, ctx, "band must-link", band, None, band_d,
                                        dict(case, threshold_saliency=0.9, connectivity=1,
                                             must_link=[[(4.0, 12.0, 12.0), (19.0, 12.0, 12.0)]]))
    assert path == api.CONNECT_GRAPH_FLOOD and reasons == api.CONNECT_REASON_MUST_LINK
    _, path, reasons, _, _ = both_faces(api, ctx, "band conn5", band, None, band_d, dict(case, connectivity=5))
    assert path == api.CONNECT_GRAPH_FLOOD and reasons & api.CONNECT_REASON_LIMITS
    good("after the limits")
