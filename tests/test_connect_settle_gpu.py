"""The option connect_settle of visfd_hip_label_connected_graph and _graph_dev (csrc/connect_graph.hip) on the
GPU: must-links, voxel weights and outward sums in doubt stay on the device path, and the results are the flood's by the
contract of tests/connect_graph_contract.py.  The calls are those of tests/connect_settle_cases.py, whose expectations
tests/test_connect_settle.py derives on the CPU from a numpy restatement of the rule.  The images are the smallest that
still cross the seed search's 64 x 8 x 8 tiles in each axis; the new kernels work on the list of candidate voxels, 256 or
1024 per workgroup, so a sheet of 630 voxels and two of them both sides of a workgroup edge are in.  Every test is a
comparison; none repeats a run."""
import numpy as np
import pytest

import connect_graph_contract as cc
import connect_graph_np as cg
import connect_settle_cases as sc
import test_connect as tc
import test_connect_graph_gpu as tgg

pytestmark = pytest.mark.gpu

_CASES = sc.all_cases()


@pytest.fixture(scope="module")
def api():
    from visfd_amd import api
    return api


@pytest.fixture(scope="module")
def ctx(api):
    c = api.Context(0)
    yield c
    c.close()


def _faces(api, ctx, name, sal, ten, direction, case, settle=1):
    """one call through both faces under the option -> [(results, path, reasons, settled)] per face, the contract checked"""
    out = []
    with ctx.options(connect_settle=settle):
        for face in ("host arrays", "device arrays"):
            if face == "host arrays":
                kw, mask, d_in, t = cc.split(sal, ten, direction, case)
                d = None if d_in is None else d_in.copy()
                got = ctx.label_connected_graph(sal, mask=mask, direction=d, tensor=t, **kw) + (d,)
            else:
                got = tgg._dev_face(api, ctx, sal, ten, direction, case)
            path, reasons, _, _ = ctx.label_connected_graph_last()
            bits = ctx.label_connected_graph_last_settled()
            print(name, face, "path", path, "reasons", cg.reason_names(reasons), "settled", cg.reason_names(bits))
            tgg._check(name, face, got, sal, ten, direction, case)
            out.append((got, path, reasons, bits))
    return out


@pytest.mark.parametrize("job", _CASES, ids=[j[0] for j in _CASES])
def test_every_case_both_faces(api, ctx, job):
    name, sal, ten, direction, case, expect = job
    for got, path, reasons, bits in _faces(api, ctx, name, sal, ten, direction, case):
        if expect["path"] == "device":
            assert path == api.CONNECT_GRAPH_DEVICE and reasons == 0, (name, path, cg.reason_names(reasons))
            assert bits == expect["settled"], (name, cg.reason_names(bits))
        else:
            assert path == api.CONNECT_GRAPH_FLOOD and reasons == expect["reasons"], (name, path, cg.reason_names(reasons))
            assert bits == 0, name


def test_tensor_voting_volume_with_must_links_and_weights(api, ctx, oracle):
    """seven islands of a voted surface, two groups of three locations, weights, a mask: 38080 voxels, several workgroups"""
    post, ten, direction = tc.tv_outputs(oracle)
    on_device = 0
    for i, case in enumerate(tc.must_link_cases(post)):
        name = "tc must-link %d" % i
        want = (cg.MUST_LINK if "must_link" in case else 0) | (cg.WEIGHTS if "voxel_weights" in case else 0)
        structural = cc.reference(name, post, ten, direction, case)[1] & ~(cg.MUST_LINK | cg.WEIGHTS | cg.OUTWARD)
        for got, path, reasons, bits in _faces(api, ctx, name, post, ten, direction, case):
            if structural:
                assert path == api.CONNECT_GRAPH_FLOOD and reasons & structural, (name, cg.reason_names(reasons))
            else:
                assert path == api.CONNECT_GRAPH_DEVICE and reasons == 0, (name, path, cg.reason_names(reasons))
                assert bits & ~cg.OUTWARD == want, (name, cg.reason_names(bits))
                on_device += 1
    assert on_device == 12      # tests/test_connect_settle.py: the restatement has no other reason on any of the six


def test_other_reasons_still_hand_over(api, ctx):
    """the twisted band of test_connect_graph_gpu.py cannot be oriented: with weights and the option on, that alone is
    the reason"""
    import test_connect_graph as tg
    band, band_d = tg._twisted_band()
    w = np.random.default_rng(2).uniform(0.5, 2, band.shape).astype(np.float32)
    case = dict(threshold_saliency=float(np.exp(-0.5)), connectivity=3, consider_dot_product_sign=False, use="v",
                standardize_directions=True, threshold_vector_saliency=-2.0, voxel_weights=w)
    for got, path, reasons, bits in _faces(api, ctx, "band weights", band, None, band_d, case):
        assert path == api.CONNECT_GRAPH_FLOOD and reasons == api.CONNECT_REASON_UNBALANCED and bits == 0


def test_option_off_beside_option_on(api, ctx):
    """one context, the same call: off, it reports what it reports today; the labelled results are the same bits"""
    name, sal, ten, direction, case, expect = _CASES[1]
    assert ctx.get_option("connect_settle") == 0
    off = _faces(api, ctx, name, sal, ten, direction, case, settle=0)
    on = _faces(api, ctx, name, sal, ten, direction, case, settle=1)
    for (g0, p0, r0, b0), (g1, p1, r1, b1) in zip(off, on):
        assert p0 == api.CONNECT_GRAPH_FLOOD and r0 == api.CONNECT_REASON_MUST_LINK and b0 == 0
        assert p1 == api.CONNECT_GRAPH_DEVICE and r1 == 0 and b1 == api.CONNECT_REASON_MUST_LINK
        for a, b in zip(g0, g1):
            assert np.array_equal(np.atleast_1d(a).view(np.uint8), np.atleast_1d(b).view(np.uint8))
    assert ctx.get_option("connect_settle") == 0


def test_must_link_without_a_labelled_voxel(api, ctx):
    name, sal, ten, direction, case, expect = _CASES[0]
    kw, mask, d_in, t = cc.split(sal, ten, direction, dict(case, threshold_saliency=100.0))
    with ctx.options(connect_settle=1):
        with pytest.raises(api.VisfdHipError, match="nearest voxel from an empty set") as e:
            ctx.label_connected_graph(sal, mask=mask, direction=d_in.copy(), tensor=t, **kw)
        assert e.value.code == 1      # VISFD_HIP_EINVAL
    with pytest.raises(api.VisfdHipError, match="nearest voxel from an empty set"):       # the flood's own message
        api.label_connected(sal, mask=mask, direction=d_in.copy(), tensor=t, **kw)
    for got, path, reasons, bits in _faces(api, ctx, name, sal, ten, direction, case):
        assert path == api.CONNECT_GRAPH_DEVICE and bits == expect["settled"]
