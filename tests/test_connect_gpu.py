"""LabelConnected with its seed search on the device (csrc/connect_seeds.hip; the flood stays on the host) against
api.label_connected (everything on the host).  Labels, cluster count, seed positions, sizes, seed saliencies and the
rewritten directions must be the same bits on every volume, and the entry must say that the device searched the seeds.

What can go wrong is the seed list -- which plateau roots are seeds, their values, their order among ties -- and the
staging, so the volumes are chosen for the search: plateaus that cross the 64 x 8 x 8 tile edges in x, in y and in z,
images where every voxel lies on a face, masks, minima, every connectivity the device search has, and one it has not."""
import os
import subprocess

import numpy as np
import pytest

import test_connect as tc
import test_connect_graph as tg
import volgen
from conftest import ROOT

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


def both(api, ctx, sal, ten, direction, case, where=None):
    """the host's result and the device-seeded call's on the same inputs, compared; -> (host result, seeds found)"""
    kw = {k: v for k, v in case.items() if not k.startswith("_")}
    use = kw.pop("use", "")
    mask = None
    if kw.pop("mask", False):       # block_mask cuts boxes of 4 x 5 x 6 voxels; thinner images get a sprinkle
        mask = volgen.block_mask(sal.shape, seed=9) if min(sal.shape) > 6 else \
            (np.random.default_rng(9).random(sal.shape) > 0.2).astype(np.float32)
    out = []
    for c in (None, ctx):
        d = direction.copy() if "v" in use else None
        r = api.label_connected(sal, mask=mask, direction=d, tensor=ten if "t" in use else None, seeds_ctx=c, **kw)
        out.append(r + (d,))
    tc.same(out[1], out[0], str(case.get("_name", "")))
    p, seeds = ctx.label_connected_device_seeds_last()
    assert p == (api.CONNECT_SEEDS_DEVICE if where is None else where), p
    assert (seeds >= out[0][1]) if p == api.CONNECT_SEEDS_DEVICE else seeds == -1
    return out[0], seeds


def test_tensor_voting_outputs_every_case(api, ctx, tv):
    """test_connect.py's five calls and its must-link / voxel-weight calls, and the variants of test_connect_graph.py
    (connectivities, mask, minima, thresholds off, signs, plateaus)"""
    post, ten, direction = tv
    found = 0
    for case in tc.cases(post) + tc.must_link_cases(post):
        host, _ = both(api, ctx, post, ten, direction, case)
        found += host[1]
    assert found > 20
    for name, case in tg._variants(post):
        sal, t, d = tg._inputs(post, ten, direction, case)
        both(api, ctx, sal, t, d, dict(case, _name=name))


@pytest.mark.parametrize("shape", [(3, 3, 3), (70, 5, 3), (20, 20, 70), (70, 20, 9), (9, 70, 20)],
                         ids=lambda s: "%dx%dx%d" % (s[2], s[1], s[0]))
def test_small_and_tile_crossing_images(api, ctx, shape):
    """random directions and tensors; the saliency once as it is and once in five levels, so that plateaus (and the seeds
    at their first voxels) run across every tile edge the shape has"""
    for conn in (1, 2, 3):
        for signs in (True, False):
            sal, ten, d, case = tg._small(shape, 3 + conn, connectivity=conn, consider_dot_product_sign=signs,
                                          standardize_directions=not signs)
            both(api, ctx, sal, ten, d, case)
            flat = (np.floor(sal * 5) / 5).astype(np.float32)
            host, seeds = both(api, ctx, flat, ten, d, dict(case, mask=conn == 2, start_from_saliency_maxima=conn != 3,
                                                            threshold_saliency=0.4 if conn != 3 else 0.6))
            both(api, ctx, flat, None, None, dict(threshold_saliency=0.8, connectivity=conn, sort_by_size=False))


def test_two_sheets_touching_through_one_voxel(api, ctx):
    sal = np.zeros((16, 20, 70), np.float32)
    rng = np.random.default_rng(5)
    sal[4] = 1 + rng.random((20, 70)).astype(np.float32)
    sal[6] = 1 + rng.random((20, 70)).astype(np.float32)
    one, _ = both(api, ctx, sal, None, None, dict(threshold_saliency=0.5, connectivity=1))
    assert one[1] == 2
    sal[5, 9, 66] = 1.5                   # the bridge, beyond the first tile in x
    joined, _ = both(api, ctx, sal, None, None, dict(threshold_saliency=0.5, connectivity=1))
    assert joined[1] == 1


def test_one_plateau_is_one_seed_and_a_discarded_seed_drops_its_basin(api, ctx, tv):
    sal = np.zeros((12, 12, 70), np.float32)
    sal[3:9, 3:9, 2:68] = 2.0             # one plateau over two tiles in x, y and z: one seed, at its first voxel
    host, seeds = both(api, ctx, sal, None, None, dict(threshold_saliency=1.0, connectivity=3))
    assert seeds == 1 and host[1] == 1 and tuple(host[2][0]) == (2.0, 3.0, 3.0) and host[3][0] == 6 * 6 * 66
    post, ten, direction = tv             # strict vector test: some maxima fail it and seed nothing
    case = dict(tc.cases(post)[3], threshold_vector_saliency=0.97)
    host, seeds = both(api, ctx, post, ten, direction, case)
    assert 0 < host[1] < seeds


def test_connectivity_beyond_the_device_search_takes_the_host_path(api, ctx):
    sal, ten, d, case = tg._small((9, 10, 11), 7, connectivity=5, consider_dot_product_sign=False)
    both(api, ctx, sal, ten, d, case, where=api.CONNECT_SEEDS_HOST)
    both(api, ctx, sal, ten, d, dict(case, connectivity=3))      # and the next call is back on the device


def test_inputs_on_which_the_flood_order_decides(api, ctx):
    """The twisted band whose normals cannot be oriented, alone, with weights and with a must-link: only the seed search
    moved, so these are calls like any other and must equal the host too"""
    sal, direction = tg._twisted_band()
    case = dict(threshold_saliency=float(np.exp(-0.5)), connectivity=3, consider_dot_product_sign=False, use="v",
                standardize_directions=True, threshold_vector_saliency=-2.0)
    host, _ = both(api, ctx, sal, None, direction, case)
    assert host[1] == 1
    both(api, ctx, sal, None, direction, dict(case, voxel_weights=np.random.default_rng(2).uniform(0.5, 2, sal.shape).astype(np.float32)))
    both(api, ctx, sal, None, direction, dict(case, threshold_saliency=0.9, connectivity=1,
                                              must_link=[[(4.0, 12.0, 12.0), (19.0, 12.0, 12.0)]]))


def test_argument_checks_on_a_live_context(api, ctx):
    before = ctx.label_connected_device_seeds_last()
    with pytest.raises(api.VisfdHipError):
        ctx.label_connected_device_seeds(np.zeros((2, 8, 8), np.float32), 0.0)
    with pytest.raises(api.VisfdHipError):
        ctx.label_connected_device_seeds(np.zeros((8, 8, 8), np.float32), 0.0, connectivity=0)
    assert ctx.label_connected_device_seeds_last() == before        # a refused call leaves the record alone


def test_cpp_function_with_a_context(tmp_path):
    """include/visfd_hip.hpp: LabelConnectedDeviceSeeds(ctx, ...) against the reference's LabelConnected, in a C++11 program"""
    exe = str(tmp_path / "shim_connect_check")
    libdir = os.path.join(ROOT, "visfd_amd")
    subprocess.check_call(["g++", "-std=c++11", "-O1", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "shim_connect_check.cpp"), "-o", exe, "-L" + libdir, "-lvisfd_hip",
                           "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "shim connect check ok" in r.stdout, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
