"""The surface points on the host: the numpy restatement (tests/surface_points_np.py) equals visfd_hip_surface_points bit for
bit on every case of tests/surface_points_cases.py, and stops doing so when one of the things the device kernel must get
right is broken in it.  No GPU needed."""
import numpy as np
import pytest

import surface_points_cases as SC
import surface_points_np as SN
from conftest import assert_bits_equal

_HOST = {}


def host(name):
    if name not in _HOST:
        from visfd_amd import api
        c = SC.get(name)
        _HOST[name] = api.surface_points_host(c["saliency"], c["direction"], **SC.call_args(c))
        for a in _HOST[name]:
            a.setflags(write=False)
    return _HOST[name]


def restated(name, **kw):
    c = SC.get(name)
    return SN.surface_points(c["saliency"], c["direction"], **dict(SC.call_args(c), **kw))


def same(a, b):
    return all(x.shape == y.shape and np.array_equal(x.view(np.uint32), y.view(np.uint32)) for x, y in zip(a, b))


@pytest.mark.parametrize("name", sorted(SC.CASES))
def test_restatement_equals_the_host_entry(name):
    want = host(name)
    got = restated(name)
    assert_bits_equal(got[0], want[0], name + " crds")
    assert_bits_equal(got[1], want[1], name + " norms")


def test_cases_cover_what_they_are_meant_to():
    n = {name: len(host(name)[0]) for name in SC.CASES}
    assert n["absent_cluster"] == 0
    assert n["no_cluster"] == 6 * 7 * 21 and 0 < n["no_cluster_masked"] < n["no_cluster"]
    assert n["sheet"] > 2048 and n["sheet_thin_image"] > 256          # more than one workgroup chunk, more than a wave
    assert n["maxd_small"] < n["sheet"] <= n["maxd_off"]                # the distance rejection acts, and only when positive
    assert n["no_ridge"] > n["sheet"]                                   # the snap drops points
    assert n["two_clusters_1"] > 0 and n["two_clusters_2"] > 0
    for name in SC.CASES:   # every walk stays far below the device's default cap, and the thick sheet above the test's cap of 8
        c = SC.get(name)
        steps = SN.surface_points(c["saliency"], c["direction"], want_steps=True, **dict(SC.call_args(c), find_ridge=False))[2]
        assert steps < 60, (name, steps)
    c = SC.get("sheet")
    assert SN.surface_points(c["saliency"], c["direction"], want_steps=True, **SC.call_args(c))[2] > 8


def test_one_voxel_sheet_with_a_long_step_has_no_backward_entry():
    c = SC.get("one_voxel_ds1")
    got = SN.surface_points(c["saliency"], c["direction"], want_steps=True, **dict(SC.call_args(c), find_ridge=False))
    assert got[2] == 0                                                  # nobody took a step: i stays 0, xyz is the voxel
    idx = np.flatnonzero(c["cluster"].ravel() == 1)
    nz, ny, nx = c["cluster"].shape
    assert np.array_equal(got[0], np.stack([idx % nx, (idx // nx) % ny, idx // (nx * ny)], 1).astype(np.float32))


def test_zero_saliency_gives_nan_average_and_the_last_entry():
    """Where every weight of a walk is zero, ave_s is 0 / 0 and the bracket search runs to the end: the host entry and the
    restatement agree there (the case is in the parametrised test); here: the case does hold such walks."""
    c = SC.get("zero_saliency_column")
    assert (c["saliency"][:, 5:10, 10:15] == 0).all() and (c["cluster"][:, 5:10, 10:15] == 1).any()


def test_golden_ply_belongs_to_the_scenario_and_is_a_thick_sheet(tmp_path):
    """tests/golden/surface_points.npz (the reference program's PLY text) was made from the files the scenario function
    builds today, and its walks are long: the sheet is nine voxels thick."""
    import os
    import sys
    from conftest import GOLDEN
    sys.path.insert(0, GOLDEN)
    import make_golden_surface_points as MG
    g = np.load(os.path.join(GOLDEN, "surface_points.npz"))
    assert MG.write_files(str(tmp_path)) == int(g["crc"])
    assert [str(a) for a in g["args"]] == SC.PROGRAM_ARGS
    text = g["ply"].tobytes().decode()
    assert int(text.split("element vertex ")[1].split()[0]) > 200


@pytest.mark.parametrize("mutant,cases", [("fma", ["no_ridge"]), ("order", ["no_ridge"]), ("rint", ["axis_half_steps"])])
def test_comparison_trips_on_mutants(mutant, cases):
    """(The snap starts from the ROUNDED walked position, so the walk's last bits show in the cases without it.)"""
    assert any(not same(restated(name, mutant=mutant), host(name)) for name in cases), mutant
