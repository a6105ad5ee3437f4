"""DiscardOverlappingBlobs on the GPU (csrc/discard_overlap.hip): every list of tests/overlap_cases.py through the
host-array and the torch device face, bit for bit against the sequential host entry and the reference's recorded outputs
(tests/golden/overlap.npz), with what ran asserted; the chain whose round count is its length, with and without the round
cap; the inputs that are handed over to the host; the option that keeps the call on the host; one context across other
stages' calls; the phase times of the option discard_overlap_time; the empty list."""
import numpy as np
import pytest

from conftest import golden
from overlap_cases import CASES

pytestmark = pytest.mark.gpu

F = np.float32


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
def expected(api):
    """the host entry's lists, computed once"""
    return {name: api.discard_overlapping_blobs(*case) for name, case in CASES.items()}


def same_bits(a, b):
    return len(a) == len(b) and all(np.asarray(x).shape == np.asarray(y).shape and
                                    np.array_equal(np.asarray(x, F).view(np.uint32), np.asarray(y, F).view(np.uint32))
                                    for x, y in zip(a, b))


def run_ctx(ctx, c, d, s, *rest):
    return ctx.discard_overlapping_blobs(c, d, s, *rest)


def run_dev(ctx, c, d, s, *rest):
    import torch
    dev = torch.device("cuda", 0)
    tc, td, ts = (torch.from_numpy(np.array(a, F)).to(dev) for a in (np.asarray(c, F).reshape(-1, 3), d, s))
    k = ctx.discard_overlapping_blobs_dev(tc, td, ts, *rest)
    return tc[:k].cpu().numpy(), td[:k].cpu().numpy(), ts[:k].cpu().numpy()


FACES = {"host_arrays": run_ctx, "device_arrays": run_dev}


@pytest.mark.parametrize("face", sorted(FACES))
def test_every_case_on_the_device(ctx, api, expected, face):
    g = golden("overlap")
    for name, case in CASES.items():
        got = FACES[face](ctx, *case)
        last = ctx.discard_overlapping_blobs_last()
        assert last["path"] == api.DISCARD_OVERLAP_PATH_DEVICE and last["reason"] == api.DISCARD_OVERLAP_REASON_NONE, (name, last)
        assert last["blobs_in"] == len(case[1]) and last["blobs_kept"] == len(got[1]), (name, last)
        assert same_bits(got, expected[name]), (face, name, len(got[1]), len(expected[name][1]), last)
        assert same_bits(got, (g[name + "_c"], g[name + "_d"], g[name + "_s"])), (face, name)


def test_round_counts_are_the_lists(ctx):
    """the rounds are the longest dependency chain of the list, whatever the launch saw of its own stores"""
    import overlap_np as on
    for name in ("chain48", "post0", "post4", "dense", "tsz0", "cells_c"):
        info = {}
        on.discard_overlapping_blobs(*CASES[name], info=info)
        run_ctx(ctx, *CASES[name])
        last = ctx.discard_overlapping_blobs_last()
        want = 0 if (info["tsz"] <= 0).any() else info["rounds"]
        assert last["rounds"] == want, (name, last, info)
        assert last["table_cells"] == max(0, int(np.prod(info["tsz"]))), (name, last)
        assert last["pairs_crit"] >= last["pairs_share"] >= 0


@pytest.mark.parametrize("face", sorted(FACES))
def test_chain_rounds_and_cap(ctx, api, expected, face):
    case = CASES["chain48"]
    got = FACES[face](ctx, *case)
    last = ctx.discard_overlapping_blobs_last()
    assert last["rounds"] == 48 and last["blobs_kept"] == 24 and last["path"] == api.DISCARD_OVERLAP_PATH_DEVICE, last
    assert same_bits(got, expected["chain48"])
    for cap in (8, 0, 47):
        with ctx.options(discard_overlap_max_rounds=cap):
            got = FACES[face](ctx, *case)
            last = ctx.discard_overlapping_blobs_last()
        assert last["path"] == api.DISCARD_OVERLAP_PATH_HANDED_OVER and last["reason"] == api.DISCARD_OVERLAP_REASON_ROUNDS, last
        assert last["rounds"] == cap and last["blobs_kept"] == 24
        assert same_bits(got, expected["chain48"]), cap
    with ctx.options(discard_overlap_max_rounds=48):
        assert same_bits(FACES[face](ctx, *case), expected["chain48"])
        assert ctx.discard_overlapping_blobs_last()["path"] == api.DISCARD_OVERLAP_PATH_DEVICE
    # a random list under a cap it exceeds
    with ctx.options(discard_overlap_max_rounds=2):
        assert same_bits(FACES[face](ctx, *CASES["post4"]), expected["post4"])
        assert ctx.discard_overlapping_blobs_last()["reason"] == api.DISCARD_OVERLAP_REASON_ROUNDS


@pytest.mark.parametrize("face", sorted(FACES))
def test_hand_over_inputs(ctx, api, face):
    c, d, s, *rest = CASES["post5"]
    for what, reason in (("nan_score", api.DISCARD_OVERLAP_REASON_NONFINITE), ("inf_coordinate", api.DISCARD_OVERLAP_REASON_NONFINITE),
                         ("negative_diameter", api.DISCARD_OVERLAP_REASON_NEGATIVE)):
        c2, d2, s2 = c.copy(), d.copy(), s.copy()
        if what == "nan_score":
            s2[17] = np.nan
        elif what == "inf_coordinate":
            c2[17, 1] = np.inf
        else:
            d2[17] = -3.0
        want = api.discard_overlapping_blobs(c2, d2, s2, *rest)
        got = FACES[face](ctx, c2, d2, s2, *rest)
        last = ctx.discard_overlapping_blobs_last()
        assert last["path"] == api.DISCARD_OVERLAP_PATH_HANDED_OVER and last["reason"] == reason and last["rounds"] == 0, (what, last)
        assert same_bits(got, want), what


@pytest.mark.parametrize("face", sorted(FACES))
def test_option_discard_overlap_host(ctx, api, expected, face):
    for name in ("post0", "n65"):
        with ctx.options(discard_overlap_host=1):
            got = FACES[face](ctx, *CASES[name])
            last = ctx.discard_overlapping_blobs_last()
        assert last["path"] == api.DISCARD_OVERLAP_PATH_HOST and last["rounds"] == 0 and last["blobs_kept"] == len(got[1]), last
        assert same_bits(got, expected[name])
    assert same_bits(api.discard_overlapping_blobs(*CASES["post0"], ctx=ctx), expected["post0"])
    assert ctx.discard_overlapping_blobs_last()["path"] == api.DISCARD_OVERLAP_PATH_DEVICE


def test_option_discard_overlap_time_reports_the_phases(api, expected):
    """off on a fresh context: five times -1; on, for a list that goes through the rounds: every phase -1 (did not run) or
    a time below a second, the reduction always timed; the list is the same either way"""
    c = api.Context(0)
    try:
        for timed in (0, 1, 0):
            with c.options(discard_overlap_time=timed):
                got = run_ctx(c, *CASES["dense"])
                last = c.discard_overlapping_blobs_last()
                ms = list(c.discard_overlapping_blobs_last_times().values())
            assert last["path"] == api.DISCARD_OVERLAP_PATH_DEVICE and last["rounds"] >= 1, last
            assert same_bits(got, expected["dense"])
            assert len(ms) == 5
            if timed:
                assert all(t == -1.0 or 0.0 <= t < 1000.0 for t in ms) and ms[0] >= 0.0, ms
            else:
                assert ms == [-1.0] * 5, ms
    finally:
        c.close()


def test_one_context_between_other_stages(ctx, api, expected):
    """the workspace is the context's: other stages' calls before and after, a poisoned workspace, a trimmed one"""
    rng = np.random.default_rng(3)
    vol = rng.normal(0, 1, (24, 24, 24)).astype(F)
    ratio = api.ratio_from_threshold(0.03)
    g0, _ = ctx.gauss_ratio(vol, (1.5, 1.5, 1.5), ratio)
    assert same_bits(run_ctx(ctx, *CASES["dense"]), expected["dense"])
    ids = ctx.find_spheres(CASES["post0"][0][:20], CASES["post0"][0], CASES["post0"][1])
    assert same_bits(run_dev(ctx, *CASES["post0"]), expected["post0"])
    g1, _ = ctx.gauss_ratio(vol, (1.5, 1.5, 1.5), ratio)
    assert np.array_equal(g0.view(np.uint32), g1.view(np.uint32))
    assert np.array_equal(ids, api.find_spheres_host(CASES["post0"][0][:20], CASES["post0"][0], CASES["post0"][1]))
    ctx.debug_poison_workspace()
    assert same_bits(run_ctx(ctx, *CASES["n257"]), expected["n257"])     # a shorter list in the larger, poisoned buffers
    ctx.trim()
    assert same_bits(run_ctx(ctx, *CASES["cells_c"]), expected["cells_c"])


@pytest.mark.parametrize("face", sorted(FACES))
def test_empty_list(ctx, api, face):
    c, d, s = np.zeros((0, 3), F), np.zeros(0, F), np.zeros(0, F)
    got = FACES[face](ctx, c, d, s, 1.0)
    assert [len(x) for x in got] == [0, 0, 0]
    last = ctx.discard_overlapping_blobs_last()
    assert last["path"] == api.DISCARD_OVERLAP_PATH_DEVICE and last["blobs_in"] == 0 and last["blobs_kept"] == 0 and last["rounds"] == 0


def test_arguments(ctx, api):
    c, d, s = CASES["post5"][:3]
    with pytest.raises(api.VisfdHipError):
        ctx.discard_overlapping_blobs(c, d, s, 1.0, scale=0)
    with pytest.raises(api.VisfdHipError):
        ctx.discard_overlapping_blobs(c, d, s, 1.0, criteria=7)


def test_program_on_the_device_writes_the_same_bytes(tmp_path):
    """filter_mrc with VISFD_HIP_DISCARD_OVERLAP_MIN_BLOBS=0 (always the device) at both call sites: -discard-blobs and
    the thinning of -find-minima / -find-maxima; the files are the host route's, byte for byte"""
    import os
    import subprocess
    from conftest import ROOT
    from overlap_cases import run_discard_blobs
    cli = os.path.join(ROOT, "visfd_amd", "cli", "filter_mrc")
    image = os.path.join(ROOT, "tests", "golden", "test_blob_detect.rec")
    for name in ("post0", "dense"):
        host, err_h = run_discard_blobs(cli, image, str(tmp_path), CASES[name], "1e30", name + "_host")
        dev, err_d = run_discard_blobs(cli, image, str(tmp_path), CASES[name], "0", name + "_dev")
        assert "(discard_overlap: host)" in err_h and "(discard_overlap: device)" in err_d
        assert host == dev and len(host) > 0, name
        assert err_h.replace("(discard_overlap: host)", "") == err_d.replace("(discard_overlap: device)", "")
    files = {}
    for route, value in (("host", "1e30"), ("device", "0")):
        env = dict(os.environ, VISFD_HIP_DISCARD_OVERLAP_MIN_BLOBS=value)
        out = [str(tmp_path / ("%s_%s.txt" % (kind, route))) for kind in ("min", "max")]
        r = subprocess.run([cli, "-in", image, "-w", "1", "-find-minima", out[0], "-find-maxima", out[1], "-diameters", "6",
                            "-radial-separation", "0.9"], capture_output=True, text=True, env=env)
        assert r.returncode == 0, r.stderr
        assert r.stderr.count("(discard_overlap: %s)" % route) == 2, r.stderr
        files[route] = [open(p, "rb").read() for p in out]
    assert files["host"] == files["device"] and all(len(b) > 0 for b in files["host"])
