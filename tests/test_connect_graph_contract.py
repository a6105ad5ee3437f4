"""LabelConnected as a graph problem, what can be said without a GPU: the new entries exist in the header, the binding and
the C++ header; the serial host walk (visfd_hip_label_connected_graph_host) keeps the contract of
tests/connect_graph_contract.py against the flood on every call of test_connect.py and test_connect_graph.py, with the path
and the reasons the restatement (connect_graph_np.py) gives; constructed calls are handed to the flood for the reason they
were constructed for; bad arguments are refused; a C++ program goes through LabelConnectedGraph."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import connect_graph_contract as cc
import connect_graph_np as cg
import test_connect as tc
import test_connect_graph as tg
from conftest import ROOT
from visfd_amd import api

NEW_SYMBOLS = ["visfd_hip_label_connected_graph", "visfd_hip_label_connected_graph_dev", "visfd_hip_label_connected_graph_host",
               "visfd_hip_label_connected_graph_last", "visfd_hip_label_connected_graph_last_times"]
REASONS = ("ASYMMETRIC", "ZERO_DOT", "UNBALANCED", "MUST_LINK", "WEIGHTS", "OUTWARD", "LIMITS")


def test_header_binding_and_cpp_header_agree():
    text = open(os.path.join(ROOT, "include", "visfd_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    L = ctypes.CDLL(api.LIB_PATH)
    for name in NEW_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, code), name
        assert hasattr(L, name) and name in api.exported_symbols(), name
    for k, name in enumerate(("DEVICE", "HOST_GRAPH", "FLOOD")):
        assert re.search(r"#define\s+VISFD_HIP_CONNECT_GRAPH_%s\s+%d\b" % (name, k), code), name
        assert getattr(api, "CONNECT_GRAPH_" + name) == k
    for name in REASONS:      # the bit values of the restatement, HALO left out
        bit = getattr(cg, name)
        assert re.search(r"#define\s+VISFD_HIP_CONNECT_REASON_%s\s+%d\b" % (name, bit), code), name
        assert getattr(api, "CONNECT_REASON_" + name) == bit
    assert not re.search(r"VISFD_HIP_CONNECT_REASON_HALO", text) and not hasattr(api, "CONNECT_REASON_HALO")
    ex = api._SIGS["visfd_hip_label_connected_ex"][1]
    assert api._SIGS["visfd_hip_label_connected_graph_host"][1] == ex
    for name in NEW_SYMBOLS[:2]:
        assert api._SIGS[name][1][1:] == ex and api._SIGS[name][1] == api._SIGS["visfd_hip_label_connected_device_seeds"][1]
    hpp = open(os.path.join(ROOT, "include", "visfd_hip.hpp")).read()
    for name in ("LabelConnectedGraph(", "visfd_hip_label_connected_graph(ctx,", "visfd_hip_label_connected_graph_host("):
        assert name in hpp, name
    # the contract is stated where the halo is
    assert "halo" in text[text.index("AS A GRAPH PROBLEM"):text.index("#define VISFD_HIP_CONNECT_GRAPH_DEVICE")]


@pytest.fixture(scope="module")
def tv_jobs(oracle):
    return cc.tv_jobs(*tc.tv_outputs(oracle))


def _walk(name, sal, ten, d, case):
    """the host walk on one call, the contract checked -> (path, reasons, expected reasons)"""
    got = cc.run_host_walk(sal, ten, d, case)
    path, reasons, n_valid, n_undecided = api.label_connected_graph_last()
    cc.check(name, got, sal, ten, d, case)
    _, want, want_valid, want_candidates = cc.reference(name, sal, ten, d, case)
    assert reasons == want, (name, cg.reason_names(reasons), cg.reason_names(want))
    assert path == (api.CONNECT_GRAPH_FLOOD if want else api.CONNECT_GRAPH_HOST_GRAPH), (name, path)
    if not want & (cg.MUST_LINK | cg.WEIGHTS | cg.LIMITS):
        assert n_valid == want_valid, (name, n_valid, want_valid)
        assert n_undecided == want_candidates, (name, n_undecided, want_candidates)
        assert ("v" in case.get("use", "")) or n_undecided == 0, name
    return path, reasons, want


def test_host_walk_keeps_the_contract_on_every_tensor_voting_call(tv_jobs):
    graph_path = 0
    for job in tv_jobs:
        path, reasons, want = _walk(*job)
        graph_path += path == api.CONNECT_GRAPH_HOST_GRAPH
    assert graph_path >= cc.N_TG
    # the 34 calls of test_connect_graph.py carry no reason but HALO: the graph path every time
    for job in tv_jobs[-cc.N_TG:]:
        assert cc.reference(*job)[1] == 0, job[0]


def test_the_flood_turns_a_halo_and_the_graph_entries_do_not(tv_jobs):
    """the CLI's call (raw eigenvectors, standardised): the flood rewrites unlabelled voxels' directions, the walk none"""
    name, sal, ten, d, case = tv_jobs[2]
    flood = cc.reference(name, sal, ten, d, case)[0]
    unlabelled = flood[0] == -1
    assert (flood[5].view(np.uint32) != d.view(np.uint32)).any(-1)[unlabelled].sum() > 100
    got = cc.run_host_walk(sal, ten, d, case)
    assert not (got[5].view(np.uint32) != d.view(np.uint32)).any(-1)[unlabelled].any()
    assert (got[5].view(np.uint32) != d.view(np.uint32)).any(-1)[~unlabelled].any()      # and does standardise the clusters


@pytest.mark.parametrize("shape", cc.SHAPES, ids=lambda s: "%dx%dx%d" % (s[2], s[1], s[0]))
def test_small_shapes_and_their_share_of_clean_calls(shape):
    """the calls of the GPU test on the host walk; with the fixed generator seed at least three quarters of each shape's
    calls must have no reason beyond HALO (the GPU test needs them on the device path), the rest agree through the flood"""
    clean = total = 0
    for conn in (1, 2, 3):
        for job in cc.shape_jobs(shape, conn):
            path, reasons, want = _walk(*job)
            total += 1
            clean += want == 0
    assert total == 16 and 4 * clean >= 3 * total, (clean, total)
    if min(shape) >= 20:
        assert clean < total      # the fall-back has its share too: around the centre of a thick image no orientation exists


def _band_case():
    sal, direction = tg._twisted_band()
    return sal, direction, dict(threshold_saliency=float(np.exp(-0.5)), connectivity=3, consider_dot_product_sign=False,
                                use="v", standardize_directions=True, threshold_vector_saliency=-2.0)


@pytest.mark.parametrize("what", ["unbalanced", "must-link", "weights", "limits"])
def test_constructed_reasons_end_on_the_flood(what):
    sal, direction, case = _band_case()
    want = cg.UNBALANCED
    if what == "must-link":
        case.update(threshold_saliency=0.9, connectivity=1, must_link=[[(4.0, 12.0, 12.0), (19.0, 12.0, 12.0)]])
        want = cg.MUST_LINK
    elif what == "weights":
        case["voxel_weights"] = np.random.default_rng(2).uniform(0.5, 2, sal.shape).astype(np.float32)
        want = cg.WEIGHTS
    elif what == "limits":
        sal, _, direction, case = tg._small((9, 10, 11), 7, connectivity=5, consider_dot_product_sign=False)
        case["use"] = "v"
        want = cg.LIMITS
    name = "constructed " + what
    got = cc.run_host_walk(sal, None, direction, case)
    path, reasons, _, _ = api.label_connected_graph_last()
    assert path == api.CONNECT_GRAPH_FLOOD and reasons & want, (what, path, cg.reason_names(reasons))
    if what in ("must-link", "weights", "limits"):
        assert reasons == want
    cc.check(name, got, sal, None, direction, case)      # the flood's labelled results, the input's unlabelled directions
    assert got[1] >= 1


def test_open_half_band_is_oriented_by_the_walk():
    sal, direction, case = _band_case()
    half = sal.copy()
    half[:, :, 12:] = 0
    _walk("half band", half, None, direction, case)


@pytest.mark.parametrize("what", ["graph path", "flood path"])
def test_lists_too_small_leave_labels_and_directions_by_the_contract(what):
    """VISFD_HIP_ECAPACITY: the count is returned, and labels and directions are what a call with room would have left, on
    the graph path (the open half band) and through the flood (the whole band: UNBALANCED)"""
    sal, direction, case = _band_case()
    if what == "graph path":
        sal = sal.copy()
        sal[:, :, 12:] = 0
    kw, _, d_in, _ = cc.split(sal, None, direction, case)
    d_room = d_in.copy()
    room = api.label_connected_graph(sal, direction=d_room, label_undefined=-5, **kw)
    want_path = api.label_connected_graph_last()[0]
    assert want_path == (api.CONNECT_GRAPH_HOST_GRAPH if what == "graph path" else api.CONNECT_GRAPH_FLOOD) and room[1] >= 1
    L = api.load_library()
    nz, ny, nx = sal.shape
    labels = np.empty(sal.shape, np.int64)
    d = d_in.copy()
    n = ctypes.c_int64(0)
    cm = np.zeros(3, np.float32)
    rc = L.visfd_hip_label_connected_graph_host(sal.ctypes.data, labels.ctypes.data, None, nx, ny, nz, kw["threshold_saliency"],
                                                d.ctypes.data, kw["threshold_vector_saliency"], -np.inf, 0, None, -np.inf, -np.inf,
                                                1, kw["connectivity"], -5, 1, 1, 1, ctypes.byref(n), cm.ctypes.data, None, None, 0,
                                                None, None, None, 0, None)
    assert rc == 4 and n.value == room[1]      # VISFD_HIP_ECAPACITY
    assert api.label_connected_graph_last()[0] == want_path
    assert np.array_equal(labels, room[0]) and np.array_equal(d.view(np.uint32), d_room.view(np.uint32))


def test_refusals_before_any_allocation():
    L = api.load_library()
    s = np.zeros((4, 4, 4), np.float32)
    lab = np.zeros((4, 4, 4), np.int64)
    n = ctypes.c_int64(0)
    tail = [s.ctypes.data, lab.ctypes.data, None, 4, 4, 4, 0.5, None, 0.0, 0.0, 1, None, 0.0, 0.0, 1, 1, -1, 1, 0, 1,
            ctypes.byref(n), None, None, None, 0, None, None, None, 0, None]
    EINVAL = 1
    for fn in (L.visfd_hip_label_connected_graph, L.visfd_hip_label_connected_graph_dev):
        assert fn(None, *tail) == EINVAL and b"null context" in L.visfd_hip_last_error()
    assert L.visfd_hip_label_connected_graph_host(*tail) == 0 and n.value == 0
    before = api.label_connected_graph_last()
    narrow = list(tail)
    narrow[3] = 2                                       # a 2-wide image
    assert L.visfd_hip_label_connected_graph_host(*narrow) == EINVAL and b"at least 3 voxels" in L.visfd_hip_last_error()
    null = list(tail)
    null[0] = None                                      # a null image
    assert L.visfd_hip_label_connected_graph_host(*null) == EINVAL and b"null image" in L.visfd_hip_last_error()
    huge = list(tail)
    huge[3:6] = [1 << 11, 1 << 10, 1 << 10]             # 2^31 voxels: refused before a voxel is read or a byte allocated
    assert L.visfd_hip_label_connected_graph_host(*huge) == EINVAL and b"too large" in L.visfd_hip_last_error()
    assert api.label_connected_graph_last() == before   # a refused call leaves the record alone
    assert L.visfd_hip_label_connected_graph_last(None, None, None, None, None) == EINVAL
    with pytest.raises(api.VisfdHipError):
        api.label_connected_graph(np.zeros((2, 8, 8), np.float32), 0.0)


def test_cpp_function_and_host_walk_in_a_program(tmp_path):
    exe = str(tmp_path / "shim_connect_graph_check")
    libdir = os.path.dirname(api.LIB_PATH)
    subprocess.check_call(["g++", "-std=c++11", "-O1", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "shim_connect_graph_check.cpp"), "-o", exe, "-L" + libdir,
                           "-lvisfd_hip", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "shim connect graph check ok" in r.stdout, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
