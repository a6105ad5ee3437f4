"""DiscardOverlappingBlobs as an order-free statement, without a GPU: the all-pairs numpy form (tests/overlap_np.py) against
the sequential host entry (csrc/blob_post.cpp), the compiled reference (oracle/_ref, when present) and the reference's
recorded outputs (tests/golden/overlap.npz, made by tests/golden/make_golden_overlap.py) on the lists of
tests/overlap_cases.py; the mutants that show the lists can tell a wrong statement from the right one; the bounds formula;
and the agreement of header, binding and option table on what csrc/discard_overlap.hip adds.  The device entries
themselves are in tests/test_overlap_gpu.py."""
import ctypes
import os
import re

import numpy as np
import pytest

import overlap_np as on
from conftest import ROOT, golden
from overlap_cases import CASES
from visfd_amd import api


def same_bits(a, b):
    return len(a) == len(b) and all(np.asarray(x).shape == np.asarray(y).shape and
                                    np.array_equal(np.asarray(x, np.float32).view(np.uint32), np.asarray(y, np.float32).view(np.uint32))
                                    for x, y in zip(a, b))


@pytest.fixture(scope="module")
def statement():
    """the numpy statement's kept lists, computed once: name -> (crds, diameters, scores, info)"""
    out = {}
    for name, (c, d, s, sep, ml, ms, crit, scale) in CASES.items():
        info = {}
        out[name] = on.discard_overlapping_blobs(c, d, s, sep, ml, ms, crit, scale, info=info) + (info,)
    return out


def test_statement_equals_host_entry(statement):
    for name, (c, d, s, sep, ml, ms, crit, scale) in CASES.items():
        assert same_bits(statement[name][:3], api.discard_overlapping_blobs(c, d, s, sep, ml, ms, crit, scale)), name


def test_statement_equals_reference(statement, ref):
    for name, (c, d, s, sep, ml, ms, crit, scale) in CASES.items():
        assert same_bits(statement[name][:3], ref.discard_overlapping_blobs(c, d, s, sep, ml, ms, crit, scale)), name


def test_statement_equals_recorded_reference(statement):
    g = golden("overlap")
    assert sorted(g.files) == sorted(name + t for name in CASES for t in ("_c", "_d", "_s"))
    for name in CASES:
        assert same_bits(statement[name][:3], (g[name + "_c"], g[name + "_d"], g[name + "_s"])), name


def test_the_lists_are_what_they_claim(statement):
    assert statement["chain48"][3]["rounds"] == 48 and len(statement["chain48"][1]) == 24
    assert list(statement["tsz0"][3]["tsz"]) == [0, 0, 0] and len(statement["tsz0"][1]) == 10
    assert list(statement["tsz1"][3]["tsz"]) == [1, 1, 1]
    assert len(statement["dense"][1]) < 50                       # almost everything goes
    assert max(v[3]["rounds"] for k, v in statement.items() if k != "chain48") <= 14   # random lists: short chains
    # centre cells on both sides of the table
    c, d, s = CASES["negative"][:3]
    bmin, bmax = on.bounds_formula(c, d)
    C, _ = on.cells(c, d, bmin, 6)
    assert (C < 0).any() and (C >= (1 + bmax - bmin) // 6).any()


@pytest.mark.parametrize("mutant", ["cell_rule", "predecessors_only", "reverse_ties"])
def test_mutants_change_the_kept_set(statement, mutant):
    """no cell rule; k < i dropped; descending ties to the smaller index: each must show on some list"""
    changed = [name for name, (c, d, s, sep, ml, ms, crit, scale) in CASES.items()
               if not same_bits(statement[name][:3],
                                on.discard_overlapping_blobs(c, d, s, sep, ml, ms, crit, scale, **{mutant: False}))]
    assert changed, mutant
    if mutant == "cell_rule":
        assert {"cells_a", "cells_b", "cells_c"} <= set(changed)


def test_the_two_forms_of_share_agree():
    c, d, s, sep, ml, ms, crit, scale = CASES["negative_volume"]
    order = on.rank(s, crit)
    c, d = c[order], d[order]
    bmin, bmax = on.bounds_formula(c, d)
    tsz = (1 + bmax - bmin) // scale
    C, R = on.cells(c, d, bmin, scale)
    ii, kk = np.nonzero(np.tril(np.ones((len(d), len(d)), bool), -1))
    table = on.share_table(C, R, tsz)
    assert np.array_equal(on.share_pairs(C, R, tsz, ii, kk), table[ii, kk])
    far = C[:, None, :] - C[None, :, :]
    pre = (far * far).sum(2) <= (R[:, None] + R[None, :]) ** 2
    assert not (table & ~pre).any() and (pre & ~table).any()      # necessary, and not sufficient


def test_bounds_formula_equals_the_sequential_loop():
    for name, (c, d, s, *_rest) in CASES.items():
        for a, b in zip(on.bounds_formula(c, d), on.bounds_sequential(c, d)):
            assert np.array_equal(a, b), name
    rng = np.random.default_rng(9)
    for _ in range(50):
        n = int(rng.integers(1, 40))
        c = rng.uniform(-9.0, 9.0, (n, 3)).astype(np.float32)
        d = rng.uniform(0.0, 5.0, n).astype(np.float32)
        for a, b in zip(on.bounds_formula(c, d), on.bounds_sequential(c, d)):
            assert np.array_equal(a, b)


def test_rank_is_sort_blobs():
    for name in ("ties_crit1", "zeros_crit1", "post0"):
        c, d, s = CASES[name][:3]
        for crit in range(1, 5):
            assert np.array_equal(on.rank(s, crit), api.sort_blobs(c, d, s, crit, False)[3].astype(np.int64)), (name, crit)


def test_host_keyword_none_is_the_host_entry():
    c, d, s, sep, ml, ms, crit, scale = CASES["post0"]
    assert same_bits(api.discard_overlapping_blobs(c, d, s, sep, ml, ms, crit, scale, ctx=None),
                     api.discard_overlapping_blobs(c, d, s, sep, ml, ms, crit, scale))


def test_program_keeps_small_lists_on_the_host(tmp_path):
    """filter_mrc -discard-blobs: below DISCARD_OVERLAP_MIN_BLOBS the walk stays on the host and needs no GPU; the
    environment override makes the program say so; the output is the host entry's list"""
    from overlap_cases import run_discard_blobs
    cli = os.path.join(ROOT, "visfd_amd", "cli", "filter_mrc")
    image = os.path.join(ROOT, "tests", "golden", "test_blob_detect.rec")
    case = CASES["post0"]
    plain, err0 = run_discard_blobs(cli, image, str(tmp_path), case, None, "plain")
    forced, err1 = run_discard_blobs(cli, image, str(tmp_path), case, "1e30", "forced")
    assert "(discard_overlap:" not in err0 and "  (discard_overlap: host)\n" in err1
    assert plain == forced
    want = api.discard_overlapping_blobs(*case)
    rows = np.array([[float(t) for t in ln.split()] for ln in plain.decode().strip().split("\n")], np.float32)
    assert len(rows) == len(want[1]) and np.array_equal(rows[:, :3], want[0]) and "%d blobs remaining" % len(rows) in err0
    src = open(os.path.join(ROOT, "visfd_amd", "cli", "filter_mrc.cpp")).read()
    m = re.search(r"const double DISCARD_OVERLAP_MIN_BLOBS = ([0-9.]+);", src)
    assert m and float(m.group(1)) == 2.0 ** round(np.log2(float(m.group(1)))), "a measured power of two"
    assert "profiles/discard_overlap_time.txt" in src and os.path.exists(os.path.join(ROOT, "profiles", "discard_overlap_time.txt"))


NEW_SYMBOLS = ["visfd_hip_discard_overlapping_blobs_ctx", "visfd_hip_discard_overlapping_blobs_dev",
               "visfd_hip_discard_overlapping_blobs_last", "visfd_hip_discard_overlapping_blobs_last_times"]


def test_abi_header_and_binding_agree():
    text = open(os.path.join(ROOT, "include", "visfd_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    L = ctypes.CDLL(api.LIB_PATH)
    for name in NEW_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, code), name
        assert hasattr(L, name) and name in api.exported_symbols(), name
    for macro in ("PATH_DEVICE", "PATH_HOST", "PATH_HANDED_OVER", "REASON_NONE", "REASON_NONFINITE", "REASON_NEGATIVE",
                  "REASON_COUNT", "REASON_BOUNDS", "REASON_CELLS", "REASON_ROUNDS"):
        value = int(re.search(r"#define VISFD_HIP_DISCARD_OVERLAP_%s (\d+)" % macro, text).group(1))
        assert value == getattr(api, "DISCARD_OVERLAP_" + macro), macro
    assert len(api.DISCARD_OVERLAP_LAST_FIELDS) == 8
    table = open(os.path.join(ROOT, "visfd_amd", "csrc", "context.hip")).read()
    for opt in ("discard_overlap_host", "discard_overlap_max_rounds", "discard_overlap_time"):
        assert re.search(r"\bVH_OPT\(%s\)" % opt, table), opt
        assert re.search(r"^ \*   %s\b" % opt, text, flags=re.M), opt
    assert "int discard_overlap_max_rounds = 256;" in open(os.path.join(ROOT, "visfd_amd", "csrc", "common.hpp")).read()
    hpp = open(os.path.join(ROOT, "include", "visfd_hip.hpp")).read()
    assert re.search(r"DiscardOverlappingBlobs\(visfd_hip_ctx\* ctx,", hpp)
    from visfd_amd import build
    assert "discard_overlap.hip" in build.SOURCES
    # the context entries refuse what they cannot take before they touch a device
    P = ctypes.c_void_p
    n = ctypes.c_int64(1)
    for fn in (L.visfd_hip_discard_overlapping_blobs_ctx, L.visfd_hip_discard_overlapping_blobs_dev):
        fn.restype = ctypes.c_int
        fn.argtypes = [P, P, P, P, ctypes.POINTER(ctypes.c_int64)] + 3 * [ctypes.c_float] + 2 * [ctypes.c_int]
        assert fn(None, None, None, None, ctypes.byref(n), 1.0, 1.0, 1.0, 3, 6) == 1
    assert L.visfd_hip_discard_overlapping_blobs_last(None, None) == 1
