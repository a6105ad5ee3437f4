"""Local minima and maxima, CPU side: the numpy restatement (tests/extrema_np.py) against what the reference program
wrote for every recorded case (tests/golden/extrema.npz: text lists byte for byte, label images voxel for voxel), the
argument checks of visfd_hip_find_extrema[_dev], and the filter_mrc flags' argument errors.  No GPU needed: every
argument check of the ABI comes before the context is touched."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import extrema_cases as EC
import extrema_np
from conftest import GOLDEN, ROOT, golden

CLI = os.path.join(ROOT, "visfd_amd", "cli", "filter_mrc")
BLOB = os.path.join(GOLDEN, "test_blob_detect.rec")


def list_text(lst, shape, voxel_width=1.0):
    """The reference's text file (handlers.cpp:1219-1244): x*w y*w z*w nvoxels score at the stream's default precision
    (%g of the float coordinates times the float width, and of the float score)."""
    nz, ny, nx = shape
    w = np.float32(voxel_width)
    lines = []
    for i, s, n in zip(*lst):
        x, y, z = i % nx, (i // nx) % ny, i // (nx * ny)
        lines.append("%g %g %g %d %g\n" % (np.float32(x) * w, np.float32(y) * w, np.float32(z) * w, n, s))
    return "".join(lines).encode()


@pytest.fixture(scope="module")
def recorded():
    return golden("extrema")


@pytest.mark.parametrize("case", EC.golden_cases(), ids=EC.case_name)
def test_restatement_equals_reference_program(recorded, case):
    name = EC.case_name(case)
    src = recorded["vol/" + case[0]]
    mask = recorded["mask/" + case[0]] if case[1] else None
    r = extrema_np.find_extrema(src, mask, **EC.case_arguments(case))
    assert list_text(r["min"], src.shape) == recorded[name + "/min_txt"].tobytes()
    assert list_text(r["max"], src.shape) == recorded[name + "/max_txt"].tobytes()
    assert np.array_equal(r["labels"], recorded[name + "/labels"])


def test_recording_covers_what_it_must(recorded):
    cases = EC.golden_cases()
    assert {c[2] for c in cases} == {"min", "max", "both"} and {c[3] for c in cases} == {1, 2, 3}
    assert {c[1] for c in cases} == {False, True} and {c[4] for c in cases} == {False, True}
    vols, masks = EC.golden_volumes()
    for k in vols:   # the generators still make the recorded inputs
        assert np.array_equal(vols[k].view(np.uint32), recorded["vol/" + k].view(np.uint32)), k
        assert np.array_equal(masks[k], recorded["mask/" + k]), k
        assert max(vols[k].shape) <= 48
    # thresholds that some extrema fail: the thresholded lists are shorter than the free ones, and not empty
    for vol in ("quant", "smooth"):
        for kind, key in (("min", "/min_txt"), ("max", "/max_txt")):
            free = recorded[EC.case_name((vol, False, kind, 3, True, False)) + key].tobytes().count(b"\n")
            thr = recorded[EC.case_name((vol, False, kind, 3, True, True)) + key].tobytes().count(b"\n")
            assert 0 < thr < free, (vol, kind, thr, free)


# ---- the C ABI's argument checks ------------------------------------------------------------------------------------
EINVAL, ECAPACITY = 1, 4


def _call(L, name, src, mask, shape, connectivity=3, labels=None, caps=(0, 0), lists=None, find=(1, 1), ctx=None):
    nz, ny, nx = shape
    n = [C.c_int64(-1), C.c_int64(-1)]
    lists = lists or [(None, None, None), (None, None, None)]
    tail = []
    for k in range(2):
        tail += list(lists[k]) + [caps[k], C.byref(n[k])]
    rc = getattr(L, name)(ctx, src, mask, nx, ny, nz, find[0], find[1], float("inf"), -float("inf"), connectivity, 1,
                          *(tail + [labels]))
    return rc, L.visfd_hip_last_error().decode()


@pytest.mark.parametrize("name", ["visfd_hip_find_extrema", "visfd_hip_find_extrema_dev"])
def test_abi_argument_checks(name):
    from visfd_amd import api
    L = api.load_library()
    assert name in api.exported_symbols()
    v = np.zeros((4, 5, 6), np.float32)
    lab = np.zeros((4, 5, 6), np.int32)
    p = v.ctypes.data
    for c in (0, 4, -1, 9):
        rc, msg = _call(L, name, p, None, v.shape, connectivity=c)
        assert rc == EINVAL and "connectivity must be 1, 2 or 3" in msg, (c, msg)
    rc, msg = _call(L, name, p, None, v.shape, labels=p)
    assert rc == EINVAL and "labels overlap src" in msg, msg
    rc, msg = _call(L, name, p, p + 16, v.shape, labels=p + 32)
    assert rc == EINVAL and "labels overlap" in msg, msg
    m = np.ones((4, 5, 6), np.float32)
    rc, msg = _call(L, name, p, m.ctypes.data, v.shape, labels=m.ctypes.data + 4 * (v.size - 1))
    assert rc == EINVAL and "labels overlap mask" in msg, msg
    # 2^31 - 2 voxels and more are refused, one fewer passes this check (and stops at the missing context)
    rc, msg = _call(L, name, p, None, (2, 1, 2 ** 30 - 1))
    assert rc == EINVAL and "fewer than 2^31 - 2 voxels" in msg, msg
    rc, msg = _call(L, name, p, None, (5, 1, 429496729))          # 2^31 - 3 voxels
    assert rc == EINVAL and msg == "null argument", msg
    rc, msg = _call(L, name, p, None, (2 ** 20, 2 ** 20, 2 ** 20))
    assert rc == EINVAL and "fewer than 2^31 - 2 voxels" in msg, msg
    # the classification launch's own limits: ny, nz <= 524280, fewer than 2^24 tiles of 64 x 8 x 8
    rc, msg = _call(L, name, p, None, (1, 524281, 64))
    assert rc == EINVAL and "at most 524280" in msg, msg
    rc, msg = _call(L, name, p, None, (524288, 1, 64))
    assert rc == EINVAL and "at most 524280" in msg, msg
    rc, msg = _call(L, name, p, None, (1, 524280, 64))
    assert rc == EINVAL and msg == "null argument", msg
    rc, msg = _call(L, name, p, None, (32768, 32768, 1))          # 4096 x 4096 tiles
    assert rc == EINVAL and "2^24 - 1 tiles" in msg, msg
    rc, msg = _call(L, name, p, None, (0, 5, 6))
    assert rc == EINVAL and "positive" in msg, msg
    rc, msg = _call(L, name, p, None, v.shape, find=(0, 0))
    assert rc == EINVAL and "neither minima nor maxima" in msg, msg
    rc, msg = _call(L, name, p, None, v.shape, caps=(-1, 0))
    assert rc == EINVAL and "negative list capacity" in msg, msg
    # the count-only call (capacities 0, no arrays) and a call with labels pass every check up to the context
    rc, msg = _call(L, name, p, None, v.shape, labels=lab.ctypes.data)
    assert rc == EINVAL and msg == "null argument", msg
    rc, msg = _call(L, name, None, None, v.shape)
    assert rc == EINVAL and msg == "null argument", msg


def test_header_documents_the_limits():
    text = open(os.path.join(ROOT, "include", "visfd_hip.h")).read()
    assert "#define VISFD_HIP_EXTREMA_MAX_CONNECTIVITY 3" in text
    assert "#define VISFD_HIP_EXTREMA_MAX_VOXELS 2147483645LL" in text   # 2^31 - 3: one below the refused 2^31 - 2
    assert "#define VISFD_HIP_EXTREMA_MAX_NY_NZ 524280" in text


# ---- filter_mrc's flags ----------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def cli():
    if not os.path.exists(CLI):
        from visfd_amd import build
        build.build(verbose=False)
    return CLI


def _run(cli, args):
    return subprocess.run([cli, "-in", BLOB] + args, capture_output=True, text=True)


@pytest.mark.parametrize("flag", ["-find-minima", "-find-maxima"])
def test_cli_find_flag_needs_a_file_name(cli, flag):
    r = _run(cli, [flag])
    assert r.returncode == 1, r.stderr
    assert "Error: The %s argument must be followed by a number.\n" % flag in r.stderr, r.stderr   # settings.cpp:2211-2212
    assert "Unrecognized" not in r.stderr


@pytest.mark.parametrize("tail", [[], ["0"], ["-2"], ["abc"]])
def test_cli_neighbor_connectivity_needs_a_positive_integer(cli, tail):
    r = _run(cli, ["-find-minima", "m.txt", "-neighbor-connectivity"] + tail)
    assert r.returncode == 1, r.stderr
    assert "Error: The -neighbor-connectivity argument must be followed by a positive integer.\n" in r.stderr, r.stderr
    assert "Unrecognized" not in r.stderr


@pytest.mark.parametrize("n", ["4", "27"])
def test_cli_neighbor_connectivity_above_three_names_the_limit(cli, n):
    r = _run(cli, ["-find-maxima", "m.txt", "-neighbor-connectivity", n])
    assert r.returncode == 1 and "must be 1, 2 or 3" in r.stderr, r.stderr


@pytest.mark.parametrize("flags", [["-find-minima", "m.txt"], ["-find-maxima", "m.txt", "-ignore-boundary-extrema"],
                                   ["-find-minima", "a.txt", "-find-maxima", "b.txt", "-boundary-extrema",
                                    "-neighbor-connectivity", "2"]])
def test_cli_extrema_refused_under_slab(cli, flags, tmp_path):
    r = subprocess.run([cli, "-in", BLOB] + flags + ["-w", "1", "-slab", "0", "1", "-"], capture_output=True, text=True,
                       cwd=str(tmp_path))
    assert r.returncode == 1 and "-slab runs with" in r.stderr, r.stderr
    assert "Unrecognized" not in r.stderr
