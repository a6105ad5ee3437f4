"""Watershed, CPU side: the heapq restatement (tests/watershed_np.py) and the library's sequential flood
(visfd_hip_watershed_host, which needs neither a context nor a device) against what the reference program wrote for every
recorded case (tests/golden/watershed.npz, voxel for voxel), the capacity protocol of the basin lists, the refusals of
the three entry points, and filter_mrc's argument errors.  No GPU needed: every argument check of the ABI comes before the
context is touched."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import watershed_cases as WC
import watershed_np
from conftest import GOLDEN, ROOT, golden

CLI = os.path.join(ROOT, "visfd_amd", "cli", "filter_mrc")
BLOB = os.path.join(GOLDEN, "test_blob_detect.rec")
EINVAL, ECAPACITY = 1, 4
INF = float("inf")


@pytest.fixture(scope="module")
def recorded():
    return golden("watershed")


@pytest.fixture(scope="module")
def api():
    from visfd_amd import api
    api.load_library()
    return api


def case_inputs(recorded, case):
    vol, mk = case[0], case[6]
    src = recorded["vol/" + vol]
    mask = recorded["mask/" + vol] if case[1] else None
    markers = WC.rounded_markers(recorded["markers/%s/%s" % (mk, vol)]) if mk else None
    return src, mask, markers


@pytest.mark.parametrize("case", WC.golden_cases(), ids=WC.case_name)
def test_restatement_and_host_flood_equal_reference_program(recorded, api, case):
    src, mask, markers = case_inputs(recorded, case)
    expected = recorded[WC.case_name(case) + "/out"].astype(np.float32)
    kw = WC.case_arguments(case)
    lab, index, score = watershed_np.watershed(src, mask, markers, **kw)
    assert np.array_equal(watershed_np.program_output(lab, mask, case[8]), expected)
    lab2, index2, score2 = api.watershed_host(src, mask, markers, **kw)
    assert np.array_equal(watershed_np.program_output(lab2, mask, case[8]), expected)
    assert np.array_equal(lab2, lab)          # the -1 of voxels with mask == 0 too, which the program's output hides
    assert np.array_equal(index2, index) and np.array_equal(score2.view(np.uint32), score.view(np.uint32))


def test_recording_covers_what_it_must(recorded):
    cases = WC.golden_cases()
    assert len(set(map(WC.case_name, cases))) == len(cases)
    for vol in ("quant", "smooth"):
        full = {c[1:6] for c in cases if c[0] == vol and c[6] is None and c[7] == 0 and c[8] == "max"}
        assert len(full) == 2 * 2 * 3 * 2 * 2
    assert {c[0] for c in cases} == {"quant", "smooth", "special", "const", "binary", "ties", "thin"}
    assert {c[6] for c in cases} == {None} | set(WC.MARKERS)
    assert any(c[6] and c[5] for c in cases) and any(c[7] == 5 for c in cases) and any(c[8] == 7 for c in cases)
    vols, masks = WC.golden_volumes()
    for k in vols:   # the generators still make the recorded inputs
        assert np.array_equal(vols[k].view(np.uint32), recorded["vol/" + k].view(np.uint32)), k
        assert np.array_equal(masks[k], recorded["mask/" + k]), k
        assert max(vols[k].shape) <= 24 and not np.isnan(vols[k]).any()
    assert np.isinf(vols["special"]).any() and (np.signbit(vols["special"]) & (vols["special"] == 0)).any()
    # the recorded images hold boundaries, undefined voxels and several basins
    out = recorded[WC.case_name(("quant", False, "min", 3, True, True, None, 0, "max")) + "/out"]
    assert (out == 0).sum() > 100 and out.max() > 5 and (out == out.max()).sum() > 100
    hide = recorded[WC.case_name(("quant", False, "min", 3, False, True, None, 0, "max")) + "/out"]
    assert (hide == 0).sum() == 0
    # a marker that sits only on voxels with mask == 0 seeds nothing
    out = recorded[WC.case_name(("quant", True, "min", 1, True, False, "masked", 0, "max")) + "/out"]
    assert 8 not in out and 5 in out


def test_repeated_marker_label_is_one_seed(recorded, api):
    src = recorded["vol/quant"]
    markers = WC.rounded_markers(recorded["markers/repeated/quant"])
    lab, index, score = api.watershed_host(src, None, markers, connectivity=1)
    given = [int(v) for v in np.unique(markers) if v > 0]
    assert {2, 4, 6} <= set(given) and (markers == 4).sum() > 1
    first = [int(np.nonzero(markers.reshape(-1) == v)[0][0]) for v in given]
    assert index.tolist() == sorted(first)    # one seed per label, in raster order of first sight
    assert np.array_equal(score, src.reshape(-1)[index])
    # (the closing relabelling maps a basin to the LAST marker found on it, so a later voxel of a repeated label renames the
    # basin that flooded it: not every given label survives)
    assert set(np.unique(lab)) <= {0} | set(given)


# ---- the capacity protocol and the refusals -------------------------------------------------------------------------
def _call(L, name, src, mask, markers, shape, labels, thr=INF, from_min=1, c=3, cap=0, lists=(None, None), ctx=None,
          want_n=True):
    nz, ny, nx = shape
    n = C.c_int64(-7)
    args = [src, mask, markers, nx, ny, nz, thr, from_min, c, 1, 0, -1, labels, lists[0], lists[1], cap,
            C.byref(n) if want_n else None]
    if name != "visfd_hip_watershed_host":
        args = [ctx] + args
    rc = getattr(L, name)(*args)
    return rc, L.visfd_hip_last_error().decode(), n.value


def test_capacity_protocol_of_the_host_entry(recorded, api):
    L = api.load_library()
    src = np.ascontiguousarray(recorded["vol/smooth"])
    want_lab, want_idx, want_sc = watershed_np.watershed(src, connectivity=3)
    nb = len(want_idx)
    assert nb > 4
    lab = np.full(src.shape, 77, np.int32)
    # count only: the labels are written, the lists are not asked for
    rc, msg, n = _call(L, "visfd_hip_watershed_host", src.ctypes.data, None, None, src.shape, lab.ctypes.data)
    assert rc == 0 and n == nb and np.array_equal(lab, want_lab)
    # too small: the count and nothing else
    lab[:] = 77
    idx, sc = np.full(nb, -5, np.int64), np.full(nb, -5, np.float32)
    rc, msg, n = _call(L, "visfd_hip_watershed_host", src.ctypes.data, None, None, src.shape, lab.ctypes.data, cap=nb - 1,
                       lists=(idx.ctypes.data, sc.ctypes.data))
    assert rc == ECAPACITY and "too small" in msg and n == nb
    assert (lab == 77).all() and (idx == -5).all() and (sc == -5).all()
    # exactly enough, and either list alone
    rc, msg, n = _call(L, "visfd_hip_watershed_host", src.ctypes.data, None, None, src.shape, lab.ctypes.data, cap=nb,
                       lists=(idx.ctypes.data, sc.ctypes.data))
    assert rc == 0 and n == nb and np.array_equal(idx, want_idx) and np.array_equal(sc, want_sc) and np.array_equal(lab, want_lab)
    idx[:] = -5
    rc, msg, n = _call(L, "visfd_hip_watershed_host", src.ctypes.data, None, None, src.shape, lab.ctypes.data, cap=nb + 3,
                       lists=(idx.ctypes.data, None))
    assert rc == 0 and np.array_equal(idx, want_idx)


@pytest.mark.parametrize("name", ["visfd_hip_watershed_host", "visfd_hip_watershed", "visfd_hip_watershed_dev"])
def test_abi_argument_checks(api, name):
    L = api.load_library()
    assert name in api.exported_symbols() and "visfd_hip_watershed_last_stats" in api.exported_symbols()
    v = np.zeros((4, 5, 6), np.float32)
    lab = np.full((4, 5, 6), 77, np.int32)
    mk = np.zeros((4, 5, 6), np.int32)
    p, pl = v.ctypes.data, lab.ctypes.data
    for c in (0, 4, -1, 9):
        rc, msg, _ = _call(L, name, p, None, None, v.shape, pl, c=c)
        assert rc == EINVAL and "connectivity must be 1, 2 or 3" in msg, (c, msg)
    rc, msg, _ = _call(L, name, p, None, None, v.shape, pl, thr=float("nan"))
    assert rc == EINVAL and "threshold is NaN" in msg, msg
    rc, msg, _ = _call(L, name, p, None, None, v.shape, p)
    assert rc == EINVAL and "labels overlap src" in msg, msg
    m = np.ones((4, 5, 6), np.float32)
    rc, msg, _ = _call(L, name, p, m.ctypes.data, None, v.shape, m.ctypes.data + 4 * (v.size - 1))
    assert rc == EINVAL and "labels overlap mask" in msg, msg
    rc, msg, _ = _call(L, name, p, None, mk.ctypes.data, v.shape, mk.ctypes.data + 16)
    assert rc == EINVAL and "labels overlap markers" in msg, msg
    # the size limits of find_extrema
    rc, msg, _ = _call(L, name, p, None, None, (2, 1, 2 ** 30 - 1), pl)
    assert rc == EINVAL and "fewer than 2^31 - 2 voxels" in msg, msg
    rc, msg, _ = _call(L, name, p, None, None, (1, 524281, 64), pl)
    assert rc == EINVAL and "at most 524280" in msg, msg
    rc, msg, _ = _call(L, name, p, None, None, (32768, 32768, 1), pl)
    assert rc == EINVAL and "2^24 - 1 tiles" in msg, msg
    rc, msg, _ = _call(L, name, p, None, None, (0, 5, 6), pl)
    assert rc == EINVAL and "positive" in msg, msg
    rc, msg, _ = _call(L, name, p, None, None, v.shape, pl, cap=-1)
    assert rc == EINVAL and "negative list capacity" in msg, msg
    rc, msg, _ = _call(L, name, p, None, None, v.shape, pl, want_n=False)
    assert rc == EINVAL and "number of basins" in msg, msg
    rc, msg, _ = _call(L, name, None, None, None, v.shape, pl)
    assert rc == EINVAL and msg == "null argument", msg
    rc, msg, _ = _call(L, name, p, None, None, v.shape, None)
    assert rc == EINVAL and msg == "null argument", msg
    assert (lab == 77).all()
    if name != "visfd_hip_watershed_host":   # a call that passes every check stops at the missing context
        rc, msg, _ = _call(L, name, p, None, None, v.shape, pl)
        assert rc == EINVAL and msg == "null argument", msg
        assert (lab == 77).all()


def test_host_entry_refuses_unmasked_nans(api):
    L = api.load_library()
    v = np.arange(120, dtype=np.float32).reshape(4, 5, 6)
    v[1, 2, 3] = np.nan
    lab = np.full(v.shape, 77, np.int32)
    rc, msg, _ = _call(L, "visfd_hip_watershed_host", v.ctypes.data, None, None, v.shape, lab.ctypes.data)
    assert rc == EINVAL and "is NaN" in msg and (lab == 77).all()
    m = np.ones(v.shape, np.float32)
    m[1, 2, 3] = 0
    rc, msg, n = _call(L, "visfd_hip_watershed_host", v.ctypes.data, m.ctypes.data, None, v.shape, lab.ctypes.data)
    assert rc == 0 and n == 1 and lab[1, 2, 3] == -1 and (np.delete(lab.reshape(-1), 1 * 30 + 2 * 6 + 3) == 1).all()


def test_masked_voxels_hold_minus_one_whatever_label_undefined_is(recorded, api):
    src, mask = recorded["vol/quant"], recorded["mask/quant"]
    lab, _, _ = api.watershed_host(src, mask, halt_threshold=4.0, connectivity=2, label_undefined=-9, label_boundary=-3)
    want, _, _ = watershed_np.watershed(src, mask, halt_threshold=4.0, connectivity=2, label_undefined=-9, label_boundary=-3)
    assert np.array_equal(lab, want)
    assert (lab[mask == 0] == -1).all() and (lab[mask != 0] != -1).all() and (lab == -9).any() and (lab == -3).any()


def test_header_documents_the_watershed():
    text = open(os.path.join(ROOT, "include", "visfd_hip.h")).read()
    assert "#define VISFD_HIP_WATERSHED_MAX_BASINS 16777216" in text
    assert "#define VISFD_HIP_WATERSHED_PATH_HOST 0" in text and "#define VISFD_HIP_WATERSHED_PATH_DEVICE 1" in text
    assert "10 bytes per voxel" in text


# ---- filter_mrc's flags ----------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def cli():
    if not os.path.exists(CLI):
        from visfd_amd import build
        build.build(verbose=False)
    return CLI


def _run(cli, args, cwd=None):
    return subprocess.run([cli, "-in", BLOB] + args, capture_output=True, text=True, cwd=cwd)


@pytest.mark.parametrize("tail", [[], ["sideways"], ["-maxima"]])
def test_cli_watershed_needs_minima_or_maxima(cli, tail):
    r = _run(cli, ["-watershed"] + tail)
    assert r.returncode == 1, r.stderr
    assert "Error: The -watershed argument must be followed by an argument:" in r.stderr, r.stderr   # settings.cpp:2602-2605
    assert 'either "minima" or "maxima"' in r.stderr and "Unrecognized" not in r.stderr


@pytest.mark.parametrize("flag,what", [("-watershed-threshold", "a number"), ("-watershed-boundary", "a number"),
                                       ("-markers", "an image file name")])
def test_cli_watershed_flags_need_their_argument(cli, flag, what):
    r = _run(cli, ["-watershed", "minima", flag])
    assert r.returncode == 1, r.stderr
    assert "Error: The %s argument must be followed by %s\n" % (flag, what) in r.stderr, r.stderr
    assert "Unrecognized" not in r.stderr


@pytest.mark.parametrize("flags", [["-watershed", "minima"], ["-watershed-hide-boundaries"],
                                   ["-watershed", "max", "-watershed-threshold", "3", "-watershed-boundary", "2"]])
def test_cli_watershed_refused_under_slab(cli, flags, tmp_path):
    r = _run(cli, flags + ["-w", "1", "-slab", "0", "1", "-"], cwd=str(tmp_path))
    assert r.returncode == 1 and "-slab runs with" in r.stderr, r.stderr
    assert "Unrecognized" not in r.stderr
