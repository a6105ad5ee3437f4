"""The exact distance maps without a GPU: the two forms of the numpy restatement (tests/distance_np.py) against each other,
the restatement of -distance-points / -distance-to-voxels against what the reference program wrote
(tests/golden/distance.npz): images bit for bit, distance files as text; and the argument errors of the two flags."""
import os
import subprocess

import numpy as np
import pytest

import distance_cases as dc
import distance_np as dn
import intensity_np as inp
from conftest import ROOT, assert_bits_equal, golden


def seed_image(shape, density, seed):
    rng = np.random.default_rng(seed)
    return (rng.random(shape) < density).astype(np.float32)


@pytest.mark.parametrize("shape", [(1, 1, 1), (1, 1, 17), (1, 17, 1), (17, 1, 1), (3, 5, 9), (6, 7, 8)])
@pytest.mark.parametrize("density", [0.0, 0.02, 0.3, 1.0])
def test_separable_form_equals_brute_force(shape, density):
    src = seed_image(shape, density, seed=sum(shape))
    mask = seed_image(shape, 0.8, seed=3)
    pts = np.array([[-3, 1, 2], [0, 0, 0], [shape[2] - 1, shape[1] - 1, shape[0] - 1], [1000, 0, 0], [2, 40, -1]])
    for kw in (dict(src=src, lo=0.5, hi=1.5), dict(src=src, mask=mask, lo=0.5, hi=1.5), dict(points=pts),
               dict(points=pts, src=src, mask=mask, lo=0.5, hi=1.5), dict()):
        a = dn.distance_sq_brute(shape, **kw)
        b = dn.distance_sq_separable(shape, **kw)
        assert a.dtype == np.int32
        assert_bits_equal(a, b, "%s %s" % (shape, sorted(kw)))
        assert a.max() <= dn.cap_of(shape)
        if not kw or (density == 0.0 and "points" not in kw):
            assert (a == dn.cap_of(shape)).all()


def test_nan_is_never_selected_and_mask_counts():
    src = np.array([[[np.nan, 1.0, 5.0, np.nan]]], np.float32)
    mask = np.array([[[1.0, 0.0, 1.0, 1.0]]], np.float32)
    assert dn.selection(src, None, -np.inf, np.inf).tolist() == [[[False, True, True, False]]]
    assert dn.selection(src, mask, 0.0, 9.0).tolist() == [[[False, False, True, False]]]
    assert dn.distance_from_points(src, [[0, 0, 0], [6, 0, 0], [9, 0, 0]], 0.0, 9.0, 1.0, mask).tolist() == [2.0, 4.0, 6.0]   # the last: cap
    assert dn.distance_from_points(src, [[0, 0, 0]], 6.0, 9.0, 2.5, mask).tolist() == [15.0]   # nothing selected: cap = 6^2


def test_root_rounds_every_step_to_float():
    """w = 1.3 is not dyadic: w * w is rounded to float before it meets (float)dsq, and dsq beyond 2^24 is rounded too"""
    w = np.float32(1.3)
    ww = np.float32(w * w)
    assert float(ww) != float(w) * float(w)
    d = np.array([4097 ** 2, 4199 ** 2, 7], np.int64)
    assert int(np.float32(4097 ** 2)) != 4097 ** 2
    assert_bits_equal(dn.root(d, 1.3), np.sqrt(d.astype(np.float32) * ww), "root")
    assert dn.root([18 * 18], 2.5).tolist() == [45.0]   # the measured value of an empty point set on 5 x 6 x 7, w = 2.5


def test_integer_points_conversion():
    w = [np.float32(2.5)] * 3
    assert dn.integer_points([[5.0, 7.5, 2.5], [-6.0, 10.0, 3.74]], w, False).tolist() == [[2, 3, 1], [-2, 4, 1]]
    assert dn.integer_points([[3, 4, 5], [0, 4, 12]], w, True).tolist() == [[2, 3, 4], [-1, 3, 11]]
    crds, in_voxels = dn.read_points_text(dc.POINT_FILES["imod.txt"])
    assert in_voxels and crds.tolist() == [[2, 3, 4], [6, 0, 8], [0, 7, 1], [-1, 3, 11]]
    crds, in_voxels = dn.read_points_text(dc.POINT_FILES["phys.txt"])
    assert not in_voxels and len(crds) == 5
    assert dn.format_distances(np.array([45, 2.5, 0, 12.747549], np.float32)) == "45\n2.5\n0\n12.7475\n"


def test_golden_holds_the_cases_inputs():
    gold = golden("distance")
    for name, (vol, mask) in dc.inputs().items():
        assert_bits_equal(gold["in/" + name], vol, name)
        assert_bits_equal(gold["mask/" + name], mask, name)
    for name, body in dc.POINT_FILES.items():
        assert gold["points/" + name].tobytes().decode() == body
    assert {k.split("/")[1] for k in gold.files if k.startswith("out/")} == set(dc.CASES)


@pytest.mark.parametrize("name", list(dc.CASES))
def test_restatement_reproduces_the_reference(name):
    gold = golden("distance")
    case = dc.CASES[name]
    vol, mask = dc.inputs()[case["input"]]
    image, text = dn.run_case(case, vol, mask, dc.POINT_FILES, inp.tail)
    assert_bits_equal(image, gold["out/" + name], name)
    if dc.writes_distances(case):
        assert text == gold["dist/" + name].tobytes().decode(), name
    else:
        assert text is None and ("dist/" + name) not in gold.files


# ---- filter_mrc's parser: decided before any image is read or a device is looked for ---------------------------------
PARSER_CASES = [
    ("points_last", ["-distance-points"],
     "Error: The -distance-points argument must be followed by a file name.\n"),
    ("voxels_three_operands", ["-distance-to-voxels", "queries.txt", "dist.txt", "3"],
     "Error: The -distance-to-voxels argument must be followed by two file names and two numbers:\n"
     "       InFile OutFile BrightnessSelectMin BrightnessSelectMax\n"),
    ("voxels_last", ["-distance-to-voxels"],
     "Error: The -distance-to-voxels argument must be followed by two file names and two numbers:\n"
     "       InFile OutFile BrightnessSelectMin BrightnessSelectMax\n"),
    ("points_slab", ["-slab", "0", "1", "-", "-distance-points", "phys.txt"],
     "Error: -slab does not combine with -distance-points: a distance map needs the whole image in one process.\n"),
    ("voxels_slab", ["-distance-to-voxels", "queries.txt", "dist.txt", "3", "6", "-slab", "0", "1", "-"],
     "Error: -slab does not combine with -distance-to-voxels: a distance map needs the whole image in one process.\n"),
    ("points_then_input_missing", ["-distance-points", "phys.txt", "-distance-points", "imod.txt"],
     "Error: Unable to open \"missing.rec\" for reading.\n"),   # both flags parse: the run gets as far as the input file
    ("voxels_then_input_missing", ["-distance-to-voxels", "queries.txt", "dist.txt", "3", "6"],
     "Error: Unable to open \"missing.rec\" for reading.\n"),
]


@pytest.mark.parametrize("name,args,message", PARSER_CASES, ids=[c[0] for c in PARSER_CASES])
def test_cli_parser(name, args, message, tmp_path):
    cli = os.path.join(ROOT, "visfd_amd", "cli", "filter_mrc")
    if not os.path.exists(cli):
        from visfd_amd import build
        build.build(verbose=False)
    r = subprocess.run([cli, "-in", "missing.rec"] + args, capture_output=True, text=True, cwd=tmp_path)
    banner, _, tail = r.stderr.partition("\n")
    assert banner.startswith("filter_mrc (")
    assert (r.returncode, r.stdout, tail) == (1, "", "\n" + message + "\n")
