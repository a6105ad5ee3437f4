"""DrawSpheres and DrawRegions, CPU side: the numpy restatement tests/draw_np.py -- the yardstick of the GPU tests -- against
images written by the real reference program (golden/draw.npz, recorded by golden/make_golden_draw.py), bitwise; and the
argument errors of the new filter_mrc flags, which need no GPU."""
import os
import subprocess

import numpy as np
import pytest

import draw_cases as DC
import draw_np as DN
from conftest import GOLDEN, ROOT, assert_bits_equal

CLI = os.path.join(ROOT, "visfd_amd", "cli", "filter_mrc")
BLOB = os.path.join(GOLDEN, "test_blob_detect.rec")
F = np.float32


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(GOLDEN, "draw.npz"))


def test_every_case_was_recorded(gold):
    """At most one case may be missing from the file (a reference run that did not exit 0); none is."""
    assert sorted(k[:-4] for k in gold.files if k.endswith("/out")) == sorted(DC.CLI_CASES)


def expected_image(name, gold):
    """The restatement's image for a case of DC.CLI_CASES (the blob cases are drawn from the recorded exact lists)."""
    case = DC.CLI_CASES[name]
    img, mask, text, w = DC.cli_inputs(name)
    if case.get("regions"):
        mask = DN.handle_mask_regions(img.shape, case["regions"], mask)
    if name in DC.BLOB_DETECT:
        sides = []
        for tag, fname, ascending in (("minima", DC.BLOB_DETECT[name]["files"][0], True),
                                      ("maxima", DC.BLOB_DETECT[name]["files"][1], False)):
            rows = gold[name + "/" + tag + "_exact"]
            dia, sc = (rows[:, 3] * F(w)).astype(F), rows[:, 4]
            if fname is not None:   # the file's order: by score, ties in list order; the coordinates stay as detected
                order = np.argsort(sc if ascending else -sc, kind="stable")
                dia, sc = dia[order], sc[order]
            sides.append((rows[:, :3], dia, sc))
        return DN.handle_blob_display(img, mask, sides[0], sides[1], w, **case["opts"])
    return DN.handle_draw_spheres(img, mask, DC.rows_of_text(text), w, **case["opts"])


DRAWN = sorted(n for n in DC.CLI_CASES if n != "maxima_thinned")


@pytest.mark.parametrize("name", DRAWN)
def test_restatement_matches_reference_program(gold, name):
    assert_bits_equal(expected_image(name, gold), gold[name + "/out"], name)


def test_reference_script_form_counts_centres(gold):
    """-background 0 -foreground 1 -sphere-radii 0 (tests/test_blob_detection.sh:35): one voxel per centre in the image."""
    img = gold["bg0_fg1_radii0/out"]
    assert int((img != 0).sum()) == DC.IN_IMAGE_CENTRES and set(np.unique(img)) == {0.0, 1.0}


def test_mask_cases_print_their_mask(gold):
    for name in ("mask_rect", "mask_sphere_minus_rect", "mask_subtract_first"):
        want = DN.handle_mask_regions(DC.CLI_SHAPE, DC.CLI_CASES[name]["regions"])
        assert_bits_equal((want != 0).astype(F), gold[name + "/out"], name)
    assert (gold["mask_subtract_first/out"] != 0).sum() > 1500      # the mask was filled with ones before the subtraction


def test_blob_lists_agree_with_the_recorded_text(gold):
    """The exact lists (from the reference's BlobDogD) are the ones the program printed: same length, same leading digits."""
    for name, spec in DC.BLOB_DETECT.items():
        for tag, fname in zip(("minima", "maxima"), spec["files"]):
            if fname is None:
                continue
            rows = gold[name + "/" + tag + "_exact"]
            text = [[float(t) for t in line.split()] for line in str(gold[name + "/" + fname]).splitlines()]
            assert len(text) == len(rows) > 0
            np.testing.assert_allclose(sorted(r[4] for r in text), sorted(rows[:, 4]), rtol=1e-5)


def test_statistics_are_serial_float_sums():
    """AverageArr / StdDevArr accumulate in float32 in raster order: on this image a float64 mean rounds differently."""
    rng = np.random.default_rng(5)
    a = (rng.random((12, 14, 16)) * 1000 + 1e4).astype(F)
    ave, sd = DN.average_stddev(a)
    assert ave.dtype == F and sd.dtype == F
    assert ave != F(a.astype(np.float64).mean()), "the case does not tell a serial float sum from an exact one"


# ---- the flags' argument errors (no GPU: they are raised before a context is created) --------------------------------------
def run(*args, cwd=None):
    return subprocess.run([CLI] + [str(a) for a in args], capture_output=True, text=True, cwd=cwd)


@pytest.mark.parametrize("flags,message", [
    (["-draw-spheres"], "must be followed by a file name"),
    (["-draw-spheres", "-background"], "must be followed by a file name"),
    (["-draw-hollow-spheres", ""], "must be followed by a file name"),
    (["-spheres", "l.txt", "-diameters"], "-diameters argument must be followed by a number"),
    (["-spheres", "l.txt", "-sphere-radii", "-3"], "-sphere-radii argument must be followed by a number"),
    (["-spheres", "l.txt", "-radii-voxels", "x"], "must be followed by a number"),
    (["-spheres", "l.txt", "-spheres-scale"], "ratio of the displyed sphere size"),
    (["-spheres", "l.txt", "-sphere-shell-ratio", "-1"], "ratio of the shell thickness"),
    (["-spheres", "l.txt", "-sphere-shell-thickness"], "must be followed by a number"),
    (["-spheres", "l.txt", "-spheres-shell-thickness-min", "-2"], "must be followed by a number"),
    (["-spheres", "l.txt", "-background"], "voxel intensity value outside the sphere"),
    (["-spheres", "l.txt", "-background-scale", "-1"], "usually between 0 and 1"),
    (["-spheres", "l.txt", "-foreground", "bright"], "voxel intensity value on the sphere"),
    (["-mask-rect", "1", "2", "3", "4", "5"], "must be followed by 6 numbers"),
    (["-mask-rectangle-subtract", "1", "2", "3", "4", "5", "x"], "must be followed by 6 numbers"),
    (["-mask-sphere", "1", "2", "3"], "must be followed by 4 numbers"),
    (["-mask-sphere-subtract", "1", "2", "", "4"], "must be followed by 4 numbers"),
    (["-random-spheres", "5", "10"], "-random-spheres is not provided"),
])
def test_draw_flag_errors(flags, message):
    r = run("-in", BLOB, *flags)
    assert r.returncode == 1 and message in r.stderr, r.stderr


@pytest.mark.parametrize("flags", [
    ["-draw-spheres", "l.txt"],
    ["-gauss", "20", "-mask-rect", "1", "9", "1", "9", "1", "9"],
    ["-gauss", "20", "-mask-sphere-subtract", "5", "5", "5", "3"],
    ["-blob", "minima", "b.txt", "160", "280", "1.05", "-out", "o.rec"],
])
def test_draw_flags_refuse_slab(flags, tmp_path):
    r = run("-in", BLOB, "-w", "19.6", *flags, "-slab", "0", "1", "-", cwd=str(tmp_path))
    assert r.returncode == 1 and "-slab does not draw" in r.stderr, r.stderr


def test_negative_background_and_foreground_are_numbers(tmp_path):
    """-background and -foreground take negative numbers (settings.cpp:2508, :2546): parsing goes on to the missing list."""
    r = run("-in", BLOB, "-draw-spheres", str(tmp_path / "missing.txt"), "-background", "-2", "-foreground", "-1.5",
            "-mask-crds-units", "voxels")
    assert r.returncode == 1 and "missing.txt" in r.stderr and "must be followed" not in r.stderr, r.stderr
