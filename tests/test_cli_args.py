"""The argument errors of filter_mrc (visfd_amd/cli/settings.hpp), one command line per family of messages.

Every case must exit with status 1 and print, after the banner line, exactly the text recorded here.  The texts were
recorded from the program as it was before its parser was given one number reader (they include the reference's own
wording, typos and missing full stops included), so they pin the messages byte for byte.  All of them are decided before
any image is read: -in names a file that does not exist (the "Unable to open" cases say so)."""
import os
import subprocess

import pytest

from conftest import ROOT

CLI = os.path.join(ROOT, "visfd_amd", "cli", "filter_mrc")
IN = ["-in", "missing.rec"]

CASES = [
    # basic arguments
    ("w_no_number", IN + ["-w"],
     "Error: The -w argument needs 1 parameter(s).\n"),
    ("w_not_a_number", IN + ["-w", "x"],
     "Error: The -w argument must be followed by a number.\n"),
    ("bin_fraction", IN + ["-bin", "1.5"],
     "Error: The -bin argument must be followed by a positive integer.\n"),
    ("no_input", ["-gauss", "2"],
     "Error: You must specify an input file (-in).\n"),
    ("input_missing", IN + ["-gauss", "2"],
     "Error: Unable to open \"missing.rec\" for reading.\n"),
    ("unknown_flag", IN + ["-frobnicate", "3"],
     "Error: Unrecognized (or unsupported on the GPU hot path) argument: \"-frobnicate\"\n"),
    # morphology, extrema, watershed
    ("dilate_last", IN + ["-dilate"],
     "Error: The -dilate argument must be followed by a nonnegative number\n"),
    ("dilate_negative", IN + ["-dilate", "-3"],
     "Error: The -dilate argument must be followed by a nonnegative number\n"),
    ("dilate_binary_soft_two", IN + ["-dilate-binary-soft", "2", "3"],
     "Error: The -dilate-binary-soft argument must be followed by nonnegative numbers\n"),
    ("find_minima_last", IN + ["-find-minima"],
     "Error: The -find-minima argument must be followed by a number.\n"),
    ("connectivity_0", IN + ["-neighbor-connectivity", "0"],
     "Error: The -neighbor-connectivity argument must be followed by a positive integer.\n"),
    ("connectivity_4", IN + ["-neighbor-connectivity", "4"],
     "Error: The -neighbor-connectivity argument must be 1, 2 or 3 (6, 18 or 26 neighbors) in this program:\n"
     "       larger neighborhoods are not supported on the GPU.\n"),
    ("connectivity_x", IN + ["-neighbor-connectivity", "x"],
     "Error: The -neighbor-connectivity argument must be followed by a positive integer.\n"),
    ("watershed_foo", IN + ["-watershed", "foo"],
     "Error: The -watershed argument must be followed by an argument:  \"type\"  \"width\"\n"
     "       The \"type\" argument must be either \"minima\" or \"maxima\".\n"
     "       (It depends on whether you want to detect dark or bright objects.)\n"),
    ("watershed_threshold_last", IN + ["-watershed-threshold"],
     "Error: The -watershed-threshold argument must be followed by a number\n"),
    ("markers_last", IN + ["-markers"],
     "Error: The -markers argument must be followed by an image file name\n"),
    # filters
    ("ggauss_negative", IN + ["-ggauss", "-1"],
     "Error: The -ggauss argument must be followed by a positive number (\"s\"),\n"
     " the Gaussian width\n"),
    ("ggauss_aniso_two", IN + ["-ggauss-aniso", "1", "2"],
     "Error: The -ggauss-aniso argument must be followed by 3 positive numbers:\n"
     " s_x  s_y  s_z\n"
     " the Gaussian widths in the X, Y, and Z direction.)\n"),
    ("dogg_one", IN + ["-dogg", "1"],
     "Error: The -dogg argument must be followed by 2 positive numbers.\n"),
    ("exponents_one", IN + ["-exponents", "2"],
     "Error: The -exponents argument must be followed by two positive numbers.\n"),
    ("dog_aniso_five", IN + ["-dog-aniso", "1", "2", "3", "4", "5"],
     "Error: The -dog-aniso argument must be followed by 6 positive numbers.\n"),
    ("normalize_filters_yes", IN + ["-normalize-filters", "yes"],
     "Error: -normalize-filters accepts \"no\" only (as in the reference, settings.cpp:492-496).\n"),
    # blobs and spheres
    ("blob_bad_kind", IN + ["-blob", "some", "b", "10", "20", "1.1"],
     "Error: The 1st parameter to \"-blob\" must be \"minima\", \"maxima\" or \"all\".\n"),
    ("blob_min_ge_max", IN + ["-blob", "minima", "b", "20", "10", "1.1"],
     "Error: -blob needs 0 < min < max and a growth ratio > 1.\n"),
    ("discard_blobs_same", IN + ["-discard-blobs", "a", "a"],
     "Error: The -discard-blobs argument must be followed by two different file names\n"),
    ("draw_spheres_last", IN + ["-draw-spheres"],
     "Error: The -draw-spheres argument must be followed by a file name\n"),
    ("diameters_negative", IN + ["-diameters", "-3"],
     "Error: The -diameters argument must be followed by a number\n"),
    ("background_last", IN + ["-background"],
     "Error: The -background argument must be followed by a number:\n"
     "       the voxel intensity value outside the sphere (normally 0).\n"),
    ("random_spheres", IN + ["-random-spheres", "5"],
     "Error: -random-spheres is not provided by this program (it needs the reference's random numbers).\n"),
    ("mask_rect_five", IN + ["-mask-rect", "1", "2", "3", "4", "5"],
     "Error: The -mask-rect argument must be followed by 6 numbers.\n"),
    ("mask_sphere_three", IN + ["-mask-sphere", "1", "2", "3"],
     "Error: The -mask-sphere argument must be followed by 4 numbers.\n"),
    # membrane and clustering
    ("membrane_foo", IN + ["-membrane", "foo", "3"],
     "Error: The -membrane argument must be followed by \"minima\" or \"maxima\" and a width.\n"),
    ("tv_best_2", IN + ["-tv-best", "2"],
     "Error: -tv-best needs a number between 0 and 1.\n"),
    ("select_cluster_negative", IN + ["-select-cluster", "-1"],
     "Error: The -select-cluster argument must be followed by a positive integer.\n"),
    ("connect_without_membrane", IN + ["-connect", "1"],
     "Error: this build clusters voxels (-connect) only after \"-membrane ... -tv ...\".\n"),
    ("connect_angle_no_threshold", IN + ["-membrane", "minima", "3", "-tv", "5", "-connect-angle", "10"],
     "Error: clustering needs a saliency threshold (-connect THRESHOLD).\n"),
    ("normals_without_connect", IN + ["-normals-file", "f"],
     "Error: this build writes surface normals (-normals-file) for a clustered surface only (-connect).\n"),
    ("load_progress_without_tv", IN + ["-membrane", "minima", "3", "-load-progress", "b"],
     "Error: -connect and -load-progress need tensor voting (-tv).\n"),
    # -slab
    ("slab_rank_out_of_range", IN + ["-slab", "2", "2", "id"],
     "Error: -slab RANK WORLD IDFILE needs 0 <= RANK < WORLD.\n"),
    ("slab_draw_spheres", IN + ["-slab", "0", "1", "-", "-draw-spheres", "f"],
     "Error: -slab does not draw: -draw-spheres, the -mask-rect / -mask-sphere flags and \"-blob ... -out\"\n"
     "       need the whole image in one process.\n"),
    # accepted: a negative background gets past the parser, and the run fails on the input file instead
    ("background_negative_accepted", IN + ["-background", "-1"],
     "Error: Unable to open \"missing.rec\" for reading.\n"),
]


@pytest.fixture(scope="module")
def cli():
    if not os.path.exists(CLI):
        from visfd_amd import build
        build.build(verbose=False)
    return CLI


@pytest.mark.parametrize("name,args,message", CASES, ids=[c[0] for c in CASES])
def test_cli_argument_error(cli, tmp_path, name, args, message):
    r = subprocess.run([cli] + args, capture_output=True, text=True, cwd=tmp_path)
    banner, _, tail = r.stderr.partition("\n")
    assert banner.startswith("filter_mrc (")
    assert (r.returncode, r.stdout, tail) == (1, "", "\n" + message + "\n")
