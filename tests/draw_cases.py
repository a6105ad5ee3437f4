"""Inputs and case tables of the drawing tests (tests/test_draw.py, tests/test_draw_gpu.py, golden/make_golden_draw.py).
Everything is rebuilt from seeds; golden/draw.npz holds the reference program's outputs only."""
import numpy as np

import volgen

F = np.float32
RECT, SPHERE = 0, 1


def image(shape, seed):
    return volgen.noise_volume(shape, seed=seed, mean=3.0, sd=50.0)


def weighted_mask(shape, seed):
    """Zeros (a block and scattered voxels) and weights in (0, 2]: a weighted mask counts as "in" wherever it is not 0."""
    rng = np.random.default_rng(seed)
    nz, ny, nx = shape
    m = np.ones(shape, F)
    m[:, : max(1, ny // 4), :] = 0
    m[rng.random(shape) < 0.15] = 0
    return (m * (2.0 - 1.99 * rng.random(shape))).astype(F)


def spheres(shape, n, seed, dmax=9.0):
    """n spheres with distinct scores; centres inside, a few outside the image (negative and beyond the far corner)."""
    rng = np.random.default_rng(seed)
    nz, ny, nx = shape
    c = (rng.random((n, 3)) * np.array([nx, ny, nz]) * 1.3 - np.array([nx, ny, nz]) * 0.15).astype(F)
    d = (rng.random(n) * dmax).astype(F)
    th = (rng.random(n) * dmax * 0.6 - 0.5).astype(F)      # negative, thin, and thicker than the radius
    fg = (np.arange(1, n + 1) * 1.25 - n * 0.5).astype(F)  # distinct, both signs
    return c, d, th, fg


# ---- DrawSpheres through the C ABI: name -> keyword arguments of draw_np.draw_spheres / Context.draw_spheres, built lazily
def _order(reverse):
    c = np.array([[6.2, 7.9, 5.1], [8.0, 8.0, 6.0], [7.5, 6.1, 7.0]], F)
    d = np.array([9.0, 8.0, 7.0], F)
    fg = np.array([10.0, 20.0, 30.0], F)
    k = slice(None, None, -1) if reverse else slice(None)
    return dict(background=image((12, 14, 16), 1), centers=c[k], diameters=d[k], foreground=fg[k])


def _thickness_edges():
    # th = 0; th = d/2 exactly; th > d/2; d = 6 (r^2 = 9 on the boundary) with a shell of 1; d = -4 (a positive square)
    c = np.array([[4, 4, 4], [12, 5, 4], [5, 12, 5], [12, 12, 6], [8, 8, 10]], F)
    d = np.array([7.0, 5.0, 5.0, 6.0, -4.0], F)
    th = np.array([0.0, 2.5, 4.0, 1.0, 1.0], F)
    return dict(background=image((12, 18, 18), 2), centers=c, diameters=d, shell_thicknesses=th,
                foreground=np.array([1, 2, 3, 4, 5], F))


def _rand(shape, n, seed, **kw):
    c, d, th, fg = spheres(shape, n, seed)
    return dict(background=image(shape, seed + 1), centers=c, diameters=d, shell_thicknesses=th, foreground=fg, **kw)


def _far_cap():
    # r^2 above 2^24: the centre far outside, only the cap of the sphere inside a 16^3 image; the shell is 3 voxels thick
    return dict(background=image((16, 16, 16), 9), centers=np.array([[-5000.0, 8.0, 8.0]], F),
                diameters=np.array([10020.0], F), shell_thicknesses=np.array([3.0], F), foreground=np.array([7.0], F))


def _empty_shell():
    shape = (10, 12, 14)
    m = np.ones(shape, F)
    m[2:7, 3:8, 4:9] = 0          # sphere 0 lies wholly in the masked block: count 0, multiplier 1
    return dict(background=image(shape, 11), centers=np.array([[6, 5, 4], [10, 9, 7]], F), diameters=np.array([3.0, 5.0], F),
                foreground=np.array([8.0, 6.0], F), mask=m, foreground_normalize=True)


SPHERE_CASES = {
    "order_forward": lambda: _order(False),
    "order_reversed": lambda: _order(True),
    "thickness_edges": _thickness_edges,
    "null_arrays": lambda: dict(background=image((9, 10, 11), 3), centers=spheres((9, 10, 11), 6, 3)[0]),
    "null_thickness_fg": lambda: dict(background=image((9, 10, 11), 3), centers=spheres((9, 10, 11), 6, 3)[0],
                                      diameters=spheres((9, 10, 11), 6, 3)[1]),
    "shape_1x1x1": lambda: dict(background=image((1, 1, 1), 4), centers=np.array([[0.2, 0.9, -0.7]], F),
                                diameters=np.array([3.0], F), foreground=np.array([5.0], F)),
    "shape_nx1": lambda: _rand((7, 9, 1), 6, 5),
    "shape_5x7x70": lambda: _rand((5, 7, 70), 12, 6, mask=weighted_mask((5, 7, 70), 60)),
    "row_of_200": lambda: dict(background=image((3, 5, 200), 7), centers=np.array([[100.0, 2.0, 1.0], [30.0, 1.0, 2.0]], F),
                               diameters=np.array([150.0, 11.0], F), shell_thicknesses=np.array([2.0, 20.0], F),
                               foreground=np.array([2.0, 3.0], F)),
    "covers_image": lambda: dict(background=image((6, 7, 8), 8), centers=np.array([[4.0, 3.0, 3.0]], F),
                                 diameters=np.array([60.0], F), foreground=np.array([4.0], F)),
    "no_spheres": lambda: dict(background=image((6, 7, 8), 8), centers=np.zeros((0, 3), F), background_rescale=0.5,
                               background_offset=2.0),
    "many_writers": lambda: dict(background=image((24, 40, 70), 10), centers=spheres((24, 40, 70), 5000, 10)[0],
                                 diameters=(spheres((24, 40, 70), 5000, 10)[1] / 3).astype(F),
                                 foreground=spheres((24, 40, 70), 5000, 10)[3]),
    "far_cap": _far_cap,
    "rescale_offset": lambda: _rand((12, 14, 16), 8, 12, background_rescale=0.3, background_offset=0.1),
    "normalize_constant": lambda: dict(background=np.full((8, 9, 10), 2.5, F), centers=spheres((8, 9, 10), 5, 13)[0],
                                       diameters=spheres((8, 9, 10), 5, 13)[1], foreground=spheres((8, 9, 10), 5, 13)[3],
                                       background_normalize=True, background_offset=0.25),
    "normalize_plain": lambda: _rand((12, 14, 16), 8, 14, background_normalize=True, background_rescale=0.2),
    "normalize_weighted_mask": lambda: _rand((12, 14, 16), 8, 15, background_normalize=True, background_rescale=0.3,
                                             background_offset=-1.5, mask=weighted_mask((12, 14, 16), 61)),
    "foreground_normalize": lambda: _rand((12, 14, 16), 8, 16, foreground_normalize=True, mask=weighted_mask((12, 14, 16), 62)),
    "empty_shell": _empty_shell,
}

# refused inputs: name -> (keyword arguments, what is wrong)
REFUSED_SPHERES = {
    "nan_centre": dict(centers=np.array([[1.0, np.nan, 2.0]], F)),
    "inf_centre": dict(centers=np.array([[np.inf, 1.0, 2.0]], F)),
    "centre_beyond_int": dict(centers=np.array([[1.0, 2.0, 3.0e9]], F)),
    "nan_diameter": dict(centers=np.array([[1.0, 2.0, 3.0]], F), diameters=np.array([np.nan], F)),
    "huge_diameter": dict(centers=np.array([[1.0, 2.0, 3.0]], F), diameters=np.array([2.0 * 26755 + 1], F)),
}


# ---- DrawRegions: name -> (image, regions, mask, negative_means_subtract)
def _regions_image(zero=False, shape=(10, 12, 14), seed=20):
    return np.zeros(shape, F) if zero else np.abs(image(shape, seed)).astype(F) * (np.indices(shape).sum(0) % 3 > 0)


_SET_SUB_SET = [(RECT, (2, 9, 1, 8, 0, 6), 1.0), (SPHERE, (6.4, 5.2, 3.7, 3.3), -1.0), (RECT, (5.5, 11.49, 4, 6, 2, 3), 2.5),
                (SPHERE, (1.0, 1.0, 1.0, 2.0), 0.0), (RECT, (-5, 3.2, 9.5, 40, 7, 30), -2.0)]

REGION_CASES = {
    "set_subtract_set": lambda: (_regions_image(), _SET_SUB_SET, None, True),
    "negative_without_subtract": lambda: (_regions_image(), _SET_SUB_SET, None, False),
    "with_mask": lambda: (_regions_image(), _SET_SUB_SET, weighted_mask((10, 12, 14), 63), True),
    "inverted_rect": lambda: (_regions_image(), [(RECT, (8, 2, 1, 8, 0, 6), 3.0), (RECT, (1, 3, 8, 1, 0, 6), 3.0)], None, True),
    "rect_outside": lambda: (_regions_image(), [(RECT, (20, 30, 1, 8, 0, 6), 3.0), (RECT, (-9, -0.6, 1, 8, 0, 6), 3.0),
                                                (RECT, (-9, -0.5, 1, 8, 0, 6), 4.0)], None, True),
    "tiny_sphere": lambda: (_regions_image(), [(SPHERE, (4.2, 5.6, 6.49, 0.4), 9.0), (SPHERE, (40, 5, 6, 2.0), 9.0),
                                               (SPHERE, (13.0, 11.0, 9.0, 2.6), 5.0)], None, True),
    "nan_value": lambda: (_regions_image(), [(RECT, (2, 5, 2, 5, 2, 5), float("nan")), (SPHERE, (8, 8, 5, 2.2), -1.0)], None, True),
    "fill_with_ones": lambda: (_regions_image(zero=True), [(SPHERE, (6, 6, 5, 3.5), -1.0), (RECT, (0, 3, 0, 3, 0, 3), -1.0)],
                               None, True),
    "fill_with_ones_masked": lambda: (_regions_image(zero=True), [(SPHERE, (6, 6, 5, 3.5), -1.0)],
                                      weighted_mask((10, 12, 14), 64), True),
    "fill_hidden_nonzero": lambda: (_hidden(True), [(SPHERE, (6, 6, 5, 3.5), -1.0)], _hidden_mask(), True),
    "fill_visible_nonzero": lambda: (_hidden(False), [(SPHERE, (6, 6, 5, 3.5), -1.0)], _hidden_mask(), True),
    "no_regions": lambda: (_regions_image(), [], None, True),
    "several_blocks": lambda: (_regions_image(shape=(20, 30, 150), seed=21),
                               [(RECT, (3, 140, 2, 27, 1, 18), 1.0), (SPHERE, (75, 15, 10, 9.7), -1.0)], None, True),
}


def _hidden_mask():
    m = np.ones((10, 12, 14), F)
    m[0, 0, 0] = 0
    return m


def _hidden(hidden):
    """All zeros except one voxel: behind the mask (the fill still happens) or in front of it (it does not)."""
    a = np.zeros((10, 12, 14), F)
    a[(0, 0, 0) if hidden else (9, 11, 13)] = 5.0
    return a


# ---- through the command line: the cases of golden/draw.npz --------------------------------------------------------------
CLI_SHAPE = (12, 14, 16)
# x y z diameter score, in voxels: distinct scores, overlapping spheres, a negative coordinate, a centre beyond the far
# corner whose sphere still reaches the image, a diameter of 0
ROWS = [(4, 5, 6, 7, 1.5), (6.4, 6, 7, 6, -2.25), (-1, 3, 4, 5, 3.5), (17, 14, 12, 8, 0.75), (9, 8, 3, 0, 4.25),
        (11, 4, 9, 5.5, -0.5), (8, 9, 6, 4, 2.0)]
IN_IMAGE_CENTRES = 5
BIG = [(6, 7, 8, 100, 1)]           # one sphere larger than the image: with -background 0 -foreground 1 it prints the mask
W_PHYS = 19.6


def rows_text(rows, w=1.0):
    return "".join(" ".join(repr(float(np.float32(x) * (np.float32(w) if k < 4 else 1))) for k, x in enumerate(r)) + "\n"
                   for r in rows)


def rows_of_text(text):
    return [tuple(float(t) for t in line.split()) for line in text.splitlines() if line.strip()]


_M = {"mask-rect": [(RECT, (2, 11, 3.4, 9.6, 1, 8), 1.0)],
      "mask-sphere-minus-rect": [(SPHERE, (7.3, 6.8, 5.5, 5.2), 1.0), (RECT, (6, 9, 0, 20, 4, 6), -1.0)],
      "mask-subtract-first": [(RECT, (3, 8, 2, 30, -4, 5), -1.0), (SPHERE, (12, 10, 9, 3.7), -1.0),
                              (SPHERE, (5, 5, 3, 1.6), 1.0)]}


def _region_flags(regions):
    out = []
    for t, c, v in regions:
        out += [("-mask-rect" if t == RECT else "-mask-sphere") + ("-subtract" if v < 0 else "")] + [repr(float(x)) for x in c]
    return out


# name -> dict(image: "seeded" | "membrane" | "blob", w, rows (None: no list file), mask: None | "block" | "blobmask",
#              args: the flags after "-in IN -w W -out OUT" ("LIST" stands for the list file), opts: what they mean to
#              draw_np.handle_draw_spheres, regions: the mask regions)
CLI_CASES = {
    "plain": dict(args=["-draw-spheres", "LIST"], opts={}),
    "bg0_fg1": dict(args=["-spheres", "LIST", "-background", "0", "-foreground", "1"],
                    opts=dict(background=0.0, background_scale=0.0, use_score=False, foreground=1.0)),
    "bg0_fg1_radii0": dict(args=["-draw-spheres", "LIST", "-background", "0", "-foreground", "1", "-sphere-radii", "0"],
                           opts=dict(background=0.0, background_scale=0.0, use_score=False, foreground=1.0, diameter=0.0)),
    "hollow_auto": dict(args=["-draw-hollow-spheres", "LIST", "-background-auto", "-background-scale", "0.2"],
                        opts=dict(thickness=0.05, background_norm=True, background_scale=0.2)),
    "mask_normalize": dict(mask="block", args=["-draw-spheres", "LIST", "-spheres-normalize"], opts=dict(foreground_norm=True)),
    "shell_ratio_scale": dict(image="membrane", args=["-draw-spheres", "LIST", "-spheres-shell-ratio", "0.3", "-spheres-scale", "1.5"],
                              opts=dict(thickness=0.3, scale=1.5)),
    "shell_thickness_score": dict(args=["-draw-spheres", "LIST", "-foreground", "3", "-sphere-shell-thickness", "1", "-spheres-score"],
                                  opts=dict(thickness=1.0, thickness_is_ratio=False, foreground=3.0)),
    "physical_units": dict(w=W_PHYS, args=["-draw-spheres", "LIST", "-sphere-shell-thickness", "25", "-background-scale", "0.5",
                                           "-background", "-7.5"],
                           opts=dict(thickness=25.0, thickness_is_ratio=False, background=-7.5, background_scale=0.0)),
    "physical_diameters": dict(w=W_PHYS, args=["-draw-spheres", "LIST", "-diameters", "70", "-background-scale", "0.5"],
                               opts=dict(diameter=70.0, background_scale=0.5)),
    "diameters_voxels": dict(w=W_PHYS, args=["-draw-spheres", "LIST", "-radii-voxels", "2.3"],
                             opts=dict(diameter=4.6, diameter_in_voxels=True)),
    "mask_rect": dict(rows=BIG, regions=_M["mask-rect"], args=["-draw-spheres", "LIST", "-background", "0", "-foreground", "1"]
                      + _region_flags(_M["mask-rect"]), opts=dict(background_scale=0.0, use_score=False)),
    "mask_sphere_minus_rect": dict(rows=BIG, regions=_M["mask-sphere-minus-rect"],
                                   args=["-draw-spheres", "LIST", "-background", "0", "-foreground", "1"]
                                   + _region_flags(_M["mask-sphere-minus-rect"]), opts=dict(background_scale=0.0, use_score=False)),
    "mask_subtract_first": dict(rows=BIG, regions=_M["mask-subtract-first"],
                                args=["-draw-spheres", "LIST", "-background", "0", "-foreground", "1", "-mask-crds-units", "voxels"]
                                + _region_flags(_M["mask-subtract-first"]), opts=dict(background_scale=0.0, use_score=False)),
    # the blob detector's picture; its list files are recorded too (the picture is drawn from them)
    "blob_minima_out": dict(image="blob", mask="blobmask", rows=None, w=W_PHYS,
                            args=["-blob", "minima", "BLOBS", "160", "280", "1.01"], opts={}),
    "blob_all_out": dict(image="blob", mask="blobmask", rows=None, w=W_PHYS,
                         args=["-blob", "all", "BLOBS", "160", "280", "1.02",
                               "-spheres-shell-ratio", "0.1"], opts=dict(thickness=0.1)),
    # extrema thinned by a diameter and a separation ratio: the list file is what changes
    "maxima_thinned": dict(image="blob", rows=None, w=1.0,
                           args=["-find-maxima", "EXTREMA", "-diameters", "6", "-radial-separation", "0.9"], opts={}),
}


LIST_FILES = {"LIST": "list.txt", "BLOBS": "blobs", "EXTREMA": "extrema.txt"}
# the text files a run writes besides its image, recorded with it
WRITTEN = {"blob_minima_out": ["blobs"], "blob_all_out": ["blobs.minima.txt", "blobs.maxima.txt"], "maxima_thinned": ["extrema.txt"]}


# the detector's own arguments behind the two blob cases (settings.cpp:1648-1764: "minima" sets the minima threshold to 0 and
# leaves the maxima threshold at -infinity, so every maximum is found -- and drawn, though no file lists it)
BLOB_DETECT = {"blob_minima_out": dict(ladder=(160.0, 280.0, 1.01), minima_threshold=0.0, maxima_threshold=-np.inf,
                                       files=("blobs", None)),
               "blob_all_out": dict(ladder=(160.0, 280.0, 1.02), minima_threshold=np.inf, maxima_threshold=-np.inf,
                                    files=("blobs.minima.txt", "blobs.maxima.txt"))}


def cli_command(name, program, workdir):
    """Writes the inputs of a case into workdir and returns the command line (output: out.rec, and the files of WRITTEN)."""
    import os
    img, mask, text, w = cli_inputs(name)
    volgen.write_mrc(os.path.join(workdir, "in.rec"), img, voxel_width=w)
    args = [program, "-in", "in.rec", "-w", repr(float(w)), "-out", "out.rec"]
    if mask is not None:
        volgen.write_mrc(os.path.join(workdir, "mask.rec"), mask, voxel_width=w)
        args += ["-mask", "mask.rec"]
    if text is not None:
        with open(os.path.join(workdir, "list.txt"), "w") as f:
            f.write(text)
    for f in ["out.rec"] + WRITTEN.get(name, []):
        if os.path.exists(os.path.join(workdir, f)):
            os.remove(os.path.join(workdir, f))
    return args + [LIST_FILES.get(a, a) for a in CLI_CASES[name]["args"]]


def cli_inputs(name):
    """-> (image, mask or None, list text or None, voxel width)"""
    import os
    case = CLI_CASES[name]
    kind = case.get("image", "seeded")
    golden = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
    if kind == "seeded":
        img = volgen.noise_volume(CLI_SHAPE, seed=700)
    elif kind == "membrane":
        img = volgen.read_mrc(os.path.join(golden, "test_image_membrane.rec"))
    else:
        img = volgen.read_mrc(os.path.join(golden, "test_blob_detect.rec"))
    img = np.ascontiguousarray(img, F)
    mask = None
    if case.get("mask") == "block":
        mask = volgen.block_mask(img.shape, seed=750)
    elif case.get("mask") == "blobmask":
        mask = np.ascontiguousarray(volgen.read_mrc(os.path.join(golden, "test_blob_detect_mask.rec")), F)
    w = case.get("w", 1.0)
    rows = case.get("rows", ROWS)
    return img, mask, None if rows is None else rows_text(rows, w), w
