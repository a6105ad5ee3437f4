"""The inputs and the command lines of the intensity-map tests (tests/test_intensity.py, tests/test_intensity_gpu.py) and of
the recorder of their goldens (tests/golden/make_golden_intensity.py)."""
import os

import numpy as np

import volgen

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SHAPE = (11, 9, 7)   # nz, ny, nx: a 7 x 9 x 11 volume


def dyadic_volume(seed=7911):
    """Multiples of 1/8 in +-250 (a few zeros of both signs among them) and a mask with about 70 % ones."""
    rng = np.random.default_rng(seed)
    v = (rng.integers(-2000, 2001, SHAPE).astype(np.float32) / np.float32(8.0)).astype(np.float32)
    v[0, 0, :3] = 0.0
    v[0, 1, :3] = -0.0
    mask = (rng.random(SHAPE) < 0.7).astype(np.float32)
    return v, mask


def select_mask(seed=7912):
    """A mask of labels 0..3 for -mask-select."""
    return np.random.default_rng(seed).integers(0, 4, SHAPE).astype(np.float32)


def wide_volume(seed=7913):
    """Magnitudes from 2^-30 to 2^30 with full mantissas: no 2^q divides them all with the sum of magnitudes below
    2^(q + 53), so the order-freedom proof fails."""
    rng = np.random.default_rng(seed)
    e = rng.integers(-30, 31, SHAPE)
    m = rng.uniform(1.0, 2.0, SHAPE)
    s = rng.choice([-1.0, 1.0], SHAPE)
    return (s * m * np.exp2(e)).astype(np.float32)


def inputs():
    """name -> (volume, mask or None)"""
    dy, dm = dyadic_volume()
    return {
        "blob": (volgen.read_mrc(os.path.join(GOLDEN, "test_blob_detect.rec")),
                 volgen.read_mrc(os.path.join(GOLDEN, "test_blob_detect_mask.rec"))),
        "membrane": (volgen.read_mrc(os.path.join(GOLDEN, "test_image_membrane.rec")), None),
        "dyadic": (dy, dm),
        "dyadic_sel": (dy, select_mask()),
        "wide": (wide_volume(), None),
    }


# (case name, input name, uses the mask, flags).  Every flag alone, reversed (a > b), with -thresh-range, with -mask, with
# -mask-select, after -gauss, and -invert combined with -rescale and with -thresh2.
CASES = [
    ("thresh", "dyadic", False, ["-thresh", "10.5"]),
    ("thresh_out", "dyadic", False, ["-thresh-out", "-3"]),
    ("thresh_range", "dyadic", False, ["-thresh", "10.5", "-thresh-range", "3", "-2.5"]),
    ("thresh2", "dyadic", False, ["-thresh2", "-100", "150.25"]),
    ("thresh2_rev", "dyadic", False, ["-thresh2", "150.25", "-100"]),
    ("thresh2_range", "dyadic", False, ["-thresh2", "-100", "150.25", "-thresh-range", "3", "-2.5"]),
    ("thresh2_rev_range", "dyadic", False, ["-thresh2-out", "150.25", "-100", "-thresh-range-out", "-1", "7"]),
    ("thresh2_equal", "dyadic", False, ["-thresh2", "20", "20", "-thresh-range", "5", "6"]),
    ("thresh4", "dyadic", False, ["-thresh4", "-200", "-100", "50", "175.5"]),
    ("thresh4_rev", "dyadic", False, ["-thresh4", "175.5", "50", "-100", "-200"]),
    ("thresh4_range", "dyadic", False, ["-thresh4-out", "-200", "-100", "50", "175.5", "-thresh-range", "2", "10"]),
    ("thresh4_degenerate", "dyadic", False, ["-thresh4", "-200", "50", "50", "50", "-thresh-range", "2", "10"]),
    ("thresh_interval", "dyadic", False, ["-thresh-interval", "-50", "80"]),
    ("thresh_interval_rev", "dyadic", False, ["-thresh-interval-out", "80", "-50", "-thresh-range", "4", "1"]),
    ("thresh_gauss", "dyadic", False, ["-thresh-gauss", "20", "75"]),
    ("thresh_gauss_range", "dyadic", False, ["-thresh-gauss-out", "-40", "30", "-thresh-range", "3", "-2.5"]),
    ("clip", "dyadic", False, ["-clip", "-100.125", "75.5"]),
    ("clip_rev", "dyadic", False, ["-clip", "75.5", "-100.125"]),
    ("cl", "dyadic", False, ["-cl", "-1", "1.5"]),
    ("cl_rev", "dyadic", False, ["-cl", "1.5", "-1"]),
    ("rescale", "dyadic", False, ["-rescale", "0.3", "-7.25"]),
    ("fill", "dyadic", False, ["-fill", "2.5"]),
    ("rescale_min_max", "dyadic", False, ["-rescale-min-max", "0", "1"]),
    ("rescale_min_max_rev", "dyadic", False, ["-rescale-min-max", "-3", "10"]),
    ("no_rescale", "dyadic", False, ["-rescale-min-max", "0", "1", "-no-rescale"]),
    ("invert", "dyadic", False, ["-invert"]),
    ("inv_rescale", "dyadic", False, ["-inv", "-rescale", "0.3", "-7.25"]),
    ("invert_thresh2", "dyadic", False, ["-invert", "-thresh2", "-100", "150.25"]),
    ("invert_rescale_min_max", "dyadic", False, ["-invert", "-rescale-min-max", "1", "0"]),
    # with -mask (voxels outside it take the -mask-out value, before -rescale-min-max)
    ("mask_thresh2", "dyadic", True, ["-thresh2", "-100", "150.25"]),
    ("mask_clip", "dyadic", True, ["-clip", "-100.125", "75.5", "-mask-out", "-9"]),
    ("mask_cl", "dyadic", True, ["-cl", "-1", "1.5"]),
    ("mask_invert", "dyadic", True, ["-invert"]),
    ("mask_invert_rescale", "dyadic", True, ["-invert", "-rescale", "2", "1", "-mask-out", "5"]),
    ("mask_rescale_min_max", "dyadic", True, ["-rescale-min-max", "0", "1", "-mask-out", "300"]),
    ("mask_thresh_gauss", "dyadic", True, ["-thresh-gauss", "20", "75"]),
    ("mask_select_invert", "dyadic_sel", True, ["-mask-select", "2", "-invert"]),
    ("mask_select_cl", "dyadic_sel", True, ["-mask-select", "3", "-cl", "-0.5", "0.5"]),
    ("mask_select_rescale_min_max", "dyadic_sel", True, ["-mask-select", "1", "-rescale-min-max", "2", "-2"]),
    # after a filter: the threshold family reads the INPUT image, the rest the filter's output
    ("gauss_thresh2", "dyadic", False, ["-gauss", "2", "-thresh2", "-100", "150.25"]),
    ("gauss_rescale", "dyadic", False, ["-gauss", "2", "-rescale", "0.3", "-7.25"]),
    ("gauss_invert", "dyadic", False, ["-gauss", "2", "-invert"]),
    ("gauss_rescale_min_max", "dyadic", True, ["-gauss", "2", "-rescale-min-max", "0", "1"]),
    # the fixtures (integer-valued) and the wide-range volume
    ("blob_invert", "blob", False, ["-invert"]),
    ("blob_mask_invert", "blob", True, ["-invert"]),
    ("blob_gauss_cl", "blob", False, ["-gauss", "120", "-cl", "-1", "1.5"]),
    ("blob_mask_rescale_min_max", "blob", True, ["-rescale-min-max", "0", "1"]),
    ("blob_thresh_interval", "blob", False, ["-thresh-interval", "30", "40"]),
    ("membrane_invert", "membrane", False, ["-invert"]),
    ("membrane_clip", "membrane", False, ["-clip", "-500", "500"]),
    ("membrane_thresh_gauss", "membrane", False, ["-thresh-gauss", "0", "400"]),
    ("wide_invert", "wide", False, ["-invert"]),
    ("wide_thresh2", "wide", False, ["-thresh2", "-1", "1000"]),
    ("wide_rescale_min_max", "wide", False, ["-rescale-min-max", "0", "1"]),
]
GAUSS_ULP_CASES = {c[0] for c in CASES if any(f.startswith("-thresh-gauss") for f in c[3])}


def voxel_width(input_name):
    """-w of a case: 1, but the blob fixture's command line is the documented one (its sigma of 120 is in physical units)."""
    return 40.0 if input_name == "blob" else 1.0


def command(case, exe, in_path, mask_path, out_path):
    name, input_name, use_mask, flags = case
    args = [exe, "-in", in_path, "-w", repr(voxel_width(input_name)), "-out", out_path]
    if use_mask:
        args += ["-mask", mask_path]
    return args + list(flags)


# the stats cases: name -> values (float32, 1-D)
def stats_inputs():
    dy, _ = dyadic_volume()
    f = np.float32
    den = np.array([1e-45, 3e-45, -1e-45, 1.1754942e-38, -5.9e-39, 2.5e-40], f)   # subnormals
    every = np.concatenate([np.exp2(np.arange(-149, 128)).astype(f), -np.exp2(np.arange(-149, 128, 3)).astype(f)])
    return {
        "cancel": np.array([2.0 ** 120, 1.0, -2.0 ** 120], f),
        "cancel_wide": np.array([2.0 ** 120, 1.5, -2.0 ** 120, 2.0 ** -100, 3.0, -2.0 ** 60, 2.0 ** 60], f),
        "denormal": den,
        "zeros": np.array([0.0, -0.0, -0.0, 0.0], f),
        "every_exponent": every,
        "one": np.array([-3.75], f),
        "dyadic": dy.reshape(-1),
        "wide": wide_volume().reshape(-1),
        "above_tie": np.array([2.0 ** 53, 1.0, 2.0 ** 53, 1.0, 1.0], f),   # 2^54 + 3: rounds up
        "tie": np.array([2.0 ** 53, 1.0, 2.0 ** 53, 1.0], f),               # 2^54 + 2: a tie, to even
        "tie_odd": np.array([2.0 ** 53, 2.0 ** 53, 4.0, 1.0, 1.0], f),       # 2^54 + 6: a tie, up to even
    }


# One pass of visfd_hip_intensity_map: name -> the keyword arguments of intensity_np.apply (visfd_amd.api.intensity takes
# the same under the names of its own signature, see map_params).  Every map kind, reversed thresholds, and the stages
# around the map.
MAP_CASES = {
    "step": dict(map=1, t=(10.5,), out_a=3.0, out_b=-2.5),
    "thresh2": dict(map=2, t=(-100.0, 150.25)),
    "thresh2_rev": dict(map=2, t=(150.25, -100.0), out_a=3.0, out_b=-2.5),
    "clip": dict(map=2, t=(-100.125, 75.5), out_a=-100.125, out_b=75.5),
    "thresh4": dict(map=3, t=(-200.0, -100.0, 50.0, 175.5), out_a=2.0, out_b=10.0),
    "thresh4_rev": dict(map=3, t=(175.5, 50.0, -100.0, -200.0)),
    "thresh4_degenerate": dict(map=3, t=(-200.0, 50.0, 50.0, 50.0), out_a=2.0, out_b=10.0),
    "interval": dict(map=3, t=(-50.0, -50.0, 80.0, 80.0)),
    "range": dict(map=4, t=(-50.0, 80.0)),
    "range_rev": dict(map=4, t=(80.0, -50.0)),
    "gauss": dict(map=5, t=(20.0, 75.0), out_a=3.0, out_b=-2.5),
    "rescale": dict(map=6, t=(0.3, -7.25)),
    "fill": dict(map=6, t=(0.0, 2.5)),
    "invert": dict(invert_ave=-12.617784992784993),
    "invert_rescale_fill": dict(map=6, t=(2.0, 1.0), invert_ave=3.3, masked_value=5.0),
    "invert_thresh2": dict(map=2, t=(-100.0, 150.25), invert_ave=3.3),
    "mask_fill": dict(masked_value=-9.0),
    "rescale01": dict(rescale01_args=(-249.25, 248.125, 1.0, -3.0)),
    "everything": dict(map=6, t=(0.3, -7.25), invert_ave=3.3, masked_value=300.0, rescale01_args=(-80.0, 300.0, 0.0, 1.0)),
}
MAP_GAUSS_CASES = {"gauss"}


def map_params(api, kw, stats_mask=False):
    """the visfd_hip_intensity of a MAP_CASES entry"""
    return api.intensity(map=kw.get("map", 0), t=kw.get("t", ()), out_a=kw.get("out_a", 0.0), out_b=kw.get("out_b", 1.0),
                         invert_ave=kw.get("invert_ave"), masked_value=kw.get("masked_value"),
                         rescale01=kw.get("rescale01_args"), stats_mask=stats_mask)


def map_volume(shape, seed=7920):
    """(src, out, mask) for a map pass: multiples of 1/8 in +-250 with the thresholds of MAP_CASES among them, a second
    image of the same kind, and a mask with about 70 % ones (at least one)."""
    rng = np.random.default_rng(seed + int(np.prod(shape)))
    src = (rng.integers(-2000, 2001, shape).astype(np.float32) / np.float32(8.0)).astype(np.float32)
    special = np.array([10.5, -100.0, 150.25, 50.0, 175.5, -200.0, 80.0, -50.0, 0.0, -0.0, 75.5, -100.125], np.float32)
    flat = src.reshape(-1)
    k = min(flat.size, special.size)
    flat[rng.permutation(flat.size)[:k]] = special[:k]
    out = (rng.integers(-2000, 2001, shape).astype(np.float32) / np.float32(8.0)).astype(np.float32)
    mask = (rng.random(shape) < 0.7).astype(np.float32)
    mask.reshape(-1)[0] = 1.0
    return src, out, mask
