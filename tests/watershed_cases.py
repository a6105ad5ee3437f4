"""Test volumes and the list of cases recorded from the reference program for the watershed tests (numpy only).  The
volumes are those of extrema_cases; tests/golden/watershed.npz holds what the reference's filter_mrc wrote for every case
(tests/golden/make_golden_watershed.py)."""
import itertools

import numpy as np

import extrema_cases as EC

f32 = np.float32
INF = float("inf")


def no_nans(v):
    """special_volume keeps its +-0 and +-inf patches; its NaNs (which the watershed refuses) become 0.5."""
    v = v.copy()
    v[np.isnan(v)] = f32(0.5)
    return v


def golden_volumes():
    vols, masks = EC.golden_volumes()
    vols["special"] = no_nans(vols["special"])
    return vols, masks


# (threshold from minima, threshold from maxima): each sits exactly on a value of its volume where the volume has levels
THRESHOLDS = {
    "smooth": (0.5, -0.5), "quant": (4.0, 3.0), "special": (0.0, 0.0), "const": (2.5, 2.5), "binary": (0.0, 1.0),
    "ties": (0.0, 0.0), "thin": (4.0, 3.0),
}


def marker_volume(name, shape, mask):
    """Float marker images as the program reads them (it rounds them).  several: distinct labels, values that round, entries
    <= 0; repeated: one label at far-apart voxels and in a clump; masked: one label only on voxels with mask == 0, another on
    both sides."""
    rng = np.random.default_rng({"several": 31, "repeated": 32, "masked": 33}[name])
    m = np.zeros(shape, f32)
    flat = m.reshape(-1)
    pick = rng.choice(flat.size, 12, replace=False)
    if name == "several":
        flat[pick[:6]] = [3, 7.4, 2, 11, 4.6, 1]           # 7.4 -> 7, 4.6 -> 5
        flat[pick[6:9]] = [-2, 0.4, -0.6]                   # ignored
    elif name == "repeated":
        flat[pick[:6]] = [4, 4, 2, 4, 2, 9]
        z, y, x = [n // 2 for n in shape]
        m[z, y:y + 2, x:x + 2] = 6
    else:
        gone = np.nonzero(np.asarray(mask).reshape(-1) == 0)[0]
        kept = np.nonzero(np.asarray(mask).reshape(-1) != 0)[0]
        flat[rng.choice(gone, 3, replace=False)] = 8        # never a seed
        flat[rng.choice(gone, 2, replace=False)] = 5
        flat[rng.choice(kept, 2, replace=False)] = 5
        flat[rng.choice(kept, 3, replace=False)] = [1, 2, 12]
    return m


MARKERS = ("several", "repeated", "masked")


def golden_cases():
    """(volume, masked, kind, connectivity, show_boundaries, threshold, markers or None, boundary label, undefined-out):
    everything crossed on the quantised and the smooth volume, a selection on the others, the marker cases, and the two
    output flags."""
    cases = []
    for vol in ("quant", "smooth"):
        cases += [(vol,) + c + (None, 0, "max") for c in
                  itertools.product((False, True), ("min", "max"), (1, 2, 3), (True, False), (False, True))]
    for vol in ("special", "const", "binary", "ties", "thin"):
        cases += [(vol,) + c + (None, 0, "max") for c in itertools.product((False, True), ("min", "max"), (3, 1), (True,), (True,))]
        cases += [(vol, False, "min", 2, False, False, None, 0, "max"), (vol, True, "max", 2, True, False, None, 0, "max")]
    for mk in MARKERS:
        masked = mk == "masked"
        cases += [("quant", masked, "min", 1, True, False, mk, 0, "max"), ("quant", masked, "max", 3, True, True, mk, 0, "max"),
                  ("smooth", masked, "min", 3, False, True, mk, 0, "max"), ("smooth", True, "max", 2, True, False, mk, 0, "max")]
    cases += [("quant", False, "min", 3, True, True, None, 5, "max"), ("quant", True, "max", 1, True, True, None, 5, 7),
              ("smooth", True, "min", 2, True, True, None, 0, 7), ("quant", True, "min", 2, True, True, "several", 5, 7)]
    return cases


def case_name(case):
    vol, masked, kind, c, show, thr, mk, lb, und = case
    return "%s_%s_%s_c%d_%s_%s_%s_b%d_u%s" % (vol, "mask" if masked else "nomask", kind, c, "show" if show else "hide",
                                              "thr" if thr else "nothr", mk or "nomarkers", lb, und)


def case_arguments(case):
    """-> keyword arguments of a watershed call for a golden case (label_undefined stays -1, as the program calls it)."""
    vol, masked, kind, c, show, thr, mk, lb, und = case
    from_min = kind == "min"
    t = THRESHOLDS[vol][0 if from_min else 1] if thr else (INF if from_min else -INF)
    return dict(halt_threshold=t, start_from_minima=from_min, connectivity=c, show_boundaries=show, label_boundary=lb)


def rounded_markers(m):
    """std::round of the float marker image (no entry of marker_volume is a half)."""
    return np.floor(np.asarray(m, np.float64) + 0.5).astype(np.int32)
