"""Test volumes for the extrema tests (numpy only), and the list of cases recorded from the reference program in
tests/golden/extrema.npz (tests/golden/make_golden_extrema.py)."""
import itertools

import numpy as np

f32 = np.float32
INF = float("inf")


def _blur(v, passes):
    """[1 2 1] / 4 along every axis, edges replicated, `passes` times."""
    v = v.astype(np.float64)
    for _ in range(passes):
        for ax in range(3):
            p = np.concatenate([np.take(v, [0], ax), v, np.take(v, [-1], ax)], ax)
            n = v.shape[ax]
            v = (np.take(p, range(0, n), ax) + 2 * np.take(p, range(1, n + 1), ax) + np.take(p, range(2, n + 2), ax)) / 4
    return v


def smooth_noise(shape, seed, passes=2):
    """Blurred Gaussian noise, unit variance: extrema every few voxels, hardly any equal neighbours."""
    v = _blur(np.random.default_rng(seed).standard_normal(shape), passes)
    return ((v - v.mean()) / v.std()).astype(f32)


def quantised_noise(shape, seed, levels=8, passes=2):
    """The same noise rounded to `levels` values 0 .. levels - 1: plateaus of every size that touch each other."""
    v = smooth_noise(shape, seed, passes).astype(np.float64)
    q = np.floor((v - v.min()) / (v.max() - v.min()) * (levels - 1e-9))
    return np.clip(q, 0, levels - 1).astype(f32)


def random_mask(shape, seed, keep=0.8):
    """A block of zeros at one corner plus single voxels knocked out at random (walls, pockets, lone survivors)."""
    rng = np.random.default_rng(seed)
    m = (rng.random(shape) < keep).astype(f32)
    m[: max(1, shape[0] // 4), : max(1, shape[1] // 3), :] = 0
    m[m != 0] = rng.choice(np.array([1.0, 0.5, -2.0], f32), int((m != 0).sum()))   # any non-zero value means "exists"
    return m


def binary_volume(shape, seed):
    """Two values, each forming large plateaus."""
    return (smooth_noise(shape, seed, passes=3) > 0).astype(f32)


def serpentine(shape, flaw=False):
    """A one-voxel-wide path of value 5 that winds through the whole volume (background 0): along x in every second row of
    every second plane, with one-voxel links at alternating ends.  With c = 1 it is one plateau of about nx*ny*nz/4 voxels,
    a maximum.  flaw: the background voxel next to the path's far end is 7, which disqualifies the whole plateau."""
    nz, ny, nx = shape
    v = np.zeros(shape, f32)
    end = None
    right = True      # the side on which the current row ends
    for zi, z in enumerate(range(0, nz, 2)):
        rows = list(range(0, ny, 2))
        if zi % 2:
            rows.reverse()
        for k, y in enumerate(rows):
            v[z, y, :] = 5
            x_end = nx - 1 if right else 0
            end = (z, y, x_end)
            if k + 1 < len(rows):
                v[z, (y + rows[k + 1]) // 2, x_end] = 5      # link to the next row of this plane
            elif z + 2 < nz:
                v[z + 1, y, x_end] = 5                        # link to the next plane
            right = not right
    if flaw:
        z, y, x = end
        spot = [(z, y + 1, x), (z, y - 1, x), (z + 1, y, x), (z - 1, y, x)]
        for p in spot:
            if all(0 <= p[d] < shape[d] for d in range(3)) and v[p] == 0:
                v[p] = 7
                break
        else:
            raise AssertionError("no background voxel next to the path's end")
    return v


def special_volume(shape, seed):
    """Quantised noise with patches of +0 next to -0, NaN voxels (single and adjacent) and +-inf voxels."""
    rng = np.random.default_rng(seed)
    v = quantised_noise(shape, seed, levels=5) - f32(2.0)          # -2 .. 2, so that 0 is a level
    zero = v == 0
    v[zero & (rng.random(shape) < 0.5)] = f32(-0.0)
    flat = v.reshape(-1)
    pick = rng.choice(flat.size, size=min(40, flat.size // 8), replace=False)
    flat[pick[0::4]] = np.nan
    flat[pick[1::4]] = np.inf
    flat[pick[2::4]] = -np.inf
    flat[(pick[3::4] + 1) % flat.size] = np.nan                   # some next to one another along x
    flat[pick[3::4]] = np.nan
    return v


def walled_volume(shape, seed):
    """-> (src, mask): smooth noise in which several voxels are walled in by the mask (all 26 neighbours masked out)."""
    rng = np.random.default_rng(seed)
    src = smooth_noise(shape, seed)
    mask = np.ones(shape, f32)
    for _ in range(6):
        z, y, x = [int(rng.integers(1, n - 1)) if n > 2 else 0 for n in shape]
        mask[max(z - 1, 0):z + 2, max(y - 1, 0):y + 2, max(x - 1, 0):x + 2] = 0
        mask[z, y, x] = 1
    return src, mask


def tie_volume(shape):
    """Separate plateaus that share one score: peaks of 3 (single voxels and pairs) and pits of -3 on a background of 0."""
    v = np.zeros(shape, f32)
    nz, ny, nx = shape
    k = 0
    for z in range(1, nz - 1, 3):
        for y in range(1, ny - 1, 3):
            for x in range(1, nx - 2, 4):
                val = f32(3.0 if k % 2 else -3.0)
                v[z, y, x] = val
                if k % 3 == 0:
                    v[z, y, x + 1] = val
                k += 1
    return v


# ---- the cases recorded from the reference program ------------------------------------------------------------------
def golden_volumes():
    vols = {
        "smooth": smooth_noise((17, 23, 19), 11),
        "quant": quantised_noise((16, 20, 24), 12),
        "special": special_volume((10, 11, 12), 13),
        "const": np.full((4, 5, 6), 2.5, f32),
        "binary": binary_volume((9, 10, 11), 14),
        "ties": tie_volume((8, 8, 11)),
        "thin": quantised_noise((13, 9, 1), 15),
    }
    masks = {k: random_mask(v.shape, 100 + i) for i, (k, v) in enumerate(sorted(vols.items()))}
    return vols, masks


THRESHOLDS = {   # (minima_threshold, maxima_threshold): some extrema fail them, some sit exactly on them
    "smooth": (-0.5, 0.5), "quant": (1.0, 5.0), "special": (0.0, 0.0), "const": (2.5, 2.5), "binary": (0.0, 1.0),
    "ties": (-3.0, 3.0), "thin": (2.0, 4.0),
}
KINDS = {"min": (True, False), "max": (False, True), "both": (True, True)}


def golden_cases():
    """(volume, masked, kind, connectivity, allow_borders, thresholds or None): everything crossed on the quantised and the
    smooth volume, and a selection on the others."""
    cases = []
    for vol in ("quant", "smooth"):
        cases += [(vol,) + c for c in itertools.product((False, True), ("min", "max", "both"), (1, 2, 3), (True, False),
                                                        (False, True))]
    for vol in ("special", "const", "binary", "ties", "thin"):
        cases += [(vol,) + c for c in itertools.product((False, True), ("min", "max", "both"), (3, 1), (True, False),
                                                        (True,))]
        cases += [(vol, False, "both", 2, True, False)]
    return cases


def case_name(case):
    vol, masked, kind, c, borders, thr = case
    return "%s_%s_%s_c%d_%s_%s" % (vol, "mask" if masked else "nomask", kind, c, "borders" if borders else "noborders",
                                   "thr" if thr else "nothr")


def case_arguments(case):
    """-> keyword arguments of find_extrema for a golden case (thresholds as the filter_mrc flags would set them)."""
    vol, masked, kind, c, borders, thr = case
    lo, hi = THRESHOLDS[vol] if thr else (INF, -INF)
    fmin, fmax = KINDS[kind]
    return dict(find_minima=fmin, find_maxima=fmax, minima_threshold=lo, maxima_threshold=hi, connectivity=c,
                allow_borders=borders)
