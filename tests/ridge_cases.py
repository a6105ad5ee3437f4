"""Inputs for the ridge stage (csrc/ridge.hip, csrc/eigen3.hpp), numpy only: the volumes whose rows are longer than one
workgroup or whose axes are 3 wide, the survivor patterns and score values of the direction kernel's compaction, the
matrices of the eigen solver and the tensors of the post-vote score.  tests/test_ridge.py shows on the CPU that the checkers
of ridge_np.py discriminate on exactly these inputs; tests/test_ridge_gpu.py runs the kernels on them.

The CPU restatement's results on these inputs (`reference`, `saliency_reference`, `score_tensors`) take the oracle as an
argument and are computed once per process."""
import numpy as np

import volgen

f32 = np.float32

# [nz, ny, nx].  voxel_of_block (ridge.hip) splits a row into blocks of 256 threads; a direction workgroup scans P voxels.
SHAPES = [
    (3, 3, 3),       # 27: smaller than one chunk; every voxel clamps to the same centre
    (3, 4, 300),     # 3600: nx past 256
    (5, 3, 513),     # 7695: three x blocks, the last holding one voxel
    (4, 257, 3),     # 3084: a 3-wide x axis
    (3, 5, 273),     # 4095: one voxel short of a chunk
    (4, 8, 128),     # 4096: exactly one chunk
    (8, 8, 128),     # 8192: exactly two chunks
    (3, 7, 391),     # 8211: two chunks plus 19 voxels
    volgen.MEM_SHAPE,   # 11440: the shape of the membrane goldens
]
HESSIAN_GPU_SHAPES = [(3, 3, 3), (3, 4, 300), (5, 3, 513), (4, 257, 3), (3, 7, 391)]
COMPACTION_SHAPES = [(3, 3, 3), (3, 5, 273), (4, 8, 128), (8, 8, 128), (3, 7, 391)]
COMPACTION_BOTH_ORDERS = (3, 7, 391)      # the others run the decreasing order only
TOO_THIN = [(2, 5, 5), (5, 2, 5), (5, 5, 2)]

SIGMAS = (1.0, 1.732)     # Gaussian half-widths 2 and 4 at the ratio below
SIGMA = 1.0               # the width of the saliency, direction and compaction cases
THRESHOLD = 0.03          # the CLI's default truncation threshold -> ratio_from_threshold
SENTINEL = f32(-6.0221e23)   # what output buffers hold before a call; no kernel here computes it

P = 4096                  # voxels per workgroup of ridge_directions_kernel: DIR_PER * BLOCK = 16 * 256 (ridge.hip)
LANES = 256               # BLOCK; lane t of a workgroup owns the voxels base + k * 256 + t, k = 0..15


def shape_id(shape):
    return "x".join(str(n) for n in shape)


def seed_of(shape):
    return 7000 + SHAPES.index(tuple(shape))


def volume(shape):
    return volgen.membrane_volume(tuple(shape), seed_of(shape))


def random_mask(shape, seed=None):
    """~70 % ones.  (volgen.block_mask needs axes of at least 5.)"""
    seed = seed_of(shape) + 500 if seed is None else seed
    return (np.random.default_rng(seed).random(tuple(shape)) > 0.3).astype(f32)


# ---- survivor patterns of the direction kernel -----------------------------------------------------------------------
def survivor_patterns(nvox):
    """name -> bool[nvox]: which voxels keep a non-zero score"""
    v = np.arange(nvox)
    rng = np.random.default_rng(nvox)
    edges = np.zeros(nvox, bool)
    for k in range(1, nvox // P + 1):       # {kP - 1, kP}: the last voxel of one workgroup and the first of the next
        edges[k * P - 1] = True
        if k * P < nvox:
            edges[k * P] = True
    first, last = np.zeros(nvox, bool), np.zeros(nvox, bool)
    first[0], last[-1] = True, True
    return {
        "all": np.ones(nvox, bool),                   # a full LDS list: 4096 entries per workgroup
        "none": np.zeros(nvox, bool),                 # an empty list
        "first": first,
        "last": last,
        "chunk_edges": edges,
        "lane255": v % LANES == LANES - 1,            # one lane keeps all 16 of its voxels, every other lane none
        "slot15": (v % P) // LANES == 15,             # only the last of each lane's 16 voxels
        "rand05": rng.random(nvox) < 0.05,
        "rand95": rng.random(nvox) < 0.95,
    }


def pattern_scores(keep):
    """positive float32 scores of every size where keep is set, +0 elsewhere"""
    rng = np.random.default_rng(int(keep.sum()) + 1)
    s = np.exp(rng.uniform(-20, 20, keep.size)).astype(f32)
    return np.where(keep, s, f32(0)).astype(f32)


# (name, value, survives): the rule is the IEEE comparison `score != 0` of the reference's host code
VALUE_CLASSES = [("one", f32(1.0), True), ("minus_one", f32(-1.0), True), ("nan", f32(np.nan), True),
                 ("denormal", f32(1e-45), True), ("minus_zero", f32(-0.0), False)]
assert f32(1e-45) != 0 and np.signbit(f32(-0.0))


def value_scores(nvox, value):
    """-> (score field with `value` at a random 5 % of the voxels and +0 elsewhere, where it was written)"""
    at = np.random.default_rng(nvox + 17).random(nvox) < 0.05
    at[nvox // 2] = True
    s = np.zeros(nvox, f32)
    s[at] = value
    return s, at


# ---- the CPU restatement's results, once per process -----------------------------------------------------------------
_cache = {}


def ratio(oracle):
    return oracle.ratio_from_threshold(THRESHOLD)


def reference(oracle, shape, sigma, masked):
    """dict(src, mask, smoothed, grad, hess): the oracle's Gaussian and CalcHessian of volume(shape)"""
    key = ("hess", tuple(shape), float(sigma), bool(masked))
    if key not in _cache:
        src = volume(shape)
        mask = random_mask(shape) if masked else None
        smoothed = oracle.gauss_ratio(src, (sigma,) * 3, ratio(oracle), mask)[0]
        grad, hess = oracle.calc_hessian(src, sigma, ratio(oracle), mask)
        _cache[key] = dict(src=src, mask=mask, smoothed=smoothed, grad=grad, hess=hess)
    return _cache[key]


def saliency_reference(oracle, shape, masked, order):
    """reference(shape, SIGMA, masked) plus the oracle's sal, dirs and d6 (eigenvalues and Shoemake triple) in `order`"""
    key = ("sal", tuple(shape), bool(masked), int(order))
    if key not in _cache:
        r = dict(reference(oracle, shape, SIGMA, masked))
        r["sal"], r["dirs"] = oracle.hessian_saliency(r["hess"], order, r["mask"])
        r["d6"] = oracle.diagonalize(r["hess"], order)
        r["valid"] = np.ones(tuple(shape), bool) if r["mask"] is None else r["mask"] != 0
        _cache[key] = r
    return _cache[key]


# ---- matrices and tensors ----------------------------------------------------------------------------------------------
def hessian_matrices(oracle):
    """the unmasked Hessians of every shape, as one [n, 6] list"""
    if "mats" not in _cache:
        _cache["mats"] = np.ascontiguousarray(np.concatenate(
            [reference(oracle, s, SIGMA, False)["hess"].reshape(-1, 6) for s in SHAPES], 0))
    return _cache["mats"]


LINEAR_SIZES = (1, 255, 256, 257, 70001)     # around one workgroup of the linear kernels, and many workgroups
TV_SHAPE, TV_SIGMA = (9, 20, 33), 3.0

SYNTHETIC_TENSORS = np.array([
    [0, 0, 0, 0, 0, 0],                                   # the zero tensor
    [1, 1, 1, 0, 0, 0], [0.1, 0.1, 0.1, 0, 0, 0], [-3.7, -3.7, -3.7, 0, 0, 0], [1e-20, 1e-20, 1e-20, 0, 0, 0],   # c * identity
    [1, 0, 0, 0, 0, 0], [0, 0, 4, 0, 0, 0], [0.36, 0, 0.64, 0, 0, 0.48], [1, 4, 9, 2, 6, 3],   # rank 1: n n^T
    [2, -1, 0.5, 0.3, -0.7, 1.1],                         # indefinite
    [1e30, 2e30, -1e30, 3e29, 0, 1e29], [3e30, 3e30, 3e30, 1e30, 1e30, 1e30],   # entries near 1e30
], f32)
N_DEGENERATE = 5      # rows 0..4 above: l0 == l1 == l2 exactly


def score_tensors(oracle):
    """[n, 6]: the vote tensors of a 6 % sparse random field (starting at a voted row), then the synthetic rows"""
    if "tensors" not in _cache:
        rng = np.random.default_rng(61)
        sal = rng.random(TV_SHAPE, dtype=f32)
        sal[rng.random(TV_SHAPE) > 0.06] = 0.0
        d = rng.standard_normal(TV_SHAPE + (3,)).astype(f32)
        d /= np.linalg.norm(d, axis=-1, keepdims=True).astype(f32)
        ten = oracle.tv_dense_stick(sal, np.ascontiguousarray(d), TV_SIGMA, 4, 2.0 ** 0.5).reshape(-1, 6)
        start = int(np.argmax(np.abs(ten).max(axis=1) > 0))
        _cache["tensors"] = np.ascontiguousarray(np.concatenate([np.roll(ten, -start, axis=0), SYNTHETIC_TENSORS], 0))
    return _cache["tensors"]


def tensors_of_size(oracle, n):
    """n rows: a prefix of score_tensors, or tiles of it; the synthetic rows close every size that has room for them"""
    base = score_tensors(oracle)
    t = np.resize(base, (n, 6)).copy()
    k = len(SYNTHETIC_TENSORS)
    if n >= 2 * k:
        t[-k:] = SYNTHETIC_TENSORS
    return np.ascontiguousarray(t)
