"""The ridge stage's references and checkers, on the CPU (tests/ridge_np.py, tests/ridge_cases.py).

Three things are shown here so that tests/test_ridge_gpu.py can rely on them:
  * the plain numpy Hessian equals the CPU restatement bit for bit, and the restatement equals the real reference templates
    (where oracle/_ref is built) on every shape of ridge_cases.py;
  * every checker passes on the restatement's own outputs with the bounds the GPU tests use, and the inputs have the
    properties those bounds rely on (well-separated eigenvalues almost everywhere, few Shoemake triples next to 0 or 1);
  * every checker trips on the mutant meant for it.  The mutants are numpy restatements of plausible kernel defects built
    from the restatement's outputs: nothing here runs on a GPU."""
import numpy as np
import pytest

import ridge_cases as rc
import ridge_np as rn
from conftest import assert_bits_equal, assert_close_rel, golden

f32 = np.float32
RTOL = 1e-5      # BASELINE.json's north_star tolerance for float voxel values
IDS = [rc.shape_id(s) for s in rc.SHAPES]


# ------------------------------------------------------------------------------- references against each other
@pytest.mark.parametrize("shape", rc.SHAPES, ids=IDS)
def test_numpy_hessian_equals_oracle(oracle, shape):
    for sigma in rc.SIGMAS:
        r = rc.reference(oracle, shape, sigma, False)
        grad, hess = rn.hessian(r["smoothed"], sigma)
        assert_bits_equal(hess, r["hess"], "hessian sigma=%g" % sigma)
        assert_bits_equal(grad, r["grad"], "gradient sigma=%g" % sigma)
        r = rc.reference(oracle, shape, sigma, True)
        grad, hess = rn.hessian(r["smoothed"], sigma)
        m = r["mask"]
        assert 0 < int((m == 0).sum()) < m.size
        # equal at the unmasked voxels; the oracle leaves the masked ones at the zeros they came with
        assert_bits_equal(rn.masked(hess, m), r["hess"], "masked hessian sigma=%g" % sigma)
        assert_bits_equal(rn.masked(grad, m), r["grad"], "masked gradient sigma=%g" % sigma)
        assert not np.any(r["hess"][m == 0]) and not np.any(r["grad"][m == 0])


@pytest.mark.parametrize("shape", rc.SHAPES, ids=IDS)
def test_oracle_equals_reference(oracle, ref, shape):
    for masked in (False, True):
        for sigma in rc.SIGMAS:
            r = rc.reference(oracle, shape, sigma, masked)
            gb, hb = ref.calc_hessian(r["src"], sigma, rc.ratio(oracle), r["mask"])
            assert_bits_equal(r["grad"], gb, "grad")
            assert_bits_equal(r["hess"], hb, "hess")
        for order in (0, 1):
            r = rc.saliency_reference(oracle, shape, masked, order)
            sb, db = ref.hessian_saliency(r["hess"], order, r["mask"])
            assert_bits_equal(r["sal"], sb, "saliency, order %d" % order)
            assert_bits_equal(r["dirs"], db, "directions, order %d" % order)
            assert_bits_equal(r["d6"], ref.diagonalize(r["hess"], order), "diagonalised hessian, order %d" % order)


def test_oracle_tensor_score_equals_reference(oracle, ref):
    t = rc.tensors_of_size(oracle, 70001)
    mask = rc.random_mask((len(t),), seed=5)
    for order in (0, 1):
        for m in (None, mask):
            a, b = np.full(len(t), rc.SENTINEL), np.full(len(t), rc.SENTINEL)
            oracle.tensor_saliency(t, order, a, m)
            ref.tensor_saliency(t, order, b, m)
            assert_bits_equal(a, b, "tensor score, order %d" % order)


# ----------------------------------------------------------------------------- the checkers on the oracle itself
@pytest.mark.parametrize("shape", rc.SHAPES, ids=IDS)
def test_checkers_pass_on_oracle(oracle, shape):
    for masked in (False, True):
        for order in (0, 1):
            r = rc.saliency_reference(oracle, shape, masked, order)
            v, h6 = r["valid"], r["hess"]
            eig = rn.check_eigenvalues(r["d6"][v], h6[v], order, RTOL, "oracle eigenvalues")
            s64 = np.where(v, rn.saliency64(h6, order), 0.0)
            assert_close_rel(r["sal"], s64, RTOL, "oracle saliency against float64")
            assert not np.any(r["sal"][~v])
            x0 = r["d6"][..., 3]
            st = rn.check_directions(r["dirs"], h6, order, x0, r["dirs"], v, "oracle directions")
            sep = float((rn.relative_gap(h6, order)[v] > 1e-2).mean())
            out = float(1.0 - rn.x0_in_band(x0)[v].mean())
            print("%s mask=%d order=%d: eigenvalue error %.3g, R_ref %.3g (%d voxels), | |d| - 1 | %.3g, well separated %.4f, "
                  "X0 out of band %.4f" % (rc.shape_id(shape), masked, order, eig, st["r_ref"], st["n_band"], st["norm_err"],
                                           sep, out))
            # what the GPU tests rely on: directions are well conditioned almost everywhere, and the band leaves out few voxels
            assert sep > 0.5
            assert out <= 0.02
            assert st["n_band"] > 0


def test_checkers_pass_on_oracle_matrices(oracle):
    g = golden("eigen")
    mats = rc.hessian_matrices(oracle)
    for oname, order in (("inc", 0), ("dec", 1)):
        a = rn.check_eigenvalues(g["diag_" + oname], g["mats"], order, RTOL, "golden eigenvalues")
        b = rn.check_eigenvalues(oracle.diagonalize(mats, order), mats, order, RTOL, "oracle eigenvalues of the hessians")
        print("order %d: eigenvalue error %.3g on eigen.npz, %.3g on the %d hessians" % (order, a, b, len(mats)))
    rn.check_eigen_frames(oracle.diagonalize, g["mats"], {0: g["diag_inc"], 1: g["diag_dec"]})


def test_tensor_score_checker_on_oracle(oracle):
    t = rc.tensors_of_size(oracle, 70001)
    for order in (0, 1):
        s = np.zeros(len(t), f32)
        oracle.tensor_saliency(t, order, s)
        worst = rn.check_tensor_score(s, t, order, s, "oracle tensor score")
        print("order %d: tensor score within %.3g of each row's largest entry" % (order, worst))
        k = len(rc.SYNTHETIC_TENSORS)
        assert not np.any(s[-k:][:rc.N_DEGENERATE]), "multiples of the identity score 0"
        swapped = np.zeros(len(t), f32)
        oracle.tensor_saliency(t, 1 - order, swapped)
        with pytest.raises(AssertionError):
            rn.check_tensor_score(swapped, t, order, s, "mutant: orders exchanged")
        d6 = oracle.diagonalize(t, order)
        with pytest.raises(AssertionError):
            rn.check_tensor_score((d6[:, 0] - d6[:, 2]).astype(f32), t, order, s, "mutant: score from l0, l2")


# ----------------------------------------------------------------------------------------------------- mutants
def _trips(fn, *a, **kw):
    with pytest.raises(AssertionError):
        fn(*a, **kw)


@pytest.mark.parametrize("shape", rc.SHAPES, ids=IDS)
def test_hessian_mutants_trip(oracle, shape):
    sigma = 1.732     # sigma != sigma * sigma
    r = rc.reference(oracle, shape, sigma, False)
    S = r["smoothed"]

    def differs(grad, hess, what, grad_too=True):
        _trips(assert_bits_equal, hess, r["hess"], what)
        if grad_too:
            _trips(assert_bits_equal, grad, r["grad"], what)

    differs(*rn.hessian_from(rn.fetcher(S, (False, False, False)), sigma), "no clamp: the stencil wraps")
    for axis in range(3):
        clamp = [True] * 3
        clamp[axis] = False
        differs(*rn.hessian_from(rn.fetcher(S, tuple(clamp)), sigma), "clamped on two axes only")
    F = rn.fetcher(S)
    flipped = lambda dx, dy, dz: F(dx, -dy, dz)      # hxy: (+,+) and (-,-) exchanged with (+,-) and (-,+)
    g, h = rn.hessian_from(flipped, sigma)
    _trips(assert_bits_equal, h[..., 3], r["hess"][..., 3], "hxy with the signs of its terms exchanged")
    differs(*rn.hessian_from(F, sigma, hess_scale=f32(sigma)), "sigma in place of sigma * sigma", grad_too=False)
    # and the unmutated stencil passes the same check
    g, h = rn.hessian_from(F, sigma)
    assert_bits_equal(h, r["hess"])
    assert_bits_equal(g, r["grad"])


@pytest.mark.parametrize("shape", rc.SHAPES, ids=IDS)
def test_eigen_and_direction_mutants_trip(oracle, shape):
    for order in (0, 1):
        r = rc.saliency_reference(oracle, shape, False, order)
        other = rc.saliency_reference(oracle, shape, False, 1 - order)
        h6, d6, x0 = r["hess"], r["d6"], r["d6"][..., 3]
        _trips(rn.check_eigenvalues, other["d6"], h6, order, RTOL, "orders exchanged")
        _, frames = oracle.evects(h6.reshape(-1, 6), order)
        row1 = np.ascontiguousarray(frames[:, 1, :]).reshape(r["dirs"].shape)
        assert_bits_equal(np.ascontiguousarray(frames[:, 0, :]).reshape(r["dirs"].shape), r["dirs"], "row 0 is the direction")
        _trips(rn.check_directions, row1, h6, order, x0, r["dirs"], None, "the direction of eigenvalue 1")
        _trips(rn.check_directions, other["dirs"], h6, order, x0, r["dirs"], None, "the direction of eigenvalue 2")
        _trips(rn.check_directions, np.ascontiguousarray(r["dirs"][..., [1, 0, 2]]), h6, order, x0, r["dirs"], None, "x and y exchanged")
        _trips(rn.check_directions, r["dirs"] * f32(1.00001), h6, order, x0, r["dirs"], None, "not a unit vector")
        # the component-wise bar of the exact mode sees the same mutants
        ok = rn.relative_gap(h6, order) > 1e-2
        for mut in (row1, np.ascontiguousarray(r["dirs"][..., [1, 0, 2]])):
            assert np.max(np.abs(mut[ok] - r["dirs"][ok])) > 2e-5
        l0, l2 = d6[..., 0].astype(np.float64), d6[..., 2].astype(np.float64)
        wrong = ((l0 * l0 - l2 * l2) ** 2).astype(f32)
        _trips(assert_close_rel, wrong, r["sal"], RTOL, "saliency from l0 and l2")
        _trips(assert_close_rel, wrong, rn.saliency64(h6, order), RTOL, "saliency from l0 and l2, against float64")
        _trips(assert_close_rel, other["sal"], rn.saliency64(h6, order), RTOL, "saliency of the other order")


def _emulate(dirs_all, keep, sentinel=rc.SENTINEL):
    """what ridge_directions_kernel leaves in a sentinel-filled buffer when it takes `keep` for the survivors"""
    out = np.full(dirs_all.shape, sentinel, f32)
    out[:, keep] = dirs_all[:, keep]
    return out


@pytest.mark.parametrize("shape", rc.COMPACTION_SHAPES, ids=[rc.shape_id(s) for s in rc.COMPACTION_SHAPES])
def test_survivor_mutants_trip(oracle, shape):
    r = rc.saliency_reference(oracle, shape, False, 1)
    nvox = r["sal"].size
    dirs_all = np.ascontiguousarray(np.moveaxis(r["dirs"], -1, 0)).reshape(3, nvox)
    assert not np.any(dirs_all.view(np.uint32) == rn.sentinel_bits(rc.SENTINEL))
    pats = rc.survivor_patterns(nvox)
    tripped = {"partial": 0, "shift": 0}
    for name, keep in pats.items():
        assert np.array_equal(rn.survivors(rc.pattern_scores(keep)), keep), name
        rn.check_survivor_directions(_emulate(dirs_all, keep), dirs_all, keep, rc.SENTINEL, name)
        if keep.any():
            # a direction written at a dropped voxel / a survivor left out / the neighbour's direction
            extra = keep.copy()
            extra[np.flatnonzero(~keep)[0] if not keep.all() else 0] = True
            if not keep.all():
                _trips(rn.check_survivor_directions, _emulate(dirs_all, extra), dirs_all, keep, rc.SENTINEL, name)
            fewer = keep.copy()
            fewer[np.flatnonzero(keep)[-1]] = False
            _trips(rn.check_survivor_directions, _emulate(dirs_all, fewer), dirs_all, keep, rc.SENTINEL, name)
            one_plane = _emulate(dirs_all, keep)
            one_plane[2, np.flatnonzero(keep)[0]] = rc.SENTINEL      # the third plane alone
            _trips(rn.check_survivor_directions, one_plane, dirs_all, keep, rc.SENTINEL, name)
        # the list drops the last partial chunk
        partial = keep.copy()
        partial[(nvox // rc.P) * rc.P:] = False
        if not np.array_equal(partial, keep):
            _trips(rn.check_survivor_directions, _emulate(dirs_all, partial), dirs_all, keep, rc.SENTINEL, name)
            tripped["partial"] += 1
        # the list is shifted by one voxel
        shifted = np.roll(keep, 1)
        if not np.array_equal(shifted, keep):
            _trips(rn.check_survivor_directions, _emulate(dirs_all, shifted), dirs_all, keep, rc.SENTINEL, name)
            tripped["shift"] += 1
    assert tripped["shift"] >= 3
    assert tripped["partial"] >= 3 or nvox % rc.P == 0
    # score values: the IEEE rule, and the mutant that takes -0 for a survivor
    for name, value, survives in rc.VALUE_CLASSES:
        sal, at = rc.value_scores(nvox, value)
        keep = rn.survivors(sal)
        assert np.array_equal(keep, at if survives else np.zeros(nvox, bool)), name
        rn.check_survivor_directions(_emulate(dirs_all, keep), dirs_all, keep, rc.SENTINEL, name)
        by_bits = sal.view(np.uint32) != 0          # mutant: compares the bits, so -0 survives
        by_order = np.nan_to_num(sal, nan=0.0) > 0  # mutant: `score > 0`, so NaN and negative scores are dropped
        flushed = np.abs(np.nan_to_num(sal, nan=1.0)) >= np.finfo(f32).tiny   # mutant: denormals flushed to zero
        for mutant, hit in ((by_bits, name == "minus_zero"), (by_order, name in ("minus_one", "nan")), (flushed, name == "denormal")):
            if hit:
                _trips(rn.check_survivor_directions, _emulate(dirs_all, mutant), dirs_all, keep, rc.SENTINEL, name)
            else:
                assert np.array_equal(mutant, keep), name
