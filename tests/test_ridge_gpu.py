"""The ridge stage on the GPU (csrc/ridge.hip, csrc/eigen3.hpp) at its edges: rows longer than one workgroup, 3-wide axes,
both eigenvalue orders, both eigen modes (context option eig_f32), the survivor compaction of the direction kernel and the
post-vote score -- against the CPU restatement, against the plain numpy / float64 references of ridge_np.py, and with the
checkers that tests/test_ridge.py shows to trip on the corresponding defects.

Bounds: Hessian, gradient, fused-vs-two-step scores and survivor directions are compared bit for bit; eigenvalues, scores
and the post-vote score within 1e-5 (BASELINE.json's north_star tolerance) of the matrix's largest entry / the field's
scale; directions by ridge_np.check_directions.  The measured values are appended to ridge_edges.txt in the suite's output
directory, beside conftest.PERVOXEL_LOG (copied to profiles/ridge_edges.txt)."""
import os

import numpy as np
import pytest

import ridge_cases as rc
import ridge_np as rn
from conftest import PERVOXEL_LOG, assert_bits_equal, assert_close_rel, golden

pytestmark = pytest.mark.gpu

f32 = np.float32
RTOL = 1e-5
PV = 0.005     # the per-voxel reading of RTOL, as in test_tolerance_modes.py: the share of significant voxels allowed to miss it
REPORT = os.path.join(os.path.dirname(PERVOXEL_LOG), "ridge_edges.txt")   # where the suite keeps what it measures


def _note(line):
    try:
        os.makedirs(os.path.dirname(REPORT), exist_ok=True)
        with open(REPORT, "a") as f:
            f.write(line + "\n")
    except OSError:
        pass


@pytest.fixture(scope="module")
def ctx():
    from visfd_amd import api
    c = api.Context(0)
    yield c
    c.close()


def _dev(a):
    import torch
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


def _full(shape, value=rc.SENTINEL):
    import torch
    return torch.full(tuple(shape), float(value), dtype=torch.float32, device="cuda:0")


def _interleaved(t):
    """planar device tensor [c, ...] -> numpy [..., c]"""
    return np.ascontiguousarray(np.moveaxis(t.cpu().numpy(), 0, -1))


def _is_sentinel(a):
    return np.ascontiguousarray(a, f32).view(np.uint32) == rn.sentinel_bits(rc.SENTINEL)


def _sid(shapes):
    return [rc.shape_id(s) for s in shapes]


# ------------------------------------------------------------------------------------------- Hessian and gradient
@pytest.mark.parametrize("shape", rc.HESSIAN_GPU_SHAPES, ids=_sid(rc.HESSIAN_GPU_SHAPES))
def test_hessian_exact(ctx, oracle, shape):
    ratio = rc.ratio(oracle)
    for sigma in rc.SIGMAS:
        for masked in (False, True):
            r = rc.reference(oracle, shape, sigma, masked)
            what = "%s sigma=%g mask=%d" % (rc.shape_id(shape), sigma, masked)
            grad, hess = ctx.calc_hessian(r["src"], sigma, ratio, r["mask"])
            assert_bits_equal(hess, r["hess"], "hessian against the oracle, " + what)
            assert_bits_equal(grad, r["grad"], "gradient against the oracle, " + what)
            g_np, h_np = rn.hessian(r["smoothed"], sigma)
            if masked:
                g_np, h_np = rn.masked(g_np, r["mask"]), rn.masked(h_np, r["mask"])
            assert_bits_equal(hess, h_np, "hessian against numpy, " + what)
            assert_bits_equal(grad, g_np, "gradient against numpy, " + what)
            none, hess2 = ctx.calc_hessian(r["src"], sigma, ratio, r["mask"], want_grad=False)
            assert none is None
            assert_bits_equal(hess2, r["hess"], "hessian without the gradient, " + what)
            # the device face: what it does not compute it must not write
            g_d, h_d = _full((3,) + tuple(shape)), _full((6,) + tuple(shape))
            ctx.calc_hessian_dev(_dev(r["src"]), g_d, h_d, sigma, ratio, _dev(r["mask"]))
            ctx.synchronize()
            g_d, h_d = _interleaved(g_d), _interleaved(h_d)
            v = np.ones(tuple(shape), bool) if r["mask"] is None else r["mask"] != 0
            assert_bits_equal(h_d[v], r["hess"][v], "device-face hessian, " + what)
            assert_bits_equal(g_d[v], r["grad"][v], "device-face gradient, " + what)
            assert np.all(_is_sentinel(h_d[~v])) and np.all(_is_sentinel(g_d[~v])), "masked voxels were written, " + what
        zero = np.zeros(tuple(shape), f32)
        src = rc.volume(shape)
        grad, hess = ctx.calc_hessian(src, sigma, ratio, zero)
        g_o, h_o = oracle.calc_hessian(src, sigma, ratio, zero)
        assert_bits_equal(hess, h_o, "hessian under an all-zero mask")
        assert_bits_equal(grad, g_o, "gradient under an all-zero mask")


@pytest.mark.parametrize("shape", rc.TOO_THIN, ids=_sid(rc.TOO_THIN))
def test_hessian_rejects_thin_volumes(ctx, shape):
    from visfd_amd import api
    with pytest.raises(api.VisfdHipError):
        ctx.calc_hessian(np.zeros(shape, f32), 1.0, 2.5)


# --------------------------------------------------------------------------------------------------- eigen solver
def test_eigen_solver_both_modes(ctx, oracle):
    g = golden("eigen")
    sets = {"eigen.npz": g["mats"], "hessians": rc.hessian_matrices(oracle)}
    for name, mats in sets.items():
        scale = rn.entry_scale(mats)
        for order in (0, 1):
            want = oracle.diagonalize(mats, order)
            got = {}
            for mode in (0, 1):
                with ctx.options(eig_f32=mode):
                    got[mode] = ctx.diagonalize(mats, order)
                what = "%s order %d eig_f32=%d" % (name, order, mode)
                e64 = rn.check_eigenvalues(got[mode], mats, order, RTOL, what + " against float64")
                eo = np.max(np.abs(got[mode][:, :3].astype(np.float64) - want[:, :3]), axis=1) / np.maximum(scale, 1e-300)
                assert eo.max() <= RTOL, "%s: eigenvalue off the oracle's by %g of the largest entry (matrix %d)" % (
                    what, eo.max(), int(np.argmax(eo)))
                equal = float(np.mean(got[mode][:, :3].view(np.uint32) == want[:, :3].view(np.uint32)))
                _note("eigenvalues %-9s order %d eig_f32=%d: error %.3g of the largest entry against float64, %.3g against the "
                      "oracle (bound %g); bit-equal to the oracle %.5f (recorded)" % (name, order, mode, e64, eo.max(), RTOL, equal))
            assert np.any(got[1][:, :3].view(np.uint32) != got[0][:, :3].view(np.uint32)), \
                "eig_f32 did not run (eigenvalue bits equal the exact mode's)"


@pytest.mark.parametrize("mode", [0, 1])
def test_eigen_solver_frames_both_modes(ctx, mode):
    g = golden("eigen")
    with ctx.options(eig_f32=mode):
        rn.check_eigen_frames(ctx.diagonalize, g["mats"], {0: g["diag_inc"], 1: g["diag_dec"]})


# ----------------------------------------------------------------------------------------- saliency and directions
@pytest.mark.parametrize("shape", rc.SHAPES, ids=_sid(rc.SHAPES))
def test_saliency_and_directions(ctx, oracle, shape):
    ratio = rc.ratio(oracle)
    shape = tuple(shape)
    for masked in (False, True):
        base = rc.reference(oracle, shape, rc.SIGMA, masked)
        src_d, mask_d = _dev(base["src"]), _dev(base["mask"])
        for order in (0, 1):
            r = rc.saliency_reference(oracle, shape, masked, order)
            v, h6, x0 = r["valid"], r["hess"], r["d6"][..., 3]
            h6_d = _dev(np.moveaxis(h6, -1, 0))
            s64 = np.where(v, rn.saliency64(h6, order), 0.0)
            well = v & (rn.relative_gap(h6, order) > 1e-2)
            assert well[v].mean() > 0.5
            for mode in (0, 1):
                what = "%s mask=%d order=%d eig_f32=%d" % (rc.shape_id(shape), masked, order, mode)
                with ctx.options(eig_f32=mode):
                    sal_h, dirs_h = ctx.hessian_saliency(h6, order, r["mask"])
                    sal_f, dirs_f = _full(shape), _full((3,) + shape)
                    ctx.ridge_saliency_dev(src_d, sal_f, dirs_f, rc.SIGMA, ratio, order, mask_d)
                    sal_s, smoothed = _full(shape), _full(shape)
                    ctx.ridge_scores_dev(src_d, sal_s, smoothed, rc.SIGMA, ratio, order, mask_d)
                    sal_d, dirs_d = _full(shape), _full((3,) + shape)
                    ctx.hessian_saliency_dev(h6_d, sal_d, dirs_d, order, mask_d)
                    ctx.synchronize()
                sal_f, dirs_f, sal_s = sal_f.cpu().numpy(), _interleaved(dirs_f), sal_s.cpu().numpy()
                sal_d, dirs_d = sal_d.cpu().numpy(), _interleaved(dirs_d)
                assert_bits_equal(sal_f, sal_s, "fused scores against ridge_scores_dev, " + what)
                # the device face of hessian_saliency: the host face's bits, and nothing written where the mask is 0
                assert_bits_equal(sal_d, sal_h, "hessian_saliency_dev scores against the host face, " + what)
                assert_bits_equal(dirs_d[v], dirs_h[v], "hessian_saliency_dev directions against the host face, " + what)
                if masked:
                    assert np.all(_is_sentinel(dirs_d[~v])), "hessian_saliency_dev wrote the direction of a masked voxel, " + what
                    assert np.all(_is_sentinel(dirs_f[~v])), "fused kernel wrote the direction of a masked voxel, " + what
                    assert not np.any(dirs_h[~v].view(np.uint32)), "host face wrote the direction of a masked voxel, " + what
                for face, sal, dirs in (("hessian_saliency", sal_h, dirs_h), ("ridge_saliency_dev", sal_f, dirs_f)):
                    w = face + ", " + what
                    assert_close_rel(sal, r["sal"], RTOL, "scores against the oracle, " + w, pervoxel=PV)
                    assert_close_rel(sal, s64, RTOL, "scores against float64, " + w)
                    assert not np.any(sal[~v].view(np.uint32)), "masked scores are +0, " + w
                    if mode == 0:
                        worst = float(np.max(np.abs(dirs[well] - r["dirs"][well])))
                        assert worst <= 2e-5, "direction %g off the oracle's, %s" % (worst, w)
                    st = rn.check_directions(dirs, h6, order, x0, r["dirs"], v, w)
                    _note("directions %-18s %s: R_ref %.3g, device residual %.3g (bound %g x R_ref, %d voxels), | |d| - 1 | "
                          "%.3g (bound %g)%s" % (face, what, st["r_ref"], st["r_got"], rn.RESIDUAL_MARGIN, st["n_band"],
                                               st["norm_err"], rn.NORM_TOL,
                                               ", worst component against the oracle %.3g (bound 2e-5)" % worst if mode == 0 else ""))
                    _note("scores     %-18s %s: %.3g of the field's scale against the oracle, %.3g against float64 (bound %g)" % (
                        face, what, np.max(np.abs(sal.astype(np.float64) - r["sal"])) / np.max(np.abs(r["sal"])),
                        np.max(np.abs(sal - s64)) / np.max(np.abs(s64)), RTOL))


# -------------------------------------------------------------------------------------------- survivor compaction
@pytest.mark.parametrize("shape", rc.COMPACTION_SHAPES, ids=_sid(rc.COMPACTION_SHAPES))
def test_survivor_compaction(ctx, oracle, shape):
    ratio = rc.ratio(oracle)
    shape = tuple(shape)
    nvox = int(np.prod(shape))
    src_d = _dev(rc.volume(shape))
    runs = [(0, 1)]                                  # (eig_f32, order)
    if shape == rc.COMPACTION_BOTH_ORDERS:
        runs += [(0, 0), (1, 1)]
    cases = [(name, rc.pattern_scores(keep)) for name, keep in rc.survivor_patterns(nvox).items()]
    cases += [(name, rc.value_scores(nvox, value)[0]) for name, value, _ in rc.VALUE_CLASSES]
    for mode, order in runs:
        what = "%s order=%d eig_f32=%d" % (rc.shape_id(shape), order, mode)
        with ctx.options(eig_f32=mode):
            sal_all, dirs_all = _full(shape), _full((3,) + shape)
            ctx.ridge_saliency_dev(src_d, sal_all, dirs_all, rc.SIGMA, ratio, order)
            sal_s, smoothed = _full(shape), _full(shape)
            ctx.ridge_scores_dev(src_d, sal_s, smoothed, rc.SIGMA, ratio, order)
            ctx.synchronize()
            dirs_all = dirs_all.cpu().numpy()
            assert not np.any(_is_sentinel(dirs_all))
            for name, sal in cases:
                keep = rn.survivors(sal)
                sal_d, dirs = _dev(sal.reshape(shape)), _full((3,) + shape)
                ctx.ridge_directions_dev(smoothed, sal_d, dirs, rc.SIGMA, order)
                ctx.synchronize()
                rn.check_survivor_directions(dirs.cpu().numpy(), dirs_all, keep, rc.SENTINEL, "%s, %s" % (name, what))
                assert_bits_equal(sal_d.cpu().numpy().reshape(-1), sal, "the scores are read only, %s, %s" % (name, what))
            # the pipeline's own sequence: scores, the top-fraction cut, directions of what is left
            thr = ctx.threshold_fraction_dev(sal_s, 0.1)
            dirs = _full((3,) + shape)
            ctx.ridge_directions_dev(smoothed, sal_s, dirs, rc.SIGMA, order)
            ctx.synchronize()
            keep = rn.survivors(sal_s.cpu().numpy().reshape(-1))
            assert keep.any() and thr > 0
            rn.check_survivor_directions(dirs.cpu().numpy(), dirs_all, keep, rc.SENTINEL, "after the cut, " + what)
        _note("compaction %s: %d patterns and score classes and the cut at 0.1 (%d of %d voxels kept), bit for bit" % (
            what, len(cases), int(keep.sum()), nvox))


# ------------------------------------------------------------------------------------------------ post-vote score
@pytest.mark.parametrize("n", rc.LINEAR_SIZES)
def test_tensor_score(ctx, oracle, n):
    t = rc.tensors_of_size(oracle, n)
    t_d = _dev(np.ascontiguousarray(t.T))
    mask = rc.random_mask((n,), seed=n)
    rng = np.random.default_rng(n)
    image, background = rng.random(n, dtype=f32), rng.random(n, dtype=f32)
    weight = (image - background).astype(f32)
    k = len(rc.SYNTHETIC_TENSORS)
    for order in (0, 1):
        want = np.zeros(n, f32)
        oracle.tensor_saliency(t, order, want)
        for mode in (0, 1):
            what = "n=%d order=%d eig_f32=%d" % (n, order, mode)
            with ctx.options(eig_f32=mode):
                s_h = np.full(n, rc.SENTINEL)
                ctx.tensor_saliency(t, order, s_h)
                s_hm = np.full(n, rc.SENTINEL)
                ctx.tensor_saliency(t, order, s_hm, mask)
                s_d, s_dm, s_w = _full((n,)), _full((n,)), _full((n,))
                ctx.tensor_saliency_dev(t_d, s_d, order)
                ctx.tensor_saliency_dev(t_d, s_dm, order, _dev(mask))
                ctx.tensor_saliency_dev(t_d, s_w, order, None, _dev(image), _dev(background))
                ctx.synchronize()
            s_d, s_dm, s_w = s_d.cpu().numpy(), s_dm.cpu().numpy(), s_w.cpu().numpy()
            worst = rn.check_tensor_score(s_h, t, order, want, "tensor_saliency, " + what)
            rn.check_tensor_score(s_d, t, order, want, "tensor_saliency_dev, " + what)
            assert_bits_equal(s_d, s_h, "device face against host face, " + what)
            for face, s, full in (("host", s_hm, s_h), ("device", s_dm, s_d)):
                assert_bits_equal(s[mask != 0], full[mask != 0], "%s face, unmasked voxels, %s" % (face, what))
                assert np.all(_is_sentinel(s[mask == 0])), "%s face wrote a masked voxel, %s" % (face, what)
            assert_bits_equal(s_w, (s_d * weight).astype(f32), "score times (image - background), " + what)
            if mode == 0 and n >= 2 * k:
                assert not np.any(s_d[-k:][:rc.N_DEGENERATE].view(np.uint32) & 0x7fffffff), \
                    "the zero tensor and multiples of the identity score 0, " + what
            s64 = rn.tensor_score64(t, order)
            _note("tensor score %s: %.3g of the field's scale against float64, %.3g against the oracle (bound %g); worst row %.3g "
                  "of its largest entry (bound %g)" % (what, np.max(np.abs(s_d - s64)) / max(np.max(np.abs(s64)), 1e-300),
                                                       np.max(np.abs(s_d.astype(np.float64) - want)) / max(float(np.max(np.abs(want))), 1e-300),
                                                       RTOL, worst, 2 * RTOL))
