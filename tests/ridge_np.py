"""Plain references and checkers for the ridge stage (csrc/ridge.hip, csrc/eigen3.hpp), numpy only: no GPU, no ctypes.

References
  hessian          the 19-point Hessian and the central-difference gradient in float32, in the operand order of
                   visfd_utils.hpp:538-564 and feature.hpp:1331-1333 (ridge.hip: hessian_at and the gradient lines of
                   hessian_kernel), every voxel using the stencil of its centre clamped to [1, n-2];
  eigh64           numpy.linalg.eigh of the full symmetric matrices in float64;
  saliency64       (l0^2 - l1^2)^2, the ridge score (handlers.cpp:1653-1740);
  tensor_score64   l0 - l1, the post-vote score (handlers.cpp:1873-1888).

Checkers, shared by tests/test_ridge.py (where they are shown to pass on the oracle and to trip on mutants) and
tests/test_ridge_gpu.py (where they judge the kernels):
  check_eigenvalues, direction_residual, relative_gap, check_directions, check_tensor_score, check_survivor_directions,
  check_eigen_frames.

Flat symmetric matrices are (xx, yy, zz, xy, yz, xz); volumes are [nz, ny, nx]; eigenvalue order 0 is increasing, 1
decreasing (selfadjoint_eigen3::INCREASING_EIVALS / DECREASING_EIVALS)."""
import numpy as np

f32 = np.float32

NORM_TOL = 1e-6            # | |d| - 1 | of a principal direction (float Shoemake round trip; the oracle reaches 4e-7)
X0_BAND = (1e-3, 1 - 1e-3)  # Shoemake X0 outside this band: the float unpacking takes a square root next to zero
RESIDUAL_MARGIN = 10.0     # device residual bound = RESIDUAL_MARGIN * the oracle's own worst residual on the same voxels


# ---------------------------------------------------------------------------------------------------- references
def fetcher(S, clamp=(True, True, True)):
    """F(dx, dy, dz): for every voxel, the value of the smoothed volume S at (centre + offset).  The centre is the voxel
    clamped to the interior [1, n-2] (visfd_utils.hpp:597-610) on the axes (z, y, x) where `clamp` is set; on the others
    the index wraps around -- that form exists for the mutants of tests/test_ridge.py only."""
    S = np.ascontiguousarray(S, f32)
    idx = [np.clip(np.arange(n), 1, n - 2) if c else np.arange(n) for n, c in zip(S.shape, clamp)]
    nz, ny, nx = S.shape

    def F(dx, dy, dz):
        return S[np.ix_((idx[0] + dz) % nz, (idx[1] + dy) % ny, (idx[2] + dx) % nx)]
    return F


def hessian_from(F, sigma, hess_scale=None):
    """(grad[..., 3], hess[..., 6]) from a fetcher, float32 throughout.  hess_scale: the factor of the second derivatives
    (sigma * sigma in float32 unless a mutant says otherwise)."""
    sg = f32(sigma)
    s2 = f32(sg * sg) if hess_scale is None else f32(hess_scale)
    half, quarter = f32(0.5), f32(0.25)
    g = [half * (F(1, 0, 0) - F(-1, 0, 0)), half * (F(0, 1, 0) - F(0, -1, 0)), half * (F(0, 0, 1) - F(0, 0, -1))]
    f0 = F(0, 0, 0)
    two_f0 = f32(2) * f0
    hxx = (F(1, 0, 0) + F(-1, 0, 0)) - two_f0
    hyy = (F(0, 1, 0) + F(0, -1, 0)) - two_f0
    hzz = (F(0, 0, 1) + F(0, 0, -1)) - two_f0
    hxy = quarter * (((F(1, 1, 0) + F(-1, -1, 0)) - F(1, -1, 0)) - F(-1, 1, 0))
    hyz = quarter * (((F(0, 1, 1) + F(0, -1, -1)) - F(0, 1, -1)) - F(0, -1, 1))
    hzx = quarter * (((F(1, 0, 1) + F(-1, 0, -1)) - F(-1, 0, 1)) - F(1, 0, -1))
    grad = np.stack([c * sg for c in g], axis=-1)
    hess = np.stack([c * s2 for c in (hxx, hyy, hzz, hxy, hyz, hzx)], axis=-1)
    assert grad.dtype == f32 and hess.dtype == f32
    return np.ascontiguousarray(grad), np.ascontiguousarray(hess)


def hessian(smoothed, sigma):
    """(grad[nz, ny, nx, 3], hess[nz, ny, nx, 6]) of a smoothed volume (every axis at least 3 wide)."""
    assert min(smoothed.shape) >= 3, "CalcHessian requires an image at least 3 voxels wide in x,y,z"
    return hessian_from(fetcher(smoothed), sigma)


def masked(field, mask, fill=0.0):
    """`field` ([nz, ny, nx, c]) with `fill` in every channel of the voxels where mask == 0."""
    out = field.copy()
    out[mask == 0] = fill
    return out


def full64(m6):
    m6 = np.asarray(m6, np.float64)
    M = np.empty(m6.shape[:-1] + (3, 3), np.float64)
    for (a, b), k in {(0, 0): 0, (1, 1): 1, (2, 2): 2, (0, 1): 3, (1, 2): 4, (0, 2): 5}.items():
        M[..., a, b] = M[..., b, a] = m6[..., k]
    return M


def entry_scale(m6):
    """max |entry| of every flat matrix, float64"""
    return np.max(np.abs(np.asarray(m6, np.float64)), axis=-1)


def eigh64(m6, order):
    """-> (values [..., 3] in the requested order, vectors [..., 3, 3] with vectors[..., k, :] the unit eigenvector of
    values[..., k]), float64.  Matrices are divided by their largest entry first, so tiny and huge ones keep their digits."""
    s = entry_scale(m6)
    safe = np.where(s > 0, s, 1.0)
    w, v = np.linalg.eigh(full64(m6) / safe[..., None, None])
    w = w * safe[..., None]
    v = np.swapaxes(v, -1, -2)
    if order == 1:
        w, v = w[..., ::-1], v[..., ::-1, :]
    else:
        assert order == 0, "eigenvalue order 0 (increasing) or 1 (decreasing)"
    return np.ascontiguousarray(w), np.ascontiguousarray(v)


def saliency64(h6, order):
    w, _ = eigh64(h6, order)
    n = w[..., 0] * w[..., 0] - w[..., 1] * w[..., 1]
    return n * n


def tensor_score64(t6, order):
    w, _ = eigh64(t6, order)
    return w[..., 0] - w[..., 1]


def relative_gap(h6, order):
    """|l0 - l1| / max|entry| (0 for the zero matrix): how well the principal direction is conditioned"""
    w, _ = eigh64(h6, order)
    s = entry_scale(h6)
    return np.abs(w[..., 0] - w[..., 1]) / np.where(s > 0, s, 1.0)


def survivors(sal):
    """The voxels whose direction the pipeline computes: the IEEE comparison sal != 0 of the reference's host code
    (handlers.cpp:1751-1835).  NaN, negative and denormal scores survive; +0 and -0 do not."""
    with np.errstate(invalid="ignore"):
        return np.asarray(sal, f32) != f32(0)


# ------------------------------------------------------------------------------------------------------ checkers
def eigenvalue_error(d6, h6, order):
    """max over the three eigenvalues of |l - l64| / max|entry|, per matrix (0 for the zero matrix when l == 0)"""
    w, _ = eigh64(h6, order)
    s = entry_scale(h6)
    err = np.max(np.abs(np.asarray(d6, np.float64)[..., :3] - w), axis=-1)
    return np.where(s > 0, err / np.where(s > 0, s, 1.0), np.where(err > 0, np.inf, 0.0))


def check_eigenvalues(d6, h6, order, rtol, what=""):
    """|l - l64| <= rtol * max|h6 entry| for every eigenvalue of every matrix; -> the worst ratio"""
    assert np.all(np.isfinite(np.asarray(d6)[..., :3])), "%s: non-finite eigenvalue" % what
    e = eigenvalue_error(d6, h6, order).reshape(-1)
    worst = float(e.max()) if e.size else 0.0
    assert worst <= rtol, "%s: eigenvalue off by %g of the matrix's largest entry (bound %g) at matrix %d" % (
        what, worst, rtol, int(np.argmax(e)))
    return worst


def direction_residual(dirs, h6, order):
    """-> (|| H d - l0 d ||_inf / max|entry|, | ||d|| - 1 |) per voxel, float64; dirs [..., 3], h6 [..., 6]"""
    d = np.asarray(dirs, np.float64)
    w, _ = eigh64(h6, order)
    s = entry_scale(h6)
    Hd = np.einsum("...ij,...j->...i", full64(h6), d)
    res = np.max(np.abs(Hd - w[..., :1] * d), axis=-1) / np.where(s > 0, s, 1.0)
    return res, np.abs(np.sqrt(np.sum(d * d, axis=-1)) - 1.0)


def x0_in_band(x0):
    x0 = np.asarray(x0, np.float64)
    return (x0 >= X0_BAND[0]) & (x0 <= X0_BAND[1])


def check_directions(dirs, h6, order, x0_ref, dirs_ref, where=None, what=""):
    """The direction criterion of both eigen modes.  On the voxels of `where` (all when None): | |d| - 1 | <= NORM_TOL; and
    on those whose oracle Shoemake X0 (`x0_ref`) lies inside X0_BAND, the residual of d as an eigenvector of eigenvalue 0
    stays within RESIDUAL_MARGIN times the oracle's own worst residual (`dirs_ref`) on the same voxels.
    -> dict(r_ref, r_got, norm_err, n_band)"""
    sel = np.ones(np.asarray(x0_ref).shape, bool) if where is None else np.asarray(where, bool)
    res, nerr = direction_residual(dirs, h6, order)
    res_ref, _ = direction_residual(dirs_ref, h6, order)
    assert np.all(np.isfinite(np.asarray(dirs)[sel])), "%s: non-finite direction" % what
    worst_norm = float(nerr[sel].max()) if sel.any() else 0.0
    assert worst_norm <= NORM_TOL, "%s: | |d| - 1 | = %g > %g" % (what, worst_norm, NORM_TOL)
    band = sel & x0_in_band(x0_ref)
    r_ref = float(res_ref[band].max()) if band.any() else 0.0
    r_got = float(res[band].max()) if band.any() else 0.0
    assert r_got <= RESIDUAL_MARGIN * r_ref, "%s: residual %g of the direction at voxel %s exceeds %g x the oracle's %g" % (
        what, r_got, np.unravel_index(int(np.argmax(np.where(band, res, -1.0))), band.shape), RESIDUAL_MARGIN, r_ref)
    return {"r_ref": r_ref, "r_got": r_got, "norm_err": worst_norm, "n_band": int(band.sum())}


def check_tensor_score(got, t6, order, want, what="", rtol=1e-5):
    """The bounds of the post-vote score: rtol of the field's scale against float64 and against `want` (the oracle) -- and,
    because one row near 1e30 sets that scale for every row, also row by row: the score is a difference of two eigenvalues,
    each within rtol of the row's largest entry (check_eigenvalues), so within 2 * rtol of it.  -> the worst row's ratio"""
    from conftest import assert_close_rel
    s64 = tensor_score64(t6, order)
    assert np.all(np.isfinite(got)), what
    assert_close_rel(got, s64, rtol, what + " against float64")
    assert_close_rel(got, want, rtol, what + " against the oracle")
    row = np.abs(np.asarray(got, np.float64) - s64) / np.maximum(entry_scale(t6), 1e-300)
    assert row.max() <= 2 * rtol, "%s: row %d off by %g of its largest entry" % (what, int(np.argmax(row)), row.max())
    return float(row.max())


def sentinel_bits(sentinel):
    return np.array([sentinel], f32).view(np.uint32)[0]


def check_survivor_directions(dirs_out, dirs_all, keep, sentinel, what=""):
    """dirs_out, dirs_all: planar [3, ...] float32; keep: [...] bool.  Bit equality with dirs_all where keep is set, the
    sentinel's bits everywhere else, in all three planes."""
    out = np.ascontiguousarray(dirs_out, f32).reshape(3, -1).view(np.uint32)
    ref = np.ascontiguousarray(dirs_all, f32).reshape(3, -1).view(np.uint32)
    k = np.asarray(keep, bool).reshape(-1)
    assert out.shape == ref.shape and out.shape[1] == k.size, (what, out.shape, ref.shape, k.size)
    sb = sentinel_bits(sentinel)
    for c in range(3):
        bad = np.flatnonzero(out[c][k] != ref[c][k])
        assert bad.size == 0, "%s: plane %d: %d of %d survivors without their direction, first at voxel %d" % (
            what, c, bad.size, int(k.sum()), int(np.flatnonzero(k)[bad[0]]))
        bad = np.flatnonzero(out[c][~k] != sb)
        assert bad.size == 0, "%s: plane %d: %d dropped voxels were written, first at voxel %d" % (
            what, c, bad.size, int(np.flatnonzero(~k)[bad[0]]))


# ---- the frame encoded by a Shoemake triple (moved here from test_gpu_parity.py so both eigen modes share the checks) ----
def shoemake_frame(sm):
    """Shoemake triple -> quaternion -> rotation matrix, the decoding half of the reference's frame round trip
    (lin3_utils.hpp:311-337 Shoemake2Quaternion, :275-305 Quaternion2Matrix), in float64 for the checks below."""
    sm = sm.astype(np.float64)
    t1, t2 = 2 * np.pi * sm[:, 1], 2 * np.pi * sm[:, 2]
    r1, r2 = np.sqrt(1.0 - sm[:, 0]), np.sqrt(sm[:, 0])
    q0, q1, q2, q3 = np.sin(t1) * r1, np.cos(t1) * r1, np.sin(t2) * r2, np.cos(t2) * r2
    M = np.empty((len(sm), 3, 3))
    M[:, 0, 0] = 1 - 2 * q2 * q2 - 2 * q3 * q3
    M[:, 1, 1] = 1 - 2 * q1 * q1 - 2 * q3 * q3
    M[:, 2, 2] = 1 - 2 * q1 * q1 - 2 * q2 * q2
    M[:, 0, 1] = 2 * (q1 * q2 - q3 * q0)
    M[:, 1, 0] = 2 * (q1 * q2 + q3 * q0)
    M[:, 1, 2] = 2 * (q2 * q3 - q1 * q0)
    M[:, 2, 1] = 2 * (q2 * q3 + q1 * q0)
    M[:, 0, 2] = 2 * (q1 * q3 + q2 * q0)
    M[:, 2, 0] = 2 * (q1 * q3 - q2 * q0)
    return M


def check_eigen_frames(diagonalize, mats, refs):
    """The body of test_gpu_parity.py::test_eigen_solver_frames, for any eigen mode.  diagonalize(mats, order) -> [n, 6];
    refs = {0: reference [n, 6] in increasing order, 1: in decreasing order}.  The Shoemake triple is decoded with the
    reference's formulas and checked three ways: the frame is orthonormal; it diagonalises the matrix (V^T diag(lambda) V = M
    within 1e-5 of the matrix's scale -- this also pins the arbitrary frames of degenerate matrices); and where the
    eigenvalues are well separated every eigenvector equals the reference's up to sign."""
    from conftest import assert_close_rel
    full = np.zeros((len(mats), 3, 3), np.float64)
    for (a, b), k in {(0, 0): 0, (1, 1): 1, (2, 2): 2, (0, 1): 3, (1, 2): 4, (0, 2): 5}.items():
        full[:, a, b] = full[:, b, a] = mats[:, k]
    scale = np.max(np.abs(mats), axis=1).astype(np.float64) + 1e-300
    for order in (0, 1):
        d = diagonalize(mats, order)
        ref = refs[order]
        assert np.all(np.isfinite(d)), "non-finite output"
        vecs, rvecs = shoemake_frame(d[:, 3:6]), shoemake_frame(ref[:, 3:6])     # rows of vecs[i] = eigenvectors
        V = vecs.astype(np.float64)
        eye = np.einsum("nij,nkj->nik", V, V)
        assert np.max(np.abs(eye - np.eye(3))) <= 2e-6, "frame not orthonormal: %g" % np.max(np.abs(eye - np.eye(3)))
        assert np.all(np.linalg.det(V) > 0.99), "frame is not a proper rotation (eigen3_simple.hpp:316-319)"
        recon = np.einsum("nki,nk,nkj->nij", V, d[:, :3].astype(np.float64), V)
        err = np.max(np.abs(recon - full), axis=(1, 2)) / scale
        assert np.max(err) <= 1e-5, "V^T diag(lambda) V != M: rel err %g at case %d" % (np.max(err), int(np.argmax(err)))
        # well-separated spectra: the reference's own eigenvectors, up to sign
        lam = np.sort(ref[:, :3].astype(np.float64), axis=1)
        gap = np.minimum(lam[:, 1] - lam[:, 0], lam[:, 2] - lam[:, 1]) / scale
        sep = gap > 1e-2
        assert sep.sum() > 3000
        dots = np.abs(np.einsum("nij,nij->ni", V[sep], rvecs[sep].astype(np.float64)))
        assert np.min(dots) >= 1.0 - 1e-6, "eigenvector differs from the reference's: |cos| = %.9f" % np.min(dots)
        # exactly degenerate inputs (multiples of the identity, the zero matrix): the reference returns the identity frame
        for i in range(len(mats)):
            if mats[i, 0] == mats[i, 1] == mats[i, 2] and not np.any(mats[i, 3:]):
                assert np.max(np.abs(np.abs(V[i]) - np.eye(3))) <= 1e-6, "frame of a multiple of the identity (case %d)" % i
                assert_close_rel(d[i, :3], ref[i, :3], 1e-6, "eigenvalues of a multiple of the identity")
