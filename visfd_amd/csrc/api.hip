// api.hip -- the filter, ridge, voting, morphology and extrema entry points of the extern "C" surface declared in
// include/visfd_hip.h (the context's are in context.hip, the blob detector's in blob_job.hip, the slab's in slab.hip).
// Device-pointer entry points orchestrate the stage functions; host-pointer entry points stage the caller's volumes
// through the context workspace (Stage, common.hpp: H2D, run, D2H) and are synchronous.
#include <algorithm>
#include <cmath>
#include <vector>

#include "common.hpp"
#include "tv_common.hpp"

namespace vh {

int gauss_dev(visfd_hip_ctx* ctx, const float* src, float* dst, const float* mask, i64 nx, i64 ny, i64 nz,
              const float sigma[3], const int hw[3], bool normalize, const GaussOpts& o) {
  VH_REQUIRE(ctx && src && dst && sigma && hw, "null argument");
  std::vector<float> t[3];
  for (int d = 0; d < 3; d++) {
    VH_REQUIRE(sigma[d] >= 0.0f, "sigma must be non-negative");
    VH_REQUIRE(hw[d] >= 0 && hw[d] <= MAX_HALFWIDTH, "filter halfwidth must be in [0, 64]");
    t[d].resize(2 * hw[d] + 1);
    host_gauss_taps(sigma[d], hw[d], t[d].data());
  }
  return dev_separable3d(ctx, src, dst, mask, nx, ny, nz, t[0].data(), hw[0], t[1].data(), hw[1], t[2].data(), hw[2],
                         normalize, o);
}

// Unmasked, both Gaussians first try the pair route (gauss_pair.hip), which declines everything it does not cover --
// arguments the calls below refuse included.
static int log_pair_try(visfd_hip_ctx* ctx, const float* src, float* dst, i64 nx, i64 ny, i64 nz, const float sa[3],
                        const float sb[3], const int hw[3], float scale, float* A, float* B) {
  if (!ctx || !src || !dst || !sa || !sb || !hw || ctx->opt.log_pair == 0) return GAUSS_DECLINED;
  LogPairRequest rq = {};
  rq.src = src; rq.dst = dst; rq.nx = nx; rq.ny = ny; rq.nz = nz; rq.scale = scale;
  for (int d = 0; d < 3; d++) {
    if (!(sa[d] >= 0.0f) || !(sb[d] >= 0.0f) || hw[d] < 0 || hw[d] > MAX_HALFWIDTH) return GAUSS_DECLINED;
    rq.a[d].h = rq.b[d].h = hw[d];
    host_gauss_taps(sa[d], hw[d], rq.a[d].t);
    host_gauss_taps(sb[d], hw[d], rq.b[d].t);
  }
  const int rc = log_pair_route(ctx, rq);
  if (rc != VISFD_HIP_OK) return rc;
  if (A) *A = (rq.a[0].t[hw[0]] * rq.a[1].t[hw[1]]) * rq.a[2].t[hw[2]];   // filter3d.hpp:1044-1046
  if (B) *B = (rq.b[0].t[hw[0]] * rq.b[1].t[hw[1]]) * rq.b[2].t[hw[2]];
  return VISFD_HIP_OK;
}

// ApplyDog (filter3d.hpp:1338-1402); with scale != 1 it is the body of ApplyLog (filter3d.hpp:1466-1498).
// dst = G_a(src); then the second Gaussian stores (dst - G_b(src)) * scale straight into dst: the launch that writes an
// element has read its minuend in the same thread, so in place is safe, and a multiplier of 1.0f is exact.
static int dog_dev(visfd_hip_ctx* ctx, const float* src, float* dst, const float* mask, i64 nx, i64 ny, i64 nz,
                   const float sa[3], const float sb[3], const int hw[3], float scale, float* A, float* B) {
  if (!mask) {
    const int rc = log_pair_try(ctx, src, dst, nx, ny, nz, sa, sb, hw, scale, A, B);
    if (rc != GAUSS_DECLINED) return rc;
  }
  VH_TRY(gauss_dev(ctx, src, dst, mask, nx, ny, nz, sa, hw, true, {A}));
  return gauss_dev(ctx, src, dst, mask, nx, ny, nz, sb, hw, true, {B, dst, scale});
}

// ApplyLog parameter derivation (filter3d.hpp:1451-1464, :1493)
LogPlan plan_log(const float sigma[3], float delta, float ratio) {
  LogPlan p;
  for (int d = 0; d < 3; d++) {
    p.sa[d] = (float)(sigma[d] * (1.0 - 0.5 * delta));
    p.sb[d] = (float)(sigma[d] * (1.0 + 0.5 * delta));
    p.hw[d] = (int)std::floor(ratio * std::fmax(p.sa[d], p.sb[d]));
  }
  p.scale = (float)(1.0 / (delta * delta));
  return p;
}

int log_dev(visfd_hip_ctx* ctx, const float* src, float* dst, const float* mask, i64 nx, i64 ny, i64 nz,
            const float sigma[3], float delta, float ratio, float* A, float* B) {
  const LogPlan p = plan_log(sigma, delta, ratio);
  for (int d = 0; d < 3; d++)
    VH_REQUIRE(p.hw[d] >= 0 && p.hw[d] <= MAX_HALFWIDTH, "LoG filter halfwidth must be in [0, 64]");
  float a = 0, b = 0;
  VH_TRY(dog_dev(ctx, src, dst, mask, nx, ny, nz, p.sa, p.sb, p.hw, p.scale, &a, &b));
  if (A) *A = a * p.scale;   // filter3d.hpp:1502-1505
  if (B) *B = b * p.scale;
  return VISFD_HIP_OK;
}

namespace {

void halfwidths_from_ratio(const float sigma[3], float ratio, int hw[3]) {   // filter3d.hpp:1240-1247: floor of the float product, at least 1
  for (int d = 0; d < 3; d++) {
    hw[d] = (int)std::floor(sigma[d] * ratio);
    if (hw[d] < 1) hw[d] = 1;
  }
}

// The isotropic Gaussian of half-width host_iso_halfwidth -- floor(sigma * ratio), feature.hpp:1223: no lower bound of 1
// here -- into dst, or into slot WS_D where dst is null (taken once the half-width has passed); *out tells where it went.
int gauss_iso_dev(visfd_hip_ctx* ctx, const float* src, float* dst, const float* mask, i64 nx, i64 ny, i64 nz, float sigma,
                  float ratio, bool normalize, const char* what, float** out = nullptr) {
  const int hwv = host_iso_halfwidth(sigma, ratio);
  VH_REQUIRE(hwv >= 0 && hwv <= MAX_HALFWIDTH, std::string(what) + " must be in [0, 64]");
  if (!dst) VH_TRY(ws(ctx, WS_D, (size_t)(nx * ny * nz), &dst));
  if (out) *out = dst;
  const float sg[3] = {sigma, sigma, sigma};
  const int hw[3] = {hwv, hwv, hwv};
  return gauss_dev(ctx, src, dst, mask, nx, ny, nz, sg, hw, normalize);
}

int calc_hessian_dev(visfd_hip_ctx* ctx, const float* src, float* grad, float* hess, const float* mask,
                     i64 nx, i64 ny, i64 nz, float sigma, float ratio) {
  VH_REQUIRE(ctx && src, "null argument");
  VH_TRY(check_dims(nx, ny, nz));
  // (dev_hessian says the same; said here, a volume too thin for the stencil is turned away before the Gaussian runs on it)
  if (nx < 3 || ny < 3 || nz < 3)
    return fail(VISFD_HIP_EINVAL, "CalcHessian requires an image at least 3 voxels wide in x,y,z");
  float* S = nullptr;
  VH_TRY(gauss_iso_dev(ctx, src, nullptr, mask, nx, ny, nz, sigma, ratio, true, "filter halfwidth", &S));
  return dev_hessian(ctx, S, mask, nx, ny, nz, sigma, grad, hess);
}

// Options of the entry points whose output is a float field: the tolerance mode where the context asks for it
GaussOpts field_opts(const visfd_hip_ctx* ctx, float* A_out) {
  GaussOpts o;
  o.A_out = A_out;
  o.fma = ctx->opt.gauss_fma != 0;
  return o;
}


// what the morphology and median faces check first; `who` and `tag` start the messages, a face without an op passes none
int face_check(visfd_hip_ctx* ctx, const float* src, float* dst, const float* mask, i64 nx, i64 ny, i64 nz, const char* who,
               const char* tag, int op = 0, int max_op = 0) {
  VH_REQUIRE(ctx && src && dst, "null argument");
  VH_REQUIRE(op >= 0 && op <= max_op, "unknown morphology op");
  VH_TRY(check_out_of_place(ctx, src, dst, mask, nx, ny, nz, who, tag));
  VH_HIP(hipSetDevice(ctx->device));
  return VISFD_HIP_OK;
}

}  // namespace
}  // namespace vh

using namespace vh;

extern "C" {

// ---- a1 ------------------------------------------------------------------------------------
int visfd_hip_gauss_taps(float sigma, int halfwidth, float* taps_out) {
  VH_REQUIRE(taps_out && halfwidth >= 0 && sigma >= 0.0f, "bad tap request");
  host_gauss_taps(sigma, halfwidth, taps_out);
  return VISFD_HIP_OK;
}
float visfd_hip_ratio_from_threshold(float thr) { return std::sqrt(-2 * std::log(thr)); }
int visfd_hip_gauss_halfwidths(const float sigma[3], float ratio, int hw[3]) {
  VH_REQUIRE(sigma && hw, "null argument");
  halfwidths_from_ratio(sigma, ratio, hw);
  return VISFD_HIP_OK;
}
// The Z window of the widest LoG in the float arithmetic of the kernels' own plan (plan_log), plus the plane the 26-neighbour
// scan reads beyond it: every slab caller of the blob stage takes its halo depth from here, so it cannot be one plane short
// of what the filters read (a double-precision restatement of floor(ratio * sigma * (1 + delta/2)) can round the other way).
int visfd_hip_blob_halo_depth(const float* blob_sigma, int n_sigma, float delta, float ratio, int* depth_out) {
  VH_REQUIRE(blob_sigma && n_sigma >= 1 && depth_out, "bad argument");
  int hw = 0;
  for (int i = 0; i < n_sigma; i++) {
    const float sg[3] = {blob_sigma[i], blob_sigma[i], blob_sigma[i]};
    hw = std::max(hw, plan_log(sg, delta, ratio).hw[2]);
  }
  *depth_out = hw + 1;
  return VISFD_HIP_OK;
}

// ---- a4 ------------------------------------------------------------------------------------
int visfd_hip_separable3d_dev(visfd_hip_ctx* ctx, const float* src, float* dst, const float* mask,
                              int64_t nx, int64_t ny, int64_t nz, const float* tx, int hx,
                              const float* ty, int hy, const float* tz, int hz, int normalize,
                              float* A_out) {
  VH_REQUIRE(ctx && src && dst && tx && ty && tz, "null argument");
  VH_HIP(hipSetDevice(ctx->device));
  return dev_separable3d(ctx, src, dst, mask, nx, ny, nz, tx, hx, ty, hy, tz, hz, normalize != 0, field_opts(ctx, A_out));
}

int visfd_hip_separable3d(visfd_hip_ctx* ctx, const float* src, float* dst, const float* mask, int64_t nx, int64_t ny,
                          int64_t nz, const float* tx, int hx, const float* ty, int hy, const float* tz, int hz,
                          int normalize, float* A_out) {
  return stage_filter(ctx, src, dst, mask, nx, ny, nz, false, [&](const float* ds, float* dd, const float* dm) {
    return visfd_hip_separable3d_dev(ctx, ds, dd, dm, nx, ny, nz, tx, hx, ty, hy, tz, hz, normalize, A_out);
  });
}

// ---- a5 ------------------------------------------------------------------------------------
int visfd_hip_apply_gauss_dev(visfd_hip_ctx* ctx, const float* src, float* dst, const float* mask,
                              int64_t nx, int64_t ny, int64_t nz, const float sigma[3],
                              const int hw[3], int normalize, float* A_out) {
  VH_REQUIRE(ctx, "null context");
  VH_HIP(hipSetDevice(ctx->device));
  return gauss_dev(ctx, src, dst, mask, nx, ny, nz, sigma, hw, normalize != 0, field_opts(ctx, A_out));
}

int visfd_hip_apply_gauss_slab_dev(visfd_hip_ctx* ctx, const float* src, float* dst, int64_t nx,
                                   int64_t ny, int64_t nz_local, int64_t z_lo, int64_t nz_global,
                                   const float sigma[3], const int hw[3], int normalize, float* A_out) {
  VH_REQUIRE(ctx, "null context");
  VH_REQUIRE(z_lo >= 0 && z_lo + nz_local <= nz_global, "slab outside the volume");
  VH_HIP(hipSetDevice(ctx->device));
  GaussOpts o = field_opts(ctx, A_out);
  o.z_lo = z_lo;
  o.nz_global = nz_global;
  return gauss_dev(ctx, src, dst, nullptr, nx, ny, nz_local, sigma, hw, normalize != 0, o);
}

int visfd_hip_apply_gauss(visfd_hip_ctx* ctx, const float* src, float* dst, const float* mask, int64_t nx, int64_t ny,
                          int64_t nz, const float sigma[3], const int hw[3], int normalize, float* A_out) {
  return stage_filter(ctx, src, dst, mask, nx, ny, nz, false, [&](const float* ds, float* dd, const float* dm) {
    return visfd_hip_apply_gauss_dev(ctx, ds, dd, dm, nx, ny, nz, sigma, hw, normalize, A_out);
  });
}

// ---- f4: LocalFluctuations (lib/visfd/filter3d.hpp:1698-1853), Gaussian weights only -------
int visfd_hip_local_fluctuations_dev(visfd_hip_ctx* ctx, const float* src, float* dst, const float* mask,
                                     int64_t nx, int64_t ny, int64_t nz, const float sigma[3], float exponent,
                                     float truncate_ratio, int normalize) {
  VH_REQUIRE(ctx && src && dst && sigma, "null argument");
  VH_REQUIRE(src != dst, "LocalFluctuations cannot run in place");
  VH_REQUIRE(exponent == 2.0f, "LocalFluctuations: only the Gaussian case (exponent 2) is provided");
  VH_HIP(hipSetDevice(ctx->device));
  VH_TRY(check_dims(nx, ny, nz));
  const i64 n = nx * ny * nz;
  int hw[3];
  halfwidths_from_ratio(sigma, truncate_ratio, hw);    // ApplyGauss(sigma[3], ratio), filter3d.hpp:1240-1247
  const float wpeak = host_gengauss3d_peak(sigma, exponent, truncate_ratio);
  float* p2 = nullptr;
  VH_TRY(ws(ctx, WS_C, (size_t)n, &p2));
  VH_TRY(gauss_dev(ctx, src, dst, mask, nx, ny, nz, sigma, hw, normalize != 0));   // local average
  VH_TRY(dev_sub_square(ctx, src, dst, p2, n));                                                      // (src - avg)^2
  VH_TRY(gauss_dev(ctx, p2, dst, mask, nx, ny, nz, sigma, hw, normalize != 0));    // its local average
  return dev_scale_clamp_sqrt(ctx, dst, n, wpeak);
}

int visfd_hip_local_fluctuations(visfd_hip_ctx* ctx, const float* src, float* dst, const float* mask, int64_t nx,
                                 int64_t ny, int64_t nz, const float sigma[3], float exponent, float truncate_ratio,
                                 int normalize) {
  return stage_filter(ctx, src, dst, mask, nx, ny, nz, false, [&](const float* ds, float* dd, const float* dm) {
    return visfd_hip_local_fluctuations_dev(ctx, ds, dd, dm, nx, ny, nz, sigma, exponent, truncate_ratio, normalize);
  });
}

// sigma = radius / (9 pi / 2)^(1/6) (filter3d.hpp:1908-1914) and, for a negative ratio, the window from the decay
// threshold: ratio = (-log thr)^(1/exponent) (bin/filter_mrc/filter3d_variants.hpp:663-669); host arithmetic
int visfd_hip_fluctuation_sigmas(const float radius[3], float exponent, float truncate_ratio, float truncate_threshold,
                                 float sigma_out[3], float* ratio_out) {
  VH_REQUIRE(radius && sigma_out && ratio_out, "null argument");
  const float r_over_sigma = (float)std::pow((9.0 / 2) * M_PI, 1.0 / 6);
  for (int d = 0; d < 3; d++) sigma_out[d] = radius[d] / r_over_sigma;
  float ratio = truncate_ratio;
  if (ratio < 0.0f) ratio = (float)std::pow((double)(-std::log(truncate_threshold)), 1.0 / (double)exponent);
  *ratio_out = ratio;
  return VISFD_HIP_OK;
}

// ---- a6 ------------------------------------------------------------------------------------
int visfd_hip_apply_dog_dev(visfd_hip_ctx* ctx, const float* src, float* dst, const float* mask,
                            int64_t nx, int64_t ny, int64_t nz, const float sa[3], const float sb[3],
                            const int hw[3], float* A, float* B) {
  VH_REQUIRE(ctx && src && dst && sa && sb && hw, "null argument");
  VH_HIP(hipSetDevice(ctx->device));
  VH_TRY(check_dims(nx, ny, nz));
  return dog_dev(ctx, src, dst, mask, nx, ny, nz, sa, sb, hw, 1.0f, A, B);
}

int visfd_hip_apply_dog(visfd_hip_ctx* ctx, const float* src, float* dst, const float* mask, int64_t nx, int64_t ny,
                        int64_t nz, const float sa[3], const float sb[3], const int hw[3], float* A, float* B) {
  return stage_filter(ctx, src, dst, mask, nx, ny, nz, false, [&](const float* ds, float* dd, const float* dm) {
    return visfd_hip_apply_dog_dev(ctx, ds, dd, dm, nx, ny, nz, sa, sb, hw, A, B);
  });
}

// ---- a7 ------------------------------------------------------------------------------------
int visfd_hip_apply_log_dev(visfd_hip_ctx* ctx, const float* src, float* dst, const float* mask,
                            int64_t nx, int64_t ny, int64_t nz, const float sigma[3], float delta,
                            float ratio, float* A, float* B) {
  VH_REQUIRE(ctx && src && dst && sigma, "null argument");
  VH_HIP(hipSetDevice(ctx->device));
  VH_TRY(check_dims(nx, ny, nz));
  return log_dev(ctx, src, dst, mask, nx, ny, nz, sigma, delta, ratio, A, B);
}

int visfd_hip_apply_log(visfd_hip_ctx* ctx, const float* src, float* dst, const float* mask, int64_t nx, int64_t ny,
                        int64_t nz, const float sigma[3], float delta, float ratio, float* A, float* B) {
  return stage_filter(ctx, src, dst, mask, nx, ny, nz, false, [&](const float* ds, float* dd, const float* dm) {
    return visfd_hip_apply_log_dev(ctx, ds, dd, dm, nx, ny, nz, sigma, delta, ratio, A, B);
  });
}

// ---- a8: the blob detector itself is in blob_job.hip; the host arithmetic around it -----------------------------
int visfd_hip_blob_diameters_to_sigmas(const float* d, int n, float* s) {
  VH_REQUIRE(n >= 0 && (n == 0 || (d && s)), "bad argument");   // empty lists have no storage
  for (int i = 0; i < n; i++) s[i] = (float)(d[i] / (2.0 * std::sqrt(3.0)));  // feature.hpp:475
  return VISFD_HIP_OK;
}
int visfd_hip_blob_sigmas_to_diameters(const float* s, int n, float* d) {
  VH_REQUIRE(n >= 0 && (n == 0 || (d && s)), "bad argument");
  for (int i = 0; i < n; i++) d[i] = (float)(s[i] * 2.0 * std::sqrt(3.0));  // feature.hpp:504
  return VISFD_HIP_OK;
}

// ---- a9 ------------------------------------------------------------------------------------
int visfd_hip_calc_hessian_dev(visfd_hip_ctx* ctx, const float* src, float* grad, float* hess,
                               const float* mask, int64_t nx, int64_t ny, int64_t nz, float sigma,
                               float ratio) {
  VH_REQUIRE(ctx, "null context");
  VH_HIP(hipSetDevice(ctx->device));
  return calc_hessian_dev(ctx, src, grad, hess, mask, nx, ny, nz, sigma, ratio);
}

int visfd_hip_calc_hessian(visfd_hip_ctx* ctx, const float* src, float* grad, float* hess, const float* mask,
                           int64_t nx, int64_t ny, int64_t nz, float sigma, float ratio) {
  VH_REQUIRE(ctx && src, "null argument");
  VH_HIP(hipSetDevice(ctx->device));
  VH_TRY(check_dims(nx, ny, nz));
  const Stage st = {ctx, (size_t)(nx * ny * nz)};
  float *ds, *dm, *dg = nullptr, *dh = nullptr, *aos = nullptr;
  VH_TRY(st.up(WS_H2D_0, src, &ds));
  VH_TRY(st.up(WS_H2D_1, mask, &dm));
  if (grad) VH_TRY(st.out(WS_H2D_2, &dg, 3));
  if (hess) VH_TRY(st.out(WS_H2D_3, &dh, 6));
  VH_TRY(st.out(WS_H2D_4, &aos, 6));
  VH_TRY(calc_hessian_dev(ctx, ds, dg, dh, dm, nx, ny, nz, sigma, ratio));
  // interleave on the device; voxels with mask==0 keep the caller's values
  if (grad) VH_TRY(st.down_interleaved(grad, dg, aos, 3, dm, true));
  if (hess) VH_TRY(st.down_interleaved(hess, dh, aos, 6, dm, true));
  return VISFD_HIP_OK;
}

// ---- a10 -----------------------------------------------------------------------------------
int visfd_hip_diagonalize_flat_sym3_dev(visfd_hip_ctx* ctx, const float* m6, float* out6, int64_t n,
                                        int order) {
  VH_REQUIRE(ctx && m6 && out6 && n >= 0, "bad argument");
  VH_REQUIRE(order == 0 || order == 1, "unsupported eigenvalue order");
  VH_HIP(hipSetDevice(ctx->device));
  if (n == 0) return VISFD_HIP_OK;
  return dev_diagonalize(ctx, m6, out6, n, order);
}

int visfd_hip_diagonalize_flat_sym3(visfd_hip_ctx* ctx, const float* m6, float* out6, int64_t n, int order) {
  VH_REQUIRE(ctx && m6 && out6 && n >= 0, "bad argument");
  VH_REQUIRE(order == 0 || order == 1, "unsupported eigenvalue order");
  VH_HIP(hipSetDevice(ctx->device));
  if (n == 0) return VISFD_HIP_OK;
  const Stage st = {ctx, (size_t)n};
  float *aos, *pin, *pout;
  VH_TRY(st.up_planar(WS_H2D_0, WS_H2D_1, m6, 6, &pin, &aos));
  VH_TRY(st.out(WS_H2D_2, &pout, 6));
  VH_TRY(dev_diagonalize(ctx, pin, pout, n, order));
  return st.down_interleaved(out6, pout, aos, 6, nullptr, false);
}

// ---- a12 (saliency) --------------------------------------------------------------------------
int visfd_hip_hessian_saliency_dev(visfd_hip_ctx* ctx, const float* hess, const float* mask, int64_t nvox,
                                   int order, float* sal, float* dir) {
  VH_REQUIRE(ctx && hess && sal && dir && nvox > 0, "bad argument");
  VH_REQUIRE(order == 0 || order == 1, "unsupported eigenvalue order");
  VH_HIP(hipSetDevice(ctx->device));
  return dev_hessian_saliency(ctx, hess, mask, nvox, order, sal, dir);
}

int visfd_hip_hessian_saliency(visfd_hip_ctx* ctx, const float* hess, const float* mask, int64_t nvox, int order,
                               float* sal, float* dir) {
  VH_REQUIRE(ctx && hess && sal && dir && nvox > 0, "bad argument");
  VH_REQUIRE(order == 0 || order == 1, "unsupported eigenvalue order");
  VH_HIP(hipSetDevice(ctx->device));
  const Stage st = {ctx, (size_t)nvox};
  float *aos, *ph, *dm, *dsal, *pdir;
  VH_TRY(st.up_planar(WS_H2D_0, WS_H2D_2, hess, 6, &ph, &aos));
  VH_TRY(st.up(WS_H2D_1, mask, &dm));
  VH_TRY(st.out(WS_H2D_3, &dsal));
  VH_TRY(st.out(WS_H2D_4, &pdir, 3));
  VH_TRY(dev_hessian_saliency(ctx, ph, dm, nvox, order, dsal, pdir));
  VH_TRY(st.down(sal, dsal));
  // direction: only voxels with mask != 0 are written (handlers.cpp:1650-1651,1738-1740)
  return st.down_interleaved(dir, pdir, aos, 3, dm, true);
}

int visfd_hip_ridge_saliency_dev(visfd_hip_ctx* ctx, const float* src, const float* mask, int64_t nx, int64_t ny,
                                 int64_t nz, float sigma, float ratio, int order, float* sal, float* dir) {
  VH_REQUIRE(ctx && src && sal && dir, "null argument");
  VH_REQUIRE(order == 0 || order == 1, "unsupported eigenvalue order");
  VH_HIP(hipSetDevice(ctx->device));
  VH_TRY(check_dims(nx, ny, nz));
  float* S = nullptr;
  VH_TRY(gauss_iso_dev(ctx, src, nullptr, mask, nx, ny, nz, sigma, ratio, true, "filter halfwidth", &S));
  return dev_ridge_saliency_fused(ctx, S, mask, nx, ny, nz, sigma, order, sal, dir);
}

// The same in two steps for callers that threshold in between (HandleTV does: handlers.cpp:1751-1797): scores for
// every voxel (the smoothed volume is handed back), then directions of the voxels whose score survived.
int visfd_hip_ridge_scores_bg_dev(visfd_hip_ctx* ctx, const float* src, const float* mask, int64_t nx, int64_t ny,
                                  int64_t nz, float sigma, float ratio, int order, const float* background, float* sal,
                                  float* smoothed) {
  VH_REQUIRE(ctx && src && sal && smoothed, "null argument");
  VH_REQUIRE(smoothed != src && smoothed != sal, "the smoothed volume needs its own buffer");
  VH_REQUIRE(order == 0 || order == 1, "unsupported eigenvalue order");
  VH_HIP(hipSetDevice(ctx->device));
  VH_TRY(check_dims(nx, ny, nz));
  VH_TRY(gauss_iso_dev(ctx, src, smoothed, mask, nx, ny, nz, sigma, ratio, true, "filter halfwidth"));
  return dev_ridge_score(ctx, smoothed, mask, nx, ny, nz, sigma, order, sal, background ? src : nullptr, background);
}
int visfd_hip_ridge_scores_dev(visfd_hip_ctx* ctx, const float* src, const float* mask, int64_t nx, int64_t ny,
                               int64_t nz, float sigma, float ratio, int order, float* sal, float* smoothed) {
  return visfd_hip_ridge_scores_bg_dev(ctx, src, mask, nx, ny, nz, sigma, ratio, order, nullptr, sal, smoothed);
}
// the background of the peak-height factor: ApplyGauss(image, sigma_background, floor(sigma_background * ratio), mask,
// normalize) -- bin/filter_mrc/handlers.cpp:1577-1592
int visfd_hip_peak_background_dev(visfd_hip_ctx* ctx, const float* src, const float* mask, int64_t nx, int64_t ny,
                                  int64_t nz, float sigma_background, float ratio, int normalize, float* background) {
  VH_REQUIRE(ctx && src && background && background != src, "bad argument");
  VH_REQUIRE(sigma_background > 0.0f, "the background width must be positive");
  VH_HIP(hipSetDevice(ctx->device));
  VH_TRY(check_dims(nx, ny, nz));
  return gauss_iso_dev(ctx, src, background, mask, nx, ny, nz, sigma_background, ratio, normalize != 0,
                       "background filter halfwidth");
}

int visfd_hip_ridge_directions_dev(visfd_hip_ctx* ctx, const float* smoothed, int64_t nx, int64_t ny, int64_t nz,
                                   float sigma, int order, const float* sal, float* dir) {
  VH_REQUIRE(ctx && smoothed && sal && dir, "null argument");
  VH_REQUIRE(order == 0 || order == 1, "unsupported eigenvalue order");
  VH_HIP(hipSetDevice(ctx->device));
  VH_TRY(check_dims(nx, ny, nz));
  return dev_ridge_directions(ctx, smoothed, sal, nx, ny, nz, sigma, order, dir);
}

// Test aids: the two consumers of an uncut saliency volume on their own (tests/test_membrane_consumers_gpu.py).
// thr_dev: one float in device memory, or null for the kernels as they run on a cut volume.
int visfd_hip_debug_ridge_directions_thr_dev(visfd_hip_ctx* ctx, const float* smoothed, int64_t nx, int64_t ny, int64_t nz,
                                             float sigma, int order, const float* sal, const float* thr_dev, float* dir) {
  VH_REQUIRE(ctx && smoothed && sal && dir, "null argument");
  VH_REQUIRE(order == 0 || order == 1, "unsupported eigenvalue order");
  VH_HIP(hipSetDevice(ctx->device));
  VH_TRY(check_dims(nx, ny, nz));
  return dev_ridge_directions(ctx, smoothed, sal, nx, ny, nz, sigma, order, dir, thr_dev);
}
// The sender lists of the whole volume (tv_list.hip) for windows of half-width h, copied to HOST arrays: rows
// (nz (ny + 1) ceil(nx / 16) words), entries (4 floats each) and positions; *nrows and *total say how many there are, and
// nothing is copied into an array that is too small.
int visfd_hip_debug_tv_lists_dev(visfd_hip_ctx* ctx, const float* sal, const float* dir, const float* thr_dev, int64_t nx,
                                 int64_t ny, int64_t nz, int h, int mode, int fold, uint32_t* rows, int64_t rows_cap, float* ent,
                                 uint32_t* pos, int64_t ent_cap, int64_t* nrows, int64_t* total, uint32_t* flags) {
  VH_REQUIRE(ctx && sal && dir && nrows && total && flags, "null argument");
  VH_REQUIRE(h >= 1 && h <= 40 && mode >= 0 && mode <= 2, "bad list parameters");
  VH_HIP(hipSetDevice(ctx->device));
  VH_TRY(check_dims(nx, ny, nz));
  VH_TRY(check_dims32(nx, ny, nz));
  VH_REQUIRE(nx <= TV_LIST_MAX_NX && ny < (1 << 24), "volume too wide for the lists");
  unsigned* counter = nullptr;
  VH_TRY(ws(ctx, WS_COUNTER, 16, &counter));
  TvListPlan plan;
  int rc = tv_list_count(ctx, sal, thr_dev, nullptr, nx, ny, nz, 0, nz, h, mode, counter,
                         reinterpret_cast<unsigned long long*>(counter + 4), counter + 6, &plan);
  VH_REQUIRE(rc != TV_DECLINED, "the lists declined the volume");
  VH_TRY(rc);
  unsigned long long tot2[2] = {0, 0};
  VH_HIP(hipMemcpyAsync(tot2, counter + 4, sizeof(tot2), hipMemcpyDeviceToHost, ctx->stream));
  VH_HIP(hipStreamSynchronize(ctx->stream));
  TvSenderLists L;
  rc = tv_list_write(ctx, plan, sal, dir, nullptr, tot2[0], (unsigned)tot2[1], 0u, fold != 0, &L);
  VH_REQUIRE(rc != TV_DECLINED, "the lists declined the volume");
  VH_TRY(rc);
  *nrows = (int64_t)plan.g.nzl * (int64_t)(ny + 1) * (int64_t)plan.g.ntx;
  *total = (int64_t)L.total;
  *flags = L.flags;
  if (rows && rows_cap >= *nrows) VH_HIP(hipMemcpyAsync(rows, L.rows, sizeof(uint32_t) * (size_t)*nrows, hipMemcpyDeviceToHost, ctx->stream));
  if (ent && pos && ent_cap >= *total && *total > 0) {
    VH_HIP(hipMemcpyAsync(ent, L.ent, sizeof(float) * 4 * (size_t)*total, hipMemcpyDeviceToHost, ctx->stream));
    VH_HIP(hipMemcpyAsync(pos, L.pos, sizeof(uint32_t) * (size_t)*total, hipMemcpyDeviceToHost, ctx->stream));
  }
  VH_HIP(hipStreamSynchronize(ctx->stream));
  return VISFD_HIP_OK;
}

// ---- a12 (threshold) -------------------------------------------------------------------------
int visfd_hip_threshold_fraction_dev(visfd_hip_ctx* ctx, float* sal, const float* mask, int64_t nvox,
                                     float fraction, float* thr_out) {
  VH_REQUIRE(ctx && sal && nvox > 0, "bad argument");
  VH_REQUIRE(fraction >= 0.0f && fraction <= 1.0f, "fraction must be in [0,1]");
  VH_HIP(hipSetDevice(ctx->device));
  return dev_threshold_fraction(ctx, sal, mask, nvox, fraction, thr_out);
}

int visfd_hip_threshold_fraction(visfd_hip_ctx* ctx, float* sal, const float* mask, int64_t nvox, float fraction,
                                 float* thr_out) {
  VH_REQUIRE(ctx && sal && nvox > 0, "bad argument");
  VH_REQUIRE(fraction >= 0.0f && fraction <= 1.0f, "fraction must be in [0,1]");
  VH_HIP(hipSetDevice(ctx->device));
  const Stage st = {ctx, (size_t)nvox};
  float *ds, *dm;
  VH_TRY(st.up(WS_H2D_0, sal, &ds));
  VH_TRY(st.up(WS_H2D_1, mask, &dm));
  VH_TRY(dev_threshold_fraction(ctx, ds, dm, nvox, fraction, thr_out));
  return st.down(sal, ds);
}

int visfd_hip_select_histogram_dev(visfd_hip_ctx* ctx, const float* sal, const float* mask, int64_t nvox,
                                   int pass, uint32_t prefix, uint64_t* hist_host, uint64_t* n_unmasked) {
  VH_REQUIRE(ctx && sal && hist_host && nvox > 0, "bad argument");
  VH_REQUIRE(pass >= 0 && pass <= 2, "round must be 0, 1 or 2");
  VH_HIP(hipSetDevice(ctx->device));
  return dev_select_histogram(ctx, sal, mask, nvox, pass, prefix, hist_host, n_unmasked);
}

int visfd_hip_select_histogram_todev(visfd_hip_ctx* ctx, const float* sal, const float* mask, int64_t nvox, int pass,
                                     uint32_t prefix, uint64_t* hist) {
  VH_REQUIRE(ctx && sal && hist && nvox > 0, "bad argument");
  VH_REQUIRE(pass >= 0 && pass <= 2, "round must be 0, 1 or 2");
  VH_HIP(hipSetDevice(ctx->device));
  return dev_select_histogram_todev(ctx, sal, mask, nvox, pass, prefix, hist);
}

int visfd_hip_apply_threshold_dev(visfd_hip_ctx* ctx, float* sal, int64_t nvox, float thr) {
  VH_REQUIRE(ctx && sal && nvox > 0, "bad argument");
  VH_HIP(hipSetDevice(ctx->device));
  return dev_apply_threshold(ctx, sal, nvox, thr);
}

// ---- f4: binning ------------------------------------------------------------------------------
int visfd_hip_bin_array3d_dev(visfd_hip_ctx* ctx, const float* src, const int64_t size_src[3], float* dst,
                              const int64_t size_dst[3], const int* offset) {
  VH_REQUIRE(ctx && src && dst && size_src && size_dst, "null argument");
  VH_HIP(hipSetDevice(ctx->device));
  return dev_bin_array3d(ctx, src, size_src, dst, size_dst, offset);
}

int visfd_hip_unbin_array3d_dev(visfd_hip_ctx* ctx, const float* src, const int64_t size_src[3], float* dst,
                                const int64_t size_dst[3], const int* offset) {
  VH_REQUIRE(ctx && src && dst && size_src && size_dst, "null argument");
  VH_HIP(hipSetDevice(ctx->device));
  return dev_unbin_array3d(ctx, src, size_src, dst, size_dst, offset);
}

// both directions of the binning: the source up, the other size down
static int resample_host(visfd_hip_ctx* ctx, const float* src, const int64_t size_src[3], float* dst, const int64_t size_dst[3],
                         const int* offset, decltype(dev_bin_array3d)* run) {
  VH_REQUIRE(ctx && src && dst && size_src && size_dst, "null argument");
  VH_HIP(hipSetDevice(ctx->device));
  VH_TRY(check_dims(size_src[0], size_src[1], size_src[2]));
  VH_TRY(check_dims(size_dst[0], size_dst[1], size_dst[2]));
  const Stage in = {ctx, (size_t)(size_src[0] * size_src[1] * size_src[2])};
  const Stage res = {ctx, (size_t)(size_dst[0] * size_dst[1] * size_dst[2])};
  float *ds, *dd;
  VH_TRY(in.up(WS_H2D_0, src, &ds));
  VH_TRY(res.out(WS_H2D_2, &dd));
  VH_TRY(run(ctx, ds, size_src, dd, size_dst, offset));
  return res.down(dst, dd);
}

int visfd_hip_bin_array3d(visfd_hip_ctx* ctx, const float* src, const int64_t size_src[3], float* dst,
                          const int64_t size_dst[3], const int* offset) {
  return resample_host(ctx, src, size_src, dst, size_dst, offset, dev_bin_array3d);
}
int visfd_hip_unbin_array3d(visfd_hip_ctx* ctx, const float* src, const int64_t size_src[3], float* dst,
                            const int64_t size_dst[3], const int* offset) {
  return resample_host(ctx, src, size_src, dst, size_dst, offset, dev_unbin_array3d);
}

// ---- a13 + a14 -------------------------------------------------------------------------------
int visfd_hip_tv_tables(float sigma_tv, float cutoff, int* h_out, float* w, float* rhat) {
  const int h = host_tv_halfwidth(sigma_tv, cutoff);
  VH_REQUIRE(h >= 0, "negative window");
  if (h_out) *h_out = h;
  if (w) host_tv_tables(sigma_tv, h, w, rhat);
  return VISFD_HIP_OK;
}

int visfd_hip_tv_dense_stick_slab_dev(visfd_hip_ctx* ctx, const float* sal, const float* dir, float* ten,
                                      const float* mask_src, const float* mask_dst, int64_t nx,
                                      int64_t ny, int64_t nz_local, int64_t z_out0, int64_t z_out1,
                                      float sigma_tv, int exponent, float cutoff, int curves) {
  VH_REQUIRE(ctx && sal && dir && ten, "null argument");
  VH_HIP(hipSetDevice(ctx->device));
  return dev_tv_dense_stick(ctx, sal, dir, ten, mask_src, mask_dst, nx, ny, nz_local, z_out0, z_out1,
                            sigma_tv, exponent, cutoff, curves != 0);
}

int visfd_hip_tv_dense_stick_dev(visfd_hip_ctx* ctx, const float* sal, const float* dir, float* ten,
                                 const float* mask_src, const float* mask_dst, int64_t nx, int64_t ny,
                                 int64_t nz, float sigma_tv, int exponent, float cutoff, int curves) {
  return visfd_hip_tv_dense_stick_slab_dev(ctx, sal, dir, ten, mask_src, mask_dst, nx, ny, nz, 0, nz,
                                           sigma_tv, exponent, cutoff, curves);
}

int visfd_hip_tv_dense_stick(visfd_hip_ctx* ctx, const float* sal, const float* dir, float* ten, const float* mask_src,
                             const float* mask_dst, int64_t nx, int64_t ny, int64_t nz, float sigma_tv, int exponent,
                             float cutoff, int curves) {
  VH_REQUIRE(ctx && sal && dir && ten, "null argument");
  VH_HIP(hipSetDevice(ctx->device));
  VH_TRY(check_dims(nx, ny, nz));
  const Stage st = {ctx, (size_t)(nx * ny * nz)};
  float *dsal, *pdir, *pten, *aos6, *dms = nullptr, *dmd = nullptr;
  VH_TRY(st.up(WS_H2D_0, sal, &dsal));
  VH_TRY(st.up_planar(WS_H2D_1, WS_H2D_2, dir, 3, &pdir));
  VH_TRY(st.out(WS_H2D_3, &pten, 6));
  VH_TRY(st.up(WS_H2D_4, mask_src, &dms));
  if (mask_dst == mask_src) dmd = dms;
  else VH_TRY(st.up(WS_A, mask_dst, &dmd));
  VH_TRY(dev_tv_dense_stick(ctx, dsal, pdir, pten, dms, dmd, nx, ny, nz, 0, nz, sigma_tv, exponent, cutoff, curves != 0));
  // tensors of voxels with mask_dst == 0 keep the caller's values (no storage in the reference)
  VH_TRY(st.out(WS_B, &aos6, 6));
  return st.down_interleaved(ten, pten, aos6, 6, dmd, true);
}

// TVDenseStick's normalisation denominators (feature.hpp:1761-1822): den[voxel] = sum of w(j) * mask_src(sender) over
// the votes the voxel receives; voxels with mask_dst == 0 keep the caller's value
int visfd_hip_tv_weight_sum(visfd_hip_ctx* ctx, const float* sal, float* den, const float* mask_src,
                            const float* mask_dst, int64_t nx, int64_t ny, int64_t nz, float sigma_tv, float cutoff) {
  VH_REQUIRE(ctx && sal && den, "null argument");
  VH_HIP(hipSetDevice(ctx->device));
  VH_TRY(check_dims(nx, ny, nz));
  const Stage st = {ctx, (size_t)(nx * ny * nz)};
  float *dsal, *dden, *dms = nullptr, *dmd = nullptr;
  VH_TRY(st.up(WS_H2D_0, sal, &dsal));
  VH_TRY(st.up(WS_H2D_1, den, &dden));
  VH_TRY(st.up(WS_H2D_4, mask_src, &dms));
  if (mask_dst == mask_src) dmd = dms;
  else VH_TRY(st.up(WS_A, mask_dst, &dmd));
  VH_TRY(dev_tv_weight_sum(ctx, dsal, dden, dms, dmd, nx, ny, nz, sigma_tv, cutoff));
  return st.down(den, dden);
}

// ---- HandleTV compute section ------------------------------------------------------------------
// The stage behind the scores, queued in one go (option membrane_queue): the select's three
// histogram / pick pairs, the sender lists' count and scan, ONE copy of {threshold, flag, list total, list flags} to pinned
// memory with an event behind it, and the direction kernel, which needs only the threshold on the device -- then the one
// wait, with those directions still queued.  No threshold pass: directions and lists cut sal for themselves.
// Unmasked fraction cuts only (n is known, so a fraction that selects no voxel is refused before anything is queued).
// TV_DECLINED: the vote's first route is not a kernel of tv_box.hip that takes the request; at most a select has run.
static int membrane_queued(visfd_hip_ctx* ctx, i64 nx, i64 ny, i64 nz, float sigma, int order, float best_fraction, float sigma_tv,
                           int exponent, float cutoff, const float* smoothed, float* sal, float* ten, float* dir, bool zero_dir,
                           const float* peak_img, const float* peak_bg, float* thr_out) {
  hipStream_t st = ctx->stream;
  const i64 n = nx * ny * nz;
  VH_TRY(select_rank_check((uint64_t)n, best_fraction));
  if (!ctx->stage_pinned) VH_HIP(hipHostMalloc(&ctx->stage_pinned, sizeof(StageReadback)));
  if (!ctx->stage_event) VH_HIP(hipEventCreateWithFlags(&ctx->stage_event, hipEventDisableTiming));
  StageReadback* block = nullptr;
  VH_TRY(ws(ctx, WS_SELECT, 1, &block));
  VH_HIP(hipMemsetAsync(block, 0, sizeof(*block), st));
  VH_TRY(dev_select_queue(ctx, sal, nullptr, n, best_fraction, &block->sel));
  const float* const thr_dev = &block->sel.thr;
  TvStagePlan plan;
  VH_TRY(dev_tv_stage_count(ctx, sal, thr_dev, nullptr, nx, ny, nz, sigma_tv, exponent, cutoff, &block->list_total,
                            &block->list_flags, &plan));
  const StageReadback* const got = static_cast<const StageReadback*>(ctx->stage_pinned);
  VH_HIP(hipMemcpyAsync(ctx->stage_pinned, block, sizeof(*block), hipMemcpyDeviceToHost, st));
  VH_HIP(hipEventRecord(ctx->stage_event, st));
  if (zero_dir) VH_HIP(hipMemsetAsync(dir, 0, sizeof(float) * 3 * (size_t)n, st));
  VH_TRY(dev_ridge_directions(ctx, smoothed, sal, nx, ny, nz, sigma, order, dir, thr_dev));
  VH_HIP(hipEventSynchronize(ctx->stage_event));   // the stage's one wait: the directions are still queued behind it
  float thr = 0.0f;
  VH_TRY(select_result(got->sel, &thr));
  if (thr_out) *thr_out = thr;
  int rc = dev_tv_stage_vote(ctx, plan, got->list_total, got->list_flags, sal, dir, ten, nullptr, nx, ny, nz, exponent);
  if (rc == TV_DECLINED) {   // (what the lists' count saw is not for this kernel: the other routes read a cut sal)
    VH_TRY(dev_apply_threshold(ctx, sal, n, thr));
    rc = dev_tv_dense_stick(ctx, sal, dir, ten, nullptr, nullptr, nx, ny, nz, 0, nz, sigma_tv, exponent, cutoff, false);
  }
  VH_TRY(rc);
  return dev_tensor_saliency(ctx, ten, nullptr, n, order, sal, peak_img, peak_bg);
}

// HandleTV's compute section on the caller's device arrays.  bg: a volume for the background (read only if
// sigma_background > 0); zero_dir: `dir` receives zeros where the score did not survive, else those voxels keep what it held.
static int membrane_stage(visfd_hip_ctx* ctx, const float* src, const float* mask, i64 nx, i64 ny, i64 nz, float sigma, float ratio,
                          int order, float best_fraction, float threshold_abs, float sigma_tv, int exponent, float cutoff,
                          float sigma_background, int normalize_background, float* bg, float* smoothed, float* sal, float* ten,
                          float* dir, bool zero_dir, float* thr_out) {
  const i64 n = nx * ny * nz;
  // optional peak-height factor (`-membrane-background`): scores and post-vote scores are multiplied by image - background
  if (sigma_background > 0.0f)
    VH_TRY(visfd_hip_peak_background_dev(ctx, src, mask, nx, ny, nz, sigma_background, ratio, normalize_background, bg));
  else bg = nullptr;
  VH_TRY(visfd_hip_ridge_scores_bg_dev(ctx, src, mask, nx, ny, nz, sigma, ratio, order, bg, sal, smoothed));
  if (ctx->opt.membrane_queue && sigma_tv > 0.0f && best_fraction >= 0.0f && !mask) {
    const int rc = membrane_queued(ctx, nx, ny, nz, sigma, order, best_fraction, sigma_tv, exponent, cutoff, smoothed, sal, ten, dir,
                                   zero_dir, bg ? src : nullptr, bg, thr_out);
    if (rc != TV_DECLINED) return rc;
  }
  float thr = threshold_abs;
  if (best_fraction >= 0.0f) VH_TRY(dev_threshold_fraction(ctx, sal, mask, n, best_fraction, &thr));
  else VH_TRY(dev_apply_threshold(ctx, sal, n, thr));
  if (thr_out) *thr_out = thr;
  // directions only where the score survived: nothing else is read downstream
  if (zero_dir) VH_HIP(hipMemsetAsync(dir, 0, sizeof(float) * 3 * (size_t)n, ctx->stream));
  VH_TRY(dev_ridge_directions(ctx, smoothed, sal, nx, ny, nz, sigma, order, dir));
  if (sigma_tv > 0.0f) {
    VH_TRY(dev_tv_dense_stick(ctx, sal, dir, ten, mask, mask, nx, ny, nz, 0, nz, sigma_tv, exponent, cutoff, false));
    VH_TRY(dev_tensor_saliency(ctx, ten, mask, n, order, sal, bg ? src : nullptr, bg));
  }
  return VISFD_HIP_OK;
}

int visfd_hip_membrane_detect_bg_dev(visfd_hip_ctx* ctx, const float* src, const float* mask, int64_t nx,
                                     int64_t ny, int64_t nz, float sigma, float ratio, int order,
                                     float best_fraction, float threshold_abs, float sigma_tv, int exponent,
                                     float cutoff, float sigma_background, int normalize_background, float* sal, float* ten,
                                     float* dir, float* thr_out) {
  VH_REQUIRE(ctx && src && sal, "null argument");
  VH_REQUIRE(order == 0 || order == 1, "unsupported eigenvalue order");
  VH_REQUIRE(best_fraction <= 1.0f, "fraction must be <= 1");
  VH_HIP(hipSetDevice(ctx->device));
  VH_TRY(check_dims(nx, ny, nz));
  const i64 n = nx * ny * nz;
  float* d = dir;
  if (!d) VH_TRY(ws(ctx, WS_TVAUX, (size_t)(3 * n), &d));
  float *smoothed = nullptr, *bg = nullptr, *t = ten;
  VH_TRY(ws(ctx, WS_D, (size_t)n, &smoothed));
  if (sigma_background > 0.0f) VH_TRY(ws(ctx, WS_C, (size_t)n, &bg));
  if (!t && sigma_tv > 0.0f) VH_TRY(ws(ctx, WS_B, (size_t)(6 * n), &t));
  // (a caller-supplied `dir` receives zeros where the score did not survive)
  return membrane_stage(ctx, src, mask, nx, ny, nz, sigma, ratio, order, best_fraction, threshold_abs, sigma_tv, exponent, cutoff,
                        sigma_background, normalize_background, bg, smoothed, sal, t, d, dir != nullptr, thr_out);
}
// The same stage with every volume the caller's: `scratch` receives the smoothed image, `background` (nullable unless
// sigma_background > 0) the background, and voxels of `dir` whose score did not survive keep what they held.
int visfd_hip_membrane_stage_dev(visfd_hip_ctx* ctx, const float* src, const float* mask, int64_t nx, int64_t ny, int64_t nz,
                                 float sigma, float ratio, int order, float best_fraction, float sigma_tv, int exponent,
                                 float cutoff, float sigma_background, int normalize_background, float* background,
                                 float* scratch, float* sal, float* dir, float* ten, float* thr_out) {
  VH_REQUIRE(ctx && src && scratch && sal && dir && ten, "null argument");
  VH_REQUIRE(order == 0 || order == 1, "unsupported eigenvalue order");
  VH_REQUIRE(best_fraction >= 0.0f && best_fraction <= 1.0f, "fraction must be in [0,1]");
  VH_REQUIRE(sigma_tv > 0.0f, "the voting width must be positive");
  VH_REQUIRE(!(sigma_background > 0.0f) || background, "the background needs a volume");
  VH_HIP(hipSetDevice(ctx->device));
  VH_TRY(check_dims(nx, ny, nz));
  return membrane_stage(ctx, src, mask, nx, ny, nz, sigma, ratio, order, best_fraction, 0.0f, sigma_tv, exponent, cutoff,
                        sigma_background, normalize_background, background, scratch, sal, ten, dir, false, thr_out);
}
int visfd_hip_membrane_detect_dev(visfd_hip_ctx* ctx, const float* src, const float* mask, int64_t nx,
                                  int64_t ny, int64_t nz, float sigma, float ratio, int order,
                                  float best_fraction, float threshold_abs, float sigma_tv, int exponent,
                                  float cutoff, float* sal, float* ten, float* dir, float* thr_out) {
  return visfd_hip_membrane_detect_bg_dev(ctx, src, mask, nx, ny, nz, sigma, ratio, order, best_fraction, threshold_abs, sigma_tv,
                                          exponent, cutoff, 0.0f, 1, sal, ten, dir, thr_out);
}

int visfd_hip_membrane_detect_bg(visfd_hip_ctx* ctx, const float* src, const float* mask, int64_t nx, int64_t ny,
                                 int64_t nz, float sigma, float ratio, int order, float best_fraction,
                                 float threshold_abs, float sigma_tv, int exponent, float cutoff,
                                 float sigma_background, int normalize_background, float* sal, float* ten, float* dir,
                                 float* thr_out) {
  VH_REQUIRE(ctx && src && sal, "null argument");
  VH_HIP(hipSetDevice(ctx->device));
  VH_TRY(check_dims(nx, ny, nz));
  const Stage st = {ctx, (size_t)(nx * ny * nz)};
  float *ds, *dm, *dsal, *pdir, *pten = nullptr, *aos = nullptr;
  VH_TRY(st.up(WS_H2D_0, src, &ds));
  VH_TRY(st.up(WS_H2D_1, mask, &dm));
  VH_TRY(st.out(WS_H2D_2, &dsal));
  VH_TRY(st.out(WS_H2D_3, &pdir, 3));
  if (ten && sigma_tv > 0.0f) {
    VH_TRY(st.out(WS_H2D_4, &pten, 6));
    VH_HIP(hipMemsetAsync(pten, 0, sizeof(float) * 6 * st.n, ctx->stream));
  }
  VH_TRY(visfd_hip_membrane_detect_bg_dev(ctx, ds, dm, nx, ny, nz, sigma, ratio, order, best_fraction, threshold_abs, sigma_tv,
                                          exponent, cutoff, sigma_background, normalize_background, dsal, pten, pdir, thr_out));
  VH_TRY(st.down(sal, dsal));
  if ((ten && pten) || dir) VH_TRY(st.out(WS_A, &aos, 6));   // the interleaving buffer of both
  if (ten && pten) VH_TRY(st.down_interleaved(ten, pten, aos, 6, nullptr, false));
  if (dir) VH_TRY(st.down_interleaved(dir, pdir, aos, 3, nullptr, false));
  return VISFD_HIP_OK;
}
int visfd_hip_membrane_detect(visfd_hip_ctx* ctx, const float* src, const float* mask, int64_t nx, int64_t ny,
                              int64_t nz, float sigma, float ratio, int order, float best_fraction,
                              float threshold_abs, float sigma_tv, int exponent, float cutoff, float* sal,
                              float* ten, float* dir, float* thr_out) {
  return visfd_hip_membrane_detect_bg(ctx, src, mask, nx, ny, nz, sigma, ratio, order, best_fraction, threshold_abs, sigma_tv,
                                      exponent, cutoff, 0.0f, 1, sal, ten, dir, thr_out);
}

// ---- a15 -------------------------------------------------------------------------------------
int visfd_hip_tensor_saliency_bg_dev(visfd_hip_ctx* ctx, const float* ten, const float* mask, int64_t nvox,
                                     int order, const float* image, const float* background, float* sal) {
  VH_REQUIRE(ctx && ten && sal && nvox > 0, "bad argument");
  VH_REQUIRE((image == nullptr) == (background == nullptr), "image and background come as a pair");
  VH_REQUIRE(order == 0 || order == 1, "unsupported eigenvalue order");
  VH_HIP(hipSetDevice(ctx->device));
  return dev_tensor_saliency(ctx, ten, mask, nvox, order, sal, image, background);
}
int visfd_hip_tensor_saliency_dev(visfd_hip_ctx* ctx, const float* ten, const float* mask, int64_t nvox,
                                  int order, float* sal) {
  return visfd_hip_tensor_saliency_bg_dev(ctx, ten, mask, nvox, order, nullptr, nullptr, sal);
}

int visfd_hip_tensor_saliency(visfd_hip_ctx* ctx, const float* ten, const float* mask, int64_t nvox, int order,
                              float* sal) {
  VH_REQUIRE(ctx && ten && sal && nvox > 0, "bad argument");
  VH_REQUIRE(order == 0 || order == 1, "unsupported eigenvalue order");
  VH_HIP(hipSetDevice(ctx->device));
  const Stage st = {ctx, (size_t)nvox};
  float *pten, *dm, *dsal;
  VH_TRY(st.up_planar(WS_H2D_0, WS_H2D_1, ten, 6, &pten));
  VH_TRY(st.up(WS_H2D_2, mask, &dm));
  VH_TRY(st.up(WS_H2D_3, sal, &dsal));
  VH_TRY(dev_tensor_saliency(ctx, pten, dm, nvox, order, dsal));
  return st.down(sal, dsal);
}

// ---- m1: grayscale morphology (lib/visfd/morphology.hpp:134-597; the orchestration is in morph.hip) ---------------
int visfd_hip_morph_last_path(visfd_hip_ctx* ctx, int* path) {
  VH_REQUIRE(ctx && path, "null argument");
  *path = ctx->morph_last_path;
  return VISFD_HIP_OK;
}

int visfd_hip_sphere_structure(float radius, float radius_max, float bmax, int* dxyz, float* b, int64_t cap,
                               int64_t* n) {
  VH_REQUIRE(n && cap >= 0 && (cap == 0 || (dxyz && b)), "bad argument");
  VH_REQUIRE(std::isfinite(radius) && std::isfinite(radius_max) && std::isfinite(bmax),
             "sphere radii and bmax must be finite");
  VH_REQUIRE(std::ceil(std::max(radius, radius_max)) <= 128.0f, "sphere radius must be at most 128 voxels");
  *n = host_sphere_structure(radius, radius_max, bmax, dxyz, b, cap);
  if (cap > 0 && cap < *n) return fail(VISFD_HIP_ECAPACITY, "structuring element has more entries than cap");
  return VISFD_HIP_OK;
}

int visfd_hip_morph_sphere_dev(visfd_hip_ctx* ctx, const float* src, float* dst, const float* mask, int64_t nx,
                               int64_t ny, int64_t nz, int op, float radius, float radius_max, float bmax) {
  VH_TRY(face_check(ctx, src, dst, mask, nx, ny, nz, "morphology", "morphology", op, VISFD_HIP_MORPH_TOP_HAT_BLACK));
  // an image of at most two levels needs no element (csrc/morph_levels.hip): decided before one is built, at any radius
  bool levels = false;
  VH_TRY(morph_levels_try(ctx, src, dst, mask, nx, ny, nz, op, radius, radius_max, bmax, &levels));
  if (levels) return VISFD_HIP_OK;
  int64_t n = 0;
  VH_TRY(visfd_hip_sphere_structure(radius, radius_max, bmax, nullptr, nullptr, 0, &n));
  std::vector<int> dxyz((size_t)(3 * n + 3));
  std::vector<float> b((size_t)(n + 1));
  VH_TRY(visfd_hip_sphere_structure(radius, radius_max, bmax, dxyz.data(), b.data(), n + 1, &n));
  MorphElem el;
  VH_TRY(morph_put_table(ctx, dxyz.data(), b.data(), n, &el));
  return morph_run(ctx, src, dst, mask, nx, ny, nz, op, el);
}

// the host faces: dst goes up too (masked voxels keep their values, the top-hats read it)
int visfd_hip_morph_sphere(visfd_hip_ctx* ctx, const float* src, float* dst, const float* mask, int64_t nx, int64_t ny,
                           int64_t nz, int op, float radius, float radius_max, float bmax) {
  VH_TRY(face_check(ctx, src, dst, mask, nx, ny, nz, "morphology", "morphology", op, VISFD_HIP_MORPH_TOP_HAT_BLACK));
  return stage_filter(ctx, src, dst, mask, nx, ny, nz, true, [&](const float* ds, float* dd, const float* dm) {
    return visfd_hip_morph_sphere_dev(ctx, ds, dd, dm, nx, ny, nz, op, radius, radius_max, bmax);
  });
}

int visfd_hip_morph_table_dev(visfd_hip_ctx* ctx, const float* src, float* dst, const float* mask, int64_t nx,
                              int64_t ny, int64_t nz, int op, const int* dxyz, const float* b, int64_t n) {
  VH_TRY(face_check(ctx, src, dst, mask, nx, ny, nz, "morphology", "morphology", op, VISFD_HIP_MORPH_ERODE));
  MorphElem el;
  VH_TRY(morph_put_table(ctx, dxyz, b, n, &el));
  return morph_run(ctx, src, dst, mask, nx, ny, nz, op, el);
}

int visfd_hip_morph_table(visfd_hip_ctx* ctx, const float* src, float* dst, const float* mask, int64_t nx, int64_t ny,
                          int64_t nz, int op, const int* dxyz, const float* b, int64_t n) {
  VH_TRY(face_check(ctx, src, dst, mask, nx, ny, nz, "morphology", "morphology", op, VISFD_HIP_MORPH_ERODE));
  return stage_filter(ctx, src, dst, mask, nx, ny, nz, true, [&](const float* ds, float* dd, const float* dm) {
    return visfd_hip_morph_table_dev(ctx, ds, dd, dm, nx, ny, nz, op, dxyz, b, n);
  });
}

// ---- m1b: the median filter (lib/visfd/filter3d.hpp:1577-1674; kernels and dispatch in median.hip) ----------------
int visfd_hip_median_last_path(visfd_hip_ctx* ctx, int* path) {
  VH_REQUIRE(ctx && path, "null argument");
  *path = ctx->median_last_path;
  return VISFD_HIP_OK;
}

int visfd_hip_median_footprint(float radius, int* dxyz, int64_t cap, int64_t* n) {
  VH_REQUIRE(n && cap >= 0 && (cap == 0 || dxyz), "bad argument");
  VH_REQUIRE(radius >= 0.0f, "the median radius must be a nonnegative number");
  VH_REQUIRE(std::ceil(radius) <= (float)VISFD_HIP_MEDIAN_MAX_RADIUS, "the median radius must be at most 16 voxels");
  const int Ri = (int)std::ceil(radius);
  int64_t m = 0;
  for (int iz = -Ri; iz <= Ri; iz++)
    for (int iy = -Ri; iy <= Ri; iy++)
      for (int ix = -Ri; ix <= Ri; ix++) {
        const float r = (float)std::sqrt((double)(ix * ix + iy * iy + iz * iz));   // filter3d.hpp:1657
        if (!(r <= radius)) continue;
        if (m < cap) {
          dxyz[3 * m] = ix;
          dxyz[3 * m + 1] = iy;
          dxyz[3 * m + 2] = iz;
        }
        m++;
      }
  *n = m;
  if (cap > 0 && cap < m) return fail(VISFD_HIP_ECAPACITY, "median footprint has more entries than cap");
  return VISFD_HIP_OK;
}

int visfd_hip_median_table_dev(visfd_hip_ctx* ctx, const float* src, float* dst, const float* mask, int64_t nx,
                               int64_t ny, int64_t nz, const int* dxyz, int64_t n) {
  VH_TRY(face_check(ctx, src, dst, mask, nx, ny, nz, "the median filter", "median"));
  MedianTab mt;
  VH_TRY(median_put_table(ctx, dxyz, n, &mt));
  return median_run(ctx, src, dst, mask, nx, ny, nz, mt);
}

int visfd_hip_median_sphere_dev(visfd_hip_ctx* ctx, const float* src, float* dst, const float* mask, int64_t nx,
                                int64_t ny, int64_t nz, float radius) {
  int64_t n = 0;   // the arrays are checked by the table entry
  VH_TRY(visfd_hip_median_footprint(radius, nullptr, 0, &n));
  std::vector<int> dxyz((size_t)(3 * n));
  VH_TRY(visfd_hip_median_footprint(radius, dxyz.data(), n, &n));
  return visfd_hip_median_table_dev(ctx, src, dst, mask, nx, ny, nz, dxyz.data(), n);
}

// the host faces: dst goes up too (masked voxels keep their values)
int visfd_hip_median_sphere(visfd_hip_ctx* ctx, const float* src, float* dst, const float* mask, int64_t nx, int64_t ny,
                            int64_t nz, float radius) {
  VH_TRY(face_check(ctx, src, dst, mask, nx, ny, nz, "the median filter", "median"));
  int64_t n = 0;
  VH_TRY(visfd_hip_median_footprint(radius, nullptr, 0, &n));   // a bad radius is refused before anything is staged
  return stage_filter(ctx, src, dst, mask, nx, ny, nz, true, [&](const float* ds, float* dd, const float* dm) {
    return visfd_hip_median_sphere_dev(ctx, ds, dd, dm, nx, ny, nz, radius);
  });
}

int visfd_hip_median_table(visfd_hip_ctx* ctx, const float* src, float* dst, const float* mask, int64_t nx, int64_t ny,
                           int64_t nz, const int* dxyz, int64_t n) {
  VH_TRY(face_check(ctx, src, dst, mask, nx, ny, nz, "the median filter", "median"));
  return stage_filter(ctx, src, dst, mask, nx, ny, nz, true, [&](const float* ds, float* dd, const float* dm) {
    return visfd_hip_median_table_dev(ctx, ds, dd, dm, nx, ny, nz, dxyz, n);
  });
}

// ---- m2: local minima and maxima with plateaus (csrc/extrema.hip) ---------------------------------
int visfd_hip_find_extrema_dev(visfd_hip_ctx* ctx, const float* src, const float* mask, int64_t nx, int64_t ny, int64_t nz,
                               int find_minima, int find_maxima, float minima_threshold, float maxima_threshold,
                               int connectivity, int allow_borders, int64_t* min_index, float* min_score,
                               int64_t* min_nvoxels, int64_t min_cap, int64_t* n_min, int64_t* max_index, float* max_score,
                               int64_t* max_nvoxels, int64_t max_cap, int64_t* n_max, int32_t* labels) {
  const ExtremaArgs a = {src, mask, nx, ny, nz, find_minima, find_maxima, minima_threshold, maxima_threshold, connectivity,
                         allow_borders, min_index, min_nvoxels, max_index, max_nvoxels, min_score, max_score, min_cap,
                         max_cap, n_min, n_max, labels};
  VH_TRY(extrema_check_args(ctx, a));
  return dev_find_extrema(ctx, a);
}

int visfd_hip_find_extrema(visfd_hip_ctx* ctx, const float* src, const float* mask, int64_t nx, int64_t ny, int64_t nz,
                           int find_minima, int find_maxima, float minima_threshold, float maxima_threshold,
                           int connectivity, int allow_borders, int64_t* min_index, float* min_score,
                           int64_t* min_nvoxels, int64_t min_cap, int64_t* n_min, int64_t* max_index, float* max_score,
                           int64_t* max_nvoxels, int64_t max_cap, int64_t* n_max, int32_t* labels) {
  ExtremaArgs a = {src, mask, nx, ny, nz, find_minima, find_maxima, minima_threshold, maxima_threshold, connectivity,
                   allow_borders, min_index, min_nvoxels, max_index, max_nvoxels, min_score, max_score, min_cap, max_cap,
                   n_min, n_max, labels};
  VH_TRY(extrema_check_args(ctx, a));
  VH_HIP(hipSetDevice(ctx->device));
  const Stage st = {ctx, (size_t)(nx * ny * nz)};
  float *ds, *dm, *dl = nullptr;
  VH_TRY(st.up(WS_H2D_0, src, &ds));
  VH_TRY(st.up(WS_H2D_1, mask, &dm));
  // the labels (32-bit words like the floats) go up when there is a mask: voxels with mask == 0 keep their values
  if (labels) VH_TRY(st.out(WS_H2D_2, &dl, 1, mask ? reinterpret_cast<const float*>(labels) : nullptr));
  a.src = ds;
  a.mask = dm;
  a.labels = reinterpret_cast<int32_t*>(dl);
  VH_TRY(dev_find_extrema(ctx, a));
  if (labels) VH_TRY(st.down(reinterpret_cast<float*>(labels), dl));
  return VISFD_HIP_OK;
}

}  // extern "C"
