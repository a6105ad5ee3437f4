// tv.hip -- dense stick tensor voting (reference lib/visfd/feature.hpp:1914-2037, :2217-2384).
//
// Receiver-centric gather, one thread per receiver voxel, so that each receiver accumulates its
// votes in exactly the reference's order (jz, jy, jx ascending over the window, sender = r - j):
//   u   = (rhat_x*n_x + rhat_y*n_y) + rhat_z*n_z          rhat = unit vector sender -> receiver
//   ang = 1 - u*u  (surfaces)   |   u*u (curves)
//   dec = ang (exponent 2) | ang*ang (exponent 4) | pow(ang, exponent/2) otherwise
//   m   = 2u*rhat - n  (surfaces)  |  n - 2u*rhat (curves)
//   T_ab += (((sal * (w*mask_src)) * dec) * m_a) * m_b      for a <= b
// all in float with separate multiplies and adds (-ffp-contract=off).
//
// Device layout: direction is 3 planes, tensor is 6 planes (xx,yy,zz,xy,yz,xz), each nvox floats.
#include <vector>

#include "tv_common.hpp"

namespace vh {

namespace {

constexpr int BLOCK = 256;

struct TvParams {
  int nx, ny, nz;        // local array extent
  int z_out0, z_out1;    // receiver planes [z_out0, z_out1)
  int h;
  int exponent;
  int curves;
  int weights_only;      // 1: no tensors -- the sum of the vote weights of every receiver into ONE plane (feature.hpp:2376-2377)
};

__device__ __forceinline__ float decay_of(float ang, int exponent) {
  if (exponent == 2) return ang;
  if (exponent == 4) return ang * ang;
  return (float)pow((double)ang, 0.5 * (double)exponent);
}

// One vote, accumulated into T[6] (xx,yy,zz,xy,yz,xz).
__device__ __forceinline__ void add_vote(float T[6], float sal, float fv, float r0, float r1, float r2,
                                         float n0, float n1, float n2, int exponent, int curves) {
  const float u = (r0 * n0 + r1 * n1) + r2 * n2;
  const float ux2 = u * 2.0f;
  const float u2 = u * u;
  const float c2 = 1.0f - u2;
  const float ang = curves ? u2 : c2;
  const float dec = decay_of(ang, exponent);
  float m0, m1, m2;
  if (curves) {
    m0 = n0 - ux2 * r0; m1 = n1 - ux2 * r1; m2 = n2 - ux2 * r2;
  } else {
    m0 = ux2 * r0 - n0; m1 = ux2 * r1 - n1; m2 = ux2 * r2 - n2;
  }
  const float base = (sal * fv) * dec;
  const float b0 = base * m0, b1 = base * m1, b2 = base * m2;
  T[0] = T[0] + b0 * m0;
  T[3] = T[3] + b0 * m1;
  T[5] = T[5] + b0 * m2;
  T[1] = T[1] + b1 * m1;
  T[4] = T[4] + b1 * m2;
  T[2] = T[2] + b2 * m2;
}

// ---------------------------------------------------------------------------------------------
// Baseline kernel: every thread walks the whole window.  Lanes of a wave are consecutive x, so
// the tap (jz,jy,jx) -- and with it w and rhat -- is wave-uniform; zero-weight taps are skipped
// for the whole wave.  Used for windows whose lookup table does not fit the tiled kernel and as
// an in-library cross-check (tests compare both against the CPU oracle).
// ---------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(BLOCK)
tv_dense_kernel(const float* __restrict__ sal, const float* __restrict__ dir,
                float* __restrict__ ten, const float* __restrict__ mask_src,
                const float* __restrict__ mask_dst, const float4* __restrict__ table /* w,rx,ry,rz */,
                TvParams p) {
  const int xblocks = (p.nx + BLOCK - 1) / BLOCK;
  unsigned b = blockIdx.x;
  const int bx = b % xblocks;
  b /= xblocks;
  const int iy = b % p.ny;
  const int iz = p.z_out0 + (int)(b / p.ny);
  const int ix = bx * BLOCK + (int)threadIdx.x;
  if (ix >= p.nx) return;
  const i64 plane = (i64)p.nx * p.ny;
  const i64 nvox = plane * p.nz;
  const i64 c = (i64)iz * plane + (i64)iy * p.nx + ix;
  if (mask_dst && mask_dst[c] == 0.0f) return;
  float T[6] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
  const int h = p.h, n = 2 * h + 1;
  for (int jz = -h; jz <= h; jz++) {
    const int sz = iz - jz;
    if (sz < 0 || sz >= p.nz) continue;
    for (int jy = -h; jy <= h; jy++) {
      const int sy = iy - jy;
      if (sy < 0 || sy >= p.ny) continue;
      const i64 row = (i64)sz * plane + (i64)sy * p.nx;
      const float4* trow = table + ((i64)(jz + h) * n + (jy + h)) * n + h;
      for (int jx = -h; jx <= h; jx++) {
        const float4 t = trow[jx];
        if (t.x == 0.0f) continue;  // wave-uniform
        const int sx = ix - jx;
        if (sx < 0 || sx >= p.nx) continue;
        const i64 s = row + sx;
        float fv = t.x;
        if (mask_src) {
          const float mv = mask_src[s];
          if (mv == 0.0f) continue;
          fv = fv * mv;
        }
        const float sv = sal[s];
        if (sv == 0.0f) continue;
        if (fv == 0.0f) continue;
        if (p.weights_only) { T[0] = T[0] + fv; continue; }     // "denominator += filter_val"
        add_vote(T, sv, fv, t.y, t.z, t.w, dir[s], dir[nvox + s], dir[2 * nvox + s], p.exponent,
                 p.curves);
      }
    }
  }
  if (p.weights_only) { ten[c] = T[0]; return; }
#pragma unroll
  for (int k = 0; k < 6; k++) ten[k * nvox + c] = T[k];
}

}  // namespace

// The vote tables of (sigma_tv, cutoff) on the device: float4 {w, rhat_x, rhat_y, rhat_z} per offset j in z, y, x order
// (filter3d.hpp:563-578, feature.hpp:2470-2478), in the five layouts of tv_common.hpp (TvTableLayout).  Built on the host
// once and kept in slot WS_TVTAB under the key (h, sigma_tv, cutoff): a launch with the same parameters queues no copy and
// never waits for the stream.
static int tv_table_device(visfd_hip_ctx* ctx, float sigma_tv, float cutoff, int h, TvTables* out) {
  const TvTableLayout l = tv_table_layout(h);
  const struct { int h; float sigma_tv, cutoff; } key = {h, sigma_tv, cutoff};
  if (!ws_holds(ctx, WS_TVTAB, &key, sizeof key)) {
    const size_t n = 2 * (size_t)h + 1, m = n * n * n;
    std::vector<float> w(m), rh(3 * m);
    host_tv_tables(sigma_tv, h, w.data(), rh.data());
    const size_t sp = (size_t)tv_padded_row(h), spb = (size_t)tv_box_row(h), nslb = (size_t)tv_box_slice(h);
    std::vector<float4> tab(l.total, make_float4(0.0f, 0.0f, 0.0f, 0.0f));
    const float rt2 = 1.41421356237309504880f;
    for (size_t k = 0; k < m; k++) {
      tab[l.packed + k] = make_float4(w[k], rh[3 * k], rh[3 * k + 1], rh[3 * k + 2]);
      tab[l.padded + (k / n) * sp + (k % n)] = tab[l.packed + k];
      const size_t kb = (k / (n * n)) * nslb + 4 + ((k / n) % n + 3) * spb + (k % n);
      tab[l.box_tol + kb] = make_float4(w[k], rt2 * rh[3 * k], rt2 * rh[3 * k + 1], rt2 * rh[3 * k + 2]);
      tab[l.box_exact + kb] = tab[l.packed + k];
      // (the square root of the float weight, rounded once; the pad entries stay exactly 0)
      tab[l.box_tol_sq + kb] = tab[l.box_tol + kb];
      tab[l.box_tol_sq + kb].x = (float)sqrt((double)w[k]);
    }
    VH_TRY(ws_put(ctx, WS_TVTAB, &key, sizeof key, tab.data(), sizeof(float4) * l.total));
  }
  const float4* const dtab = static_cast<const float4*>(ctx->slot_ptr[WS_TVTAB]);
  *out = {dtab + l.packed, dtab + l.padded, dtab + l.box_tol, dtab + l.box_exact, dtab + l.box_tol_sq, h};
  return VISFD_HIP_OK;
}

namespace {

struct TvRequest {
  const float *sal, *dir;
  float* out;              // six tensor planes, or ONE plane of weight sums (weights_only)
  const float *mask_src, *mask_dst;
  i64 nx, ny, nz;
  i64 z_out0, z_out1;      // receiver planes [z_out0, z_out1)
  int exponent;
  bool curves, weights_only;
};

enum class TvRoute { BoxTol, BoxExact, Tiled, Baseline };

// The routes a request may take under the context's options, in the order they are tried; returns their number.
int tv_routes(const visfd_hip_options& opt, const TvRequest& rq, TvRoute routes[4]) {
  int n = 0;
  const bool box = !opt.tv_dense && !rq.curves && !rq.weights_only;
  // tolerance mode (option tv_fma): fused multiply-adds, sub-patches with two sender streams, box-tested hit lists
  // (tv_box.hip); windows and vote forms it does not take fall through to the exact kernels
  if (box && opt.tv_fma) routes[n++] = TvRoute::BoxTol;
  // exact arithmetic in the same kernel structure (surfaces, exponent 2 or 4, source mask absent or binary, finite
  // saliencies; option tv_exact_tiled = 1 keeps the round-2 kernel)
  if (box && !opt.tv_exact_tiled) routes[n++] = TvRoute::BoxExact;
  if (!opt.tv_dense) routes[n++] = TvRoute::Tiled;
  // windows the tiled kernel declines (h = 0, h > 40, slices beyond LDS) and the tv_dense option: the baseline kernel, same
  // order of accumulation; it takes everything
  routes[n++] = TvRoute::Baseline;
  return n;
}

int tv_baseline(visfd_hip_ctx* ctx, const TvRequest& rq, const TvTables& tab) {
  TvParams p;
  p.nx = (int)rq.nx; p.ny = (int)rq.ny; p.nz = (int)rq.nz;
  p.z_out0 = (int)rq.z_out0; p.z_out1 = (int)rq.z_out1;
  p.h = tab.h; p.exponent = rq.exponent; p.curves = rq.curves ? 1 : 0; p.weights_only = rq.weights_only ? 1 : 0;
  const i64 nb = ((rq.nx + BLOCK - 1) / BLOCK) * rq.ny * (rq.z_out1 - rq.z_out0);
  if (nb > 0x7fffffffLL) return fail(VISFD_HIP_EINVAL, "volume too large for one launch");
  tv_dense_kernel<<<dim3((unsigned)nb), dim3(BLOCK), 0, ctx->stream>>>(rq.sal, rq.dir, rq.out, rq.mask_src, rq.mask_dst,
                                                                       tab.packed, p);
  VH_HIP(hipGetLastError());
  return VISFD_HIP_OK;
}

int tv_dispatch(visfd_hip_ctx* ctx, const TvRequest& rq, float sigma_tv, float cutoff) {
  const int h = host_tv_halfwidth(sigma_tv, cutoff);
  VH_REQUIRE(h >= 0 && h <= 255, "tensor-voting window halfwidth out of range");
  TvTables tab;
  VH_TRY(tv_table_device(ctx, sigma_tv, cutoff, h, &tab));
  TvRoute routes[4];
  const int nroutes = tv_routes(ctx->opt, rq, routes);
  int rc = TV_DECLINED;
  for (int i = 0; i < nroutes && rc == TV_DECLINED; i++) {
    switch (routes[i]) {
      case TvRoute::BoxTol:
      case TvRoute::BoxExact: {
        const bool exact = routes[i] == TvRoute::BoxExact;
        rc = dev_tv_box(ctx, rq.sal, rq.dir, rq.out, rq.mask_src, rq.mask_dst, rq.nx, rq.ny, rq.nz, rq.z_out0, rq.z_out1, h,
                        exact ? tab.box_exact : tab.box_tol, tab.box_tol_sq, rq.exponent, exact);
        break;
      }
      case TvRoute::Tiled:
        rc = dev_tv_tiled(ctx, rq.sal, rq.dir, rq.out, rq.mask_src, rq.mask_dst, rq.nx, rq.ny, rq.nz, rq.z_out0, rq.z_out1, h,
                          tab.padded, rq.exponent, rq.curves, rq.weights_only);
        break;
      case TvRoute::Baseline:
        rc = tv_baseline(ctx, rq, tab);
        break;
    }
  }
  return rc;   // (never TV_DECLINED: the baseline, always the last route, does not decline)
}

}  // namespace

int dev_tv_dense_stick(visfd_hip_ctx* ctx, const float* sal, const float* dir, float* ten,
                       const float* mask_src, const float* mask_dst, i64 nx, i64 ny, i64 nz,
                       i64 z_out0, i64 z_out1, float sigma_tv, int exponent, float cutoff, bool curves) {
  VH_TRY(check_dims(nx, ny, nz));
  VH_TRY(check_dims32(nx, ny, nz));
  VH_REQUIRE(z_out0 >= 0 && z_out1 <= nz && z_out0 <= z_out1, "bad receiver plane range");
  if (z_out0 == z_out1) return VISFD_HIP_OK;
  return tv_dispatch(ctx, {sal, dir, ten, mask_src, mask_dst, nx, ny, nz, z_out0, z_out1, exponent, curves, false}, sigma_tv,
                     cutoff);
}

// (tv_common.hpp: TvStagePlan)  The surface vote of a whole volume in two halves around the caller's one read.
int dev_tv_stage_count(visfd_hip_ctx* ctx, const float* sal, const float* thr_dev, const float* mask, i64 nx, i64 ny, i64 nz,
                       float sigma_tv, int exponent, float cutoff, unsigned long long* total_dev, unsigned* flags_dev,
                       TvStagePlan* plan) {
  VH_TRY(check_dims(nx, ny, nz));
  VH_TRY(check_dims32(nx, ny, nz));
  const int h = host_tv_halfwidth(sigma_tv, cutoff);
  VH_REQUIRE(h >= 0 && h <= 255, "tensor-voting window halfwidth out of range");
  TvRoute routes[4];
  tv_routes(ctx->opt, {sal, nullptr, nullptr, mask, mask, nx, ny, nz, 0, nz, exponent, false, false}, routes);
  if (routes[0] != TvRoute::BoxTol && routes[0] != TvRoute::BoxExact) return TV_DECLINED;
  TvTables tab;
  VH_TRY(tv_table_device(ctx, sigma_tv, cutoff, h, &tab));
  const bool exact = routes[0] == TvRoute::BoxExact;
  *plan = {h, exact, exact ? tab.box_exact : tab.box_tol, tab.box_tol_sq, {}};
  return dev_tv_box_count(ctx, sal, thr_dev, mask, nx, ny, nz, 0, nz, h, exponent, exact, total_dev, flags_dev, &plan->lists);
}

int dev_tv_stage_vote(visfd_hip_ctx* ctx, const TvStagePlan& plan, unsigned long long total, unsigned flags, const float* sal,
                      const float* dir, float* ten, const float* mask, i64 nx, i64 ny, i64 nz, int exponent) {
  return dev_tv_box_vote(ctx, plan.lists, total, flags, sal, dir, ten, mask, mask, nx, ny, nz, 0, nz, plan.h, plan.dtab_box,
                         plan.dtab_box_sq, exponent, plan.exact);
}

// The sum of the weights of the votes every receiver takes (one plane-sized volume): the "denominator" TVDenseStick
// accumulates for its normalisation (feature.hpp:1761-1822, 2376-2382) -- w(j) * mask_src(sender) over the in-bounds
// senders with non-zero saliency, source mask and weight, added in vote order.
int dev_tv_weight_sum(visfd_hip_ctx* ctx, const float* sal, float* den, const float* mask_src, const float* mask_dst, i64 nx,
                      i64 ny, i64 nz, float sigma_tv, float cutoff) {
  VH_TRY(check_dims(nx, ny, nz));
  VH_TRY(check_dims32(nx, ny, nz));
  return tv_dispatch(ctx, {sal, nullptr, den, mask_src, mask_dst, nx, ny, nz, 0, nz, 4, false, true}, sigma_tv, cutoff);
}

}  // namespace vh
