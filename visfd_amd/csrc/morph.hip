// morph.hip -- grayscale morphology with an arbitrary structuring element: Dilate / Erode
// (reference lib/visfd/morphology.hpp:134-229), the building block of DilateSphere, ErodeSphere, OpenSphere,
// CloseSphere and the two top-hats (:241-597; the orchestration is at the end of this file).
//
// Exact by construction: every voxel walks the element in the reference's order and keeps its running value with the
// reference's compare-select (std::max / std::min: cur = (cur < c) ? c : cur, cur = (c < cur) ? c : cur), so NaN
// candidates never win, ties keep the first candidate in element order (the sign of a zero result), and a voxel without
// any candidate ends at -inf / +inf.  Excluded neighbours (mask == 0) arrive as NaN in `src` (dev_nan_masked, or the
// NaN an intermediate pass writes at masked voxels): a NaN candidate leaves the running value alone, exactly like a
// skipped one.  Outside the image nothing is read.
//
// Two kernels, both exact:
//  morph_kernel       the general element walk (any element; soft b, arbitrary tables, flat balls of radius > 10)
//  morph_runs_kernel  flat elements made of symmetric X-runs (every flat ball up to radius 10): see below
//
// morph_kernel layout: a workgroup is 64 x 4 voxels of one plane (a wave reads 64 consecutive floats per element entry); the
// element index is the same across the workgroup, so the entries come in through scalar loads and their offsets are
// scalar arithmetic.  A workgroup whose voxels and whole element footprint lie inside the image takes the loop without
// bounds tests.  Elements whose b are all +0.0f (flat balls) skip the add: f - (+0) == f bit for bit where it can win,
// and the dilation adds its +0.0f once at the end (the winner is the same; -0 turns into +0 as the reference's f + 0 does).
#include <algorithm>
#include <cmath>
#include <vector>

#include "common.hpp"

namespace vh {

namespace {

constexpr int MX = 64, MY = 4;

template <bool DILATE, bool FLAT>
__device__ __forceinline__ void morph_take(float& cur, float f, float b) {
  const float c = FLAT ? f : (DILATE ? f + b : f - b);
  if (DILATE)
    cur = (cur < c) ? c : cur;
  else
    cur = (c < cur) ? c : cur;
}

// the result of voxel i: voxels with mask == 0 are not written (or get NaN in an intermediate image, so that the next pass
// does not take them as candidates); the top-hats' subtraction is fused here
__device__ __forceinline__ void morph_store(float* __restrict__ dst, const float* __restrict__ mask, i64 i, float cur,
                                            int epi, int nan_masked) {
  if (mask && mask[i] == 0.0f) {
    if (nan_masked) dst[i] = NAN;
    return;
  }
  float v = cur;
  if (epi == 1)
    v = dst[i] - cur;   // WhiteTopHatSphere: dest -= open(src)          (morphology.hpp:545-549)
  else if (epi == 2)
    v = cur - dst[i];   // BlackTopHatSphere: dest = close(src) - dest   (morphology.hpp:587-591)
  dst[i] = v;
}

template <bool DILATE, bool FLAT>
__global__ void __launch_bounds__(MX * MY)
morph_kernel(const float* __restrict__ src, float* __restrict__ dst, const float* __restrict__ mask,
             const int4* __restrict__ tab, int n, int nx, int ny, int nz, int lox, int loy, int loz, int hix, int hiy,
             int hiz, int epi, int nan_masked) {
  const int x0 = blockIdx.x * MX, y0 = blockIdx.y * MY;
  const int x = x0 + threadIdx.x, y = y0 + threadIdx.y;
  const bool mine = x < nx && y < ny;
  const i64 plane = (i64)nx * ny;
  // every voxel of the workgroup in the image, and every neighbour the element reaches from them
  const bool xy_inside = x0 + MX <= nx && y0 + MY <= ny && x0 + lox >= 0 && y0 + loy >= 0 && x0 + MX - 1 + hix < nx &&
                         y0 + MY - 1 + hiy < ny;
  for (int z = blockIdx.z; z < nz; z += gridDim.z) {
    const i64 i = (i64)z * plane + (i64)y * nx + x;
    float cur = DILATE ? -INFINITY : INFINITY;
    if (xy_inside && z + loz >= 0 && z + hiz < nz) {
      const float* p = src + i;
#pragma unroll 8
      for (int k = 0; k < n; k++) {
        const int4 e = tab[k];
        morph_take<DILATE, FLAT>(cur, p[(i64)e.z * plane + (i64)e.y * nx + e.x], __int_as_float(e.w));
      }
    } else if (mine) {
      for (int k = 0; k < n; k++) {
        const int4 e = tab[k];
        const int X = x + e.x, Y = y + e.y, Z = z + e.z;
        if ((unsigned)X >= (unsigned)nx || (unsigned)Y >= (unsigned)ny || (unsigned)Z >= (unsigned)nz) continue;
        morph_take<DILATE, FLAT>(cur, src[(i64)Z * plane + (i64)Y * nx + X], __int_as_float(e.w));
      }
    }
    if (!mine) continue;
    if (DILATE && FLAT) cur = cur + 0.0f;
    morph_store(dst, mask, i, cur, epi, nan_masked);
  }
}

// ---- morph_runs_kernel: flat elements made of symmetric X-runs --------------------------------------------------------
// Every (dy, dz) row of the element is a run dx = -L..L.  For one input plane the 1-D window extrema of every half-length
// come from M_0 = the row, M_{L+1}(x) = max(M_L(x-1), M_L(x), M_L(x+1)) (one v_max3; the middle term matters only for
// L = 0, where the two outer windows leave x out); an output voxel is the extremum, over the element's rows,
// of M_{L(dy,dz)}(x) of row y+dy of plane z+dz.  A workgroup owns 64 x 8 x 8 outputs (a thread: one x, two y, eight z);
// it marches through the input planes z0-R .. z0+7+R, builds all R+1 levels of the plane's (8+2R) rows in LDS (outside
// the image: the -inf / +inf sentinel) and folds them into the outputs the plane reaches.
// Exactness: NaN candidates (masked neighbours are NaN) become the sentinel as they enter LDS, which is what the
// reference's compare-select makes of them (they never win; a voxel without other candidates stays at -inf / +inf); the flat element
// adds +0.0f to every candidate, so the dilation's result + 0.0f is the reference's (only +-0 tie, and both end as +0);
// an erosion whose minimum compares equal to 0 walks the element in reference order once more and takes the first zero
// candidate (its sign is the reference's: the first zero candidate is the one its running minimum keeps).
constexpr int RX = 64, RTY = 8, RTZ = 8;
struct RunLens {
  signed char L[(2 * MORPH_RUN_MAX_R + 1) * (2 * MORPH_RUN_MAX_R + 1)];
};

template <bool DILATE>
__device__ __forceinline__ float ext(float a, float b) {
  return DILATE ? fmaxf(a, b) : fminf(a, b);
}

template <bool DILATE>
__global__ void __launch_bounds__(RX * 4)
morph_runs_kernel(const float* __restrict__ src, float* __restrict__ dst, const float* __restrict__ mask,
                  const int4* __restrict__ tab, int n, RunLens rl, int R, int nx, int ny, int nz, int epi, int nan_masked) {
  extern __shared__ float lv[];   // (R+1) levels of H rows of W floats
  const int tx = threadIdx.x, ty = threadIdx.y, tid = ty * RX + tx;
  const int x0 = blockIdx.x * RX, y0 = blockIdx.y * RTY, z0 = blockIdx.z * RTZ;
  const int W = RX + 2 * R, H = RTY + 2 * R, LV = W * H, S = 2 * R + 1;
  const i64 plane = (i64)nx * ny;
  const float sent = DILATE ? -INFINITY : INFINITY;
  float acc[RTZ][2];
#pragma unroll
  for (int o = 0; o < RTZ; o++) acc[o][0] = acc[o][1] = sent;
  const int p_lo = max(z0 - R, 0), p_hi = min(z0 + RTZ - 1 + R, nz - 1);
  for (int p = p_lo; p <= p_hi; p++) {
    __syncthreads();   // the previous plane's levels have been read
    for (int k = tid; k < LV; k += RX * 4) {
      const int X = x0 - R + k % W, Y = y0 - R + k / W;
      const float f = (X >= 0 && X < nx && Y >= 0 && Y < ny) ? src[(i64)p * plane + (i64)Y * nx + X] : sent;
      lv[k] = (f == f) ? f : sent;   // NaN (masked neighbours too) never wins: the sentinel says the same, and a
                                     // signalling NaN must not reach v_max / v_min (IEEE mode returns a quiet NaN)
    }
    __syncthreads();
    for (int L = 1; L <= R; L++) {
      const float* prev = lv + (L - 1) * LV;
      float* cur = lv + L * LV;
      for (int k = tid; k < LV; k += RX * 4) {
        const int c = k % W;
        cur[k] = (c >= 1 && c < W - 1) ? ext<DILATE>(prev[k - 1], ext<DILATE>(prev[k], prev[k + 1])) : sent;   // valid on [L, W-1-L]
      }
      __syncthreads();
    }
#pragma unroll
    for (int o = 0; o < RTZ; o++) {
      const int dz = p - (z0 + o);
      if (dz < -R || dz > R) continue;
      for (int dy = -R; dy <= R; dy++) {
        const int L = rl.L[(dz + R) * S + dy + R];
        if (L < 0) continue;
        const float* row = lv + L * LV + (ty + dy + R) * W + tx + R;
        acc[o][0] = ext<DILATE>(acc[o][0], row[0]);
        acc[o][1] = ext<DILATE>(acc[o][1], row[4 * W]);
      }
    }
  }
  const int x = x0 + tx;
  if (x >= nx) return;
#pragma unroll
  for (int o = 0; o < RTZ; o++) {
    const int z = z0 + o;
    if (z >= nz) break;
#pragma unroll
    for (int j = 0; j < 2; j++) {
      const int y = y0 + ty + 4 * j;
      if (y >= ny) continue;
      const i64 i = (i64)z * plane + (i64)y * nx + x;
      float v = acc[o][j];
      if (DILATE) {
        v = v + 0.0f;
      } else if (v == 0.0f) {   // zero-sign fix-up: the first zero candidate in element order
        for (int k = 0; k < n; k++) {
          const int4 e = tab[k];
          const int X = x + e.x, Y = y + e.y, Z = z + e.z;
          if ((unsigned)X >= (unsigned)nx || (unsigned)Y >= (unsigned)ny || (unsigned)Z >= (unsigned)nz) continue;
          const float f = src[(i64)Z * plane + (i64)Y * nx + X];
          if (f == 0.0f) {
            v = f;
            break;
          }
        }
      }
      morph_store(dst, mask, i, v, epi, nan_masked);
    }
  }
}

__global__ void __launch_bounds__(256) nan_masked_kernel(const float* __restrict__ src, const float* __restrict__ mask,
                                                         float* __restrict__ out, i64 n) {
  for (i64 i = (i64)blockIdx.x * 256 + threadIdx.x; i < n; i += (i64)gridDim.x * 256)
    out[i] = (mask[i] == 0.0f) ? NAN : src[i];
}

}  // namespace

int dev_nan_masked(visfd_hip_ctx* ctx, const float* src, const float* mask, float* out, i64 n) {
  const unsigned g = grid_for(n, 256, (i64)ctx->num_cus * 16);
  nan_masked_kernel<<<dim3(g), dim3(256), 0, ctx->stream>>>(src, mask, out, n);
  VH_HIP(hipGetLastError());
  return VISFD_HIP_OK;
}

int dev_morph_table(visfd_hip_ctx* ctx, const float* src, float* dst, const float* mask, i64 nx, i64 ny, i64 nz,
                    const MorphElem& el, bool dilate, int epi, bool nan_masked, int* path) {
  VH_REQUIRE(nx < (1 << 30) && ny < (1 << 30) && nz < (1 << 30), "morphology: image dimensions must be below 2^30");
  VH_REQUIRE(el.n >= 0 && el.n < ((i64)1 << 31), "morphology: too many structuring element entries");
  const int4* tab = static_cast<const int4*>(ctx->slot_ptr[WS_MORPH_TAB]);
  VH_REQUIRE(tab || el.n == 0, "morphology: no structuring element on the device");
  const int n = (int)el.n;
  if (el.runs && el.n > 0) {
    VH_REQUIRE(el.R >= 0 && el.R <= MORPH_RUN_MAX_R, "morphology: X-run element too wide");
    RunLens rl;
    std::memcpy(rl.L, el.run_len, sizeof(rl.L));
    const size_t lds = sizeof(float) * (size_t)(el.R + 1) * (RX + 2 * el.R) * (RTY + 2 * el.R);
    const dim3 grid((unsigned)((nx + RX - 1) / RX), (unsigned)((ny + RTY - 1) / RTY), (unsigned)((nz + RTZ - 1) / RTZ));
    VH_REQUIRE(grid.z <= 65535u, "morphology: too many planes");
    const dim3 block(RX, 4);
    if (dilate) {
      VH_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&morph_runs_kernel<true>),
                                 hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
      morph_runs_kernel<true><<<grid, block, lds, ctx->stream>>>(src, dst, mask, tab, n, rl, el.R, (int)nx, (int)ny,
                                                                 (int)nz, epi, nan_masked ? 1 : 0);
    } else {
      VH_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&morph_runs_kernel<false>),
                                 hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
      morph_runs_kernel<false><<<grid, block, lds, ctx->stream>>>(src, dst, mask, tab, n, rl, el.R, (int)nx, (int)ny,
                                                                  (int)nz, epi, nan_masked ? 1 : 0);
    }
    VH_HIP(hipGetLastError());
    *path = VISFD_HIP_MORPH_PATH_XRUNS;
    return VISFD_HIP_OK;
  }
  const int* lo = el.lo;
  const int* hi = el.hi;
  const bool flat = el.flat;
  const dim3 grid((unsigned)((nx + MX - 1) / MX), (unsigned)((ny + MY - 1) / MY), (unsigned)(nz < 65535 ? nz : 65535));
  const dim3 block(MX, MY);
#define VH_MORPH_LAUNCH(D, F)                                                                                          \
  morph_kernel<D, F><<<grid, block, 0, ctx->stream>>>(src, dst, mask, tab, n, (int)nx, (int)ny, (int)nz, lo[0],       \
                                                      lo[1], lo[2], hi[0], hi[1], hi[2], epi, nan_masked ? 1 : 0)
  if (dilate && flat) VH_MORPH_LAUNCH(true, true);
  else if (dilate) VH_MORPH_LAUNCH(true, false);
  else if (flat) VH_MORPH_LAUNCH(false, true);
  else VH_MORPH_LAUNCH(false, false);
#undef VH_MORPH_LAUNCH
  VH_HIP(hipGetLastError());
  *path = VISFD_HIP_MORPH_PATH_GENERAL;
  return VISFD_HIP_OK;
}

// puts the element in slot WS_MORPH_TAB (4 ints per entry: dx, dy, dz, bits of b); an element equal to the one already
// there is not sent again.  Fills `el`: count, bounding box, flatness and, for flat elements made of symmetric X-runs,
// the run length of every (dy, dz) row (the X-run kernel's input).
int morph_put_table(visfd_hip_ctx* ctx, const int* dxyz, const float* b, i64 n, MorphElem* el) {
  VH_REQUIRE(n >= 0 && n < ((i64)1 << 31), "morphology: too many structuring element entries");
  VH_REQUIRE(n == 0 || (dxyz && b), "null argument");
  std::vector<int> t((size_t)(4 * n));
  el->n = n;
  el->flat = true;
  int* lo = el->lo;
  int* hi = el->hi;
  for (int d = 0; d < 3; d++) lo[d] = hi[d] = 0;
  for (i64 k = 0; k < n; k++) {
    for (int d = 0; d < 3; d++) {
      const int v = dxyz[3 * k + d];
      VH_REQUIRE(v > -(1 << 30) && v < (1 << 30), "morphology: structuring element offsets must be below 2^30");
      lo[d] = (k == 0 || v < lo[d]) ? v : lo[d];
      hi[d] = (k == 0 || v > hi[d]) ? v : hi[d];
      t[4 * k + d] = v;
    }
    int bits;
    std::memcpy(&bits, &b[k], 4);
    t[4 * k + 3] = bits;
    if (bits != 0) el->flat = false;
  }
  // X-runs: each (dy, dz) row holds exactly the offsets dx = -L..L (in any order, repeats allowed)
  el->runs = false;
  int R = 0;
  for (int d = 0; d < 3; d++) R = std::max(R, std::max(-lo[d], hi[d]));
  if (n > 0 && el->flat && R <= MORPH_RUN_MAX_R) {
    const int S = 2 * R + 1;
    std::vector<uint32_t> rows((size_t)(S * S), 0u);   // bit dx + R of row (dy, dz)
    for (i64 k = 0; k < n; k++) rows[(size_t)((t[4 * k + 2] + R) * S + t[4 * k + 1] + R)] |= 1u << (t[4 * k] + R);
    bool ok = true;
    for (int r = 0; r < S * S && ok; r++) {
      el->run_len[r] = -1;
      if (!rows[r]) continue;
      int L = 0;
      while (L < R && (rows[r] >> (R - L - 1) & 1u)) L++;
      const uint32_t want = ((1u << (2 * L + 1)) - 1u) << (R - L);
      ok = rows[r] == want;
      el->run_len[r] = (signed char)L;
    }
    el->runs = ok;
    el->R = R;
  }
  const size_t bytes = sizeof(int) * t.size();
  if (n == 0 || ws_holds(ctx, WS_MORPH_TAB, t.data(), bytes)) return VISFD_HIP_OK;
  return ws_put(ctx, WS_MORPH_TAB, t.data(), bytes, t.data(), bytes);
}

// one op with the element in WS_MORPH_TAB.  Open = erode then dilate, close = dilate then erode (morphology.hpp:431-510),
// both steps with the same mask and element; the top-hats fuse their subtraction into the second step.
int morph_run(visfd_hip_ctx* ctx, const float* src, float* dst, const float* mask, i64 nx, i64 ny, i64 nz, int op,
              MorphElem el) {
  if (ctx->opt.morph_general) el.runs = false;
  const i64 nv = nx * ny * nz;
  const float* s0 = src;
  if (mask) {
    float* sn = nullptr;
    VH_TRY(ws(ctx, WS_MORPH_SRC, (size_t)nv, &sn));
    VH_TRY(dev_nan_masked(ctx, src, mask, sn, nv));
    s0 = sn;
  }
  int path = 0;
  if (op == VISFD_HIP_MORPH_DILATE || op == VISFD_HIP_MORPH_ERODE) {
    VH_TRY(dev_morph_table(ctx, s0, dst, mask, nx, ny, nz, el, op == VISFD_HIP_MORPH_DILATE, 0, false, &path));
    ctx->morph_last_path = path;
    return VISFD_HIP_OK;
  }
  float* tmp = nullptr;
  VH_TRY(ws(ctx, WS_MORPH_TMP, (size_t)nv, &tmp));
  const bool dilate_first = (op == VISFD_HIP_MORPH_CLOSE || op == VISFD_HIP_MORPH_TOP_HAT_BLACK);
  const int epi = op == VISFD_HIP_MORPH_TOP_HAT_WHITE ? 1 : op == VISFD_HIP_MORPH_TOP_HAT_BLACK ? 2 : 0;
  VH_TRY(dev_morph_table(ctx, s0, tmp, mask, nx, ny, nz, el, dilate_first, 0, mask != nullptr, &path));
  VH_TRY(dev_morph_table(ctx, tmp, dst, mask, nx, ny, nz, el, !dilate_first, epi, false, &path));
  ctx->morph_last_path = path;
  return VISFD_HIP_OK;
}

}  // namespace vh
