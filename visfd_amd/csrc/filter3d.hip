// filter3d.hip -- the general (non-separable) linear filter: Filter3D::Apply with an arbitrary table of
// (2 hx + 1)(2 hy + 1)(2 hz + 1) weights (reference lib/visfd/filter3d.hpp:37-530), the generalised Gaussian and
// difference-of-generalised-Gaussians built on it (HandleGGauss / HandleDogg, bin/filter_mrc/handlers.cpp:167-293) and
// LocalFluctuations for any exponent (filter3d.hpp:1698-1853).  The entry points are at the end of this file.
//
// Contract (Filter3D::ApplyToVoxel, filter3d.hpp:403-458, and the loop around it, :167-197), float throughout:
//   a voxel with mask == 0 gets dst = 0 and den = 0 -- also when nobody asked for den, where the reference dereferences a
//   null pointer (:182): that is the one behaviour this project defines for itself;
//   otherwise g = 0, den = 0, then for jz, jy, jx ascending from -h to +h: sender s = i - j, skipped outside the image;
//   fv = H[j]; with a mask, skipped where mask(s) == 0, else fv = fv * mask(s); g += fv * src(s); den += fv
//   (multiply, then add: this file is built with -ffp-contract=off and uses no fma);
//   normalised: dst = g / den where den > 0, else g (:100-108).
//
// What exactness allows: g and den start at +0 and round-to-nearest never makes -0 of a sum that holds a +0, so adding
// (+-0) * finite changes nothing.  For FINITE source values a skipped tap and a tap with a zero product therefore give
// the same bits, which lets a kernel (1) drop the table's zero entries up front (a spherical support zeroes about
// half of its cube), (2) take masked senders and senders outside the image as zero factors without a branch.  The
// price, and the one divergence from the reference: a NaN or Inf under a zero weight or outside the mask need not poison
// its neighbours (the general kernel drops zero entries, the tiled one multiplies those inside a non-zero column).
// (h * mask) * src keeps that operand order: a weighted mask is legal, so mask * src is never formed.
// Without a mask den is needed only where the window leaves the image: everywhere else it is one number, the float sum
// of the table in order, which the host computes.
//
// Two kernels (dev_filter3d chooses; visfd_hip_filter3d_last_path reports; both give the same bits for finite inputs):
// filter3d_tiled_kernel stages source planes in LDS and keeps 8 output planes per thread (described where it stands); it
// takes every window whose patches fit LDS.  filter3d_kernel takes the rest, and everything under the option
// filter3d_general.  Its layout is the morphology element walk's (csrc/morph.hip): a workgroup is 64 x 4 voxels of one
// plane and walks the planes of its column; the entry index is the same across the workgroup, so entries come in through
// scalar loads; a wave reads 64 consecutive floats per entry.  A workgroup whose voxels and whole window lie inside the
// image takes the loop without bounds tests, on sender offsets the host computed for the image at hand.  No limit on the
// window beyond the table's size.  All voxel indices are 64-bit.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "common.hpp"

namespace vh {

namespace {

constexpr int FX = 64, FY = 4;

// The table on the device: n entries (jx, jy, jz, bits of h) for workgroups that test every sender, then the same n
// entries as (lo, hi, bits of h, 0) with lo/hi the 64-bit BYTE offset of the sender from the receiver for the image at
// hand, -4 (jz nx ny + jy nx + jx), for workgroups that test none: the host forms the product once per table and image.
template <bool MASK>
__global__ void __launch_bounds__(FX * FY)
filter3d_kernel(const float* __restrict__ src, float* __restrict__ dst, const float* __restrict__ mask,
                float* __restrict__ den_out, const int4* __restrict__ tab, int n, int nx, int ny, int nz, int hx, int hy,
                int hz, int normalize, float den_inside) {
  const int x0 = blockIdx.x * FX, y0 = blockIdx.y * FY;
  const int x = x0 + threadIdx.x, y = y0 + threadIdx.y;
  const bool mine = x < nx && y < ny;
  const i64 plane = (i64)nx * ny;
  // every voxel of the workgroup in the image, and every sender the window reaches from them; a plane's byte offsets
  // fit 32 bits, so a load is a scalar base (plane and entry) plus one 32-bit lane offset
  const bool xy_inside = x0 + FX <= nx && y0 + FY <= ny && x0 - hx >= 0 && y0 - hy >= 0 && x0 + FX - 1 + hx < nx &&
                         y0 + FY - 1 + hy < ny && plane < ((i64)1 << 30);
  const int4* __restrict__ otab = tab + n;
  for (int z = blockIdx.z; z < nz; z += gridDim.z) {
    const i64 i = (i64)z * plane + (i64)y * nx + x;
    float g = 0.0f, den = 0.0f;
    if (xy_inside && z - hz >= 0 && z + hz < nz) {
      const char* p = reinterpret_cast<const char*>(src + (i64)z * plane);
      const char* pm = MASK ? reinterpret_cast<const char*>(mask + (i64)z * plane) : nullptr;
      const unsigned lane = (unsigned)(y * nx + x) * 4u;
#pragma unroll 4
      for (int k = 0; k < n; k++) {
        const int4 e = otab[k];
        const i64 off = (i64)(((unsigned long long)(unsigned)e.y << 32) | (unsigned)e.x);
        float fv = __int_as_float(e.z);
        if (MASK) {
          fv = fv * *reinterpret_cast<const float*>(pm + off + lane);
          den += fv;
        }
        const float dg = fv * *reinterpret_cast<const float*>(p + off + lane);
        g += dg;
      }
      if (!MASK) den = den_inside;
    } else if (mine) {
      for (int k = 0; k < n; k++) {
        const int4 e = tab[k];
        const int X = x - e.x, Y = y - e.y, Z = z - e.z;
        if ((unsigned)X >= (unsigned)nx || (unsigned)Y >= (unsigned)ny || (unsigned)Z >= (unsigned)nz) continue;
        const i64 s = (i64)Z * plane + (i64)Y * nx + X;
        float fv = __int_as_float(e.w);
        if (MASK) fv = fv * mask[s];
        const float dg = fv * src[s];
        g += dg;
        den += fv;
      }
    }
    if (!mine) continue;
    if (MASK && mask[i] == 0.0f) {
      g = 0.0f;
      den = 0.0f;
    } else if (normalize && den > 0.0f) {
      g = g / den;
    }
    dst[i] = g;
    if (den_out) den_out[i] = den;
  }
}

// The tiled kernel.  Every sum runs in jz ascending order, that is over source planes in DESCENDING z.  A workgroup owns
// FK consecutive output planes of a 64 x 4 column (FK accumulators per thread, FK more for den in the DEN form) and
// streams the source planes from z0 + FK - 1 + hz down to z0 - hz; each plane's (4 + 2 hy) x (64 + 2 hx) patch is staged
// in LDS (0 outside the image), in the DEN form the mask's patch too (0 outside the image, 1 inside where there is no
// mask).  For jy, jx ascending a thread reads the staged value once and feeds every output plane the source plane
// reaches with that plane's own H[jz][jy][jx]: per output voxel the order is exactly the reference's.  The table's device
// form for this kernel (filter3d_put_table): the columns (jy, jx) that hold a non-zero entry, in order, each as its patch
// offset (hy - jy) PW + (hx - jx) followed by its 2 hz + 1 weights with FK - 1 zeros before and after, so that output plane
// k of source plane zs finds its weight at k + (z0 - zs + hz + FK - 1) without a test: a weight of 0 for the planes the
// source plane does not reach, whose zero product changes nothing (see above).  Weights and offsets are wave-uniform.
constexpr int FK = 8;

template <bool DEN>
__device__ __forceinline__ void tiled_column(const int* __restrict__ cols, int ncols, int stride, int d,
                                             const float* __restrict__ ps, const float* __restrict__ pm, float (&g)[FK],
                                             float (&den)[FK]) {
  for (int c = 0; c < ncols; c++) {
    const int* col = cols + (i64)c * stride;
    const int lo = col[0];
    const float v = ps[lo];
    const float m = DEN ? pm[lo] : 0.0f;
#pragma unroll
    for (int k = 0; k < FK; k++) {
      float fv = __int_as_float(col[1 + d + k]);
      if (DEN) {
        fv = fv * m;
        den[k] += fv;
      }
      const float dg = fv * v;
      g[k] += dg;
    }
  }
}

template <bool DEN>
__device__ __forceinline__ void tiled_planes(const float* __restrict__ src, const float* __restrict__ mask,
                                             const int* __restrict__ cols, int ncols, int nx, int ny, int nz, int hx, int hy,
                                             int hz, int x0, int y0, int z0, float* lds, float (&g)[FK], float (&den)[FK]) {
  const int PW = FX + 2 * hx, PH = FY + 2 * hy, stride = 1 + 2 * hz + 1 + 2 * (FK - 1);
  const i64 plane = (i64)nx * ny;
  float* ps = lds;
  float* pm = lds + PH * PW;
  const int tid = threadIdx.y * FX + threadIdx.x, here = threadIdx.y * PW + threadIdx.x;
  const int zs_hi = min(nz - 1, z0 + FK - 1 + hz), zs_lo = max(0, z0 - hz);   // planes outside the image send nothing
  for (int zs = zs_hi; zs >= zs_lo; zs--) {
    __syncthreads();   // the plane before this one has been read
    for (int e = tid; e < PH * PW; e += FX * FY) {
      const int py = e / PW, px = e - py * PW;
      const int X = x0 - hx + px, Y = y0 - hy + py;
      const bool in = (unsigned)X < (unsigned)nx && (unsigned)Y < (unsigned)ny;
      const i64 s = (i64)zs * plane + (i64)Y * nx + X;
      ps[e] = in ? src[s] : 0.0f;
      if (DEN) pm[e] = in ? (mask ? mask[s] : 1.0f) : 0.0f;
    }
    __syncthreads();
    tiled_column<DEN>(cols, ncols, stride, z0 - zs + hz + FK - 1, ps + here, pm + here, g, den);
  }
}

__global__ void __launch_bounds__(FX * FY)
filter3d_tiled_kernel(const float* __restrict__ src, float* __restrict__ dst, const float* __restrict__ mask,
                      float* __restrict__ den_out, const int* __restrict__ cols, int ncols, int nx, int ny, int nz, int hx,
                      int hy, int hz, int normalize, float den_inside) {
  extern __shared__ float lds[];
  const int x0 = blockIdx.x * FX, y0 = blockIdx.y * FY, z0 = blockIdx.z * FK;
  const int x = x0 + threadIdx.x, y = y0 + threadIdx.y;
  // every sender the window reaches from the workgroup's voxels in the image: then, without a mask, den is one number
  const bool inside = x0 - hx >= 0 && y0 - hy >= 0 && z0 - hz >= 0 && x0 + FX - 1 + hx < nx && y0 + FY - 1 + hy < ny &&
                      z0 + FK - 1 + hz < nz;
  const bool need_den = mask || (!inside && (normalize || den_out));
  float g[FK], den[FK];
#pragma unroll
  for (int k = 0; k < FK; k++) g[k] = den[k] = 0.0f;
  if (need_den)
    tiled_planes<true>(src, mask, cols, ncols, nx, ny, nz, hx, hy, hz, x0, y0, z0, lds, g, den);
  else
    tiled_planes<false>(src, mask, cols, ncols, nx, ny, nz, hx, hy, hz, x0, y0, z0, lds, g, den);
  if (x >= nx || y >= ny) return;
  const i64 plane = (i64)nx * ny;
#pragma unroll
  for (int k = 0; k < FK; k++) {
    if (z0 + k >= nz) break;
    const i64 i = (i64)(z0 + k) * plane + (i64)y * nx + x;
    float gk = g[k], dk = need_den ? den[k] : den_inside;
    if (mask && mask[i] == 0.0f) {
      gk = 0.0f;
      dk = 0.0f;
    } else if (normalize && dk > 0.0f) {
      gk = gk / dk;
    }
    dst[i] = gk;
    if (den_out) den_out[i] = dk;
  }
}

// The tiled kernel takes a window whose two patches (source and mask) fit 48 KB of LDS, whatever the call stages.
bool tiled_accepts(const int hw[3]) {
  return (i64)(FX + 2 * hw[0]) * (FY + 2 * hw[1]) * 2 * (i64)sizeof(float) <= 48 * 1024;
}


int check_halfwidths(const int hw[3]) {
  VH_REQUIRE(hw, "null argument");
  for (int d = 0; d < 3; d++) VH_REQUIRE(hw[d] >= 0, "filter half-widths must not be negative");
  for (int d = 0; d < 3; d++) VH_REQUIRE(hw[d] <= 1024, "filter half-widths must be at most 1024");
  // 127^3 fits: far beyond what a dense filter is used for, and small enough that a table and its device form are MBs
  VH_REQUIRE((2 * (i64)hw[0] + 1) * (2 * (i64)hw[1] + 1) * (2 * (i64)hw[2] + 1) <= ((i64)1 << 21),
             "filter table must have at most 2^21 entries");
  return VISFD_HIP_OK;
}

i64 table_size(const int hw[3]) { return (2 * (i64)hw[0] + 1) * (2 * (i64)hw[1] + 1) * (2 * (i64)hw[2] + 1); }

// everything that can be said about a filter call without a device
int filter3d_check(visfd_hip_ctx* ctx, const float* src, float* dst, const float* mask, i64 nx, i64 ny, i64 nz,
                   const float* den_out) {
  VH_TRY(check_out_of_place(ctx, src, dst, mask, nx, ny, nz, "the 3-D filter", "the 3-D filter"));
  const i64 n = nx * ny * nz;
  VH_REQUIRE(!overlaps(den_out, dst, n) && !overlaps(den_out, src, n) && !overlaps(den_out, mask, n),
             "the 3-D filter: the denominator overlaps another array");
  return VISFD_HIP_OK;
}

// The table's non-zero entries into slot WS_F3D_TAB in the two forms filter3d_kernel reads (jz outermost, then jy, then
// jx, each ascending).  The slot's key is the window, the image's row and plane lengths and the raw table it expanded
// last: a call with the same ones compares the bytes and sends nothing.  *den_inside = the float sum of the entries
// in order: the denominator of every voxel whose window lies inside an unmasked image.
int filter3d_put_table(visfd_hip_ctx* ctx, const float* table, const int hw[3], i64 nx, i64 ny, i64* n_out,
                       float* den_inside) {
  const size_t size = (size_t)table_size(hw);
  const int64_t head[5] = {hw[0], hw[1], hw[2], nx, ny};
  std::vector<unsigned char> key(sizeof head + sizeof(float) * size);
  std::memcpy(key.data(), head, sizeof head);
  std::memcpy(key.data() + sizeof head, table, sizeof(float) * size);
  if (ws_holds(ctx, WS_F3D_TAB, key.data(), key.size())) {
    *n_out = ctx->f3d.n;
    *den_inside = ctx->f3d.den;
    return VISFD_HIP_OK;
  }
  std::vector<int> near, far;   // the tested form, the offset form
  float total = 0.0f;
  const float* h = table;
  for (int jz = -hw[2]; jz <= hw[2]; jz++)
    for (int jy = -hw[1]; jy <= hw[1]; jy++)
      for (int jx = -hw[0]; jx <= hw[0]; jx++, h++) {
        if (*h == 0.0f) continue;
        int bits;
        std::memcpy(&bits, h, 4);
        const int e[4] = {jx, jy, jz, bits};
        near.insert(near.end(), e, e + 4);
        const unsigned long long off = (unsigned long long)(-4 * (jz * nx * ny + jy * nx + jx));
        const int o[4] = {(int)(unsigned)(off & 0xffffffffu), (int)(unsigned)(off >> 32), bits, 0};
        far.insert(far.end(), o, o + 4);
        total += *h;
      }
  *n_out = (i64)(near.size() / 4);
  *den_inside = total;
  if (near.empty()) return VISFD_HIP_OK;   // nothing to read: whatever the slot holds stays valid for its own key
  near.insert(near.end(), far.begin(), far.end());
  // the tiled kernel's form (see there): per non-zero column its patch offset and its padded weights along jz
  const int PW = FX + 2 * hw[0], stride = 1 + 2 * hw[2] + 1 + 2 * (FK - 1);
  const i64 slab = (2 * (i64)hw[1] + 1) * (2 * hw[0] + 1);
  i64 ncols = 0;
  if (tiled_accepts(hw))
    for (int jy = -hw[1]; jy <= hw[1]; jy++)
      for (int jx = -hw[0]; jx <= hw[0]; jx++) {
        const float* col = table + (i64)(jy + hw[1]) * (2 * hw[0] + 1) + (jx + hw[0]);
        bool any = false;
        for (int jz = 0; jz <= 2 * hw[2]; jz++) any = any || col[jz * slab] != 0.0f;
        if (!any) continue;
        const size_t at = near.size();
        near.resize(at + (size_t)stride, 0);
        near[at] = (hw[1] - jy) * PW + (hw[0] - jx);
        for (int jz = 0; jz <= 2 * hw[2]; jz++) std::memcpy(&near[at + 1 + (FK - 1) + jz], &col[jz * slab], 4);
        ncols++;
      }
  VH_TRY(ws_put(ctx, WS_F3D_TAB, key.data(), key.size(), near.data(), sizeof(int) * near.size()));
  ctx->f3d = {*n_out, ncols, total};
  return VISFD_HIP_OK;
}

}  // namespace

int dev_filter3d(visfd_hip_ctx* ctx, const float* src, float* dst, const float* mask, i64 nx, i64 ny, i64 nz,
                 const float* table, const int hw[3], bool normalize, float* den_out) {
  VH_REQUIRE(table, "null argument");
  VH_TRY(check_halfwidths(hw));
  VH_TRY(filter3d_check(ctx, src, dst, mask, nx, ny, nz, den_out));
  VH_REQUIRE(nx < (1 << 30) && ny < (1 << 30) && nz < (1 << 30), "the 3-D filter: image dimensions must be below 2^30");
  i64 n = 0;
  float den_inside = 0.0f;
  VH_TRY(filter3d_put_table(ctx, table, hw, nx, ny, &n, &den_inside));
  const int4* tab = static_cast<const int4*>(ctx->slot_ptr[WS_F3D_TAB]);
  VH_REQUIRE(tab || n == 0, "the 3-D filter: no table on the device");
  const dim3 block(FX, FY);
  const unsigned gx = (unsigned)((nx + FX - 1) / FX), gy = (unsigned)((ny + FY - 1) / FY);
  VH_REQUIRE(gy <= 65535u, "the 3-D filter: too many rows");
  // the tiled kernel where its patches fit (and the table has an entry to stage for), else the general one
  const bool tiled = !ctx->opt.filter3d_general && n > 0 && tiled_accepts(hw) && (nz + FK - 1) / FK <= 65535;
  ctx->f3d_last_path = tiled ? VISFD_HIP_FILTER3D_PATH_TILED : VISFD_HIP_FILTER3D_PATH_GENERAL;
  if (tiled) {
    const int* cols = reinterpret_cast<const int*>(tab + 2 * n);
    const size_t patch = (size_t)(FX + 2 * hw[0]) * (FY + 2 * hw[1]) * sizeof(float);
    const size_t lds = (mask || normalize || den_out) ? 2 * patch : patch;
    filter3d_tiled_kernel<<<dim3(gx, gy, (unsigned)((nz + FK - 1) / FK)), block, lds, ctx->stream>>>(
        src, dst, mask, den_out, cols, (int)ctx->f3d.ncols, (int)nx, (int)ny, (int)nz, hw[0], hw[1], hw[2],
        normalize ? 1 : 0, den_inside);
    VH_HIP(hipGetLastError());
    return VISFD_HIP_OK;
  }
  const dim3 grid(gx, gy, (unsigned)(nz < 65535 ? nz : 65535));
  if (mask)
    filter3d_kernel<true><<<grid, block, 0, ctx->stream>>>(src, dst, mask, den_out, tab, (int)n, (int)nx, (int)ny, (int)nz,
                                                           hw[0], hw[1], hw[2], normalize ? 1 : 0, den_inside);
  else
    filter3d_kernel<false><<<grid, block, 0, ctx->stream>>>(src, dst, nullptr, den_out, tab, (int)n, (int)nx, (int)ny,
                                                            (int)nz, hw[0], hw[1], hw[2], normalize ? 1 : 0, den_inside);
  VH_HIP(hipGetLastError());
  return VISFD_HIP_OK;
}

namespace {

// the windows the table makers accept: what check_halfwidths accepts, said before any table is allocated
int window_of(const float width[3], float m_exp, float ratio, float threshold, int hw[3]) {
  VH_REQUIRE(width && hw, "null argument");
  host_gengauss3d_halfwidths(width, m_exp, ratio, threshold, hw);
  return check_halfwidths(hw);
}

}  // namespace
}  // namespace vh

using namespace vh;

extern "C" {

// ---- g1: the tables (host arithmetic, no context) -------------------------------------------------------------------
int visfd_hip_gengauss3d_halfwidths(const float width[3], float m_exp, float truncate_ratio, float truncate_threshold,
                                    int halfwidth_out[3]) {
  VH_REQUIRE(width && halfwidth_out, "null argument");
  host_gengauss3d_halfwidths(width, m_exp, truncate_ratio, truncate_threshold, halfwidth_out);
  return VISFD_HIP_OK;
}

int visfd_hip_gengauss3d_table(const float width[3], float m_exp, const int halfwidth[3], float* table, int64_t cap,
                               int64_t* n, float* A_out) {
  VH_REQUIRE(width && n && cap >= 0 && (cap == 0 || table), "bad argument");
  VH_TRY(check_halfwidths(halfwidth));
  *n = table_size(halfwidth);
  if (cap == 0 && !A_out) return VISFD_HIP_OK;
  if (cap > 0 && cap < *n) return fail(VISFD_HIP_ECAPACITY, "filter table has more entries than cap");
  std::vector<float> own;
  if (cap == 0) {
    own.resize((size_t)*n);
    table = own.data();
  }
  host_gengauss3d_table(width, m_exp, halfwidth, table, A_out);
  return VISFD_HIP_OK;
}

int visfd_hip_dogg3d_table(const float width_a[3], const float width_b[3], float m_exp, float n_exp, float truncate_ratio,
                           float truncate_threshold, int halfwidth_out[3], float* table, int64_t cap, int64_t* n,
                           float* A_out, float* B_out) {
  VH_REQUIRE(width_a && width_b && halfwidth_out && n && cap >= 0 && (cap == 0 || table), "bad argument");
  int ha[3], hb[3];
  VH_TRY(window_of(width_a, m_exp, truncate_ratio, truncate_threshold, ha));
  VH_TRY(window_of(width_b, n_exp, truncate_ratio, truncate_threshold, hb));
  for (int d = 0; d < 3; d++) halfwidth_out[d] = std::max(ha[d], hb[d]);
  *n = table_size(halfwidth_out);
  if (cap > 0 && cap < *n) return fail(VISFD_HIP_ECAPACITY, "filter table has more entries than cap");
  host_dogg3d_table(width_a, width_b, m_exp, n_exp, truncate_ratio, truncate_threshold, halfwidth_out, table, cap, A_out,
                    B_out);
  return VISFD_HIP_OK;
}

// ---- g2: Filter3D::Apply -------------------------------------------------------------------------------------------
int visfd_hip_filter3d_dev(visfd_hip_ctx* ctx, const float* src, float* dst, const float* mask, int64_t nx, int64_t ny,
                           int64_t nz, const float* table, const int halfwidth[3], int normalize, float* den_out) {
  VH_REQUIRE(ctx, "null context");
  VH_HIP(hipSetDevice(ctx->device));
  return dev_filter3d(ctx, src, dst, mask, nx, ny, nz, table, halfwidth, normalize != 0, den_out);
}

int visfd_hip_filter3d(visfd_hip_ctx* ctx, const float* src, float* dst, const float* mask, int64_t nx, int64_t ny,
                       int64_t nz, const float* table, const int halfwidth[3], int normalize, float* den_out) {
  VH_REQUIRE(table, "null argument");
  VH_TRY(check_halfwidths(halfwidth));
  VH_TRY(filter3d_check(ctx, src, dst, mask, nx, ny, nz, den_out));
  return stage_filter(ctx, src, dst, mask, nx, ny, nz, false, [&](const float* ds, float* dd, const float* dm) {
    const Stage st = {ctx, (size_t)(nx * ny * nz)};
    float* dden = nullptr;
    if (den_out) VH_TRY(st.out(WS_H2D_3, &dden));
    VH_TRY(dev_filter3d(ctx, ds, dd, dm, nx, ny, nz, table, halfwidth, normalize != 0, dden));
    if (den_out) VH_TRY(st.down(den_out, dden));
    return (int)VISFD_HIP_OK;
  });
}

int visfd_hip_filter3d_last_path(visfd_hip_ctx* ctx, int* path) {
  VH_REQUIRE(ctx && path, "null argument");
  *path = ctx->f3d_last_path;
  return VISFD_HIP_OK;
}

// ---- g3: HandleGGauss: GenFilterGenGauss3D(width, m, halfwidth) applied (handlers.cpp:167-187) -----------------------
int visfd_hip_apply_ggauss_dev(visfd_hip_ctx* ctx, const float* src, float* dst, const float* mask, int64_t nx, int64_t ny,
                               int64_t nz, const float width[3], float m_exp, const int halfwidth[3], int normalize,
                               float* A_out) {
  VH_REQUIRE(ctx && width, "null argument");
  VH_TRY(check_halfwidths(halfwidth));
  VH_TRY(filter3d_check(ctx, src, dst, mask, nx, ny, nz, nullptr));
  VH_HIP(hipSetDevice(ctx->device));
  std::vector<float> t((size_t)table_size(halfwidth));
  host_gengauss3d_table(width, m_exp, halfwidth, t.data(), A_out);
  return dev_filter3d(ctx, src, dst, mask, nx, ny, nz, t.data(), halfwidth, normalize != 0, nullptr);
}

int visfd_hip_apply_ggauss(visfd_hip_ctx* ctx, const float* src, float* dst, const float* mask, int64_t nx, int64_t ny,
                           int64_t nz, const float width[3], float m_exp, const int halfwidth[3], int normalize,
                           float* A_out) {
  VH_REQUIRE(width, "null argument");
  VH_TRY(check_halfwidths(halfwidth));
  VH_TRY(filter3d_check(ctx, src, dst, mask, nx, ny, nz, nullptr));
  return stage_filter(ctx, src, dst, mask, nx, ny, nz, false, [&](const float* ds, float* dd, const float* dm) {
    return visfd_hip_apply_ggauss_dev(ctx, ds, dd, dm, nx, ny, nz, width, m_exp, halfwidth, normalize, A_out);
  });
}

// ---- g4: HandleDogg: GenFilterDogg3D(width_a, width_b, m, n, ratio, threshold) applied, never normalised
//      (handlers.cpp:265-293) -------------------------------------------------------------------------------------------
int visfd_hip_apply_dogg_dev(visfd_hip_ctx* ctx, const float* src, float* dst, const float* mask, int64_t nx, int64_t ny,
                             int64_t nz, const float width_a[3], const float width_b[3], float m_exp, float n_exp,
                             float truncate_ratio, float truncate_threshold, float* A_out, float* B_out) {
  VH_REQUIRE(ctx, "null context");
  VH_TRY(filter3d_check(ctx, src, dst, mask, nx, ny, nz, nullptr));
  int hw[3];
  int64_t n = 0;
  VH_TRY(visfd_hip_dogg3d_table(width_a, width_b, m_exp, n_exp, truncate_ratio, truncate_threshold, hw, nullptr, 0, &n,
                                nullptr, nullptr));
  VH_TRY(check_halfwidths(hw));
  VH_HIP(hipSetDevice(ctx->device));
  std::vector<float> t((size_t)n);
  VH_TRY(visfd_hip_dogg3d_table(width_a, width_b, m_exp, n_exp, truncate_ratio, truncate_threshold, hw, t.data(), n, &n,
                                A_out, B_out));
  return dev_filter3d(ctx, src, dst, mask, nx, ny, nz, t.data(), hw, false, nullptr);
}

int visfd_hip_apply_dogg(visfd_hip_ctx* ctx, const float* src, float* dst, const float* mask, int64_t nx, int64_t ny,
                         int64_t nz, const float width_a[3], const float width_b[3], float m_exp, float n_exp,
                         float truncate_ratio, float truncate_threshold, float* A_out, float* B_out) {
  VH_TRY(filter3d_check(ctx, src, dst, mask, nx, ny, nz, nullptr));
  return stage_filter(ctx, src, dst, mask, nx, ny, nz, false, [&](const float* ds, float* dd, const float* dm) {
    return visfd_hip_apply_dogg_dev(ctx, ds, dd, dm, nx, ny, nz, width_a, width_b, m_exp, n_exp, truncate_ratio,
                                    truncate_threshold, A_out, B_out);
  });
}

// ---- g5: LocalFluctuations for any exponent (filter3d.hpp:1713-1847) ------------------------------------------------
// w = GenFilterGenGauss3D(sigma, exponent, ratio) times (float)(1.0 / wpeak) (the reciprocal in double, the product per
// entry in float); P = src - W(src); P = P * P; W(P) with the same mask and flag; times wpeak, clamped at 0, square root.
// Exponent 2 forwards to the separable path, as the reference does.
int visfd_hip_local_fluctuations_gen_dev(visfd_hip_ctx* ctx, const float* src, float* dst, const float* mask, int64_t nx,
                                         int64_t ny, int64_t nz, const float sigma[3], float exponent, float truncate_ratio,
                                         int normalize) {
  VH_REQUIRE(ctx && src && dst && sigma, "null argument");
  if (exponent == 2.0f)
    return visfd_hip_local_fluctuations_dev(ctx, src, dst, mask, nx, ny, nz, sigma, exponent, truncate_ratio, normalize);
  VH_TRY(filter3d_check(ctx, src, dst, mask, nx, ny, nz, nullptr));
  VH_REQUIRE(truncate_ratio >= 0.0f, "LocalFluctuations: the truncation ratio must not be negative");
  int hw[3];
  VH_TRY(window_of(sigma, exponent, truncate_ratio, 0.0f, hw));
  VH_HIP(hipSetDevice(ctx->device));
  const i64 n = nx * ny * nz;
  std::vector<float> w((size_t)table_size(hw));
  float wpeak = 0.0f;
  host_gengauss3d_table(sigma, exponent, hw, w.data(), &wpeak);
  const float scale = (float)(1.0 / wpeak);
  for (size_t k = 0; k < w.size(); k++) w[k] *= scale;
  float* p2 = nullptr;
  VH_TRY(ws(ctx, WS_C, (size_t)n, &p2));
  VH_TRY(dev_filter3d(ctx, src, dst, mask, nx, ny, nz, w.data(), hw, normalize != 0, nullptr));   // local average
  VH_TRY(dev_sub_square(ctx, src, dst, p2, n));                                                    // (src - avg)^2
  VH_TRY(dev_filter3d(ctx, p2, dst, mask, nx, ny, nz, w.data(), hw, normalize != 0, nullptr));    // its local average
  return dev_scale_clamp_sqrt(ctx, dst, n, wpeak);
}

int visfd_hip_local_fluctuations_gen(visfd_hip_ctx* ctx, const float* src, float* dst, const float* mask, int64_t nx,
                                     int64_t ny, int64_t nz, const float sigma[3], float exponent, float truncate_ratio,
                                     int normalize) {
  VH_REQUIRE(ctx && src && dst && sigma, "null argument");
  VH_TRY(filter3d_check(ctx, src, dst, mask, nx, ny, nz, nullptr));
  return stage_filter(ctx, src, dst, mask, nx, ny, nz, false, [&](const float* ds, float* dd, const float* dm) {
    return visfd_hip_local_fluctuations_gen_dev(ctx, ds, dd, dm, nx, ny, nz, sigma, exponent, truncate_ratio, normalize);
  });
}

}  // extern "C"
