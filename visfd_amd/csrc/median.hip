// median.hip -- the median filter with an arbitrary footprint: Median / MedianSphere (reference lib/visfd/filter3d.hpp:
// 1577-1674).  The reference's footprint loop never ends once a neighbour is skipped (its `continue` does not advance
// the iterator), so the contract is the one DESIGN.md section 4.9 states: for a voxel with mask != 0 the values at voxel +
// entry that lie inside the image and have mask != 0 are collected (n of them), and the one of rank n / 2 (0-based,
// ascending) is written; n == 0 writes +0.0f; voxels with mask == 0 are not written.
//
// Selection, not accumulation: a float with bits u has the key (sign set) ? ~u : u | 0x80000000, and keys compare as
// unsigned integers (operator< on finite values and infinities; -0 before +0; NaNs by sign and payload beyond the
// infinities).  The key of rank r among a voxel's candidates is the largest v with #{keys < v} <= r, found bit by bit from
// the top: one walk over the footprint per bit.  Every 32-bit pattern is a legal key, so an excluded cell cannot be told
// by its key: both kernels count a voxel's n on its own, and may then let excluded cells carry the key 0xffffffff, which no
// candidate exceeds (ranks below n are not moved by them).  A first walk takes the smallest and largest key the voxel sees:
// the bits above their highest difference are the answer's, and the rounds start below them (a constant neighbourhood
// needs none).
//
// Two kernels, both exact:
//  median_tiled_kernel    footprints whose bounding box fits LDS: a workgroup of 256 threads owns 64 x 4 x 4 outputs and
//                         loads their cells (outputs + bounding box) once, as keys, with one validity bit per cell behind
//                         them; a thread owns a column of 4 outputs.  The entries' LDS offsets are the same for every lane
//                         (scalar loads), and a wave's 64 lanes read 64 consecutive words.  Footprints of 7, 19, 33, 81
//                         and 123 entries (the balls of radius 1, 1.5, 2, 2.5, 3) are compiled with the entry count: an
//                         output's keys are read into registers once and sorted there by a network instead of bisected
//  median_general_kernel  any footprint: neighbours from global memory, bounds and mask tested per entry (a workgroup whose
//                         whole reach lies inside an unmasked image skips the tests)
#include <algorithm>
#include <vector>

#include "common.hpp"
#include "wave.hpp"

namespace vh {

namespace {

constexpr int TX = 64, TY = 4, TZ = 4;   // the tiled kernel's outputs per workgroup (block 64 x 4, TZ outputs per thread)
constexpr int GX = 64, GY = 4;           // the general kernel's block: 64 x 4 voxels of one plane
constexpr size_t TILED_LDS_BYTES = 64 * 1024;   // the tiled kernel's budget: balls up to radius 5 (74 x 14 x 14 cells)

__device__ __forceinline__ uint32_t key_of(uint32_t u) { return (u & 0x80000000u) ? ~u : (u | 0x80000000u); }
__device__ __forceinline__ uint32_t bits_of(uint32_t k) { return (k & 0x80000000u) ? (k & 0x7fffffffu) : ~k; }

// the bits of the answer that the voxel's smallest and largest key share; *top: the highest bit left to decide (-1: none)
__device__ __forceinline__ uint32_t shared_prefix(uint32_t lo, uint32_t hi, int* top) {
  const uint32_t d = lo ^ hi;
  if (!d) {
    *top = -1;
    return lo;
  }
  *top = 31 - __clz(d);
  return hi & ~((2u << *top) - 1u);
}

// Small footprints: the NREG keys of one output in registers, sorted by Batcher's merge exchange (Knuth 5.2.2 M; valid
// for any count; 16, 98, 246, 864, 1416 compare-exchanges of one v_min_u32 and one v_max_u32 for 7, 19, 33, 81, 123 keys),
// then the key of the rank picked.  Excluded cells hold 0xffffffff and end up behind every rank below n.
template <int NREG>
__device__ __forceinline__ uint32_t select_in_registers(const uint32_t* p, const int* __restrict__ off, int rank) {
  uint32_t k[NREG];
#pragma unroll
  for (int j = 0; j < NREG; j++) k[j] = p[off[j]];
#pragma unroll
  for (int P = 1; P < NREG; P *= 2)
#pragma unroll
    for (int K = P; K >= 1; K /= 2)
#pragma unroll
      for (int J = K % P; J <= NREG - 1 - K; J += 2 * K)
#pragma unroll
        for (int I = 0; I <= (K - 1 < NREG - J - K - 1 ? K - 1 : NREG - J - K - 1); I++)
          if ((I + J) / (2 * P) == (I + J + K) / (2 * P)) {
            const uint32_t a = k[I + J], b = k[I + J + K];
            k[I + J] = min(a, b);
            k[I + J + K] = max(a, b);
          }
  uint32_t res = k[0];
#pragma unroll
  for (int j = 1; j < NREG; j++) res = (rank == j) ? k[j] : res;
  return res;
}

// NREG > 0: the footprint has exactly NREG entries and an output's keys are held in registers; 0: any entry count, every
// walk reads LDS
template <int NREG>
__global__ void __launch_bounds__(TX * TY)
median_tiled_kernel(const uint32_t* __restrict__ src, uint32_t* __restrict__ dst, const float* __restrict__ mask,
                    const int* __restrict__ off, int n, int nx, int ny, int nz, int lox, int loy, int loz, int W, int H,
                    int D) {
  extern __shared__ uint32_t lds[];
  const int cells = W * H * D;
  uint32_t* keys = lds;            // cell (cx, cy, cz) at cx + W * (cy + H * cz): voxel (x0 + lox + cx, ...)
  uint32_t* vbits = lds + cells;   // bit c & 31 of word c >> 5: cell c is inside the image and not masked
  const int tx = threadIdx.x, ty = threadIdx.y, tid = ty * TX + tx;
  const int x0 = blockIdx.x * TX, y0 = blockIdx.y * TY, z0 = blockIdx.z * TZ;
  const i64 plane = (i64)nx * ny;
  const int cx0 = x0 + lox, cy0 = y0 + loy, cz0 = z0 + loz;
  // no cell of the workgroup is excluded: every voxel collects all n entries
  const bool all_valid = !mask && cx0 >= 0 && cy0 >= 0 && cz0 >= 0 && cx0 + W <= nx && cy0 + H <= ny && cz0 + D <= nz;
  for (int base = 0; base < cells; base += TX * TY) {   // a wave takes 64 consecutive cells: two words of validity bits
    const int c = base + tid;
    bool valid = false;
    if (c < cells) {
      const int cx = c % W, r = c / W, cy = r % H, cz = r / H;
      const int X = cx0 + cx, Y = cy0 + cy, Z = cz0 + cz;
      uint32_t k = 0xffffffffu;
      if ((unsigned)X < (unsigned)nx && (unsigned)Y < (unsigned)ny && (unsigned)Z < (unsigned)nz) {
        const i64 g = (i64)Z * plane + (i64)Y * nx + X;
        if (!mask || !(mask[g] == 0.0f)) {
          valid = true;
          k = key_of(src[g]);
        }
      }
      keys[c] = k;
    }
    const unsigned long long b = __ballot(valid);
    // base is the same for every thread, so whole waves take every trip; TX is WAVE, so wave_lane() is the lane
    if (wave_lane() == 0 && c < cells) {   // c is a multiple of 64 here; the bit array is padded to whole pairs of words
      vbits[c >> 5] = (uint32_t)b;
      vbits[(c >> 5) + 1] = (uint32_t)(b >> 32);
    }
  }
  __syncthreads();
  const int x = x0 + tx, y = y0 + ty;
  if (x >= nx || y >= ny) return;
  for (int o = 0; o < TZ; o++) {
    const int z = z0 + o;
    if (z >= nz) break;
    const i64 i = (i64)z * plane + (i64)y * nx + x;
    if (mask && mask[i] == 0.0f) continue;
    const int cb = tx + W * (ty + H * o);   // the cell of entry k is cb + off[k]
    int cnt = n;
    if (!all_valid) {
      cnt = 0;
      for (int k = 0; k < n; k++) {
        const int c = cb + off[k];
        cnt += (vbits[c >> 5] >> (c & 31)) & 1u;
      }
    }
    if (cnt == 0) {
      dst[i] = 0u;   // +0.0f
      continue;
    }
    const int rank = cnt >> 1;
    const uint32_t* p = keys + cb;
    if (NREG > 0) {
      dst[i] = bits_of(select_in_registers<(NREG > 0 ? NREG : 1)>(p, off, rank));
      continue;
    }
    uint32_t lo = 0xffffffffu, hi = 0u;
#pragma unroll 8
    for (int k = 0; k < n; k++) {
      const uint32_t v = p[off[k]];
      lo = min(lo, v);
      hi = max(hi, v);
    }
    int top;
    uint32_t res = shared_prefix(lo, hi, &top);
    for (int b = top; b >= 0; b--) {
      const uint32_t cand = res | (1u << b);
      int below = 0;
#pragma unroll 8
      for (int k = 0; k < n; k++) below += p[off[k]] < cand;
      if (below <= rank) res = cand;
    }
    dst[i] = bits_of(res);
  }
}

// the key of the neighbour `e` of voxel (x, y, z); false: outside the image or masked (never with CHECK = false)
template <bool CHECK>
__device__ __forceinline__ bool neighbour_key(const uint32_t* __restrict__ src, const float* __restrict__ mask, int4 e,
                                              int x, int y, int z, int nx, int ny, int nz, i64 plane, uint32_t* key) {
  const int X = x + e.x, Y = y + e.y, Z = z + e.z;
  if (CHECK && ((unsigned)X >= (unsigned)nx || (unsigned)Y >= (unsigned)ny || (unsigned)Z >= (unsigned)nz)) return false;
  const i64 g = (i64)Z * plane + (i64)Y * nx + X;
  if (CHECK && mask && mask[g] == 0.0f) return false;
  *key = key_of(src[g]);
  return true;
}

template <bool CHECK>
__device__ __forceinline__ uint32_t median_walk(const uint32_t* __restrict__ src, const float* __restrict__ mask,
                                                const int4* __restrict__ tab, int n, int x, int y, int z, int nx, int ny,
                                                int nz, i64 plane) {
  int cnt = 0;
  uint32_t lo = 0xffffffffu, hi = 0u, v;
  for (int k = 0; k < n; k++) {
    if (!neighbour_key<CHECK>(src, mask, tab[k], x, y, z, nx, ny, nz, plane, &v)) continue;
    cnt++;
    lo = min(lo, v);
    hi = max(hi, v);
  }
  if (cnt == 0) return 0u;   // +0.0f
  const int rank = cnt >> 1;
  int top;
  uint32_t res = shared_prefix(lo, hi, &top);
  for (int b = top; b >= 0; b--) {
    const uint32_t cand = res | (1u << b);
    int below = 0;
    for (int k = 0; k < n; k++)
      if (neighbour_key<CHECK>(src, mask, tab[k], x, y, z, nx, ny, nz, plane, &v)) below += v < cand;
    if (below <= rank) res = cand;
  }
  return bits_of(res);
}

__global__ void __launch_bounds__(GX * GY)
median_general_kernel(const uint32_t* __restrict__ src, uint32_t* __restrict__ dst, const float* __restrict__ mask,
                      const int4* __restrict__ tab, int n, int nx, int ny, int nz, int lox, int loy, int loz, int hix,
                      int hiy, int hiz) {
  const int x0 = blockIdx.x * GX, y0 = blockIdx.y * GY;
  const int x = x0 + threadIdx.x, y = y0 + threadIdx.y;
  const bool mine = x < nx && y < ny;
  const i64 plane = (i64)nx * ny;
  // no mask, every voxel of the workgroup in the image, and every neighbour the footprint reaches from them
  const bool xy_inside = !mask && x0 + GX <= nx && y0 + GY <= ny && x0 + lox >= 0 && y0 + loy >= 0 &&
                         x0 + GX - 1 + hix < nx && y0 + GY - 1 + hiy < ny;
  for (int z = blockIdx.z; z < nz; z += gridDim.z) {
    if (!mine) continue;
    const i64 i = (i64)z * plane + (i64)y * nx + x;
    if (mask && mask[i] == 0.0f) continue;
    if (xy_inside && z + loz >= 0 && z + hiz < nz)
      dst[i] = median_walk<false>(src, mask, tab, n, x, y, z, nx, ny, nz, plane);
    else
      dst[i] = median_walk<true>(src, mask, tab, n, x, y, z, nx, ny, nz, plane);
  }
}

enum class MedianRoute { Tiled, General };

// The routes a footprint may take under the context's options, in the order they are tried; returns their number.
int median_routes(const visfd_hip_options& opt, MedianRoute routes[2]) {
  int n = 0;
  if (!opt.median_general) routes[n++] = MedianRoute::Tiled;   // declines a bounding box beyond its LDS budget
  routes[n++] = MedianRoute::General;                          // takes everything
  return n;
}

constexpr int MEDIAN_DECLINED = -1;

size_t tiled_lds_bytes(const MedianTab& mt) {
  const size_t cells = (size_t)mt.W * mt.H * mt.D;
  return sizeof(uint32_t) * (cells + 2 * ((cells + 63) / 64));
}

int median_tiled(visfd_hip_ctx* ctx, const uint32_t* src, uint32_t* dst, const float* mask, i64 nx, i64 ny, i64 nz,
                 const MedianTab& mt) {
  const size_t lds = tiled_lds_bytes(mt);
  const dim3 grid((unsigned)((nx + TX - 1) / TX), (unsigned)((ny + TY - 1) / TY), (unsigned)((nz + TZ - 1) / TZ));
  if (lds > TILED_LDS_BYTES || grid.y > 65535u || grid.z > 65535u) return MEDIAN_DECLINED;
  const int* off = static_cast<const int*>(ctx->slot_ptr[WS_MEDIAN_TAB]) + 4 * mt.n;
#define VH_MEDIAN_LAUNCH(NREG)                                                                                           \
  median_tiled_kernel<NREG><<<grid, dim3(TX, TY), lds, ctx->stream>>>(src, dst, mask, off, (int)mt.n, (int)nx, (int)ny,   \
                                                                      (int)nz, mt.lo[0], mt.lo[1], mt.lo[2], mt.W, mt.H, mt.D)
  switch (mt.n) {   // the balls of radius 1, 1.5, 2, 2.5 and 3
    case 7: VH_MEDIAN_LAUNCH(7); break;
    case 19: VH_MEDIAN_LAUNCH(19); break;
    case 33: VH_MEDIAN_LAUNCH(33); break;
    case 81: VH_MEDIAN_LAUNCH(81); break;
    case 123: VH_MEDIAN_LAUNCH(123); break;
    default: VH_MEDIAN_LAUNCH(0); break;
  }
#undef VH_MEDIAN_LAUNCH
  VH_HIP(hipGetLastError());
  ctx->median_last_path = VISFD_HIP_MEDIAN_PATH_TILED;
  return VISFD_HIP_OK;
}

int median_general(visfd_hip_ctx* ctx, const uint32_t* src, uint32_t* dst, const float* mask, i64 nx, i64 ny, i64 nz,
                   const MedianTab& mt) {
  const int4* tab = static_cast<const int4*>(ctx->slot_ptr[WS_MEDIAN_TAB]);
  const dim3 grid((unsigned)((nx + GX - 1) / GX), (unsigned)((ny + GY - 1) / GY), (unsigned)(nz < 65535 ? nz : 65535));
  VH_REQUIRE(grid.y <= 65535u, "median: ny must be at most 262140");
  median_general_kernel<<<grid, dim3(GX, GY), 0, ctx->stream>>>(src, dst, mask, tab, (int)mt.n, (int)nx, (int)ny, (int)nz,
                                                                mt.lo[0], mt.lo[1], mt.lo[2], mt.hi[0], mt.hi[1],
                                                                mt.hi[2]);
  VH_HIP(hipGetLastError());
  ctx->median_last_path = VISFD_HIP_MEDIAN_PATH_GENERAL;
  return VISFD_HIP_OK;
}

}  // namespace

// puts the footprint in slot WS_MEDIAN_TAB: n entries (dx, dy, dz, 0), then the n cell offsets of the tiled kernel's LDS
// image, (dx - lox) + W * ((dy - loy) + H * (dz - loz)); a footprint equal to the one already there is not sent again
int median_put_table(visfd_hip_ctx* ctx, const int* dxyz, i64 n, MedianTab* mt) {
  VH_REQUIRE(n >= 1 && n <= VISFD_HIP_MEDIAN_MAX_ENTRIES, "median: a footprint has between 1 and 32768 entries");
  VH_REQUIRE(dxyz, "null argument");
  mt->n = n;
  for (i64 k = 0; k < n; k++)
    for (int d = 0; d < 3; d++) {
      const int v = dxyz[3 * k + d];
      VH_REQUIRE(v >= -VISFD_HIP_MEDIAN_MAX_RADIUS && v <= VISFD_HIP_MEDIAN_MAX_RADIUS,
                 "median: footprint offsets must be within 16 voxels of the centre");
      mt->lo[d] = (k == 0 || v < mt->lo[d]) ? v : mt->lo[d];
      mt->hi[d] = (k == 0 || v > mt->hi[d]) ? v : mt->hi[d];
    }
  mt->W = TX + mt->hi[0] - mt->lo[0];
  mt->H = TY + mt->hi[1] - mt->lo[1];
  mt->D = TZ + mt->hi[2] - mt->lo[2];
  std::vector<int> t((size_t)(5 * n));
  for (i64 k = 0; k < n; k++) {
    const int* e = dxyz + 3 * k;
    for (int d = 0; d < 3; d++) t[4 * k + d] = e[d];
    t[4 * k + 3] = 0;
    t[4 * n + k] = (e[0] - mt->lo[0]) + mt->W * ((e[1] - mt->lo[1]) + mt->H * (e[2] - mt->lo[2]));
  }
  const size_t bytes = sizeof(int) * t.size();
  if (ws_holds(ctx, WS_MEDIAN_TAB, t.data(), bytes)) return VISFD_HIP_OK;
  return ws_put(ctx, WS_MEDIAN_TAB, t.data(), bytes, t.data(), bytes);
}

int median_run(visfd_hip_ctx* ctx, const float* src, float* dst, const float* mask, i64 nx, i64 ny, i64 nz,
               const MedianTab& mt) {
  VH_REQUIRE(nx < (1 << 30) && ny < (1 << 30) && nz < (1 << 30), "median: image dimensions must be below 2^30");
  VH_REQUIRE(ctx->slot_ptr[WS_MEDIAN_TAB] && !ctx->slot_key[WS_MEDIAN_TAB].empty(), "median: no footprint on the device");
  const uint32_t* s = reinterpret_cast<const uint32_t*>(src);   // bit patterns throughout: a median has no arithmetic
  uint32_t* d = reinterpret_cast<uint32_t*>(dst);
  MedianRoute routes[2];
  const int nroutes = median_routes(ctx->opt, routes);
  int rc = MEDIAN_DECLINED;
  for (int i = 0; i < nroutes && rc == MEDIAN_DECLINED; i++)
    rc = routes[i] == MedianRoute::Tiled ? median_tiled(ctx, s, d, mask, nx, ny, nz, mt)
                                         : median_general(ctx, s, d, mask, nx, ny, nz, mt);
  return rc;
}

}  // namespace vh
