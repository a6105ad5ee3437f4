// tv_list.hip -- THE SENDER LISTS of tv_box.hip's kernels, built once per launch.
//
// For every listed plane z and every tile column tx (TX = 16 receiver columns), the salient, unmasked senders of the columns
// [TX tx - h, TX tx + TX + h) -- everything a tile of that column can reach in x -- as one list in DESCENDING (y, x) (the order
// the vote kernel's row-range culling needs), 20 bytes per entry: float4 {saliency * 1/4 or 1/2 (* mask value), normal} and one
// word {x - (TX tx - h), y << 8}.  A sender appears in the lists of the tile columns that reach it (2.5 on average at h = 12).
// rows[(zl (ny + 1) + y) ntx + tx]: index (into the global entry arrays) of the first entry of list (zl, tx) with a row
// below y -- so the entries of the rows [ylo, yhi] are [rows[.. yhi + 1 ..], rows[.. ylo ..]).
// Three kernels: count per (plane, row, tile column); suffix sums per (plane, tile column) with one atomic add per list for
// its place in the global arrays; write.  A WAVE takes one image row: its salient flags as a bit mask in LDS, every
// window's count / every sender's place in its windows by popcounts over at most four words.
#include <algorithm>

#include "tv_common.hpp"

namespace vh {

using namespace box_tile;

namespace {

using ListGeo = TvListGeo;
constexpr int LNT = 256;
constexpr int LWORDS_MAX = TV_LIST_MAX_NX / 32;

__device__ __forceinline__ unsigned popc_range(const unsigned* w, int lo, int hi) {   // set bits of [lo, hi), hi - lo <= 96
  unsigned c = 0;
  for (int i = lo >> 5; i <= (hi - 1) >> 5 && lo < hi; i++) {
    unsigned m = w[i];
    if (i == (lo >> 5)) m &= ~0u << (lo & 31);
    if (i == ((hi - 1) >> 5) && (hi & 31)) m &= ~0u >> (32 - (hi & 31));
    c += (unsigned)__builtin_popcount(m);
  }
  return c;
}

template <bool WRITE, int MODE>
__global__ void __launch_bounds__(LNT)
tvl_row_kernel(const float* __restrict__ sal, const float* __restrict__ dir, const float* __restrict__ mask_src, ListGeo g,
               unsigned* __restrict__ rows, float4* __restrict__ ent, unsigned* __restrict__ pos,
               unsigned* __restrict__ neg_flag /* count pass: set if a listed saliency (times its mask value) is not positive */,
               int fold /* write pass: records {c, a n} instead of {s, n} (vote_fma) */,
               const float* __restrict__ thr_dev /* nullable: sal is uncut, and a voxel below *thr_dev is not salient (ridge.hip:
                                                    ridge_directions_kernel has the same predicate) */) {
  // ONE WAVE PER IMAGE ROW (no workgroup barrier: a wave's bit mask is its own): its salient flags as a bit mask in LDS,
  // 64 voxels per ballot.  A wave is a chain of memory round trips, so every phase requests LB chunks' worth of loads before
  // it uses the first (the loops are otherwise one round trip per 64 voxels: 8 ms for the write pass at 1024^3)
  constexpr int LB = 8;
  __shared__ unsigned bits_all[LNT / 64][LWORDS_MAX + 4];
  __shared__ unsigned base_all[WRITE ? LNT / 64 : 1][WRITE ? LWORDS_MAX * 2 + 4 : 1];   // write pass: the row's first entry per list
  __shared__ unsigned cum_all[WRITE ? LNT / 64 : 1][WRITE ? LWORDS_MAX / 2 + 4 : 1];    // write pass: salient voxels before chunk c
  const int wave = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6), lane = threadIdx.x & 63;
  const i64 r = (i64)blockIdx.x * (LNT / 64) + wave;      // row number among the listed rows
  if (r >= (i64)g.nzl * g.ny) return;                      // (uniform per wave)
  unsigned* const bits = bits_all[wave];
  const int y = (int)(r % g.ny), zl = (int)(r / g.ny);
  const i64 plane = (i64)g.nx * g.ny, nvox = plane * g.nz;
  const i64 row = (i64)(g.zl0 + zl) * plane + (i64)y * g.nx;
  const int nchunks = (g.nx + 63) >> 6;
  unsigned* const rrow = rows + ((size_t)zl * (size_t)(g.ny + 1) + (size_t)y) * (size_t)g.ntx;
  if (WRITE) {   // (requested first: used after the flags)
    unsigned* const base = base_all[WRITE ? wave : 0];
    for (int tx = lane; tx < g.ntx; tx += 64) base[tx] = rrow[g.ntx + tx];
  }
  unsigned any = 0, total = 0;
  unsigned* const cum = cum_all[WRITE ? wave : 0];
  const bool cut = thr_dev != nullptr;
  const float thr = cut ? *thr_dev : 0.0f;
  for (int c0 = 0; c0 < nchunks; c0 += LB) {   // uniform
    float v[LB], m[LB];
#pragma unroll
    for (int k = 0; k < LB; k++) {
      const int x = 64 * (c0 + k) + lane;
      v[k] = x < g.nx ? sal[row + x] : 0.0f;
      m[k] = (mask_src && x < g.nx) ? mask_src[row + x] : 1.0f;
    }
#pragma unroll
    for (int k = 0; k < LB; k++) {
      if (c0 + k >= nchunks) break;   // uniform
      const bool f = v[k] != 0.0f && m[k] != 0.0f && !(cut && v[k] < thr);
      const unsigned long long bal = __builtin_amdgcn_ballot_w64(f);
      if (lane == 0) {
        bits[2 * (c0 + k)] = (unsigned)bal;
        bits[2 * (c0 + k) + 1] = (unsigned)(bal >> 32);
        if (WRITE) cum[c0 + k] = total;
      }
      any |= (unsigned)bal | (unsigned)(bal >> 32);
      if (WRITE) total += (unsigned)__builtin_popcountll(bal);
      if (!WRITE && f) {
        const float s = mask_src ? v[k] * m[k] : v[k];
        if (!(s > 0.0f)) atomicOr(neg_flag, 1u);   // (rare: negative peak heights, masks with negative values, NaN)
        if (!(__builtin_fabsf(s) <= 3.402823466e38f)) atomicOr(neg_flag, 2u);   // non-finite: the exact form declines
        if (mask_src && m[k] != 1.0f) atomicOr(neg_flag, 4u);   // a weighted source mask: its value is a factor of the exact vote
      }
    }
  }
  __builtin_amdgcn_wave_barrier();
  asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
  if (!WRITE) {
    for (int tx = lane; tx < g.ntx; tx += 64)
      rrow[tx] = any ? popc_range(bits, max(TX * tx - g.h, 0), min(TX * tx + TX + g.h, g.nx)) : 0u;
    return;
  }
  if (!any) return;   // (uniform)
  const unsigned* const base = base_all[WRITE ? wave : 0];
  // lane j takes the row's j-th salient voxel (all lanes busy: the fold's double-precision roots at 3 live lanes per chunk
  // were most of this pass)
  for (unsigned j0 = 0; j0 < total; j0 += 64) {   // uniform
    const unsigned j = j0 + lane;
    if (j >= total) break;
    int lo = 0, hi = nchunks;
    while (hi - lo > 1) {
      const int mid = (lo + hi) >> 1;
      if (cum[mid] <= j) lo = mid; else hi = mid;
    }
    unsigned k = j - cum[lo];
    unsigned w = bits[2 * lo];
    int x = 64 * lo;
    {
      const unsigned t = (unsigned)__builtin_popcount(w);
      if (k >= t) { k -= t; x += 32; w = bits[2 * lo + 1]; }
    }
#pragma unroll
    for (int sft = 16; sft >= 1; sft >>= 1) {
      const unsigned t = (unsigned)__builtin_popcount(w & ((1u << sft) - 1u));
      if (k >= t) { k -= t; x += sft; w >>= sft; }
    }
    // (MODE 1: the exact form's lists carry the saliency itself)
    float4 q = make_float4(sal[row + x] * (MODE == 0 ? 0.25f : (MODE == 2 ? 0.5f : 1.0f)), dir[row + x], dir[nvox + row + x], dir[2 * nvox + row + x]);
    if (mask_src) q.x = q.x * mask_src[row + x];
    if (fold) {   // a = s^(1/6) (exponent 4) or s^(1/4) (exponent 2), rounded once from double
      const double r2 = sqrt((double)q.x);
      const float a = (float)(MODE == 0 ? cbrt(r2) : sqrt(r2));
      q = make_float4(2.0f * a * a, a * q.y, a * q.z, a * q.w);
    }
    // tile columns whose window holds x: TX tx - h <= x < TX tx + TX + h
    const int t0 = max((x - TX - g.h) / TX + ((x - TX - g.h) >= 0 ? 1 : 0), 0);
    const int t1 = min((x + g.h) / TX, g.ntx - 1);
    for (int tx = t0; tx <= t1; tx++) {
      const int lo_x = TX * tx - g.h, hi_x = min(TX * tx + TX + g.h, g.nx);
      if (x < lo_x || x >= hi_x) continue;
      // rows[.. y + 1 ..] = first entry of the rows below y + 1 = first entry of row y; within the row: descending x
      const unsigned idx = base[tx] + popc_range(bits, x + 1, hi_x);
      ent[idx] = q;
      pos[idx] = (unsigned)(x - lo_x) | ((unsigned)y << 8);
    }
  }
}

// one thread per list (zl, tx): counts -> offsets.  Before: rows[zl][y][tx] = entries of row y (y < ny).  After:
// rows[zl][y][tx] = base + (entries of the rows >= y): the index behind row y's last entry... see the header comment; the
// list's place `base` in the global arrays comes from one atomic add (the lists' order in memory does not matter).
__global__ void __launch_bounds__(LNT)
tvl_scan_kernel(ListGeo g, unsigned* __restrict__ rows, unsigned long long* __restrict__ total) {
  const int i = blockIdx.x * LNT + threadIdx.x;
  if (i >= g.nzl * g.ntx) return;
  const int zl = i / g.ntx, tx = i - zl * g.ntx;
  unsigned* const col = rows + (size_t)zl * (size_t)(g.ny + 1) * (size_t)g.ntx + tx;
  unsigned sum = 0;
  for (int y = 0; y < g.ny; y++) sum += col[(size_t)y * g.ntx];
  const unsigned base = (unsigned)atomicAdd(total, (unsigned long long)sum);
  // descending rows: the entries of row y sit behind those of every row above it
  unsigned run = base;
  unsigned prev = col[(size_t)(g.ny - 1) * g.ntx];
  col[(size_t)g.ny * g.ntx] = run;            // rows below ny: the list's first entry
  for (int y = g.ny - 1; y >= 0; y--) {
    const unsigned c = prev;
    if (y > 0) prev = col[(size_t)(y - 1) * g.ntx];
    run += c;
    col[(size_t)y * g.ntx] = run;              // first entry of a row below y = behind row y's entries
  }
}

}  // namespace

namespace {
auto row_kernel(bool write, int mode) {   // (one signature)
  if (write) return mode == 1 ? tvl_row_kernel<true, 1> : mode == 0 ? tvl_row_kernel<true, 0> : tvl_row_kernel<true, 2>;
  return mode == 1 ? tvl_row_kernel<false, 1> : mode == 0 ? tvl_row_kernel<false, 0> : tvl_row_kernel<false, 2>;
}
}  // namespace

// (tv_common.hpp: TvListPlan)  The count pass and the scan, queued.  counter: the 16 words of WS_COUNTER, all zeroed here.
int tv_list_count(visfd_hip_ctx* ctx, const float* sal, const float* thr_dev, const float* mask_src, i64 nx, i64 ny, i64 nz,
                  i64 z_out0, i64 z_out1, int h, int mode, unsigned* counter, unsigned long long* total_dev, unsigned* flags_dev,
                  TvListPlan* plan) {
  hipStream_t st = ctx->stream;
  ListGeo g;
  g.nx = (int)nx; g.ny = (int)ny; g.nz = (int)nz; g.h = h; g.ntx = (int)((nx + TX - 1) / TX);
  g.zl0 = (int)std::max<i64>(z_out0 - h, 0);
  g.nzl = (int)(std::min<i64>(z_out1 + h, nz) - g.zl0);
  const size_t nrows = (size_t)g.nzl * (size_t)(ny + 1) * (size_t)g.ntx;
  if ((i64)g.nzl * ny > 0x7fffffffLL) return TV_DECLINED;
  unsigned* rows = nullptr;
  if (ws(ctx, WS_TVLIST, nrows, &rows) != VISFD_HIP_OK) { set_error(""); (void)hipGetLastError(); return TV_DECLINED; }
  VH_HIP(hipMemsetAsync(counter, 0, 16 * sizeof(unsigned), st));
  const unsigned row_blocks = (unsigned)(((i64)g.nzl * ny + LNT / 64 - 1) / (LNT / 64));
  row_kernel(false, mode)<<<dim3(row_blocks), dim3(LNT), 0, st>>>(sal, nullptr, mask_src, g, rows, nullptr, nullptr, flags_dev, 0, thr_dev);
  tvl_scan_kernel<<<dim3((unsigned)(((size_t)g.nzl * g.ntx + LNT - 1) / LNT)), dim3(LNT), 0, st>>>(g, rows, total_dev);
  VH_HIP(hipGetLastError());
  *plan = {g, rows, row_blocks, mode, thr_dev};
  return VISFD_HIP_OK;
}

// The write pass, once the host has {total, flags} of the plan's count pass: total sizes the entry arrays, the flags decide
// whether the caller has a use for the lists and whether their records are folded.
int tv_list_write(visfd_hip_ctx* ctx, const TvListPlan& plan, const float* sal, const float* dir, const float* mask_src,
                  unsigned long long total, unsigned flags, unsigned decline_on, bool may_fold, TvSenderLists* out) {
  hipStream_t st = ctx->stream;
  if (flags & decline_on) return TV_DECLINED;
  if (total >= (1ull << 32) - 2048) return TV_DECLINED;   // 32-bit entry indices
  const int fold = (may_fold && !(flags & TVL_NOT_POSITIVE)) ? 1 : 0;
  unsigned char* lists = nullptr;
  if (ws(ctx, WS_TVSCRATCH, (size_t)(total + 16) * 20, &lists) != VISFD_HIP_OK) { set_error(""); (void)hipGetLastError(); return TV_DECLINED; }
  float4* const ent = reinterpret_cast<float4*>(lists);
  unsigned* const pos = reinterpret_cast<unsigned*>(lists + (size_t)(total + 16) * 16);
  if (ctx->opt.tv_poison) VH_HIP(hipMemsetAsync(lists, 0xff, (size_t)(total + 16) * 20, st));
  row_kernel(true, plan.mode)<<<dim3(plan.row_blocks), dim3(LNT), 0, st>>>(sal, dir, mask_src, plan.g, plan.rows, ent, pos, nullptr, fold,
                                                                           plan.thr_dev);
  VH_HIP(hipGetLastError());
  *out = {ent, pos, plan.rows, total, flags, fold != 0, plan.g.zl0, plan.g.nzl};
  return VISFD_HIP_OK;
}

}  // namespace vh
