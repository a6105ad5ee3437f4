// discard_overlap.hip -- DiscardOverlappingBlobs (lib/visfd/feature.hpp:720-913) on the device.  The contract is in
// include/visfd_hip.h; the sequential form is visfd_hip_discard_overlapping_blobs (csrc/blob_post.cpp).
//
// The host walk visits the sorted list once; a blob reads the occupancy grid's cells it reaches and, when nothing it finds
// there makes it go, adds itself to them.  A cell only ever gains entries, so what blob i finds is a function of the blobs
// before it alone:
//     keep(i) = not exists k < i : keep(k) and share(i, k) and crit(i, k)
//   crit(i, k)    the discard criterion of blob_post.cpp, expression by expression (floats; doubles where M_PI enters)
//   share(i, k)   the two blobs have a cell of the table in common: with C = (int)floor((x - bmin) / scale) per axis and
//                 R = (int)ceil((d / 2) / scale) + 1, a cell c with 0 <= c < tsz on every axis, |c - C_i|^2 <= R_i^2 and
//                 |c - C_k|^2 <= R_k^2.  |C_i - C_k|^2 <= (R_i + R_k)^2 is necessary, not sufficient.
// The recursion is resolved in rounds (Jacobi): a blob with a kept conflicting predecessor is discarded, one with no
// undecided conflicting predecessor left is kept, the others wait.  The number of rounds is the longest chain of
// dependencies, short for lists a detector produces; past the cap (option discard_overlap_max_rounds) the host finishes
// the list from the states reached (vh::overlap_walk_sorted), with the same bits.
//
// Device work, all on the context's stream:
//   reduce_kernel     the bounds min(c - ceil(d/2)), max(c + ceil(d/2)), the range of the centres and the largest diameter
//                     (float extrema are exact), and one flag word: a non-finite value, a negative diameter
//   key_kernel        score or |score| as a monotone 32-bit integer, -0 folded onto +0
//   radix sort        rocPRIM, stable, ascending, values = original indices; descending is the exact reverse of the whole
//                     ascending order, so equal keys then go to the larger index first (std::pair's order reversed)
//   gather_kernel     the records {x, y, z, d} and the scores in sorted order
//   cell_kernel       the centre cell of every record over the range of all C as one integer, and the buckets' counts
//   scan + sort       the buckets' offsets; the records again, in bucket order (stable: positions ascend within a cell)
//   round_kernel      one launch per round over the list of undecided blobs.  A wave takes one blob; its box of cells (reach
//                     R_i + R_max) is a set of (z, y) rows, each a contiguous stream of candidates between two offsets;
//                     64 rows at a time, the lanes deal the rows' candidates among themselves.  Per candidate: k < i, the
//                     integer pre-test, state != discarded, crit, and only then the exact share.
//   flag/scan/scatter the kept records, in sorted order, into the three arrays
// A state word is (round << 2) | state, written by ordinary vector stores.  A reader treats a word stamped with the running
// round as undecided, so what a launch computes does not depend on which of its own stores a wave happens to see: states
// cross workgroups at launch boundaries only, and the round count of a list is a property of the list.
#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>

#include <algorithm>
#include <cmath>
#include <limits>

#include "common.hpp"
#include "wave.hpp"

namespace vh {
namespace {

constexpr int OV_BLOCK = 256;
constexpr i64 OV_MAX_CELLS = (i64)1 << 27;   // table cells, and cells of the bucket range, beyond which the host takes the list
constexpr unsigned OV_FLAG_NONFINITE = 1u, OV_FLAG_NEGATIVE = 2u;

// the words of the reduction, as monotone integers: [0..2] min(c - reff), [3..5] max(c + reff), [6..8] min c, [9..11] max c,
// [12] max d, [13] the flag word; then the counters (64-bit): [0] undecided blobs of the next round, [1] pairs that reached
// crit, [2] pairs that reached the exact share, [3] blobs kept
constexpr int OV_RED_WORDS = 16;
constexpr int OV_COUNTERS = 4;

struct OvParams {
  int bmin[3], tsz[3];
  int cmin[3], cdim[3];   // the bucket range: cells cmin .. cmin + cdim - 1 per axis
  float scale;
  int rmax;
  float ratio, max_large, max_small;
  int need_volume;        // 0: both volume limits are +infinity, no quotient exceeds them
  unsigned round;
};

__host__ __device__ inline unsigned mono_bits(float x) {   // a < b  <=>  mono(a) < mono(b), for non-NaN floats
  unsigned u;
#if defined(__HIP_DEVICE_COMPILE__)
  u = __float_as_uint(x);
#else
  std::memcpy(&u, &x, 4);
#endif
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
inline float mono_float(unsigned m) {
  const unsigned u = (m & 0x80000000u) ? (m & 0x7FFFFFFFu) : ~m;
  float x;
  std::memcpy(&x, &u, 4);
  return x;
}
__host__ __device__ inline bool finite_f(float x) { return x - x == 0.0f; }

// blob_post.cpp:147-153, the same float expressions
__host__ __device__ inline int cell_coord(float x, int bmin, float scale) { return (int)floorf((x - (float)bmin) / scale); }
__host__ __device__ inline int cell_reach(float d, float scale) { return (int)ceilf((d / 2) / scale) + 1; }

// lib/visfd/visfd_utils.hpp:95-118 as csrc/blob_post.cpp states it
__device__ inline float sphere_overlap_dev(float rij, float Ri, float Rj) {
  if (Ri > Rj) { const float t = Ri; Ri = Rj; Rj = t; }
  if (rij <= Ri) return (float)((4 * M_PI / 3) * Ri * Ri * Ri);
  const float xi = (float)(0.5 * (1.0 / rij) * (rij * rij + Ri * Ri - Rj * Rj));
  const float xj = (float)(0.5 * (1.0 / rij) * (rij * rij + Rj * Rj - Ri * Ri));
  const float qi = xi / Ri, qj = xj / Rj;
  const float ti = Ri * Ri * Ri * (2 - qi * (3 - qi * qi));
  const float tj = Rj * Rj * Rj * (2 - qj * (3 - qj * qj));
  return (float)((M_PI / 3) * (ti + tj));
}

// blob_post.cpp, the body of the loop over a cell's entries
__device__ inline bool crit_dev(const float4& bi, const float4& bk, const OvParams& p) {
  const float rik = sqrtf((bi.x - bk.x) * (bi.x - bk.x) + (bi.y - bk.y) * (bi.y - bk.y) + (bi.z - bk.z) * (bi.z - bk.z));
  const float ri = bi.w / 2, rk = bk.w / 2;
  bool discard = rik < (ri + rk) * p.ratio;
  if (p.need_volume) {
    const float vol = sphere_overlap_dev(rik, ri, rk);
    const float vi = (float)((4 * M_PI / 3) * (ri * ri * ri));
    const float vk = (float)((4 * M_PI / 3) * (rk * rk * rk));
    float v_large = vi, v_small = vk;
    if (vk > vi) { v_large = vk; v_small = vi; }
    if ((vol / v_small > p.max_small) || (vol / v_large > p.max_large)) discard = true;
  }
  return discard;
}

__device__ inline bool in_table(int x, int y, int z, const OvParams& p) {
  return x >= 0 && x < p.tsz[0] && y >= 0 && y < p.tsz[1] && z >= 0 && z < p.tsz[2];
}

// the exact share: the pre-test has passed, dsq = |C_i - C_k|^2
__device__ inline bool share_dev(int ix, int iy, int iz, int Ri, int kx, int ky, int kz, int Rk, int dsq, const OvParams& p) {
  if (dsq <= Rk * Rk && in_table(ix, iy, iz, p)) return true;   // C_i is a cell of both
  if (dsq <= Ri * Ri && in_table(kx, ky, kz, p)) return true;   // C_k is
  // the cells of the smaller ball that lie in the table, against the larger ball
  int sx = ix, sy = iy, sz = iz, Rs = Ri, lx = kx, ly = ky, lz = kz, Rl = Rk;
  if (Rk < Ri) { sx = kx; sy = ky; sz = kz; Rs = Rk; lx = ix; ly = iy; lz = iz; Rl = Ri; }
  const int Rssq = Rs * Rs, Rlsq = Rl * Rl;
  const int z0 = max(sz - Rs, 0), z1 = min(sz + Rs, p.tsz[2] - 1);
  const int y0 = max(sy - Rs, 0), y1 = min(sy + Rs, p.tsz[1] - 1);
  const int x0 = max(sx - Rs, 0), x1 = min(sx + Rs, p.tsz[0] - 1);
  for (int z = z0; z <= z1; z++)
    for (int y = y0; y <= y1; y++) {
      const int a = (z - sz) * (z - sz) + (y - sy) * (y - sy), b = (z - lz) * (z - lz) + (y - ly) * (y - ly);
      if (a > Rssq || b > Rlsq) continue;
      for (int x = x0; x <= x1; x++)
        if (a + (x - sx) * (x - sx) <= Rssq && b + (x - lx) * (x - lx) <= Rlsq) return true;
    }
  return false;
}

// ---- preparation ----------------------------------------------------------------------------------------------------------
// red: OV_RED_WORDS words, the minima preset to all ones and the rest to zero
__global__ __launch_bounds__(OV_BLOCK) void reduce_kernel(const float* __restrict__ crds, const float* __restrict__ diam,
                                                          const float* __restrict__ score, i64 n, unsigned* __restrict__ red) {
  unsigned lo[3] = {~0u, ~0u, ~0u}, hi[3] = {0u, 0u, 0u}, clo[3] = {~0u, ~0u, ~0u}, chi[3] = {0u, 0u, 0u}, dmax = 0u, flags = 0u;
  const i64 stride = (i64)gridDim.x * blockDim.x;
  for (i64 i = (i64)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    const float d = diam[i];
    const float reff = ceilf(d / 2);
    if (!finite_f(d) || !finite_f(score[i])) flags |= OV_FLAG_NONFINITE;
    if (d < 0.0f) flags |= OV_FLAG_NEGATIVE;
    dmax = max(dmax, mono_bits(d));
#pragma unroll
    for (int a = 0; a < 3; a++) {
      const float c = crds[3 * i + a];
      if (!finite_f(c)) flags |= OV_FLAG_NONFINITE;
      lo[a] = min(lo[a], mono_bits(c - reff));
      hi[a] = max(hi[a], mono_bits(c + reff));
      clo[a] = min(clo[a], mono_bits(c));
      chi[a] = max(chi[a], mono_bits(c));
    }
  }
  // behind the grid-stride loop every lane is back; one without a blob holds the neutral words
  const bool lead = wave_lane() == 0;
#pragma unroll
  for (int a = 0; a < 3; a++) {
    const unsigned v0 = wave_min(lo[a]), v1 = wave_max(hi[a]), v2 = wave_min(clo[a]), v3 = wave_max(chi[a]);
    if (lead) {
      atomicMin(&red[a], v0);
      atomicMax(&red[3 + a], v1);
      atomicMin(&red[6 + a], v2);
      atomicMax(&red[9 + a], v3);
    }
  }
  const unsigned vd = wave_max(dmax);
  const unsigned long long any1 = __ballot((flags & OV_FLAG_NONFINITE) != 0u), any2 = __ballot((flags & OV_FLAG_NEGATIVE) != 0u);
  if (lead) {
    atomicMax(&red[12], vd);
    const unsigned f = (any1 ? OV_FLAG_NONFINITE : 0u) | (any2 ? OV_FLAG_NEGATIVE : 0u);
    if (f) atomicOr(&red[13], f);
  }
}

__global__ __launch_bounds__(OV_BLOCK) void key_kernel(const float* __restrict__ score, i64 n, int magnitude,
                                                       unsigned* __restrict__ key, unsigned* __restrict__ idx) {
  const i64 i = (i64)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  unsigned u = __float_as_uint(score[i]);
  if (magnitude) u &= 0x7FFFFFFFu;
  if ((u & 0x7FFFFFFFu) == 0u) u = 0u;   // -0 compares equal to +0: one key
  key[i] = mono_bits(__uint_as_float(u));
  idx[i] = (unsigned)i;
}

__global__ __launch_bounds__(OV_BLOCK) void iota_kernel(unsigned* __restrict__ a, i64 n) {
  const i64 i = (i64)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) a[i] = (unsigned)i;
}

// order: the ascending ranking (null: the list stays as it is); reversed: position q takes order[n - 1 - q]
__global__ __launch_bounds__(OV_BLOCK) void gather_kernel(const float* __restrict__ crds, const float* __restrict__ diam,
                                                          const float* __restrict__ score, const unsigned* __restrict__ order,
                                                          int reversed, i64 n, float4* __restrict__ rec,
                                                          float* __restrict__ sscore) {
  const i64 q = (i64)blockIdx.x * blockDim.x + threadIdx.x;
  if (q >= n) return;
  const i64 j = order ? (i64)order[reversed ? n - 1 - q : q] : q;
  rec[q] = make_float4(crds[3 * j], crds[3 * j + 1], crds[3 * j + 2], diam[j]);
  sscore[q] = score[j];
}

// counts: one word per cell of the bucket range, zeroed
__global__ __launch_bounds__(OV_BLOCK) void cell_kernel(const float4* __restrict__ rec, i64 n, OvParams p,
                                                        unsigned* __restrict__ key, unsigned* __restrict__ pos,
                                                        unsigned* __restrict__ counts) {
  const i64 q = (i64)blockIdx.x * blockDim.x + threadIdx.x;
  if (q >= n) return;
  const float4 r = rec[q];
  // the range was computed from the extreme centres with the same expression: 0 <= c < cdim (the clamps change nothing)
  const int cx = min(max(cell_coord(r.x, p.bmin[0], p.scale) - p.cmin[0], 0), p.cdim[0] - 1),
            cy = min(max(cell_coord(r.y, p.bmin[1], p.scale) - p.cmin[1], 0), p.cdim[1] - 1),
            cz = min(max(cell_coord(r.z, p.bmin[2], p.scale) - p.cmin[2], 0), p.cdim[2] - 1);
  const unsigned cell = ((unsigned)cz * (unsigned)p.cdim[1] + (unsigned)cy) * (unsigned)p.cdim[0] + (unsigned)cx;
  key[q] = cell;
  pos[q] = (unsigned)q;
  atomicAdd(&counts[cell], 1u);
}

__global__ __launch_bounds__(OV_BLOCK) void bucket_gather_kernel(const float4* __restrict__ rec, const unsigned* __restrict__ bpos,
                                                                 i64 n, float4* __restrict__ brec) {
  const i64 j = (i64)blockIdx.x * blockDim.x + threadIdx.x;
  if (j < n) brec[j] = rec[bpos[j]];
}

__global__ __launch_bounds__(OV_BLOCK) void fill_kernel(unsigned* __restrict__ a, i64 n, unsigned v) {
  const i64 i = (i64)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) a[i] = v;
}

// ---- a round --------------------------------------------------------------------------------------------------------------
// One wave per entry of `und`.  state is read and written here (no __restrict__: its loads stay on the vector path).
__global__ __launch_bounds__(OV_BLOCK) void round_kernel(const float4* __restrict__ rec, const float4* __restrict__ brec,
                                                         const unsigned* __restrict__ bpos, const unsigned* __restrict__ offsets,
                                                         unsigned* state, const unsigned* __restrict__ und, unsigned n_und,
                                                         unsigned* __restrict__ und_next, unsigned long long* __restrict__ counters,
                                                         OvParams p) {
  const i64 wave = ((i64)blockIdx.x * OV_BLOCK + threadIdx.x) / WAVE;
  const int lane = wave_lane();
  if (wave >= n_und) return;   // the whole wave
  const unsigned i = und[wave];
  const float4 me = rec[i];
  const int ix = cell_coord(me.x, p.bmin[0], p.scale), iy = cell_coord(me.y, p.bmin[1], p.scale),
            iz = cell_coord(me.z, p.bmin[2], p.scale), Ri = cell_reach(me.w, p.scale);
  const int reach = Ri + p.rmax;
  // the box, in cells of the bucket range
  const int x0 = max(ix - reach, p.cmin[0]) - p.cmin[0], x1 = min(ix + reach, p.cmin[0] + p.cdim[0] - 1) - p.cmin[0];
  const int y0 = max(iy - reach, p.cmin[1]) - p.cmin[1], y1 = min(iy + reach, p.cmin[1] + p.cdim[1] - 1) - p.cmin[1];
  const int z0 = max(iz - reach, p.cmin[2]) - p.cmin[2], z1 = min(iz + reach, p.cmin[2] + p.cdim[2] - 1) - p.cmin[2];
  // the blob's own cell is in the range, so the box is not empty; an empty one would have no rows
  const int ny = y1 - y0 + 1, nrows = (x1 < x0 || y1 < y0 || z1 < z0) ? 0 : ny * (z1 - z0 + 1);
  bool found = false, pending = false;
  unsigned n_crit = 0u, n_share = 0u;
  for (int rbase = 0; rbase < nrows; rbase += WAVE) {
    const int r = rbase + lane;
    unsigned start = 0u, cnt = 0u;
    if (r < nrows) {
      const unsigned row = ((unsigned)(z0 + r / ny) * (unsigned)p.cdim[1] + (unsigned)(y0 + r % ny)) * (unsigned)p.cdim[0];
      start = offsets[row + (unsigned)x0];
      cnt = offsets[row + (unsigned)x1 + 1u] - start;
    }
    unsigned incl = cnt;   // candidates of rows rbase .. r
#pragma unroll
    for (int d = 1; d < WAVE; d <<= 1) {
      const unsigned t = (unsigned)__shfl_up((int)incl, d, WAVE);
      if (lane >= d) incl += t;
    }
    const unsigned total = (unsigned)__shfl((int)incl, WAVE - 1, WAVE);
    const unsigned excl = incl - cnt;
    for (unsigned tb = 0u; tb < total; tb += WAVE) {
      const unsigned t = tb + (unsigned)lane;
      int lo = 0, hi = WAVE - 1;   // the first row whose inclusive count exceeds t
#pragma unroll
      for (int s = 0; s < 6; s++) {
        const int mid = (lo + hi) >> 1;
        const unsigned v = (unsigned)__shfl((int)incl, mid, WAVE);
        if (v > t) hi = mid; else lo = mid + 1;
      }
      lo = min(lo, WAVE - 1);
      const unsigned s0 = (unsigned)__shfl((int)start, lo, WAVE), e0 = (unsigned)__shfl((int)excl, lo, WAVE);
      if (t < total) {
        const unsigned j = s0 + (t - e0);
        const unsigned k = bpos[j];
        if (k < i) {
          const float4 other = brec[j];
          const int kx = cell_coord(other.x, p.bmin[0], p.scale), ky = cell_coord(other.y, p.bmin[1], p.scale),
                    kz = cell_coord(other.z, p.bmin[2], p.scale), Rk = cell_reach(other.w, p.scale);
          const int dsq = (ix - kx) * (ix - kx) + (iy - ky) * (iy - ky) + (iz - kz) * (iz - kz);
          if (dsq <= (Ri + Rk) * (Ri + Rk)) {
            const unsigned w = state[k];
            const unsigned st = (w >> 2) == p.round ? (unsigned)OVERLAP_UNDECIDED : (w & 3u);
            if (st != (unsigned)OVERLAP_DISCARDED) {
              n_crit++;
              if (crit_dev(me, other, p)) {
                n_share++;
                if (share_dev(ix, iy, iz, Ri, kx, ky, kz, Rk, dsq, p)) {
                  if (st == (unsigned)OVERLAP_KEPT) found = true; else pending = true;
                }
              }
            }
          }
        }
      }
      if (__any(found)) break;
    }
    if (__any(found)) break;
  }
  const bool any_found = __any(found), any_pending = __any(pending);
#pragma unroll
  for (int d = WAVE / 2; d >= 1; d >>= 1) {
    n_crit += (unsigned)__shfl_xor((int)n_crit, d, WAVE);
    n_share += (unsigned)__shfl_xor((int)n_share, d, WAVE);
  }
  if (lane == 0) {
    if (any_found) state[i] = (p.round << 2) | (unsigned)OVERLAP_DISCARDED;
    else if (!any_pending) state[i] = (p.round << 2) | (unsigned)OVERLAP_KEPT;
    else und_next[atomicAdd(&counters[0], 1ull)] = i;
    if (n_crit) atomicAdd(&counters[1], (unsigned long long)n_crit);
    if (n_share) atomicAdd(&counters[2], (unsigned long long)n_share);
  }
}

// ---- compaction -----------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(OV_BLOCK) void kept_flag_kernel(const unsigned* __restrict__ state, i64 n, unsigned* __restrict__ flag) {
  const i64 q = (i64)blockIdx.x * blockDim.x + threadIdx.x;
  if (q < n) flag[q] = (state[q] & 3u) == (unsigned)OVERLAP_KEPT ? 1u : 0u;
}
__global__ __launch_bounds__(OV_BLOCK) void states_byte_kernel(const unsigned* __restrict__ state, i64 n, unsigned char* __restrict__ out) {
  const i64 q = (i64)blockIdx.x * blockDim.x + threadIdx.x;
  if (q < n) out[q] = (unsigned char)(state[q] & 3u);
}
// where[q]: the exclusive count of kept records before q.  rec and sscore are copies, so the three arrays may be the inputs.
__global__ __launch_bounds__(OV_BLOCK) void scatter_kernel(const float4* __restrict__ rec, const float* __restrict__ sscore,
                                                           const unsigned* __restrict__ flag, const unsigned* __restrict__ where,
                                                           i64 n, float* __restrict__ crds, float* __restrict__ diam,
                                                           float* __restrict__ score, unsigned long long* __restrict__ counters) {
  const i64 q = (i64)blockIdx.x * blockDim.x + threadIdx.x;
  if (q >= n) return;
  if (q == n - 1) counters[3] = (unsigned long long)where[q] + flag[q];
  if (!flag[q]) return;
  const float4 r = rec[q];
  const i64 o = where[q];
  crds[3 * o] = r.x; crds[3 * o + 1] = r.y; crds[3 * o + 2] = r.z;
  diam[o] = r.w;
  score[o] = sscore[q];
}

inline unsigned blocks(i64 n) { return (unsigned)((n + OV_BLOCK - 1) / OV_BLOCK); }
inline size_t align256(size_t b) { return (b + 255) / 256 * 256; }

// option discard_overlap_time: events on the stream at the phase boundaries (reduction | ranking and records | buckets |
// rounds | compaction), read after the call's last wait
enum { PH_REDUCE = 0, PH_RANK, PH_BUCKETS, PH_ROUNDS, PH_COMPACT, PH_COUNT };

struct Plan {   // what the core found out and did
  PhaseClock<PH_COUNT> clock;
  int reason = VISFD_HIP_DISCARD_OVERLAP_REASON_NONE;
  i64 rounds = 0, kept = 0, pairs_crit = 0, pairs_share = 0, cells = 0;
  bool on_host = false;           // the round cap was reached: hc, hd, hs hold the finished list
  std::vector<float> hc, hd, hs;
};

// The three arrays on the device, n >= 1.  Returns with the stream idle.  plan->reason != NONE and !plan->on_host: nothing
// was written, the list belongs to the host entry.  on_host: the arrays are untouched too, the result is in the plan.
int discard_dev(visfd_hip_ctx* ctx, float* crds, float* diam, float* score, i64 n, float ratio, float max_large, float max_small,
                int criteria, int scale, Plan* plan) {
  hipStream_t st = ctx->stream;
  plan->clock.start(st, ctx->opt.discard_overlap_time != 0);
  // ---- the reduction: values and bounds
  size_t sort_bytes = 0, scan_bytes = 0;
  {
    unsigned* nul = nullptr;
    VH_HIP(rocprim::radix_sort_pairs(nullptr, sort_bytes, nul, nul, nul, nul, (size_t)n, 0u, 32u, st));
  }
  unsigned* red = nullptr;
  {
    char* t = nullptr;
    VH_TRY(ws(ctx, WS_OVL_TEMP, (size_t)256, &t));
    red = reinterpret_cast<unsigned*>(t);
  }
  {
    unsigned init[OV_RED_WORDS] = {};
    for (int a = 0; a < 3; a++) init[a] = init[6 + a] = ~0u;
    VH_HIP(hipMemcpyAsync(red, init, sizeof(init), hipMemcpyHostToDevice, st));
    VH_HIP(hipStreamSynchronize(st));   // init lives on this frame
  }
  reduce_kernel<<<grid_for(n, OV_BLOCK, (i64)ctx->num_cus * 8), OV_BLOCK, 0, st>>>(crds, diam, score, n, red);
  VH_HIP(hipGetLastError());
  unsigned r[OV_RED_WORDS];
  VH_HIP(hipMemcpyAsync(r, red, sizeof(r), hipMemcpyDeviceToHost, st));
  VH_HIP(hipStreamSynchronize(st));
  if (r[13] & OV_FLAG_NONFINITE) { plan->reason = VISFD_HIP_DISCARD_OVERLAP_REASON_NONFINITE; return VISFD_HIP_OK; }
  if (r[13] & OV_FLAG_NEGATIVE) { plan->reason = VISFD_HIP_DISCARD_OVERLAP_REASON_NEGATIVE; return VISFD_HIP_OK; }
  OvParams p = {};
  bool has_grid = true;
  double cells = 1.0;
  for (int a = 0; a < 3; a++) {
    const float lo = mono_float(r[a]), hi = mono_float(r[3 + a]);
    if (!(lo >= -2147483648.0f && hi < 2147483648.0f)) { plan->reason = VISFD_HIP_DISCARD_OVERLAP_REASON_BOUNDS; return VISFD_HIP_OK; }
    // the sequential loop (blob_post.cpp) equals these for finite values and diameters >= 0: its bmin is set by the first
    // blob and then only lowered; its bmax starts at -1 and is only raised, so a list below -1 on an axis keeps -1 there
    const int bmin = (int)lo, bmax = std::max((int)hi, -1);
    const i64 span = (i64)1 + bmax - bmin;
    if (span > (i64)std::numeric_limits<int>::max()) { plan->reason = VISFD_HIP_DISCARD_OVERLAP_REASON_BOUNDS; return VISFD_HIP_OK; }
    p.bmin[a] = bmin;
    p.tsz[a] = (int)(span / scale);
    if (p.tsz[a] <= 0) has_grid = false;
    cells *= (double)std::max(p.tsz[a], 0);
  }
  if (has_grid && cells > (double)OV_MAX_CELLS) { plan->reason = VISFD_HIP_DISCARD_OVERLAP_REASON_CELLS; return VISFD_HIP_OK; }
  plan->cells = has_grid ? (i64)cells : 0;
  p.scale = (float)scale;
  i64 ncell = 1;
  if (has_grid) {
    double bucket = 1.0;
    for (int a = 0; a < 3; a++) {
      // C is monotone in the coordinate: its range is that of the extreme centres.  Centres lie within the bounds, so with
      // a table of at most 2^27 cells these quotients are far inside the int range.
      const int c0 = cell_coord(mono_float(r[6 + a]), p.bmin[a], p.scale), c1 = cell_coord(mono_float(r[9 + a]), p.bmin[a], p.scale);
      p.cmin[a] = c0;
      p.cdim[a] = c1 - c0 + 1;
      bucket *= (double)p.cdim[a];
    }
    if (bucket > (double)OV_MAX_CELLS) { plan->reason = VISFD_HIP_DISCARD_OVERLAP_REASON_CELLS; return VISFD_HIP_OK; }
    ncell = (i64)bucket;
    p.rmax = cell_reach(mono_float(r[12]), p.scale);
  }
  p.ratio = ratio; p.max_large = max_large; p.max_small = max_small;
  const float inf = std::numeric_limits<float>::infinity();
  p.need_volume = (max_large == inf && max_small == inf) ? 0 : 1;

  // ---- the workspace
  VH_HIP(rocprim::exclusive_scan(nullptr, scan_bytes, (unsigned*)nullptr, (unsigned*)nullptr, 0u,
                                 (size_t)std::max<i64>(ncell + 1, n), rocprim::plus<unsigned>(), st));
  const size_t temp_bytes = std::max(sort_bytes, scan_bytes);
  char* temp_base = nullptr;
  VH_TRY(ws(ctx, WS_OVL_TEMP, (size_t)256 + align256(temp_bytes), &temp_base));
  unsigned long long* counters = reinterpret_cast<unsigned long long*>(temp_base + OV_RED_WORDS * sizeof(unsigned));
  void* temp = temp_base + 256;
  const size_t un = (size_t)n;
  char* list = nullptr;
  VH_TRY(ws(ctx, WS_OVL_LIST, 2 * align256(16 * un) + 8 * align256(4 * un), &list));
  float4* rec = reinterpret_cast<float4*>(list); list += align256(16 * un);
  float4* brec = reinterpret_cast<float4*>(list); list += align256(16 * un);
  unsigned* word[8];
  for (int k = 0; k < 8; k++) { word[k] = reinterpret_cast<unsigned*>(list); list += align256(4 * un); }
  unsigned *keyA = word[0], *keyB = word[1], *valA = word[2], *valB = word[3], *state = word[4], *undA = word[5], *undB = word[6];
  float* sscore = reinterpret_cast<float*>(word[7]);
  unsigned* offsets = nullptr;
  VH_TRY(ws(ctx, WS_OVL_CELLS, (size_t)ncell + 1, &offsets));
  VH_HIP(hipMemsetAsync(counters, 0, OV_COUNTERS * sizeof(unsigned long long), st));

  // ---- ranking and records
  plan->clock.mark(PH_RANK);
  const unsigned g = blocks(n);
  if (criteria != VISFD_HIP_DO_NOT_SORT) {
    const bool magnitude = criteria == VISFD_HIP_SORT_DECREASING_MAGNITUDE || criteria == VISFD_HIP_SORT_INCREASING_MAGNITUDE;
    const bool descending = criteria == VISFD_HIP_SORT_DECREASING || criteria == VISFD_HIP_SORT_DECREASING_MAGNITUDE;
    key_kernel<<<g, OV_BLOCK, 0, st>>>(score, n, magnitude ? 1 : 0, keyA, valA);
    size_t tb = temp_bytes;
    VH_HIP(rocprim::radix_sort_pairs(temp, tb, keyA, keyB, valA, valB, un, 0u, 32u, st));
    gather_kernel<<<g, OV_BLOCK, 0, st>>>(crds, diam, score, valB, descending ? 1 : 0, n, rec, sscore);
  } else {
    gather_kernel<<<g, OV_BLOCK, 0, st>>>(crds, diam, score, nullptr, 0, n, rec, sscore);
  }
  VH_HIP(hipGetLastError());

  if (!has_grid) {
    fill_kernel<<<g, OV_BLOCK, 0, st>>>(state, n, (unsigned)OVERLAP_KEPT);   // no table, no cell in common: nothing collides
  } else {
    // ---- buckets
    plan->clock.mark(PH_BUCKETS);
    VH_HIP(hipMemsetAsync(offsets, 0, sizeof(unsigned) * ((size_t)ncell + 1), st));
    VH_HIP(hipMemsetAsync(state, 0, sizeof(unsigned) * un, st));
    cell_kernel<<<g, OV_BLOCK, 0, st>>>(rec, n, p, keyA, valA, offsets);
    size_t tb = temp_bytes;
    VH_HIP(rocprim::exclusive_scan(temp, tb, offsets, offsets, 0u, (size_t)ncell + 1, rocprim::plus<unsigned>(), st));
    unsigned bits = 1;
    while (bits < 32 && ((i64)1 << bits) < ncell) bits++;
    tb = temp_bytes;
    VH_HIP(rocprim::radix_sort_pairs(temp, tb, keyA, keyB, valA, valB, un, 0u, bits, st));
    unsigned* bpos = valB;
    bucket_gather_kernel<<<g, OV_BLOCK, 0, st>>>(rec, bpos, n, brec);
    iota_kernel<<<g, OV_BLOCK, 0, st>>>(undA, n);
    VH_HIP(hipGetLastError());
    // ---- rounds
    plan->clock.mark(PH_ROUNDS);
    const i64 max_rounds = std::max(0, ctx->opt.discard_overlap_max_rounds);
    i64 n_und = n;
    unsigned *cur = undA, *next = undB;
    while (n_und > 0) {
      if (plan->rounds >= max_rounds) break;
      plan->rounds++;
      p.round = (unsigned)plan->rounds;
      VH_HIP(hipMemsetAsync(counters, 0, sizeof(unsigned long long), st));
      const i64 waves_per_block = OV_BLOCK / WAVE;
      round_kernel<<<(unsigned)((n_und + waves_per_block - 1) / waves_per_block), OV_BLOCK, 0, st>>>(
          rec, brec, bpos, offsets, state, cur, (unsigned)n_und, next, counters, p);
      VH_HIP(hipGetLastError());
      unsigned long long left = 0;
      VH_HIP(hipMemcpyAsync(&left, counters, sizeof(left), hipMemcpyDeviceToHost, st));
      VH_HIP(hipStreamSynchronize(st));
      n_und = (i64)left;
      std::swap(cur, next);
    }
    if (n_und > 0) {
      // the cap: sorted records, scores and states to the host, which finishes the walk
      plan->reason = VISFD_HIP_DISCARD_OVERLAP_REASON_ROUNDS;
      plan->on_host = true;
      unsigned char* bytes = reinterpret_cast<unsigned char*>(keyA);
      plan->clock.mark(PH_COUNT);
      states_byte_kernel<<<g, OV_BLOCK, 0, st>>>(state, n, bytes);
      VH_HIP(hipGetLastError());
      std::vector<float> hrec(4 * un);
      std::vector<unsigned char> hst(un);
      plan->hs.resize(un);
      VH_HIP(hipMemcpyAsync(hrec.data(), rec, 16 * un, hipMemcpyDeviceToHost, st));
      VH_HIP(hipMemcpyAsync(plan->hs.data(), sscore, 4 * un, hipMemcpyDeviceToHost, st));
      VH_HIP(hipMemcpyAsync(hst.data(), bytes, un, hipMemcpyDeviceToHost, st));
      unsigned long long c[OV_COUNTERS];
      VH_HIP(hipMemcpyAsync(c, counters, sizeof(c), hipMemcpyDeviceToHost, st));
      VH_HIP(hipStreamSynchronize(st));
      plan->pairs_crit = (i64)c[1];
      plan->pairs_share = (i64)c[2];
      plan->hc.resize(3 * un);
      plan->hd.resize(un);
      for (size_t q = 0; q < un; q++) {
        plan->hc[3 * q] = hrec[4 * q]; plan->hc[3 * q + 1] = hrec[4 * q + 1]; plan->hc[3 * q + 2] = hrec[4 * q + 2];
        plan->hd[q] = hrec[4 * q + 3];
      }
      int64_t m = n;
      overlap_walk_sorted(plan->hc.data(), plan->hd.data(), plan->hs.data(), &m, hst.data(), ratio, max_large, max_small, scale);
      plan->kept = m;
      return VISFD_HIP_OK;
    }
  }
  // ---- compaction
  plan->clock.mark(PH_COMPACT);
  kept_flag_kernel<<<g, OV_BLOCK, 0, st>>>(state, n, keyA);
  size_t tb = temp_bytes;
  VH_HIP(rocprim::exclusive_scan(temp, tb, keyA, keyB, 0u, un, rocprim::plus<unsigned>(), st));
  scatter_kernel<<<g, OV_BLOCK, 0, st>>>(rec, sscore, keyA, keyB, n, crds, diam, score, counters);
  VH_HIP(hipGetLastError());
  plan->clock.mark(PH_COUNT);
  unsigned long long c[OV_COUNTERS];
  VH_HIP(hipMemcpyAsync(c, counters, sizeof(c), hipMemcpyDeviceToHost, st));
  VH_HIP(hipStreamSynchronize(st));
  plan->pairs_crit = (i64)c[1];
  plan->pairs_share = (i64)c[2];
  plan->kept = (i64)c[3];
  return VISFD_HIP_OK;
}

int check_args(const visfd_hip_ctx* ctx, const float* crds, const float* diam, const float* score, const int64_t* n, int criteria,
               int scale) {
  VH_REQUIRE(ctx, "null context");
  VH_REQUIRE(n && *n >= 0, "discard_overlapping_blobs: bad count");
  VH_REQUIRE(scale >= 1, "discard_overlapping_blobs: scale must be >= 1");
  VH_REQUIRE(criteria >= 0 && criteria <= VISFD_HIP_SORT_INCREASING_MAGNITUDE, "sort_blobs: unknown sort criteria");
  VH_REQUIRE(*n == 0 || (crds && diam && score), "sort_blobs: null list");
  return VISFD_HIP_OK;
}

void remember(visfd_hip_ctx* ctx, int path, Plan& plan, i64 n_in, i64 kept) {
  plan.clock.read(ctx->discard_overlap_ms);
  int64_t* L = ctx->discard_overlap_last;
  L[0] = path; L[1] = plan.reason; L[2] = plan.rounds; L[3] = n_in; L[4] = kept;
  L[5] = plan.pairs_crit; L[6] = plan.pairs_share; L[7] = plan.cells;
}

}  // namespace
}  // namespace vh

using namespace vh;

extern "C" {

int visfd_hip_discard_overlapping_blobs_last(visfd_hip_ctx* ctx, int64_t info[8]) {
  VH_REQUIRE(ctx && info, "null argument");
  for (int k = 0; k < 8; k++) info[k] = ctx->discard_overlap_last[k];
  return VISFD_HIP_OK;
}

int visfd_hip_discard_overlapping_blobs_last_times(visfd_hip_ctx* ctx, float ms[5]) {
  VH_REQUIRE(ctx && ms, "null argument");
  for (int k = 0; k < PH_COUNT; k++) ms[k] = ctx->discard_overlap_ms[k];
  return VISFD_HIP_OK;
}

int visfd_hip_discard_overlapping_blobs_ctx(visfd_hip_ctx* ctx, float* crds, float* diameters, float* scores, int64_t* n_inout,
                                            float min_radial_separation_ratio, float max_volume_overlap_large,
                                            float max_volume_overlap_small, int sort_criteria, int scale) {
  VH_TRY(check_args(ctx, crds, diameters, scores, n_inout, sort_criteria, scale));
  const i64 n = *n_inout;
  Plan plan;
  const bool by_option = ctx->opt.discard_overlap_host != 0;
  if (!by_option && n >= ((i64)1 << 31)) plan.reason = VISFD_HIP_DISCARD_OVERLAP_REASON_COUNT;
  float *dc = nullptr, *dd = nullptr, *ds = nullptr;
  if (!by_option && n > 0 && plan.reason == VISFD_HIP_DISCARD_OVERLAP_REASON_NONE) {
    VH_HIP(hipSetDevice(ctx->device));
    const Stage sb = {ctx, (size_t)n};
    VH_TRY(sb.up(WS_H2D_0, crds, &dc, 3));
    VH_TRY(sb.up(WS_H2D_1, diameters, &dd));
    VH_TRY(sb.up(WS_H2D_2, scores, &ds));
    VH_TRY(discard_dev(ctx, dc, dd, ds, n, min_radial_separation_ratio, max_volume_overlap_large, max_volume_overlap_small,
                       sort_criteria, scale, &plan));
  }
  if (by_option || (plan.reason != VISFD_HIP_DISCARD_OVERLAP_REASON_NONE && !plan.on_host)) {
    VH_TRY(visfd_hip_discard_overlapping_blobs(crds, diameters, scores, n_inout, min_radial_separation_ratio,
                                               max_volume_overlap_large, max_volume_overlap_small, sort_criteria, scale));
    remember(ctx, by_option ? VISFD_HIP_DISCARD_OVERLAP_PATH_HOST : VISFD_HIP_DISCARD_OVERLAP_PATH_HANDED_OVER, plan, n, *n_inout);
    return VISFD_HIP_OK;
  }
  if (plan.on_host) {
    std::memcpy(crds, plan.hc.data(), sizeof(float) * 3 * (size_t)plan.kept);
    std::memcpy(diameters, plan.hd.data(), sizeof(float) * (size_t)plan.kept);
    std::memcpy(scores, plan.hs.data(), sizeof(float) * (size_t)plan.kept);
    *n_inout = plan.kept;
    remember(ctx, VISFD_HIP_DISCARD_OVERLAP_PATH_HANDED_OVER, plan, n, plan.kept);
    return VISFD_HIP_OK;
  }
  if (plan.kept > 0) {
    const Stage sk = {ctx, (size_t)plan.kept};
    VH_HIP(hipMemcpyAsync(crds, dc, sizeof(float) * 3 * sk.n, hipMemcpyDeviceToHost, ctx->stream));
    VH_HIP(hipMemcpyAsync(diameters, dd, sizeof(float) * sk.n, hipMemcpyDeviceToHost, ctx->stream));
    VH_TRY(sk.down(scores, ds));
  }
  *n_inout = plan.kept;
  remember(ctx, VISFD_HIP_DISCARD_OVERLAP_PATH_DEVICE, plan, n, plan.kept);
  return VISFD_HIP_OK;
}

int visfd_hip_discard_overlapping_blobs_dev(visfd_hip_ctx* ctx, float* crds, float* diameters, float* scores, int64_t* n_inout,
                                            float min_radial_separation_ratio, float max_volume_overlap_large,
                                            float max_volume_overlap_small, int sort_criteria, int scale) {
  VH_TRY(check_args(ctx, crds, diameters, scores, n_inout, sort_criteria, scale));
  const i64 n = *n_inout;
  Plan plan;
  VH_HIP(hipSetDevice(ctx->device));
  const bool by_option = ctx->opt.discard_overlap_host != 0;
  if (!by_option && n >= ((i64)1 << 31)) plan.reason = VISFD_HIP_DISCARD_OVERLAP_REASON_COUNT;
  if (!by_option && n > 0 && plan.reason == VISFD_HIP_DISCARD_OVERLAP_REASON_NONE)
    VH_TRY(discard_dev(ctx, crds, diameters, scores, n, min_radial_separation_ratio, max_volume_overlap_large,
                       max_volume_overlap_small, sort_criteria, scale, &plan));
  int path = VISFD_HIP_DISCARD_OVERLAP_PATH_DEVICE;
  if (by_option || (plan.reason != VISFD_HIP_DISCARD_OVERLAP_REASON_NONE && !plan.on_host)) {
    // the device arrays down, the host entry, the kept list up
    path = by_option ? VISFD_HIP_DISCARD_OVERLAP_PATH_HOST : VISFD_HIP_DISCARD_OVERLAP_PATH_HANDED_OVER;
    plan.hc.resize(3 * (size_t)n); plan.hd.resize((size_t)n); plan.hs.resize((size_t)n);
    if (n > 0) {
      VH_HIP(hipMemcpyAsync(plan.hc.data(), crds, sizeof(float) * 3 * (size_t)n, hipMemcpyDeviceToHost, ctx->stream));
      VH_HIP(hipMemcpyAsync(plan.hd.data(), diameters, sizeof(float) * (size_t)n, hipMemcpyDeviceToHost, ctx->stream));
      VH_HIP(hipMemcpyAsync(plan.hs.data(), scores, sizeof(float) * (size_t)n, hipMemcpyDeviceToHost, ctx->stream));
      VH_HIP(hipStreamSynchronize(ctx->stream));
    }
    int64_t m = n;
    VH_TRY(visfd_hip_discard_overlapping_blobs(plan.hc.data(), plan.hd.data(), plan.hs.data(), &m, min_radial_separation_ratio,
                                               max_volume_overlap_large, max_volume_overlap_small, sort_criteria, scale));
    plan.kept = m;
    plan.on_host = true;
  } else if (plan.on_host) {
    path = VISFD_HIP_DISCARD_OVERLAP_PATH_HANDED_OVER;
  }
  if (plan.on_host && plan.kept > 0) {
    const size_t k = (size_t)plan.kept;
    VH_HIP(hipMemcpyAsync(crds, plan.hc.data(), sizeof(float) * 3 * k, hipMemcpyHostToDevice, ctx->stream));
    VH_HIP(hipMemcpyAsync(diameters, plan.hd.data(), sizeof(float) * k, hipMemcpyHostToDevice, ctx->stream));
    VH_HIP(hipMemcpyAsync(scores, plan.hs.data(), sizeof(float) * k, hipMemcpyHostToDevice, ctx->stream));
    VH_HIP(hipStreamSynchronize(ctx->stream));
  }
  *n_inout = plan.kept;
  remember(ctx, path, plan, n, plan.kept);
  return VISFD_HIP_OK;
}

}  // extern "C"
