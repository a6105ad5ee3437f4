// select.hip -- exact global top-fraction threshold of the ridge saliency
// (reference bin/filter_mrc/handlers.cpp:1751-1797).
//
// The reference sorts all unmasked saliencies in descending order on one thread and reads entry
// floor(n*fraction).  Here the same order statistic is found exactly with a three-digit radix
// select (11 + 11 + 10 bits) over the order-preserving 32-bit key of the float: each round is one
// 4 B/voxel sweep that builds a 2048-bin histogram in LDS per workgroup and merges it with a few
// global atomics.  Rounds also shard across GPUs: per-rank histograms are summed between a round's
// histogram and its pick (SelectReduce: the slab stage of slab.hip), or by a caller that walks with
// the public histogram entry points.
#include <cmath>
#include <vector>

#include "common.hpp"
#include "select_pick.hpp"

namespace vh {

namespace {

constexpr int BLOCK = 256;
constexpr int NBINS = 2048;

__device__ __forceinline__ uint32_t order_key(float f) {
  const uint32_t u = __float_as_uint(f);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__host__ __device__ inline float key_to_float(uint32_t k) {
  const uint32_t u = (k & 0x80000000u) ? (k & 0x7fffffffu) : ~k;
  float f;
  __builtin_memcpy(&f, &u, 4);
  return f;
}

// digit layout of the 32-bit key: round 0 = bits 31..21, round 1 = bits 20..10, round 2 = bits 9..0.
// `prefix` holds the already-selected higher digits (right-aligned); only keys matching it count.  DEVPREFIX: the digits
// come from the select's state block on the device, where pick_kernel left them (no host step between the rounds).
template <bool DEVPREFIX>
__global__ void __launch_bounds__(BLOCK)
histogram_kernel(const float* __restrict__ sal, const float* __restrict__ mask, i64 n, int round,
                 uint32_t prefix_arg, const SelectState* __restrict__ state, unsigned long long* __restrict__ hist) {
  __shared__ unsigned int lh[NBINS];
  const uint32_t prefix = DEVPREFIX ? state->prefix : prefix_arg;
  for (int i = threadIdx.x; i < NBINS; i += BLOCK) lh[i] = 0;
  __syncthreads();
  const int shift = (round == 0) ? 21 : (round == 1) ? 10 : 0;
  const uint32_t dmask = (round == 2) ? 0x3ffu : 0x7ffu;
  const int pshift = (round == 0) ? 32 : (round == 1) ? 21 : 10;
  auto count = [&](float v) {
    const uint32_t k = order_key(v);
    if (round > 0 && (k >> pshift) != prefix) return;
    atomicAdd(&lh[(k >> shift) & dmask], 1u);
  };
  const i64 step = (i64)gridDim.x * BLOCK;
  // four values per load, two loads in flight (one dword per thread and trip ran at 3.3 TB/s); the tail and unaligned or
  // masked volumes one by one
  const i64 n4 = (!mask && (reinterpret_cast<uintptr_t>(sal) & 15u) == 0) ? (n >> 2) : 0;
  const float4* sal4 = reinterpret_cast<const float4*>(sal);
  i64 j = (i64)blockIdx.x * BLOCK + threadIdx.x;
  for (; j + step < n4; j += 2 * step) {
    const float4 a = sal4[j], b = sal4[j + step];
    count(a.x); count(a.y); count(a.z); count(a.w);
    count(b.x); count(b.y); count(b.z); count(b.w);
  }
  if (j < n4) {
    const float4 a = sal4[j];
    count(a.x); count(a.y); count(a.z); count(a.w);
  }
  for (i64 i = 4 * n4 + (i64)blockIdx.x * BLOCK + threadIdx.x; i < n; i += step) {
    if (mask && mask[i] == 0.0f) continue;
    count(sal[i]);
  }
  __syncthreads();
  for (int i = threadIdx.x; i < NBINS; i += BLOCK) {
    const unsigned int c = lh[i];
    if (c) atomicAdd(&hist[i], (unsigned long long)c);
  }
}

// The host's step between two rounds, on the device: ONE workgroup reads the round's histogram (and zeroes it for the next
// round), thread 0 walks it from the top -- first the 256 sums of 8 neighbouring bins, then the 8 bins of the chunk that walk
// stops in: the same bin and the same remainder as one walk over all 2048, by the same function -- and leaves {digits so
// far, rank left} in the state block; after round 2 the threshold itself.  Round 0 also turns its total into the rank.
__global__ void __launch_bounds__(BLOCK)
pick_kernel(unsigned long long* __restrict__ hist, int round, float fraction, SelectState* __restrict__ state) {
  constexpr int PER = NBINS / BLOCK;
  __shared__ uint64_t lh[NBINS];
  __shared__ uint64_t chunk[BLOCK];
  const int t = threadIdx.x;
  uint64_t sum = 0;
#pragma unroll
  for (int i = 0; i < PER; i++) {
    const uint64_t c = hist[t * PER + i];
    hist[t * PER + i] = 0;
    lh[t * PER + i] = c;
    sum += c;
  }
  chunk[t] = sum;
  __syncthreads();
  if (t != 0) return;
  uint64_t k = 0;
  uint32_t prefix = 0;
  if (round == 0) {
    uint64_t n = 0;
    for (int i = 0; i < BLOCK; i++) n += chunk[i];
    state->n = n;
    state->flag = 0;
    if (!select_rank(n, fraction, &k)) {
      state->flag = SELECT_NO_VOXEL;
      state->thr = __builtin_inff();   // (consumers queued behind a failed select keep nothing finite)
      return;
    }
  } else {
    if (state->flag) return;
    k = state->k;
    prefix = state->prefix;
  }
  const int c = select_pick_bin(chunk, BLOCK, &k);
  const int d = c < 0 ? -1 : select_pick_bin(lh + c * PER, PER, &k);
  if (d < 0) {
    state->flag = SELECT_INCONSISTENT;
    state->thr = __builtin_inff();
    return;
  }
  prefix = (prefix << (round == 2 ? 10 : 11)) | (uint32_t)(c * PER + d);
  state->prefix = prefix;
  state->k = k;
  if (round == 2) state->thr = key_to_float(prefix);
}

__global__ void __launch_bounds__(BLOCK)
apply_threshold_kernel(float* __restrict__ sal, i64 n, float thr) {
  i64 i = (i64)blockIdx.x * BLOCK + threadIdx.x;
  const i64 step = (i64)gridDim.x * BLOCK;
  for (; i < n; i += step) {
    const float s = sal[i];
    if (s < thr) sal[i] = 0.0f;
  }
}

}  // namespace

int dev_select_histogram(visfd_hip_ctx* ctx, const float* sal, const float* mask, i64 nvox, int pass,
                         uint32_t prefix, uint64_t* hist_host, uint64_t* n_unmasked_host) {
  // per-workgroup counters are 32-bit: each workgroup sees at most nvox/grid + BLOCK elements
  unsigned long long* hist = nullptr;
  VH_TRY(ws(ctx, WS_HIST, (size_t)NBINS, &hist));
  hipStream_t st = ctx->stream;
  VH_HIP(hipMemsetAsync(hist, 0, sizeof(unsigned long long) * NBINS, st));
  const unsigned g = grid_for(nvox, BLOCK, (i64)ctx->num_cus * 32);
  histogram_kernel<false><<<dim3(g), dim3(BLOCK), 0, st>>>(sal, mask, nvox, pass, prefix, nullptr, hist);
  VH_HIP(hipGetLastError());
  VH_HIP(hipMemcpyAsync(hist_host, hist, sizeof(uint64_t) * NBINS, hipMemcpyDeviceToHost, st));
  VH_HIP(hipStreamSynchronize(st));
  if (n_unmasked_host) {
    uint64_t tot = 0;
    for (int b = 0; b < NBINS; b++) tot += hist_host[b];
    *n_unmasked_host = tot;
  }
  return VISFD_HIP_OK;
}

// The same histogram left on the device (2048 counters, zeroed here first), asynchronous: multi-GPU callers all-reduce it
// there and fetch the sum once.
int dev_select_histogram_todev(visfd_hip_ctx* ctx, const float* sal, const float* mask, i64 nvox, int pass, uint32_t prefix,
                               uint64_t* hist) {
  hipStream_t st = ctx->stream;
  VH_HIP(hipMemsetAsync(hist, 0, sizeof(unsigned long long) * NBINS, st));
  const unsigned g = grid_for(nvox, BLOCK, (i64)ctx->num_cus * 32);
  histogram_kernel<false><<<dim3(g), dim3(BLOCK), 0, st>>>(sal, mask, nvox, pass, prefix, nullptr, reinterpret_cast<unsigned long long*>(hist));
  VH_HIP(hipGetLastError());
  return VISFD_HIP_OK;
}

int dev_apply_threshold(visfd_hip_ctx* ctx, float* sal, i64 nvox, float thr) {
  const unsigned g = grid_for(nvox, BLOCK, (i64)ctx->num_cus * 32);
  apply_threshold_kernel<<<dim3(g), dim3(BLOCK), 0, ctx->stream>>>(sal, nvox, thr);
  VH_HIP(hipGetLastError());
  return VISFD_HIP_OK;
}

// The whole select queued with no host step: the three histogram / pick pairs.  *state (device memory) then holds the
// threshold, or a flag that select_result turns into the error.  A masked select takes its n from round 0's total.
// reduce (nullable): the ranks of a slab run sum their counters between a round's histogram and its pick (SelectReduce),
// so pick_kernel applies select_rank to the GLOBAL n and walks the global histogram -- the single volume's select on the
// single volume's counts.  A fraction that selects no voxel is flagged by round 0's pick; rounds 1 and 2 are queued all the
// same (their picks return at once), so every rank makes the same three reductions whatever the outcome.
int dev_select_queue(visfd_hip_ctx* ctx, const float* sal, const float* mask, i64 nvox, float fraction, SelectState* state,
                     const SelectReduce* reduce) {
  unsigned long long* hist = nullptr;
  VH_TRY(ws(ctx, WS_HIST, (size_t)NBINS, &hist));
  hipStream_t st = ctx->stream;
  VH_HIP(hipMemsetAsync(hist, 0, sizeof(unsigned long long) * NBINS, st));   // (every pick leaves it zeroed for the next round)
  const unsigned g = grid_for(nvox, BLOCK, (i64)ctx->num_cus * 32);
  for (int round = 0; round < 3; round++) {
    histogram_kernel<true><<<dim3(g), dim3(BLOCK), 0, st>>>(sal, mask, nvox, round, 0u, state, hist);
    if (reduce) VH_TRY(reduce->sum(reduce->user, reinterpret_cast<uint64_t*>(hist), (size_t)NBINS, st));
    pick_kernel<<<dim3(1), dim3(BLOCK), 0, st>>>(hist, round, fraction, state);
  }
  VH_HIP(hipGetLastError());
  return VISFD_HIP_OK;
}

static const char* const kNoVoxel = "threshold fraction selects no voxel (the reference would read past its array)";
static const char* const kInconsistent = "radix select: inconsistent histogram";

int select_result(const SelectState& s, float* thr_out) {
  if (s.flag & SELECT_NO_VOXEL) return fail(VISFD_HIP_EINVAL, kNoVoxel);
  if (s.flag) return fail(VISFD_HIP_EDEVICE, kInconsistent);
  if (thr_out) *thr_out = s.thr;
  return VISFD_HIP_OK;
}
int select_rank_check(uint64_t n, float fraction) {
  uint64_t k = 0;
  if (!select_rank(n, fraction, &k)) return fail(VISFD_HIP_EINVAL, kNoVoxel);
  return VISFD_HIP_OK;
}

// The rounds queued back to back with the digit picked on the device and ONE wait for the state block; sal is cut only once
// the threshold is known to exist.  With `reduce` it is the slab stage's select over all ranks' owned voxels.
int dev_threshold_queued(visfd_hip_ctx* ctx, float* sal, const float* mask, i64 nvox, float fraction, float* thr_out,
                         const SelectReduce* reduce) {
  StageReadback* block = nullptr;   // (the slot's one layout; only the select's part is used here)
  VH_TRY(ws(ctx, WS_SELECT, 1, &block));
  VH_TRY(dev_select_queue(ctx, sal, mask, nvox, fraction, &block->sel, reduce));
  SelectState got;
  VH_HIP(hipMemcpyAsync(&got, &block->sel, sizeof(got), hipMemcpyDeviceToHost, ctx->stream));
  VH_HIP(hipStreamSynchronize(ctx->stream));
  float thr = 0.0f;
  VH_TRY(select_result(got, &thr));
  if (thr_out) *thr_out = thr;
  return dev_apply_threshold(ctx, sal, nvox, thr);
}

// Option membrane_queue: the queued form above; 0: a wait and a host walk after every round.  The same bits either way.
int dev_threshold_fraction(visfd_hip_ctx* ctx, float* sal, const float* mask, i64 nvox, float fraction,
                           float* thr_out) {
  if (ctx->opt.membrane_queue) return dev_threshold_queued(ctx, sal, mask, nvox, fraction, thr_out);
  std::vector<uint64_t> h(NBINS);
  uint64_t n_unmasked = 0, k = 0;
  VH_TRY(dev_select_histogram(ctx, sal, mask, nvox, 0, 0, h.data(), &n_unmasked));
  if (!select_rank(n_unmasked, fraction, &k)) return fail(VISFD_HIP_EINVAL, kNoVoxel);
  uint32_t key = 0;
  for (int round = 0; round < 3; round++) {
    if (round > 0) VH_TRY(dev_select_histogram(ctx, sal, mask, nvox, round, key, h.data(), nullptr));
    const int d = select_pick_bin(h.data(), NBINS, &k);
    if (d < 0) return fail(VISFD_HIP_EDEVICE, kInconsistent);
    key = (key << (round == 2 ? 10 : 11)) | (uint32_t)d;
  }
  const float thr = key_to_float(key);
  if (thr_out) *thr_out = thr;
  return dev_apply_threshold(ctx, sal, nvox, thr);
}

}  // namespace vh
