// wave.hpp -- the wave-level idioms of the kernels, once: reductions, scans, ranks and appends over a wave's 64 lanes.
// Device code only.  The contract every caller keeps:
//  1. All 64 lanes of the wave make the call: none has returned or sits in a branch or loop trip the others have left.
//     Callers round loop bounds up to whole waves and give idle lanes a neutral value; where the three lines above a
//     call do not show it, a comment there says why the wave is whole.
//  2. wave_lane() is threadIdx.x & 63: the lane only where the block's x-extent is a multiple of 64.  Other callers pass
//     their own lane to the helpers that take one, and do not call those that say they use wave_lane().
//  3. A reduction is the xor butterfly with offsets 32, 16, 8, 4, 2, 1, in that order, the result in every lane.  The
//     order is part of the contract: connect_graph.hip sums doubles with it, and the sum's bits depend on it.
#pragma once
#include <hip/hip_runtime.h>

namespace vh {
constexpr int WAVE = 64;
__device__ __forceinline__ int wave_lane() { return threadIdx.x & (WAVE - 1); }

// op(a, b) over the wave's values of v, in every lane (contract 3)
template <typename T, typename Op>
__device__ __forceinline__ T wave_reduce(T v, Op op) {
#pragma unroll
  for (int o = WAVE / 2; o > 0; o >>= 1) v = op(v, __shfl_xor(v, o, WAVE));
  return v;
}
template <typename T> __device__ __forceinline__ T wave_sum(T v) { return wave_reduce(v, [](T a, T b) { return a + b; }); }
template <typename T> __device__ __forceinline__ T wave_min(T v) { return wave_reduce(v, [](T a, T b) { return b < a ? b : a; }); }
template <typename T> __device__ __forceinline__ T wave_max(T v) { return wave_reduce(v, [](T a, T b) { return b > a ? b : a; }); }
template <typename T> __device__ __forceinline__ T wave_or(T v) { return wave_reduce(v, [](T a, T b) { return a | b; }); }

// inclusive scan: lane l gets op over the values of lanes 0..l; without an op, their sum
template <typename T, typename Op>
__device__ __forceinline__ T wave_scan(T v, int lane, Op op) {
#pragma unroll
  for (int d = 1; d < WAVE; d <<= 1) {
    const T u = __shfl_up(v, d, WAVE);
    if (lane >= d) v = op(v, u);
  }
  return v;
}
template <typename T> __device__ __forceinline__ T wave_scan(T v, int lane) { return wave_scan(v, lane, [](T a, T b) { return a + b; }); }

// of a ballot: the first set lane (-1: none), and the number of set lanes below `lane`
__device__ __forceinline__ int wave_leader(unsigned long long mask) { return __ffsll((long long)mask) - 1; }
__device__ __forceinline__ int wave_rank(unsigned long long mask, int lane) { return __popcll(mask & ((1ull << lane) - 1ull)); }

// position of a hit in the list behind `counter`: one atomic per wave (0 in a wave without a hit).  Uses wave_lane().
__device__ __forceinline__ unsigned long long wave_append(bool hit, unsigned long long* counter) {
  const unsigned long long m = __ballot(hit);
  if (m == 0) return 0;
  const int lane = wave_lane();
  const int first = wave_leader(m);
  unsigned long long base = 0;
  if (lane == first) base = atomicAdd(counter, (unsigned long long)__popcll(m));
  base = __shfl(base, first);
  return base + wave_rank(m, lane);
}

// *counter += the wave's sum of `mine`: one atomic, none for a sum of zero.  Uses wave_lane().
__device__ __forceinline__ void wave_count(unsigned long long mine, unsigned long long* counter) {
  mine = wave_sum(mine);
  if (wave_lane() == 0 && mine) atomicAdd(counter, mine);
}

// key < 0: the lane holds nothing.  True when the lanes that hold a key agree on it; it is then *common (-1 where no lane
// holds any), and the wave can send one atomic for all of them.
__device__ __forceinline__ bool wave_agree(int key, int* common) {
  const unsigned long long holds = __ballot(key >= 0);
  if (!holds) { *common = -1; return true; }
  const int first = __shfl(key, wave_leader(holds));
  *common = first;
  return __ballot(key >= 0 && key != first) == 0;
}
}  // namespace vh
