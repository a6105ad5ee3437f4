// morph_levels.hip -- flat-ball morphology of images that hold at most two levels, at any radius.
//
// DilateSphere with bmax == 0 (reference lib/visfd/morphology.hpp:253-263) keeps offset (ix, iy, iz) when
// (float)sqrt((double)(ix^2 + iy^2 + iz^2)) <= radius, inside a cube of half-width ceil(max(radius, radius_max)).  The
// test is monotone in d^2 = ix^2 + iy^2 + iz^2 and every offset that passes has |component| <= radius, so the element is
// {d^2 <= T} with T = host_flat_ball_dsq_max(radius), whatever the cube.  On an image whose voxels with mask != 0 hold
// the levels lo < hi only, the element walk of csrc/morph.hip therefore gives, at every voxel x with mask != 0,
//
//   dilation   hi + 0.0f  if some voxel of level hi (mask != 0) lies within d^2 <= T of x, else lo + 0.0f
//   erosion    lo         if some voxel of level lo (mask != 0) lies within d^2 <= T of x, else hi   (f - (+0) is f)
//
// (x itself is a candidate, so one of the two always holds), and that is a threshold on the exact squared distance to
// the nearest voxel of a level: csrc/distance.hip computes it in O(voxels) at any radius.  Nothing is built or uploaded
// per radius; open, close and the top-hats are the same two steps and epilogues as morph_run's, the levels of the
// second step following from the first (a dilation turns -0 into +0).  A one-level image is the case lo == hi.
//
// Eligibility is decided by census_kernel: one sweep of source and mask, 16 bytes per lane and array.  A wave keeps the
// patterns it has met in two uniform registers (a ballot finds the lanes that hold another one); a third pattern, a NaN
// or a pair that compares equal (+0 / -0) sets the record's flag at once, and every wave reads the flag before each
// tile, so a noise volume is turned away after its first tiles.  At its end a wave puts its patterns into the record's
// two slots by compare-and-swap (a slot goes from empty to one pattern, once); a pattern that finds both slots taken by
// others sets the flag.  The record is all the host reads back.
#include <algorithm>
#include <cmath>
#include <cstring>

#include "common.hpp"
#include "wave.hpp"

namespace vh {

namespace {

constexpr int BLOCK = 256;
constexpr int TILE_VECS = 4;   // float4 loads in flight per lane and array

// slot: 0 = empty, else 2^32 | the pattern
struct CensusRecord {
  unsigned long long slot[2];
  unsigned flag;   // not eligible
  unsigned pad[3];
};

// the patterns a wave has met: the same values in every lane
struct WaveLevels {
  unsigned w0 = 0, w1 = 0;
  int n = 0;
  bool bad = false;
};

// every lane of the wave calls this together; `valid`: the lane holds a voxel with mask != 0
__device__ __forceinline__ void census_fold(WaveLevels& L, unsigned bits, bool valid) {
  const float f = __uint_as_float(bits);
  if (__ballot(valid && f != f)) {
    L.bad = true;
    return;
  }
  unsigned long long pend = __ballot(valid && !(L.n > 0 && bits == L.w0) && !(L.n > 1 && bits == L.w1));
  while (pend) {   // at most two rounds
    if (L.n == 2) {
      L.bad = true;
      return;
    }
    const unsigned p = (unsigned)__shfl((int)bits, wave_leader(pend), WAVE);
    if (L.n == 0) L.w0 = p; else L.w1 = p;
    L.n++;
    pend = __ballot(valid && bits != L.w0 && !(L.n > 1 && bits == L.w1));
  }
  if (L.n == 2 && __uint_as_float(L.w0) == __uint_as_float(L.w1)) L.bad = true;
}

__device__ __forceinline__ bool census_flagged(CensusRecord* rec) {
  return __hip_atomic_load(&rec->flag, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0u;
}

__device__ __forceinline__ void census_merge(CensusRecord* rec, unsigned bits) {
  const unsigned long long key = (1ull << 32) | bits;
  for (int s = 0; s < 2; s++) {
    const unsigned long long old = atomicCAS(&rec->slot[s], 0ull, key);
    if (old == 0ull || old == key) return;
  }
  atomicOr(&rec->flag, 1u);
}

// VEC: src and mask are 16-byte aligned; the n4 = n / 4 whole float4 go through the tiles, the last n % 4 voxels through
// the first wave.  Otherwise every voxel goes through one-float tiles.
template <bool VEC>
__global__ void __launch_bounds__(BLOCK)
census_kernel(const float* __restrict__ src, const float* __restrict__ mask, i64 n, CensusRecord* __restrict__ rec) {
  const int lane = wave_lane();
  const i64 wave = (i64)blockIdx.x * (BLOCK / WAVE) + (threadIdx.x >> 6);
  const i64 nwaves = (i64)gridDim.x * (BLOCK / WAVE);
  WaveLevels L;
  const i64 items = VEC ? n / 4 : n;                                  // float4 or float
  const i64 ntiles = (items + WAVE * TILE_VECS - 1) / (WAVE * TILE_VECS);
  for (i64 t = wave; t < ntiles && !L.bad; t += nwaves) {
    if (census_flagged(rec)) return;   // somebody else has seen enough (one load of one word: the whole wave leaves, or none of it)
    const i64 i0 = t * (WAVE * TILE_VECS) + lane;
    if (VEC) {
      const float4* s4 = reinterpret_cast<const float4*>(src);
      const float4* m4 = reinterpret_cast<const float4*>(mask);
      float4 v[TILE_VECS], k[TILE_VECS];
#pragma unroll
      for (int j = 0; j < TILE_VECS; j++) {
        const i64 i = i0 + (i64)j * WAVE;
        v[j] = i < items ? s4[i] : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        k[j] = (i < items && mask) ? m4[i] : make_float4(1.0f, 1.0f, 1.0f, 1.0f);
      }
#pragma unroll
      for (int j = 0; j < TILE_VECS; j++) {
        const bool in = i0 + (i64)j * WAVE < items;
        census_fold(L, __float_as_uint(v[j].x), in && k[j].x != 0.0f);
        census_fold(L, __float_as_uint(v[j].y), in && k[j].y != 0.0f);
        census_fold(L, __float_as_uint(v[j].z), in && k[j].z != 0.0f);
        census_fold(L, __float_as_uint(v[j].w), in && k[j].w != 0.0f);
      }
    } else {
      float v[TILE_VECS], k[TILE_VECS];
#pragma unroll
      for (int j = 0; j < TILE_VECS; j++) {
        const i64 i = i0 + (i64)j * WAVE;
        v[j] = i < items ? src[i] : 0.0f;
        k[j] = (i < items && mask) ? mask[i] : 1.0f;
      }
#pragma unroll
      for (int j = 0; j < TILE_VECS; j++)
        census_fold(L, __float_as_uint(v[j]), i0 + (i64)j * WAVE < items && k[j] != 0.0f);
    }
  }
  if (VEC && wave == 0 && !L.bad) {
    const i64 i = (n / 4) * 4 + lane;
    const bool in = i < n;
    const float v = in ? src[i] : 0.0f;
    const float k = (in && mask) ? mask[i] : 1.0f;
    census_fold(L, __float_as_uint(v), in && k != 0.0f);
  }
  if (lane != 0) return;
  if (L.bad) {
    atomicOr(&rec->flag, 1u);
    return;
  }
  if (L.n > 0) census_merge(rec, L.w0);
  if (L.n > 1) census_merge(rec, L.w1);
}

// at most two levels among the voxels with mask != 0, no NaN, the two unequal: *count of them in lv[0] <= lv[1], or
// *eligible = false
int census(visfd_hip_ctx* ctx, const float* src, const float* mask, i64 n, bool* eligible, int* count, float lv[2]) {
  CensusRecord* rec = nullptr;
  VH_TRY(ws(ctx, WS_DIST_POINTS, sizeof(CensusRecord) / sizeof(int), reinterpret_cast<int**>(&rec)));
  VH_HIP(hipMemsetAsync(rec, 0, sizeof(CensusRecord), ctx->stream));
  const bool vec = (reinterpret_cast<uintptr_t>(src) % 16 == 0) && (reinterpret_cast<uintptr_t>(mask) % 16 == 0);
  const i64 per_block = (i64)BLOCK * TILE_VECS * (vec ? 4 : 1);
  const unsigned grid = grid_for(n, (int)per_block, (i64)ctx->num_cus * 8);
  if (vec) census_kernel<true><<<grid, BLOCK, 0, ctx->stream>>>(src, mask, n, rec);
  else census_kernel<false><<<grid, BLOCK, 0, ctx->stream>>>(src, mask, n, rec);
  VH_HIP(hipGetLastError());
  CensusRecord h;
  VH_HIP(hipMemcpyAsync(&h, rec, sizeof(h), hipMemcpyDeviceToHost, ctx->stream));
  VH_HIP(hipStreamSynchronize(ctx->stream));
  *eligible = false;
  *count = 0;
  if (h.flag) return VISFD_HIP_OK;
  for (int s = 0; s < 2; s++) {
    if (!h.slot[s]) continue;
    const unsigned bits = (unsigned)h.slot[s];
    std::memcpy(&lv[(*count)++], &bits, 4);
  }
  if (*count == 2) {
    if (lv[0] == lv[1]) return VISFD_HIP_OK;   // +0 and -0 from different waves
    if (lv[1] < lv[0]) std::swap(lv[0], lv[1]);
  }
  *eligible = true;
  return VISFD_HIP_OK;
}

unsigned bits_of(float f) {
  unsigned u;
  std::memcpy(&u, &f, 4);
  return u;
}

}  // namespace

i64 host_flat_ball_dsq_max(float radius) {
  // the test is monotone in n (sqrt and both roundings are) and holds at 0: bisect for its last n; saturates at 2^62
  i64 lo = 0, hi = (i64)1 << 62;
  if ((float)std::sqrt((double)hi) <= radius) return hi;
  while (hi - lo > 1) {   // test(lo) holds, test(hi) does not
    const i64 mid = lo + (hi - lo) / 2;
    if ((float)std::sqrt((double)mid) <= radius) lo = mid; else hi = mid;
  }
  return lo;
}

int morph_levels_try(visfd_hip_ctx* ctx, const float* src, float* dst, const float* mask, i64 nx, i64 ny, i64 nz, int op,
                     float radius, float radius_max, float bmax, bool* taken) {
  *taken = false;
  const int mode = ctx->opt.morph_levels;
  if (mode == 0 || ctx->opt.morph_general) return VISFD_HIP_OK;
  if (!(bmax == 0.0f) || !std::isfinite(radius) || radius < 0.0f || !std::isfinite(radius_max)) return VISFD_HIP_OK;
  if (nx + ny + nz > VISFD_HIP_DISTANCE_MAX_DIM_SUM) return VISFD_HIP_OK;
  if (mode == 1 && !(std::ceil(radius) > (float)MORPH_RUN_MAX_R || radius >= MORPH_LEVELS_R0)) return VISFD_HIP_OK;
  const i64 nv = nx * ny * nz;
  bool eligible = false;
  int count = 0;
  float lv[2] = {0.0f, 0.0f};
  VH_TRY(census(ctx, src, mask, nv, &eligible, &count, lv));
  if (!eligible) return VISFD_HIP_OK;
  float lo = lv[0], hi = count == 2 ? lv[1] : lv[0];   // no voxel with mask != 0: nothing is written, any level does

  const i64 S = nx + ny + nz;
  const int t = (int)std::min<i64>(host_flat_ball_dsq_max(radius), S * S - 1);   // distances inside the image are below cap = S^2
  int* dsq = nullptr;
  VH_TRY(ws(ctx, WS_DIST_DSQ, (size_t)nv, &dsq));
  // one Dilate / Erode of an image with the levels lo <= hi: the seeds are the voxels of the level that spreads
  auto step = [&](const float* s, float* d, bool dilate, int epi, bool nan_masked) -> int {
    LevelsEpilogue e;
    e.dst = d;
    e.mask = mask;
    e.t = t;
    e.near_bits = bits_of(dilate ? hi + 0.0f : lo);
    e.far_bits = bits_of(dilate ? lo + 0.0f : hi);
    e.epi = epi;
    e.nan_masked = nan_masked ? 1 : 0;
    VH_TRY(dev_distance_levels(ctx, s, mask, nx, ny, nz, dilate ? hi : lo, dsq, e));
    if (dilate) {   // what the image holds now
      lo = lo + 0.0f;
      hi = hi + 0.0f;
    }
    return VISFD_HIP_OK;
  };
  if (op == VISFD_HIP_MORPH_DILATE || op == VISFD_HIP_MORPH_ERODE) {
    VH_TRY(step(src, dst, op == VISFD_HIP_MORPH_DILATE, 0, false));
  } else {
    float* tmp = nullptr;
    VH_TRY(ws(ctx, WS_MORPH_TMP, (size_t)nv, &tmp));
    const bool dilate_first = (op == VISFD_HIP_MORPH_CLOSE || op == VISFD_HIP_MORPH_TOP_HAT_BLACK);
    const int epi = op == VISFD_HIP_MORPH_TOP_HAT_WHITE ? 1 : op == VISFD_HIP_MORPH_TOP_HAT_BLACK ? 2 : 0;
    VH_TRY(step(src, tmp, dilate_first, 0, mask != nullptr));
    VH_TRY(step(tmp, dst, !dilate_first, epi, false));
  }
  ctx->morph_last_path = VISFD_HIP_MORPH_PATH_LEVELS;
  *taken = true;
  return VISFD_HIP_OK;
}

}  // namespace vh

using namespace vh;

extern "C" int visfd_hip_flat_ball_dsq_max(float radius, int64_t* t) {
  VH_REQUIRE(t, "null argument");
  VH_REQUIRE(std::isfinite(radius) && radius >= 0.0f, "the radius of a flat ball must be finite and not negative");
  *t = host_flat_ball_dsq_max(radius);
  return VISFD_HIP_OK;
}
