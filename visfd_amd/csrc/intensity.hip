// intensity.hip -- image statistics with an exact sum, and the intensity maps that end a filter_mrc run (the semantics
// are stated in include/visfd_hip.h, the scalar arithmetic is csrc/intensity.hpp).
//
// One kernel, intensity_kernel<MAP, STATS>: MAP applies vh_intensity::apply to every voxel and stores it, STATS adds the
// value it has read (or written) to the statistics.  Elements [0, head) and the last tail < 4 are taken one per lane,
// the 4 * nvec between them as float4: head is where the arrays reach a 16-byte boundary, which needs their addresses to
// agree modulo 16 -- where they do not, everything is `head`.
//
// The exact sum.  A finite float is m * 2^(max(e, 1) - 150) with e its exponent field and m its 24-bit mantissa (the
// hidden bit included unless e == 0).  Per e the kernel keeps three integers: the sum of the m of the positive values, the
// sum of the m of the negative values (64-bit each: 2^33 voxels * 2^24 < 2^64) and the OR of all m.  Integer adds commute,
// so the bins do not depend on the grid or on which workgroup comes first.  A wave reduces before it touches LDS: it
// takes the exponent of its first pending lane, adds up the lanes that share it with shuffles, and one lane issues the
// three LDS atomics; tomogram values share two or three exponents, so that is two or three rounds per 64 values.  A
// workgroup adds its non-empty bins to the global ones once, at its end.  The host then forms P = sum pos[e] << shift(e) and
// N likewise as multi-word integers, rounds P - N once to double, and proves order-freedom from P + N and the lowest bit
// set in any mantissa (combine()).
#include <algorithm>

#include "common.hpp"
#include "intensity.hpp"
#include "wave.hpp"

namespace vh {

namespace {

constexpr int BLOCK = 256;
constexpr int NBINS = 256;   // exponent fields 0..254 (255: not finite, counted apart)

// the same layout in LDS, in the workspace slot and on the host
struct StatsBins {
  unsigned long long pos[NBINS], neg[NBINS];
  unsigned long long count, nonfinite;
  unsigned int orr[NBINS];
  unsigned int min_key_inv, max_key;   // ~(smallest key) and the largest key, so that zeros are the empty state
};

__host__ __device__ inline uint32_t key_of(uint32_t u) { return (u & 0x80000000u) ? ~u : (u | 0x80000000u); }
__host__ __device__ inline uint32_t bits_of(uint32_t k) { return (k & 0x80000000u) ? (k & 0x7fffffffu) : ~k; }

// what a thread carries between values
struct Tally {
  unsigned long long count = 0, nonfinite = 0;
  uint32_t min_key_inv = 0, max_key = 0;
};

// Every lane of the wave calls this together; `take`: the lane has a value for the statistics.
__device__ __forceinline__ void tally(StatsBins* lds, Tally& t, float v, bool take, int lane) {
  const uint32_t u = __float_as_uint(v);
  const uint32_t e = (u >> 23) & 255u;
  const bool fin = take && e != 255u;
  const uint32_t m = e ? ((u & 0x7fffffu) | 0x800000u) : (u & 0x7fffffu);
  if (take) {
    t.count++;
    if (e == 255u) t.nonfinite++;
    else {
      const uint32_t k = key_of(u);
      t.min_key_inv = max(t.min_key_inv, ~k);
      t.max_key = max(t.max_key, k);
    }
  }
  const bool pending = fin && m != 0u;
  unsigned long long todo = __ballot(pending);
  while (todo) {   // the same for every lane
    const int leader = wave_leader(todo);
    const uint32_t e0 = __shfl(e, leader);
    const bool mine = pending && e == e0;
    const uint32_t p = wave_sum(mine && !(u >> 31) ? m : 0u);   // 64 * 2^24 fits
    const uint32_t q = wave_sum(mine && (u >> 31) ? m : 0u);
    const uint32_t o = wave_or(mine ? m : 0u);
    if (lane == 0) {
      if (p) atomicAdd(&lds->pos[e0], (unsigned long long)p);
      if (q) atomicAdd(&lds->neg[e0], (unsigned long long)q);
      atomicOr(&lds->orr[e0], o);
    }
    todo &= ~__ballot(mine);
  }
}

struct KernelArgs {
  const float* in;     // MAP: the threshold family's input (null when not read); !MAP: the image
  float* out;          // MAP only
  const float* mask;
  i64 head, nvec, n;   // n = head + 4 * nvec + tail
  int load_out;        // MAP: the stages look at what out holds
  visfd_hip_intensity p;
};

template <bool MAP, bool STATS>
__device__ __forceinline__ float one_voxel(const KernelArgs& a, float vin, float vout, float mk, bool* take) {
  const bool in_mask = !a.mask || mk != 0.0f;
  if (!MAP) {
    *take = in_mask;
    return vin;
  }
  *take = !a.p.stats_mask || in_mask;
  return vh_intensity::apply(a.p, vin, vout, in_mask);
}

template <bool MAP, bool STATS>
__global__ void __launch_bounds__(BLOCK) intensity_kernel(KernelArgs a, StatsBins* bins) {
  __shared__ StatsBins lds;
  const int tid = threadIdx.x, lane = wave_lane();
  if (STATS) {
    for (int b = tid; b < NBINS; b += BLOCK) {
      lds.pos[b] = 0;
      lds.neg[b] = 0;
      lds.orr[b] = 0;
    }
    if (tid == 0) {
      lds.count = 0;
      lds.nonfinite = 0;
      lds.min_key_inv = 0;
      lds.max_key = 0;
    }
    __syncthreads();
  }
  Tally t;
  const i64 stride = (i64)gridDim.x * BLOCK;
  const i64 wave0 = (i64)blockIdx.x * BLOCK + (tid & ~63);   // the wave's first item: a wave's trip counts are uniform
  // the elements taken one by one: [0, head) and the tail behind the vectors
  const i64 nscalar = a.n - 4 * a.nvec;
  for (i64 w = wave0; w < nscalar; w += stride) {
    const i64 j = w + lane;
    const bool have = j < nscalar;
    float v = 0.0f;
    bool take = false;
    if (have) {
      const i64 i = j < a.head ? j : j + 4 * a.nvec;
      const float mk = a.mask ? a.mask[i] : 1.0f;
      const float vin = a.in ? a.in[i] : 0.0f;
      const float vout = (MAP && a.load_out) ? a.out[i] : 0.0f;
      v = one_voxel<MAP, STATS>(a, vin, vout, mk, &take);
      if (MAP) a.out[i] = v;
    }
    if (STATS) tally(&lds, t, v, have && take, lane);
  }
  // the vectors
  const float4* in4 = a.in ? reinterpret_cast<const float4*>(a.in + a.head) : nullptr;
  const float4* mask4 = a.mask ? reinterpret_cast<const float4*>(a.mask + a.head) : nullptr;
  float4* out4 = MAP ? reinterpret_cast<float4*>(a.out + a.head) : nullptr;
  for (i64 w = wave0; w < a.nvec; w += stride) {
    const i64 j = w + lane;
    const bool have = j < a.nvec;
    float v[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    bool take[4] = {false, false, false, false};
    if (have) {
      const float4 mk = mask4 ? mask4[j] : make_float4(1.0f, 1.0f, 1.0f, 1.0f);
      const float4 vin = in4 ? in4[j] : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
      const float4 vout = (MAP && a.load_out) ? out4[j] : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
      v[0] = one_voxel<MAP, STATS>(a, vin.x, vout.x, mk.x, &take[0]);
      v[1] = one_voxel<MAP, STATS>(a, vin.y, vout.y, mk.y, &take[1]);
      v[2] = one_voxel<MAP, STATS>(a, vin.z, vout.z, mk.z, &take[2]);
      v[3] = one_voxel<MAP, STATS>(a, vin.w, vout.w, mk.w, &take[3]);
      if (MAP) out4[j] = make_float4(v[0], v[1], v[2], v[3]);
    }
    if (STATS) {
#pragma unroll
      for (int c = 0; c < 4; c++) tally(&lds, t, v[c], have && take[c], lane);
    }
  }
  if (!STATS) return;
  if (t.count) {
    atomicAdd(&lds.count, t.count);
    if (t.nonfinite) atomicAdd(&lds.nonfinite, t.nonfinite);
    atomicMax(&lds.min_key_inv, t.min_key_inv);
    atomicMax(&lds.max_key, t.max_key);
  }
  __syncthreads();
  for (int b = tid; b < NBINS; b += BLOCK) {
    if (lds.pos[b]) atomicAdd(&bins->pos[b], lds.pos[b]);
    if (lds.neg[b]) atomicAdd(&bins->neg[b], lds.neg[b]);
    if (lds.orr[b]) atomicOr(&bins->orr[b], lds.orr[b]);
  }
  if (tid == 0 && lds.count) {
    atomicAdd(&bins->count, lds.count);
    if (lds.nonfinite) atomicAdd(&bins->nonfinite, lds.nonfinite);
    atomicMax(&bins->min_key_inv, lds.min_key_inv);
    atomicMax(&bins->max_key, lds.max_key);
  }
}

// ---- the host's half: bins -> visfd_hip_stats ------------------------------------------------------------------------
// A non-negative integer of 320 bits, enough for 2^64 * 2^(254 - 1) of the largest bin; bit 0 weighs 2^-149
struct Wide {
  static constexpr int W = 5;
  uint64_t w[W] = {0, 0, 0, 0, 0};
  void add_shifted(uint64_t v, int shift) {   // += v << shift
    if (!v) return;
    const int word = shift >> 6, bit = shift & 63;
    uint64_t part[2] = {v << bit, bit ? v >> (64 - bit) : 0};
    unsigned carry = 0;
    for (int k = word; k < W; k++) {
      const uint64_t add = (k - word < 2 ? part[k - word] : 0);
      if (k - word >= 2 && !carry) break;
      const uint64_t s = w[k] + add;
      const unsigned c1 = s < add;
      const uint64_t s2 = s + carry;
      const unsigned c2 = s2 < s;
      w[k] = s2;
      carry = c1 | c2;
    }
  }
  int compare(const Wide& o) const {
    for (int k = W - 1; k >= 0; k--)
      if (w[k] != o.w[k]) return w[k] < o.w[k] ? -1 : 1;
    return 0;
  }
  void sub(const Wide& o) {   // *this >= o
    unsigned borrow = 0;
    for (int k = 0; k < W; k++) {
      const uint64_t d = w[k] - o.w[k];
      const unsigned b1 = w[k] < o.w[k];
      const uint64_t d2 = d - borrow;
      const unsigned b2 = d < borrow;
      w[k] = d2;
      borrow = b1 | b2;
    }
  }
  void add(const Wide& o) {
    unsigned carry = 0;
    for (int k = 0; k < W; k++) {
      const uint64_t s = w[k] + o.w[k];
      const unsigned c1 = s < o.w[k];
      const uint64_t s2 = s + carry;
      const unsigned c2 = s2 < s;
      w[k] = s2;
      carry = c1 | c2;
    }
  }
  int bit_length() const {
    for (int k = W - 1; k >= 0; k--)
      if (w[k]) return 64 * k + 64 - __builtin_clzll(w[k]);
    return 0;
  }
  bool bit(int i) const { return (w[i >> 6] >> (i & 63)) & 1u; }
  bool any_below(int i) const {   // a bit set among bits [0, i)
    for (int k = 0; k < W; k++) {
      if (64 * (k + 1) <= i) {
        if (w[k]) return true;
      } else {
        const int r = i - 64 * k;
        return r > 0 && (w[k] & ((r >= 64 ? ~0ull : (1ull << r) - 1ull))) != 0;
      }
    }
    return false;
  }
  uint64_t bits_from(int lo, int count) const {   // bits [lo, lo + count), count <= 64
    uint64_t r = 0;
    for (int i = 0; i < count; i++)
      if (lo + i < 64 * W && bit(lo + i)) r |= 1ull << i;
    return r;
  }
  // the value times 2^-149, rounded to nearest, ties to even
  double to_double() const {
    const int len = bit_length();
    if (len <= 53) return std::ldexp((double)w[0], -149);   // exact: a double holds 53 bits at any exponent reached here
    const int drop = len - 53;
    uint64_t top = bits_from(drop, 53);
    const bool half = bit(drop - 1), sticky = any_below(drop - 1);
    if (half && (sticky || (top & 1ull))) top++;   // 2^53 after the carry is still exact
    return std::ldexp((double)top, drop - 149);
  }
};

inline int bin_shift(int e) { return (e ? e : 1) - 1; }   // the weight of bin e is 2^(bin_shift(e) - 149)

void combine(const StatsBins& b, visfd_hip_stats* out) {
  out->count = (int64_t)b.count;
  out->n_nonfinite = (int64_t)b.nonfinite;
  out->reserved = 0;
  Wide P, N;
  int q = 1 << 30;   // the lowest set bit of any value, as a bit position of Wide
  for (int e = 0; e < 255; e++) {
    P.add_shifted(b.pos[e], bin_shift(e));
    N.add_shifted(b.neg[e], bin_shift(e));
    if (b.orr[e]) q = std::min(q, bin_shift(e) + __builtin_ctz(b.orr[e]));
  }
  Wide M = P;
  M.add(N);
  const int c = P.compare(N);
  double s = 0.0;
  if (c > 0) {
    P.sub(N);
    s = P.to_double();
  } else if (c < 0) {
    N.sub(P);
    s = -N.to_double();
  }
  out->sum = s;
  out->order_free = (M.bit_length() <= q + 53) ? 1 : 0;   // sum |x| < 2^(q + 53); all zeros: 0 <= anything
  const bool any_finite = b.count > b.nonfinite;
  uint32_t lo = any_finite ? bits_of(~b.min_key_inv) : 0u, hi = any_finite ? bits_of(b.max_key) : 0u;
  std::memcpy(&out->min, &lo, 4);
  std::memcpy(&out->max, &hi, 4);
}

void host_tally(StatsBins* b, float v) {
  uint32_t u;
  std::memcpy(&u, &v, 4);
  const uint32_t e = (u >> 23) & 255u;
  b->count++;
  if (e == 255u) {
    b->nonfinite++;
    return;
  }
  const uint32_t k = key_of(u);
  b->min_key_inv = std::max(b->min_key_inv, ~k);
  b->max_key = std::max(b->max_key, k);
  const uint32_t m = e ? ((u & 0x7fffffu) | 0x800000u) : (u & 0x7fffffu);
  if (u >> 31) b->neg[e] += m;
  else b->pos[e] += m;
  b->orr[e] |= m;
}

int check_map(const float* in, const float* out, const float* mask, i64 nx, i64 ny, i64 nz, const visfd_hip_intensity* p) {
  VH_REQUIRE(out && p, "null argument");
  VH_TRY(check_dims(nx, ny, nz));
  VH_REQUIRE(p->map >= VISFD_HIP_MAP_NONE && p->map <= VISFD_HIP_MAP_RESCALE, "intensity map: unknown map kind");
  VH_REQUIRE(in || !vh_intensity::reads_input(p->map), "intensity map: the threshold maps need the input image");
  const i64 n = nx * ny * nz;
  VH_REQUIRE(in == out || !overlaps(in, out, n), "intensity map: out overlaps in (only in == out is allowed)");
  VH_REQUIRE(!overlaps(mask, out, n), "intensity map: out overlaps mask");
  return VISFD_HIP_OK;
}

// where the vector part starts (or n when the arrays' addresses disagree modulo 16)
i64 head_of(i64 n, const void* a, const void* b, const void* c) {
  const void* ptrs[3] = {a, b, c};
  int mis = -1;
  for (const void* p : ptrs) {
    if (!p) continue;
    const int m = (int)((reinterpret_cast<uintptr_t>(p) >> 2) & 3u);
    if (mis >= 0 && m != mis) return n;
    mis = m;
  }
  const i64 head = (4 - mis) & 3;
  return std::min(head, n);
}

int launch(visfd_hip_ctx* ctx, bool map, const float* in, float* out, const float* mask, i64 n,
           const visfd_hip_intensity* p, visfd_hip_stats* stats_out) {
  for (const void* q : {(const void*)in, (const void*)out, (const void*)mask})
    VH_REQUIRE((reinterpret_cast<uintptr_t>(q) & 3u) == 0, "image arrays must be 4-byte aligned");
  KernelArgs a;
  std::memset(&a, 0, sizeof(a));
  a.mask = mask;
  a.n = n;
  if (map) {
    a.p = *p;
    a.in = vh_intensity::reads_input(p->map) ? in : nullptr;
    a.out = out;
    a.load_out = vh_intensity::reads_output(*p) ? 1 : 0;
  } else {
    a.in = in;
  }
  a.head = head_of(n, a.in, a.out, a.mask);
  a.nvec = (n - a.head) / 4;
  StatsBins* bins = nullptr;
  if (stats_out) {
    VH_TRY(ws(ctx, WS_INTENSITY, 1, &bins));
    VH_HIP(hipMemsetAsync(bins, 0, sizeof(StatsBins), ctx->stream));
  }
  const i64 items = std::max(a.nvec, n - 4 * a.nvec);
  const i64 cap = ctx->opt.stats_blocks > 0 ? ctx->opt.stats_blocks : (i64)ctx->num_cus * 8;
  const unsigned grid = grid_for(items, BLOCK, cap);
  if (map && stats_out) intensity_kernel<true, true><<<grid, BLOCK, 0, ctx->stream>>>(a, bins);
  else if (map) intensity_kernel<true, false><<<grid, BLOCK, 0, ctx->stream>>>(a, bins);
  else intensity_kernel<false, true><<<grid, BLOCK, 0, ctx->stream>>>(a, bins);
  VH_HIP(hipGetLastError());
  if (stats_out) {
    StatsBins host;
    VH_HIP(hipMemcpyAsync(&host, bins, sizeof(StatsBins), hipMemcpyDeviceToHost, ctx->stream));
    VH_HIP(hipStreamSynchronize(ctx->stream));
    combine(host, stats_out);
  }
  return VISFD_HIP_OK;
}

}  // namespace
}  // namespace vh

using namespace vh;

extern "C" {

int visfd_hip_image_stats_host(const float* src, const float* mask, int64_t n, visfd_hip_stats* out) {
  VH_REQUIRE(src && out, "null argument");
  VH_REQUIRE(n >= 1, "image statistics: n must be positive");
  StatsBins b;
  std::memset(&b, 0, sizeof(b));
  for (int64_t i = 0; i < n; i++)
    if (!mask || mask[i] != 0.0f) host_tally(&b, src[i]);
  combine(b, out);
  return VISFD_HIP_OK;
}

int visfd_hip_image_stats_dev(visfd_hip_ctx* ctx, const float* src, const float* mask, int64_t n, visfd_hip_stats* out) {
  VH_REQUIRE(ctx && src && out, "null argument");
  VH_REQUIRE(n >= 1, "image statistics: n must be positive");
  VH_HIP(hipSetDevice(ctx->device));
  return launch(ctx, false, src, nullptr, mask, n, nullptr, out);
}

int visfd_hip_image_stats(visfd_hip_ctx* ctx, const float* src, const float* mask, int64_t n, visfd_hip_stats* out) {
  VH_REQUIRE(ctx && src && out, "null argument");
  VH_REQUIRE(n >= 1, "image statistics: n must be positive");
  VH_HIP(hipSetDevice(ctx->device));
  const Stage st = {ctx, (size_t)n};
  float *ds, *dm;
  VH_TRY(st.up(WS_H2D_0, src, &ds));
  VH_TRY(st.up(WS_H2D_1, mask, &dm));
  return visfd_hip_image_stats_dev(ctx, ds, dm, n, out);
}

int visfd_hip_intensity_map_host(const float* in, float* out, const float* mask, int64_t nx, int64_t ny, int64_t nz,
                                 const visfd_hip_intensity* p, visfd_hip_stats* stats_out) {
  VH_TRY(check_map(in, out, mask, nx, ny, nz, p));
  const int64_t n = nx * ny * nz;
  const bool rd = vh_intensity::reads_input(p->map);
  StatsBins b;
  std::memset(&b, 0, sizeof(b));
  for (int64_t i = 0; i < n; i++) {
    const bool in_mask = !mask || mask[i] != 0.0f;
    const float v = vh_intensity::apply(*p, rd ? in[i] : 0.0f, out[i], in_mask);
    out[i] = v;
    if (stats_out && (!p->stats_mask || in_mask)) host_tally(&b, v);
  }
  if (stats_out) combine(b, stats_out);
  return VISFD_HIP_OK;
}

int visfd_hip_intensity_map_dev(visfd_hip_ctx* ctx, const float* in, float* out, const float* mask, int64_t nx, int64_t ny,
                                int64_t nz, const visfd_hip_intensity* p, visfd_hip_stats* stats_out) {
  VH_REQUIRE(ctx, "null argument");
  VH_TRY(check_map(in, out, mask, nx, ny, nz, p));
  VH_HIP(hipSetDevice(ctx->device));
  return launch(ctx, true, in, out, mask, nx * ny * nz, p, stats_out);
}

int visfd_hip_intensity_map(visfd_hip_ctx* ctx, const float* in, float* out, const float* mask, int64_t nx, int64_t ny,
                            int64_t nz, const visfd_hip_intensity* p, visfd_hip_stats* stats_out) {
  VH_REQUIRE(ctx, "null argument");
  VH_TRY(check_map(in, out, mask, nx, ny, nz, p));
  VH_HIP(hipSetDevice(ctx->device));
  const Stage st = {ctx, (size_t)(nx * ny * nz)};
  const bool rd = vh_intensity::reads_input(p->map);
  float *di = nullptr, *dm = nullptr, *dout = nullptr;
  if (rd && in != out) VH_TRY(st.up(WS_H2D_0, in, &di));
  VH_TRY(st.up(WS_H2D_1, mask, &dm));
  // out goes up when a stage looks at it, and when it is also the threshold maps' input
  VH_TRY(st.out(WS_H2D_2, &dout, 1, (vh_intensity::reads_output(*p) || (rd && in == out)) ? out : nullptr));
  if (rd && in == out) di = dout;
  VH_TRY(launch(ctx, true, di, dout, dm, nx * ny * nz, p, stats_out));
  return st.down(out, dout);
}

}  // extern "C"
