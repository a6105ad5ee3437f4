// find_spheres.hip -- FindSpheres (lib/visfd/visfd_utils.hpp:271-359) without its table: for every query point the largest
// index among the spheres that contain it, plus one (0: none).  The contract is in include/visfd_hip.h.
//
// The reference paints every sphere of the list into an integer table spanning the queries' bounding box and reads the
// queries off it, so a later sphere overwrites an earlier one.  What a query reads is max{i + 1 : sphere i contains it},
// an integer max-reduction over (query, sphere) pairs: no table, no dependence on the image size, and -- an integer
// maximum does not depend on arrival order -- the same bits on every run (the argument of draw.hip's owner volume).
//
// Device work, all on the context's stream:
//   prep_queries_kernel   (int)crds, 16 bytes per query, padded to whole batches
//   prep_spheres_kernel   (centre, diameter) -> one 16-byte record (cx, cy, cz, Rsqr), padded to whole passes with records
//                         that contain no query.  Both raise bits of one flag word: a value the contract refuses, a sphere
//                         too large for the 32-bit sum of squares.
//   search_kernel         a workgroup takes one pass of FS_PASS records and one batch of FS_QB queries.  Every lane loads
//                         its records with 16-byte loads; the batch's queries are the same for the whole wave (scalar
//                         registers).  A pair costs 3 subtractions, 3 clamps, 3 24-bit multiply-adds, a compare and a
//                         select, all integer.  A lane meets its records in increasing index order, so the select keeps
//                         the maximum.  Waves that found nothing skip the reduction; otherwise the batch's maxima go across
//                         the wave by shuffles, across the workgroup through LDS, and the workgroup issues at most one
//                         integer atomicMax per query on the zero-initialised ids.
// A record carries one number for both tests of the reference, |q - c| <= R per axis and |q - c|^2 <= Rsqr.  With R >= 1
// (r = d/2 > 1/2) the second implies the first: (R + 1)^2 >= (r + 1/2)^2 = r^2 + r + 1/4 > ceil(r^2 - 1/2).  With R = 0
// (every d <= 1) the first admits the centre voxel only, while Rsqr = ceil(r^2 - 1/2) grows with |d| for negative d (d = -3:
// R = 0, Rsqr = 2): there the record's number is 0, not Rsqr.  tests/test_supervised.py sweeps both ranges.
#include <algorithm>
#include <cmath>
#include <limits>

#include "common.hpp"
#include "wave.hpp"

namespace vh {
namespace {

constexpr int FS_BLOCK = 256;                    // threads of a search workgroup (four waves)
constexpr int FS_WAVES = FS_BLOCK / WAVE;
constexpr int FS_UNROLL = 8;                     // records per lane
constexpr int FS_PASS = FS_BLOCK * FS_UNROLL;    // spheres per workgroup pass
constexpr int FS_QB = 16;                        // queries per batch
// The 32-bit sum: per-axis differences are clamped to +-FS_FAR, whose square exceeds every Rsqr the 32-bit kernel is given
// (those below FS_FAR^2) and three of whose squares fit a signed 32-bit word (3 * 26754^2 = 2147329548 < 2^31); FS_FAR < 2^23,
// so the products are signed 24-bit multiplies.  A list with a larger sphere (a diameter beyond 53 000 voxels) runs the
// 64-bit form.  A record whose Rsqr word is FS_NEVER contains nothing: -1 as the signed word the 32-bit form compares with.
constexpr int FS_FAR = 26754;
constexpr unsigned FS_NARROW_RSQR_END = (unsigned)FS_FAR * FS_FAR;
constexpr int FS_FAR_WIDE = 65536;               // its square exceeds every Rsqr there is (R <= 46340)
constexpr unsigned FS_NEVER = 0xFFFFFFFFu;
// q - c is formed in 32 bits and may wrap.  Queries are >= 0, so it wraps only where the true difference is 2^31 or more;
// with every centre >= FS_MIN_CENTRE the wrapped value lies within 65536 of -2^31, which is as far as the true one.  A
// sphere with a centre coordinate below FS_MIN_CENTRE holds no query (R <= 46340) and becomes a record that contains nothing.
constexpr int FS_MIN_CENTRE = -65536;
constexpr unsigned FS_FLAG_INVALID = 1u, FS_FLAG_WIDE = 2u;

// (int)x where the conversion is defined, the nearest int beyond
__host__ __device__ inline int trunc_sat(float x) {
  if (x >= 2147483648.0f) return 2147483647;
  if (x <= -2147483648.0f) return -2147483647 - 1;
  return (int)x;
}
__host__ __device__ inline bool finite_f(float x) { return x - x == 0.0f; }

// a query the contract accepts: finite, and its truncation is not negative
__host__ __device__ inline bool query_ok(float x) { return finite_f(x) && x > -1.0f; }

// visfd_utils.hpp:324-327.  diameter / 2 is a float; "- 0.5" promotes to double; SQR(x) is ((x)*(x)), a float product.
// Returns false for what the contract refuses (non-finite, R > VISFD_HIP_FIND_SPHERES_MAX_R); *rsqr then means nothing.
__host__ __device__ inline bool sphere_rsqr(float diameter, unsigned* rsqr) {
  *rsqr = 0;
  if (!finite_f(diameter)) return false;
  const float r = diameter / 2;
  const double R = ceil((double)r - 0.5);
  if (R > (double)VISFD_HIP_FIND_SPHERES_MAX_R) return false;
  // R <= 0 (every diameter up to 1, the negative ones included): the R test leaves the centre voxel alone, whatever
  // SQR(d/2) is -- it grows with |d| for negative d.  Only from R >= 1 on does Rsqr imply the R test (file header).
  if (R <= 0.0) return true;
  const float rr = r * r;
  const double Q = ceil((double)rr - 0.5);   // 0.5 < r <= 46340.5 here: between 0 and 46340.5^2 + 1, fits 32 bits
  *rsqr = Q > 0.0 ? (unsigned)Q : 0u;
  return true;
}

// the record of a sphere whose values have passed sphere_rsqr and finite_f
__host__ __device__ inline int4 make_record(float x, float y, float z, unsigned rsqr) {
  const int cx = trunc_sat(x), cy = trunc_sat(y), cz = trunc_sat(z);
  if (cx < FS_MIN_CENTRE || cy < FS_MIN_CENTRE || cz < FS_MIN_CENTRE) return make_int4(0, 0, 0, (int)FS_NEVER);
  return make_int4(cx, cy, cz, (int)rsqr);
}

__host__ __device__ inline int clamped_diff(int q, int c, int far) {
  const int d = (int)((unsigned)q - (unsigned)c);
  return d < -far ? -far : (d > far ? far : d);
}

// does the sphere of record r (centre, Rsqr) contain the query?
template <bool WIDE>
__host__ __device__ inline bool contains(int qx, int qy, int qz, const int4& r) {
  if (WIDE) {
    const long long dx = clamped_diff(qx, r.x, FS_FAR_WIDE), dy = clamped_diff(qy, r.y, FS_FAR_WIDE),
                    dz = clamped_diff(qz, r.z, FS_FAR_WIDE);
    return (unsigned)r.w != FS_NEVER && dx * dx + dy * dy + dz * dz <= (long long)(unsigned)r.w;
  }
  const int dx = clamped_diff(qx, r.x, FS_FAR), dy = clamped_diff(qy, r.y, FS_FAR), dz = clamped_diff(qz, r.z, FS_FAR);
#if defined(__HIP_DEVICE_COMPILE__)
  return __mul24(dx, dx) + __mul24(dy, dy) + __mul24(dz, dz) <= r.w;
#else
  return dx * dx + dy * dy + dz * dz <= r.w;
#endif
}

// ---- the two preparation launches ---------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void prep_queries_kernel(const float* __restrict__ crds, i64 n, i64 n_pad,
                                                           int4* __restrict__ out, unsigned* __restrict__ flags) {
  const i64 stride = (i64)gridDim.x * blockDim.x;
  for (i64 i = (i64)blockIdx.x * blockDim.x + threadIdx.x; i < n_pad; i += stride) {
    int4 q = make_int4(0, 0, 0, 0);   // padding: results of these are never written
    if (i < n) {
      const float x = crds[3 * i], y = crds[3 * i + 1], z = crds[3 * i + 2];
      if (!(query_ok(x) && query_ok(y) && query_ok(z))) atomicOr(flags, FS_FLAG_INVALID);
      q = make_int4(trunc_sat(x), trunc_sat(y), trunc_sat(z), 0);
    }
    out[i] = q;
  }
}

__global__ __launch_bounds__(256) void prep_spheres_kernel(const float* __restrict__ crds, const float* __restrict__ diameters,
                                                           i64 n, i64 n_pad, int4* __restrict__ out,
                                                           unsigned* __restrict__ flags) {
  const i64 stride = (i64)gridDim.x * blockDim.x;
  for (i64 i = (i64)blockIdx.x * blockDim.x + threadIdx.x; i < n_pad; i += stride) {
    int4 r = make_int4(0, 0, 0, (int)FS_NEVER);
    if (i < n) {
      const float x = crds[3 * i], y = crds[3 * i + 1], z = crds[3 * i + 2];
      unsigned rsqr;
      const bool ok = sphere_rsqr(diameters[i], &rsqr) && finite_f(x) && finite_f(y) && finite_f(z);
      if (!ok) atomicOr(flags, FS_FLAG_INVALID);
      else if (rsqr >= FS_NARROW_RSQR_END) atomicOr(flags, FS_FLAG_WIDE);
      r = make_record(x, y, z, rsqr);
    }
    out[i] = r;
  }
}

// ---- the search ---------------------------------------------------------------------------------------------------------
// grid (batches, passes): blockIdx.x is the query batch, so workgroups that run together read the same records.
// rec holds whole passes and qry whole batches (the preparation launches pad both), so the loops have no bounds tests.
template <bool WIDE>
__global__ __launch_bounds__(FS_BLOCK) void search_kernel(const int4* __restrict__ rec, const int4* __restrict__ qry,
                                                          i64 batch0, i64 pass0, i64 n_crds,
                                                          unsigned long long* __restrict__ ids) {
  __shared__ unsigned s_best[FS_WAVES][FS_QB];
  const i64 batch = batch0 + blockIdx.x, pass = pass0 + blockIdx.y;
  const int4* __restrict__ q = qry + batch * FS_QB;          // the same address in every lane
  const i64 first = pass * FS_PASS + threadIdx.x;             // below 2^31 + FS_PASS
  unsigned best[FS_QB];
#pragma unroll
  for (int j = 0; j < FS_QB; j++) best[j] = 0u;
#pragma unroll
  for (int u = 0; u < FS_UNROLL; u++) {
    const i64 i = first + (i64)u * FS_BLOCK;
    const int4 r = rec[i];
    const unsigned id = (unsigned)i + 1u;
#pragma unroll
    for (int j = 0; j < FS_QB; j++) {
      const int4 p = q[j];
      best[j] = contains<WIDE>(p.x, p.y, p.z, r) ? id : best[j];   // ids only grow along a lane's records
    }
  }
  unsigned any = 0u;
#pragma unroll
  for (int j = 0; j < FS_QB; j++) any |= best[j];
  const int lane = wave_lane(), wave = threadIdx.x / WAVE;
  if (__ballot(any != 0u) != 0ull) {   // the usual wave found nothing: it skips the shuffles (the whole wave does)
#pragma unroll
    for (int j = 0; j < FS_QB; j++) {
      unsigned v = best[j];
#pragma unroll
      for (int d = WAVE / 2; d >= 1; d >>= 1) {
        const unsigned o = (unsigned)__shfl_xor((int)v, d, WAVE);
        v = v > o ? v : o;
      }
      if (lane == 0) s_best[wave][j] = v;
    }
  } else if (lane < FS_QB) {
    s_best[wave][lane] = 0u;
  }
  __syncthreads();
  if (threadIdx.x < FS_QB) {
    unsigned m = 0u;
#pragma unroll
    for (int w = 0; w < FS_WAVES; w++) m = m > s_best[w][threadIdx.x] ? m : s_best[w][threadIdx.x];
    const i64 k = batch * FS_QB + threadIdx.x;
    if (m != 0u && k < n_crds) atomicMax(&ids[k], (unsigned long long)m);
  }
}

i64 round_up(i64 n, i64 m) { return (n + m - 1) / m * m; }

// what the host can say about the values: the flag bits the preparation launches would raise
unsigned host_flags(const float* crds, i64 n_crds, const float* sc, const float* sd, i64 n_spheres) {
  unsigned flags = 0u;
  for (i64 i = 0; i < 3 * n_crds; i++)
    if (!query_ok(crds[i])) return FS_FLAG_INVALID;
  for (i64 i = 0; i < n_spheres; i++) {
    unsigned rsqr;
    if (!(sphere_rsqr(sd[i], &rsqr) && finite_f(sc[3 * i]) && finite_f(sc[3 * i + 1]) && finite_f(sc[3 * i + 2])))
      return FS_FLAG_INVALID;
    if (rsqr >= FS_NARROW_RSQR_END) flags |= FS_FLAG_WIDE;
  }
  return flags;
}

int check_counts(const float* crds, i64 n_crds, const float* sc, const float* sd, i64 n_spheres, const int64_t* ids) {
  VH_REQUIRE(n_crds >= 0 && n_spheres >= 0, "find_spheres: negative count");
  VH_REQUIRE(n_spheres < ((i64)1 << 31), "find_spheres: 2^31 spheres or more");
  VH_REQUIRE(n_crds == 0 || (crds && ids), "find_spheres: null query or result array");
  VH_REQUIRE(n_spheres == 0 || (sc && sd), "find_spheres: null sphere array");
  return VISFD_HIP_OK;
}

int refuse_values() {
  return fail(VISFD_HIP_EINVAL,
              "find_spheres: a query with a negative or non-finite coordinate, a non-finite sphere, or a sphere radius "
              "beyond " + std::to_string(VISFD_HIP_FIND_SPHERES_MAX_R) + " voxels");
}

// the walk over the pairs on the host; the values have been checked
void host_walk(const float* crds, i64 n_crds, const float* sc, const float* sd, i64 n_spheres, int64_t* ids) {
  std::vector<int4> rec((size_t)n_spheres);
  for (i64 i = 0; i < n_spheres; i++) {
    unsigned rsqr;
    sphere_rsqr(sd[i], &rsqr);
    rec[(size_t)i] = make_record(sc[3 * i], sc[3 * i + 1], sc[3 * i + 2], rsqr);
  }
  for (i64 k = 0; k < n_crds; k++) {
    const int qx = trunc_sat(crds[3 * k]), qy = trunc_sat(crds[3 * k + 1]), qz = trunc_sat(crds[3 * k + 2]);
    i64 i = n_spheres - 1;
    while (i >= 0 && !contains<true>(qx, qy, qz, rec[(size_t)i])) i--;   // the last sphere that holds it
    ids[k] = i + 1;
  }
}

// Device arrays in, device ids out.  known_flags: what the host has found out about the values already (null: nobody
// has looked, the call waits for the flag word of the preparation launches).
int search_dev(visfd_hip_ctx* ctx, const float* crds, i64 n_crds, const float* sc, const float* sd, i64 n_spheres,
               int64_t* ids, const unsigned* known_flags) {
  const i64 nq_pad = round_up(n_crds, FS_QB), ns_pad = round_up(n_spheres, FS_PASS);
  int4 *qry = nullptr, *rec = nullptr;
  VH_TRY(ws(ctx, WS_FS_QUERIES, (size_t)nq_pad + 1, &qry));   // the last entry holds the flag word
  VH_TRY(ws(ctx, WS_FS_RECORDS, (size_t)ns_pad, &rec));
  unsigned* flags = reinterpret_cast<unsigned*>(qry + nq_pad);
  VH_HIP(hipMemsetAsync(flags, 0, sizeof(int4), ctx->stream));
  const i64 cap = (i64)ctx->num_cus * 16;
  prep_queries_kernel<<<grid_for(nq_pad, 256, cap), 256, 0, ctx->stream>>>(crds, n_crds, nq_pad, qry, flags);
  prep_spheres_kernel<<<grid_for(ns_pad, 256, cap), 256, 0, ctx->stream>>>(sc, sd, n_spheres, ns_pad, rec, flags);
  VH_HIP(hipGetLastError());
  unsigned f = 0u;
  if (known_flags) f = *known_flags;
  else {
    VH_HIP(hipMemcpyAsync(&f, flags, sizeof(unsigned), hipMemcpyDeviceToHost, ctx->stream));
    VH_HIP(hipStreamSynchronize(ctx->stream));
  }
  if (f & FS_FLAG_INVALID) return refuse_values();
  if (n_crds > 0) VH_HIP(hipMemsetAsync(ids, 0, sizeof(int64_t) * (size_t)n_crds, ctx->stream));
  const i64 n_batches = nq_pad / FS_QB, n_passes = ns_pad / FS_PASS;
  unsigned long long* out = reinterpret_cast<unsigned long long*>(ids);
  for (i64 p0 = 0; p0 < n_passes; p0 += 65535)
    for (i64 b0 = 0; b0 < n_batches; b0 += (i64)1 << 20) {
      const dim3 grid((unsigned)std::min<i64>(n_batches - b0, (i64)1 << 20), (unsigned)std::min<i64>(n_passes - p0, 65535));
      if (f & FS_FLAG_WIDE) search_kernel<true><<<grid, FS_BLOCK, 0, ctx->stream>>>(rec, qry, b0, p0, n_crds, out);
      else search_kernel<false><<<grid, FS_BLOCK, 0, ctx->stream>>>(rec, qry, b0, p0, n_crds, out);
    }
  VH_HIP(hipGetLastError());
  ctx->find_spheres_last_path = VISFD_HIP_FIND_SPHERES_PATH_DEVICE;
  return VISFD_HIP_OK;
}

}  // namespace
}  // namespace vh

using namespace vh;

extern "C" {

int visfd_hip_find_spheres_last_path(visfd_hip_ctx* ctx, int* path) {
  VH_REQUIRE(ctx && path, "null argument");
  *path = ctx->find_spheres_last_path;
  return VISFD_HIP_OK;
}

int visfd_hip_find_spheres_host(const float* crds, int64_t n_crds, const float* sphere_crds, const float* sphere_diameters,
                                int64_t n_spheres, int64_t* ids) {
  VH_TRY(check_counts(crds, n_crds, sphere_crds, sphere_diameters, n_spheres, ids));
  if (host_flags(crds, n_crds, sphere_crds, sphere_diameters, n_spheres) & FS_FLAG_INVALID) return refuse_values();
  host_walk(crds, n_crds, sphere_crds, sphere_diameters, n_spheres, ids);
  return VISFD_HIP_OK;
}

int visfd_hip_find_spheres(visfd_hip_ctx* ctx, const float* crds, int64_t n_crds, const float* sphere_crds,
                           const float* sphere_diameters, int64_t n_spheres, int64_t* ids) {
  VH_REQUIRE(ctx, "null context");
  VH_TRY(check_counts(crds, n_crds, sphere_crds, sphere_diameters, n_spheres, ids));
  const unsigned flags = host_flags(crds, n_crds, sphere_crds, sphere_diameters, n_spheres);
  if (flags & FS_FLAG_INVALID) return refuse_values();
  if (ctx->opt.find_spheres_host) {
    host_walk(crds, n_crds, sphere_crds, sphere_diameters, n_spheres, ids);
    ctx->find_spheres_last_path = VISFD_HIP_FIND_SPHERES_PATH_HOST;
    return VISFD_HIP_OK;
  }
  VH_HIP(hipSetDevice(ctx->device));
  if (n_crds == 0) {
    ctx->find_spheres_last_path = VISFD_HIP_FIND_SPHERES_PATH_DEVICE;
    return VISFD_HIP_OK;
  }
  const Stage sq = {ctx, (size_t)n_crds}, ss = {ctx, (size_t)n_spheres};
  float *dq, *dc = nullptr, *dd = nullptr, *di;
  VH_TRY(sq.up(WS_H2D_0, crds, &dq, 3));
  if (n_spheres > 0) {
    VH_TRY(ss.up(WS_H2D_1, sphere_crds, &dc, 3));
    VH_TRY(ss.up(WS_H2D_2, sphere_diameters, &dd));
  }
  VH_TRY(sq.out(WS_H2D_3, &di, 2));   // an int64 travels as the two 4-byte words it is
  VH_TRY(search_dev(ctx, dq, n_crds, dc, dd, n_spheres, reinterpret_cast<int64_t*>(di), &flags));
  return sq.down(reinterpret_cast<float*>(ids), di, 2);
}

int visfd_hip_find_spheres_dev(visfd_hip_ctx* ctx, const float* crds, int64_t n_crds, const float* sphere_crds,
                               const float* sphere_diameters, int64_t n_spheres, int64_t* ids) {
  VH_REQUIRE(ctx, "null context");
  VH_TRY(check_counts(crds, n_crds, sphere_crds, sphere_diameters, n_spheres, ids));
  VH_HIP(hipSetDevice(ctx->device));
  if (ctx->opt.find_spheres_host) {   // device arrays down, the walk, ids up: returns with the stream idle
    std::vector<float> q((size_t)(3 * n_crds)), c((size_t)(3 * n_spheres)), d((size_t)n_spheres);
    std::vector<int64_t> out((size_t)n_crds);
    if (n_crds > 0) VH_HIP(hipMemcpyAsync(q.data(), crds, sizeof(float) * q.size(), hipMemcpyDeviceToHost, ctx->stream));
    if (n_spheres > 0) {
      VH_HIP(hipMemcpyAsync(c.data(), sphere_crds, sizeof(float) * c.size(), hipMemcpyDeviceToHost, ctx->stream));
      VH_HIP(hipMemcpyAsync(d.data(), sphere_diameters, sizeof(float) * d.size(), hipMemcpyDeviceToHost, ctx->stream));
    }
    VH_HIP(hipStreamSynchronize(ctx->stream));
    if (host_flags(q.data(), n_crds, c.data(), d.data(), n_spheres) & FS_FLAG_INVALID) return refuse_values();
    host_walk(q.data(), n_crds, c.data(), d.data(), n_spheres, out.data());
    if (n_crds > 0) {
      VH_HIP(hipMemcpyAsync(ids, out.data(), sizeof(int64_t) * out.size(), hipMemcpyHostToDevice, ctx->stream));
      VH_HIP(hipStreamSynchronize(ctx->stream));
    }
    ctx->find_spheres_last_path = VISFD_HIP_FIND_SPHERES_PATH_HOST;
    return VISFD_HIP_OK;
  }
  return search_dev(ctx, crds, n_crds, sphere_crds, sphere_diameters, n_spheres, ids, nullptr);
}

}  // extern "C"
