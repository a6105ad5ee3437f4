// distance.hip -- exact squared Euclidean distance maps: the arithmetic of the reference's HandleDistanceToPoints and
// HandleDistancePointsToFeature (bin/filter_mrc/handlers_unsupported.cpp:1393-1550), which loop over every point for
// every voxel and over every voxel for every point.  The quantity is an integer,
//
//   dsq(v) = min(cap, min over seeds s of |v - s|^2),      cap = (nx + ny + nz)^2,
//
// so every result here is bit for bit, and the float outputs are sqrtf((float)dsq * (w * w)) with each step rounded to
// float.  Seeds are the selected voxels (image given, mask != 0, lo <= I <= hi: a NaN is never selected) and the listed
// integer points, which may lie anywhere.  nx + ny + nz <= 46340 keeps cap below 2^31 (the reference's int overflows
// beyond it).
//
// Integer ranges.  Two positions of the image are less than cap apart: (nx-1)^2 + (ny-1)^2 + (nz-1)^2 < (nx+ny+nz)^2.
// Hence a distance to a seed INSIDE the image is never clipped, the value cap in the volume means "no seed seen yet" and
// nothing else, and such voxels are skipped instead of entering a sum.  Every sum the passes form is (a - b)^2 + g with
// a, b positions on one axis and g a squared distance within the other axes: again less than cap < 2^31, so int32 holds
// it.  Axis lengths are below 2^16, so a stack entry packs its two positions into one word.
//
// The transform (option distance_general = 0), three passes in place over the int32 volume:
//  rows_kernel      along x, one wave per row: a forward sweep leaves the distance to the nearest seed at or left of x, a
//                   backward sweep takes the minimum with the one to the right and squares it.  The nearest seed within a
//                   chunk of 64 comes from the wave's ballot, the one beyond it from a carried position.
//  envelope_kernel  along y, then along z: D(i) = min_j g(j) + (i - j)^2 by the lower envelope of parabolas (Meijster,
//                   Roerdink, Hesselink 2000; Felzenszwalb, Huttenlocher 2012).  Lanes map to x, so the loads of g(x, j)
//                   for one j are 64 consecutive words; a wave owns 64 columns and a stack of (vertex, start, value) per
//                   column in workspace, laid out [entry][lane].  The z pass ends with the minimum over the listed points
//                   that lie outside the image (few; staged in LDS), which the separable passes cannot see.
// Listed points inside the image are scattered into the volume as zeros before the row pass.
//
// The general walk (distance_general = 1; also what listed points outside the image and query points outside the image
// cost): per voxel a loop over all listed points (points_min_kernel) and over all selected voxels (brute_voxels_kernel);
// per query point a reduction over all selected voxels (reduce_points_kernel: per wave a shuffle reduction, then one
// atomicMin per wave and point).
#include <algorithm>
#include <cmath>
#include <vector>

#include "common.hpp"
#include "wave.hpp"

namespace vh {

namespace {

constexpr int BLOCK = 256, WAVES = BLOCK / WAVE;
constexpr int LDS_POINTS = 256;     // listed points a block stages at a time
constexpr int REDUCE_POINTS = 16;   // query points of one reduction pass
constexpr int PREFETCH = 8;         // envelope passes: loads of g in flight per column
constexpr int NONE = 0x7fffffff;    // row pass: no seed on that side

__device__ __forceinline__ bool selected(const float* __restrict__ src, const float* __restrict__ mask, float lo, float hi,
                                         i64 i) {
  if (mask && mask[i] == 0.0f) return false;
  const float v = src[i];
  return v >= lo && v <= hi;
}

__global__ void __launch_bounds__(BLOCK) fill_kernel(int* __restrict__ dsq, i64 n, int value) {
  for (i64 i = (i64)blockIdx.x * BLOCK + threadIdx.x; i < n; i += (i64)gridDim.x * BLOCK) dsq[i] = value;
}

// pts: n points (x, y, z); those inside the image become zeros of the volume
__global__ void __launch_bounds__(BLOCK) scatter_kernel(int* __restrict__ dsq, const int* __restrict__ pts, i64 n, int nx,
                                                        int ny, int nz) {
  for (i64 k = (i64)blockIdx.x * BLOCK + threadIdx.x; k < n; k += (i64)gridDim.x * BLOCK) {
    const int x = pts[3 * k], y = pts[3 * k + 1], z = pts[3 * k + 2];
    if ((unsigned)x < (unsigned)nx && (unsigned)y < (unsigned)ny && (unsigned)z < (unsigned)nz)
      dsq[((i64)z * ny + y) * nx + x] = 0;
  }
}

// flags: the volume holds zeros at the scattered points (and ones elsewhere); src (nullable) adds the selected voxels
__global__ void __launch_bounds__(BLOCK)
rows_kernel(const float* __restrict__ src, const float* __restrict__ mask, float lo, float hi, int* __restrict__ dsq,
            int flags, int nx, i64 nrows, int cap) {
  const int lane = wave_lane();
  const i64 nwaves = (i64)gridDim.x * WAVES;
  const int last = ((nx - 1) / WAVE) * WAVE;
  for (i64 row = (i64)blockIdx.x * WAVES + (threadIdx.x >> 6); row < nrows; row += nwaves) {
    int* line = dsq + row * nx;
    const i64 base = row * nx;
    int carry = -1;   // x of the last seed of the chunks already swept
    for (int c0 = 0; c0 <= last; c0 += WAVE) {
      const int x = c0 + lane;
      bool seed = false;
      if (x < nx) {
        if (flags) seed = line[x] == 0;
        if (src && !seed) seed = selected(src, mask, lo, hi, base + x);
      }
      const unsigned long long b = __ballot(seed);
      const unsigned long long mine = b & ((2ull << lane) - 1ull);   // seeds at or left of this lane
      const int left = mine ? c0 + 63 - __clzll((long long)mine) : carry;
      if (x < nx) line[x] = left >= 0 ? x - left : NONE;
      if (b) carry = c0 + 63 - __clzll((long long)b);
    }
    carry = -1;
    for (int c0 = last; c0 >= 0; c0 -= WAVE) {
      const int x = c0 + lane;
      const int dl = x < nx ? line[x] : NONE;
      const unsigned long long b = __ballot(dl == 0);
      const unsigned long long mine = b & (~0ull << lane);           // seeds at or right of this lane
      const int right = mine ? c0 + wave_leader(mine) : carry;
      int d = dl;
      if (right >= 0) d = min(d, right - x);
      if (x < nx) line[x] = d == NONE ? cap : d * d;                 // d < 2^16
      if (b) carry = c0 + wave_leader(b);
    }
  }
}

// the squared distance from (x, y, z) to point p, in 64 bits: the host has dropped the points farther than cap from the
// image, so a coordinate difference is below 2^18
__device__ __forceinline__ i64 point_dsq(int x, int y, int z, const int* p) {
  const i64 dx = (i64)x - p[0], dy = (i64)y - p[1], dz = (i64)z - p[2];
  return dx * dx + dy * dy + dz * dz;
}

// One pass of the transform along an axis of m voxels, in place.  A unit of work is 64 columns: column `lane` of unit u
// starts at dsq[(u / xchunks) * outer_stride + (u % xchunks) * 64 + lane] and steps by `step`.  A wave's stack holds m
// entries of 64 lanes: {vertex | start << 16, value at the vertex}.
// FINAL (the z pass: u / xchunks is y, the position along the axis is z): the minimum with the first npts <= LDS_POINTS
// listed points outside the image.
// What a pass does with the value d of position `off` of the column that starts at col, a place inside dsq: StoreDsq
// writes it back.  An Out with ALWAYS visits the columns without a parabola too (d = cap everywhere).
struct StoreDsq {
  static constexpr bool ALWAYS = false;
  __device__ __forceinline__ void operator()(int* __restrict__ col, const int* dsq, i64 off, int d) const { col[off] = d; }
};
// The last pass of two-level morphology (csrc/morph_levels.hip): the float result instead of the distance, which is
// not stored.  The arithmetic is morph_store's (csrc/morph.hip).
struct StoreLevels {
  static constexpr bool ALWAYS = true;
  LevelsEpilogue e;
  __device__ __forceinline__ void operator()(int* __restrict__ col, const int* dsq, i64 off, int d) const {
    const i64 i = (col - dsq) + off;
    if (e.mask && e.mask[i] == 0.0f) {
      if (e.nan_masked) e.dst[i] = NAN;
      return;
    }
    const float cur = __uint_as_float(d <= e.t ? e.near_bits : e.far_bits);
    float v = cur;
    if (e.epi == 1)
      v = e.dst[i] - cur;
    else if (e.epi == 2)
      v = cur - e.dst[i];
    e.dst[i] = v;
  }
};

template <bool FINAL, class Out>
__device__ __forceinline__ void envelope_pass(int* __restrict__ dsq, int2* __restrict__ stack, int m, i64 step,
                                              i64 outer_stride, int nx, i64 nunits, int xchunks, int cap,
                                              const int* spts, int npts, const Out& out) {
  const int lane = wave_lane();
  const i64 wave = (i64)blockIdx.x * WAVES + (threadIdx.x >> 6);
  const i64 nwaves = (i64)gridDim.x * WAVES;
  int2* st = stack + wave * m * WAVE + lane;   // entry q of this column: st[q * WAVE]
  for (i64 unit = wave; unit < nunits; unit += nwaves) {
    const i64 outer = unit / xchunks;
    const int x = (int)(unit % xchunks) * WAVE + lane;
    if (x >= nx) continue;
    int* col = dsq + outer * outer_stride + x;
    // the top of the stack in registers: vertex ts, first position tt where it is the minimum, value tg at the vertex
    int q = -1, ts = 0, tt = 0, tg = 0;
    for (int u0 = 0; u0 < m; u0 += PREFETCH) {
      int gb[PREFETCH];   // the loads do not depend on the stack: PREFETCH of them in flight per column
#pragma unroll
      for (int k = 0; k < PREFETCH; k++) gb[k] = u0 + k < m ? col[(i64)(u0 + k) * step] : cap;
#pragma unroll
      for (int k = 0; k < PREFETCH; k++) {
      const int u = u0 + k, gu = gb[k];
      if (gu == cap) continue;   // no seed in this voxel's lower-dimensional slice (or past the end): not a parabola
      // pops: at most one per earlier push, and q never goes below -1
      while (q >= 0) {
        const int a = tt - ts, b = tt - u;
        if (a * a + tg <= b * b + gu) break;   // the top still wins where it starts
        q--;
        if (q >= 0) {
          const int2 e = st[(i64)q * WAVE];
          ts = e.x & 0xffff;
          tt = (int)((unsigned)e.x >> 16);
          tg = e.y;
        }
      }
      if (q < 0) {
        q = 0;
        ts = u; tt = 0; tg = gu;
        st[0] = make_int2(u, gu);
      } else {
        // the last position where the top is at least as good as u: floor(((u^2 + gu) - (ts^2 + tg)) / (2 (u - ts))).
        // Both terms are below cap < 2^31 and, the top winning at tt >= 0, the numerator is not negative: a 32-bit
        // truncating division is the floor.
        const int num = (u * u + gu) - (ts * ts + tg);
        const int w = 1 + (int)((unsigned)num / (unsigned)(2 * (u - ts)));
        if (w < m) {   // w > tt: starts grow along the stack, and q <= u < m
          q++;
          ts = u; tt = w; tg = gu;
          st[(i64)q * WAVE] = make_int2(u | (w << 16), gu);
        }
      }
      }
    }
    if (q < 0 && !(FINAL && npts > 0) && !Out::ALWAYS) continue;   // the column holds cap everywhere already
    for (int u = m - 1; u >= 0; u--) {
      int d = cap;
      if (q >= 0) {
        const int a = u - ts;
        d = a * a + tg;
      }
      if (FINAL) {
        i64 best = d;
        for (int k = 0; k < npts; k++) best = min(best, point_dsq(x, (int)outer, u, spts + 3 * k));
        d = (int)best;
      }
      out(col, dsq, (i64)u * step, d);
      if (q > 0 && u == tt) {
        q--;
        const int2 e = st[(i64)q * WAVE];
        ts = e.x & 0xffff;
        tt = (int)((unsigned)e.x >> 16);
        tg = e.y;
      }
    }
  }
}

template <bool FINAL>
__global__ void __launch_bounds__(BLOCK)
envelope_kernel(int* __restrict__ dsq, int2* __restrict__ stack, int m, i64 step, i64 outer_stride, int nx, i64 nunits,
                int xchunks, int cap, const int* __restrict__ pts, int npts) {
  __shared__ int spts[3 * LDS_POINTS];
  if (FINAL) {
    for (int k = threadIdx.x; k < 3 * npts; k += BLOCK) spts[k] = pts[k];
    __syncthreads();
  }
  envelope_pass<FINAL>(dsq, stack, m, step, outer_stride, nx, nunits, xchunks, cap, spts, npts, StoreDsq());
}

// the z pass of dev_distance_levels: no listed points, and the epilogue instead of the store
__global__ void __launch_bounds__(BLOCK)
envelope_levels_kernel(int* __restrict__ dsq, int2* __restrict__ stack, int m, i64 step, i64 outer_stride, int nx,
                       i64 nunits, int xchunks, int cap, StoreLevels out) {
  envelope_pass<false>(dsq, stack, m, step, outer_stride, nx, nunits, xchunks, cap, nullptr, 0, out);
}

// dsq = min(dsq, distance to the nearest of n listed points), a block staging LDS_POINTS of them at a time
__global__ void __launch_bounds__(BLOCK)
points_min_kernel(int* __restrict__ dsq, const int* __restrict__ pts, i64 n, int nx, int ny, int nz) {
  __shared__ int spts[3 * LDS_POINTS];
  const int x = blockIdx.x * BLOCK + threadIdx.x;
  const i64 nrows = (i64)ny * nz;
  for (i64 row = blockIdx.y; row < nrows; row += gridDim.y) {
    const int y = (int)(row % ny), z = (int)(row / ny);
    i64 best = x < nx ? dsq[row * nx + x] : 0;
    for (i64 k0 = 0; k0 < n; k0 += LDS_POINTS) {
      const int cnt = (int)min((i64)LDS_POINTS, n - k0);
      __syncthreads();
      for (int k = threadIdx.x; k < 3 * cnt; k += BLOCK) spts[k] = pts[3 * k0 + k];
      __syncthreads();
      for (int k = 0; k < cnt; k++) best = min(best, point_dsq(x, y, z, spts + 3 * k));
    }
    if (x < nx) dsq[row * nx + x] = (int)best;
  }
}

// dsq = min(dsq, distance to the nearest selected voxel): every voxel against every voxel (uniform loads of the image)
__global__ void __launch_bounds__(BLOCK)
brute_voxels_kernel(const float* __restrict__ src, const float* __restrict__ mask, float lo, float hi,
                    int* __restrict__ dsq, int nx, int ny, int nz) {
  const int x = blockIdx.x * BLOCK + threadIdx.x;
  const i64 nrows = (i64)ny * nz;
  for (i64 row = blockIdx.y; row < nrows; row += gridDim.y) {
    if (x >= nx) continue;
    const int y = (int)(row % ny), z = (int)(row / ny);
    int best = dsq[row * nx + x];
    for (int uz = 0; uz < nz; uz++)
      for (int uy = 0; uy < ny; uy++) {
        const int dyz = (y - uy) * (y - uy) + (z - uz) * (z - uz);
        const i64 base = ((i64)uz * ny + uy) * nx;
        for (int ux = 0; ux < nx; ux++)
          if (selected(src, mask, lo, hi, base + ux)) best = min(best, (x - ux) * (x - ux) + dyz);
      }
    dsq[row * nx + x] = best;
  }
}

// res[q[4 k + 3]] = dsq at query point k (x, y, z, slot), which lies inside the image
__global__ void __launch_bounds__(BLOCK) gather_kernel(const int* __restrict__ dsq, const int* __restrict__ q, i64 n,
                                                       int nx, int ny, int* __restrict__ res) {
  for (i64 k = (i64)blockIdx.x * BLOCK + threadIdx.x; k < n; k += (i64)gridDim.x * BLOCK)
    res[q[4 * k + 3]] = dsq[((i64)q[4 * k + 2] * ny + q[4 * k + 1]) * nx + q[4 * k]];
}

// res[slot] = min(res[slot], distance from query point k to the nearest selected voxel) for the cnt <= REDUCE_POINTS
// query points (x, y, z, slot) at q
__global__ void __launch_bounds__(BLOCK)
reduce_points_kernel(const float* __restrict__ src, const float* __restrict__ mask, float lo, float hi, int nx, int ny,
                     int nz, const int* __restrict__ q, int cnt, int cap, int* __restrict__ res) {
  i64 best[REDUCE_POINTS];
#pragma unroll
  for (int k = 0; k < REDUCE_POINTS; k++) best[k] = cap;
  const i64 nrows = (i64)ny * nz;
  for (i64 row = blockIdx.x; row < nrows; row += gridDim.x) {
    const int y = (int)(row % ny), z = (int)(row / ny);
    for (int x = threadIdx.x; x < nx; x += BLOCK) {
      if (!selected(src, mask, lo, hi, row * nx + x)) continue;
#pragma unroll
      for (int k = 0; k < REDUCE_POINTS; k++)
        if (k < cnt) best[k] = min(best[k], point_dsq(x, y, z, q + 4 * k));
    }
  }
#pragma unroll
  for (int k = 0; k < REDUCE_POINTS; k++) {
    int v = (int)best[k];   // at most cap
    for (int off = WAVE / 2; off > 0; off >>= 1) v = min(v, __shfl_xor(v, off, WAVE));
    if (k < cnt && wave_lane() == 0 && v < cap) atomicMin(&res[q[4 * k + 3]], v);
  }
}

// dst = sqrtf((float)dsq * ww) where mask != 0: the reference's `sqrt(rminsq_int * SQR(voxel_width_))`, each step in float
__global__ void __launch_bounds__(BLOCK) root_kernel(const int* __restrict__ dsq, float* __restrict__ dst,
                                                     const float* __restrict__ mask, i64 n, float ww) {
  for (i64 i = (i64)blockIdx.x * BLOCK + threadIdx.x; i < n; i += (i64)gridDim.x * BLOCK) {
    if (mask && mask[i] == 0.0f) continue;
    dst[i] = sqrtf((float)dsq[i] * ww);   // correctly rounded (hipcc default -fhip-fp32-correctly-rounded-divide-sqrt; __fsqrt_rn is not)
  }
}

// a point farther than cap from every voxel changes nothing; the others lie within 46340 voxels of the image
bool within_cap(const int* p, i64 nx, i64 ny, i64 nz, i64 cap) {
  const i64 n[3] = {nx, ny, nz};
  i64 sum = 0;
  for (int d = 0; d < 3; d++) {
    i64 e = 0;
    if (p[d] < 0) e = -(i64)p[d];
    else if (p[d] >= n[d]) e = (i64)p[d] - (n[d] - 1);
    e = std::min<i64>(e, 46341);
    sum += e * e;
  }
  return sum < cap;
}
bool inside(const int* p, i64 nx, i64 ny, i64 nz) {
  return p[0] >= 0 && p[0] < nx && p[1] >= 0 && p[1] < ny && p[2] >= 0 && p[2] < nz;
}

unsigned rows_grid(i64 nrows) { return (unsigned)std::min<i64>(nrows, 65535); }

int check_common(visfd_hip_ctx* ctx, i64 nx, i64 ny, i64 nz, const int32_t* points, i64 npoints) {
  VH_REQUIRE(ctx, "null argument");
  VH_TRY(check_dims(nx, ny, nz));
  VH_REQUIRE(nx + ny + nz <= VISFD_HIP_DISTANCE_MAX_DIM_SUM, "distance: nx + ny + nz must be at most 46340");
  VH_REQUIRE(npoints >= 0, "distance: the number of points must not be negative");
  VH_REQUIRE(points || npoints == 0, "distance: null point list");
  return VISFD_HIP_OK;
}

// `host` to `dev`, a place inside slot WS_DIST_POINTS that the caller has reserved; returns once the copy has left the vector
int put_ints(visfd_hip_ctx* ctx, int* dev, const std::vector<int>& host) {
  if (host.empty()) return VISFD_HIP_OK;
  VH_HIP(hipMemcpyAsync(dev, host.data(), sizeof(int) * host.size(), hipMemcpyHostToDevice, ctx->stream));
  VH_HIP(hipStreamSynchronize(ctx->stream));
  return VISFD_HIP_OK;
}

}  // namespace

int dev_distance_sq(visfd_hip_ctx* ctx, const float* src, const float* mask, i64 nx, i64 ny, i64 nz, float lo, float hi,
                    const int32_t* points, i64 npoints, int32_t* dsq) {
  VH_TRY(check_common(ctx, nx, ny, nz, points, npoints));
  VH_REQUIRE(dsq, "null argument");
  const i64 n = nx * ny * nz, S = nx + ny + nz;
  const int cap = (int)(S * S);
  const bool general = ctx->opt.distance_general != 0;
  // the listed points that can matter, those inside the image first
  std::vector<int> in, out;
  in.reserve((size_t)(3 * npoints));
  for (i64 k = 0; k < npoints; k++) {
    const int* p = points + 3 * k;
    if (inside(p, nx, ny, nz)) in.insert(in.end(), p, p + 3);
    else if (within_cap(p, nx, ny, nz, cap)) out.insert(out.end(), p, p + 3);
  }
  const i64 n_in = (i64)in.size() / 3, n_out = (i64)out.size() / 3;
  in.insert(in.end(), out.begin(), out.end());
  int* dpts = nullptr;
  VH_TRY(ws(ctx, WS_DIST_POINTS, in.size(), &dpts));
  VH_TRY(put_ints(ctx, dpts, in));
  const unsigned flat_grid = grid_for(n, BLOCK, (i64)ctx->num_cus * 16);
  const dim3 row_grid((unsigned)((nx + BLOCK - 1) / BLOCK), rows_grid(ny * nz));
  if (general) {
    fill_kernel<<<flat_grid, BLOCK, 0, ctx->stream>>>(dsq, n, cap);
    if (n_in + n_out > 0)
      points_min_kernel<<<row_grid, BLOCK, 0, ctx->stream>>>(dsq, dpts, n_in + n_out, (int)nx, (int)ny, (int)nz);
    if (src) brute_voxels_kernel<<<row_grid, BLOCK, 0, ctx->stream>>>(src, mask, lo, hi, dsq, (int)nx, (int)ny, (int)nz);
    VH_HIP(hipGetLastError());
    ctx->distance_last_path = VISFD_HIP_DISTANCE_PATH_GENERAL;
    return VISFD_HIP_OK;
  }
  if (n_in > 0) {
    fill_kernel<<<flat_grid, BLOCK, 0, ctx->stream>>>(dsq, n, 1);
    scatter_kernel<<<grid_for(n_in, BLOCK, (i64)ctx->num_cus * 16), BLOCK, 0, ctx->stream>>>(dsq, dpts, n_in, (int)nx, (int)ny,
                                                                                             (int)nz);
  }
  const i64 max_waves = (i64)ctx->num_cus * 16;   // four waves per SIMD
  const i64 nrows = ny * nz;
  rows_kernel<<<(unsigned)((std::min(nrows, max_waves) + WAVES - 1) / WAVES), BLOCK, 0, ctx->stream>>>(
      src, mask, lo, hi, dsq, n_in > 0 ? 1 : 0, (int)nx, nrows, cap);
  const int xchunks = (int)((nx + WAVE - 1) / WAVE);
  const i64 units_y = nz * xchunks, units_z = ny * xchunks;
  const i64 waves_y = std::min(units_y, max_waves), waves_z = std::min(units_z, max_waves);
  int2* stack = nullptr;
  VH_TRY(ws(ctx, WS_DIST_STACK, (size_t)std::max(waves_y * ny, waves_z * nz) * WAVE, &stack));
  const int first_out = (int)std::min<i64>(n_out, LDS_POINTS);
  envelope_kernel<false><<<(unsigned)((waves_y + WAVES - 1) / WAVES), BLOCK, 0, ctx->stream>>>(
      dsq, stack, (int)ny, nx, nx * ny, (int)nx, units_y, xchunks, cap, nullptr, 0);
  envelope_kernel<true><<<(unsigned)((waves_z + WAVES - 1) / WAVES), BLOCK, 0, ctx->stream>>>(
      dsq, stack, (int)nz, nx * ny, nx, (int)nx, units_z, xchunks, cap, dpts + 3 * n_in, first_out);
  if (n_out > first_out)
    points_min_kernel<<<row_grid, BLOCK, 0, ctx->stream>>>(dsq, dpts + 3 * (n_in + first_out), n_out - first_out, (int)nx,
                                                           (int)ny, (int)nz);
  VH_HIP(hipGetLastError());
  ctx->distance_last_path = VISFD_HIP_DISTANCE_PATH_TRANSFORM;
  return VISFD_HIP_OK;
}

int dev_distance_levels(visfd_hip_ctx* ctx, const float* src, const float* mask, i64 nx, i64 ny, i64 nz, float level,
                        int32_t* dsq, const LevelsEpilogue& e) {
  VH_TRY(check_common(ctx, nx, ny, nz, nullptr, 0));
  VH_REQUIRE(src && dsq && e.dst, "null argument");
  const i64 S = nx + ny + nz;
  const int cap = (int)(S * S);
  const i64 max_waves = (i64)ctx->num_cus * 16, nrows = ny * nz;
  rows_kernel<<<(unsigned)((std::min(nrows, max_waves) + WAVES - 1) / WAVES), BLOCK, 0, ctx->stream>>>(
      src, mask, level, level, dsq, 0, (int)nx, nrows, cap);
  const int xchunks = (int)((nx + WAVE - 1) / WAVE);
  const i64 units_y = nz * xchunks, units_z = ny * xchunks;
  const i64 waves_y = std::min(units_y, max_waves), waves_z = std::min(units_z, max_waves);
  int2* stack = nullptr;
  VH_TRY(ws(ctx, WS_DIST_STACK, (size_t)std::max(waves_y * ny, waves_z * nz) * WAVE, &stack));
  envelope_kernel<false><<<(unsigned)((waves_y + WAVES - 1) / WAVES), BLOCK, 0, ctx->stream>>>(
      dsq, stack, (int)ny, nx, nx * ny, (int)nx, units_y, xchunks, cap, nullptr, 0);
  StoreLevels out;
  out.e = e;
  envelope_levels_kernel<<<(unsigned)((waves_z + WAVES - 1) / WAVES), BLOCK, 0, ctx->stream>>>(
      dsq, stack, (int)nz, nx * ny, nx, (int)nx, units_z, xchunks, cap, out);
  VH_HIP(hipGetLastError());
  return VISFD_HIP_OK;
}

namespace {

int to_points_dev(visfd_hip_ctx* ctx, float* dst, const float* mask, i64 nx, i64 ny, i64 nz, const int32_t* points,
                  i64 npoints, float voxel_width) {
  int* dsq = nullptr;
  VH_TRY(ws(ctx, WS_DIST_DSQ, (size_t)(nx * ny * nz), &dsq));
  VH_TRY(dev_distance_sq(ctx, nullptr, nullptr, nx, ny, nz, 0.0f, 0.0f, points, npoints, dsq));
  const i64 n = nx * ny * nz;
  root_kernel<<<grid_for(n, BLOCK, (i64)ctx->num_cus * 16), BLOCK, 0, ctx->stream>>>(dsq, dst, mask, n,
                                                                                     voxel_width * voxel_width);
  VH_HIP(hipGetLastError());
  return VISFD_HIP_OK;
}

int from_points_dev(visfd_hip_ctx* ctx, const float* src, const float* mask, i64 nx, i64 ny, i64 nz, float lo, float hi,
                    const int32_t* points, i64 npoints, float voxel_width, float* out) {
  const i64 S = nx + ny + nz;
  const int cap = (int)(S * S);
  const bool general = ctx->opt.distance_general != 0;
  // query points (x, y, z, slot): those read from the transform, then those reduced over the selected voxels
  std::vector<int> look, walk;
  for (i64 k = 0; k < npoints; k++) {
    const int* p = points + 3 * k;
    std::vector<int>* list = nullptr;
    if (!general && inside(p, nx, ny, nz)) list = &look;
    else if (within_cap(p, nx, ny, nz, cap)) list = &walk;
    if (!list) continue;   // farther than cap from every voxel: cap
    list->insert(list->end(), p, p + 3);
    list->push_back((int)k);
  }
  const i64 n_look = (i64)look.size() / 4, n_walk = (i64)walk.size() / 4;
  std::vector<int> res((size_t)npoints, cap);
  if (npoints > 0) {
    int* dsq = nullptr;
    if (n_look > 0) {
      VH_TRY(ws(ctx, WS_DIST_DSQ, (size_t)(nx * ny * nz), &dsq));
      VH_TRY(dev_distance_sq(ctx, src, mask, nx, ny, nz, lo, hi, nullptr, 0, dsq));   // takes WS_DIST_POINTS first
    }
    look.insert(look.end(), walk.begin(), walk.end());
    int* dq = nullptr;
    VH_TRY(ws(ctx, WS_DIST_POINTS, look.size() + (size_t)npoints, &dq));
    int* dres = dq + look.size();
    VH_TRY(put_ints(ctx, dq, look));
    VH_TRY(put_ints(ctx, dres, res));
    if (n_look > 0)
      gather_kernel<<<grid_for(n_look, BLOCK, (i64)ctx->num_cus * 16), BLOCK, 0, ctx->stream>>>(dsq, dq, n_look, (int)nx,
                                                                                                (int)ny, dres);
    const unsigned grid = (unsigned)std::min<i64>(ny * nz, (i64)ctx->num_cus * 8);
    for (i64 k0 = 0; k0 < n_walk; k0 += REDUCE_POINTS)
      reduce_points_kernel<<<grid, BLOCK, 0, ctx->stream>>>(src, mask, lo, hi, (int)nx, (int)ny, (int)nz,
                                                            dq + 4 * (n_look + k0),
                                                            (int)std::min<i64>(REDUCE_POINTS, n_walk - k0), cap, dres);
    VH_HIP(hipGetLastError());
    VH_HIP(hipMemcpyAsync(res.data(), dres, sizeof(int) * res.size(), hipMemcpyDeviceToHost, ctx->stream));
  }
  ctx->distance_last_path = general ? VISFD_HIP_DISTANCE_PATH_GENERAL : VISFD_HIP_DISTANCE_PATH_TRANSFORM;
  VH_HIP(hipStreamSynchronize(ctx->stream));
  const float ww = voxel_width * voxel_width;
  for (i64 k = 0; k < npoints; k++) out[k] = std::sqrt((float)res[(size_t)k] * ww);
  return VISFD_HIP_OK;
}

int check_to_points(visfd_hip_ctx* ctx, const float* dst, const float* mask, i64 nx, i64 ny, i64 nz,
                    const int32_t* points, i64 npoints) {
  VH_TRY(check_common(ctx, nx, ny, nz, points, npoints));
  VH_REQUIRE(dst, "null argument");
  VH_REQUIRE(!overlap_bytes(dst, sizeof(float) * (size_t)(nx * ny * nz), mask, sizeof(float) * (size_t)(nx * ny * nz)),
             "distance: dst overlaps mask");
  return VISFD_HIP_OK;
}

int check_from_points(visfd_hip_ctx* ctx, const float* src, i64 nx, i64 ny, i64 nz, const int32_t* points, i64 npoints,
                      const float* out) {
  VH_TRY(check_common(ctx, nx, ny, nz, points, npoints));
  VH_REQUIRE(src, "null argument");
  VH_REQUIRE(out || npoints == 0, "null argument");
  return VISFD_HIP_OK;
}

}  // namespace
}  // namespace vh

using namespace vh;

extern "C" {

int visfd_hip_distance_last_path(visfd_hip_ctx* ctx, int* path) {
  VH_REQUIRE(ctx && path, "null argument");
  *path = ctx->distance_last_path;
  return VISFD_HIP_OK;
}

int visfd_hip_distance_sq_dev(visfd_hip_ctx* ctx, const float* src, const float* mask, int64_t nx, int64_t ny, int64_t nz,
                              float lo, float hi, const int32_t* points, int64_t npoints, int32_t* dsq) {
  VH_TRY(check_common(ctx, nx, ny, nz, points, npoints));
  VH_REQUIRE(dsq, "null argument");
  VH_HIP(hipSetDevice(ctx->device));
  return dev_distance_sq(ctx, src, mask, nx, ny, nz, lo, hi, points, npoints, dsq);
}

int visfd_hip_distance_sq(visfd_hip_ctx* ctx, const float* src, const float* mask, int64_t nx, int64_t ny, int64_t nz,
                          float lo, float hi, const int32_t* points, int64_t npoints, int32_t* dsq) {
  VH_TRY(check_common(ctx, nx, ny, nz, points, npoints));
  VH_REQUIRE(dsq, "null argument");
  VH_HIP(hipSetDevice(ctx->device));
  const Stage st = {ctx, (size_t)(nx * ny * nz)};
  float *ds, *dm, *dd;   // the int32 volume travels as the 4-byte words it is
  VH_TRY(st.up(WS_H2D_0, src, &ds));
  VH_TRY(st.up(WS_H2D_1, src ? mask : nullptr, &dm));
  VH_TRY(st.out(WS_H2D_2, &dd));
  VH_TRY(dev_distance_sq(ctx, ds, dm, nx, ny, nz, lo, hi, points, npoints, reinterpret_cast<int32_t*>(dd)));
  return st.down(reinterpret_cast<float*>(dsq), dd);
}

int visfd_hip_distance_to_points_dev(visfd_hip_ctx* ctx, float* dst, const float* mask, int64_t nx, int64_t ny, int64_t nz,
                                     const int32_t* points, int64_t npoints, float voxel_width) {
  VH_TRY(check_to_points(ctx, dst, mask, nx, ny, nz, points, npoints));
  VH_HIP(hipSetDevice(ctx->device));
  return to_points_dev(ctx, dst, mask, nx, ny, nz, points, npoints, voxel_width);
}

int visfd_hip_distance_to_points(visfd_hip_ctx* ctx, float* dst, const float* mask, int64_t nx, int64_t ny, int64_t nz,
                                 const int32_t* points, int64_t npoints, float voxel_width) {
  VH_TRY(check_to_points(ctx, dst, mask, nx, ny, nz, points, npoints));
  VH_HIP(hipSetDevice(ctx->device));
  const Stage st = {ctx, (size_t)(nx * ny * nz)};
  float *dm, *dd;
  VH_TRY(st.up(WS_H2D_1, mask, &dm));
  VH_TRY(st.out(WS_H2D_2, &dd, 1, mask ? dst : nullptr));   // with a mask some voxels keep the caller's values
  VH_TRY(to_points_dev(ctx, dd, dm, nx, ny, nz, points, npoints, voxel_width));
  return st.down(dst, dd);
}

int visfd_hip_distance_from_points_dev(visfd_hip_ctx* ctx, const float* src, const float* mask, int64_t nx, int64_t ny,
                                       int64_t nz, float lo, float hi, const int32_t* points, int64_t npoints,
                                       float voxel_width, float* out) {
  VH_TRY(check_from_points(ctx, src, nx, ny, nz, points, npoints, out));
  VH_HIP(hipSetDevice(ctx->device));
  return from_points_dev(ctx, src, mask, nx, ny, nz, lo, hi, points, npoints, voxel_width, out);
}

int visfd_hip_distance_from_points(visfd_hip_ctx* ctx, const float* src, const float* mask, int64_t nx, int64_t ny,
                                   int64_t nz, float lo, float hi, const int32_t* points, int64_t npoints,
                                   float voxel_width, float* out) {
  VH_TRY(check_from_points(ctx, src, nx, ny, nz, points, npoints, out));
  VH_HIP(hipSetDevice(ctx->device));
  const Stage st = {ctx, (size_t)(nx * ny * nz)};
  float *ds, *dm;
  VH_TRY(st.up(WS_H2D_0, src, &ds));
  VH_TRY(st.up(WS_H2D_1, mask, &dm));
  return from_points_dev(ctx, ds, dm, nx, ny, nz, lo, hi, points, npoints, voxel_width, out);
}

}  // extern "C"
