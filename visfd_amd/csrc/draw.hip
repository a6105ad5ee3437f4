// draw.hip -- DrawSpheres and DrawRegions (reference lib/visfd/draw.hpp:90-457) and their entry points.
//
// DrawSpheres.  In the reference every sphere overwrites what earlier ones wrote, so a voxel ends with the value of the
// LAST sphere in list order whose shell holds it, or with the background expression.  Here:
//   1. an owner volume (one uint32 per voxel, slot WS_DRAW_OWNER) is zeroed;
//   2. scatter_kernel<false>: the rows (z, y) of each sphere's bounding box CLIPPED to the image are dealt to waves, lanes
//      along x; a voxel of the shell takes atomicMax(owner, i + 1).  A maximum does not depend on arrival order;
//   3. (foreground_normalize only) scatter_kernel<true> counts each sphere's in-image, unmasked shell voxels and
//      value_kernel turns them into fg[i] * (float)(1.0 / n_i);
//   4. resolve_kernel, the one pass over the volume: owner 0 or mask == 0 gives the background expression (two float
//      roundings: multiply, then add the offset), anything else the owner's value.  It reads and writes the same index, so
//      dst may be the background array.
// The mask is not part of a sphere's geometry: it is looked at in the resolve (and the count) only.
// What stays on the host: the float statistics of background_normalize (AverageArr / StdDevArr accumulate in float in raster
// order, visfd_utils.hpp:685-790 -- no parallel sum gives those bits) and the per-list double loops (draw.hpp:298-311).
//
// DrawRegions is not a hot path (masks have a handful of regions): one stream-ordered launch per region over its clipped
// box gives the reference's sequential meaning.
#include <cmath>
#include <vector>

#include "common.hpp"
#include "wave.hpp"

namespace vh {

namespace {

constexpr int BLOCK = 256;
constexpr int MAX_RS = 26754;   // 3 * Rs^2 < 2^31: beyond it the reference's `int rsqr` overflows (draw.hpp:411, :424)

struct SphereRec {
  int cx, cy, cz;      // centre (draw.hpp:365-367)
  int x0, x1;          // clipped box: x0..x1, ny_rows rows from y0, planes from z0
  int y0, ny_rows, z0;
  float rmin2, rmax2;  // draw.hpp:377-381
  unsigned id;         // list index + 1
  int pad;
};

// the record that owns row r: the first k with row_end[k] > r
__device__ inline int rec_of_row(const i64* __restrict__ row_end, int nrec, i64 r) {
  int lo = 0, hi = nrec - 1;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (row_end[mid] > r) hi = mid;
    else lo = mid + 1;
  }
  return lo;
}

// COUNT false: owner[v] = max(owner[v], id) over the shell voxels of every row.
// COUNT true:  count[id - 1] += the row's shell voxels with mask != 0.
template <bool COUNT>
__global__ void __launch_bounds__(BLOCK)
scatter_kernel(const SphereRec* __restrict__ rec, const i64* __restrict__ row_end, int nrec, i64 nrows,
               unsigned* __restrict__ owner, const float* __restrict__ mask, unsigned long long* __restrict__ count, int nx,
               int ny) {
  const int lane = wave_lane();
  const i64 wave = ((i64)blockIdx.x * BLOCK + threadIdx.x) / WAVE;
  const i64 nwaves = (i64)gridDim.x * (BLOCK / WAVE);
  // a wave takes a run of consecutive rows: one search for the first, then the records are walked in order
  const i64 per_wave = (nrows + nwaves - 1) / nwaves;
  const i64 r0 = wave * per_wave, r1 = r0 + per_wave < nrows ? r0 + per_wave : nrows;
  if (r0 >= r1) return;
  int k = rec_of_row(row_end, nrec, r0);
  SphereRec s = rec[k];
  i64 first = k ? row_end[k - 1] : 0, end = row_end[k];
  for (i64 r = r0; r < r1; r++) {
    while (r >= end) {   // records hold at least one row each
      first = end;
      k++;
      s = rec[k];
      end = row_end[k];
    }
    const i64 local = r - first;
    const int y = s.y0 + (int)(local % s.ny_rows), z = s.z0 + (int)(local / s.ny_rows);
    const int jy = y - s.cy, jz = z - s.cz;
    const int base = jy * jy + jz * jz;
    // int -> float conversion is monotone, so a row whose jx = 0 voxel is already outside holds no shell voxel
    if (!((float)base <= s.rmax2)) continue;
    const i64 row = ((i64)z * ny + y) * nx;
    unsigned long long mine = 0;
    for (int x = s.x0 + lane; x <= s.x1; x += WAVE) {
      const int jx = x - s.cx;
      const float rsqr = (float)(jx * jx + base);   // the reference compares its int rsqr as a float (draw.hpp:425)
      if (s.rmin2 <= rsqr && rsqr <= s.rmax2) {
        if (COUNT) mine += (!mask || mask[row + x] != 0.0f) ? 1 : 0;
        else atomicMax(&owner[row + x], s.id);
      }
    }
    // the wave's rows and skips: every lane is here.  __shfl_down measured 0.5-1.7 % faster than wave_count (profiles/wave_refactor_time.txt)
    if (COUNT) {
      for (int d = WAVE / 2; d > 0; d >>= 1) mine += __shfl_down(mine, d, WAVE);
      if (lane == 0 && mine) atomicAdd(&count[s.id - 1], mine);
    }
  }
}

// draw.hpp:418-420, :440: the multiplier is the double 1.0 / n rounded to float; n == 0 leaves it 1
__global__ void __launch_bounds__(BLOCK)
value_kernel(float* __restrict__ value, const unsigned long long* __restrict__ count, i64 n) {
  for (i64 i = (i64)blockIdx.x * BLOCK + threadIdx.x; i < n; i += (i64)gridDim.x * BLOCK) {
    const unsigned long long c = count[i];
    const float mult = c > 0 ? (float)(1.0 / (double)c) : 1.0f;
    value[i] = value[i] * mult;
  }
}

struct Background {
  float rescale, offset;
  int normalize;        // draw.hpp:334-342
  int stddev_positive;
  float ave, stddev;
  double rms;
};

__global__ void __launch_bounds__(BLOCK)
resolve_kernel(float* dst, const float* bg, const float* __restrict__ mask, const unsigned* __restrict__ owner,
               const float* __restrict__ value, Background b, i64 n) {
  for (i64 i = (i64)blockIdx.x * BLOCK + threadIdx.x; i < n; i += (i64)gridDim.x * BLOCK) {
    const unsigned o = owner ? owner[i] : 0u;
    float v;
    if (o && (!mask || mask[i] != 0.0f)) {
      v = value[o - 1];
    } else {
      if (!b.normalize) v = bg[i] * b.rescale;
      else if (b.stddev_positive) v = (float)((double)((bg[i] - b.ave) / b.stddev) * b.rms * (double)b.rescale);
      else v = 0.0f;
      v = v + b.offset;   // a second rounding (draw.hpp:352); the build has -ffp-contract=off
    }
    dst[i] = v;
  }
}

// AverageArr and StdDevArr (visfd_utils.hpp:685-790): float accumulators in raster order, the mask as weights
void host_stats(const float* h, const float* w, i64 n, float* ave_out, float* stddev_out) {
  float total = 0.0f, denom = 0.0f;
  for (i64 i = 0; i < n; i++) {
    float v = h[i];
    if (w) {
      v *= w[i];
      denom += w[i];
    } else {
      denom += 1.0f;
    }
    total += v;
  }
  const float ave = total / denom;
  total = 0.0f;
  denom = 0.0f;
  for (i64 i = 0; i < n; i++) {
    float v = h[i] - ave;
    v *= v;
    if (w) {
      v *= w[i];
      denom += w[i];
    } else {
      denom += 1.0f;
    }
    total += v;
  }
  *ave_out = ave;
  *stddev_out = std::sqrt(total / denom);
}

struct SpheresArgs {
  float* dst;
  const float* mask;
  const float* background;
  i64 nx, ny, nz;
  const float *centers, *diameters, *thicknesses, *foreground;
  i64 n;
  float offset, rescale;
  bool background_normalize, foreground_normalize;
  int* any_center_outside;
  const float *host_background, *host_mask;   // the same arrays on the host where the caller has them (for the statistics)
};

bool fits_int(float c) { return std::isfinite(c) && c >= -2147483648.0f && c < 2147483648.0f; }

// Everything that can be refused is refused here, before the device is touched; fills the records of the spheres whose
// clipped box is not empty and the running row count.
int plan_spheres(const SpheresArgs& a, std::vector<SphereRec>* recs, std::vector<i64>* row_end, bool* outside) {
  VH_REQUIRE(a.dst && a.background, "DrawSpheres: null image (the background is required, draw.hpp:321)");
  VH_TRY(check_dims(a.nx, a.ny, a.nz));
  VH_TRY(check_dims32(a.nx, a.ny, a.nz));
  VH_REQUIRE(a.n >= 0 && a.n <= 2147483646LL, "DrawSpheres: at most 2^31 - 2 spheres");
  VH_REQUIRE(a.n == 0 || a.centers, "DrawSpheres: null centers");
  const i64 nvox = a.nx * a.ny * a.nz;
  VH_REQUIRE(a.dst == a.background || !overlaps(a.dst, a.background, nvox), "DrawSpheres: dst partly overlaps the background");
  VH_REQUIRE(!overlaps(a.dst, a.mask, nvox), "DrawSpheres: dst overlaps mask");
  *outside = false;
  i64 rows = 0;
  const i64 size[3] = {a.nx, a.ny, a.nz};
  for (i64 i = 0; i < a.n; i++) {
    const float* c = a.centers + 3 * i;
    VH_REQUIRE(fits_int(c[0]) && fits_int(c[1]) && fits_int(c[2]), "DrawSpheres: a centre is not finite or not representable as int");
    const float d = a.diameters ? a.diameters[i] : 0.0f;            // draw.hpp:261-279
    const float th = a.thicknesses ? a.thicknesses[i] : d / 2;
    VH_REQUIRE(std::isfinite(d), "DrawSpheres: a diameter is not finite");
    const double rs_d = std::ceil(d / 2 - 0.5);                     // draw.hpp:375
    VH_REQUIRE(rs_d <= (double)MAX_RS, "DrawSpheres: diameter too large (3 Rs^2 must stay below 2^31)");
    const int Rs = rs_d < 0 ? 0 : (int)rs_d;
    SphereRec s;
    s.cx = (int)c[0];
    s.cy = (int)c[1];
    s.cz = (int)c[2];
    const float half = d / 2;
    s.rmax2 = half * half;
    s.rmin2 = 0.0f;
    if (th > 0.0 && half - th > 0.0) s.rmin2 = (half - th) * (half - th);
    const int cc[3] = {s.cx, s.cy, s.cz};
    i64 lo[3], hi[3];
    bool empty = false;
    for (int k = 0; k < 3; k++) {
      if (cc[k] < 0 || cc[k] >= size[k]) *outside = true;
      lo[k] = std::max<i64>((i64)cc[k] - Rs, 0);
      hi[k] = std::min<i64>((i64)cc[k] + Rs, size[k] - 1);
      empty = empty || lo[k] > hi[k];
    }
    if (empty) continue;
    s.x0 = (int)lo[0];
    s.x1 = (int)hi[0];
    s.y0 = (int)lo[1];
    s.ny_rows = (int)(hi[1] - lo[1] + 1);
    s.z0 = (int)lo[2];
    s.id = (unsigned)(i + 1);
    s.pad = 0;
    rows += (i64)s.ny_rows * (hi[2] - lo[2] + 1);
    recs->push_back(s);
    row_end->push_back(rows);
  }
  return VISFD_HIP_OK;
}

inline size_t align8(size_t b) { return (b + 7) & ~(size_t)7; }

int draw_spheres(visfd_hip_ctx* ctx, const SpheresArgs& a) {
  VH_REQUIRE(ctx, "null context");
  std::vector<SphereRec> recs;
  std::vector<i64> row_end;
  bool outside = false;
  VH_TRY(plan_spheres(a, &recs, &row_end, &outside));
  VH_HIP(hipSetDevice(ctx->device));
  const i64 nvox = a.nx * a.ny * a.nz;

  Background b = {a.rescale, a.offset, a.background_normalize ? 1 : 0, 0, 0.0f, 1.0f, 1.0};
  if (a.background_normalize) {
    std::vector<float> hb, hm;
    const float *pb = a.host_background, *pm = a.host_mask;
    if (!pb) {   // device face: the statistics need the arrays on the host
      hb.resize((size_t)nvox);
      VH_HIP(hipMemcpyAsync(hb.data(), a.background, sizeof(float) * nvox, hipMemcpyDeviceToHost, ctx->stream));
      if (a.mask) {
        hm.resize((size_t)nvox);
        VH_HIP(hipMemcpyAsync(hm.data(), a.mask, sizeof(float) * nvox, hipMemcpyDeviceToHost, ctx->stream));
      }
      VH_HIP(hipStreamSynchronize(ctx->stream));
      pb = hb.data();
      pm = a.mask ? hm.data() : nullptr;
    }
    host_stats(pb, pm, nvox, &b.ave, &b.stddev);
    b.stddev_positive = b.stddev > 0.0 ? 1 : 0;
    double rms = 0.0;   // draw.hpp:306-310; the square is taken in float
    for (i64 i = 0; i < a.n; i++) {
      const float f = a.foreground ? a.foreground[i] : 1.0f;
      rms += f * f;
    }
    if (a.n > 0) rms = std::sqrt(rms / (double)a.n);
    b.rms = rms;
  }

  // option draw_time: events around the three phases (the call then waits for the last one); without spheres the
  // first two boundaries stay here, with spheres they are marked again below
  PhaseClock<3> clock;
  clock.start(ctx->stream, ctx->opt.draw_time != 0);
  clock.mark(1);

  unsigned* owner = nullptr;
  float* value = nullptr;
  const unsigned gvox = grid_for(nvox, BLOCK, (i64)ctx->num_cus * 64);
  if (!recs.empty()) {
    // one slot: values [n] | counts [n] (foreground_normalize) | records | running row counts
    const size_t nrec = recs.size();
    const size_t off_cnt = align8(sizeof(float) * (size_t)a.n);
    const size_t off_rec = off_cnt + (a.foreground_normalize ? sizeof(unsigned long long) * (size_t)a.n : 0);
    const size_t off_row = off_rec + align8(sizeof(SphereRec) * nrec);
    char* tab = nullptr;
    VH_TRY(ws(ctx, WS_DRAW_TAB, off_row + sizeof(i64) * nrec, &tab));
    VH_TRY(ws(ctx, WS_DRAW_OWNER, (size_t)nvox, &owner));
    value = reinterpret_cast<float*>(tab);
    unsigned long long* count = reinterpret_cast<unsigned long long*>(tab + off_cnt);
    SphereRec* drec = reinterpret_cast<SphereRec*>(tab + off_rec);
    i64* drow = reinterpret_cast<i64*>(tab + off_row);
    std::vector<float> ones;
    const float* fg = a.foreground;
    if (!fg) {
      ones.assign((size_t)a.n, 1.0f);
      fg = ones.data();
    }
    VH_HIP(hipMemcpyAsync(value, fg, sizeof(float) * (size_t)a.n, hipMemcpyHostToDevice, ctx->stream));
    VH_HIP(hipMemcpyAsync(drec, recs.data(), sizeof(SphereRec) * nrec, hipMemcpyHostToDevice, ctx->stream));
    VH_HIP(hipMemcpyAsync(drow, row_end.data(), sizeof(i64) * nrec, hipMemcpyHostToDevice, ctx->stream));
    clock.mark(0);
    VH_HIP(hipMemsetAsync(owner, 0, sizeof(unsigned) * (size_t)nvox, ctx->stream));
    clock.mark(1);
    const i64 nrows = row_end.back();
    const unsigned grows = grid_for(nrows, BLOCK / WAVE, (i64)ctx->num_cus * 64);
    scatter_kernel<false><<<dim3(grows), dim3(BLOCK), 0, ctx->stream>>>(drec, drow, (int)nrec, nrows, owner, nullptr, nullptr,
                                                                        (int)a.nx, (int)a.ny);
    VH_HIP(hipGetLastError());
    if (a.foreground_normalize) {
      VH_HIP(hipMemsetAsync(count, 0, sizeof(unsigned long long) * (size_t)a.n, ctx->stream));
      scatter_kernel<true><<<dim3(grows), dim3(BLOCK), 0, ctx->stream>>>(drec, drow, (int)nrec, nrows, nullptr, a.mask, count,
                                                                         (int)a.nx, (int)a.ny);
      VH_HIP(hipGetLastError());
      value_kernel<<<dim3(grid_for(a.n, BLOCK, (i64)ctx->num_cus * 64)), dim3(BLOCK), 0, ctx->stream>>>(value, count, a.n);
      VH_HIP(hipGetLastError());
    }
  }
  clock.mark(2);
  resolve_kernel<<<dim3(gvox), dim3(BLOCK), 0, ctx->stream>>>(a.dst, a.background, a.mask, owner, value, b, nvox);
  VH_HIP(hipGetLastError());
  clock.mark(3);
  if (clock.on) {
    VH_HIP(hipStreamSynchronize(ctx->stream));
    clock.read(ctx->draw_ms);
  }
  if (a.any_center_outside) *a.any_center_outside = outside ? 1 : 0;
  return VISFD_HIP_OK;
}

// ---- DrawRegions ------------------------------------------------------------------------------------------------------

// draw.hpp:165-173 and :202-210
__device__ inline void put(float* dst, const float* mask, i64 i, float value, int subtract) {
  if (mask && mask[i] == 0.0f) return;
  if (value < 0) {
    if (subtract && dst[i] > 0) dst[i] = 0.0f;
  } else {
    dst[i] = value;
  }
}

struct Box {
  int x0, y0, z0, bx, by, bz;   // origin and extent, inside the image
};

__global__ void __launch_bounds__(BLOCK)
region_rect_kernel(float* dst, const float* __restrict__ mask, Box b, int nx, int ny, float value, int subtract) {
  const i64 n = (i64)b.bx * b.by * b.bz;
  for (i64 i = (i64)blockIdx.x * BLOCK + threadIdx.x; i < n; i += (i64)gridDim.x * BLOCK) {
    const int x = b.x0 + (int)(i % b.bx);
    const i64 r = i / b.bx;
    const int y = b.y0 + (int)(r % b.by), z = b.z0 + (int)(r / b.by);
    put(dst, mask, ((i64)z * ny + y) * nx + x, value, subtract);
  }
}

// draw.hpp:146-152: per row, x runs over |jx| <= floor(sqrt(R * R - (jy * jy + jz * jz))), all in float
__global__ void __launch_bounds__(BLOCK)
region_sphere_kernel(float* dst, const float* __restrict__ mask, Box b, int nx, int ny, int cx, int cy, int cz, float R,
                     float value, int subtract) {
  const i64 n = (i64)b.bx * b.by * b.bz;
  for (i64 i = (i64)blockIdx.x * BLOCK + threadIdx.x; i < n; i += (i64)gridDim.x * BLOCK) {
    const int x = b.x0 + (int)(i % b.bx);
    const i64 r = i / b.bx;
    const int y = b.y0 + (int)(r % b.by), z = b.z0 + (int)(r / b.by);
    const int jx = x - cx, jy = y - cy, jz = z - cz;
    const float descr = R * R - (float)(jy * jy + jz * jz);
    if (descr < 0.0f) continue;
    const int xrange = (int)floorf(sqrtf(descr));
    if (jx < -xrange || jx > xrange) continue;
    put(dst, mask, ((i64)z * ny + y) * nx + x, value, subtract);
  }
}

// draw.hpp:108-132: *flag becomes non-zero when an unmasked voxel is not 0; then, if it stayed 0, unmasked voxels become 1
__global__ void __launch_bounds__(BLOCK)
any_nonzero_kernel(const float* __restrict__ dst, const float* __restrict__ mask, i64 n, unsigned* flag) {
  bool any = false;
  for (i64 i = (i64)blockIdx.x * BLOCK + threadIdx.x; i < n; i += (i64)gridDim.x * BLOCK)
    any = any || ((!mask || mask[i] != 0.0f) && dst[i] != 0.0f);
  if (any) atomicOr(flag, 1u);
}
__global__ void __launch_bounds__(BLOCK)
fill_ones_kernel(float* dst, const float* __restrict__ mask, i64 n, const unsigned* __restrict__ flag) {
  if (*flag) return;
  for (i64 i = (i64)blockIdx.x * BLOCK + threadIdx.x; i < n; i += (i64)gridDim.x * BLOCK)
    if (!mask || mask[i] != 0.0f) dst[i] = 1.0f;
}

// the part of [lo, hi] (floats, as the reference holds them) inside [0, n - 1]; false: empty (draw.hpp:190-198)
bool rect_range(float fmin, float fmax, i64 n, int* o, int* len) {
  const float lo = std::max<float>((float)std::floor(fmin + 0.5), 0);
  const float hi = std::min<float>((float)std::floor(fmax + 0.5), (float)(n - 1));
  if (!(lo <= hi)) return false;
  const i64 ilo = (i64)lo, ihi = std::min<i64>((i64)hi, n - 1);
  if (ilo > ihi) return false;
  *o = (int)ilo;
  *len = (int)(ihi - ilo + 1);
  return true;
}

int draw_regions(visfd_hip_ctx* ctx, float* dst, const float* mask, i64 nx, i64 ny, i64 nz, const visfd_hip_region* regions,
                 i64 n, bool subtract) {
  VH_REQUIRE(ctx && dst, "null argument");
  VH_TRY(check_dims(nx, ny, nz));
  VH_TRY(check_dims32(nx, ny, nz));
  VH_REQUIRE(n >= 0 && (n == 0 || regions), "DrawRegions: bad region list");
  const i64 nvox = nx * ny * nz;
  VH_REQUIRE(!overlaps(dst, mask, nvox), "DrawRegions: dst overlaps mask");
  for (i64 i = 0; i < n; i++) {
    const visfd_hip_region& g = regions[i];
    VH_REQUIRE(g.type == VISFD_HIP_REGION_RECT || g.type == VISFD_HIP_REGION_SPHERE, "DrawRegions: unknown region type");
    if (g.type != VISFD_HIP_REGION_SPHERE) continue;
    for (int k = 0; k < 3; k++)
      VH_REQUIRE(std::isfinite(g.c[k]) && std::fabs(std::floor(g.c[k] + 0.5)) < 2147483648.0,
                 "DrawRegions: a sphere centre is not finite or not representable as int");
    // 2 Ri^2 must stay below 2^31 (the reference's int jy * jy + jz * jz)
    VH_REQUIRE(std::isfinite(g.c[3]) && std::ceil(g.c[3] - 0.5) <= 32767.0, "DrawRegions: sphere radius not finite or too large");
  }
  VH_HIP(hipSetDevice(ctx->device));
  const i64 cap = (i64)ctx->num_cus * 64;
  if (subtract && n > 0 && regions[0].value < 0) {
    unsigned* flag = nullptr;
    VH_TRY(ws(ctx, WS_DRAW_TAB, 2, &flag));
    VH_HIP(hipMemsetAsync(flag, 0, sizeof(unsigned), ctx->stream));
    any_nonzero_kernel<<<dim3(grid_for(nvox, BLOCK, cap)), dim3(BLOCK), 0, ctx->stream>>>(dst, mask, nvox, flag);
    VH_HIP(hipGetLastError());
    fill_ones_kernel<<<dim3(grid_for(nvox, BLOCK, cap)), dim3(BLOCK), 0, ctx->stream>>>(dst, mask, nvox, flag);
    VH_HIP(hipGetLastError());
  }
  const i64 size[3] = {nx, ny, nz};
  for (i64 i = 0; i < n; i++) {
    const visfd_hip_region& g = regions[i];
    int o[3], len[3];
    bool empty = false;
    if (g.type == VISFD_HIP_REGION_RECT) {
      for (int k = 0; k < 3; k++) empty = empty || !rect_range(g.c[2 * k], g.c[2 * k + 1], size[k], &o[k], &len[k]);
      if (empty) continue;
      const Box b = {o[0], o[1], o[2], len[0], len[1], len[2]};
      region_rect_kernel<<<dim3(grid_for((i64)len[0] * len[1] * len[2], BLOCK, cap)), dim3(BLOCK), 0, ctx->stream>>>(
          dst, mask, b, (int)nx, (int)ny, g.value, subtract ? 1 : 0);
    } else {
      const float R = g.c[3];
      const int Ri = (int)std::ceil(R - 0.5);   // draw.hpp:141-145
      int c[3];
      for (int k = 0; k < 3; k++) {
        c[k] = (int)std::floor(g.c[k] + 0.5);
        const i64 lo = std::max<i64>((i64)c[k] - Ri, 0), hi = std::min<i64>((i64)c[k] + Ri, size[k] - 1);
        empty = empty || lo > hi;
        o[k] = (int)lo;
        len[k] = (int)(hi - lo + 1);
      }
      if (empty) continue;
      const Box b = {o[0], o[1], o[2], len[0], len[1], len[2]};
      region_sphere_kernel<<<dim3(grid_for((i64)len[0] * len[1] * len[2], BLOCK, cap)), dim3(BLOCK), 0, ctx->stream>>>(
          dst, mask, b, (int)nx, (int)ny, c[0], c[1], c[2], R, g.value, subtract ? 1 : 0);
    }
    VH_HIP(hipGetLastError());
  }
  return VISFD_HIP_OK;
}

}  // namespace
}  // namespace vh

using namespace vh;

extern "C" {

int visfd_hip_draw_spheres_dev(visfd_hip_ctx* ctx, float* dst, const float* mask, const float* background, int64_t nx,
                               int64_t ny, int64_t nz, const float* centers, const float* diameters,
                               const float* shell_thicknesses, const float* foreground, int64_t n, float background_offset,
                               float background_rescale, int background_normalize, int foreground_normalize,
                               int* any_center_outside) {
  const SpheresArgs a = {dst, mask, background, nx, ny, nz, centers, diameters, shell_thicknesses, foreground, n,
                         background_offset, background_rescale, background_normalize != 0, foreground_normalize != 0,
                         any_center_outside, nullptr, nullptr};
  return draw_spheres(ctx, a);
}

int visfd_hip_draw_spheres(visfd_hip_ctx* ctx, float* dst, const float* mask, const float* background, int64_t nx, int64_t ny,
                           int64_t nz, const float* centers, const float* diameters, const float* shell_thicknesses,
                           const float* foreground, int64_t n, float background_offset, float background_rescale,
                           int background_normalize, int foreground_normalize, int* any_center_outside) {
  SpheresArgs a = {dst, mask, background, nx, ny, nz, centers, diameters, shell_thicknesses, foreground, n,
                   background_offset, background_rescale, background_normalize != 0, foreground_normalize != 0,
                   any_center_outside, background, mask};
  // the staged background is the source; the device copy of dst is written in full, and comes down only on success
  return stage_filter(ctx, background, dst, mask, nx, ny, nz, false, [&](const float* db, float* dd, const float* dm) {
    a.dst = dd;
    a.background = db;
    a.mask = dm;
    return draw_spheres(ctx, a);
  });
}

int visfd_hip_draw_last_times(visfd_hip_ctx* ctx, float ms[3]) {
  VH_REQUIRE(ctx && ms, "null argument");
  for (int k = 0; k < 3; k++) ms[k] = ctx->draw_ms[k];
  return VISFD_HIP_OK;
}

int visfd_hip_draw_regions_dev(visfd_hip_ctx* ctx, float* dst, const float* mask, int64_t nx, int64_t ny, int64_t nz,
                               const visfd_hip_region* regions, int64_t n, int negative_means_subtract) {
  return draw_regions(ctx, dst, mask, nx, ny, nz, regions, n, negative_means_subtract != 0);
}

int visfd_hip_draw_regions(visfd_hip_ctx* ctx, float* dst, const float* mask, int64_t nx, int64_t ny, int64_t nz,
                           const visfd_hip_region* regions, int64_t n, int negative_means_subtract) {
  VH_REQUIRE(ctx && dst, "null argument");
  // dst is read (subtraction, the all-zero test) and only partly written: its device copy starts from the caller's values
  return stage_filter(ctx, dst, dst, mask, nx, ny, nz, true, [&](const float*, float* dd, const float* dm) {
    return draw_regions(ctx, dd, dm, nx, ny, nz, regions, n, negative_means_subtract != 0);
  });
}

}  // extern "C"
