// surface_points.hip -- the oriented point cloud of a clustered surface (`-normals-file`; reference
// bin/filter_mrc/handlers.cpp:2039-2309, host form visfd_hip_surface_points in connect.cpp) on the device.
//
//   select   one sweep over the label image and the mask, 16 bytes per load: a selection bit per voxel (a byte per lane),
//            counts per workgroup chunk; a one-workgroup scan of the chunk counts; the selected voxels' indices written
//            from the bits in raster order (wave prefix by shuffles, wave totals in LDS, chunk offsets from the scan).
//   walk     one lane per listed voxel, neighbours in the list in neighbouring lanes.  The statements are those of the host
//            loop, operand order kept, plain IEEE float (no contraction; `/`, sqrtf and roundf are the correctly rounded
//            or exact forms on the device as on the host).  What differs is what is kept: the host keeps every position,
//            arc length and weight of a walk in vectors; a lane keeps the backward weights only (one float per step, in
//            the batch's scratch, [step][lane]), takes the arc lengths from one table per call (s_k = 0 + ds, k times, and
//            its negation: they do not depend on the image) and walks again to the two positions the average lies between.
//            The backward walk runs first so that the sums run in the host's order, farthest backward entry first.
//   ridge    per point the Hessian and the clamped central-difference gradient of the saliency at round(xyz), the text of
//            connect_graph.hpp / connect.cpp; the 3x3 eigen solve (glibc's atan2f, cosf, sinf), the rejections and the
//            voxel_width scaling run on the host over the compacted points (host_surface_ridge_finish, connect.cpp).
//
// Termination and bounds: a walk takes at most `cap` steps per direction (option surface_steps_cap); every position is
// tested as a float (rounded, still a float; a NaN fails) against the image before an index is formed from it, and ends
// the walk as "left the image" otherwise.  A call in which a walk reaches the cap, or a walked point rounds outside the
// image (the host entry would read out of range there), is handed over to the host entry.
#include <chrono>
#include <cmath>
#include <vector>

#include "common.hpp"
#include "connect_graph.hpp"
#include "connect_host.hpp"
#include "wave.hpp"

namespace vh {
namespace {

constexpr int BLOCK = 256;
constexpr int PER_LANE = 8;                     // voxels per lane of the select sweep: two 16-byte loads per image
constexpr int SCAN_BLOCK = 1024;
constexpr i64 WALK_BATCH = 262144;              // lanes per walk launch: what the scratch is sized by
constexpr i64 MAX_DIM = (i64)1 << 24;           // positions are floats

__device__ __forceinline__ void load8(const float* __restrict__ p, i64 base, float v[8]) {
  const float4 a = *reinterpret_cast<const float4*>(p + base);
  const float4 b = *reinterpret_cast<const float4*>(p + base + 4);
  v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w;
  v[4] = b.x; v[5] = b.y; v[6] = b.z; v[7] = b.w;
}

// bits[g]: bit k set where voxel 8 g + k is selected (mask != 0 and label == want; a null image selects everything);
// chunk_count[b]: the selected voxels of workgroup b's BLOCK * PER_LANE voxels.  VEC: both images are 16-byte aligned.
template <bool VEC>
__global__ void __launch_bounds__(BLOCK)
select_kernel(const float* __restrict__ C, const float* __restrict__ M, i64 n, float want, unsigned char* __restrict__ bits,
              unsigned* __restrict__ chunk_count) {
  __shared__ unsigned wsum[BLOCK / WAVE];
  const i64 g = (i64)blockIdx.x * BLOCK + threadIdx.x;
  const i64 base = g * PER_LANE;
  unsigned b = 0;
  if (VEC && base + PER_LANE <= n) {
    float c[8], m[8];
    if (C) load8(C, base, c);
    if (M) load8(M, base, m);
#pragma unroll
    for (int k = 0; k < PER_LANE; k++)
      if ((!M || m[k] != 0.0f) && (!C || c[k] == want)) b |= 1u << k;
  } else {
    for (int k = 0; k < PER_LANE; k++) {
      const i64 i = base + k;
      if (i < n && (!M || M[i] != 0.0f) && (!C || C[i] == want)) b |= 1u << k;
    }
  }
  bits[g] = (unsigned char)b;   // the array has a byte for every launched lane
  const unsigned s = wave_sum((unsigned)__popc(b));
  if (wave_lane() == 0) wsum[threadIdx.x / WAVE] = s;
  __syncthreads();
  if (threadIdx.x == 0) {
    unsigned t = 0;
    for (int w = 0; w < BLOCK / WAVE; w++) t += wsum[w];
    chunk_count[blockIdx.x] = t;
  }
}

// one workgroup: chunk_off[b] = the selected voxels before chunk b; *total = all of them
__global__ void __launch_bounds__(SCAN_BLOCK)
scan_kernel(const unsigned* __restrict__ chunk_count, i64 nchunks, unsigned long long* __restrict__ chunk_off,
            unsigned long long* __restrict__ total) {
  __shared__ unsigned wtot[SCAN_BLOCK / WAVE];
  const int lane = wave_lane(), wave = threadIdx.x / WAVE;
  unsigned long long carry = 0;
  for (i64 t0 = 0; t0 < nchunks; t0 += SCAN_BLOCK) {
    const i64 b = t0 + threadIdx.x;
    const unsigned v = b < nchunks ? chunk_count[b] : 0u;   // at most BLOCK * PER_LANE each: a tile's sum fits 32 bits
    const unsigned incl = wave_scan(v, lane);
    if (lane == WAVE - 1) wtot[wave] = incl;
    __syncthreads();
    unsigned before = 0, tile = 0;
    for (int w = 0; w < SCAN_BLOCK / WAVE; w++) {
      if (w < wave) before += wtot[w];
      tile += wtot[w];
    }
    if (b < nchunks) chunk_off[b] = carry + before + (incl - v);
    carry += tile;
    __syncthreads();
  }
  if (threadIdx.x == 0) *total = carry;
}

// the listed indices from the bits, raster order; `count` is the list's length (the scan's total)
__global__ void __launch_bounds__(BLOCK)
list_kernel(const unsigned char* __restrict__ bits, const unsigned long long* __restrict__ chunk_off, i64 count,
            i64* __restrict__ list) {
  __shared__ unsigned wtot[BLOCK / WAVE];
  const int lane = wave_lane(), wave = threadIdx.x / WAVE;
  const i64 g = (i64)blockIdx.x * BLOCK + threadIdx.x;
  unsigned b = bits[g];
  const unsigned v = (unsigned)__popc(b);
  const unsigned incl = wave_scan(v, lane);
  if (lane == WAVE - 1) wtot[wave] = incl;
  __syncthreads();
  unsigned before = 0;
  for (int w = 0; w < wave; w++) before += wtot[w];
  i64 pos = (i64)chunk_off[blockIdx.x] + before + (incl - v);
  while (b) {
    const int k = __ffs((int)b) - 1;
    b &= b - 1;
    if (pos < count) list[pos] = g * PER_LANE + k;   // always true: the counts come from these bits
    pos++;
  }
}

struct Volumes {
  const float* S;
  const float* C;
  const float* M;
  const float *Vx, *Vy, *Vz;
  int nx, ny, nz;
};

// voxel2cluster == NULL (handlers.cpp:2053-2065): every unmasked voxel as it is
__global__ void __launch_bounds__(BLOCK)
plain_kernel(Volumes v, const i64* __restrict__ list, i64 count, float wx, float wy, float wz, float* __restrict__ xyz,
             float* __restrict__ nrm) {
  const i64 k = (i64)blockIdx.x * BLOCK + threadIdx.x;
  if (k >= count) return;
  const i64 c = list[k];
  const int ix = (int)(c % v.nx), iy = (int)((c / v.nx) % v.ny), iz = (int)(c / ((i64)v.nx * v.ny));
  xyz[3 * k] = ix * wx;
  xyz[3 * k + 1] = iy * wy;
  xyz[3 * k + 2] = iz * wz;
  nrm[3 * k] = v.Vx[c];
  nrm[3 * k + 1] = v.Vy[c];
  nrm[3 * k + 2] = v.Vz[c];
}

// The voxel a position rounds to, if it lies in the image: the test is made on the rounded FLOATS (a NaN or an infinity
// fails every comparison), the index is formed only afterwards.
__device__ __forceinline__ bool voxel_of(const Volumes& v, const float r[3], i64* c) {
  const float tx = roundf(r[0]), ty = roundf(r[1]), tz = roundf(r[2]);
  if (!(tx >= 0.0f && tx <= (float)(v.nx - 1) && ty >= 0.0f && ty <= (float)(v.ny - 1) && tz >= 0.0f && tz <= (float)(v.nz - 1)))
    return false;
  *c = ((i64)(int)tz * v.ny + (int)ty) * v.nx + (int)tx;
  return true;
}
// the loop test of both walks: inside, unmasked, same cluster
__device__ __forceinline__ bool member_of(const Volumes& v, const float r[3], float cluster, i64* c) {
  i64 q;
  if (!voxel_of(v, r, &q)) return false;
  if (v.M && v.M[q] == 0.0f) return false;
  if (v.C[q] != cluster) return false;
  *c = q;
  return true;
}
__device__ __forceinline__ float length_at(const Volumes& v, i64 c, float d[3]) {
  d[0] = v.Vx[c]; d[1] = v.Vy[c]; d[2] = v.Vz[c];
  return sqrtf(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]);
}
// one step from the voxel c: r[d] += ds * drds[d] with sds = ds, r[d] -= ds * drds[d] with sds = -ds (the product's sign
// is exact, and adding a negated number is subtracting it)
__device__ __forceinline__ void advance(const Volumes& v, i64 c, float sds, float r[3]) {
  float d[3];
  const float norm = length_at(v, c, d);
  for (int k = 0; k < 3; k++) r[k] += sds * (d[k] / norm);
}

enum : unsigned { FLAG_STEPS = VISFD_HIP_SURFACE_POINTS_REASON_STEPS, FLAG_BOUNDS = VISFD_HIP_SURFACE_POINTS_REASON_BOUNDS };

// Entries [first, first + count) of the list.  sT[k], k = 0..cap + 1: the arc length after k forward steps.  scratch:
// cap x stride floats, stride >= count.  stats[0]: the reason flags, stats[1]: the longest walk; *steps: all steps taken.
__global__ void __launch_bounds__(BLOCK)
walk_kernel(Volumes v, const i64* __restrict__ list, i64 first, i64 count, float ds, int cap, const float* __restrict__ sT,
            float* __restrict__ scratch, i64 stride, float* __restrict__ xyz, float* __restrict__ nrm,
            unsigned* __restrict__ stats, unsigned long long* __restrict__ steps) {
  const i64 lane_id = (i64)blockIdx.x * BLOCK + threadIdx.x;
  unsigned longest = 0, taken = 0;   // taken: every step of this lane, the failing last ones and the second walk included
  if (lane_id < count) {
    const i64 k = first + lane_id;
    const i64 c = list[k];
    const int ix = (int)(c % v.nx), iy = (int)((c / v.nx) % v.ny), iz = (int)(c / ((i64)v.nx * v.ny));
    const float start[3] = {(float)ix, (float)iy, (float)iz};
    const float cluster = v.C[c], Sc = v.S[c];
    float out[3] = {start[0], start[1], start[2]}, normal[3];
    i64 cn = c;   // the voxel whose direction becomes the normal
    if (ds > 0.0f) {
      bool capped = false;
      // backwards first: the weights into the scratch, nearest first
      float r[3] = {start[0], start[1], start[2]};
      i64 cp = c;
      int nb = 0;
      for (;;) {
        advance(v, cp, -ds, r);
        i64 cq;
        if (!member_of(v, r, cluster, &cq)) break;
        if (nb == cap) { capped = true; break; }
        scratch[(i64)nb * stride + lane_id] = v.S[cq];
        nb++;
        cp = cq;
      }
      float sum_s = 0.0f, sum_w = 0.0f;
      for (int j = nb - 1; j >= 0; j--) {   // from the most negative s
        const float w = scratch[(i64)j * stride + lane_id];
        sum_s += w * -sT[j + 1];
        sum_w += w;
      }
      // forwards: entry 0 is the voxel itself
      r[0] = start[0]; r[1] = start[1]; r[2] = start[2];
      cp = c;
      int nf = 0;
      for (;;) {
        const float w = v.S[cp];
        sum_s += w * sT[nf];
        sum_w += w;
        nf++;
        advance(v, cp, ds, r);
        if (!member_of(v, r, cluster, &cp)) break;
        if (nf == cap + 1) { capped = true; break; }
      }
      longest = (unsigned)(nb > nf - 1 ? nb : nf - 1);
      taken = (unsigned)(nb + 1 + nf);
      if (capped) {
        atomicOr(&stats[0], FLAG_STEPS);
      } else {
        const float ave_s = sum_s / sum_w;
        const int N = nb + nf;
        // entry j of the joined list has s = -sT[nb - j] below nb, sT[j - nb] from nb on
        int i = 0;
        float lo = nb > 0 ? -sT[nb] : sT[0];
        while (i + 1 < N) {
          i++;
          const float hi = i < nb ? -sT[nb - i] : sT[i - nb];
          if (lo <= ave_s && ave_s <= hi) break;
          lo = hi;
        }
        // vR[i] and vR[i + 1] by walking again: the same statements give the same bits
        float ri[3], rj[3] = {0.0f, 0.0f, 0.0f};
        const bool has_next = i + 1 < N;
        bool ok = true;
        r[0] = start[0]; r[1] = start[1]; r[2] = start[2];
        cp = c;
        if (i >= nb) {
          for (int f = 0; f < i - nb && ok; f++) {
            advance(v, cp, ds, r);
            ok = voxel_of(v, r, &cp);
          }
          for (int d = 0; d < 3; d++) ri[d] = r[d];
          cn = cp;
          if (has_next && ok) {
            advance(v, cp, ds, r);
            for (int d = 0; d < 3; d++) rj[d] = r[d];
          }
        } else {
          const int b = nb - 1 - i;   // vR[i] is the position after b + 1 backward steps, vR[i + 1] the one after b
          for (int f = 0; f < b && ok; f++) {
            advance(v, cp, -ds, r);
            ok = voxel_of(v, r, &cp);
          }
          for (int d = 0; d < 3; d++) rj[d] = r[d];
          if (ok) {
            advance(v, cp, -ds, r);
            ok = voxel_of(v, r, &cn);
          }
          for (int d = 0; d < 3; d++) ri[d] = r[d];
        }
        if (!ok) {   // cannot happen: the first walk accepted these positions
          atomicOr(&stats[0], FLAG_BOUNDS);
          cn = c;
        }
        taken += (unsigned)(i >= nb ? i - nb + (has_next ? 1 : 0) : nb - i);
        const float si = i < nb ? -sT[nb - i] : sT[i - nb];
        const float sj = has_next ? (i + 1 < nb ? -sT[nb - i - 1] : sT[i + 1 - nb]) : 0.0f;
        for (int d = 0; d < 3; d++) {
          if (has_next) out[d] = (ri[d] + (rj[d] - ri[d]) * ((ave_s - si) / (sj - si)));
          else out[d] = ri[d];
        }
      }
    }
    float dir[3];
    const float norm = length_at(v, cn, dir);
    for (int d = 0; d < 3; d++) {
      normal[d] = dir[d] / norm;
      normal[d] *= Sc;
    }
    for (int d = 0; d < 3; d++) {
      xyz[3 * k + d] = out[d];
      nrm[3 * k + d] = normal[d];
    }
  }
  // the walks sit inside `if (lane_id < count)`: every lane arrives here, one without a walk with zeros
  for (int o = WAVE / 2; o > 0; o >>= 1) {
    const unsigned u = __shfl_xor(longest, o, WAVE);
    longest = u > longest ? u : longest;
  }
  taken = wave_sum(taken);
  if (wave_lane() == 0 && longest > 0) atomicMax(&stats[1], longest);
  if (wave_lane() == 0 && taken > 0) atomicAdd(steps, (unsigned long long)taken);
}

// rec[9k..]: the Hessian (xx, yy, zz, xy, yz, xz; visfd_utils.hpp:528-616) and the gradient (:631-669) of the saliency at
// round(xyz[3k..]), stencils moved one voxel inwards at a face
__global__ void __launch_bounds__(BLOCK)
ridge_gather_kernel(Volumes v, const float* __restrict__ xyz, i64 count, float* __restrict__ rec, unsigned* __restrict__ stats) {
  const i64 k = (i64)blockIdx.x * BLOCK + threadIdx.x;
  if (k >= count) return;
  const float r[3] = {xyz[3 * k], xyz[3 * k + 1], xyz[3 * k + 2]};
  float out[9] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
  i64 c;
  if (voxel_of(v, r, &c)) {
    int gx = (int)(c % v.nx), gy = (int)((c / v.nx) % v.ny), gz = (int)(c / ((i64)v.nx * v.ny));
    cg::Params p = {};
    p.nx = v.nx; p.ny = v.ny; p.nz = v.nz;
    cg::hessian6(p, v.S, gx, gy, gz, out);
    if (gx == 0) gx++; else if (gx == v.nx - 1) gx--;
    if (gy == 0) gy++; else if (gy == v.ny - 1) gy--;
    if (gz == 0) gz++; else if (gz == v.nz - 1) gz--;
    const i64 sy = v.nx, sz = (i64)v.nx * v.ny;
    const float* s = v.S + ((i64)gz * v.ny + gy) * v.nx + gx;
    out[6] = (float)(0.5 * (s[1] - s[-1]));
    out[7] = (float)(0.5 * (s[sy] - s[-sy]));
    out[8] = (float)(0.5 * (s[sz] - s[-sz]));
  } else {
    atomicOr(&stats[0], FLAG_BOUNDS);
  }
  for (int d = 0; d < 9; d++) rec[9 * k + d] = out[d];
}

// ---- orchestration --------------------------------------------------------------------------------------------------------
struct Call {
  i64 nx, ny, nz;
  int select_cluster;
  const float* voxel_width;
  float curve_ds;
  int find_ridge;
  float max_distance;
  float* crds;    // device or host memory
  float* norms;
  i64 capacity;
  int64_t* n_points;
};

inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }
inline size_t align16(size_t b) { return (b + 15) & ~(size_t)15; }

int check_call(const visfd_hip_ctx* ctx, const float* S, const float* V, const Call& a) {
  VH_REQUIRE(ctx && S && V && a.voxel_width && a.n_points, "surface_points: null argument");
  VH_TRY(check_dims(a.nx, a.ny, a.nz));
  VH_REQUIRE(a.nx >= 3 && a.ny >= 3 && a.nz >= 3, "surface_points: the image must be at least 3 voxels wide");
  VH_REQUIRE(a.nx < MAX_DIM && a.ny < MAX_DIM && a.nz < MAX_DIM, "surface_points: a dimension of 2^24 or more");
  VH_REQUIRE((a.crds == nullptr) == (a.norms == nullptr), "surface_points: crds and norms go together");
  VH_REQUIRE(a.capacity >= 0, "surface_points: negative capacity");
  return VISFD_HIP_OK;
}

void record(visfd_hip_ctx* ctx, int path, unsigned reasons, i64 selected, i64 points, i64 longest, i64 steps = 0) {
  ctx->surface_points_last[0] = path;
  ctx->surface_points_last[1] = reasons;
  ctx->surface_points_last[2] = selected;
  ctx->surface_points_last[3] = points;
  ctx->surface_points_last[4] = longest;
  ctx->surface_points_last[5] = steps;
}

// `count` points from the host arrays to the caller's, which may be device memory; waits
int deliver(visfd_hip_ctx* ctx, const Call& a, const float* xyz, const float* nrm, i64 count, hipMemcpyKind kind) {
  *a.n_points = count;
  if (!a.crds) return VISFD_HIP_OK;
  if (count > a.capacity) return fail(VISFD_HIP_ECAPACITY, "surface_points: output arrays too small");
  if (count > 0) {
    VH_HIP(hipMemcpyAsync(a.crds, xyz, sizeof(float) * 3 * (size_t)count, kind, ctx->stream));
    VH_HIP(hipMemcpyAsync(a.norms, nrm, sizeof(float) * 3 * (size_t)count, kind, ctx->stream));
  }
  VH_HIP(hipStreamSynchronize(ctx->stream));
  return VISFD_HIP_OK;
}

// The device path on device volumes.  *handed: the reasons for which the host entry has to run the call instead (nothing
// has been written to the caller's arrays then).
int run_device(visfd_hip_ctx* ctx, const Volumes& v, const Call& a, unsigned* handed) {
  *handed = 0;
  const i64 n = a.nx * a.ny * a.nz;
  const i64 ngroups = (n + PER_LANE - 1) / PER_LANE;
  const i64 nchunks = (ngroups + BLOCK - 1) / BLOCK;
  VH_REQUIRE(nchunks < ((i64)1 << 31), "surface_points: image too large");
  int cap = ctx->opt.surface_steps_cap;
  if (cap < 1) cap = 1;
  if (cap > 65536) cap = 65536;
  const bool walk = a.curve_ds > 0.0f && v.C;

  unsigned char* bits = nullptr;
  char* tab = nullptr;
  VH_TRY(ws(ctx, WS_SP_BITS, (size_t)(nchunks * BLOCK), &bits));
  const size_t off_off = align16(sizeof(unsigned) * (size_t)nchunks);
  const size_t off_cnt = off_off + sizeof(unsigned long long) * (size_t)nchunks;
  const size_t off_tab = off_cnt + 32;
  VH_TRY(ws(ctx, WS_SP_CHUNKS, off_tab + sizeof(float) * ((size_t)cap + 2), &tab));
  unsigned* chunk_count = reinterpret_cast<unsigned*>(tab);
  unsigned long long* chunk_off = reinterpret_cast<unsigned long long*>(tab + off_off);
  unsigned long long* total = reinterpret_cast<unsigned long long*>(tab + off_cnt);
  unsigned* stats = reinterpret_cast<unsigned*>(tab + off_cnt + 8);
  unsigned long long* steps = reinterpret_cast<unsigned long long*>(tab + off_cnt + 16);
  float* sT = reinterpret_cast<float*>(tab + off_tab);

  std::vector<float> table((size_t)cap + 2);
  if (walk) {   // s = 0; s += ds: the host loop's own statement
    float s = 0.0f;
    for (int k = 0; k < cap + 2; k++) { table[(size_t)k] = s; s += a.curve_ds; }
  }

  PhaseClock<3> clock;   // option surface_points_time
  const bool timed = ctx->opt.surface_points_time != 0;
  for (int k = 0; k < 4; k++) ctx->surface_points_ms[k] = -1.0f;
  VH_HIP(hipMemsetAsync(total, 0, 32, ctx->stream));
  if (walk) VH_HIP(hipMemcpyAsync(sT, table.data(), sizeof(float) * table.size(), hipMemcpyHostToDevice, ctx->stream));
  clock.start(ctx->stream, timed);
  const float want = (float)a.select_cluster;
  if ((!v.C || aligned16(v.C)) && (!v.M || aligned16(v.M)))
    select_kernel<true><<<dim3((unsigned)nchunks), dim3(BLOCK), 0, ctx->stream>>>(v.C, v.M, n, want, bits, chunk_count);
  else
    select_kernel<false><<<dim3((unsigned)nchunks), dim3(BLOCK), 0, ctx->stream>>>(v.C, v.M, n, want, bits, chunk_count);
  VH_HIP(hipGetLastError());
  scan_kernel<<<dim3(1), dim3(SCAN_BLOCK), 0, ctx->stream>>>(chunk_count, nchunks, chunk_off, total);
  VH_HIP(hipGetLastError());
  unsigned long long nsel_u = 0;
  VH_HIP(hipMemcpyAsync(&nsel_u, total, sizeof(nsel_u), hipMemcpyDeviceToHost, ctx->stream));
  VH_HIP(hipStreamSynchronize(ctx->stream));   // (also: `table` has been read)
  const i64 nsel = (i64)nsel_u;
  if (nsel == 0) {
    record(ctx, VISFD_HIP_SURFACE_POINTS_PATH_DEVICE, 0, 0, 0, 0);
    *a.n_points = 0;
    return VISFD_HIP_OK;
  }
  if (!a.crds && !(v.C && a.find_ridge)) {   // counting only, and every selected voxel is a point
    record(ctx, VISFD_HIP_SURFACE_POINTS_PATH_DEVICE, 0, nsel, nsel, 0);
    *a.n_points = nsel;
    return VISFD_HIP_OK;
  }

  i64* list = nullptr;
  float* out = nullptr;
  VH_TRY(ws(ctx, WS_SP_LIST, (size_t)nsel, &list));
  const bool ridge = v.C && a.find_ridge;
  VH_TRY(ws(ctx, WS_SP_OUT, (size_t)nsel * (ridge ? 15 : 6), &out));
  float* xyz = out;
  float* nrm = out + 3 * nsel;
  float* rec = out + 6 * nsel;
  list_kernel<<<dim3((unsigned)nchunks), dim3(BLOCK), 0, ctx->stream>>>(bits, chunk_off, nsel, list);
  VH_HIP(hipGetLastError());
  clock.mark(1);

  if (!v.C) {
    plain_kernel<<<dim3(grid_for(nsel, BLOCK)), dim3(BLOCK), 0, ctx->stream>>>(v, list, nsel, a.voxel_width[0], a.voxel_width[1],
                                                                              a.voxel_width[2], xyz, nrm);
    VH_HIP(hipGetLastError());
  } else {
    const i64 stride = nsel < WALK_BATCH ? nsel : WALK_BATCH;
    float* scratch = nullptr;
    if (walk) VH_TRY(ws(ctx, WS_SP_SCRATCH, (size_t)stride * (size_t)cap, &scratch));
    for (i64 first = 0; first < nsel; first += WALK_BATCH) {   // the batches share the scratch: the stream orders them
      const i64 count = nsel - first < WALK_BATCH ? nsel - first : WALK_BATCH;
      walk_kernel<<<dim3(grid_for(count, BLOCK)), dim3(BLOCK), 0, ctx->stream>>>(v, list, first, count, walk ? a.curve_ds : 0.0f,
                                                                                cap, sT, scratch, stride, xyz, nrm, stats, steps);
      VH_HIP(hipGetLastError());
    }
  }
  clock.mark(2);
  if (ridge) {
    ridge_gather_kernel<<<dim3(grid_for(nsel, BLOCK)), dim3(BLOCK), 0, ctx->stream>>>(v, xyz, nsel, rec, stats);
    VH_HIP(hipGetLastError());
  }
  clock.mark(3);
  unsigned st[2] = {0, 0};
  unsigned long long nsteps = 0;
  VH_HIP(hipMemcpyAsync(st, stats, sizeof(st), hipMemcpyDeviceToHost, ctx->stream));
  VH_HIP(hipMemcpyAsync(&nsteps, steps, sizeof(nsteps), hipMemcpyDeviceToHost, ctx->stream));
  VH_HIP(hipStreamSynchronize(ctx->stream));
  if (clock.on) clock.read(ctx->surface_points_ms);
  if (st[0]) {
    *handed = st[0];
    record(ctx, VISFD_HIP_SURFACE_POINTS_PATH_HANDED_OVER, st[0], nsel, -1, st[1], (i64)nsteps);
    return VISFD_HIP_OK;
  }

  const std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now();
  int rc;
  i64 points = nsel;
  if (!ridge) {
    rc = deliver(ctx, a, xyz, nrm, nsel, hipMemcpyDefault);
  } else {
    std::vector<float> hx(3 * (size_t)nsel), hn(3 * (size_t)nsel), hr(9 * (size_t)nsel);
    VH_HIP(hipMemcpyAsync(hx.data(), xyz, sizeof(float) * hx.size(), hipMemcpyDeviceToHost, ctx->stream));
    VH_HIP(hipMemcpyAsync(hn.data(), nrm, sizeof(float) * hn.size(), hipMemcpyDeviceToHost, ctx->stream));
    VH_HIP(hipMemcpyAsync(hr.data(), rec, sizeof(float) * hr.size(), hipMemcpyDeviceToHost, ctx->stream));
    VH_HIP(hipStreamSynchronize(ctx->stream));
    const int size[3] = {(int)a.nx, (int)a.ny, (int)a.nz};
    points = host_surface_ridge_finish(hx.data(), hn.data(), hr.data(), nsel, size, a.voxel_width, a.max_distance);
    rc = deliver(ctx, a, hx.data(), hn.data(), points, hipMemcpyDefault);
  }
  if (timed)
    ctx->surface_points_ms[3] = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count();
  record(ctx, VISFD_HIP_SURFACE_POINTS_PATH_DEVICE, 0, nsel, points, st[1], (i64)nsteps);
  return rc;
}

}  // namespace
}  // namespace vh

using namespace vh;

extern "C" {

int visfd_hip_surface_points_ctx(visfd_hip_ctx* ctx, const float* saliency, const float* voxel2cluster, const float* direction,
                                 const float* mask, int64_t nx, int64_t ny, int64_t nz, int select_cluster,
                                 const float voxel_width[3], float curve_ds, int find_ridge, float max_distance_to_feature,
                                 float* crds, float* norms, int64_t capacity, int64_t* n_points) {
  const Call a = {nx, ny, nz, select_cluster, voxel_width, curve_ds, find_ridge, max_distance_to_feature, crds, norms, capacity,
                  n_points};
  VH_TRY(check_call(ctx, saliency, direction, a));
  VH_HIP(hipSetDevice(ctx->device));
  const size_t n = (size_t)(nx * ny * nz);
  const Stage st = {ctx, n};
  float *dS, *dC, *dM, *dV;
  VH_TRY(st.up(WS_H2D_0, saliency, &dS));
  VH_TRY(st.up(WS_H2D_1, voxel2cluster, &dC));
  VH_TRY(st.up(WS_H2D_2, mask, &dM));
  VH_TRY(st.up_planar(WS_H2D_3, WS_H2D_4, direction, 3, &dV));
  const Volumes v = {dS, dC, dM, dV, dV + n, dV + 2 * n, (int)nx, (int)ny, (int)nz};
  unsigned handed = 0;
  VH_TRY(run_device(ctx, v, a, &handed));
  if (!handed) return VISFD_HIP_OK;
  const int rc = visfd_hip_surface_points(saliency, voxel2cluster, direction, mask, nx, ny, nz, select_cluster, voxel_width, curve_ds,
                                          find_ridge, max_distance_to_feature, crds, norms, capacity, n_points);
  ctx->surface_points_last[3] = *n_points;
  return rc;
}

int visfd_hip_surface_points_dev(visfd_hip_ctx* ctx, const float* saliency, const float* voxel2cluster, const float* direction,
                                 const float* mask, int64_t nx, int64_t ny, int64_t nz, int select_cluster,
                                 const float voxel_width[3], float curve_ds, int find_ridge, float max_distance_to_feature,
                                 float* crds, float* norms, int64_t capacity, int64_t* n_points) {
  const Call a = {nx, ny, nz, select_cluster, voxel_width, curve_ds, find_ridge, max_distance_to_feature, crds, norms, capacity,
                  n_points};
  VH_TRY(check_call(ctx, saliency, direction, a));
  VH_HIP(hipSetDevice(ctx->device));
  const size_t n = (size_t)(nx * ny * nz);
  const Volumes v = {saliency, voxel2cluster, mask, direction, direction + n, direction + 2 * n, (int)nx, (int)ny, (int)nz};
  unsigned handed = 0;
  VH_TRY(run_device(ctx, v, a, &handed));
  if (!handed) return VISFD_HIP_OK;
  // the hand-over: the volumes to the host, the directions interleaved as the host entry reads them
  VH_REQUIRE((int64_t)n < (1LL << 31), "surface_points: the host entry that has to finish this call takes fewer than 2^31 voxels");
  std::vector<float> hs(n), hc, hm, hp(3 * n), hv(3 * n);
  VH_HIP(hipMemcpyAsync(hs.data(), saliency, sizeof(float) * n, hipMemcpyDeviceToHost, ctx->stream));
  if (voxel2cluster) { hc.resize(n); VH_HIP(hipMemcpyAsync(hc.data(), voxel2cluster, sizeof(float) * n, hipMemcpyDeviceToHost, ctx->stream)); }
  if (mask) { hm.resize(n); VH_HIP(hipMemcpyAsync(hm.data(), mask, sizeof(float) * n, hipMemcpyDeviceToHost, ctx->stream)); }
  VH_HIP(hipMemcpyAsync(hp.data(), direction, sizeof(float) * 3 * n, hipMemcpyDeviceToHost, ctx->stream));
  VH_HIP(hipStreamSynchronize(ctx->stream));
  for (size_t i = 0; i < n; i++)
    for (int d = 0; d < 3; d++) hv[3 * i + d] = hp[(size_t)d * n + i];
  std::vector<float>().swap(hp);
  const float* pc = voxel2cluster ? hc.data() : nullptr;
  const float* pm = mask ? hm.data() : nullptr;
  int64_t count = 0;
  VH_TRY(visfd_hip_surface_points(hs.data(), pc, hv.data(), pm, nx, ny, nz, select_cluster, voxel_width, curve_ds, find_ridge,
                                  max_distance_to_feature, nullptr, nullptr, 0, &count));
  std::vector<float> hx(3 * (size_t)count + 3), hn(3 * (size_t)count + 3);
  VH_TRY(visfd_hip_surface_points(hs.data(), pc, hv.data(), pm, nx, ny, nz, select_cluster, voxel_width, curve_ds, find_ridge,
                                  max_distance_to_feature, hx.data(), hn.data(), count, &count));
  ctx->surface_points_last[3] = count;
  return deliver(ctx, a, hx.data(), hn.data(), count, hipMemcpyDefault);
}

int visfd_hip_surface_points_last(visfd_hip_ctx* ctx, int64_t out[6]) {
  VH_REQUIRE(ctx && out, "null argument");
  for (int k = 0; k < 6; k++) out[k] = ctx->surface_points_last[k];
  return VISFD_HIP_OK;
}

int visfd_hip_surface_points_last_times(visfd_hip_ctx* ctx, float ms[4]) {
  VH_REQUIRE(ctx && ms, "null argument");
  for (int k = 0; k < 4; k++) ms[k] = ctx->surface_points_ms[k];
  return VISFD_HIP_OK;
}

}  // extern "C"
