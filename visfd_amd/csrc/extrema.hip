// extrema.hip -- plateau-aware local minima and maxima: _FindExtrema (reference lib/visfd/morphology_implementation.hpp:
// 57-515), the engine of FindMinima / FindMaxima and of filter_mrc's -find-minima / -find-maxima.
//
// A plateau is a maximal set of existing voxels (mask != 0) joined through neighbour pairs of equal value; it is a
// minimum unless a member has a lower existing neighbour, a maximum unless a member has a higher one, and -- when
// borders are not allowed -- neither if a member has a neighbour that is outside the image or masked out.  Nothing is
// rounded here: the results are indices, counts and copied floats, and they are the reference's, ties and quirks included.
//
// Six kernels, none of them launched more often than once (twice for the list kernel) whatever the plateaus look like:
//  classify   an LDS tile with a one-voxel halo; one byte per voxel: has a lower / a higher / an equal neighbour, touches
//             a missing one, is itself masked out.  A voxel without an equal neighbour is a plateau of its own and is
//             finished here; the others get parent[i] = i and count[i] = 0.
//  merge      union-find over the voxels that have an equal neighbour: each looks at the forward half of its
//             neighbourhood and unites itself with every equal neighbour there.  Roots are hooked with atomicMin towards
//             the smaller linear index, so the surviving representative of a plateau is its first voxel in raster order
//             (the reference's root); finds halve their paths with atomicMin as they go.
//  flatten    parent[i] = root(i).
//  reduce     members OR their disqualifying bits into the root's byte and add themselves to the root's count.
//  list       every root (and every voxel without an equal neighbour) that is an extremum and passes its threshold is
//             counted (first launch) and written as (index, score, voxels) into lists of exactly that size (second).
//  labels     the reference's label image; see write_labels_kernel.
// The lists are put in order on the host (they are small next to the volume): the reference's std::sort of (score, raster
// position) for the minima, its exact reverse for the maxima.
//
// Parent pointers only ever decrease, so there are no cycles, and a pointer read late (another CU's L1 is not refreshed)
// is an older link of the same final set: finds still terminate and unions still end in one tree.  Reads of parent[] in
// the merge and flatten kernels are relaxed device-scope atomic loads all the same.
#include <algorithm>
#include <cmath>

#include "common.hpp"
#include "tile.hpp"
#include "union_find.hpp"
#include "wave.hpp"

namespace vh {

namespace {

constexpr unsigned F_LOWER = 1u, F_HIGHER = 2u, F_EQUAL = 4u, F_MISSING = 8u, F_MASKED = 0x80u;

struct Rec {   // one list entry as the list kernel writes it
  int index;
  float score;
  int nvoxels;
};

template <int C>
__global__ void __launch_bounds__(256)
classify_kernel(const float* __restrict__ src, const float* __restrict__ mask, unsigned char* __restrict__ flags,
                int* __restrict__ parent, int* __restrict__ count, int nx, int ny, int nz) {
  __shared__ unsigned tile[LZ * LY * LX];
  const int tx = threadIdx.x, ty = threadIdx.y;
  const int x0 = blockIdx.x * TX, y0 = blockIdx.y * TY, z0 = blockIdx.z * TZ;
  const i64 plane = (i64)nx * ny;
  load_tile(src, mask, 0u, tile, nx, ny, nz);
  const int x = x0 + tx;
  if (x >= nx) return;
#pragma unroll
  for (int o = 0; o < TZ; o++) {
    const int z = z0 + o;
    if (z >= nz) break;
#pragma unroll
    for (int j = 0; j < 2; j++) {
      const int yy = ty + 4 * j, y = y0 + yy;
      if (y >= ny) continue;
      const unsigned* c = tile + ((o + 1) * LY + yy + 1) * LX + tx + 1;
      const unsigned cb = c[0];
      unsigned f = 0;
      if (cb == GONE_BITS) {
        f = F_MASKED;
      } else {
        const float cv = __uint_as_float(cb);
#pragma unroll
        for (int dz = -1; dz <= 1; dz++)
#pragma unroll
          for (int dy = -1; dy <= 1; dy++)
#pragma unroll
            for (int dx = -1; dx <= 1; dx++) {
              if ((dx == 0 && dy == 0 && dz == 0) || dx * dx + dy * dy + dz * dz > C) continue;
              const unsigned nb = c[(dz * LY + dy) * LX + dx];
              const float nv = __uint_as_float(nb);
              if (nb == GONE_BITS) f |= F_MISSING;
              else if (nv == cv) f |= F_EQUAL;
              else if (nv < cv) f |= F_LOWER;
              else if (nv > cv) f |= F_HIGHER;   // a NaN on either side: none of the three
            }
      }
      const i64 i = (i64)z * plane + (i64)y * nx + x;
      flags[i] = (unsigned char)f;
      if (f & F_EQUAL) {
        parent[i] = (int)i;
        count[i] = 0;
      }
    }
  }
}

template <int C>
__global__ void __launch_bounds__(256)
merge_kernel(const float* __restrict__ src, const unsigned char* __restrict__ flags, int* parent, int nx, int ny, int nz,
             i64 nvox) {
  const i64 plane = (i64)nx * ny;
  for (i64 i = (i64)blockIdx.x * 256 + threadIdx.x; i < nvox; i += (i64)gridDim.x * 256) {
    if (!(flags[i] & F_EQUAL)) continue;
    const int z = (int)(i / plane);
    const int r = (int)(i - (i64)z * plane);
    const int y = r / nx, x = r - y * nx;
    const float v = src[i];
    // the forward half of the neighbourhood: (dz, dy, dx) after (0, 0, 0) in raster order
#pragma unroll
    for (int dz = 0; dz <= 1; dz++)
#pragma unroll
      for (int dy = -1; dy <= 1; dy++)
#pragma unroll
        for (int dx = -1; dx <= 1; dx++) {
          if (dx * dx + dy * dy + dz * dz > C) continue;
          if (dz == 0 && (dy < 0 || (dy == 0 && dx <= 0))) continue;
          const int X = x + dx, Y = y + dy, Z = z + dz;
          if ((unsigned)X >= (unsigned)nx || (unsigned)Y >= (unsigned)ny || Z >= nz) continue;
          const i64 j = i + (i64)dz * plane + (i64)dy * nx + dx;
          if ((flags[j] & F_EQUAL) && src[j] == v) unite(parent, (int)i, (int)j);   // F_EQUAL: j exists
        }
  }
}

__global__ void __launch_bounds__(256) flatten_kernel(const unsigned char* __restrict__ flags, int* parent, i64 nvox) {
  for (i64 i = (i64)blockIdx.x * 256 + threadIdx.x; i < nvox; i += (i64)gridDim.x * 256) {
    if (!(flags[i] & F_EQUAL)) continue;
    int x = (int)i;
    for (;;) {   // roots do not move any more; other entries only get closer to theirs
      const int p = ld_parent(parent + x);
      if (p == x) break;
      x = p;
    }
    parent[i] = x;
  }
}

// flags is written (the roots' bytes, through the 32-bit words that hold them: nvox is padded to a multiple of 4) and
// read (every member's own byte; a root's byte only gains bits that its members have)
__global__ void __launch_bounds__(256) reduce_kernel(unsigned char* flags, const int* __restrict__ parent, int* count,
                                                     i64 nvox) {
  const i64 n_round = (nvox + 63) / 64 * 64;   // whole waves stay together for the ballots
  for (i64 i = (i64)blockIdx.x * 256 + threadIdx.x; i < n_round; i += (i64)gridDim.x * 256) {
    const unsigned f = i < nvox ? flags[i] : 0u;
    const bool member = (f & F_EQUAL) != 0;
    const int r = member ? parent[i] : -1;
    // one add per wave where all of a wave's members share their root (the inside of a large plateau)
    const unsigned long long m = __ballot(member);
    if (m == 0) continue;
    const int first = wave_leader(m);
    const int r0 = __shfl(r, first);
    const bool uniform = __ballot(member && r != r0) == 0;
    if (uniform) {
      if (wave_lane() == first) atomicAdd(count + r0, __popcll(m));
    } else if (member) {
      atomicAdd(count + r, 1);
    }
    const unsigned bits = f & (F_LOWER | F_HIGHER | F_MISSING);
    if (member && r != (int)i && (bits & ~(unsigned)flags[r]))
      atomicOr(reinterpret_cast<unsigned*>(flags) + (r >> 2), bits << ((r & 3) * 8));
  }
}

__device__ __forceinline__ unsigned plateau_kind(unsigned f, int allow_borders) {   // bit 0: minimum, bit 1: maximum
  if (!allow_borders && (f & F_MISSING)) return 0u;
  return ((f & F_LOWER) ? 0u : 1u) | ((f & F_HIGHER) ? 0u : 2u);
}

// counters[0], [1]: listed minima and maxima.  out_min / out_max null: count only.
__global__ void __launch_bounds__(256)
list_kernel(const float* __restrict__ src, const unsigned char* __restrict__ flags, const int* __restrict__ parent,
            const int* __restrict__ count, i64 nvox, int find_min, int find_max, float min_thr, float max_thr,
            int allow_borders, unsigned long long* counters, Rec* __restrict__ out_min, Rec* __restrict__ out_max) {
  const i64 n_round = (nvox + 63) / 64 * 64;
  for (i64 i = (i64)blockIdx.x * 256 + threadIdx.x; i < n_round; i += (i64)gridDim.x * 256) {
    const unsigned f = i < nvox ? flags[i] : F_MASKED;
    bool root = !(f & F_MASKED);
    if (root && (f & F_EQUAL)) root = parent[i] == (int)i;
    const unsigned kind = root ? plateau_kind(f, allow_borders) : 0u;
    const float v = kind ? src[i] : 0.0f;
    const bool is_min = find_min && (kind & 1u) && v <= min_thr;   // a NaN passes neither test
    const bool is_max = find_max && (kind & 2u) && v >= max_thr;
    if (__ballot(is_min || is_max) == 0) continue;
    const int n = (is_min || is_max) ? ((f & F_EQUAL) ? count[i] : 1) : 0;
    const unsigned long long pmin = wave_append(is_min, counters + 0);
    const unsigned long long pmax = wave_append(is_max, counters + 1);
    if (is_min && out_min) out_min[pmin] = Rec{(int)i, v, n};
    if (is_max && out_max) out_max[pmax] = Rec{(int)i, v, n};
  }
}

// how many entries of the ascending list idx[0..n) are <= key
__device__ __forceinline__ int count_le(const int* __restrict__ idx, int n, int key) {
  int lo = 0, hi = n;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (idx[mid] <= key) lo = mid + 1;
    else hi = mid;
  }
  return lo;
}

// The reference numbers plateaus as it meets their roots in raster order (morphology_implementation.hpp:330-338): a
// maximum gets the number of maxima listed so far, its own entry included if it is listed -- so a maximum that failed its
// threshold carries the number of the listed maximum before it, or 0; otherwise a minimum gets minus that number of the
// minima list; everything else 0.  The numbers are then replaced by the entries' 1-based positions in the sorted lists
// (:432-487), and negative labels are negated when only one kind was sought (:498-502).  idx_*: the listed roots in
// raster order, rank_*: their positions in the sorted lists.  Voxels with mask == 0 are left alone.
__global__ void __launch_bounds__(256)
write_labels_kernel(const unsigned char* __restrict__ flags, const int* __restrict__ parent, i64 nvox, int allow_borders,
                    const int* __restrict__ idx_min, const int* __restrict__ rank_min, int n_min,
                    const int* __restrict__ idx_max, const int* __restrict__ rank_max, int n_max, int negate,
                    int* __restrict__ labels) {
  for (i64 i = (i64)blockIdx.x * 256 + threadIdx.x; i < nvox; i += (i64)gridDim.x * 256) {
    unsigned f = flags[i];
    if (f & F_MASKED) continue;
    int r = (int)i;
    if (f & F_EQUAL) {
      r = parent[i];
      f = flags[r];
    }
    const unsigned kind = plateau_kind(f, allow_borders);
    int label = 0;
    if (kind & 2u) {
      const int k = count_le(idx_max, n_max, r);
      label = k ? rank_max[k - 1] : 0;
    } else if (kind & 1u) {
      const int k = count_le(idx_min, n_min, r);
      label = k ? -rank_min[k - 1] : 0;
      if (negate) label = -label;
    }
    labels[i] = label;
  }
}

// ascending in (score, raster position), the order std::sort gives the reference's (score, position) tuples: +0 and -0
// tie (no NaN is ever listed); the maxima are that order reversed
void sort_list(std::vector<Rec>& v, bool maxima) {
  std::sort(v.begin(), v.end(), [](const Rec& a, const Rec& b) {
    if (a.score < b.score) return true;
    if (b.score < a.score) return false;
    return a.index < b.index;
  });
  if (maxima) std::reverse(v.begin(), v.end());
}

// the listed roots in raster order and their 1-based positions in the sorted list, on the device
int put_ranks(visfd_hip_ctx* ctx, const std::vector<Rec>& sorted, std::vector<int>& host, int* dev) {
  const size_t n = sorted.size();
  std::vector<std::pair<int, int>> byidx(n);
  for (size_t k = 0; k < n; k++) byidx[k] = std::make_pair(sorted[k].index, (int)k + 1);
  std::sort(byidx.begin(), byidx.end());
  host.resize(2 * n);
  for (size_t k = 0; k < n; k++) {
    host[k] = byidx[k].first;
    host[n + k] = byidx[k].second;
  }
  if (n) VH_HIP(hipMemcpyAsync(dev, host.data(), sizeof(int) * 2 * n, hipMemcpyHostToDevice, ctx->stream));
  return VISFD_HIP_OK;
}

}  // namespace

// everything that can be said without a device, the context last
int extrema_check_args(const visfd_hip_ctx* ctx, const ExtremaArgs& a) {
  VH_REQUIRE(a.connectivity >= 1 && a.connectivity <= VISFD_HIP_EXTREMA_MAX_CONNECTIVITY,
             "find_extrema: connectivity must be 1, 2 or 3 (6, 18 or 26 neighbours)");
  VH_TRY(check_dims(a.nx, a.ny, a.nz));
  const i64 lim = VISFD_HIP_EXTREMA_MAX_VOXELS;
  VH_REQUIRE(a.nx <= lim && a.ny <= lim && a.nz <= lim && a.nx * a.ny <= lim && a.nx * a.ny * a.nz <= lim,
             "find_extrema: the image must have fewer than 2^31 - 2 voxels");
  // the classification pass is one launch of 64 x 8 x 8 tiles: 65535 tiles along y and z, 2^24 workgroups in all
  const i64 tiles = tile_count(a.nx, a.ny, a.nz);
  VH_REQUIRE(a.ny <= VISFD_HIP_EXTREMA_MAX_NY_NZ && a.nz <= VISFD_HIP_EXTREMA_MAX_NY_NZ && tiles < ((i64)1 << 24),
             "find_extrema: ny and nz must be at most 524280, and the image at most 2^24 - 1 tiles of 64 x 8 x 8 voxels");
  VH_REQUIRE(a.find_minima || a.find_maxima, "find_extrema: neither minima nor maxima asked for");
  VH_REQUIRE(a.min_cap >= 0 && a.max_cap >= 0, "find_extrema: negative list capacity");
  VH_REQUIRE(!a.find_minima || a.n_min, "find_extrema: minima asked for without a place for their count");
  VH_REQUIRE(!a.find_maxima || a.n_max, "find_extrema: maxima asked for without a place for their count");
  const size_t nv = (size_t)(a.nx * a.ny * a.nz);
  VH_REQUIRE(!overlap_bytes(a.labels, 4 * nv, a.src, 4 * nv), "find_extrema: labels overlap src");
  VH_REQUIRE(!overlap_bytes(a.labels, 4 * nv, a.mask, 4 * nv), "find_extrema: labels overlap mask");
  VH_REQUIRE(ctx && a.src, "null argument");
  return VISFD_HIP_OK;
}

namespace {

void copy_out(const std::vector<Rec>& v, int64_t* index, float* score, int64_t* nvoxels) {
  for (size_t k = 0; k < v.size(); k++) {
    if (index) index[k] = v[k].index;
    if (score) score[k] = v[k].score;
    if (nvoxels) nvoxels[k] = v[k].nvoxels;
  }
}

template <int C>
int classify_and_merge(visfd_hip_ctx* ctx, const float* src, const float* mask, unsigned char* flags, int* parent,
                       int* count, i64 nx, i64 ny, i64 nz, unsigned g) {
  const dim3 grid((unsigned)((nx + TX - 1) / TX), (unsigned)((ny + TY - 1) / TY), (unsigned)((nz + TZ - 1) / TZ));
  classify_kernel<C><<<grid, dim3(TX, 4), 0, ctx->stream>>>(src, mask, flags, parent, count, (int)nx, (int)ny, (int)nz);
  VH_HIP(hipGetLastError());
  merge_kernel<C><<<dim3(g), dim3(256), 0, ctx->stream>>>(src, flags, parent, (int)nx, (int)ny, (int)nz, nx * ny * nz);
  VH_HIP(hipGetLastError());
  return VISFD_HIP_OK;
}

}  // namespace

namespace {

// what the search leaves on the device, and its two lists
struct Found {
  unsigned char* flags = nullptr;
  int *parent = nullptr, *count = nullptr;
  unsigned long long* counters = nullptr;
  unsigned g = 1;
  unsigned long long n[2] = {0, 0};
  std::vector<Rec> mins, maxs;   // in output order
};

// classification, plateaus and the two list lengths; returns with the stream idle
int count_stage(visfd_hip_ctx* ctx, const ExtremaArgs& a, Found& f) {
  VH_HIP(hipSetDevice(ctx->device));
  const i64 nv = a.nx * a.ny * a.nz;
  const unsigned g = f.g = grid_for(nv, 256, (i64)ctx->num_cus * 16);
  VH_TRY(ws(ctx, WS_EXT_FLAGS, (size_t)((nv + 3) / 4 * 4), &f.flags));
  VH_TRY(ws(ctx, WS_EXT_PARENT, (size_t)nv, &f.parent));
  VH_TRY(ws(ctx, WS_EXT_COUNT, (size_t)nv, &f.count));
  VH_TRY(ws(ctx, WS_EXT_COUNTERS, 2, &f.counters));
  if (a.connectivity == 1) VH_TRY(classify_and_merge<1>(ctx, a.src, a.mask, f.flags, f.parent, f.count, a.nx, a.ny, a.nz, g));
  if (a.connectivity == 2) VH_TRY(classify_and_merge<2>(ctx, a.src, a.mask, f.flags, f.parent, f.count, a.nx, a.ny, a.nz, g));
  if (a.connectivity == 3) VH_TRY(classify_and_merge<3>(ctx, a.src, a.mask, f.flags, f.parent, f.count, a.nx, a.ny, a.nz, g));
  flatten_kernel<<<dim3(g), dim3(256), 0, ctx->stream>>>(f.flags, f.parent, nv);
  VH_HIP(hipGetLastError());
  reduce_kernel<<<dim3(g), dim3(256), 0, ctx->stream>>>(f.flags, f.parent, f.count, nv);
  VH_HIP(hipGetLastError());

  VH_HIP(hipMemsetAsync(f.counters, 0, sizeof(f.n), ctx->stream));
  list_kernel<<<dim3(g), dim3(256), 0, ctx->stream>>>(a.src, f.flags, f.parent, f.count, nv, a.find_minima, a.find_maxima,
                                                      a.minima_threshold, a.maxima_threshold, a.allow_borders, f.counters,
                                                      nullptr, nullptr);
  VH_HIP(hipGetLastError());
  VH_HIP(hipMemcpyAsync(f.n, f.counters, sizeof(f.n), hipMemcpyDeviceToHost, ctx->stream));
  VH_HIP(hipStreamSynchronize(ctx->stream));
  return VISFD_HIP_OK;
}

// the lists themselves, sorted; returns with the stream idle
int list_stage(visfd_hip_ctx* ctx, const ExtremaArgs& a, Found& f) {
  const i64 nv = a.nx * a.ny * a.nz;
  const unsigned long long* n = f.n;
  Rec* recs = nullptr;
  VH_TRY(ws(ctx, WS_EXT_LIST, (size_t)(n[0] + n[1]), &recs));
  VH_HIP(hipMemsetAsync(f.counters, 0, sizeof(f.n), ctx->stream));
  list_kernel<<<dim3(f.g), dim3(256), 0, ctx->stream>>>(a.src, f.flags, f.parent, f.count, nv, a.find_minima, a.find_maxima,
                                                        a.minima_threshold, a.maxima_threshold, a.allow_borders, f.counters,
                                                        recs, recs + n[0]);
  VH_HIP(hipGetLastError());
  f.mins.resize((size_t)n[0]);
  f.maxs.resize((size_t)n[1]);
  if (n[0]) VH_HIP(hipMemcpyAsync(f.mins.data(), recs, sizeof(Rec) * n[0], hipMemcpyDeviceToHost, ctx->stream));
  if (n[1]) VH_HIP(hipMemcpyAsync(f.maxs.data(), recs + n[0], sizeof(Rec) * n[1], hipMemcpyDeviceToHost, ctx->stream));
  VH_HIP(hipStreamSynchronize(ctx->stream));
  sort_list(f.mins, false);
  sort_list(f.maxs, true);
  return VISFD_HIP_OK;
}

}  // namespace

// src, mask, labels on the device; the lists on the host.  Returns with the stream idle.
int dev_find_extrema(visfd_hip_ctx* ctx, const ExtremaArgs& a) {
  Found f;
  VH_TRY(count_stage(ctx, a, f));
  const i64 nv = a.nx * a.ny * a.nz;
  const unsigned long long* n = f.n;
  if (a.n_min) *a.n_min = (int64_t)n[0];
  if (a.n_max) *a.n_max = (int64_t)n[1];
  const bool short_min = a.min_cap > 0 && (unsigned long long)a.min_cap < n[0];
  const bool short_max = a.max_cap > 0 && (unsigned long long)a.max_cap < n[1];
  if (short_min || short_max) return fail(VISFD_HIP_ECAPACITY, "find_extrema: an output list is too small");
  const bool want_min = a.find_minima && (a.min_cap > 0 || a.labels), want_max = a.find_maxima && (a.max_cap > 0 || a.labels);
  if (!want_min && !want_max) return VISFD_HIP_OK;   // counting only

  VH_TRY(list_stage(ctx, a, f));
  if (a.min_cap > 0) copy_out(f.mins, a.min_index, a.min_score, a.min_nvoxels);
  if (a.max_cap > 0) copy_out(f.maxs, a.max_index, a.max_score, a.max_nvoxels);
  if (!a.labels) return VISFD_HIP_OK;

  int* ranks = nullptr;
  VH_TRY(ws(ctx, WS_EXT_RANKS, (size_t)(2 * (n[0] + n[1])), &ranks));
  std::vector<int> hmin, hmax;
  int* rmin = ranks;
  int* rmax = ranks + 2 * n[0];
  VH_TRY(put_ranks(ctx, f.mins, hmin, rmin));
  VH_TRY(put_ranks(ctx, f.maxs, hmax, rmax));
  write_labels_kernel<<<dim3(f.g), dim3(256), 0, ctx->stream>>>(f.flags, f.parent, nv, a.allow_borders, rmin, rmin + n[0],
                                                                (int)n[0], rmax, rmax + n[1], (int)n[1],
                                                                (a.find_minima && a.find_maxima) ? 0 : 1, a.labels);
  VH_HIP(hipGetLastError());
  VH_HIP(hipStreamSynchronize(ctx->stream));   // hmin / hmax go out of scope
  return VISFD_HIP_OK;
}

// The watershed's seeds (watershed.hip): the whole sorted list of one kind, borders allowed, whatever its length -- the
// plateaus' roots and their values.  Returns with the stream idle.
int dev_extrema_seeds(visfd_hip_ctx* ctx, const float* src, const float* mask, i64 nx, i64 ny, i64 nz, bool minima,
                      float threshold, int connectivity, std::vector<int>* index, std::vector<float>* score) {
  ExtremaArgs a = {};
  a.src = src;
  a.mask = mask;
  a.nx = nx;
  a.ny = ny;
  a.nz = nz;
  a.find_minima = minima;
  a.find_maxima = !minima;
  a.minima_threshold = a.maxima_threshold = threshold;
  a.connectivity = connectivity;
  a.allow_borders = 1;
  Found f;
  VH_TRY(count_stage(ctx, a, f));
  VH_TRY(list_stage(ctx, a, f));
  const std::vector<Rec>& v = minima ? f.mins : f.maxs;
  index->resize(v.size());
  score->resize(v.size());
  for (size_t k = 0; k < v.size(); k++) {
    (*index)[k] = v[k].index;
    (*score)[k] = v[k].score;
  }
  return VISFD_HIP_OK;
}

}  // namespace vh
