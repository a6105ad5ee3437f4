// watershed.hip -- watershed segmentation from the image's own minima or maxima: Watershed (reference
// lib/visfd/segmentation.hpp:65-559), the engine of filter_mrc's -watershed.  The reference floods from a priority queue;
// without markers its result is a function of each voxel's neighbourhood, and that function is computed here
// by label propagation.  With markers the flood is serial and runs on the host (watershed_host.cpp), as it does under the
// option watershed_host.
//
// s = value, or -value when starting from maxima (a flipped sign bit: exact).  A voxel is eligible when mask != 0 and
// s <= SIGN * halt_threshold; its neighbours N(v) are the voxels inside the image with mask != 0.  An eligible voxel is
//   interior  no neighbour is lower: a voxel of a plateau's inside.  Interior voxels joined through equal-valued pairs form
//             a component (union-find, union_find.hpp); a minimum plateau is one component, and its root is the seed's.
//   chain     exactly one neighbour attains the lowest lower value: the voxel carries what that neighbour carries.
//   join      several do: it carries the largest of theirs.
// A node is a join or a component's root.  The carried basin c is the least solution of
//   c(seed root) = its place in the seed list
//   c(join)      = max c over the neighbours that attain the lowest lower value
//   c(component) = max over its seed and the chains and joins of its own value next to any member
// and every other voxel reads its node's c.
//
// The kernels:
//  classify   an LDS tile with a one-voxel halo (as extrema.hip's): kind and link per voxel -- an interior voxel or a join
//             links to itself, a chain voxel to its one lowest neighbour; c = -1; an unmasked NaN raises a flag.
//  merge      interior voxels unite with their equal interior neighbours (forward half) and note, in a byte plane of its
//             own, whether an equal neighbour is a chain or a join (a feeder of their component).
//  seed       c[root of seed k] = k.
//  compress   pointer jumping over the links -- down pointers, then union-find parents -- until every eligible voxel links
//             to the node at their end: eight steps per voxel and launch, one host flag read per launch.
//  round      Jacobi rounds over the nodes: a join takes the max over its lowest neighbours' nodes, an interior voxel with
//             a feeder raises its root with atomicMax.  The host reads one flag per round and stops when nothing rose.  A
//             node of value v depends on nodes of lower values and, for a component, on the joins of its own value: at most
//             2 L rounds for L distinct eligible values, plus the one that changes nothing.
//  spread     c[i] = c[node of i].
//  qualify / bound / finish   boundaries (show_boundaries) and the labels, see below.
//
// No kernel depends on seeing, in the same launch, what another workgroup wrote.  c only ever grows and every right-hand
// side is a max, so a value read late is only a smaller one of the same final solution and the next round sees the rest;
// links only ever move further along their own path, and an older link is still a link of that path; a boundary state only
// moves from pending to final.  Reads of link[], c[] and the states that another workgroup may be writing are relaxed
// device-scope atomic loads all the same.
#include <algorithm>
#include <cmath>

#include "common.hpp"
#include "tile.hpp"
#include "union_find.hpp"
#include "watershed_host.hpp"
#include "wave.hpp"

namespace vh {

namespace {

constexpr unsigned K_NONE = 0u, K_INT = 1u, K_CHAIN = 2u, K_JOIN = 3u, K_BITS = 3u;   // K_NONE: not eligible
constexpr unsigned F_EQUAL = 4u;      // interior: has an equal neighbour
constexpr unsigned F_MASKED = 0x80u;  // mask == 0
constexpr unsigned char B_NO = 0, B_YES = 1, B_PENDING = 2;

// f(dx, dy, dz, n) for the neighbours of the connectivity, n = the offset's place among the 27
template <int C, typename F>
__device__ __forceinline__ void each_offset(F f) {
#pragma unroll
  for (int dz = -1; dz <= 1; dz++)
#pragma unroll
    for (int dy = -1; dy <= 1; dy++)
#pragma unroll
      for (int dx = -1; dx <= 1; dx++) {
        if ((dx == 0 && dy == 0 && dz == 0) || dx * dx + dy * dy + dz * dz > C) continue;
        f(dx, dy, dz, (dz + 1) * 9 + (dy + 1) * 3 + dx + 1);
      }
}

struct Dims {
  int nx, ny, nz;
  i64 plane;
};

// f(j, n) for the neighbours of voxel i that lie inside the image
template <int C, typename F>
__device__ __forceinline__ void each_neighbour(i64 i, const Dims& d, F f) {
  const int z = (int)(i / d.plane);
  const int r = (int)(i - (i64)z * d.plane);
  const int y = r / d.nx, x = r - y * d.nx;
  each_offset<C>([&](int dx, int dy, int dz, int n) {
    if ((unsigned)(x + dx) < (unsigned)d.nx && (unsigned)(y + dy) < (unsigned)d.ny && (unsigned)(z + dz) < (unsigned)d.nz)
      f(i + (i64)dz * d.plane + (i64)dy * d.nx + dx, n);
  });
}

__device__ __forceinline__ int ld_int(const int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void st_int(int* p, int v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ float s_of(const float* src, i64 i, unsigned flip) { return __uint_as_float(__float_as_uint(src[i]) ^ flip); }

// one store per wave in which `hit` holds anywhere
__device__ __forceinline__ void raise(bool hit, unsigned* flag) {
  const unsigned long long m = __ballot(hit);
  if (m && wave_lane() == wave_leader(m)) atomicOr(flag, 1u);
}

template <int C>
__global__ void __launch_bounds__(256)
classify_kernel(const float* __restrict__ src, const float* __restrict__ mask, unsigned flip, float thr_s,
                unsigned char* __restrict__ kind, int* __restrict__ link, int* __restrict__ c, unsigned* nan_flag, int nx,
                int ny, int nz) {
  __shared__ unsigned tile[LZ * LY * LX];
  const int tx = threadIdx.x, ty = threadIdx.y;
  const int x0 = blockIdx.x * TX, y0 = blockIdx.y * TY, z0 = blockIdx.z * TZ;
  const i64 plane = (i64)nx * ny;
  if (load_tile(src, mask, flip, tile, nx, ny, nz)) atomicOr(nan_flag, 1u);
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
      const unsigned* t = tile + ((o + 1) * LY + yy + 1) * LX + tx + 1;
      const unsigned cb = t[0];
      const float cs = __uint_as_float(cb);
      const i64 i = (i64)z * plane + (i64)y * nx + x;
      unsigned k = K_NONE;
      int l = (int)i;
      if (cb == GONE_BITS) {
        k = F_MASKED;
      } else if (cs <= thr_s) {   // a NaN is not
        bool equal = false;
        int n_low = 0, off = 0;
        float lowest = 0.0f;
        each_offset<C>([&](int dx, int dy, int dz, int) {
          const unsigned nb = t[(dz * LY + dy) * LX + dx];
          const float ns = __uint_as_float(nb);
          if (nb == GONE_BITS) return;
          if (ns == cs) {
            equal = true;
          } else if (ns < cs) {
            if (n_low == 0 || ns < lowest) {
              lowest = ns;
              n_low = 1;
              off = (dz * ny + dy) * nx + dx;   // |off| <= plane + nx + 1 < 2^31
            } else if (ns == lowest) {
              n_low++;
            }
          }
        });
        if (n_low == 0) k = K_INT | (equal ? F_EQUAL : 0u);
        else if (n_low > 1) k = K_JOIN;
        else {
          k = K_CHAIN;
          l = (int)i + off;
        }
      }
      kind[i] = (unsigned char)k;
      link[i] = l;
      c[i] = -1;
    }
  }
}

// feed[i], written for every interior voxel with an equal neighbour: one of those neighbours is a chain or a join, a feeder
// of the voxel's component.  (A plane of its own -- the boundary states' slot, which is not in use yet -- so that no byte
// of kind is written while other threads read it.)
template <int C>
__global__ void __launch_bounds__(256)
merge_kernel(const float* __restrict__ src, const unsigned char* __restrict__ kind, int* link,
             unsigned char* __restrict__ feed, Dims d, i64 nvox) {
  for (i64 i = (i64)blockIdx.x * 256 + threadIdx.x; i < nvox; i += (i64)gridDim.x * 256) {
    if ((kind[i] & (K_BITS | F_EQUAL)) != (K_INT | F_EQUAL)) continue;
    const float v = src[i];
    bool fed = false;
    each_neighbour<C>(i, d, [&](i64 j, int) {
      const unsigned kj = kind[j] & K_BITS;
      if (kj == K_NONE || src[j] != v) return;   // an equal neighbour with mask != 0 is eligible too
      if (kj != K_INT) fed = true;
      else if (j > i) unite(link, (int)i, (int)j);
    });
    feed[i] = fed ? 1 : 0;
  }
}

__global__ void __launch_bounds__(256) seed_kernel(const int* __restrict__ seeds, int n, int* c) {
  const int k = blockIdx.x * 256 + threadIdx.x;
  if (k < n) c[seeds[k]] = k;
}

// Pointer jumping: every eligible voxel moves its link up to eight steps along its path and reports whether the end is
// still ahead.  Only a voxel's own link is written: a shortcut stored into another voxel's link could arrive after that
// voxel has stored a later one and put an older link back.  Every value a link takes lies further along the voxel's own
// path, so a reader that meets a fresher one only skips more.  A path of length d is done after about log(d) / 3 launches,
// whatever the order in which the workgroups run (a long strictly monotone ramp is the worst case).
__global__ void __launch_bounds__(256) compress_kernel(const unsigned char* __restrict__ kind, int* link, unsigned* unsettled,
                                                       i64 nvox) {
  const i64 n_round = (nvox + 63) / 64 * 64;   // whole waves stay together for the ballot
  for (i64 i = (i64)blockIdx.x * 256 + threadIdx.x; i < n_round; i += (i64)gridDim.x * 256) {
    bool ahead = false;
    if (i < nvox && (kind[i] & K_BITS) != K_NONE) {
      const int first = ld_int(link + i);
      int x = first, p = ld_int(link + x);
#pragma unroll 1
      for (int k = 0; k < 8 && p != x; k++) {
        x = p;
        p = ld_int(link + x);
      }
      if (x != first) st_int(link + i, x);
      ahead = p != x;
    }
    raise(ahead, unsettled);
  }
}

template <int C>
__global__ void __launch_bounds__(256)
round_kernel(const float* __restrict__ src, unsigned flip, const unsigned char* __restrict__ kind,
             const unsigned char* __restrict__ feed, const int* __restrict__ link, int* c, unsigned* changed, Dims d,
             i64 nvox) {
  const i64 n_round = (nvox + 63) / 64 * 64;   // whole waves stay together for the ballot
  for (i64 i = (i64)blockIdx.x * 256 + threadIdx.x; i < n_round; i += (i64)gridDim.x * 256) {
    const unsigned k = i < nvox ? kind[i] : 0u;
    bool rose = false;
    if ((k & K_BITS) == K_JOIN) {
      const float cs = s_of(src, i, flip);
      float lowest = cs;
      int best = -1;
      each_neighbour<C>(i, d, [&](i64 j, int) {
        if ((kind[j] & K_BITS) == K_NONE) return;
        const float ns = s_of(src, j, flip);
        if (!(ns < cs) || ns > lowest) return;
        const int cj = ld_int(c + link[j]);
        best = ns < lowest ? cj : max(best, cj);
        lowest = ns;
      });
      if (best > ld_int(c + i)) {
        atomicMax(c + i, best);
        rose = true;
      }
    } else if ((k & (K_BITS | F_EQUAL)) == (K_INT | F_EQUAL) && feed[i]) {
      const float v = src[i];
      int best = -1;
      each_neighbour<C>(i, d, [&](i64 j, int) {
        const unsigned kj = kind[j] & K_BITS;
        if ((kj == K_CHAIN || kj == K_JOIN) && src[j] == v) best = max(best, ld_int(c + link[j]));
      });
      const int r = link[i];
      if (best > ld_int(c + r)) {
        atomicMax(c + r, best);
        rose = true;
      }
    }
    raise(rose, changed);
  }
}

// a node's c is read by others and rewritten by nobody here
__global__ void __launch_bounds__(256) spread_kernel(const unsigned char* __restrict__ kind, const int* __restrict__ link,
                                                     int* c, i64 nvox) {
  for (i64 i = (i64)blockIdx.x * 256 + threadIdx.x; i < nvox; i += (i64)gridDim.x * 256) {
    if ((kind[i] & K_BITS) == K_NONE) continue;
    const int r = link[i];
    if (r != (int)i) c[i] = c[r];
  }
}

// Boundaries.  b(v) holds when an eligible neighbour x with !b(x) has s(x) < s(v) and c(x) != c(v), or s(x) == s(v) and
// c(x) > c(v): x is then labelled before v in the flood (lower first, within a value the larger basin first) and carries
// another basin.  Such an x is a qualifying neighbour; qual gets one bit per neighbour offset, and a voxel without any is
// no boundary at once.
template <int C>
__global__ void __launch_bounds__(256)
qualify_kernel(const float* __restrict__ src, unsigned flip, const unsigned char* __restrict__ kind,
               const int* __restrict__ c, unsigned* __restrict__ qual, unsigned char* __restrict__ state, Dims d, i64 nvox) {
  for (i64 i = (i64)blockIdx.x * 256 + threadIdx.x; i < nvox; i += (i64)gridDim.x * 256) {
    unsigned bits = 0;
    if ((kind[i] & K_BITS) != K_NONE) {
      const float cs = s_of(src, i, flip);
      const int ci = c[i];
      each_neighbour<C>(i, d, [&](i64 j, int n) {
        if ((kind[j] & K_BITS) == K_NONE) return;
        const float ns = s_of(src, j, flip);
        const int cj = c[j];
        if ((ns < cs && cj != ci) || (ns == cs && cj > ci)) bits |= 1u << n;
      });
    }
    qual[i] = bits;
    state[i] = bits ? B_PENDING : B_NO;
  }
}

// A pending voxel is a boundary as soon as one qualifying neighbour is known not to be one, and is none once all of them
// are known to be.  A workgroup takes its tile's states and their halo into LDS, iterates the tile to its fixed point
// there (the halo stays as it was read) and writes back what it settled; the host repeats the launch while anything is
// pending.  The pending voxels that come first in the order (s ascending, c descending) have only settled neighbours to
// wait for, so every launch settles some.
template <int C>
__global__ void __launch_bounds__(256)
bound_kernel(const unsigned* __restrict__ qual, unsigned char* state, unsigned* pending, int nx, int ny, int nz) {
  __shared__ unsigned char tile[LZ * LY * LX];
  const int tx = threadIdx.x, ty = threadIdx.y, tid = ty * TX + tx;
  const int x0 = blockIdx.x * TX, y0 = blockIdx.y * TY, z0 = blockIdx.z * TZ;
  const i64 plane = (i64)nx * ny;
  for (int k = tid; k < LZ * LY * LX; k += 256) {
    const int lx = k % LX, ly = (k / LX) % LY, lz = k / (LX * LY);
    const int X = x0 - 1 + lx, Y = y0 - 1 + ly, Z = z0 - 1 + lz;
    unsigned char b = B_NO;   // outside the image: never looked at (no qualifying bit points there)
    if ((unsigned)X < (unsigned)nx && (unsigned)Y < (unsigned)ny && (unsigned)Z < (unsigned)nz)
      b = __hip_atomic_load(state + ((i64)Z * plane + (i64)Y * nx + X), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    tile[k] = b;
  }
  __syncthreads();
  const int x = x0 + tx;
  unsigned q[2 * TZ];
  unsigned todo = 0;   // bit o * 2 + j: this voxel of mine is pending
#pragma unroll
  for (int o = 0; o < TZ; o++)
#pragma unroll
    for (int j = 0; j < 2; j++) {
      const int yy = ty + 4 * j, y = y0 + yy, z = z0 + o;
      q[o * 2 + j] = 0;
      if (x < nx && y < ny && z < nz && tile[((o + 1) * LY + yy + 1) * LX + tx + 1] == B_PENDING) {
        q[o * 2 + j] = qual[(i64)z * plane + (i64)y * nx + x];
        todo |= 1u << (o * 2 + j);
      }
    }
  for (;;) {   // every thread of the workgroup takes every turn: the barriers are not skipped
    unsigned settled = 0, yes = 0;
#pragma unroll
    for (int o = 0; o < TZ; o++)
#pragma unroll
      for (int j = 0; j < 2; j++) {
        if (!(todo & (1u << (o * 2 + j)))) continue;
        const unsigned char* t = tile + ((o + 1) * LY + ty + 4 * j + 1) * LX + tx + 1;
        const unsigned bits = q[o * 2 + j];
        bool any_no = false, all_yes = true;
        each_offset<C>([&](int dx, int dy, int dz, int n) {
          if (!(bits & (1u << n))) return;
          const unsigned char b = t[(dz * LY + dy) * LX + dx];
          any_no |= b == B_NO;
          all_yes &= b == B_YES;
        });
        if (any_no || all_yes) {
          settled |= 1u << (o * 2 + j);
          if (any_no) yes |= 1u << (o * 2 + j);
        }
      }
    __syncthreads();   // every read of this turn is done
#pragma unroll
    for (int o = 0; o < TZ; o++)
#pragma unroll
      for (int j = 0; j < 2; j++)
        if (settled & (1u << (o * 2 + j))) {
          const unsigned char b = (yes & (1u << (o * 2 + j))) ? B_YES : B_NO;
          tile[((o + 1) * LY + ty + 4 * j + 1) * LX + tx + 1] = b;
          state[(i64)(z0 + o) * plane + (i64)(y0 + ty + 4 * j) * nx + x] = b;
        }
    todo &= ~settled;
    if (!__syncthreads_or(settled != 0)) break;
  }
  if (todo) atomicOr(pending, 1u);
}

// The reference's closing passes (segmentation.hpp:486-517): boundaries (0) become label_boundary, then whatever is -1
// becomes label_undefined, both on voxels with mask != 0 only.  state null: no boundaries were asked for.
__global__ void __launch_bounds__(256)
finish_kernel(const unsigned char* __restrict__ kind, const int* __restrict__ c, const unsigned char* __restrict__ state,
              int label_boundary, int label_undefined, int* __restrict__ labels, i64 nvox) {
  for (i64 i = (i64)blockIdx.x * 256 + threadIdx.x; i < nvox; i += (i64)gridDim.x * 256) {
    const unsigned k = kind[i];
    int label = -1;
    if (!(k & F_MASKED)) {
      if ((k & K_BITS) != K_NONE && c[i] >= 0) label = (state && state[i] == B_YES) ? 0 : c[i] + 1;
      if (label == 0 && label_boundary != 0) label = label_boundary;
      if (label == -1 && label_undefined != -1) label = label_undefined;
    }
    labels[i] = label;
  }
}

template <int C>
int propagate(visfd_hip_ctx* ctx, const WatershedArgs& a, unsigned flip, unsigned char* kind, int* link, int* c,
              unsigned char* state, unsigned* flags, unsigned g, int64_t rounds[2]) {
  const Dims d = {(int)a.nx, (int)a.ny, (int)a.nz, a.nx * a.ny};
  const i64 nv = a.nx * a.ny * a.nz;
  merge_kernel<C><<<dim3(g), dim3(256), 0, ctx->stream>>>(a.src, kind, link, state, d, nv);
  VH_HIP(hipGetLastError());
  unsigned again = 1;
  while (again) {
    VH_HIP(hipMemsetAsync(flags + 1, 0, sizeof(unsigned), ctx->stream));
    compress_kernel<<<dim3(g), dim3(256), 0, ctx->stream>>>(kind, link, flags + 1, nv);
    VH_HIP(hipGetLastError());
    VH_HIP(hipMemcpyAsync(&again, flags + 1, sizeof(unsigned), hipMemcpyDeviceToHost, ctx->stream));
    VH_HIP(hipStreamSynchronize(ctx->stream));
  }
  again = 1;
  while (again) {
    VH_HIP(hipMemsetAsync(flags + 1, 0, sizeof(unsigned), ctx->stream));
    round_kernel<C><<<dim3(g), dim3(256), 0, ctx->stream>>>(a.src, flip, kind, state, link, c, flags + 1, d, nv);
    VH_HIP(hipGetLastError());
    VH_HIP(hipMemcpyAsync(&again, flags + 1, sizeof(unsigned), hipMemcpyDeviceToHost, ctx->stream));
    VH_HIP(hipStreamSynchronize(ctx->stream));
    rounds[0]++;
  }
  spread_kernel<<<dim3(g), dim3(256), 0, ctx->stream>>>(kind, link, c, nv);
  VH_HIP(hipGetLastError());
  if (!a.show_boundaries) return VISFD_HIP_OK;
  unsigned* qual = reinterpret_cast<unsigned*>(link);   // the links are not needed any more
  qualify_kernel<C><<<dim3(g), dim3(256), 0, ctx->stream>>>(a.src, flip, kind, c, qual, state, d, nv);
  VH_HIP(hipGetLastError());
  const dim3 grid((unsigned)((a.nx + TX - 1) / TX), (unsigned)((a.ny + TY - 1) / TY), (unsigned)((a.nz + TZ - 1) / TZ));
  again = 1;
  while (again) {
    VH_HIP(hipMemsetAsync(flags + 1, 0, sizeof(unsigned), ctx->stream));
    bound_kernel<C><<<grid, dim3(TX, 4), 0, ctx->stream>>>(qual, state, flags + 1, d.nx, d.ny, d.nz);
    VH_HIP(hipGetLastError());
    VH_HIP(hipMemcpyAsync(&again, flags + 1, sizeof(unsigned), hipMemcpyDeviceToHost, ctx->stream));
    VH_HIP(hipStreamSynchronize(ctx->stream));
    rounds[1]++;
  }
  return VISFD_HIP_OK;
}

template <int C>
void launch_classify(visfd_hip_ctx* ctx, const WatershedArgs& a, unsigned flip, float thr_s, unsigned char* kind, int* link,
                     int* c, unsigned* flags) {
  const dim3 grid((unsigned)((a.nx + TX - 1) / TX), (unsigned)((a.ny + TY - 1) / TY), (unsigned)((a.nz + TZ - 1) / TZ));
  classify_kernel<C><<<grid, dim3(TX, 4), 0, ctx->stream>>>(a.src, a.mask, flip, thr_s, kind, link, c, flags, (int)a.nx,
                                                            (int)a.ny, (int)a.nz);
}

// everything that can be said without a device; the context is checked by the caller
int watershed_check_args(const WatershedArgs& a) {
  VH_REQUIRE(a.connectivity >= 1 && a.connectivity <= VISFD_HIP_EXTREMA_MAX_CONNECTIVITY,
             "watershed: connectivity must be 1, 2 or 3 (6, 18 or 26 neighbours)");
  VH_TRY(check_dims(a.nx, a.ny, a.nz));
  const i64 lim = VISFD_HIP_EXTREMA_MAX_VOXELS;
  VH_REQUIRE(a.nx <= lim && a.ny <= lim && a.nz <= lim && a.nx * a.ny <= lim && a.nx * a.ny * a.nz <= lim,
             "watershed: the image must have fewer than 2^31 - 2 voxels");
  const i64 tiles = tile_count(a.nx, a.ny, a.nz);
  VH_REQUIRE(a.ny <= VISFD_HIP_EXTREMA_MAX_NY_NZ && a.nz <= VISFD_HIP_EXTREMA_MAX_NY_NZ && tiles < ((i64)1 << 24),
             "watershed: ny and nz must be at most 524280, and the image at most 2^24 - 1 tiles of 64 x 8 x 8 voxels");
  VH_REQUIRE(a.halt_threshold == a.halt_threshold, "watershed: the halt threshold is NaN");
  VH_REQUIRE(a.basin_cap >= 0, "watershed: negative list capacity");
  VH_REQUIRE(a.n_basins, "watershed: no place for the number of basins");
  const size_t nv = (size_t)(a.nx * a.ny * a.nz);
  // the array that labels starts in is named first: a pointer aimed into one array may also run on into whatever the
  // allocator put behind it, and the message must not depend on where the arrays lie; then the order is src, mask, markers
  VH_REQUIRE(!overlap_bytes(a.labels, 1, a.src, 4 * nv), "watershed: labels overlap src");
  VH_REQUIRE(!overlap_bytes(a.labels, 1, a.mask, 4 * nv), "watershed: labels overlap mask");
  VH_REQUIRE(!overlap_bytes(a.labels, 1, a.markers, 4 * nv), "watershed: labels overlap markers");
  VH_REQUIRE(!overlap_bytes(a.labels, 4 * nv, a.src, 4 * nv), "watershed: labels overlap src");
  VH_REQUIRE(!overlap_bytes(a.labels, 4 * nv, a.mask, 4 * nv), "watershed: labels overlap mask");
  VH_REQUIRE(!overlap_bytes(a.labels, 4 * nv, a.markers, 4 * nv), "watershed: labels overlap markers");
  VH_REQUIRE(a.src && a.labels, "null argument");
  return VISFD_HIP_OK;
}

// host arrays throughout; no context
int run_host(const WatershedArgs& a) {
  if (host_any_unmasked_nan(a.src, a.mask, a.nx * a.ny * a.nz))
    return fail(VISFD_HIP_EINVAL, "watershed: a voxel with mask != 0 is NaN");
  std::string err;
  const int rc = host_watershed(a, &err);
  return rc == VISFD_HIP_OK ? rc : fail(rc, err);
}

void set_stats(visfd_hip_ctx* ctx, int path, const int64_t rounds[2], int64_t n) {
  ctx->wsh_stats[0] = path;
  ctx->wsh_stats[1] = rounds[0];
  ctx->wsh_stats[2] = rounds[1];
  ctx->wsh_stats[3] = n;
}

// src, mask, labels on the device, no markers; the lists on the host.  Returns with the stream idle.
int dev_watershed(visfd_hip_ctx* ctx, const WatershedArgs& a) {
  VH_HIP(hipSetDevice(ctx->device));
  const i64 nv = a.nx * a.ny * a.nz;
  const unsigned g = grid_for(nv, 256, (i64)ctx->num_cus * 16);
  unsigned char *kind = nullptr, *state = nullptr;
  int *link = nullptr, *c = nullptr, *seeds = nullptr;
  unsigned* flags = nullptr;
  VH_TRY(ws(ctx, WS_WSH_KIND, (size_t)nv, &kind));
  VH_TRY(ws(ctx, WS_WSH_LINK, (size_t)nv, &link));
  VH_TRY(ws(ctx, WS_WSH_C, (size_t)nv, &c));
  VH_TRY(ws(ctx, WS_WSH_STATE, (size_t)nv, &state));   // the feeder plane first, the boundary states afterwards
  VH_TRY(ws(ctx, WS_WSH_FLAGS, 2, &flags));
  const bool minima = a.start_from_minima != 0;
  const unsigned flip = minima ? 0u : 0x80000000u;
  const float thr_s = minima ? a.halt_threshold : -a.halt_threshold;
  VH_HIP(hipMemsetAsync(flags, 0, 2 * sizeof(unsigned), ctx->stream));
  if (a.connectivity == 1) launch_classify<1>(ctx, a, flip, thr_s, kind, link, c, flags);
  if (a.connectivity == 2) launch_classify<2>(ctx, a, flip, thr_s, kind, link, c, flags);
  if (a.connectivity == 3) launch_classify<3>(ctx, a, flip, thr_s, kind, link, c, flags);
  VH_HIP(hipGetLastError());
  unsigned saw_nan = 0;   // read before anything else is spent on an image that is refused
  VH_HIP(hipMemcpyAsync(&saw_nan, flags, sizeof(unsigned), hipMemcpyDeviceToHost, ctx->stream));
  VH_HIP(hipStreamSynchronize(ctx->stream));
  if (saw_nan) return fail(VISFD_HIP_EINVAL, "watershed: a voxel with mask != 0 is NaN");
  std::vector<int> index;
  std::vector<float> score;
  VH_TRY(dev_extrema_seeds(ctx, a.src, a.mask, a.nx, a.ny, a.nz, minima, a.halt_threshold, a.connectivity, &index, &score));
  const i64 n = (i64)index.size();
  *a.n_basins = n;
  VH_REQUIRE(n <= VISFD_HIP_WATERSHED_MAX_BASINS,
             "watershed: more than 2^24 basins (the reference's labels are not exact beyond that)");
  if (a.basin_cap > 0 && a.basin_cap < n) return fail(VISFD_HIP_ECAPACITY, "watershed: the basin list is too small");
  if (a.basin_cap > 0)
    for (i64 k = 0; k < n; k++) {
      if (a.basin_index) a.basin_index[k] = index[(size_t)k];
      if (a.basin_score) a.basin_score[k] = score[(size_t)k];
    }
  if (n) {
    VH_TRY(ws(ctx, WS_WSH_SEEDS, (size_t)n, &seeds));
    VH_HIP(hipMemcpyAsync(seeds, index.data(), sizeof(int) * (size_t)n, hipMemcpyHostToDevice, ctx->stream));
    seed_kernel<<<dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx->stream>>>(seeds, (int)n, c);
    VH_HIP(hipGetLastError());
  }
  int64_t rounds[2] = {0, 0};
  if (a.connectivity == 1) VH_TRY(propagate<1>(ctx, a, flip, kind, link, c, state, flags, g, rounds));
  if (a.connectivity == 2) VH_TRY(propagate<2>(ctx, a, flip, kind, link, c, state, flags, g, rounds));
  if (a.connectivity == 3) VH_TRY(propagate<3>(ctx, a, flip, kind, link, c, state, flags, g, rounds));
  finish_kernel<<<dim3(g), dim3(256), 0, ctx->stream>>>(kind, c, a.show_boundaries ? state : nullptr, a.label_boundary, a.label_undefined, a.labels, nv);
  VH_HIP(hipGetLastError());
  VH_HIP(hipStreamSynchronize(ctx->stream));
  set_stats(ctx, VISFD_HIP_WATERSHED_PATH_DEVICE, rounds, n);
  return VISFD_HIP_OK;
}

bool on_host(const visfd_hip_ctx* ctx, const WatershedArgs& a) { return a.markers || ctx->opt.watershed_host; }

}  // namespace
}  // namespace vh

using namespace vh;

extern "C" {

int visfd_hip_watershed_host(const float* src, const float* mask, const int32_t* markers, int64_t nx, int64_t ny, int64_t nz,
                             float halt_threshold, int start_from_minima, int connectivity, int show_boundaries,
                             int32_t label_boundary, int32_t label_undefined, int32_t* labels, int64_t* basin_index,
                             float* basin_score, int64_t basin_cap, int64_t* n_basins) {
  const WatershedArgs a = {src, mask, markers, nx, ny, nz, halt_threshold, start_from_minima, connectivity, show_boundaries,
                           label_boundary, label_undefined, labels, basin_index, basin_score, basin_cap, n_basins};
  VH_TRY(watershed_check_args(a));
  return run_host(a);
}

int visfd_hip_watershed_dev(visfd_hip_ctx* ctx, const float* src, const float* mask, const int32_t* markers, int64_t nx,
                            int64_t ny, int64_t nz, float halt_threshold, int start_from_minima, int connectivity,
                            int show_boundaries, int32_t label_boundary, int32_t label_undefined, int32_t* labels,
                            int64_t* basin_index, float* basin_score, int64_t basin_cap, int64_t* n_basins) {
  WatershedArgs a = {src, mask, markers, nx, ny, nz, halt_threshold, start_from_minima, connectivity, show_boundaries,
                     label_boundary, label_undefined, labels, basin_index, basin_score, basin_cap, n_basins};
  VH_TRY(watershed_check_args(a));
  VH_REQUIRE(ctx, "null argument");
  if (!on_host(ctx, a)) return dev_watershed(ctx, a);
  // the sequential flood: everything comes down, the labels go back up
  VH_HIP(hipSetDevice(ctx->device));
  const size_t nv = (size_t)(nx * ny * nz);
  std::vector<float> hs(nv), hm(mask ? nv : 0);
  std::vector<int32_t> hk(markers ? nv : 0), hl(nv);
  VH_HIP(hipMemcpyAsync(hs.data(), src, 4 * nv, hipMemcpyDeviceToHost, ctx->stream));
  if (mask) VH_HIP(hipMemcpyAsync(hm.data(), mask, 4 * nv, hipMemcpyDeviceToHost, ctx->stream));
  if (markers) VH_HIP(hipMemcpyAsync(hk.data(), markers, 4 * nv, hipMemcpyDeviceToHost, ctx->stream));
  VH_HIP(hipStreamSynchronize(ctx->stream));
  a.src = hs.data();
  a.mask = mask ? hm.data() : nullptr;
  a.markers = markers ? hk.data() : nullptr;
  a.labels = hl.data();
  VH_TRY(run_host(a));
  VH_HIP(hipMemcpyAsync(labels, hl.data(), 4 * nv, hipMemcpyHostToDevice, ctx->stream));
  VH_HIP(hipStreamSynchronize(ctx->stream));
  const int64_t none[2] = {0, 0};
  set_stats(ctx, VISFD_HIP_WATERSHED_PATH_HOST, none, *n_basins);
  return VISFD_HIP_OK;
}

int visfd_hip_watershed(visfd_hip_ctx* ctx, const float* src, const float* mask, const int32_t* markers, int64_t nx,
                        int64_t ny, int64_t nz, float halt_threshold, int start_from_minima, int connectivity,
                        int show_boundaries, int32_t label_boundary, int32_t label_undefined, int32_t* labels,
                        int64_t* basin_index, float* basin_score, int64_t basin_cap, int64_t* n_basins) {
  WatershedArgs a = {src, mask, markers, nx, ny, nz, halt_threshold, start_from_minima, connectivity, show_boundaries,
                     label_boundary, label_undefined, labels, basin_index, basin_score, basin_cap, n_basins};
  VH_TRY(watershed_check_args(a));
  VH_REQUIRE(ctx, "null argument");
  if (on_host(ctx, a)) {
    VH_TRY(run_host(a));
    const int64_t none[2] = {0, 0};
    set_stats(ctx, VISFD_HIP_WATERSHED_PATH_HOST, none, *n_basins);
    return VISFD_HIP_OK;
  }
  VH_HIP(hipSetDevice(ctx->device));
  const Stage st = {ctx, (size_t)(nx * ny * nz)};
  float *ds, *dm, *dl;
  VH_TRY(st.up(WS_H2D_0, src, &ds));
  VH_TRY(st.up(WS_H2D_1, mask, &dm));
  VH_TRY(st.out(WS_H2D_2, &dl));   // 32-bit words like the floats; every one of them is written
  a.src = ds;
  a.mask = dm;
  a.labels = reinterpret_cast<int32_t*>(dl);
  VH_TRY(dev_watershed(ctx, a));
  return st.down(reinterpret_cast<float*>(labels), dl);
}

int visfd_hip_watershed_last_stats(visfd_hip_ctx* ctx, int64_t out[4]) {
  VH_REQUIRE(ctx && out, "null argument");
  for (int k = 0; k < 4; k++) out[k] = ctx->wsh_stats[k];
  return VISFD_HIP_OK;
}

}  // extern "C"
