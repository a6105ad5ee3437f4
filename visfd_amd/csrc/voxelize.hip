// voxelize.hip -- VoxelizeMesh: which grid samples lie inside a closed triangle mesh (the job of the reference's
// bin/voxelize_mesh/voxelize_mesh.py, which asks vtk), and its entry points.
//
// The answer is defined in integers (include/visfd_hip.h states the rule): vertices are quantised on the host to 1/1024
// voxel, rays run along x, a triangle covers a row (iy, iz) by three edge tests with a symbolic tie-break, and its crossing
// toggles the first sample behind it.  On the device:
//   1. the toggle volume (slot WS_VOX_TOGGLE; per row nx + 1 bits in 32-bit words) is zeroed;
//   2. scatter: every covered (triangle, row) pair flips bit k of its row with atomicXor, k = floor(x_c / 1024) + 1 clamped
//      to [0, nx].  XOR does not depend on arrival order.  Two paths share the row routine:
//        scatter_small_kernel  one lane per triangle walks the rows of its clipped box (at most SMALL_ROWS of them: Poisson
//                              meshes have several triangles per voxel, most covering no sample at all);
//        scatter_tiled_kernel  larger boxes are cut into TILE x TILE rows, one wave per (triangle, tile) item, one lane per
//                              row.  The host, which has walked every vertex for the quantisation anyway, counts the tiles
//                              per triangle and scans them; a wave finds its triangle by bisection of the running counts.
//      The cover test is exact in int64 (|q| <= 2^29: differences below 2^31, products below 2^62).  k is estimated in double
//      and accepted only if the exact sign of the plane function (93 bits: __int128) says it is the smallest k with
//      x_c < 1024 k; otherwise k is bisected with that sign (always, under the test option voxelize_bisect).
//   3. fill_kernel, the one pass over the image: an inclusive prefix-XOR along each row (shift-XOR steps inside a word, a
//      wave scan of the words' parities across them, a carry between chunks of 64 words), expanded to floats with 16-byte
//      stores that are contiguous across lanes.  Bit nx of a row is its total parity: odd for no row of a closed mesh.
#include <algorithm>
#include <cmath>
#include <vector>

#include "common.hpp"
#include "wave.hpp"

namespace vh {

namespace {

constexpr int BLOCK = 256;
constexpr int QBITS = 10;             // 1024 units per voxel
constexpr int QMAX = 1 << 29;         // |q| <= 2^29
constexpr int TILE = 8;               // a tile is TILE x TILE rows: one lane each
constexpr int SMALL_ROWS = 16;        // clipped boxes of at most this many rows are walked by one lane
constexpr i64 MAX_NX = (i64)1 << 19;
constexpr i64 MAX_VOXELS = (i64)1 << 31;

typedef __int128 i128;

// the rows (iy, iz) of the image inside a triangle's projected bounding box, both ends included; y0 > y1 or z0 > z1: none
struct RowBox {
  int y0, y1, z0, z1;
};

__host__ __device__ inline int imin3(int a, int b, int c) { return a < b ? (a < c ? a : c) : (b < c ? b : c); }
__host__ __device__ inline int imax3(int a, int b, int c) { return a > b ? (a > c ? a : c) : (b > c ? b : c); }

// a, b, c: the quantised vertices (x, y, z).  q / 1024 rounded up for the low end, down for the high end (>> is the
// arithmetic shift here, so negative values round towards minus infinity)
__host__ __device__ inline RowBox row_box(const int* a, const int* b, const int* c, int ny, int nz) {
  RowBox r;
  const int one = (1 << QBITS) - 1;
  r.y0 = (imin3(a[1], b[1], c[1]) + one) >> QBITS;
  r.y1 = imax3(a[1], b[1], c[1]) >> QBITS;
  r.z0 = (imin3(a[2], b[2], c[2]) + one) >> QBITS;
  r.z1 = imax3(a[2], b[2], c[2]) >> QBITS;
  if (r.y0 < 0) r.y0 = 0;
  if (r.z0 < 0) r.z0 = 0;
  if (r.y1 > ny - 1) r.y1 = ny - 1;
  if (r.z1 > nz - 1) r.z1 = nz - 1;
  return r;
}
__host__ __device__ inline i64 box_rows(const RowBox& r) {
  return (r.y0 > r.y1 || r.z0 > r.z1) ? 0 : (i64)(r.y1 - r.y0 + 1) * (r.z1 - r.z0 + 1);
}
__host__ __device__ inline i64 area2_of(const int* a, const int* b, const int* c) {
  return (i64)(b[1] - a[1]) * (c[2] - a[2]) - (i64)(b[2] - a[2]) * (c[1] - a[1]);
}

struct Tri {
  int a[3], b[3], c[3];
  i64 n[3];   // (B - A) x (C - A); n[0] is area2
};

__device__ inline void load_tri(const int* __restrict__ q, const int* __restrict__ tri, i64 t, Tri* T) {
  const int ia = tri[3 * t], ib = tri[3 * t + 1], ic = tri[3 * t + 2];
  for (int d = 0; d < 3; d++) {
    T->a[d] = q[3 * (i64)ia + d];
    T->b[d] = q[3 * (i64)ib + d];
    T->c[d] = q[3 * (i64)ic + d];
  }
  const i64 bx = T->b[0] - T->a[0], by = T->b[1] - T->a[1], bz = T->b[2] - T->a[2];
  const i64 cx = T->c[0] - T->a[0], cy = T->c[1] - T->a[1], cz = T->c[2] - T->a[2];
  T->n[0] = by * cz - bz * cy;
  T->n[1] = bz * cx - bx * cz;
  T->n[2] = bx * cy - by * cx;
}

__device__ inline int sgn(i64 v) { return (v > 0) - (v < 0); }

// the side of the directed edge a -> b (projected: u = y, v = z) on which the sample lies, the sample moved by (+eps, +eps^2)
__device__ inline int edge_side(const int* a, const int* b, i64 pu, i64 pv) {
  const i64 du = b[1] - a[1], dv = b[2] - a[2];
  const i64 E = du * (pv - a[2]) - dv * (pu - a[1]);   // the sample is inside the triangle's box: |pu - au| < 2^31
  if (E) return sgn(E);
  if (dv) return -sgn(dv);
  return sgn(du);
}

// One (triangle, row) pair, the row inside the triangle's clipped box: false when the triangle does not cover the row,
// otherwise its crossing toggles bit k of the row.
__device__ inline bool scatter_row(const Tri& T, int iy, int iz, int nx, int ny, int W, bool bisect,
                                   unsigned* __restrict__ toggle) {
  const i64 pu = (i64)iy << QBITS, pv = (i64)iz << QBITS;
  const int s = sgn(T.n[0]);
  if (edge_side(T.a, T.b, pu, pv) != s || edge_side(T.b, T.c, pu, pv) != s || edge_side(T.c, T.a, pu, pv) != s) return false;
  // x_c / 1024 = num / den with num = Ax Nx - Ny (pu - Ay) - Nz (pv - Az), den = 1024 Nx; both made to have den > 0
  const i64 du = pu - T.a[1], dv = pv - T.a[2];
  i128 num = (i128)T.a[0] * T.n[0] - (i128)T.n[1] * du - (i128)T.n[2] * dv;
  if (s < 0) num = -num;
  const i128 den = (i128)(s < 0 ? -T.n[0] : T.n[0]) << QBITS;
  // k: the smallest of [0, nx] with num < k den (x_c < 1024 k), nx when there is none
  auto behind = [&](int k) { return num < (i128)k * den; };
  double est = ((double)T.a[0] * (double)T.n[0] - ((double)T.n[1] * (double)du + (double)T.n[2] * (double)dv)) /
               ((double)T.n[0] * 1024.0);
  est = floor(est) + 1.0;
  int k = !(est > 0.0) ? 0 : (est >= (double)nx ? nx : (int)est);
  const bool exact = !bisect && (k == 0 || !behind(k - 1)) && (k == nx || behind(k));
  if (!exact) {
    int lo = 0, hi = nx;
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      if (behind(mid)) hi = mid;
      else lo = mid + 1;
    }
    k = lo;
  }
  atomicXor(&toggle[((i64)iz * ny + iy) * W + (k >> 5)], 1u << (k & 31));
  return true;
}

// the scatter kernels' count: __shfl_down measured a microsecond faster there than wave_count (profiles/wave_refactor_time.txt)
__device__ inline void add_count(unsigned long long mine, unsigned long long* counter) {
  for (int d = WAVE / 2; d > 0; d >>= 1) mine += __shfl_down(mine, d, WAVE);
  if ((threadIdx.x & (WAVE - 1)) == 0 && mine) atomicAdd(counter, mine);
}

// one lane per triangle; triangles with larger boxes are left to the tiled kernel
__global__ void __launch_bounds__(BLOCK)
scatter_small_kernel(const int* __restrict__ q, const int* __restrict__ tri, i64 m, int nx, int ny, int nz, int W,
                     bool bisect, unsigned* __restrict__ toggle, unsigned long long* __restrict__ crossings) {
  unsigned long long mine = 0;
  for (i64 t = (i64)blockIdx.x * BLOCK + threadIdx.x; t < m; t += (i64)gridDim.x * BLOCK) {
    Tri T;
    load_tri(q, tri, t, &T);
    if (T.n[0] == 0) continue;
    const RowBox r = row_box(T.a, T.b, T.c, ny, nz);
    const i64 rows = box_rows(r);
    if (rows == 0 || rows > SMALL_ROWS) continue;
    for (int iz = r.z0; iz <= r.z1; iz++)
      for (int iy = r.y0; iy <= r.y1; iy++) mine += scatter_row(T, iy, iz, nx, ny, W, bisect, toggle) ? 1 : 0;
  }
  add_count(mine, crossings);   // behind the grid-stride loop every lane is back
}

// the tiled triangle that owns item i: the first k with item_end[k] > i
__device__ inline int tri_of_item(const i64* __restrict__ item_end, int n, i64 i) {
  int lo = 0, hi = n - 1;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (item_end[mid] > i) hi = mid;
    else lo = mid + 1;
  }
  return lo;
}

// one wave per (triangle, tile) item, one lane per row of the tile; a wave takes a run of consecutive items
__global__ void __launch_bounds__(BLOCK)
scatter_tiled_kernel(const int* __restrict__ q, const int* __restrict__ tri, const int* __restrict__ tiled_id,
                     const i64* __restrict__ item_end, int ntiled, i64 nitems, int nx, int ny, int nz, int W,
                     bool bisect, unsigned* __restrict__ toggle, unsigned long long* __restrict__ crossings) {
  const int lane = threadIdx.x & (WAVE - 1);
  const i64 wave = ((i64)blockIdx.x * BLOCK + threadIdx.x) / WAVE;
  const i64 nwaves = (i64)gridDim.x * (BLOCK / WAVE);
  const i64 per_wave = (nitems + nwaves - 1) / nwaves;
  const i64 i0 = wave * per_wave, i1 = i0 + per_wave < nitems ? i0 + per_wave : nitems;
  unsigned long long mine = 0;
  if (i0 < i1) {
    int k = tri_of_item(item_end, ntiled, i0);
    i64 first = k ? item_end[k - 1] : 0, end = item_end[k];
    Tri T;
    load_tri(q, tri, tiled_id[k], &T);
    RowBox r = row_box(T.a, T.b, T.c, ny, nz);
    for (i64 i = i0; i < i1; i++) {
      while (i >= end) {   // every listed triangle has at least one item
        first = end;
        k++;
        end = item_end[k];
        load_tri(q, tri, tiled_id[k], &T);
        r = row_box(T.a, T.b, T.c, ny, nz);
      }
      const i64 local = i - first;
      const int tiles_y = (r.y1 - r.y0 + TILE) / TILE;
      const int iy = r.y0 + (int)(local % tiles_y) * TILE + (lane & (TILE - 1));
      const int iz = r.z0 + (int)(local / tiles_y) * TILE + lane / TILE;
      if (iy <= r.y1 && iz <= r.z1) mine += scatter_row(T, iy, iz, nx, ny, W, bisect, toggle) ? 1 : 0;
    }
  }
  add_count(mine, crossings);   // a wave without items skips the `if` above and arrives with zeros
}

// One wave per row.  VEC: nx is a multiple of 4 and dst is 16-byte aligned, so a lane stores four voxels at once.
// counters[1] += rows of odd total parity, counters[2] += inside voxels.
template <bool VEC>
__global__ void __launch_bounds__(BLOCK)
fill_kernel(const unsigned* __restrict__ toggle, float* __restrict__ dst, int nx, i64 nrows, int W,
            unsigned long long* __restrict__ counters) {
  const int lane = wave_lane();
  const i64 wave = ((i64)blockIdx.x * BLOCK + threadIdx.x) / WAVE;
  const i64 nwaves = (i64)gridDim.x * (BLOCK / WAVE);
  unsigned long long inside = 0, odd = 0;
  for (i64 row = wave; row < nrows; row += nwaves) {
    const unsigned* __restrict__ tr = toggle + row * W;
    float* __restrict__ out = dst + row * nx;
    unsigned carry = 0;   // all ones when the words before this chunk hold an odd number of toggles
    for (int w0 = 0; w0 < W; w0 += WAVE) {
      const int wi = w0 + lane;
      unsigned x = wi < W ? tr[wi] : 0u;
      x ^= x << 1;
      x ^= x << 2;
      x ^= x << 4;
      x ^= x << 8;
      x ^= x << 16;
      const unsigned own = x >> 31;   // the parity of this lane's word
      // the parity of the words of lanes 0..lane
      const unsigned scan = wave_scan(own, lane, [](unsigned a, unsigned b) { return a ^ b; });
      x ^= ((scan ^ own) ? ~0u : 0u) ^ carry;
      carry ^= __shfl(scan, WAVE - 1, WAVE) ? ~0u : 0u;
      // x: bit b says whether sample 32 wi + b is inside
      const int left = nx - 32 * wi;   // samples of the row from this word on
      if (left > 0) inside += __popc(left >= 32 ? x : (x & ((1u << left) - 1u)));
      if (wi == (nx >> 5)) odd += (x >> (nx & 31)) & 1u;
      const int vox0 = 32 * w0;
      if (VEC) {
        for (int it = 0; it < 8; it++) {
          if (vox0 + it * 256 >= nx) break;
          const int v = vox0 + it * 256 + 4 * lane;
          const unsigned word = __shfl(x, it * 8 + (lane >> 3), WAVE);
          if (v < nx) {
            const unsigned nib = word >> (4 * (lane & 7));
            float4 f;
            f.x = (nib & 1u) ? 1.0f : 0.0f;
            f.y = (nib & 2u) ? 1.0f : 0.0f;
            f.z = (nib & 4u) ? 1.0f : 0.0f;
            f.w = (nib & 8u) ? 1.0f : 0.0f;
            *reinterpret_cast<float4*>(out + v) = f;
          }
        }
      } else {
        for (int it = 0; it < 32; it++) {
          if (vox0 + it * 64 >= nx) break;
          const int v = vox0 + it * 64 + lane;
          const unsigned word = __shfl(x, it * 2 + (lane >> 5), WAVE);
          if (v < nx) out[v] = ((word >> (lane & 31)) & 1u) ? 1.0f : 0.0f;
        }
      }
    }
  }
  wave_count(odd, counters + 1);   // rows and word chunks are the wave's: every lane has left the loops
  wave_count(inside, counters + 2);
}

// ---- host: quantisation, the edge census, the plan -------------------------------------------------------------------

int quantize_host(const float* v, i64 n, double w, const double* origin, int32_t* q) {
  VH_REQUIRE(n >= 0 && (n == 0 || v) && origin && (n == 0 || q), "voxelize: bad vertex list");
  VH_REQUIRE(w != 0.0 && std::isfinite(w), "voxelize: the voxel width is zero or not finite");
  for (i64 i = 0; i < 3 * n; i++) {
    VH_REQUIRE(std::isfinite(v[i]), "voxelize: a vertex is not finite");
    double t = (double)v[i] / w;
    t = t - origin[i % 3];
    t = t * 1024.0;
    const double r = std::nearbyint(t);
    VH_REQUIRE(std::fabs(r) <= (double)QMAX, "voxelize: a vertex lies more than 2^19 voxels from voxel 0");
    q[i] = (int32_t)r;
  }
  return VISFD_HIP_OK;
}

int check_indices(const int32_t* tri, i64 m, i64 n) {
  VH_REQUIRE(m >= 0 && (m == 0 || tri) && n >= 0 && n <= 2147483647LL, "voxelize: bad triangle list");
  for (i64 i = 0; i < 3 * m; i++)
    VH_REQUIRE(tri[i] >= 0 && (i64)tri[i] < n, "voxelize: a triangle index is out of range");
  return VISFD_HIP_OK;
}

int edges_host(const int32_t* tri, i64 m, i64 n, i64* boundary, i64* nonmanifold) {
  VH_TRY(check_indices(tri, m, n));
  std::vector<uint64_t> keys((size_t)(3 * m));
  for (i64 t = 0; t < m; t++)
    for (int e = 0; e < 3; e++) {
      const uint32_t a = (uint32_t)tri[3 * t + e], b = (uint32_t)tri[3 * t + (e + 1) % 3];
      keys[(size_t)(3 * t + e)] = a < b ? ((uint64_t)a << 32) | b : ((uint64_t)b << 32) | a;
    }
  std::sort(keys.begin(), keys.end());
  i64 nb = 0, nn = 0;
  for (size_t i = 0; i < keys.size();) {
    size_t j = i + 1;
    while (j < keys.size() && keys[j] == keys[i]) j++;
    if (j - i == 1) nb++;
    else if (j - i > 2) nn++;
    i = j;
  }
  if (boundary) *boundary = nb;
  if (nonmanifold) *nonmanifold = nn;
  return VISFD_HIP_OK;
}

inline size_t align8(size_t b) { return (b + 7) & ~(size_t)7; }

struct MeshArgs {
  const float* vertices;
  i64 n;
  const int32_t* triangles;
  i64 m;
  double w;
  const double* origin;
  i64 nx, ny, nz;
  bool check_closed;
};

// everything that can be refused is refused here, before the device is touched; `q` receives the quantised vertices
int check_mesh(const visfd_hip_ctx* ctx, const MeshArgs& a, const float* dst, std::vector<int32_t>* q) {
  VH_REQUIRE(ctx && dst && a.origin, "null argument");
  VH_TRY(check_dims(a.nx, a.ny, a.nz));
  VH_TRY(check_dims32(a.nx, a.ny, a.nz));
  VH_REQUIRE(a.nx < MAX_NX, "voxelize: nx must be below 2^19");
  VH_REQUIRE(a.nx * a.ny < MAX_VOXELS && a.nx * a.ny * a.nz < MAX_VOXELS, "voxelize: the image must have fewer than 2^31 voxels");
  VH_REQUIRE(a.n >= 0 && a.n <= 2147483647LL && (a.n == 0 || a.vertices), "voxelize: bad vertex list");
  q->resize((size_t)(3 * a.n));
  VH_TRY(quantize_host(a.vertices, a.n, a.w, a.origin, q->data()));
  VH_TRY(check_indices(a.triangles, a.m, a.n));
  if (a.check_closed) {
    i64 nb = 0, nn = 0;
    VH_TRY(edges_host(a.triangles, a.m, a.n, &nb, &nn));
    if (nb || nn)
      return fail(VISFD_HIP_EINVAL, "voxelize: the surface is not closed and manifold: " + std::to_string(nb) +
                                        " boundary edges, " + std::to_string(nn) + " non-manifold edges");
  }
  return VISFD_HIP_OK;
}

int voxelize(visfd_hip_ctx* ctx, const MeshArgs& a, const std::vector<int32_t>& q, float* dst) {
  VH_HIP(hipSetDevice(ctx->device));
  const int nx = (int)a.nx, ny = (int)a.ny, nz = (int)a.nz;
  const i64 nrows = a.ny * a.nz;
  const int W = (nx + 1 + 31) / 32;

  // the plan: the triangles no ray can cross, and those whose boxes are cut into tiles
  i64 skipped = 0;
  std::vector<int> tiled_id;
  std::vector<i64> item_end;
  i64 nitems = 0;
  for (i64 t = 0; t < a.m; t++) {
    const int* A = &q[3 * (size_t)a.triangles[3 * t]];
    const int* B = &q[3 * (size_t)a.triangles[3 * t + 1]];
    const int* C = &q[3 * (size_t)a.triangles[3 * t + 2]];
    if (area2_of(A, B, C) == 0) {
      skipped++;
      continue;
    }
    const RowBox r = row_box(A, B, C, ny, nz);
    if (box_rows(r) <= SMALL_ROWS) continue;
    nitems += (i64)((r.y1 - r.y0 + TILE) / TILE) * ((r.z1 - r.z0 + TILE) / TILE);
    tiled_id.push_back((int)t);
    item_end.push_back(nitems);
  }

  const size_t ntiled = tiled_id.size();
  const size_t off_tri = align8(sizeof(int) * q.size());
  const size_t off_id = off_tri + align8(sizeof(int) * 3 * (size_t)a.m);
  const size_t off_end = off_id + align8(sizeof(int) * ntiled);
  const size_t off_cnt = off_end + sizeof(i64) * ntiled;
  char* tab = nullptr;
  unsigned* toggle = nullptr;
  VH_TRY(ws(ctx, WS_VOX_MESH, off_cnt + 3 * sizeof(unsigned long long), &tab));
  VH_TRY(ws(ctx, WS_VOX_TOGGLE, (size_t)nrows * W, &toggle));
  int* dq = reinterpret_cast<int*>(tab);
  int* dtri = reinterpret_cast<int*>(tab + off_tri);
  int* did = reinterpret_cast<int*>(tab + off_id);
  i64* dend = reinterpret_cast<i64*>(tab + off_end);
  unsigned long long* counters = reinterpret_cast<unsigned long long*>(tab + off_cnt);

  PhaseClock<3> clock;   // option voxelize_time
  if (a.m > 0) {
    VH_HIP(hipMemcpyAsync(dq, q.data(), sizeof(int) * q.size(), hipMemcpyHostToDevice, ctx->stream));
    VH_HIP(hipMemcpyAsync(dtri, a.triangles, sizeof(int) * 3 * (size_t)a.m, hipMemcpyHostToDevice, ctx->stream));
  }
  if (ntiled) {
    VH_HIP(hipMemcpyAsync(did, tiled_id.data(), sizeof(int) * ntiled, hipMemcpyHostToDevice, ctx->stream));
    VH_HIP(hipMemcpyAsync(dend, item_end.data(), sizeof(i64) * ntiled, hipMemcpyHostToDevice, ctx->stream));
  }
  VH_HIP(hipMemsetAsync(counters, 0, 3 * sizeof(unsigned long long), ctx->stream));
  clock.start(ctx->stream, ctx->opt.voxelize_time != 0);
  VH_HIP(hipMemsetAsync(toggle, 0, sizeof(unsigned) * (size_t)nrows * W, ctx->stream));
  clock.mark(1);
  const i64 cap = (i64)ctx->num_cus * 64;
  const bool bisect = ctx->opt.voxelize_bisect != 0;   // tests: k never from the estimate
  if (a.m > 0) {
    scatter_small_kernel<<<dim3(grid_for(a.m, BLOCK, cap)), dim3(BLOCK), 0, ctx->stream>>>(dq, dtri, a.m, nx, ny, nz, W, bisect,
                                                                                          toggle, counters);
    VH_HIP(hipGetLastError());
  }
  if (nitems > 0) {
    scatter_tiled_kernel<<<dim3(grid_for(nitems, BLOCK / WAVE, cap)), dim3(BLOCK), 0, ctx->stream>>>(
        dq, dtri, did, dend, (int)ntiled, nitems, nx, ny, nz, W, bisect, toggle, counters);
    VH_HIP(hipGetLastError());
  }
  clock.mark(2);
  const unsigned grows = grid_for(nrows, BLOCK / WAVE, cap);
  if (nx % 4 == 0 && reinterpret_cast<uintptr_t>(dst) % 16 == 0)
    fill_kernel<true><<<dim3(grows), dim3(BLOCK), 0, ctx->stream>>>(toggle, dst, nx, nrows, W, counters);
  else
    fill_kernel<false><<<dim3(grows), dim3(BLOCK), 0, ctx->stream>>>(toggle, dst, nx, nrows, W, counters);
  VH_HIP(hipGetLastError());
  clock.mark(3);
  unsigned long long c[3] = {0, 0, 0};
  VH_HIP(hipMemcpyAsync(c, counters, sizeof(c), hipMemcpyDeviceToHost, ctx->stream));
  VH_HIP(hipStreamSynchronize(ctx->stream));
  if (clock.on) clock.read(ctx->voxelize_ms);
  ctx->voxelize_stats[0] = (int64_t)c[0];
  ctx->voxelize_stats[1] = skipped;
  ctx->voxelize_stats[2] = (int64_t)c[1];
  ctx->voxelize_stats[3] = (int64_t)c[2];
  return VISFD_HIP_OK;
}

}  // namespace
}  // namespace vh

using namespace vh;

extern "C" {

int visfd_hip_voxelize_mesh_dev(visfd_hip_ctx* ctx, const float* vertices, int64_t n_vertices, const int32_t* triangles,
                                int64_t n_triangles, double voxel_width, const double origin[3], int64_t nx, int64_t ny,
                                int64_t nz, int check_closed, float* dst) {
  const MeshArgs a = {vertices, n_vertices, triangles, n_triangles, voxel_width, origin, nx, ny, nz, check_closed != 0};
  std::vector<int32_t> q;
  VH_TRY(check_mesh(ctx, a, dst, &q));
  return voxelize(ctx, a, q, dst);
}

int visfd_hip_voxelize_mesh(visfd_hip_ctx* ctx, const float* vertices, int64_t n_vertices, const int32_t* triangles,
                            int64_t n_triangles, double voxel_width, const double origin[3], int64_t nx, int64_t ny,
                            int64_t nz, int check_closed, float* dst) {
  const MeshArgs a = {vertices, n_vertices, triangles, n_triangles, voxel_width, origin, nx, ny, nz, check_closed != 0};
  std::vector<int32_t> q;
  VH_TRY(check_mesh(ctx, a, dst, &q));
  VH_HIP(hipSetDevice(ctx->device));
  const Stage st = {ctx, (size_t)(nx * ny * nz)};
  float* dd = nullptr;
  VH_TRY(st.out(WS_H2D_2, &dd));
  VH_TRY(voxelize(ctx, a, q, dd));
  return st.down(dst, dd);
}

int visfd_hip_voxelize_last(visfd_hip_ctx* ctx, int64_t stats[4]) {
  VH_REQUIRE(ctx && stats, "null argument");
  for (int k = 0; k < 4; k++) stats[k] = ctx->voxelize_stats[k];
  return VISFD_HIP_OK;
}

int visfd_hip_voxelize_last_times(visfd_hip_ctx* ctx, float ms[3]) {
  VH_REQUIRE(ctx && ms, "null argument");
  for (int k = 0; k < 3; k++) ms[k] = ctx->voxelize_ms[k];
  return VISFD_HIP_OK;
}

int visfd_hip_voxelize_quantize_host(const float* vertices, int64_t n_vertices, double voxel_width, const double origin[3],
                                     int32_t* q) {
  return quantize_host(vertices, n_vertices, voxel_width, origin, q);
}

int visfd_hip_mesh_edges_host(const int32_t* triangles, int64_t n_triangles, int64_t n_vertices, int64_t* boundary_edges,
                              int64_t* nonmanifold_edges) {
  return edges_host(triangles, n_triangles, n_vertices, boundary_edges, nonmanifold_edges);
}

}  // extern "C"
