// isosurface.hip -- the closed triangle mesh of {v < iso} or {v > iso} of a volume: marching tetrahedra on the Kuhn split of
// every grid cell, the image surrounded by one layer of outside nodes (definition: include/visfd_hip.h).
//
//   classify   one lane per lower node (the cells' lower corners, -1 .. n - 1 per axis, in key order): the insideness of the
//              cell's 8 corners as one byte.  A lane tests the 4 nodes of its own x column and takes the column at x + 1 from
//              the next lane by a shuffle (the wave's last lane tests it itself); the crossing edges that start at the node
//              and the cell's triangle count follow from the byte.  Counts per workgroup chunk, reduced with csrc/wave.hpp.
//   scan       one workgroup: the chunks' vertex and triangle offsets, the totals.  The host reads the totals here.
//   vertices   every node's first vertex id (chunk offset + prefix within the workgroup) and its vertices.
//   triangles  per cell and tet the polygon of its case from a table; a vertex id is first[a] + the set bits of a's mask
//              below the edge's class.
// Nothing is placed with an atomic: two calls write the same bytes.  The host walk (visfd_hip_isosurface_host) runs the same
// statements (node_inside, edge_vertex, the tables) serially; the build's -ffp-contract=off keeps the one double add of a
// coordinate apart from the division before it.
#include <cmath>
#include <mutex>
#include <vector>

#include "common.hpp"
#include "wave.hpp"

namespace vh {
namespace {

constexpr int BLOCK = 256;
constexpr int ROUNDS = 4;                  // a workgroup takes ROUNDS x BLOCK consecutive keys
constexpr int CHUNK = BLOCK * ROUNDS;
constexpr int SCAN_BLOCK = 1024;
constexpr i64 MAX_VERTICES = 2147483647LL;

// Corner b (0..7) of a cell, as the bit of its code: 0 is the lower node a, b = k + 1 is a + dir_k with the 7 edge
// directions (1,0,0) (0,1,0) (0,0,1) (1,1,0) (0,1,1) (1,0,1) (1,1,1).  Bit b of these says whether the corner has x, y, z + 1.
constexpr unsigned CORNER_X = 0xD2, CORNER_Y = 0xB4, CORNER_Z = 0xE8;

struct Tables {
  // per tet and case (bit p: corner p of the tet is inside): bits 0-1 the triangles, then 6 bits per polygon vertex: the code
  // bit of the edge's lower end (3 bits) and the edge's class (3 bits)
  unsigned poly[6][16];
  unsigned char ntri[256];       // triangles of a cell, by its code
  unsigned char corner[6][4];    // code bit of a tet's corner
};

int bit_of(const int o[3]) {
  for (int b = 0; b < 8; b++)
    if ((int)((CORNER_X >> b) & 1) == o[0] && (int)((CORNER_Y >> b) & 1) == o[1] && (int)((CORNER_Z >> b) & 1) == o[2]) return b;
  return -1;
}

void build_tables(Tables* T) {
  static const int PERM[6][3] = {{0, 1, 2}, {0, 2, 1}, {1, 0, 2}, {1, 2, 0}, {2, 0, 1}, {2, 1, 0}};
  for (int t = 0; t < 6; t++) {
    int off[4][3] = {};
    for (int p = 1; p < 4; p++) {
      for (int d = 0; d < 3; d++) off[p][d] = off[p - 1][d];
      off[p][PERM[t][p - 1]] += 1;
    }
    for (int p = 0; p < 4; p++) T->corner[t][p] = (unsigned char)bit_of(off[p]);
    for (int c = 0; c < 16; c++) {
      int I[4], O[4], ni = 0, no = 0;
      for (int p = 0; p < 4; p++) {
        if ((c >> p) & 1) I[ni++] = p; else O[no++] = p;
      }
      T->poly[t][c] = 0;
      if (ni == 0 || no == 0) continue;
      int e[4][2], n = 0;   // (inside corner, outside corner)
      if (ni == 1) {
        for (int k = 0; k < no; k++) { e[n][0] = I[0]; e[n][1] = O[k]; n++; }
      } else if (ni == 3) {
        for (int k = 0; k < ni; k++) { e[n][0] = I[k]; e[n][1] = O[0]; n++; }
      } else {
        const int q[4][2] = {{I[0], O[0]}, {I[0], O[1]}, {I[1], O[1]}, {I[1], O[0]}};
        for (int k = 0; k < 4; k++) { e[k][0] = q[k][0]; e[k][1] = q[k][1]; }
        n = 4;
      }
      // twice the edge midpoints; (P1 - P0) x (P2 - P0) against no * sum(I) - ni * sum(O), a positive multiple of the
      // vector from the outside corners' mean to the inside corners' mean
      int P[3][3], toin[3];
      for (int k = 0; k < 3; k++)
        for (int d = 0; d < 3; d++) P[k][d] = off[e[k][0]][d] + off[e[k][1]][d];
      for (int d = 0; d < 3; d++) {
        int si = 0, so = 0;
        for (int k = 0; k < ni; k++) si += off[I[k]][d];
        for (int k = 0; k < no; k++) so += off[O[k]][d];
        toin[d] = no * si - ni * so;
      }
      const int u[3] = {P[1][0] - P[0][0], P[1][1] - P[0][1], P[1][2] - P[0][2]};
      const int w[3] = {P[2][0] - P[0][0], P[2][1] - P[0][1], P[2][2] - P[0][2]};
      const int nrm[3] = {u[1] * w[2] - u[2] * w[1], u[2] * w[0] - u[0] * w[2], u[0] * w[1] - u[1] * w[0]};
      const bool reverse = nrm[0] * toin[0] + nrm[1] * toin[1] + nrm[2] * toin[2] > 0;
      unsigned word = (unsigned)(n - 2);
      for (int k = 0; k < n; k++) {
        const int* ed = e[reverse ? n - 1 - k : k];
        const int lo = ed[0] < ed[1] ? ed[0] : ed[1], hi = ed[0] < ed[1] ? ed[1] : ed[0];
        const int diff[3] = {off[hi][0] - off[lo][0], off[hi][1] - off[lo][1], off[hi][2] - off[lo][2]};
        const unsigned enc = (unsigned)T->corner[t][lo] | ((unsigned)(bit_of(diff) - 1) << 3);
        word |= enc << (2 + 6 * k);
      }
      T->poly[t][c] = word;
    }
  }
  for (int code = 0; code < 256; code++) {
    int n = 0;
    for (int t = 0; t < 6; t++) {
      int c = 0;
      for (int p = 0; p < 4; p++) c |= ((code >> T->corner[t][p]) & 1) << p;
      n += (int)(T->poly[t][c] & 3u);
    }
    T->ntri[code] = (unsigned char)n;
  }
}

const Tables& tables() {
  static Tables T;
  static std::once_flag once;
  std::call_once(once, [] { build_tables(&T); });
  return T;
}

struct Grid {
  const float* vol;
  int nx, ny, nz;
  i64 rx, rxy;   // lower nodes per row (nx + 1) and per plane
  i64 nl;        // lower nodes
  double iso;
  int side;
};

Grid make_grid(const float* vol, i64 nx, i64 ny, i64 nz, double iso, int side) {
  Grid g;
  g.vol = vol;
  g.nx = (int)nx; g.ny = (int)ny; g.nz = (int)nz;
  g.rx = nx + 1;
  g.rxy = (nx + 1) * (ny + 1);
  g.nl = g.rxy * (nz + 1);
  g.iso = iso;
  g.side = side;
  return g;
}

__host__ __device__ inline bool node_inside(float v, double iso, int side) {   // a NaN fails both comparisons
  const double d = (double)v;
  return side == VISFD_HIP_ISO_BELOW ? d < iso : d > iso;
}
__host__ __device__ inline bool in_image(const Grid& g, int x, int y, int z) {
  return x >= 0 && x < g.nx && y >= 0 && y < g.ny && z >= 0 && z < g.nz;
}
__host__ __device__ inline bool inside_at(const Grid& g, int x, int y, int z) {   // border nodes are outside
  if (!in_image(g, x, y, z)) return false;
  return node_inside(g.vol[((i64)z * g.ny + y) * g.nx + x], g.iso, g.side);
}
// the nodes (x, y, z), (x, y + 1, z), (x, y, z + 1), (x, y + 1, z + 1) as bits 0..3
__host__ __device__ inline unsigned column_at(const Grid& g, int x, int y, int z) {
  if (x < 0 || x >= g.nx) return 0u;
  return (inside_at(g, x, y, z) ? 1u : 0u) | (inside_at(g, x, y + 1, z) ? 2u : 0u) | (inside_at(g, x, y, z + 1) ? 4u : 0u) |
         (inside_at(g, x, y + 1, z + 1) ? 8u : 0u);
}
// the cell's code from the columns at a_x and a_x + 1
__host__ __device__ inline unsigned code_of(unsigned mine, unsigned next) {
  return (mine & 1u) | ((next & 1u) << 1) | ((mine & 2u) << 1) | ((mine & 4u) << 1) | ((next & 2u) << 3) | ((mine & 8u) << 2) |
         ((next & 4u) << 4) | ((next & 8u) << 4);
}
// the edges that start at the lower node and cross the surface, bit = class
__host__ __device__ inline unsigned mask_of(unsigned code) { return ((code >> 1) ^ (0u - (code & 1u))) & 0x7Fu; }
__host__ __device__ inline void node_of(const Grid& g, i64 key, int* ax, int* ay, int* az) {
  *ax = (int)(key % g.rx) - 1;
  *ay = (int)((key / g.rx) % (g.ny + 1)) - 1;
  *az = (int)(key / g.rxy) - 1;
}
__host__ __device__ inline bool on_image_face(const Grid& g, int x, int y, int z) {
  return x == 0 || x == g.nx - 1 || y == 0 || y == g.ny - 1 || z == 0 || z == g.nz - 1;
}

// the vertex on the edge of class cls from node (ax, ay, az)
__host__ __device__ inline void edge_vertex(const Grid& g, int ax, int ay, int az, int cls, float out[3]) {
  const int dx = (int)((CORNER_X >> (cls + 1)) & 1), dy = (int)((CORNER_Y >> (cls + 1)) & 1), dz = (int)((CORNER_Z >> (cls + 1)) & 1);
  double t = 0.5;
  if (in_image(g, ax, ay, az) && in_image(g, ax + dx, ay + dy, az + dz)) {
    const double va = (double)g.vol[((i64)az * g.ny + ay) * g.nx + ax];
    const double vb = (double)g.vol[((i64)(az + dz) * g.ny + (ay + dy)) * g.nx + (ax + dx)];
    t = (g.iso - va) / (vb - va);
    if (!__builtin_isfinite(t)) t = 0.5;
    if (t < 1.0 / 64.0) t = 1.0 / 64.0;
    if (t > 63.0 / 64.0) t = 63.0 / 64.0;
  }
  out[0] = dx ? (float)((double)ax + t) : (float)ax;
  out[1] = dy ? (float)((double)ay + t) : (float)ay;
  out[2] = dz ? (float)((double)az + t) : (float)az;
}

// a cell's triangles in order (tet, first / second); `lookup(key, cls)` is the id of the vertex on that edge
template <typename Lookup>
__host__ __device__ inline void cell_triangles(const Grid& g, const unsigned* poly, const unsigned char* corner, unsigned code,
                                               i64 key, int32_t* out, Lookup lookup) {
  for (int t = 0; t < 6; t++) {
    unsigned c = 0;
    for (int p = 0; p < 4; p++) c |= ((code >> corner[4 * t + p]) & 1u) << p;
    const unsigned word = poly[16 * t + c];
    const int k = (int)(word & 3u);
    if (k == 0) continue;
    int32_t id[4] = {0, 0, 0, 0};
    for (int j = 0; j < k + 2; j++) {
      const unsigned enc = (word >> (2 + 6 * j)) & 63u;
      const unsigned b = enc & 7u;
      const i64 nkey = key + (i64)((CORNER_Z >> b) & 1) * g.rxy + (i64)((CORNER_Y >> b) & 1) * g.rx + (i64)((CORNER_X >> b) & 1);
      id[j] = lookup(nkey, (int)(enc >> 3));
    }
    out[0] = id[0]; out[1] = id[1]; out[2] = id[2];
    out += 3;
    if (k == 2) {
      out[0] = id[0]; out[1] = id[2]; out[2] = id[3];
      out += 3;
    }
  }
}

// ---- kernels -----------------------------------------------------------------------------------------------------------------
// code[key]; chunk[b] = (vertices, triangles, inside nodes, 1 if an inside node lies on a face of the image) of workgroup b
__global__ void __launch_bounds__(BLOCK)
classify_kernel(Grid g, const Tables* __restrict__ tab, unsigned char* __restrict__ code, uint4* __restrict__ chunk) {
  __shared__ unsigned char s_ntri[256];
  __shared__ unsigned wsum[4][BLOCK / WAVE];
  s_ntri[threadIdx.x] = tab->ntri[threadIdx.x];   // BLOCK == 256
  __syncthreads();
  const int lane = wave_lane();
  unsigned nv = 0, nt = 0, nin = 0, cap = 0;
  for (int r = 0; r < ROUNDS; r++) {   // uniform bounds: the wave stays whole for the shuffle, idle lanes hold 0
    const i64 key = ((i64)blockIdx.x * ROUNDS + r) * BLOCK + threadIdx.x;
    const bool live = key < g.nl;
    int ax = 0, ay = 0, az = 0;
    unsigned mine = 0;
    if (live) {
      node_of(g, key, &ax, &ay, &az);
      mine = column_at(g, ax, ay, az);
    }
    unsigned next = __shfl_down(mine, 1, WAVE);   // lane + 1 holds key + 1: the node at x + 1 unless this one ends its row
    if (live) {
      if (ax == g.nx - 1) next = 0;   // x + 1 is a border node
      else if (lane == WAVE - 1) next = column_at(g, ax + 1, ay, az);
      const unsigned c = code_of(mine, next);
      code[key] = (unsigned char)c;
      nv += (unsigned)__popc(mask_of(c));
      nt += s_ntri[c];
      nin += c & 1u;
      if ((c & 1u) && on_image_face(g, ax, ay, az)) cap = 1;
    }
  }
  nv = wave_sum(nv);
  nt = wave_sum(nt);
  nin = wave_sum(nin);
  cap = wave_or(cap);
  if (lane == 0) {
    const int w = threadIdx.x / WAVE;
    wsum[0][w] = nv; wsum[1][w] = nt; wsum[2][w] = nin; wsum[3][w] = cap;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    uint4 s = make_uint4(0, 0, 0, 0);
    for (int w = 0; w < BLOCK / WAVE; w++) { s.x += wsum[0][w]; s.y += wsum[1][w]; s.z += wsum[2][w]; s.w |= wsum[3][w]; }
    chunk[blockIdx.x] = s;
  }
}

// one workgroup: off[b] = (vertices, triangles) before chunk b; totals = vertices, triangles, inside nodes, cap flag
__global__ void __launch_bounds__(SCAN_BLOCK)
scan_kernel(const uint4* __restrict__ chunk, i64 nchunks, ulonglong2* __restrict__ off, unsigned long long* __restrict__ totals) {
  __shared__ unsigned wtot[4][SCAN_BLOCK / WAVE];
  const int lane = wave_lane(), wave = threadIdx.x / WAVE;
  unsigned long long carry_v = 0, carry_t = 0, carry_in = 0;
  unsigned any_cap = 0;
  for (i64 t0 = 0; t0 < nchunks; t0 += SCAN_BLOCK) {
    const i64 b = t0 + threadIdx.x;
    const uint4 c = b < nchunks ? chunk[b] : make_uint4(0, 0, 0, 0);   // at most 12 CHUNK each: a tile's sum fits 32 bits
    const unsigned iv = wave_scan(c.x, lane), it = wave_scan(c.y, lane);
    const unsigned in = wave_sum(c.z), cp = wave_or(c.w);
    if (lane == WAVE - 1) { wtot[0][wave] = iv; wtot[1][wave] = it; wtot[2][wave] = in; wtot[3][wave] = cp; }
    __syncthreads();
    unsigned before_v = 0, before_t = 0, tile_v = 0, tile_t = 0, tile_in = 0;
    for (int w = 0; w < SCAN_BLOCK / WAVE; w++) {
      if (w < wave) { before_v += wtot[0][w]; before_t += wtot[1][w]; }
      tile_v += wtot[0][w]; tile_t += wtot[1][w]; tile_in += wtot[2][w];
      any_cap |= wtot[3][w];
    }
    if (b < nchunks) off[b] = make_ulonglong2(carry_v + before_v + (iv - c.x), carry_t + before_t + (it - c.y));
    carry_v += tile_v; carry_t += tile_t; carry_in += tile_in;
    __syncthreads();
  }
  if (threadIdx.x == 0) { totals[0] = carry_v; totals[1] = carry_t; totals[2] = carry_in; totals[3] = any_cap; }
}

// exclusive prefix of v over the workgroup's lanes; *total: the workgroup's sum.  Every lane of the workgroup calls.
__device__ __forceinline__ unsigned block_prefix(unsigned v, unsigned* wtot, unsigned* total) {
  const int lane = wave_lane(), wave = threadIdx.x / WAVE;
  const unsigned incl = wave_scan(v, lane);
  if (lane == WAVE - 1) wtot[wave] = incl;
  __syncthreads();
  unsigned before = 0, all = 0;
  for (int w = 0; w < BLOCK / WAVE; w++) {
    if (w < wave) before += wtot[w];
    all += wtot[w];
  }
  __syncthreads();   // wtot is free again
  *total = all;
  return before + (incl - v);
}

// first[key] for every lower node; with verts, the vertices (fewer than 2^31: the host has checked the total)
__global__ void __launch_bounds__(BLOCK)
vertices_kernel(Grid g, const unsigned char* __restrict__ code, const ulonglong2* __restrict__ off, int32_t* __restrict__ first,
                float* __restrict__ verts) {
  __shared__ unsigned wtot[BLOCK / WAVE];
  i64 base = (i64)off[blockIdx.x].x;
  for (int r = 0; r < ROUNDS; r++) {
    const i64 key = ((i64)blockIdx.x * ROUNDS + r) * BLOCK + threadIdx.x;
    const bool live = key < g.nl;
    unsigned m = live ? mask_of(code[key]) : 0u;
    unsigned total;
    i64 pos = base + block_prefix((unsigned)__popc(m), wtot, &total);
    base += total;
    if (!live) continue;   // no wave-level call below
    first[key] = (int32_t)pos;
    if (!verts || !m) continue;
    int ax, ay, az;
    node_of(g, key, &ax, &ay, &az);
    while (m) {
      const int cls = __ffs((int)m) - 1;
      m &= m - 1;
      float p[3];
      edge_vertex(g, ax, ay, az, cls, p);
      verts[3 * pos] = p[0];
      verts[3 * pos + 1] = p[1];
      verts[3 * pos + 2] = p[2];
      pos++;
    }
  }
}

__global__ void __launch_bounds__(BLOCK)
triangles_kernel(Grid g, const Tables* __restrict__ tab, const unsigned char* __restrict__ code, const int32_t* __restrict__ first,
                 const ulonglong2* __restrict__ off, int32_t* __restrict__ tris) {
  __shared__ unsigned s_poly[96];
  __shared__ unsigned char s_corner[24];
  __shared__ unsigned char s_ntri[256];
  __shared__ unsigned wtot[BLOCK / WAVE];
  if (threadIdx.x < 96) s_poly[threadIdx.x] = tab->poly[threadIdx.x / 16][threadIdx.x % 16];
  if (threadIdx.x < 24) s_corner[threadIdx.x] = tab->corner[threadIdx.x / 4][threadIdx.x % 4];
  s_ntri[threadIdx.x] = tab->ntri[threadIdx.x];
  __syncthreads();
  i64 base = (i64)off[blockIdx.x].y;
  for (int r = 0; r < ROUNDS; r++) {
    const i64 key = ((i64)blockIdx.x * ROUNDS + r) * BLOCK + threadIdx.x;
    const bool live = key < g.nl;
    const unsigned c = live ? code[key] : 0u;
    const unsigned n = s_ntri[c];   // 0 for an idle lane's code 0
    unsigned total;
    const i64 pos = base + block_prefix(n, wtot, &total);
    base += total;
    if (!n) continue;
    // an edge that crosses has its lower end among the lower nodes (a border node beyond them has only border nodes above
    // it), so nkey < nl; the test keeps a wrong table from reading outside the arrays
    cell_triangles(g, s_poly, s_corner, c, key, tris + 3 * pos, [&](i64 nkey, int cls) -> int32_t {
      if (nkey >= g.nl) return 0;
      return first[nkey] + (int32_t)__popc(mask_of(code[nkey]) & ((1u << cls) - 1u));
    });
  }
}

// ---- orchestration -----------------------------------------------------------------------------------------------------------
struct Call {
  i64 nx, ny, nz;
  double iso;
  int side;
  float* verts;      // device or host memory, by the face
  i64 vcap;
  int32_t* tris;
  i64 tcap;
  int64_t *nv, *nt;
};

int check_call(const float* vol, const Call& a) {
  VH_REQUIRE(vol && a.nv && a.nt, "isosurface: null argument");
  VH_REQUIRE(a.nx >= 1 && a.ny >= 1 && a.nz >= 1, "isosurface: every dimension must be at least 1");
  VH_REQUIRE(a.nx < (1LL << 31) - 2 && a.ny < (1LL << 31) - 2 && a.nz < (1LL << 31) - 2, "isosurface: dimension too large");
  VH_REQUIRE(a.side == VISFD_HIP_ISO_BELOW || a.side == VISFD_HIP_ISO_ABOVE, "isosurface: unknown side");
  VH_REQUIRE(std::isfinite(a.iso), "isosurface: the level is not finite");
  VH_REQUIRE(a.vcap >= 0 && a.tcap >= 0, "isosurface: negative capacity");
  return VISFD_HIP_OK;
}

int too_many(i64 nv) {
  if (nv > MAX_VERTICES) return fail(VISFD_HIP_EINVAL, "isosurface: more than 2^31 - 1 vertices");
  return VISFD_HIP_OK;
}

// what the counts leave to do: *want_v / *want_t say which arrays get written, the return value what the call answers
int plan_outputs(const Call& a, i64 nv, i64 nt, bool* want_v, bool* want_t) {
  *a.nv = nv;
  *a.nt = nt;
  *want_v = a.verts && a.vcap >= nv;
  *want_t = a.tris && a.tcap >= nt;
  if ((a.verts && !*want_v) || (a.tris && !*want_t)) return fail(VISFD_HIP_ECAPACITY, "isosurface: an output array is too small");
  return VISFD_HIP_OK;
}

// vol on the device; the outputs on the device (host_out == false) or on the host
int run_device(visfd_hip_ctx* ctx, const float* vol, const Call& a, bool host_out) {
  const Grid g = make_grid(vol, a.nx, a.ny, a.nz, a.iso, a.side);
  const i64 nchunks = (g.nl + CHUNK - 1) / CHUNK;
  VH_REQUIRE(nchunks < (1LL << 31), "isosurface: image too large");
  static const char key[] = "isosurface tables 1";
  if (!ws_holds(ctx, WS_ISO_TAB, key, sizeof(key))) VH_TRY(ws_put(ctx, WS_ISO_TAB, key, sizeof(key), &tables(), sizeof(Tables)));
  const Tables* tab = static_cast<const Tables*>(ctx->slot_ptr[WS_ISO_TAB]);
  unsigned char* code = nullptr;
  char* aux = nullptr;
  VH_TRY(ws(ctx, WS_ISO_CODE, (size_t)g.nl, &code));
  VH_TRY(ws(ctx, WS_ISO_CHUNKS, (size_t)nchunks * (sizeof(uint4) + sizeof(ulonglong2)) + 32, &aux));
  ulonglong2* off = reinterpret_cast<ulonglong2*>(aux);
  uint4* chunk = reinterpret_cast<uint4*>(aux + (size_t)nchunks * sizeof(ulonglong2));
  unsigned long long* totals = reinterpret_cast<unsigned long long*>(aux + (size_t)nchunks * (sizeof(uint4) + sizeof(ulonglong2)));

  PhaseClock<4> clock;   // option isosurface_time
  for (int k = 0; k < 4; k++) ctx->isosurface_ms[k] = -1.0f;
  clock.start(ctx->stream, ctx->opt.isosurface_time != 0);
  classify_kernel<<<dim3((unsigned)nchunks), dim3(BLOCK), 0, ctx->stream>>>(g, tab, code, chunk);
  VH_HIP(hipGetLastError());
  clock.mark(1);
  scan_kernel<<<dim3(1), dim3(SCAN_BLOCK), 0, ctx->stream>>>(chunk, nchunks, off, totals);
  VH_HIP(hipGetLastError());
  unsigned long long tot[4] = {0, 0, 0, 0};
  VH_HIP(hipMemcpyAsync(tot, totals, sizeof(tot), hipMemcpyDeviceToHost, ctx->stream));
  clock.mark(2);
  VH_HIP(hipStreamSynchronize(ctx->stream));
  const i64 nv = (i64)tot[0], nt = (i64)tot[1];
  VH_TRY(too_many(nv));
  ctx->isosurface_last[0] = nv;
  ctx->isosurface_last[1] = nt;
  ctx->isosurface_last[2] = (i64)tot[2];
  ctx->isosurface_last[3] = (i64)tot[3];
  bool want_v, want_t;
  const int answer = plan_outputs(a, nv, nt, &want_v, &want_t);
  if (want_v || want_t) {
    float* dv = want_v ? a.verts : nullptr;
    int32_t* dt = want_t ? a.tris : nullptr;
    if (host_out) {
      char* out = nullptr;
      const size_t vbytes = want_v ? sizeof(float) * 3 * (size_t)nv : 0, tbytes = want_t ? sizeof(int32_t) * 3 * (size_t)nt : 0;
      VH_TRY(ws(ctx, WS_ISO_OUT, vbytes + tbytes, &out));
      dv = want_v ? reinterpret_cast<float*>(out) : nullptr;
      dt = want_t ? reinterpret_cast<int32_t*>(out + vbytes) : nullptr;
    }
    int32_t* first = nullptr;
    VH_TRY(ws(ctx, WS_ISO_FIRST, (size_t)g.nl, &first));
    clock.mark(2);   // again: the scan's phase ends after the host has read the totals and the buffers stand
    if (nv > 0) {   // without a vertex there is no triangle, and nobody reads first
      vertices_kernel<<<dim3((unsigned)nchunks), dim3(BLOCK), 0, ctx->stream>>>(g, code, off, first, dv);
      VH_HIP(hipGetLastError());
      clock.mark(3);
      if (dt) {
        triangles_kernel<<<dim3((unsigned)nchunks), dim3(BLOCK), 0, ctx->stream>>>(g, tab, code, first, off, dt);
        VH_HIP(hipGetLastError());
      }
    }
    clock.mark(4);
    if (host_out) {
      if (want_v && nv > 0) VH_HIP(hipMemcpyAsync(a.verts, dv, sizeof(float) * 3 * (size_t)nv, hipMemcpyDeviceToHost, ctx->stream));
      if (want_t && nt > 0) VH_HIP(hipMemcpyAsync(a.tris, dt, sizeof(int32_t) * 3 * (size_t)nt, hipMemcpyDeviceToHost, ctx->stream));
    }
    VH_HIP(hipStreamSynchronize(ctx->stream));
  }
  if (clock.on) clock.read(ctx->isosurface_ms);
  return answer;
}

}  // namespace
}  // namespace vh

using namespace vh;

extern "C" {

int visfd_hip_isosurface_host(const float* vol, int64_t nx, int64_t ny, int64_t nz, double iso, int side, float* vertices,
                              int64_t vertices_cap, int32_t* triangles, int64_t triangles_cap, int64_t* n_vertices,
                              int64_t* n_triangles) {
  const Call a = {nx, ny, nz, iso, side, vertices, vertices_cap, triangles, triangles_cap, n_vertices, n_triangles};
  VH_TRY(check_call(vol, a));
  const Grid g = make_grid(vol, nx, ny, nz, iso, side);
  const Tables& T = tables();
  std::vector<unsigned char> code((size_t)g.nl);
  i64 nv = 0, nt = 0;
  for (i64 key = 0; key < g.nl; key++) {
    int ax, ay, az;
    node_of(g, key, &ax, &ay, &az);
    const unsigned c = code_of(column_at(g, ax, ay, az), column_at(g, ax + 1, ay, az));
    code[(size_t)key] = (unsigned char)c;
    nv += __builtin_popcount(mask_of(c));
    nt += T.ntri[c];
  }
  VH_TRY(too_many(nv));
  bool want_v, want_t;
  const int answer = plan_outputs(a, nv, nt, &want_v, &want_t);
  if (!want_v && !want_t) return answer;
  std::vector<int32_t> first;
  if (want_t) first.resize((size_t)g.nl);
  i64 pos = 0;
  for (i64 key = 0; key < g.nl; key++) {
    unsigned m = mask_of(code[(size_t)key]);
    if (want_t) first[(size_t)key] = (int32_t)pos;
    if (!want_v) { pos += __builtin_popcount(m); continue; }
    int ax, ay, az;
    node_of(g, key, &ax, &ay, &az);
    for (; m; m &= m - 1) {
      edge_vertex(g, ax, ay, az, __builtin_ctz(m), vertices + 3 * pos);
      pos++;
    }
  }
  if (want_t) {
    int32_t* out = triangles;
    for (i64 key = 0; key < g.nl; key++) {
      const unsigned c = code[(size_t)key];
      if (!T.ntri[c]) continue;
      cell_triangles(g, &T.poly[0][0], &T.corner[0][0], c, key, out, [&](i64 nkey, int cls) -> int32_t {
        return first[(size_t)nkey] + (int32_t)__builtin_popcount(mask_of(code[(size_t)nkey]) & ((1u << cls) - 1u));
      });
      out += 3 * T.ntri[c];
    }
  }
  return answer;
}

int visfd_hip_isosurface(visfd_hip_ctx* ctx, const float* vol, int64_t nx, int64_t ny, int64_t nz, double iso, int side,
                         float* vertices, int64_t vertices_cap, int32_t* triangles, int64_t triangles_cap, int64_t* n_vertices,
                         int64_t* n_triangles) {
  const Call a = {nx, ny, nz, iso, side, vertices, vertices_cap, triangles, triangles_cap, n_vertices, n_triangles};
  VH_REQUIRE(ctx, "isosurface: null context");
  VH_TRY(check_call(vol, a));
  VH_HIP(hipSetDevice(ctx->device));
  const Stage st = {ctx, (size_t)(nx * ny * nz)};
  float* dvol;
  VH_TRY(st.up(WS_H2D_0, vol, &dvol));
  return run_device(ctx, dvol, a, true);
}

int visfd_hip_isosurface_dev(visfd_hip_ctx* ctx, const float* vol, int64_t nx, int64_t ny, int64_t nz, double iso, int side,
                             float* vertices, int64_t vertices_cap, int32_t* triangles, int64_t triangles_cap,
                             int64_t* n_vertices, int64_t* n_triangles) {
  const Call a = {nx, ny, nz, iso, side, vertices, vertices_cap, triangles, triangles_cap, n_vertices, n_triangles};
  VH_REQUIRE(ctx, "isosurface: null context");
  VH_TRY(check_call(vol, a));
  const size_t nbytes = sizeof(float) * (size_t)(nx * ny * nz);
  const size_t vbytes = sizeof(float) * 3 * (size_t)vertices_cap, tbytes = sizeof(int32_t) * 3 * (size_t)triangles_cap;
  VH_REQUIRE(!overlap_bytes(vol, nbytes, vertices, vbytes) && !overlap_bytes(vol, nbytes, triangles, tbytes),
             "isosurface: an output overlaps the volume");
  VH_REQUIRE(!overlap_bytes(vertices, vbytes, triangles, tbytes), "isosurface: the outputs overlap");
  VH_HIP(hipSetDevice(ctx->device));
  return run_device(ctx, vol, a, false);
}

int visfd_hip_isosurface_last(visfd_hip_ctx* ctx, int64_t stats[4]) {
  VH_REQUIRE(ctx && stats, "null argument");
  for (int k = 0; k < 4; k++) stats[k] = ctx->isosurface_last[k];
  return VISFD_HIP_OK;
}

int visfd_hip_isosurface_last_times(visfd_hip_ctx* ctx, float ms[4]) {
  VH_REQUIRE(ctx && ms, "null argument");
  for (int k = 0; k < 4; k++) ms[k] = ctx->isosurface_ms[k];
  return VISFD_HIP_OK;
}

}  // extern "C"
