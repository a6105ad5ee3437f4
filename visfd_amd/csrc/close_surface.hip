// close_surface.hip -- an oriented point cloud closed into a 0/1 image on the voxel grid (no reference
// counterpart: the reference's Example 3 leaves this step to SSDRecon / PoissonRecon, meshlab and voxelize_mesh.py), and its
// entry points.  include/visfd_hip.h states the definition; this is the grid form of Poisson surface reconstruction:
//   1. splat_kernel: the normals spread trilinearly into three int64 volumes (slot WS_CS_ACC) over the padded box, every
//      contribution an integer (2^-24 units) added with a 64-bit integer atomic, so the volumes do not depend on arrival order;
//   2. divergence_kernel: b = div V by central differences in float, V converted from the integers on the fly, and the
//      partial sums of b^2;
//   3. the solve of Laplace(chi) = b, chi = 0 outside the box: V(0,3) multigrid cycles in float32 with a damped Jacobi
//      smoother (jacobi_kernel), full weighting fused with the residual (resid_restrict_kernel: at the finest level it also
//      sums the residual's squares, which is the stopping test of the cycle before) and trilinear interpolation fused with
//      the correction (prolong_kernel).  An axis of n nodes is coarsened to floor(n / 2) nodes at the odd fine indices while
//      n >= 3, so any box works.  Where the far boundary then no longer lies a whole coarse spacing behind the last node, the
//      coarse operator takes the true distance (delta spacings: the Shortley-Weller form of the second difference); without
//      that the cycle diverges on boxes such as 48^3.  The coarsest level (every axis at most 2 nodes) gets 24 sweeps.
//   4. sample_kernel: chi interpolated at the used points, summed in double in a fixed order (block trees, then one block
//      over the partial sums: reduce_kernel), the level iso = sum / n_used;
//   5. face_kernel (orientation auto: the two candidate sets counted on the faces of the padded box) and cut_kernel.
// Nothing here adds floats with atomics and every float reduction has a fixed shape, so a call returns the same bits on
// every run.  The sweeps read and write 16 bytes per lane along x (rows are padded to a multiple of 4 floats, the slack
// kept at zero), march along z with the column's three planes in registers, take x neighbours from the adjacent lanes and
// y neighbours from rows the same workgroup has just read.  Index arithmetic is in i64.
#include <cfloat>
#include <cmath>
#include <vector>

#include "common.hpp"
#include "wave.hpp"

namespace vh {

namespace {

constexpr int BLOCK = 256;
constexpr int ROWS = BLOCK / WAVE;       // the sweeps: one wave per row, four rows per workgroup
constexpr int CTX = 32, CTY = 8;         // resid_restrict_kernel: the coarse tile of a workgroup
constexpr int POST_SWEEPS = 3;
constexpr int COARSEST_SWEEPS = 24;
constexpr float OMEGA = 0.857142857f;    // 6/7: the damping that smooths best for the 7-point operator
constexpr double SPLAT_SCALE = 16777216.0;       // 2^24
constexpr double SPLAT_UNSCALE = 1.0 / 16777216.0;
constexpr float NORMAL_MAX = 1073741824.0f;      // 2^30
constexpr i64 MAX_DIM = 65535;
constexpr int MAX_LEVELS = 20;

// the padded box and where the image sits in it
struct Box {
  i64 nx, ny, nz;   // the image
  i64 pad;
  i64 Nx, Ny, Nz;   // the box
};

// One used point: the low corner of its cell in the box and the fractions.
struct PointCell {
  i64 i[3];
  double f[3];
};

__host__ __device__ inline bool finite_f(float v) { return fabsf(v) <= FLT_MAX; }

__host__ __device__ inline bool point_cell(const float* p, const float* nrm, const Box& B, PointCell* c) {
  const i64 N[3] = {B.Nx, B.Ny, B.Nz};
  for (int d = 0; d < 3; d++)
    if (!finite_f(p[d]) || !finite_f(nrm[d]) || fabsf(nrm[d]) > NORMAL_MAX) return false;
  for (int d = 0; d < 3; d++) {
    const double pd = (double)p[d];
    const double fl = floor(pd);
    if (!(fl >= -(double)B.pad && fl + (double)B.pad + 1.0 <= (double)(N[d] - 1))) return false;
    c->i[d] = (i64)fl + B.pad;
    c->f[d] = pd - fl;
  }
  return true;
}

// the 24 integer contributions of a used point, corner by corner (z outermost), channel innermost
template <typename Add>
__host__ __device__ inline void splat_point(const PointCell& c, const float* nrm, const Box& B, Add add) {
  for (int cz = 0; cz < 2; cz++) {
    const double wz = cz ? c.f[2] : 1.0 - c.f[2];
    for (int cy = 0; cy < 2; cy++) {
      const double wy = cy ? c.f[1] : 1.0 - c.f[1];
      for (int cx = 0; cx < 2; cx++) {
        const double wx = cx ? c.f[0] : 1.0 - c.f[0];
        const double w = (wx * wy) * wz;
        const i64 node = ((c.i[2] + cz) * B.Ny + (c.i[1] + cy)) * B.Nx + (c.i[0] + cx);
        for (int d = 0; d < 3; d++) add(d, node, (long long)llrint((w * (double)nrm[d]) * SPLAT_SCALE));
      }
    }
  }
}

// counters[0] += used points, counters[1] += skipped points
__global__ void __launch_bounds__(BLOCK)
splat_kernel(const float* __restrict__ points, const float* __restrict__ normals, i64 n, Box B, long long* __restrict__ acc,
             unsigned long long* __restrict__ counters) {
  const i64 nodes = B.Nx * B.Ny * B.Nz;
  unsigned long long used = 0, skipped = 0;
  for (i64 i = (i64)blockIdx.x * BLOCK + threadIdx.x; i < n; i += (i64)gridDim.x * BLOCK) {
    const float p[3] = {points[3 * i], points[3 * i + 1], points[3 * i + 2]};
    const float m[3] = {normals[3 * i], normals[3 * i + 1], normals[3 * i + 2]};
    PointCell c;
    if (!point_cell(p, m, B, &c)) {
      skipped++;
      continue;
    }
    used++;
    splat_point(c, m, B, [&](int d, i64 node, long long v) {
      if (v) atomicAdd(reinterpret_cast<unsigned long long*>(acc + d * nodes + node), (unsigned long long)v);
    });
  }
  wave_count(used, counters);   // behind the grid-stride loop every lane is back
  wave_count(skipped, counters + 1);
}

// ---- fixed-order sums ---------------------------------------------------------------------------------------------------

// the workgroup's sum of `mine` in a fixed tree, valid in thread 0
__device__ inline double block_sum(double mine, double* red) {
  const int tid = threadIdx.y * blockDim.x + threadIdx.x;
  red[tid] = mine;
  __syncthreads();
  for (int s = BLOCK / 2; s > 0; s >>= 1) {
    if (tid < s) red[tid] += red[tid + s];
    __syncthreads();
  }
  return red[0];
}

__device__ inline i64 block_linear() { return ((i64)blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x; }

// one workgroup: *out = the sum of partial[0 .. n), each thread its strided share in order, then the tree
__global__ void __launch_bounds__(BLOCK) reduce_kernel(const double* __restrict__ partial, i64 n, double* __restrict__ out) {
  __shared__ double red[BLOCK];
  double s = 0.0;
  for (i64 i = threadIdx.x; i < n; i += BLOCK) s += partial[i];
  s = block_sum(s, red);
  if (threadIdx.x == 0) *out = s;
}

// ---- a level of the multigrid hierarchy ------------------------------------------------------------------------------------

struct Lvl {
  int nx, ny, nz;
  int P;             // floats per row: nx rounded up to a multiple of 4
  float c[3];        // 1 / h_d^2
  float lo_last[3];  // the coefficient of the lower neighbour at the last node of axis d: c * 2 / (1 + delta)
  float d_last[3];   // that node's share of the diagonal: c * 2 / delta (elsewhere 2 c)
};

__device__ inline float4 ld4(const float* p) { return *reinterpret_cast<const float4*>(p); }
__device__ inline float4 zero4() { return make_float4(0.0f, 0.0f, 0.0f, 0.0f); }

// One damped Jacobi sweep: out = u + OMEGA (A u - b) / D.  ZERO: u is zero and is not read.  One lane per four nodes of a
// row, a wave per row, the workgroup marches over planes [z0, z0 + zlen).
template <bool ZERO>
__global__ void __launch_bounds__(BLOCK)
jacobi_kernel(Lvl L, const float* __restrict__ u, const float* __restrict__ b, float* __restrict__ out, int zlen) {
  const int lane = threadIdx.x;
  const int q = blockIdx.x * WAVE + lane, y = blockIdx.y * ROWS + threadIdx.y;
  if (y >= L.ny) return;   // the whole wave
  const int Q = L.P >> 2;
  const bool act = q < Q;
  const int z0 = blockIdx.z * zlen, z1 = min(z0 + zlen, L.nz);
  const i64 plane = (i64)L.P * L.ny;
  const i64 col = (i64)y * L.P + 4 * (i64)q;
  const int x0 = 4 * q;
  // per node of the quad: the lower-neighbour coefficient and the diagonal share along x
  float lox[4], dx[4];
  for (int j = 0; j < 4; j++) {
    const bool last = x0 + j == L.nx - 1;
    lox[j] = last ? L.lo_last[0] : L.c[0];
    dx[j] = last ? L.d_last[0] : 2.0f * L.c[0];
  }
  const float loy = y == L.ny - 1 ? L.lo_last[1] : L.c[1], dy = y == L.ny - 1 ? L.d_last[1] : 2.0f * L.c[1];
  float4 zm = zero4(), cur = zero4();
  if (!ZERO && act) {
    if (z0 > 0) zm = ld4(u + (i64)(z0 - 1) * plane + col);
    cur = ld4(u + (i64)z0 * plane + col);
  }
  for (int z = z0; z < z1; z++) {
    const i64 at = (i64)z * plane + col;
    const float loz = z == L.nz - 1 ? L.lo_last[2] : L.c[2], dz = z == L.nz - 1 ? L.d_last[2] : 2.0f * L.c[2];
    float4 zp = zero4(), ym = zero4(), yp = zero4(), bq = zero4();
    float left = 0.0f, right = 0.0f;
    if (!ZERO) {
      if (act) {
        if (z + 1 < L.nz) zp = ld4(u + at + plane);
        if (y > 0) ym = ld4(u + at - L.P);
        if (y + 1 < L.ny) yp = ld4(u + at + L.P);
      }
      left = __shfl_up(cur.w, 1, WAVE);
      right = __shfl_down(cur.x, 1, WAVE);
      if (lane == 0) left = (act && q > 0) ? u[at - 1] : 0.0f;
      if (lane == WAVE - 1) right = (act && q + 1 < Q) ? u[at + 4] : 0.0f;
    }
    if (act) {
      bq = ld4(b + at);
      const float uc[4] = {cur.x, cur.y, cur.z, cur.w};
      const float xm[4] = {left, cur.x, cur.y, cur.z}, xp[4] = {cur.y, cur.z, cur.w, right};
      const float ymv[4] = {ym.x, ym.y, ym.z, ym.w}, ypv[4] = {yp.x, yp.y, yp.z, yp.w};
      const float zmv[4] = {zm.x, zm.y, zm.z, zm.w}, zpv[4] = {zp.x, zp.y, zp.z, zp.w};
      const float bv[4] = {bq.x, bq.y, bq.z, bq.w};
      float r[4];
      for (int j = 0; j < 4; j++) {
        const float D = (dx[j] + dy) + dz;
        float v;
        if (ZERO) {
          v = -(OMEGA * bv[j]) / D;
        } else {
          const float off = ((lox[j] * xm[j] + L.c[0] * xp[j]) + (loy * ymv[j] + L.c[1] * ypv[j])) +
                            (loz * zmv[j] + L.c[2] * zpv[j]);
          v = uc[j] + (OMEGA * ((off - D * uc[j]) - bv[j])) / D;
        }
        r[j] = x0 + j < L.nx ? v : 0.0f;
      }
      *reinterpret_cast<float4*>(out + at) = make_float4(r[0], r[1], r[2], r[3]);
    }
    zm = cur;
    cur = zp;
  }
}

// b - A u at a node of level F (scalar loads: the caller's workgroup reads every node it needs seven times from cache)
template <bool ZERO>
__device__ inline float residual_at(const Lvl& F, const float* __restrict__ u, const float* __restrict__ b, int x, int y,
                                    int z) {
  const i64 plane = (i64)F.P * F.ny;
  const i64 at = (i64)z * plane + (i64)y * F.P + x;
  const float bv = b[at];
  if (ZERO) return bv;
  const bool lx = x == F.nx - 1, ly = y == F.ny - 1, lz = z == F.nz - 1;
  const float uc = u[at];
  const float xm = x > 0 ? u[at - 1] : 0.0f, xp = lx ? 0.0f : u[at + 1];
  const float ym = y > 0 ? u[at - F.P] : 0.0f, yp = ly ? 0.0f : u[at + F.P];
  const float zm = z > 0 ? u[at - plane] : 0.0f, zp = lz ? 0.0f : u[at + plane];
  const float D = ((lx ? F.d_last[0] : 2.0f * F.c[0]) + (ly ? F.d_last[1] : 2.0f * F.c[1])) +
                  (lz ? F.d_last[2] : 2.0f * F.c[2]);
  const float off = (((lx ? F.lo_last[0] : F.c[0]) * xm + F.c[0] * xp) + ((ly ? F.lo_last[1] : F.c[1]) * ym + F.c[1] * yp)) +
                    ((lz ? F.lo_last[2] : F.c[2]) * zm + F.c[2] * zp);
  return bv - (off - D * uc);
}

// The residual of level F restricted to level C by full weighting (1/4, 1/2, 1/4 along every coarsened axis; coarse node j
// sits at fine node 2 j + 1).  A workgroup owns CTX x CTY coarse columns and marches over coarse planes [k0, k0 + zlen): the
// residual of one fine plane over the tile's footprint goes through LDS, each thread folds it in x and y, and the three
// planes of a coarse node are folded in registers (the plane two coarse nodes share is computed once).  ZERO: u is zero.
// NORM: partial[workgroup] = the sum of the squared residuals of the fine nodes this workgroup is the first to see.
template <bool ZERO, bool NORM>
__global__ void __launch_bounds__(BLOCK)
resid_restrict_kernel(Lvl F, Lvl C, int cox, int coy, int coz, const float* __restrict__ u, const float* __restrict__ b,
                      float* __restrict__ bc, int zlen, double* __restrict__ partial) {
  __shared__ float r[2 * CTY + 1][2 * CTX + 2];
  __shared__ double red[BLOCK];
  const int tx = threadIdx.x, ty = threadIdx.y, tid = ty * CTX + tx;
  const int X0 = blockIdx.x * CTX, Y0 = blockIdx.y * CTY;
  const int fx0 = cox ? 2 * X0 : X0, fy0 = coy ? 2 * Y0 : Y0;
  const int EX = cox ? 2 * CTX + 1 : CTX, EY = coy ? 2 * CTY + 1 : CTY;
  const int lx = cox ? 2 * tx + 1 : tx, ly = coy ? 2 * ty + 1 : ty;
  const bool lastx = blockIdx.x == gridDim.x - 1, lasty = blockIdx.y == gridDim.y - 1;
  const int k0 = blockIdx.z * zlen, k1 = min(k0 + zlen, C.nz);
  const int jx = X0 + tx, jy = Y0 + ty;
  const bool valid = jx < C.nx && jy < C.ny;
  double ss = 0.0;

  // the residual of fine plane zf over the footprint, folded in x and y for this thread's coarse column
  auto fold_plane = [&](int zf, bool count) -> float {
    __syncthreads();
    for (int i = tid; i < EX * EY; i += BLOCK) {
      const int py = i / EX, px = i - py * EX;
      const int x = fx0 + px, y = fy0 + py;
      float v = 0.0f;
      if (x < F.nx && y < F.ny && zf < F.nz) v = residual_at<ZERO>(F, u, b, x, y, zf);
      r[py][px] = v;
      if (NORM && count && (px < EX - 1 || !cox || lastx) && (py < EY - 1 || !coy || lasty)) ss += (double)v * (double)v;
    }
    __syncthreads();
    auto row = [&](int py) -> float {
      return cox ? (0.25f * r[py][lx - 1] + 0.5f * r[py][lx]) + 0.25f * r[py][lx + 1] : r[py][lx];
    };
    return coy ? (0.25f * row(ly - 1) + 0.5f * row(ly)) + 0.25f * row(ly + 1) : row(ly);
  };

  const i64 cplane = (i64)C.P * C.ny;
  float carry = coz ? fold_plane(2 * k0, true) : 0.0f;
  for (int k = k0; k < k1; k++) {
    float v;
    if (coz) {
      const float mid = fold_plane(2 * k + 1, true);
      // counted here when it stays in this workgroup as the next node's carry or is the last plane of all; otherwise the
      // workgroup that marches on from k1 counts it as its first plane
      const float nxt = fold_plane(2 * k + 2, k + 1 < k1 || k == C.nz - 1);
      v = (0.25f * carry + 0.5f * mid) + 0.25f * nxt;
      carry = nxt;
    } else {
      v = fold_plane(k, true);
    }
    if (valid) bc[(i64)k * cplane + (i64)jy * C.P + jx] = v;
  }
  if (NORM) {
    const double s = block_sum(ss, red);
    if (tid == 0) partial[block_linear()] = s;
  }
}

// the coarse nodes fine node i interpolates from along one axis, and their weights (a node that does not exist: weight 0)
__device__ inline void interp_axis(int co, int i, int nc, int* a, float* wa, int* bq, float* wb) {
  *bq = 0;
  *wb = 0.0f;
  if (!co) {
    *a = i;
    *wa = 1.0f;
  } else if (i & 1) {
    *a = i >> 1;
    *wa = *a < nc ? 1.0f : 0.0f;
    if (*a >= nc) *a = 0;
  } else {
    *a = (i >> 1) - 1;
    *wa = *a >= 0 ? 0.5f : 0.0f;
    if (*a < 0) *a = 0;
    *bq = i >> 1;
    *wb = *bq < nc ? 0.5f : 0.0f;
    if (*bq >= nc) *bq = 0;
  }
}

// u += P e (ZERO: u = P e), P the trilinear interpolation from level C to level F; one lane per four fine nodes of a row
template <bool ZERO>
__global__ void __launch_bounds__(BLOCK)
prolong_kernel(Lvl F, Lvl C, int cox, int coy, int coz, const float* __restrict__ e, float* __restrict__ u) {
  const int q = blockIdx.x * WAVE + threadIdx.x, y = blockIdx.y * ROWS + threadIdx.y;
  if (q >= (F.P >> 2) || y >= F.ny) return;
  const i64 fplane = (i64)F.P * F.ny, cplane = (i64)C.P * C.ny;
  int ya, yb;
  float wya, wyb;
  interp_axis(coy, y, C.ny, &ya, &wya, &yb, &wyb);
  for (int z = blockIdx.z; z < F.nz; z += gridDim.z) {
    int za, zb;
    float wza, wzb;
    interp_axis(coz, z, C.nz, &za, &wza, &zb, &wzb);
    float acc[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    for (int kz = 0; kz < 2; kz++) {
      const float wz = kz ? wzb : wza;
      if (wz == 0.0f) continue;
      for (int ky = 0; ky < 2; ky++) {
        const float w = wz * (ky ? wyb : wya);
        if (w == 0.0f) continue;
        const float* __restrict__ row = e + (i64)(kz ? zb : za) * cplane + (i64)(ky ? yb : ya) * C.P;
        float v[4];
        if (cox) {
          const int j = 2 * q;   // fine nodes 4q .. 4q+3 lie between coarse nodes 2q-1, 2q, 2q+1
          const float c0 = j - 1 >= 0 && j - 1 < C.nx ? row[j - 1] : 0.0f;
          const float c1 = j < C.nx ? row[j] : 0.0f;
          const float c2 = j + 1 < C.nx ? row[j + 1] : 0.0f;
          v[0] = 0.5f * (c0 + c1);
          v[1] = c1;
          v[2] = 0.5f * (c1 + c2);
          v[3] = c2;
        } else {
          const float4 t = ld4(row + 4 * q);
          v[0] = t.x;
          v[1] = t.y;
          v[2] = t.z;
          v[3] = t.w;
        }
        for (int j = 0; j < 4; j++) acc[j] += w * v[j];
      }
    }
    float* __restrict__ dst = u + (i64)z * fplane + (i64)y * F.P + 4 * (i64)q;
    float4 o = ZERO ? zero4() : ld4(dst);
    o.x = 4 * q + 0 < F.nx ? o.x + acc[0] : 0.0f;
    o.y = 4 * q + 1 < F.nx ? o.y + acc[1] : 0.0f;
    o.z = 4 * q + 2 < F.nx ? o.z + acc[2] : 0.0f;
    o.w = 4 * q + 3 < F.nx ? o.w + acc[3] : 0.0f;
    *reinterpret_cast<float4*>(dst) = o;
  }
}

// b = div V over the box (rows of P floats, the slack zero), V = (float)((double)acc * 2^-24) and zero outside the box;
// partial[workgroup] = the workgroup's sum of b^2
__global__ void __launch_bounds__(BLOCK)
divergence_kernel(Box B, int P, const long long* __restrict__ acc, float* __restrict__ b, double* __restrict__ partial) {
  __shared__ double red[BLOCK];
  const int q = blockIdx.x * WAVE + threadIdx.x, y = blockIdx.y * ROWS + threadIdx.y;
  const i64 nodes = B.Nx * B.Ny * B.Nz;
  double ss = 0.0;
  if (q < (P >> 2) && y < B.Ny) {
    for (i64 z = blockIdx.z; z < B.Nz; z += gridDim.z) {
      float o[4];
      for (int j = 0; j < 4; j++) {
        const i64 x = 4 * (i64)q + j;
        float v = 0.0f;
        if (x < B.Nx) {
          const i64 at = (z * B.Ny + y) * B.Nx + x;
          auto V = [&](int d, i64 node) -> float { return (float)((double)acc[d * nodes + node] * SPLAT_UNSCALE); };
          const float xp = x + 1 < B.Nx ? V(0, at + 1) : 0.0f, xm = x > 0 ? V(0, at - 1) : 0.0f;
          const float yp = y + 1 < B.Ny ? V(1, at + B.Nx) : 0.0f, ym = y > 0 ? V(1, at - B.Nx) : 0.0f;
          const float zp = z + 1 < B.Nz ? V(2, at + B.Nx * B.Ny) : 0.0f, zm = z > 0 ? V(2, at - B.Nx * B.Ny) : 0.0f;
          v = (0.5f * (xp - xm) + 0.5f * (yp - ym)) + 0.5f * (zp - zm);
          ss += (double)v * (double)v;
        }
        o[j] = v;
      }
      *reinterpret_cast<float4*>(b + (z * B.Ny + y) * (i64)P + 4 * (i64)q) = make_float4(o[0], o[1], o[2], o[3]);
    }
  }
  const double s = block_sum(ss, red);
  if (threadIdx.x == 0 && threadIdx.y == 0) partial[block_linear()] = s;
}

// partial[workgroup] = the sum over its used points of chi interpolated trilinearly, in double
__global__ void __launch_bounds__(BLOCK)
sample_kernel(const float* __restrict__ points, const float* __restrict__ normals, i64 n, Box B, int P,
              const float* __restrict__ chi, double* __restrict__ partial) {
  __shared__ double red[BLOCK];
  const i64 i = (i64)blockIdx.x * BLOCK + threadIdx.x;
  double v = 0.0;
  if (i < n) {
    const float p[3] = {points[3 * i], points[3 * i + 1], points[3 * i + 2]};
    const float m[3] = {normals[3 * i], normals[3 * i + 1], normals[3 * i + 2]};
    PointCell c;
    if (point_cell(p, m, B, &c)) {
      for (int cz = 0; cz < 2; cz++) {
        const double wz = cz ? c.f[2] : 1.0 - c.f[2];
        for (int cy = 0; cy < 2; cy++) {
          const double wy = cy ? c.f[1] : 1.0 - c.f[1];
          for (int cx = 0; cx < 2; cx++) {
            const double wx = cx ? c.f[0] : 1.0 - c.f[0];
            v += ((wx * wy) * wz) * (double)chi[((c.i[2] + cz) * B.Ny + (c.i[1] + cy)) * (i64)P + (c.i[0] + cx)];
          }
        }
      }
    }
  }
  const double s = block_sum(v, red);
  if (threadIdx.x == 0) partial[blockIdx.x] = s;
}

// counters[2] += nodes on the faces of the box with chi < iso, counters[3] += those with chi > iso (every node once)
__global__ void __launch_bounds__(BLOCK)
face_kernel(Box B, int P, const float* __restrict__ chi, double iso, unsigned long long* __restrict__ counters) {
  const i64 nxy = B.Nx * B.Ny, nxz = B.Nx * (B.Nz - 2), nyz = (B.Ny - 2) * (B.Nz - 2);
  const i64 total = 2 * (nxy + nxz + nyz);
  unsigned long long lo = 0, hi = 0;
  for (i64 i = (i64)blockIdx.x * BLOCK + threadIdx.x; i < total; i += (i64)gridDim.x * BLOCK) {
    i64 x, y, z, k = i;
    if (k < 2 * nxy) {
      z = k < nxy ? 0 : B.Nz - 1;
      k %= nxy;
      y = k / B.Nx;
      x = k - y * B.Nx;
    } else if ((k -= 2 * nxy) < 2 * nxz) {
      y = k < nxz ? 0 : B.Ny - 1;
      k %= nxz;
      z = 1 + k / B.Nx;
      x = k % B.Nx;
    } else {
      k -= 2 * nxz;
      x = k < nyz ? 0 : B.Nx - 1;
      k %= nyz;
      z = 1 + k / (B.Ny - 2);
      y = 1 + k % (B.Ny - 2);
    }
    const double c = (double)chi[(z * B.Ny + y) * (i64)P + x];
    lo += c < iso ? 1 : 0;
    hi += c > iso ? 1 : 0;
  }
  wave_count(lo, counters + 2);   // behind the grid-stride loop every lane is back
  wave_count(hi, counters + 3);
}

// mask = 1 where chi < iso (inward: chi > iso) over the image, chi_out (nullable) = chi there;
// counters[4] += mask voxels on a face of the image
__global__ void __launch_bounds__(BLOCK)
cut_kernel(Box B, int P, const float* __restrict__ chi, double iso, int inward, float* __restrict__ mask,
           float* __restrict__ chi_out, unsigned long long* __restrict__ counters) {
  const i64 n = B.nx * B.ny * B.nz;
  unsigned long long touch = 0;
  for (i64 i = (i64)blockIdx.x * BLOCK + threadIdx.x; i < n; i += (i64)gridDim.x * BLOCK) {
    const i64 z = i / (B.nx * B.ny), rem = i - z * (B.nx * B.ny);
    const i64 y = rem / B.nx, x = rem - y * B.nx;
    const float c = chi[((z + B.pad) * B.Ny + (y + B.pad)) * (i64)P + (x + B.pad)];
    const bool in = inward ? (double)c > iso : (double)c < iso;
    mask[i] = in ? 1.0f : 0.0f;
    if (chi_out) chi_out[i] = c;
    if (in && (x == 0 || y == 0 || z == 0 || x == B.nx - 1 || y == B.ny - 1 || z == B.nz - 1)) touch++;
  }
  wave_count(touch, counters + 4);   // behind the grid-stride loop every lane is back
}

// ---- host -------------------------------------------------------------------------------------------------------------------

struct Args {
  const float* points;
  const float* normals;
  i64 n;
  i64 nx, ny, nz, pad;
  int orientation;
};

int check_args(const void* ctx_or_flag, const Args& a, const void* out) {
  VH_REQUIRE(ctx_or_flag && out, "null argument");
  VH_REQUIRE(a.nx >= 3 && a.ny >= 3 && a.nz >= 3, "close_surface: every image dimension must be at least 3");
  VH_REQUIRE(a.pad >= 0 && a.n >= 0, "close_surface: negative pad or point count");
  VH_REQUIRE(a.n == 0 || (a.points && a.normals), "close_surface: null point or normal array");
  VH_REQUIRE(a.orientation >= VISFD_HIP_CLOSE_OUTWARD && a.orientation <= VISFD_HIP_CLOSE_AUTO,
             "close_surface: unknown orientation");
  VH_REQUIRE(a.pad <= MAX_DIM && a.nx + 2 * a.pad <= MAX_DIM && a.ny + 2 * a.pad <= MAX_DIM && a.nz + 2 * a.pad <= MAX_DIM,
             "close_surface: a padded dimension above 65535");
  return VISFD_HIP_OK;
}

Box box_of(const Args& a) {
  Box B;
  B.nx = a.nx, B.ny = a.ny, B.nz = a.nz, B.pad = a.pad;
  B.Nx = a.nx + 2 * a.pad, B.Ny = a.ny + 2 * a.pad, B.Nz = a.nz + 2 * a.pad;
  return B;
}

struct Level {
  Lvl g;
  int co[3];          // which axes the step to the next level coarsens
  float* buf[2];      // the iterate ping-pongs between them
  int cur = 0;
  float* b;
  size_t floats() const { return (size_t)g.P * g.ny * g.nz; }
};

// the hierarchy below a box: sizes, spacings, boundary distances
std::vector<Level> plan_levels(const Box& B) {
  std::vector<Level> L;
  int n[3] = {(int)B.Nx, (int)B.Ny, (int)B.Nz};
  double c[3] = {1.0, 1.0, 1.0}, delta[3] = {1.0, 1.0, 1.0};
  for (;;) {
    Level lv;
    lv.g.nx = n[0], lv.g.ny = n[1], lv.g.nz = n[2];
    lv.g.P = (n[0] + 3) & ~3;
    for (int d = 0; d < 3; d++) {
      lv.g.c[d] = (float)c[d];
      lv.g.lo_last[d] = (float)(c[d] * 2.0 / (1.0 + delta[d]));
      lv.g.d_last[d] = (float)(c[d] * 2.0 / delta[d]);
      lv.co[d] = n[d] >= 3;
    }
    lv.buf[0] = lv.buf[1] = lv.b = nullptr;
    L.push_back(lv);
    if (!(lv.co[0] || lv.co[1] || lv.co[2]) || (int)L.size() == MAX_LEVELS) break;
    for (int d = 0; d < 3; d++)
      if (lv.co[d]) {
        delta[d] = (n[d] & 1) ? 0.5 * (1.0 + delta[d]) : 0.5 * delta[d];
        n[d] /= 2;
        c[d] *= 0.25;
      }
  }
  return L;
}

struct SweepGrid {
  dim3 grid;
  int zlen;
};
// rows x quads in workgroups of gx x gy, the planes cut into marches so that the chip has a few workgroups per CU
SweepGrid sweep_grid(int gx, int gy, int nz) {
  i64 chunks = 2048 / ((i64)gx * gy);
  if (chunks < 1) chunks = 1;
  if (chunks > nz) chunks = nz;
  const int zlen = (int)((nz + chunks - 1) / chunks);
  return {dim3((unsigned)gx, (unsigned)gy, (unsigned)((nz + zlen - 1) / zlen)), zlen};
}
inline int quads_x(const Lvl& g) { return ((g.P >> 2) + WAVE - 1) / WAVE; }
inline int rows_y(const Lvl& g) { return (g.ny + ROWS - 1) / ROWS; }

int sweep(visfd_hip_ctx* ctx, Level& lv, bool zero) {
  const SweepGrid sg = sweep_grid(quads_x(lv.g), rows_y(lv.g), lv.g.nz);
  const dim3 block(WAVE, ROWS);
  if (zero)
    jacobi_kernel<true><<<sg.grid, block, 0, ctx->stream>>>(lv.g, lv.buf[lv.cur], lv.b, lv.buf[lv.cur ^ 1], sg.zlen);
  else
    jacobi_kernel<false><<<sg.grid, block, 0, ctx->stream>>>(lv.g, lv.buf[lv.cur], lv.b, lv.buf[lv.cur ^ 1], sg.zlen);
  VH_HIP(hipGetLastError());
  lv.cur ^= 1;
  return VISFD_HIP_OK;
}

// workgroups of resid_restrict_kernel from level `f` to the next
SweepGrid restrict_grid(const Level& c) {
  return sweep_grid((c.g.nx + CTX - 1) / CTX, (c.g.ny + CTY - 1) / CTY, c.g.nz);
}

// b of level l + 1 = the restricted residual of level l (zero: its iterate is zero); norm: the partial sums of squares
int restrict_residual(visfd_hip_ctx* ctx, std::vector<Level>& L, size_t l, bool zero, double* partial) {
  Level &f = L[l], &c = L[l + 1];
  const SweepGrid sg = restrict_grid(c);
  const dim3 block(CTX, CTY);
  if (partial)
    resid_restrict_kernel<false, true><<<sg.grid, block, 0, ctx->stream>>>(f.g, c.g, f.co[0], f.co[1], f.co[2], f.buf[f.cur], f.b,
                                                                           c.b, sg.zlen, partial);
  else if (zero)
    resid_restrict_kernel<true, false><<<sg.grid, block, 0, ctx->stream>>>(f.g, c.g, f.co[0], f.co[1], f.co[2], f.buf[f.cur], f.b,
                                                                           c.b, sg.zlen, nullptr);
  else
    resid_restrict_kernel<false, false><<<sg.grid, block, 0, ctx->stream>>>(f.g, c.g, f.co[0], f.co[1], f.co[2], f.buf[f.cur],
                                                                            f.b, c.b, sg.zlen, nullptr);
  VH_HIP(hipGetLastError());
  return VISFD_HIP_OK;
}

// Level l from its right-hand side, the iterate zero on entry except at level 0, whose restriction the caller has run.
int cycle_below(visfd_hip_ctx* ctx, std::vector<Level>& L, size_t l) {
  Level& lv = L[l];
  if (l + 1 == L.size()) {
    for (int s = 0; s < COARSEST_SWEEPS; s++) VH_TRY(sweep(ctx, lv, s == 0));
    return VISFD_HIP_OK;
  }
  if (l > 0) VH_TRY(restrict_residual(ctx, L, l, true, nullptr));
  VH_TRY(cycle_below(ctx, L, l + 1));
  const Level& c = L[l + 1];
  const dim3 grid((unsigned)quads_x(lv.g), (unsigned)rows_y(lv.g), (unsigned)std::min(lv.g.nz, 1024));
  const dim3 block(WAVE, ROWS);
  if (l > 0)
    prolong_kernel<true><<<grid, block, 0, ctx->stream>>>(lv.g, c.g, lv.co[0], lv.co[1], lv.co[2], c.buf[c.cur], lv.buf[lv.cur]);
  else
    prolong_kernel<false><<<grid, block, 0, ctx->stream>>>(lv.g, c.g, lv.co[0], lv.co[1], lv.co[2], c.buf[c.cur], lv.buf[lv.cur]);
  VH_HIP(hipGetLastError());
  for (int s = 0; s < POST_SWEEPS; s++) VH_TRY(sweep(ctx, lv, false));
  return VISFD_HIP_OK;
}

inline size_t align16(size_t b) { return (b + 15) & ~(size_t)15; }

// device buffers of one call
struct Work {
  long long* acc;
  double* partial;
  double* sums;                   // [0] sum b^2, [1] sum r^2, [2] the samples' sum
  unsigned long long* counters;   // used, skipped, face nodes below, face nodes above, mask voxels on a face
  size_t npartial;
};

int get_work(visfd_hip_ctx* ctx, const Box& B, i64 n, const std::vector<Level>& L, Work* w) {
  const i64 nodes = B.Nx * B.Ny * B.Nz;
  VH_TRY(ws(ctx, WS_CS_ACC, (size_t)(3 * nodes), &w->acc));
  // the partial sums: the divergence's workgroups, the finest restriction's, the sampler's
  const Lvl& g = L[0].g;
  size_t np = (size_t)quads_x(g) * rows_y(g) * (size_t)std::min<i64>(B.Nz, 1024);
  if (L.size() > 1) {
    const SweepGrid sg = restrict_grid(L[1]);
    np = std::max(np, (size_t)sg.grid.x * sg.grid.y * sg.grid.z);
  }
  np = std::max(np, (size_t)((n + BLOCK - 1) / BLOCK));
  np = std::max<size_t>(np, 1);
  char* aux = nullptr;
  VH_TRY(ws(ctx, WS_CS_AUX, align16(sizeof(double) * np) + 8 * sizeof(double) + 8 * sizeof(unsigned long long), &aux));
  w->partial = reinterpret_cast<double*>(aux);
  w->sums = reinterpret_cast<double*>(aux + align16(sizeof(double) * np));
  w->counters = reinterpret_cast<unsigned long long*>(w->sums + 8);
  w->npartial = np;
  return VISFD_HIP_OK;
}

// steps 1 of the definition on device arrays: the three volumes zeroed and filled, counters[0..1] set; asynchronous
int splat_dev(visfd_hip_ctx* ctx, const Args& a, const Box& B, const Work& w) {
  const i64 nodes = B.Nx * B.Ny * B.Nz;
  VH_HIP(hipMemsetAsync(w.acc, 0, sizeof(long long) * 3 * (size_t)nodes, ctx->stream));
  VH_HIP(hipMemsetAsync(w.counters, 0, 8 * sizeof(unsigned long long), ctx->stream));
  if (a.n > 0) {
    splat_kernel<<<dim3(grid_for(a.n, BLOCK, (i64)ctx->num_cus * 16)), dim3(BLOCK), 0, ctx->stream>>>(a.points, a.normals, a.n, B,
                                                                                                    w.acc, w.counters);
    VH_HIP(hipGetLastError());
  }
  return VISFD_HIP_OK;
}

int reduce_to(visfd_hip_ctx* ctx, const Work& w, size_t n, int which) {
  reduce_kernel<<<dim3(1), dim3(BLOCK), 0, ctx->stream>>>(w.partial, (i64)n, w.sums + which);
  VH_HIP(hipGetLastError());
  return VISFD_HIP_OK;
}

// points, normals, mask, chi_out (nullable): device arrays.  Returns with the stream idle.
int close_surface_dev(visfd_hip_ctx* ctx, const Args& a, float* mask, float* chi_out) {
  VH_HIP(hipSetDevice(ctx->device));
  const Box B = box_of(a);
  std::vector<Level> L = plan_levels(B);
  Work w;
  VH_TRY(get_work(ctx, B, a.n, L, &w));
  size_t total = 0;
  for (const Level& lv : L) total += 3 * lv.floats();
  float* grid = nullptr;
  VH_TRY(ws(ctx, WS_CS_GRID, total, &grid));
  for (Level& lv : L) {
    lv.buf[0] = grid, lv.buf[1] = grid + lv.floats(), lv.b = grid + 2 * lv.floats();
    grid += 3 * lv.floats();
  }
  Level& top = L[0];
  const int P = top.g.P;
  const i64 nimage = a.nx * a.ny * a.nz;
  int64_t* last = ctx->close_surface_last;
  for (int k = 0; k < 6; k++) last[k] = 0;
  last[3] = VISFD_HIP_CLOSE_STOP_NONE;
  last[4] = a.orientation == VISFD_HIP_CLOSE_INWARD ? VISFD_HIP_CLOSE_INWARD : VISFD_HIP_CLOSE_OUTWARD;
  ctx->close_surface_values[0] = ctx->close_surface_values[1] = 0.0;

  PhaseClock<3> clock;   // option close_surface_time
  clock.start(ctx->stream, ctx->opt.close_surface_time != 0);
  VH_TRY(splat_dev(ctx, a, B, w));
  const dim3 block(WAVE, ROWS);
  const dim3 dgrid((unsigned)quads_x(top.g), (unsigned)rows_y(top.g), (unsigned)std::min<i64>(B.Nz, 1024));
  divergence_kernel<<<dgrid, block, 0, ctx->stream>>>(B, P, w.acc, top.b, w.partial);
  VH_HIP(hipGetLastError());
  VH_TRY(reduce_to(ctx, w, (size_t)dgrid.x * dgrid.y * dgrid.z, 0));
  VH_HIP(hipMemsetAsync(top.buf[0], 0, sizeof(float) * top.floats(), ctx->stream));
  unsigned long long counts[2] = {0, 0};
  double bb = 0.0;
  VH_HIP(hipMemcpyAsync(counts, w.counters, sizeof(counts), hipMemcpyDeviceToHost, ctx->stream));
  VH_HIP(hipMemcpyAsync(&bb, w.sums, sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  VH_HIP(hipStreamSynchronize(ctx->stream));
  last[0] = (int64_t)counts[0];
  last[1] = (int64_t)counts[1];
  clock.mark(1);

  if (counts[0] > 0 && bb > 0.0) {
    const double rtol = std::pow(10.0, -(double)ctx->opt.close_surface_rtol_exp);
    const int cap = ctx->opt.close_surface_max_cycles < 0 ? 0 : ctx->opt.close_surface_max_cycles;
    const SweepGrid sg = restrict_grid(L[1]);
    for (int cycles = 0;; cycles++) {
      // the residual of the iterate so far, restricted for the cycle that may follow
      double rr = bb;
      if (cycles == 0) {   // the iterate is zero: the residual is b, nothing to sum and nothing to wait for
        VH_TRY(restrict_residual(ctx, L, 0, true, nullptr));
      } else {
        VH_TRY(restrict_residual(ctx, L, 0, false, w.partial));
        VH_TRY(reduce_to(ctx, w, (size_t)sg.grid.x * sg.grid.y * sg.grid.z, 1));
        VH_HIP(hipMemcpyAsync(&rr, w.sums + 1, sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
        VH_HIP(hipStreamSynchronize(ctx->stream));
      }
      const double ratio = std::sqrt(rr) / std::sqrt(bb);
      last[2] = cycles;
      ctx->close_surface_values[0] = ratio;
      if (ratio <= rtol) {
        last[3] = VISFD_HIP_CLOSE_STOP_RTOL;
        break;
      }
      if (cycles >= cap || !(ratio == ratio)) {
        last[3] = VISFD_HIP_CLOSE_STOP_CAP;
        break;
      }
      VH_TRY(cycle_below(ctx, L, 0));
    }
  }
  clock.mark(2);

  const float* chi = top.buf[top.cur];
  double iso = 0.0;
  int inward = a.orientation == VISFD_HIP_CLOSE_INWARD;
  unsigned long long c5[5] = {0, 0, 0, 0, 0};
  if (counts[0] > 0) {
    const size_t nb = (size_t)((a.n + BLOCK - 1) / BLOCK);
    sample_kernel<<<dim3((unsigned)nb), dim3(BLOCK), 0, ctx->stream>>>(a.points, a.normals, a.n, B, P, chi, w.partial);
    VH_HIP(hipGetLastError());
    VH_TRY(reduce_to(ctx, w, nb, 2));
    double sum = 0.0;
    VH_HIP(hipMemcpyAsync(&sum, w.sums + 2, sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    VH_HIP(hipStreamSynchronize(ctx->stream));
    iso = sum / (double)counts[0];
    if (a.orientation == VISFD_HIP_CLOSE_AUTO) {
      const i64 faces = 2 * (B.Nx * B.Ny + B.Nx * (B.Nz - 2) + (B.Ny - 2) * (B.Nz - 2));
      face_kernel<<<dim3(grid_for(faces, BLOCK, (i64)ctx->num_cus * 8)), dim3(BLOCK), 0, ctx->stream>>>(B, P, chi, iso, w.counters);
      VH_HIP(hipGetLastError());
      VH_HIP(hipMemcpyAsync(c5, w.counters, sizeof(c5), hipMemcpyDeviceToHost, ctx->stream));
      VH_HIP(hipStreamSynchronize(ctx->stream));
      inward = c5[2] <= c5[3] ? 0 : 1;   // the set with fewer nodes on the faces; a tie: outward
    }
    cut_kernel<<<dim3(grid_for(nimage, BLOCK, (i64)ctx->num_cus * 16)), dim3(BLOCK), 0, ctx->stream>>>(B, P, chi, iso, inward, mask,
                                                                                                   chi_out, w.counters);
    VH_HIP(hipGetLastError());
    VH_HIP(hipMemcpyAsync(c5, w.counters, sizeof(c5), hipMemcpyDeviceToHost, ctx->stream));
  } else {
    VH_HIP(hipMemsetAsync(mask, 0, sizeof(float) * (size_t)nimage, ctx->stream));
    if (chi_out) VH_HIP(hipMemsetAsync(chi_out, 0, sizeof(float) * (size_t)nimage, ctx->stream));
  }
  clock.mark(3);
  VH_HIP(hipStreamSynchronize(ctx->stream));
  if (clock.on) clock.read(ctx->close_surface_ms);
  last[4] = inward ? VISFD_HIP_CLOSE_INWARD : VISFD_HIP_CLOSE_OUTWARD;
  last[5] = c5[4] > 0 ? 1 : 0;
  ctx->close_surface_values[1] = iso;
  return VISFD_HIP_OK;
}

int splat_host(const Args& a, int64_t* acc, int64_t counts[2]) {
  const Box B = box_of(a);
  const i64 nodes = B.Nx * B.Ny * B.Nz;
  for (i64 i = 0; i < 3 * nodes; i++) acc[i] = 0;
  i64 used = 0, skipped = 0;
  for (i64 i = 0; i < a.n; i++) {
    PointCell c;
    if (!point_cell(a.points + 3 * i, a.normals + 3 * i, B, &c)) {
      skipped++;
      continue;
    }
    used++;
    splat_point(c, a.normals + 3 * i, B, [&](int d, i64 node, long long v) { acc[d * nodes + node] += v; });
  }
  if (counts) counts[0] = used, counts[1] = skipped;
  return VISFD_HIP_OK;
}

// the point lists of a host-array call into slots WS_H2D_0 and WS_H2D_1
int points_up(visfd_hip_ctx* ctx, Args* a) {
  if (a->n == 0) return VISFD_HIP_OK;
  float *dp = nullptr, *dn = nullptr;
  VH_TRY(ws(ctx, WS_H2D_0, (size_t)(3 * a->n), &dp));
  VH_TRY(ws(ctx, WS_H2D_1, (size_t)(3 * a->n), &dn));
  VH_HIP(hipMemcpyAsync(dp, a->points, sizeof(float) * 3 * (size_t)a->n, hipMemcpyHostToDevice, ctx->stream));
  VH_HIP(hipMemcpyAsync(dn, a->normals, sizeof(float) * 3 * (size_t)a->n, hipMemcpyHostToDevice, ctx->stream));
  a->points = dp, a->normals = dn;
  return VISFD_HIP_OK;
}

// the volumes of step 1 into `acc` (device when acc_on_device), the point lists on the device already
int splat_only(visfd_hip_ctx* ctx, const Args& a, int64_t* acc, bool acc_on_device, int64_t counts[2]) {
  const Box B = box_of(a);
  const std::vector<Level> L = plan_levels(B);
  Work w;
  VH_TRY(get_work(ctx, B, a.n, L, &w));
  VH_TRY(splat_dev(ctx, a, B, w));
  const size_t bytes = sizeof(int64_t) * 3 * (size_t)(B.Nx * B.Ny * B.Nz);
  VH_HIP(hipMemcpyAsync(acc, w.acc, bytes, acc_on_device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, ctx->stream));
  unsigned long long c[2] = {0, 0};
  VH_HIP(hipMemcpyAsync(c, w.counters, sizeof(c), hipMemcpyDeviceToHost, ctx->stream));
  VH_HIP(hipStreamSynchronize(ctx->stream));
  if (counts) counts[0] = (int64_t)c[0], counts[1] = (int64_t)c[1];
  return VISFD_HIP_OK;
}

}  // namespace
}  // namespace vh

using namespace vh;

extern "C" {

int visfd_hip_close_surface_dev(visfd_hip_ctx* ctx, const float* points, const float* normals, int64_t n, int64_t nx, int64_t ny,
                                int64_t nz, int64_t pad, int orientation, float* mask, float* chi_out) {
  const Args a = {points, normals, n, nx, ny, nz, pad, orientation};
  VH_TRY(check_args(ctx, a, mask));
  const size_t image = sizeof(float) * (size_t)(nx * ny * nz), list = sizeof(float) * 3 * (size_t)n;
  VH_REQUIRE(!overlap_bytes(mask, image, chi_out, image), "close_surface: chi_out overlaps mask");
  for (const float* out : {(const float*)mask, (const float*)chi_out})
    VH_REQUIRE(!overlap_bytes(out, image, points, list) && !overlap_bytes(out, image, normals, list),
               "close_surface: an output overlaps the point or normal list");
  return close_surface_dev(ctx, a, mask, chi_out);
}

int visfd_hip_close_surface(visfd_hip_ctx* ctx, const float* points, const float* normals, int64_t n, int64_t nx, int64_t ny,
                            int64_t nz, int64_t pad, int orientation, float* mask, float* chi_out) {
  Args a = {points, normals, n, nx, ny, nz, pad, orientation};
  VH_TRY(check_args(ctx, a, mask));
  VH_HIP(hipSetDevice(ctx->device));
  VH_TRY(points_up(ctx, &a));
  const Stage st = {ctx, (size_t)(nx * ny * nz)};
  float *dm = nullptr, *dc = nullptr;
  VH_TRY(st.out(WS_H2D_2, &dm));
  if (chi_out) VH_TRY(st.out(WS_H2D_3, &dc));
  VH_TRY(close_surface_dev(ctx, a, dm, dc));
  if (chi_out) VH_HIP(hipMemcpyAsync(chi_out, dc, sizeof(float) * st.n, hipMemcpyDeviceToHost, ctx->stream));
  return st.down(mask, dm);
}

int visfd_hip_close_surface_splat_dev(visfd_hip_ctx* ctx, const float* points, const float* normals, int64_t n, int64_t nx,
                                      int64_t ny, int64_t nz, int64_t pad, int64_t* acc, int64_t counts[2]) {
  const Args a = {points, normals, n, nx, ny, nz, pad, VISFD_HIP_CLOSE_OUTWARD};
  VH_TRY(check_args(ctx, a, acc));
  VH_HIP(hipSetDevice(ctx->device));
  return splat_only(ctx, a, acc, true, counts);
}

int visfd_hip_close_surface_splat(visfd_hip_ctx* ctx, const float* points, const float* normals, int64_t n, int64_t nx,
                                  int64_t ny, int64_t nz, int64_t pad, int64_t* acc, int64_t counts[2]) {
  Args a = {points, normals, n, nx, ny, nz, pad, VISFD_HIP_CLOSE_OUTWARD};
  VH_TRY(check_args(ctx, a, acc));
  VH_HIP(hipSetDevice(ctx->device));
  VH_TRY(points_up(ctx, &a));
  return splat_only(ctx, a, acc, false, counts);
}

int visfd_hip_close_surface_splat_host(const float* points, const float* normals, int64_t n, int64_t nx, int64_t ny, int64_t nz,
                                       int64_t pad, int64_t* acc, int64_t counts[2]) {
  const Args a = {points, normals, n, nx, ny, nz, pad, VISFD_HIP_CLOSE_OUTWARD};
  VH_TRY(check_args(acc, a, acc));
  return splat_host(a, acc, counts);
}

int visfd_hip_close_surface_last(visfd_hip_ctx* ctx, int64_t stats[6], double values[2]) {
  VH_REQUIRE(ctx && stats && values, "null argument");
  for (int k = 0; k < 6; k++) stats[k] = ctx->close_surface_last[k];
  values[0] = ctx->close_surface_values[0];
  values[1] = ctx->close_surface_values[1];
  return VISFD_HIP_OK;
}

int visfd_hip_close_surface_last_times(visfd_hip_ctx* ctx, float ms[3]) {
  VH_REQUIRE(ctx && ms, "null argument");
  for (int k = 0; k < 3; k++) ms[k] = ctx->close_surface_ms[k];
  return VISFD_HIP_OK;
}

}  // extern "C"
