// gauss_pair.hip -- both Gaussians of one DoG/LoG scale in two shared launches (unmasked, normalised, one half-width H on
// the three axes, H = 6..10), for gfx950.  dst = (G_a(src) - G_b(src)) * scale with the bits of ApplyDog / ApplyLog
// (lib/visfd/filter3d.hpp:1338-1402, :1466-1498).
//
//   pair_z_kernel    reads src once and writes the Z-filtered volumes of both filters (workspace slots WS_A, WS_B): 12 B/voxel
//   pair_yx_kernel   reads the two, runs the Y and X passes of both, normalises each, stores (g_a - g_b) * scale: 12 B/voxel
//
// against 52 B/voxel for two Gaussians of three single-axis launches each (csrc/gauss.hip), which is what a window too wide
// for the single sweep's register ring (H > 8, csrc/gauss_fused.hip) took before.  G_a is never written to memory, and dst
// may be src: the first launch has consumed src before the second one writes.
//
// Arithmetic contract: that of csrc/gauss.hip (pass order Z -> Y -> X, each pass rounded to float; per output the terms
// t[j]*f[i-j] added with j ascending, multiply and add separate: -ffp-contract=off; then / ((Dx*Dy)*Dz) per filter; then the
// epilogue's two roundings).  The Z and Y passes are marches in SCATTER form, as the Z pass of csrc/gauss_fused.hip (its header
// has the order argument): j ascending means the sources of an output arrive in DESCENDING position, so a march DOWN the
// axis can add the term of each arriving sample to the 2H+1 running sums in flight, each in the reference's order; with
// taps symmetric bit for bit (checked on the host) t[j]*f and t[-j]*f are the same IEEE product, H+1 multiplies per sample
// and filter.  Every sum starts from its first product instead of +0.0; as in gauss_fused.hip that can only turn a +0.0 into a
// -0.0, which changes no non-zero value downstream and is undone by adding +0.0 once before the normaliser.  Zero extension:
// a 0.0f sample adds an exact zero, which equals skipping the term (filter1d.hpp:98-99).
#include <type_traits>

#include "common.hpp"

namespace vh {

namespace {

constexpr int Z_NT = 256;     // pair_z_kernel: threads per workgroup, one (x, y) column each
constexpr int Z_PF = 8;       // planes requested ahead of the one being added
constexpr int YX_NT = 256;    // pair_yx_kernel: columns per workgroup, X halo included.  Measured at 1024^3, H = 10, one LoG
                              // scale: 128 / 192 / 256 / 320 / 384 columns 8.9 / 9.0 / 8.5-8.8 / 10.5 / 10.1 ms: three or more
                              // workgroups per CU, each in another phase of its turn, keep the SIMDs busy across the barriers
constexpr int YX_PF = 12;     // rows requested ahead, per filter (8 and 16 time the same)
constexpr int Z_CHUNK = 256;  // default march lengths; every chunk pays a 2H warm-up
constexpr int Y_CHUNK = 512;

#ifdef VH_PAIR_STAMPS   // development build (tools/build_variant.py only): where a wave of pair_yx_kernel spends its time
__device__ unsigned long long g_pair_stamps[8];
#define VH_STAMP(i) do { const unsigned long long t_ = __builtin_amdgcn_s_memtime(); st_acc[i] += t_ - st_last; st_last = t_; } while (0)
#else
#define VH_STAMP(i) do { } while (0)
#endif

// tap |j| of filter a and of filter b
template <int H>
struct PairTaps {
  float a[H + 1], b[H + 1];
};

template <int B, int E, class F>
__device__ __forceinline__ void static_for(F&& f) {
  if constexpr (B < E) {
    f(std::integral_constant<int, B>{});
    static_for<B + 1, E>(f);
  }
}

// The taps of both filters into VGPRs: a VALU instruction with an SGPR operand issues at half rate on gfx950
// (profiles/r02_microbench_valu.txt).  The empty asm keeps the compiler from folding the copies back into the scalars.
template <int H>
__device__ __forceinline__ void taps_to_vgprs(const PairTaps<H>& tp, float (&ta)[H + 1], float (&tb)[H + 1]) {
#pragma unroll
  for (int m = 0; m <= H; m++) {
    ta[m] = tp.a[m];
    tb[m] = tp.b[m];
    asm volatile("" : "+v"(ta[m]));
    asm volatile("" : "+v"(tb[m]));
  }
}

// One sample into the 2H+1 running sums of one filter at ring phase U: the sample is source i-j of the output in slot
// (U + H - j) mod W; slot U is complete afterwards, slot (U - 1) mod W has just been started.
template <int H, int U>
__device__ __forceinline__ void scatter(float (&ring)[2 * H + 1], const float (&t)[H + 1], float x) {
  constexpr int W = 2 * H + 1;
  float pr[H + 1];
#pragma unroll
  for (int m = 0; m <= H; m++) pr[m] = t[m] * x;
#pragma unroll
  for (int j = -H; j <= H; j++) {
    const int s = (U + H - j) % W;
    if (j == -H) ring[s] = pr[H];
    else ring[s] = ring[s] + pr[j < 0 ? -j : j];
    // the sum is formed HERE: left alone, the compiler sinks the adds of a slot towards the store that ends its chain, and
    // the products of 2H+1 samples stay live until then
    asm volatile("" : "+v"(ring[s]));
  }
}

// Launch 1.  Thread = one column of the [ny][nx] plane (the plane is contiguous, so columns are simply plane offsets and
// every load and store is coalesced; planes are below 2 GiB); blockIdx.y = chunk of output planes [zs, ze).  Step s of the march takes source plane
// ze-1+H-s and completes output plane ze-1+2H-s; the step count is rounded up to whole turns of the ring, so that the
// unrolled body has no exits (the steps past the chunk load nothing and store nothing).
template <int H>
__global__ void __launch_bounds__(Z_NT, 4)
pair_z_kernel(const float* __restrict__ src, float* __restrict__ za, float* __restrict__ zb, PairTaps<H> tp, i64 plane, int nz,
              int zchunk) {
  constexpr int W = 2 * H + 1;
  const i64 c = (i64)blockIdx.x * Z_NT + threadIdx.x;
  if (c >= plane) return;   // (no barrier in this kernel)
  float ta[H + 1], tb[H + 1];
  taps_to_vgprs<H>(tp, ta, tb);
  const int zs = blockIdx.y * zchunk;
  const int ze = min(zs + zchunk, nz);
  const int nsteps = ze - zs + 2 * H;
  const int ktop = ze - 1 + H;
  const float* p = src + c;
  // The sample of step s.  Every step loads, from a plane clamped into the volume, and a plane outside it (zero extension)
  // turns into 0.0f where the value is used: a branch around the load would make every wait for an older load a wait for all.
  auto load = [&](int s) -> float { return p[(i64)min(max(ktop - s, 0), nz - 1) * plane]; };
  auto inside = [&](int s) -> bool { return ktop - s >= 0 && ktop - s < nz; };
  float ra[W], rb[W], q[Z_PF];
#pragma unroll
  for (int m = 0; m < W; m++) ra[m] = rb[m] = 0.0f;
#pragma unroll
  for (int i = 0; i < Z_PF; i++) q[i] = load(i);
#pragma nounroll   // (nor peeled: the queue's shifts are renamed away inside the unrolled body as it is)
  for (int nb = 0; nb < nsteps; nb += W) {
    static_for<0, W>([&](auto U) {
      constexpr int u = decltype(U)::value;
      const int s = nb + u;
      const float x = inside(s) ? q[0] : 0.0f;
#pragma unroll
      for (int i = 0; i + 1 < Z_PF; i++) q[i] = q[i + 1];
      q[Z_PF - 1] = load(s + Z_PF);
      scatter<H, u>(ra, ta, x);
      scatter<H, u>(rb, tb, x);
      // Buffer stores, non-temporal, without a branch: a step that completes no plane of this chunk stores through a
      // zero-length descriptor, which drops the store (as csrc/gauss_fused.hip masks its loads).  Behind a branch the two
      // stores would make every wait for the sample of a step a wait for the stores of the steps before it as well.
      const int z = ktop + H - s;
      const bool done = s >= 2 * H && z >= zs;
      const i64 o = done ? (i64)z * plane : 0;
      const int len = done ? (int)(plane * 4) : 0;
      const __amdgpu_buffer_rsrc_t sa = __builtin_amdgcn_make_buffer_rsrc((void*)(za + o), 0, len, 0x00020000);
      const __amdgpu_buffer_rsrc_t sb = __builtin_amdgcn_make_buffer_rsrc((void*)(zb + o), 0, len, 0x00020000);
      __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, ra[u]), sa, (int)c * 4, 0, 2);
      __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, rb[u]), sb, (int)c * 4, 0, 2);
      __builtin_amdgcn_sched_barrier(0);   // steps are scheduled one by one: interleaved, their products outlive the registers
    });
  }
}

// Launch 2.  A workgroup owns YX_NT adjacent x-columns of one z (the TX output columns of its tile and H halo columns on
// either side: the only halo of this route) and a chunk [ys, ye) of rows; every thread marches its column down in y with
// two rings, exactly as launch 1 marches in z.  One turn of the ring completes W rows of both filters, which go to LDS; the
// X pass then gathers the 2H+1 window as conv_row_kernel does, four adjacent outputs per task from 16-byte LDS reads,
// divides each filter by its normaliser and stores the difference.
//
// The X task reads nothing from global memory: the normaliser lines it needs, Dx over the tile and Dy over the chunk's rows,
// are parked in LDS once per workgroup (sKx, sKy), and the tasks are dealt over the quads of the tile that lie inside the
// image only (the last tile of a row is mostly outside it).  A wave all of whose columns lie outside the image has nothing
// to march: it zeroes its LDS columns once, requests nothing, and only joins the barriers and the X pass.
template <int H>
struct YxCfg {
  static constexpr int W = 2 * H + 1;
  static constexpr int XW = (2 * H + 4 + 3) / 4;          // 16-byte reads that cover the window of four outputs
  static constexpr int TX = YX_NT + 4 - 4 * XW;           // output columns per tile: the last task's reads end inside the row
  static constexpr int QPR = TX / 4;                      // tasks per row
  static constexpr int LDS = (int)sizeof(float) * (2 * W * YX_NT + 2 * TX + 2 * Y_CHUNK);
  static_assert(TX % 4 == 0 && TX + 2 * H <= YX_NT && TX > 0, "tile width");
  static_assert(LDS <= 64 * 1024, "LDS rows of both filters and the normaliser lines");
  static_assert(H > 8 || 4 * LDS <= 160 * 1024, "four workgroups per CU up to H = 8");
};

template <int H>
__global__ void __launch_bounds__(YX_NT, 3)
pair_yx_kernel(const float* __restrict__ za, const float* __restrict__ zb, float* __restrict__ dst, PairTaps<H> tp,
               const float* __restrict__ Da, const float* __restrict__ Db, i64 dz_offset, int nx, int ny, int ychunk,
               int xtiles, int ychunks, float scale, int vec_ok) {
  typedef YxCfg<H> C;
  constexpr int W = C::W;
  __shared__ __attribute__((aligned(16))) float sA[W][YX_NT];
  __shared__ __attribute__((aligned(16))) float sB[W][YX_NT];
  __shared__ __attribute__((aligned(16))) float sKx[2][C::TX];    // Dx of filter a | b over the tile's output columns
  __shared__ float sKy[2][Y_CHUNK];                               // Dy of filter a | b over the chunk's rows (ychunk <= Y_CHUNK)
#ifdef VH_PAIR_STAMPS
  unsigned long long st_acc[5] = {0, 0, 0, 0, 0};
  unsigned long long st_last = __builtin_amdgcn_s_memtime();
#endif
  float ta[H + 1], tb[H + 1];
  taps_to_vgprs<H>(tp, ta, tb);
  unsigned b = blockIdx.x;
  const int bx = b % xtiles;
  b /= xtiles;
  const int by = b % ychunks;
  const int z = b / ychunks;
  const int tid = threadIdx.x;
  const int x0 = bx * C::TX;
  const int xc = x0 - H + tid;   // this thread's column (LDS index tid)
  const bool col_ok = xc >= 0 && xc < nx;
  // the wave's first column is at or past the end of the row (its last one is never left of the image: x0 >= 0, H < 64)
  const bool idle = x0 - H + 64 * __builtin_amdgcn_readfirstlane(tid >> 6) >= nx;
  const int ys = by * ychunk;
  const int ye = min(ys + ychunk, ny);
  const int nsteps = ye - ys + 2 * H;
  const int ktop = ye - 1 + H;
  const i64 zoff = (i64)z * nx * ny;
  const float* pa = za + zoff + min(max(xc, 0), nx - 1);
  const float* pb = zb + zoff + min(max(xc, 0), nx - 1);
  // as in launch 1: every step loads, from a row and a column clamped into the image, and zero extension is applied on use
  auto row_off = [&](int s) -> i64 { return (i64)min(max(ktop - s, 0), ny - 1) * nx; };
  auto inside = [&](int s) -> bool { return col_ok && ktop - s >= 0 && ktop - s < ny; };
  float ra[W], rb[W], qa[YX_PF], qb[YX_PF];
#pragma unroll
  for (int m = 0; m < W; m++) ra[m] = rb[m] = 0.0f;
  if (!idle) {
#pragma unroll
    for (int i = 0; i < YX_PF; i++) {
      qa[i] = pa[row_off(i)];
      qb[i] = pb[row_off(i)];
    }
  } else {
#pragma unroll
    for (int i = 0; i < YX_PF; i++) qa[i] = qb[i] = 0.0f;
#pragma unroll
    for (int m = 0; m < W; m++) sA[m][tid] = sB[m][tid] = 0.0f;   // what marching zero extension would leave, up to the zero's sign
  }
  // normaliser lines of each filter: Dx | Dy | Dz(global)
  const float* Dax = Da; const float* Day = Da + nx; const float* Daz = Da + nx + ny + dz_offset;
  const float* Dbx = Db; const float* Dby = Db + nx; const float* Dbz = Db + nx + ny + dz_offset;
  const float daz = Daz[z], dbz = Dbz[z];
  if (tid < C::TX) {   // (visible to the X pass after the first turn's barrier)
    const int xi = min(x0 + tid, nx - 1);
    sKx[0][tid] = Dax[xi];
    sKx[1][tid] = Dbx[xi];
  }
  for (int i = tid; i < ye - ys; i += YX_NT) {
    sKy[0][i] = Day[ys + i];
    sKy[1][i] = Dby[ys + i];
  }
  float* const out_plane = dst + zoff;
  // X tasks: (row u, quad qd) = task / QV, task % QV over the QV quads of this tile inside the image, task = tid, tid + YX_NT,
  // ...: kept as a pair that is stepped, so that the (uniform) QV costs one division per kernel
  const int QV = min(C::QPR, (nx - x0 + 3) >> 2);
  const int u_first = tid / QV, q_first = tid - u_first * QV;
  const int u_step = YX_NT / QV, q_step = YX_NT - u_step * QV;

  // one X task: row u of the turn that began at step nb, outputs x0 + 4 qd .. + 3; LDS index of output x0 + i is i + H
  auto x_task = [&](int u, int qd, int nb) {
    const int s = nb + u;
    const int y = ktop + H - s;
    const int x = x0 + 4 * qd;
    if (s < 2 * H || y < ys || x >= nx) return;
    float ga[4], gb[4];
    {
      float v[4 * C::XW];
#pragma unroll
      for (int k = 0; k < C::XW; k++) {
        const float4 t4 = *reinterpret_cast<const float4*>(&sA[u][4 * qd + 4 * k]);
        v[4 * k] = t4.x; v[4 * k + 1] = t4.y; v[4 * k + 2] = t4.z; v[4 * k + 3] = t4.w;
      }
#pragma unroll
      for (int jj = 0; jj < W; jj++) {   // j = jj - H ascending <=> window index descending
        const float t = ta[jj < H ? H - jj : jj - H];
#pragma unroll
        for (int k = 0; k < 4; k++) {
          const float term = t * v[2 * H - jj + k];
          ga[k] = jj == 0 ? term : ga[k] + term;
        }
      }
    }
    {
      float v[4 * C::XW];
#pragma unroll
      for (int k = 0; k < C::XW; k++) {
        const float4 t4 = *reinterpret_cast<const float4*>(&sB[u][4 * qd + 4 * k]);
        v[4 * k] = t4.x; v[4 * k + 1] = t4.y; v[4 * k + 2] = t4.z; v[4 * k + 3] = t4.w;
      }
#pragma unroll
      for (int jj = 0; jj < W; jj++) {
        const float t = tb[jj < H ? H - jj : jj - H];
#pragma unroll
        for (int k = 0; k < 4; k++) {
          const float term = t * v[2 * H - jj + k];
          gb[k] = jj == 0 ? term : gb[k] + term;
        }
      }
    }
    const float4 ka = *reinterpret_cast<const float4*>(&sKx[0][4 * qd]);
    const float4 kb = *reinterpret_cast<const float4*>(&sKx[1][4 * qd]);
    const float dxa[4] = {ka.x, ka.y, ka.z, ka.w}, dxb[4] = {kb.x, kb.y, kb.z, kb.w};
    const float day = sKy[0][y - ys], dby = sKy[1][y - ys];
    // the sums started from their first product: +0.0 once restores the reference's zero signs (see the header)
    float da[4], db[4];
    bool ones_a = true, ones_b = true;
#pragma unroll
    for (int k = 0; k < 4; k++) {
      ga[k] = ga[k] + 0.0f;
      gb[k] = gb[k] + 0.0f;
      da[k] = (dxa[k] * day) * daz;   // (Dx*Dy) first, then *Dz (filter3d.hpp:1016-1018)
      db[k] = (dxb[k] * dby) * dbz;
      ones_a = ones_a && da[k] == 1.0f;
      ones_b = ones_b && db[k] == 1.0f;
    }
    // x / 1.0f is x for every x: where every divisor of a filter is exactly 1 in the whole wave (the interior, for about half
    // of all filters) its divisions are skipped, as the single sweep's wave_one does; each filter on its own, so that a scale
    // with one such filter divides half as often
    if (__builtin_amdgcn_ballot_w64(!ones_a) != 0ull) {
#pragma unroll
      for (int k = 0; k < 4; k++) ga[k] = ga[k] / da[k];
    }
    if (__builtin_amdgcn_ballot_w64(!ones_b) != 0ull) {
#pragma unroll
      for (int k = 0; k < 4; k++) gb[k] = gb[k] / db[k];
    }
    float r[4];
#pragma unroll
    for (int k = 0; k < 4; k++) {   // the DoG/LoG epilogue (filter3d.hpp:1387-1390, :1495-1498): two roundings
      const float dd = ga[k] - gb[k];
      r[k] = dd * scale;
    }
    float* o = out_plane + (i64)y * nx + x;
    if (vec_ok && x + 3 < nx) {
      typedef float v4f __attribute__((ext_vector_type(4)));
      const v4f r4 = {r[0], r[1], r[2], r[3]};
      __builtin_nontemporal_store(r4, reinterpret_cast<v4f*>(o));
    } else {
#pragma unroll
      for (int k = 0; k < 4; k++)
        if (x + k < nx) __builtin_nontemporal_store(r[k], &o[k]);
    }
  };
  auto march_step = [&](auto U, int nb) {
    constexpr int u = decltype(U)::value;
    const int s = nb + u;
    const bool in = inside(s);
    const float xa = in ? qa[0] : 0.0f, xb = in ? qb[0] : 0.0f;
#pragma unroll
    for (int i = 0; i + 1 < YX_PF; i++) { qa[i] = qa[i + 1]; qb[i] = qb[i + 1]; }
    qa[YX_PF - 1] = pa[row_off(s + YX_PF)];
    qb[YX_PF - 1] = pb[row_off(s + YX_PF)];
    scatter<H, u>(ra, ta, xa);
    scatter<H, u>(rb, tb, xb);
    sA[u][tid] = ra[u];   // row y = ktop + H - s of this turn (not an output row while s < 2H or y < ys)
    sB[u][tid] = rb[u];
    __builtin_amdgcn_sched_barrier(0);   // (as in launch 1)
  };

  VH_STAMP(0);
#pragma nounroll
  for (int nb = 0; nb < nsteps; nb += W) {
    if (!idle) static_for<0, W>([&](auto U) { march_step(U, nb); });
    VH_STAMP(1);
    __syncthreads();
    VH_STAMP(2);
    // X pass over the W rows of this turn, at a raised issue priority: the waves that are in it hold their whole workgroup
    // at the second barrier, so they go before the marching waves of the other workgroups on the SIMD
    __builtin_amdgcn_s_setprio(2);
    for (int u = u_first, qd = q_first; u < W;) {
      x_task(u, qd, nb);
      u += u_step;
      qd += q_step;
      if (qd >= QV) { qd -= QV; u++; }
    }
    __builtin_amdgcn_s_setprio(0);
    VH_STAMP(3);
    __syncthreads();   // the rows are overwritten by the next turn
    VH_STAMP(4);
  }
#ifdef VH_PAIR_STAMPS
  if ((tid & 63) == 0) {
#pragma unroll
    for (int i = 0; i < 5; i++) atomicAdd(&g_pair_stamps[i], st_acc[i]);
  }
#endif
}

// Which half-widths take the route under log_pair = 1: filled from tools/log_pair_time.py (profiles/pair_yx_time.txt: one LoG
// scale at 1024^3, H = 6 / 7 / 8 / 9 / 10: -1.4 / -1.9 / -2.2 / -5.7 / -6.0 ms against spreads below 0.2 ms).  H = 5 is not
// instantiated: its single sweeps take 2.6-2.9 ms each, the route's two launches would have to fit into 5.5 ms.
constexpr int PAIR_H_MIN = 6, PAIR_H_MAX = 10;
const bool kPairWins[PAIR_H_MAX + 1] = {false, false, false, false, false, false, /*6*/ true, /*7*/ true, /*8*/ true,
                                        /*9*/ true, /*10*/ true};

bool bit_symmetric(const Taps& T) {
  for (int j = 1; j <= T.h; j++)
    if (std::memcmp(&T.t[T.h + j], &T.t[T.h - j], sizeof(float)) != 0) return false;
  return true;
}
bool same_bits(const Taps& A, const Taps& B) {
  return A.h == B.h && std::memcmp(A.t, B.t, sizeof(float) * (2 * A.h + 1)) == 0;
}

template <int H>
int launch_pair(visfd_hip_ctx* ctx, const LogPairRequest& rq, const float* Da, const float* Db) {
  typedef YxCfg<H> C;
  const i64 nx = rq.nx, ny = rq.ny, nz = rq.nz, plane = nx * ny, n = plane * nz;
  float *za = nullptr, *zb = nullptr;
  VH_TRY(ws(ctx, WS_A, (size_t)n, &za));
  VH_TRY(ws(ctx, WS_B, (size_t)n, &zb));
  PairTaps<H> tz, tyx;
  for (int m = 0; m <= H; m++) {
    tz.a[m] = rq.a[2].t[H + m];  tz.b[m] = rq.b[2].t[H + m];
    tyx.a[m] = rq.a[0].t[H + m]; tyx.b[m] = rq.b[0].t[H + m];
  }
  const int opt_chunk = ctx->opt.log_pair_chunk;
  i64 zchunk = opt_chunk > 0 ? opt_chunk : Z_CHUNK;
  if ((nz + zchunk - 1) / zchunk > 65535) zchunk = (nz + 65534) / 65535;   // chunks ride in blockIdx.y
  const i64 zblocks = (plane + Z_NT - 1) / Z_NT, zchunks = (nz + zchunk - 1) / zchunk;
  const i64 ychunk = opt_chunk > 0 && opt_chunk < Y_CHUNK ? opt_chunk : Y_CHUNK;   // (the kernel parks Dy of a chunk in LDS)
  const i64 xtiles = (nx + C::TX - 1) / C::TX, ychunks = (ny + ychunk - 1) / ychunk;
  const i64 yxblocks = xtiles * ychunks * nz;
  if (zblocks > 0x7fffffffLL || yxblocks > 0x7fffffffLL) return fail(VISFD_HIP_EINVAL, "volume too large for one launch");
  pair_z_kernel<H><<<dim3((unsigned)zblocks, (unsigned)zchunks), dim3(Z_NT), 0, ctx->stream>>>(rq.src, za, zb, tz, plane, (int)nz,
                                                                                                (int)zchunk);
  VH_HIP(hipGetLastError());
  const int vec_ok = ((nx & 3) == 0) && ((reinterpret_cast<uintptr_t>(rq.dst) & 15) == 0);
  pair_yx_kernel<H><<<dim3((unsigned)yxblocks), dim3(YX_NT), 0, ctx->stream>>>(za, zb, rq.dst, tyx, Da, Db, rq.z_lo, (int)nx, (int)ny,
                                                                                (int)ychunk, (int)xtiles, (int)ychunks, rq.scale,
                                                                                vec_ok);
  VH_HIP(hipGetLastError());
#ifdef VH_PAIR_STAMPS
  {
    unsigned long long st8[8], z8[8] = {};
    VH_HIP(hipStreamSynchronize(ctx->stream));
    VH_HIP(hipMemcpyFromSymbol(st8, HIP_SYMBOL(g_pair_stamps), sizeof(st8)));
    double tot = 0;
    for (int i = 0; i < 5; i++) tot += (double)st8[i];
    fprintf(stderr, "[pair_yx stamps H=%d] share of wave time: prologue %.3f | march %.3f | wait at barrier 1 %.3f | X tasks %.3f | "
            "wait at barrier 2 %.3f  (total %.4g ticks over %lld waves)\n", H, st8[0] / tot, st8[1] / tot, st8[2] / tot, st8[3] / tot,
            st8[4] / tot, tot, (long long)yxblocks * (YX_NT / 64));
    VH_HIP(hipMemcpyToSymbol(HIP_SYMBOL(g_pair_stamps), z8, sizeof(z8)));
  }
#endif
  return VISFD_HIP_OK;
}

}  // namespace

// Both Gaussians of an unmasked, normalised DoG/LoG scale, or GAUSS_DECLINED with nothing launched: the caller then runs the
// two Gaussians one after the other as before.  Applies to one half-width H = 6..10 on the three axes, taps symmetric bit
// for bit, the same taps along x and y (one set of tap registers serves both passes of launch 2), planes below 2 GiB.
int log_pair_route(visfd_hip_ctx* ctx, const LogPairRequest& rq) {
  const int mode = ctx->opt.log_pair;
  const int H = rq.a[0].h;
  if (mode == 0 || ctx->opt.gauss_3pass || H < PAIR_H_MIN || H > PAIR_H_MAX) return GAUSS_DECLINED;
  if (mode == 1 && !kPairWins[H]) return GAUSS_DECLINED;
  if (rq.nx <= 0 || rq.ny <= 0 || rq.nz <= 0 || rq.nx * rq.ny >= (1LL << 29) || rq.nz >= (1LL << 31)) return GAUSS_DECLINED;
  for (int d = 0; d < 3; d++)
    if (rq.a[d].h != H || rq.b[d].h != H || !bit_symmetric(rq.a[d]) || !bit_symmetric(rq.b[d])) return GAUSS_DECLINED;
  if (!same_bits(rq.a[0], rq.a[1]) || !same_bits(rq.b[0], rq.b[1])) return GAUSS_DECLINED;
  const i64 nz_global = rq.nz_global ? rq.nz_global : rq.nz;
  const i64 lines = rq.nx + rq.ny + nz_global;
  float* D = nullptr;
  VH_TRY(ws(ctx, WS_NORM, (size_t)(2 * lines), &D));
  VH_TRY(dev_norm_lines(ctx, D, rq.nx, rq.ny, nz_global, rq.a[0], rq.a[1], rq.a[2]));
  VH_TRY(dev_norm_lines(ctx, D + lines, rq.nx, rq.ny, nz_global, rq.b[0], rq.b[1], rq.b[2]));
  switch (H) {
    case 6: return launch_pair<6>(ctx, rq, D, D + lines);
    case 7: return launch_pair<7>(ctx, rq, D, D + lines);
    case 8: return launch_pair<8>(ctx, rq, D, D + lines);
    case 9: return launch_pair<9>(ctx, rq, D, D + lines);
    default: return launch_pair<10>(ctx, rq, D, D + lines);
  }
}

}  // namespace vh
