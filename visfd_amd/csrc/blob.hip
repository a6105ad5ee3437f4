// blob.hip -- 4-D (x,y,z,scale) strict non-max / non-min scan of the scale-space blob detector
// (reference lib/visfd/feature.hpp:212-346).
//
// A voxel of the middle LoG volume is a minimum iff it is strictly smaller than all 80
// neighbours in (x,y,z,scale), all 26 spatial neighbours are inside the image and unmasked, the
// voxel itself is unmasked, its score is negative and passes the (absolute) threshold; maxima are
// symmetric (feature.hpp:231-304).  Float comparisons are exact, so indices match the reference
// bit-for-bit whenever the three LoG volumes do.
//
// Two kernels:
//   1. candidates: an HBM sweep of the MIDDLE volume only (4 B/voxel).  A wave owns 62 columns by 4 rows and marches
//      along z on its own (three planes requested ahead, no barrier, no LDS tile): the min and max of x-1, x, x+1 come
//      from the neighbouring lanes, three rows fold into the 3x3 values, and a three-plane register ring
//      gives the 3x3x3 box min/max.  A voxel is a candidate when it equals the box min (or max)
//      and passes the sign/threshold tests -- a non-strict superset of the 26-neighbour rule.
//      (The form before it staged 64 x 8 tiles in LDS, four planes per step behind two workgroup barriers, and ran at
//      3.1 TB/s with a third of its waves' time spent at those barriers and in the flush: profiles/blob_stall_stamps.txt.)
//   2. verify: one thread per candidate repeats the reference's exact test on all 80 neighbours
//      (strict comparisons, masks) and appends the survivors.
// LoG volumes are smooth, so candidates are a small fraction of the voxels and kernel 2 is cheap.
#include <algorithm>
#include <cstdlib>
#include <limits>
#include <type_traits>

#include "common.hpp"
#include "wave.hpp"

namespace vh {

namespace {

constexpr int BLOCK = 512;              // threads per workgroup of both kernels
constexpr int SWV = BLOCK / 64;         // candidate sweep: waves per workgroup, stacked in y; no wave ever waits for another
constexpr int SOX = 62;                 // output columns per wave (lanes 1..62; lanes 0 and 63 hold the x halo)
constexpr int SR = 4;                   // output rows per wave: SR + 2 rows are loaded per plane
constexpr int SPF = 3;                  // planes requested ahead (a multiple of 3: the plane ring is indexed statically)
constexpr int WCAP = 2 * SR * 64;       // candidate indices a wave parks in LDS between two flushes: a step's fit behind the mark
static_assert(SPF % 3 == 0, "the plane ring is indexed statically");

#ifdef VH_BLOB_STAMPS   // development build (tools/build_variant.py only): where a wave of the candidate sweep spends its time
__device__ unsigned long long g_blob_stamps[8];
#define VH_STAMP(i) do { const unsigned long long t_ = __builtin_amdgcn_s_memtime(); st_acc[i] += t_ - st_last; st_last = t_; } while (0)
#else
#define VH_STAMP(i) do { } while (0)
#endif

struct Cand {
  int ix, iy, iz;
  int kind;  // 0 = minimum, 1 = maximum
  float score;
};

template <int B, int E, class F>
__device__ __forceinline__ void static_for(F&& f) {
  if constexpr (B < E) {
    f(std::integral_constant<int, B>{});
    static_for<B + 1, E>(f);
  }
}

// the value of the lane below / above (DPP wave shifts; what lane 0 / lane 63 receive is never used)
__device__ __forceinline__ float lane_below(float v) {
  return __builtin_bit_cast(float, __builtin_amdgcn_mov_dpp(__builtin_bit_cast(int, v), 0x138, 0xf, 0xf, true));
}
__device__ __forceinline__ float lane_above(float v) {
  return __builtin_bit_cast(float, __builtin_amdgcn_mov_dpp(__builtin_bit_cast(int, v), 0x130, 0xf, 0xf, true));
}

// A WAVE owns SOX columns by SR rows and marches along z on its own, as the Z march of csrc/gauss_pair.hip does: no barrier
// and no LDS tile.  Per plane it loads its SR + 2 rows (64 columns: the outputs and one halo column on either side), takes
// the row-wise min and max of x-1, x, x+1 from its neighbouring lanes, folds three rows into the 3x3 values and keeps those
// of three planes in a register ring.  The eight waves of a workgroup are stacked in y, so the rows two of them share are
// requested on the same CU at about the same time.  Candidates (linear voxel indices) are parked in the wave's own LDS
// strip, counted in a scalar (ballots: no LDS atomic), and written out with ONE global atomic per flush: every wave of the
// grid adds to the same counter, and atomics on one address are served one at a time by L2.
__global__ void __launch_bounds__(BLOCK, 6)   // six waves per SIMD: three workgroups per CU
blob_candidates_kernel(const float* __restrict__ mid, const float* __restrict__ mask, int nx, int ny, int nz,
                       float min_thr, float max_thr, int zchunk, int tiles_x, int tiles_y,
                       unsigned long long* __restrict__ out, unsigned long long capacity,
                       unsigned long long* __restrict__ counter) {
  __shared__ unsigned long long buf[SWV][WCAP];
  unsigned b = blockIdx.x;
  const int tile_x = b % tiles_x;
  b /= tiles_x;
  const int tile_y = b % tiles_y;
  const int chunk = b / tiles_y;
  const int zs = max(1, chunk * zchunk), ze = min(nz - 1, (chunk + 1) * zchunk);  // interior planes only
  if (zs >= ze) return;
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int gx = tile_x * SOX + lane;                 // lane 0: the halo column left of the first output (x >= 0)
  const int yb = tile_y * (SWV * SR) + wave * SR;     // the halo row above this wave's first output row
  if (yb + 1 > ny - 2) return;                        // no interior row (no barrier in this kernel)
#ifdef VH_BLOB_STAMPS
  unsigned long long st_acc[4] = {0, 0, 0, 0};
  unsigned long long st_last = __builtin_amdgcn_s_memtime();
#endif
  const i64 plane = (i64)nx * ny;
  const bool col_ok = lane >= 1 && lane <= SOX && gx <= nx - 2;   // an interior column that this wave reports
  unsigned long long* const wbuf = buf[wave];

  // Raw buffer loads through one descriptor per plane (planes below 2 GiB: the host checks), the lane's column in the
  // vector offset and the row in the scalar one.  Every load is inside the volume and none sits in a branch (a conditional
  // load is closed by a full s_waitcnt at its join): a column or row past the image is clamped to the last one, a plane past
  // the chunk to plane ze.  What a clamped load returns only reaches face voxels and voxels outside the image, which are
  // never reported (feature.hpp:245-252).
  const int col_off = min(gx, nx - 1) * 4;   // BYTE offsets inside a plane
  int row_off[SR + 2];
#pragma unroll
  for (int r = 0; r < SR + 2; r++) row_off[r] = min(yb + r, ny - 1) * nx * 4;
  const int plane_bytes = (int)(plane * 4);
  auto fetch = [&](int z, float (&v)[SR + 2]) {
    const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc((void*)(mid + (i64)min(z, ze) * plane), 0, plane_bytes,
                                                                        0x00020000);
#pragma unroll
    for (int r = 0; r < SR + 2; r++) v[r] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rs, col_off, row_off[r], 0));
  };
  const int p0 = (yb + 1) * nx + gx;   // in-plane index of this lane's first output
  unsigned cnt = 0;   // candidates parked in wbuf: uniform
  auto flush = [&]() {
    unsigned long long base = 0;
    if (lane == 0) base = atomicAdd(counter, (unsigned long long)cnt);
    base = __shfl(base, 0);
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();   // the wave's LDS instructions complete in order: its appends are visible to all its lanes
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    for (unsigned i = lane; i < cnt; i += 64)
      if (base + i < capacity) out[base + i] = wbuf[i];
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    cnt = 0;
  };

  // 3x3 min / max and the centre value of three planes: slot t % 3 takes the plane that arrives at step t
  float m9n[3][SR], m9x[3][SR], ctr[3][SR];
#pragma unroll
  for (int k = 0; k < 3; k++)
#pragma unroll
    for (int j = 0; j < SR; j++) m9n[k][j] = m9x[k][j] = ctr[k][j] = 0.0f;
  float q[SPF][SR + 2];
#pragma unroll
  for (int i = 0; i < SPF; i++) {
    fetch(zs - 1 + i, q[i]);
    __builtin_amdgcn_sched_barrier(0);   // oldest plane first: the wait counts of the loop are those of its entry as well
  }
  const int nsteps = ze - zs + 2;   // planes zs-1 .. ze arrive; the step count is rounded up to whole turns of the queue
  VH_STAMP(0);
#pragma nounroll
  for (int nb = 0; nb < nsteps; nb += SPF) {
    static_for<0, SPF>([&](auto U) {
      constexpr int u = decltype(U)::value;
      constexpr int nxt = u % 3, cur = (u + 2) % 3, prv = (u + 1) % 3;
      const int t = nb + u;   // plane zs - 1 + t arrives; plane z = zs + t - 2 is decided
      float hn[SR + 2], hx[SR + 2], hc[SR + 2];
#pragma unroll
      for (int r = 0; r < SR + 2; r++) {
        const float v = q[u][r], lo = lane_below(v), hi = lane_above(v);
        hn[r] = fminf(fminf(lo, v), hi);
        hx[r] = fmaxf(fmaxf(lo, v), hi);
        hc[r] = v;
      }
      // the requests stay BEHIND the last use of the values they replace: hoisted above it, they land in other registers
      // and are copied into place at the loop's end, behind a wait for all of them
      __builtin_amdgcn_sched_barrier(0);
      fetch(zs - 1 + t + SPF, q[u]);
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int j = 0; j < SR; j++) {
        m9n[nxt][j] = fminf(fminf(hn[j], hn[j + 1]), hn[j + 2]);
        m9x[nxt][j] = fmaxf(fmaxf(hx[j], hx[j + 1]), hx[j + 2]);
        // a copy of its own: left in the register it was loaded into, the centre value outlives the queue slot by two steps
        // and every slot's loads are moved into place at the loop's end, behind a wait for all of them
        asm volatile("v_mov_b32 %0, %1" : "=v"(ctr[nxt][j]) : "v"(hc[j + 1]));
      }
      VH_STAMP(1);
      const int z = zs + t - 2;
      if (t >= 2 && z < ze) {   // uniform
#pragma unroll
        for (int j = 0; j < SR; j++) {
          const int gy = yb + 1 + j;
          const float e = ctr[cur][j];
          const float bmin = fminf(fminf(m9n[prv][j], m9n[cur][j]), m9n[nxt][j]);
          const float bmax = fmaxf(fmaxf(m9x[prv][j], m9x[cur][j]), m9x[nxt][j]);
          const bool is_min = (e == bmin) && (e < 0.0f) && (e < min_thr);
          const bool is_max = (e == bmax) && (e > 0.0f) && (e > max_thr);
          const i64 v = (i64)z * plane + (p0 + j * nx);
          bool cand = col_ok && gy <= ny - 2 && (is_min || is_max);
          if (cand && mask && mask[v] == 0.0f) cand = false;
          const unsigned long long bal = __ballot(cand);
          if (bal != 0ull) {   // uniform
            if (cand) wbuf[cnt + (unsigned)wave_rank(bal, lane)] = (unsigned long long)v;
            cnt += (unsigned)__popcll(bal);
          }
        }
        VH_STAMP(2);
        if (cnt > (unsigned)(WCAP - SR * 64)) {   // the next step might not fit
          flush();
          VH_STAMP(3);
        }
      }
    });
  }
  if (cnt) flush();
  VH_STAMP(3);
#ifdef VH_BLOB_STAMPS
  if (lane == 0) {
#pragma unroll
    for (int i = 0; i < 4; i++) atomicAdd(&g_blob_stamps[i], st_acc[i]);
  }
#endif
}

__global__ void __launch_bounds__(BLOCK)
blob_verify_kernel(const unsigned long long* __restrict__ cand_idx, const unsigned long long* __restrict__ n_cand_ptr,
                   unsigned long long cand_capacity,
                   const float* __restrict__ lo, const float* __restrict__ mid, const float* __restrict__ hi,
                   const float* __restrict__ mask, int nx, int ny, int nz, float min_thr, float max_thr,
                   Cand* __restrict__ out, unsigned long long capacity, unsigned long long* __restrict__ counter) {
  // the number of candidates is read on the device (no host round trip between the two kernels); an overflowed
  // candidate list is cut at its capacity here and reported by the host afterwards
  unsigned long long n_cand = *n_cand_ptr;
  if (n_cand > cand_capacity) n_cand = cand_capacity;
  for (unsigned long long t = (unsigned long long)blockIdx.x * BLOCK + threadIdx.x; t < n_cand;
       t += (unsigned long long)gridDim.x * BLOCK) {
  const i64 c = (i64)cand_idx[t];
  const i64 plane = (i64)nx * ny;
  const int iz = (int)(c / plane);
  const int rem = (int)(c - (i64)iz * plane);
  const int iy = rem / nx, ix = rem - iy * nx;
  const float e = mid[c];
  bool is_min = (e < 0.0f) && (e < min_thr);
  bool is_max = (e > 0.0f) && (e > max_thr);
  // the two other-scale values at the same position decide most candidates: test them first
  {
    const float a = lo[c], b = hi[c];
    if (a <= e || b <= e) is_min = false;
    if (a >= e || b >= e) is_max = false;
  }
  const float* vol[3] = {mid, lo, hi};
  for (int r = 0; r < 3 && (is_min || is_max); r++) {
    const float* v = vol[r];
    for (int jz = -1; jz <= 1; jz++)
      for (int jy = -1; jy <= 1; jy++) {
        const i64 row = c + (i64)jz * plane + (i64)jy * nx;
#pragma unroll
        for (int jx = -1; jx <= 1; jx++) {
          if (r == 0 && jz == 0 && jy == 0 && jx == 0) continue;
          const i64 q = row + jx;
          if (mask && r == 0 && mask[q] == 0.0f) { is_min = false; is_max = false; }
          const float nb = v[q];
          if (nb <= e) is_min = false;
          if (nb >= e) is_max = false;
        }
      }
  }
  if (is_min || is_max) {
    const unsigned long long slot = atomicAdd(counter, 1ULL);
    if (slot < capacity) {
      Cand cd;
      cd.ix = ix; cd.iy = iy; cd.iz = iz;
      cd.kind = is_min ? 0 : 1;
      cd.score = e;
      out[slot] = cd;
    }
  }
  }   // next candidate of this thread
}

}  // namespace

// The scan of one scale in two halves, so that a caller can queue the next scale's filters before it waits for
// this scale's list (BlobDog runs a dozen scales back to back): blob_scan_launch only enqueues the two kernels on
// the context's stream (buffer set 0 or 1: candidate codes, survivors, counters) and records an event;
// blob_scan_collect waits for that event on an auxiliary stream, copies the survivors to the host there (the main
// stream keeps running), sorts them and appends them to the lists; *overflow tells that a buffer overflowed (the caller
// then repeats the scale with dev_blob_scan, which grows the buffers).  Any call of the context may come between the
// two: the launch records where it writes and how much fits (ScanPending), the collect reads only that record, and
// whatever would free or overwrite those buffers collects first (blob_jobs_drain, common.hpp).
struct ScanBufs {
  unsigned long long* idx = nullptr;
  Cand* cand = nullptr;
  unsigned long long* counters = nullptr;   // [0]: candidates, [1]: verified
  size_t cap_idx = 0, cap_out = 0;
};

static int scan_bufs(visfd_hip_ctx* ctx, int set, ScanBufs* B, bool pipelined, i64 nvox) {
  // at least 4 M candidates / 1 M survivors, and room for 1 voxel in 32 / 128 (noise volumes at 1024^3 give ~1 in
  // 100 / 1 in 4000 per scale): the pipelined scan then does not overflow on its first call
  constexpr size_t NSET = 3;   // buffer sets of the pipelined scan (blob_job.hip: BlobJob::NSET)
  size_t cap_idx = ctx->slot_bytes[WS_TVAUX] / sizeof(unsigned long long) / NSET;
  if (cap_idx < (1u << 22)) cap_idx = 1u << 22;
  if (cap_idx < (size_t)(nvox / 32)) cap_idx = (size_t)(nvox / 32);
  size_t cap_out = ctx->slot_bytes[WS_CAND] / sizeof(Cand) / NSET;
  if (cap_out < (1u << 20)) cap_out = 1u << 20;
  if (cap_out < (size_t)(nvox / 128)) cap_out = (size_t)(nvox / 128);
  unsigned long long* idx = nullptr;
  Cand* cand = nullptr;
  unsigned long long* counters = nullptr;
  VH_TRY(ws(ctx, WS_TVAUX, NSET * cap_idx, &idx));
  VH_TRY(ws(ctx, WS_CAND, NSET * cap_out, &cand));
  VH_TRY(ws(ctx, WS_SCANCNT, 8, &counters));   // (2 words per set)
  B->idx = idx + (size_t)set * cap_idx;
  B->cand = cand + (size_t)set * cap_out;
  B->counters = counters + 2 * set;
  B->cap_idx = cap_idx;
  B->cap_out = cap_out;
  if (pipelined) {   // test hook: pretend the buffers of the pipelined form are tiny, so that its overflow path runs
    if (ctx->opt.blob_test_cap > 0) {
      const size_t v = (size_t)ctx->opt.blob_test_cap;
      if (v < B->cap_idx) B->cap_idx = v;
      if (v < B->cap_out) B->cap_out = v;
    }
  }
  return VISFD_HIP_OK;
}

static void sort_and_append(std::vector<Cand>& h, i64 nx, i64 ny, int scale_index, float sigma,
                            std::vector<visfd_hip_blob>* minima, std::vector<visfd_hip_blob>* maxima) {
  // deterministic order (the device appends in arrival order): by (iz, iy, ix), i.e. by linear voxel index.
  // LSD radix sort of (index, position) pairs: lists reach 250 k entries per scale at 1024^3, where a
  // comparison sort of the records cost 12 ms.
  const size_t m = h.size();
  std::vector<unsigned long long> key(m), key2(m);
  std::vector<unsigned int> pos(m), pos2(m);
  unsigned long long maxkey = 0;
  for (size_t i = 0; i < m; i++) {
    key[i] = (unsigned long long)(((i64)h[i].iz * ny + h[i].iy) * nx + h[i].ix);
    pos[i] = (unsigned int)i;
    if (key[i] > maxkey) maxkey = key[i];
  }
  constexpr int RB = 11;
  for (int shift = 0; shift < 64 && (maxkey >> shift) != 0; shift += RB) {
    size_t hist[(1 << RB) + 1] = {0};
    for (size_t i = 0; i < m; i++) hist[((key[i] >> shift) & ((1u << RB) - 1)) + 1]++;
    for (int b = 0; b < (1 << RB); b++) hist[b + 1] += hist[b];
    for (size_t i = 0; i < m; i++) {
      const size_t d = hist[(key[i] >> shift) & ((1u << RB) - 1)]++;
      key2[d] = key[i];
      pos2[d] = pos[i];
    }
    key.swap(key2);
    pos.swap(pos2);
  }
  for (size_t i = 0; i < m; i++) {
    const Cand& cd = h[pos[i]];
    visfd_hip_blob bl;
    bl.ix = cd.ix; bl.iy = cd.iy; bl.iz = cd.iz;
    bl.scale = scale_index;
    bl.sigma = sigma;
    bl.score = cd.score;
    (cd.kind == 0 ? minima : maxima)->push_back(bl);
  }
}

static int scan_enqueue(visfd_hip_ctx* ctx, const ScanBufs& B, const float* lo, const float* mid, const float* hi,
                        const float* mask, i64 nx, i64 ny, i64 nz, float min_thr, float max_thr) {
  hipStream_t st = ctx->stream;
  if (nx * ny >= (1LL << 29)) return fail(VISFD_HIP_EINVAL, "planes of 2 GiB and more are not supported by the blob scan");
  // interior columns 1 .. nx-2 in strips of SOX, interior rows 1 .. ny-2 in bands of SWV * SR
  const int tiles_x = (int)std::max<i64>(1, (nx - 2 + SOX - 1) / SOX);
  const int tiles_y = (int)std::max<i64>(1, (ny - 2 + SWV * SR - 1) / (SWV * SR));
  const i64 tiles = (i64)tiles_x * tiles_y;
  i64 want_chunks = ((i64)ctx->num_cus * 16 + tiles - 1) / tiles;
  if (want_chunks < 1) want_chunks = 1;
  i64 zchunk = (nz + want_chunks - 1) / want_chunks;
  if (zchunk < 16) zchunk = 16;
  const i64 nchunks = (nz + zchunk - 1) / zchunk;
  const i64 nblocks = tiles * nchunks;
  if (nblocks > 0x7fffffffLL) return fail(VISFD_HIP_EINVAL, "volume too large for one launch");
  VH_HIP(hipMemsetAsync(B.counters, 0, 2 * sizeof(unsigned long long), st));
  blob_candidates_kernel<<<dim3((unsigned)nblocks), dim3(BLOCK), 0, st>>>(
      mid, mask, (int)nx, (int)ny, (int)nz, min_thr, max_thr, (int)zchunk, tiles_x, tiles_y, B.idx,
      (unsigned long long)B.cap_idx, B.counters);
  VH_HIP(hipGetLastError());
  blob_verify_kernel<<<dim3((unsigned)(ctx->num_cus * 8)), dim3(BLOCK), 0, st>>>(
      B.idx, B.counters, (unsigned long long)B.cap_idx, lo, mid, hi, mask, (int)nx, (int)ny, (int)nz, min_thr, max_thr,
      B.cand, (unsigned long long)B.cap_out, B.counters + 1);
  VH_HIP(hipGetLastError());
#ifdef VH_BLOB_STAMPS
  {
    unsigned long long st8[8], z8[8] = {};
    VH_HIP(hipStreamSynchronize(st));
    VH_HIP(hipMemcpyFromSymbol(st8, HIP_SYMBOL(g_blob_stamps), sizeof(st8)));
    double tot = 0;
    for (int i = 0; i < 4; i++) tot += (double)st8[i];
    fprintf(stderr, "[blob scan stamps] share of wave time: prologue %.3f | wait for the plane + row and 3x3 extrema + requests %.3f | "
            "tests + append %.3f | flush %.3f  (total %.4g ticks)\n", st8[0] / tot, st8[1] / tot, st8[2] / tot, st8[3] / tot, tot);
    VH_HIP(hipMemcpyToSymbol(HIP_SYMBOL(g_blob_stamps), z8, sizeof(z8)));
  }
#endif
  return VISFD_HIP_OK;
}

int blob_scan_launch(visfd_hip_ctx* ctx, const BlobJob* owner, int set, hipEvent_t done, const float* lo, const float* mid,
                     const float* hi, const float* mask, i64 nx, i64 ny, i64 nz, float min_thr, float max_thr,
                     ScanPending* pending) {
  VH_TRY(blob_jobs_drain(ctx, owner));   // the buffer sets and counters are the context's: another job's pending lists first
  ScanBufs B;
  VH_TRY(scan_bufs(ctx, set, &B, true, nx * ny * nz));
  VH_TRY(scan_enqueue(ctx, B, lo, mid, hi, mask, nx, ny, nz, min_thr, max_thr));
  VH_HIP(hipEventRecord(done, ctx->stream));
  // the candidate codes (B.idx) are not recorded: only the two kernels just queued read them, and the stream orders
  // every later user of WS_TVAUX behind those (ws_get waits for the stream before it frees a slot)
  pending->counters = B.counters;
  pending->survivors = B.cand;
  pending->cap_idx = B.cap_idx;
  pending->cap_out = B.cap_out;
  return VISFD_HIP_OK;
}

int blob_scan_collect(visfd_hip_ctx* ctx, const ScanPending& B, hipEvent_t done, hipStream_t aux, i64 nx, i64 ny,
                      int scale_index,
                      float sigma, std::vector<visfd_hip_blob>* minima, std::vector<visfd_hip_blob>* maxima,
                      bool* overflow) {
  // only what the launch recorded: slot sizes, options and the slots themselves may have changed since (blob_jobs_drain
  // runs before anything frees or overwrites what `B` points to)
  *overflow = false;
  VH_HIP(hipStreamWaitEvent(aux, done, 0));
  unsigned long long c2[2] = {0, 0};
  VH_HIP(hipMemcpyAsync(c2, B.counters, sizeof(c2), hipMemcpyDeviceToHost, aux));
  VH_HIP(hipStreamSynchronize(aux));
  if (ctx->opt.debug) fprintf(stderr, "[blob scan] scale %d: %llu candidates, %llu blobs\n", scale_index, c2[0], c2[1]);
  if (c2[0] > B.cap_idx || c2[1] > B.cap_out) { *overflow = true; return VISFD_HIP_OK; }
  std::vector<Cand> h((size_t)c2[1]);
  if (c2[1]) {
    VH_HIP(hipMemcpyAsync(h.data(), B.survivors, sizeof(Cand) * (size_t)c2[1], hipMemcpyDeviceToHost, aux));
    VH_HIP(hipStreamSynchronize(aux));
  }
  sort_and_append(h, nx, ny, scale_index, sigma, minima, maxima);
  return VISFD_HIP_OK;
}

// One scale, synchronously (also the fallback of the pipelined form: grows its buffers until the lists fit).
int dev_blob_scan(visfd_hip_ctx* ctx, const float* lo, const float* mid, const float* hi,
                  const float* mask, i64 nx, i64 ny, i64 nz, int scale_index, float sigma,
                  float min_thr, float max_thr, bool want_min, bool want_max,
                  std::vector<visfd_hip_blob>* minima, std::vector<visfd_hip_blob>* maxima) {
  if (nx < 3 || ny < 3 || nz < 3) return VISFD_HIP_OK;  // no interior voxels: nothing can be a blob
  if (nx >= (1LL << 31) || ny >= (1LL << 31) || nz >= (1LL << 31))
    return fail(VISFD_HIP_EINVAL, "dimension too large");
  const float inf = std::numeric_limits<float>::infinity();
  if (!want_min) min_thr = -inf;   // nothing is < -inf
  if (!want_max) max_thr = inf;
  hipStream_t st = ctx->stream;
  VH_TRY(blob_jobs_drain(ctx));   // set 0 and its counters may hold a pending scan of a job (never the caller's: `end` collects first)
  for (int attempt = 0; attempt < 4; attempt++) {
    ScanBufs B;
    VH_TRY(scan_bufs(ctx, 0, &B, false, nx * ny * nz));
    VH_TRY(scan_enqueue(ctx, B, lo, mid, hi, mask, nx, ny, nz, min_thr, max_thr));
    unsigned long long c2[2] = {0, 0};
    VH_HIP(hipMemcpyAsync(c2, B.counters, sizeof(c2), hipMemcpyDeviceToHost, st));
    VH_HIP(hipStreamSynchronize(st));
    if (ctx->opt.debug) fprintf(stderr, "[blob scan] scale %d: %llu candidates\n", scale_index, c2[0]);
    if (c2[0] > B.cap_idx) {   // rare: grow and rescan
      unsigned long long* p = nullptr;
      VH_TRY(ws(ctx, WS_TVAUX, 3 * (size_t)c2[0] + 16, &p));   // (a third of the slot per buffer set: scan_bufs)
      continue;
    }
    if (c2[1] > B.cap_out) {
      Cand* p = nullptr;
      VH_TRY(ws(ctx, WS_CAND, 3 * (size_t)c2[1] + 16, &p));
      continue;
    }
    std::vector<Cand> h((size_t)c2[1]);
    if (c2[1]) {
      VH_HIP(hipMemcpyAsync(h.data(), B.cand, sizeof(Cand) * (size_t)c2[1], hipMemcpyDeviceToHost, st));
      VH_HIP(hipStreamSynchronize(st));
    }
    sort_and_append(h, nx, ny, scale_index, sigma, minima, maxima);
    return VISFD_HIP_OK;
  }
  return fail(VISFD_HIP_EDEVICE, "blob candidate list kept overflowing");
}

}  // namespace vh
