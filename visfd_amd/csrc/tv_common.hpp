// tv_common.hpp -- what the tensor-voting translation units (tv.hip, tv_tiled.hip, tv_box.hip, tv_list.hip) share: the
// geometry of the vote tables, the launch plan of the persistent kernels, and the routes' declarations.
#pragma once

#include <algorithm>

#include "common.hpp"

namespace vh {

// A route's third answer besides VISFD_HIP_OK (it ran) and an error code (all positive): it does not take this request, or
// gave up before it wrote anything, and the next route is tried (tv.hip: tv_dispatch).  VH_TRY passes it up like an error.
// A route that declines after it had started leaves no error set (set_error(""), hipGetLastError()).
constexpr int TV_DECLINED = -1;

// ---- the vote tables ----------------------------------------------------------------------------------------------------
// row stride (in float4 entries) of the tiled kernel's vote table: 2h+1 rounded up to 4 modulo 8 (tv_tiled.hip: LDS banks)
inline int tv_padded_row(int h) {
  int sp = 2 * h + 1;
  while ((sp & 7) != 4) sp++;
  return sp;
}

// vote table of tv_box.hip: a slice has 3 zero rows above and below its 2h+1 rows and rows of
// tv_box_row(h) entries -- at least 3 zero entries behind the 2h+1 of a row, 4 modulo 8 (LDS banks) -- behind 4 guard
// entries: entry (jy, jx) of slice jz at 4 + (jy + h + 3) * row + (jx + h); everything else is zero, so that the receivers
// of a 4 x 4 sub-patch a sender does not reach read a zero weight
inline int tv_box_row(int h) {
  int sp = 2 * h + 1 + 3;
  while ((sp & 7) != 4) sp++;
  return sp;
}
inline int tv_box_slice(int h) { return (2 * h + 1 + 6) * tv_box_row(h) + 8; }

// The five tables of one (sigma_tv, cutoff) in ONE device buffer (tv.hip: tv_table_device), n = 2h+1, float4 entries:
//   packed     n^3                   the reference's {w, rhat} (baseline kernel)
//   padded     n^2 tv_padded_row     the same with padded rows (tiled kernel; pad entries are never read)
//   box_tol    (n+1) tv_box_slice    {w, sqrt(2) rhat} in the slice layout above (tolerance kernel), then a slice of zeros
//   box_exact  (n+1) tv_box_slice    {w, rhat} in that layout (exact box kernel), then a slice of zeros
//   box_tol_sq (n+1) tv_box_slice    box_tol with (float)sqrt((double)w) in w's place (tolerance kernel, exponent 4 with folded
//                                    saliencies: the 17-instruction vote of tv_box.hip), then a slice of zeros
// The zero rows, row tails and slices of the box tables ARE read.
struct TvTableLayout {
  size_t packed, padded, box_tol, box_exact, box_tol_sq;   // first entry of each table (its size: up to the next one)
  size_t total;
};
inline TvTableLayout tv_table_layout(int h) {
  const size_t n = 2 * (size_t)h + 1;
  TvTableLayout l;
  l.packed = 0;
  l.padded = l.packed + n * n * n;
  l.box_tol = l.padded + n * n * (size_t)tv_padded_row(h);
  l.box_exact = l.box_tol + (n + 1) * (size_t)tv_box_slice(h);
  l.box_tol_sq = l.box_exact + (n + 1) * (size_t)tv_box_slice(h);
  l.total = l.box_tol_sq + (n + 1) * (size_t)tv_box_slice(h);
  return l;
}
struct TvTables {
  const float4 *packed, *padded, *box_tol, *box_exact, *box_tol_sq;
  int h;
};

// ---- device helpers -----------------------------------------------------------------------------------------------------
// LDS (address space 3) pointers as 32-bit integers and back
__device__ __forceinline__ unsigned lds_addr(const void* p) {
  return (unsigned)(uintptr_t)(const __attribute__((address_space(3))) void*)p;
}
template <typename T>
__device__ __forceinline__ const __attribute__((address_space(3))) T* lds_ptr(unsigned a) {
  return (const __attribute__((address_space(3))) T*)(uintptr_t)a;
}

// The tile of tv_box.hip's kernels, which the sender lists of tv_list.hip are cut for (tv_tiled.hip has its own)
namespace box_tile {
constexpr int NT = 512;
constexpr int NW = NT / 64;
constexpr int TX = 16, TY = 4 * NW;    // a workgroup's tile of receivers: 16 x 32 on ONE pair of planes (z, z+1) per pass
}  // namespace box_tile

// ---- the launch plan of the persistent kernels (tv_tiled.hip, tv_box.hip) -----------------------------------------------
// Units of work: a tile over a run of zrun receiver planes (default_zrun, or option tv_zrun, cut to the range).  *nblk = 0:
// nothing to do.
inline int tv_plan_units(const visfd_hip_ctx* ctx, int default_zrun, int tiles_x, int tiles_y, i64 z_out0, i64 z_out1,
                         int* zrun, i64* nblk) {
  int zr = default_zrun;
  if (ctx->opt.tv_zrun >= 1 && ctx->opt.tv_zrun <= 4096) zr = ctx->opt.tv_zrun;   // tuning aid
  if ((i64)zr > z_out1 - z_out0) zr = (int)(z_out1 - z_out0);
  if (zr < 1) zr = 1;
  const i64 nruns = (z_out1 - z_out0 + zr - 1) / zr;
  *zrun = zr;
  *nblk = std::max<i64>((i64)tiles_x * tiles_y * nruns, 0);
  if (*nblk > 0x7fffffffLL) return fail(VISFD_HIP_EINVAL, "volume too large for one launch");
  return VISFD_HIP_OK;
}
// Persistent workgroups, each claiming units from a counter: as many as the chip holds at once.
inline i64 tv_plan_grid(const visfd_hip_ctx* ctx, size_t wg_per_cu, i64 nblk) {
  i64 ngrid = (i64)ctx->num_cus * (i64)wg_per_cu;
  // slab runs: workgroup slots left free for the transport's kernels while a halo is in flight (slab.hip) -- counted
  // against THIS kernel's own chip-filling grid
  if (ctx->opt.tv_reserve_wg > 0) ngrid = std::max<i64>(ngrid - ctx->opt.tv_reserve_wg, 1);
  if (ctx->opt.tv_max_wg > 0 && ngrid > ctx->opt.tv_max_wg) ngrid = ctx->opt.tv_max_wg;   // tests: many units per workgroup
  return std::min(ngrid, nblk);
}

// Sets a kernel's dynamic-LDS limit and launches it on the context's stream.
template <typename... KArgs, typename... Args>
inline int tv_launch_lds(visfd_hip_ctx* ctx, void (*kernel)(KArgs...), i64 ngrid, int nthreads, size_t lds, Args... args) {
  VH_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  kernel<<<dim3((unsigned)ngrid), dim3(nthreads), lds, ctx->stream>>>(args...);
  return VISFD_HIP_OK;
}

// ---- the routes (tv.hip tries them in order; each returns VISFD_HIP_OK, TV_DECLINED or an error) -------------------------
// tv_tiled.hip.  dtab: TvTables::padded
int dev_tv_tiled(visfd_hip_ctx* ctx, const float* sal, const float* dir, float* ten, const float* mask_src,
                 const float* mask_dst, i64 nx, i64 ny, i64 nz, i64 z_out0, i64 z_out1, int h, const float4* dtab, int exponent,
                 bool curves, bool weights_only);
// tv_box.hip.  dtab_box: TvTables::box_exact if exact, else TvTables::box_tol; dtab_box_sq: TvTables::box_tol_sq (not read if exact)
int dev_tv_box(visfd_hip_ctx* ctx, const float* sal, const float* dir, float* ten, const float* mask_src, const float* mask_dst,
               i64 nx, i64 ny, i64 nz, i64 z_out0, i64 z_out1, int h, const float4* dtab_box, const float4* dtab_box_sq, int exponent,
               bool exact);


// tv_list.hip: the launch-wide sender lists of tv_box.hip's kernels for the receiver planes [z_out0, z_out1) -- the planes
// [zl0, zl0 + nzl) they reach -- in WS_TVSCRATCH (entries) and WS_TVLIST (rows).  flags: what the count pass saw among the
// listed saliencies (times their mask values).
constexpr int TV_LIST_MAX_NX = 16384;       // a row's salient flags are a bit mask in LDS
constexpr unsigned TVL_NOT_POSITIVE = 1u;   // (rare: negative peak heights, masks with negative values, NaN)
constexpr unsigned TVL_NON_FINITE = 2u;
constexpr unsigned TVL_WEIGHTED_MASK = 4u;  // a source mask value other than 0 and 1
struct TvSenderLists {
  const float4* ent;      // {saliency (scaled), normal}, or {c, a n} if folded (tv_box.hip: vote_fma)
  const unsigned* pos;
  const unsigned* rows;
  unsigned long long total;
  unsigned flags;
  bool folded;
  int zl0, nzl;
};
// mode: the saliency's scaling -- 0: 1/4 (tolerance vote, exponent 4), 2: 1/2 (exponent 2), 1: none (exact vote).
// decline_on: flags with which the caller has no use for the lists (TV_DECLINED before they are written).
// may_fold: records are folded if every listed saliency is positive.
// Two halves around the caller's read of {total, flags} (dev_tv_box waits for it at once; api.hip's membrane_stage reads it
// together with other words and with more work queued behind them): tv_list_count queues the count pass and the scan,
// which leave the two in *total_dev and *flags_dev (device words zeroed by the caller, or among the 16 of `counter`, which
// are zeroed here); tv_list_write is everything after the read.
// thr_dev (nullable, device memory): sal is uncut, and only voxels with !(s < *thr_dev) are salient.
struct TvListGeo {
  int nx, ny, nz;
  int zl0, nzl;   // listed planes [zl0, zl0 + nzl)
  int ntx, h;
};
struct TvListPlan {
  TvListGeo g;
  unsigned* rows;
  unsigned row_blocks;
  int mode;
  const float* thr_dev;
};
int tv_list_count(visfd_hip_ctx* ctx, const float* sal, const float* thr_dev, const float* mask_src, i64 nx, i64 ny, i64 nz,
                  i64 z_out0, i64 z_out1, int h, int mode, unsigned* counter, unsigned long long* total_dev, unsigned* flags_dev,
                  TvListPlan* plan);
int tv_list_write(visfd_hip_ctx* ctx, const TvListPlan& plan, const float* sal, const float* dir, const float* mask_src,
                  unsigned long long total, unsigned flags, unsigned decline_on, bool may_fold, TvSenderLists* out);

// tv_box.hip in the same two halves: dev_tv_box_count checks the request as dev_tv_box does (TV_DECLINED before anything is
// queued) and queues the lists' count; dev_tv_box_vote writes the lists and votes.  dev_tv_box is the two around one read.
int dev_tv_box_count(visfd_hip_ctx* ctx, const float* sal, const float* thr_dev, const float* mask_src, i64 nx, i64 ny, i64 nz,
                     i64 z_out0, i64 z_out1, int h, int exponent, bool exact, unsigned long long* total_dev, unsigned* flags_dev,
                     TvListPlan* plan);
int dev_tv_box_vote(visfd_hip_ctx* ctx, const TvListPlan& plan, unsigned long long total, unsigned flags, const float* sal,
                    const float* dir, float* ten, const float* mask_src, const float* mask_dst, i64 nx, i64 ny, i64 nz, i64 z_out0,
                    i64 z_out1, int h, const float4* dtab_box, const float4* dtab_box_sq, int exponent, bool exact);

// tv.hip, for the queued membrane stage: the vote of the whole volume by the request's FIRST route, in those halves.
// dev_tv_stage_count returns TV_DECLINED (nothing queued) unless that route is a form of tv_box.hip that takes the request.
struct TvStagePlan {
  int h;
  bool exact;
  const float4 *dtab_box, *dtab_box_sq;
  TvListPlan lists;
};
int dev_tv_stage_count(visfd_hip_ctx* ctx, const float* sal, const float* thr_dev, const float* mask, i64 nx, i64 ny, i64 nz,
                       float sigma_tv, int exponent, float cutoff, unsigned long long* total_dev, unsigned* flags_dev,
                       TvStagePlan* plan);
int dev_tv_stage_vote(visfd_hip_ctx* ctx, const TvStagePlan& plan, unsigned long long total, unsigned flags, const float* sal,
                      const float* dir, float* ten, const float* mask, i64 nx, i64 ny, i64 nz, int exponent);

}  // namespace vh
