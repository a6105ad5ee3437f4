/* visfd_hip.h -- C ABI of libvisfd_hip.so: the MI355X (gfx950) implementation of VISFD's dense
 * 3-D filtering hot path (separable Gaussian -> DoG/LoG blob detection -> Hessian/eigen ridge
 * saliency -> dense stick tensor voting).
 *
 * This is the drop-in boundary.  The reference has no FFI layer: its interface
 * for this path is the header-only template API in namespace visfd plus the filter_mrc handlers.
 * Each entry point below names the reference function it replaces (file:line under the
 * reference root).  include/visfd_hip.hpp re-creates the visfd:: templates on top of this ABI
 * (float*** arguments), INTEGRATION.md shows the binding a maintainer adds.
 *
 * Conventions
 *  - plain C, no torch/STL types; every function returns 0 on success or a VISFD_HIP_E* code;
 *    visfd_hip_last_error() returns the message of the last failure on the calling thread.
 *  - volumes are contiguous float32, row-major [iz][iy][ix], x fastest (lib/visfd/alloc3d.hpp:16-23);
 *    sizes are 64-bit (the reference's int arithmetic overflows at 2^31 voxels, alloc3d.hpp:33-35).
 *  - "mask" pointers may be NULL (= no mask); a voxel is masked out when mask == 0.
 *  - two faces per operation:
 *        visfd_hip_<op>      host pointers  (drop-in: copies in, runs, copies out, synchronous)
 *        visfd_hip_<op>_dev  device pointers (asynchronous on the context's HIP stream; the caller
 *                            owns the buffers; multi-channel fields are CHANNEL-PLANAR on the device)
 *  - multi-channel fields on the HOST face use the reference's layouts: direction/gradient as
 *    3 interleaved floats per voxel (array<float,3>***, handlers.cpp:1547-1556); Hessian / vote
 *    tensor as 6 interleaved floats per voxel in the order xx,yy,zz,xy,yz,xz
 *    (lib/visfd/lin3_utils.hpp:400-406).  On the DEVICE face they are channel-planar:
 *    field[c*nvox + voxel].
 *  - callee owns its temporaries (as the reference does: filter3d.hpp:731,1362; feature.hpp:1243),
 *    kept in the context's workspace between calls.
 */
#ifndef VISFD_HIP_H
#define VISFD_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define VISFD_HIP_OK 0
#define VISFD_HIP_EINVAL 1   /* bad argument (the reference would assert or throw VisfdErr) */
#define VISFD_HIP_EDEVICE 2  /* HIP runtime failure / no gfx950 device */
#define VISFD_HIP_ENOMEM 3   /* device allocation failed */
#define VISFD_HIP_ECAPACITY 4 /* an output list was too small; counts are still returned */

/* selfadjoint_eigen3::EigenOrderType (lib/visfd/eigen3_simple.hpp:36-43); only the two orders
 * the hot path uses (bin/filter_mrc/handlers.cpp:1524-1535). */
#define VISFD_HIP_INCREASING_EIVALS 0
#define VISFD_HIP_DECREASING_EIVALS 1

typedef struct visfd_hip_ctx visfd_hip_ctx;

/* ---- lifecycle ------------------------------------------------------------------------------- */
/* device: HIP ordinal.  stream: a hipStream_t to run on (e.g. the caller's), or NULL to create one. */
int visfd_hip_create(int device, void* stream, visfd_hip_ctx** out);
/* also aborts the context's blob jobs that were begun and not ended (their handles are then no longer live) */
int visfd_hip_destroy(visfd_hip_ctx* ctx);
int visfd_hip_synchronize(visfd_hip_ctx* ctx);
/* the hipStream_t every _dev entry point of this context runs on (the one given to visfd_hip_create, or the context's own) */
void* visfd_hip_get_stream(visfd_hip_ctx* ctx);
/* release the cached workspace (it otherwise persists between calls).  Allowed at any time, also between the halves of a
 * blob job: what the job has queued is fetched to the host first. */
int visfd_hip_trim(visfd_hip_ctx* ctx);
const char* visfd_hip_last_error(void);
int visfd_hip_abi_version(void);   /* 10: entry points only get added between versions (since 10 was set: the
                                     * morphology entries visfd_hip_sphere_structure, visfd_hip_morph_sphere[_dev],
                                     * visfd_hip_morph_table[_dev] and visfd_hip_morph_last_path; then
                                     * visfd_hip_blob_jobs_pending and visfd_hip_debug_poison_workspace; then the
                                     * general 3-D filter: visfd_hip_gengauss3d_halfwidths, _gengauss3d_table,
                                     * _dogg3d_table, _filter3d[_dev], _filter3d_last_path, _apply_ggauss[_dev],
                                     * _apply_dogg[_dev] and _local_fluctuations_gen[_dev]; then the drawing entries
                                     * visfd_hip_draw_spheres[_dev], visfd_hip_draw_regions[_dev] and
                                     * visfd_hip_draw_last_times; then the watershed: visfd_hip_watershed_host,
                                     * visfd_hip_watershed[_dev] and visfd_hip_watershed_last_stats; then the median
                                     * filter: visfd_hip_median_footprint, visfd_hip_median_sphere[_dev],
                                     * visfd_hip_median_table[_dev] and visfd_hip_median_last_path; then the image
                                     * statistics and intensity maps: visfd_hip_image_stats[_dev|_host] and
                                     * visfd_hip_intensity_map[_dev|_host]; then the distance maps:
                                     * visfd_hip_distance_sq[_dev], visfd_hip_distance_to_points[_dev],
                                     * visfd_hip_distance_from_points[_dev] and visfd_hip_distance_last_path; then the
                                     * supervised blob thresholds: visfd_hip_find_spheres[_dev|_host],
                                     * visfd_hip_find_spheres_last_path, visfd_hip_choose_threshold_1d,
                                     * visfd_hip_find_blob_scores, visfd_hip_choose_blob_score_thresholds[_multi] and
                                     * visfd_hip_discard_blobs_by_score_supervised; then LabelConnected's seed search
                                     * on the device: visfd_hip_label_connected_device_seeds and
                                     * visfd_hip_label_connected_device_seeds_last; then LabelConnected as a graph
                                     * problem: visfd_hip_label_connected_graph[_dev|_host], _graph_last and
                                     * _graph_last_times; then DiscardOverlappingBlobs on the device:
                                     * visfd_hip_discard_overlapping_blobs_ctx, _dev, _last and
                                     * _last_times; then the mesh voxeliser: visfd_hip_voxelize_mesh[_dev],
                                     * visfd_hip_voxelize_last, _last_times, visfd_hip_voxelize_quantize_host and
                                     * visfd_hip_mesh_edges_host; then the flat ball as a threshold,
                                     * visfd_hip_flat_ball_dsq_max; then the closing of an oriented point cloud into a
                                     * mask: visfd_hip_close_surface[_dev], visfd_hip_close_surface_splat[_dev|_host],
                                     * visfd_hip_close_surface_last and _last_times; then the membrane stage on the
                                     * caller's arrays, visfd_hip_membrane_stage_dev, with the option membrane_queue and
                                     * the test aids visfd_hip_debug_ridge_directions_thr_dev and _debug_tv_lists_dev;
                                     * then the isosurface mesh: visfd_hip_isosurface[_dev|_host], visfd_hip_isosurface_last
                                     * and _last_times) */
/* Tuning and test switches of a context (integers; unknown names are VISFD_HIP_EINVAL).  A new context starts from the
 * environment (VISFD_HIP_<NAME>, read once in visfd_hip_create); nothing reads the environment afterwards.
 *   gauss_3pass      1: the separable filter always takes its three single-axis passes
 *   gauss_wg_per_cu  workgroups per CU the single-sweep filter cuts the volume into (default 2)
 *   log_pair         both Gaussians of an unmasked DoG / LoG / BlobDog scale in two shared launches (csrc/gauss_pair.hip; one
 *                    half-width 6..10 on the three axes): 0 never, 1 (default) for the half-widths its table lists, 2 wherever
 *                    it applies; results are bit-identical either way
 *   log_pair_chunk   march length of those two launches along z and y (0, the default: 256 and 512); results are
 *                    bit-identical for every value
 *   membrane_queue   the membrane stage (visfd_hip_membrane_detect*_dev, visfd_hip_membrane_stage_dev, and the select of
 *                    visfd_hip_threshold_fraction*) queued without host steps: 1 (default) the select's digits are picked on
 *                    the device, the stage makes no threshold pass and waits once; 0: a host walk after every select round,
 *                    the threshold pass, a wait for the sender lists' length.  Results are bit-identical either way
 *   tv_dense         1: tensor voting by the baseline kernel
 *   tv_fma           1: TOLERANCE MODE of tensor voting (surfaces, angular exponent 2 or 4): the vote chain with fused
 *                    multiply-adds.  Tensors are then within 1e-5 of the field's scale of the reference's instead of
 *                    bit-identical to them (BASELINE north_star: 1e-5 relative for float voxel values); default 0 = exact
 *   gauss_fma        1: TOLERANCE MODE of the plain separable Gaussian (ApplyGauss / ApplySeparable, symmetric taps,
 *                    no mask): fused multiply-adds and a reciprocal normaliser, same 1e-5 bar.  DoG / LoG / BlobDog feed
 *                    index comparisons and ignore it (always the reference's bits); default 0 = exact
 *   eig_f32          1: TOLERANCE MODE of the device eigen solver (ridge scores and directions, post-vote score, the
 *                    diagonalise batch): its one angle -- atan2, sin, cos -- in single precision; eigenvalues move by about
 *                    one float ulp.  default 0 = the reference's double-precision angle (eigen3_simple.hpp:74-81)
 *   tv_exact_tiled   1: exact tensor voting always runs the general kernel (csrc/tv_tiled.hip), never the faster exact form of
 *                    csrc/tv_box.hip (surfaces, exponent 2 or 4, source mask absent or of zeros and ones); results are bit-identical either way
 *   tv_no_fold       tests: tolerance-mode voting keeps the saliency as a factor of every vote even when all saliencies are
 *                    positive (by default they are then folded into the listed normals: 18 instead of 19 instructions)
 *   tv_poison        tests: NaN bit patterns in LDS, list memory and the output before the kernels of csrc/tv_box.hip run (both forms)
 *   tv_reserve_wg    workgroup slots a voting kernel leaves free of its chip-filling grid (slab runs set it while a halo is in
 *                    flight, so that the transport's kernels find room; default 0)
 *   tv_zrun          receiver planes per unit of work (default 8 in csrc/tv_box.hip, 32 in csrc/tv_tiled.hip)
 *   tv_no_replay     csrc/tv_tiled.hip only: every sender plane is listed again for every receiver plane (no reuse within a run)
 *   tv_max_wg        cap on the number of persistent workgroups (tests: forces many units of work per workgroup)
 *   blob_test_cap    tests: capacity the pipelined blob scan pretends to have (exercises its overflow path)
 *   morph_general    1: morphology always walks the element entry by entry (csrc/morph.hip), never takes the flat X-run
 *                    kernel; results are bit-identical either way
 *   morph_levels     visfd_hip_morph_sphere[_dev] with bmax == 0 on an image of at most two levels (see there) as a threshold
 *                    on the exact distance map (csrc/morph_levels.hip), any radius: 0 never; 1 (default) when eligible and
 *                    ceil(radius) > 10 (beyond the X-run kernel) or radius >= R0 = 5 (R0: the smallest radius timed at which
 *                    it beats the X-run kernel in dilate, erode and open on 1024^3, profiles/morph_levels_time.txt; below
 *                    it no census runs); 2 whenever eligible;
 *                    results are bit-identical for every value
 *   filter3d_general 1: the general 3-D filter always walks the table entry by entry (csrc/filter3d.hip), never takes the
 *                    LDS-tiled kernel; results are bit-identical either way
 *   median_general   1: the median filter always walks the footprint in global memory (csrc/median.hip), never takes the
 *                    LDS-tiled kernel; results are bit-identical either way
 *   distance_general 1: the distance maps always take the brute-force walks (csrc/distance.hip: every voxel against every
 *                    seed, every query point against every selected voxel), never the separable transform; results are
 *                    bit-identical either way
 *   stats_blocks     workgroups of the statistics / intensity-map kernel (csrc/intensity.hip; 0, the default: eight per CU, and
 *                    never more than the image has work for); results are bit-identical for every value
 *   draw_time        1: visfd_hip_draw_spheres[_dev] times its three phases with events and waits for them
 *                    (visfd_hip_draw_last_times); default 0
 *   connect_time     1: visfd_hip_label_connected_graph[_dev] time their stages on the host clock and wait for the stream
 *                    at each (visfd_hip_label_connected_graph_last_times); default 0
 *   connect_settle   1: visfd_hip_label_connected_graph[_dev] keep calls with must-link constraints, voxel weights or a
 *                    cluster whose outward sum is in doubt on the device path: the nearest labelled voxels are searched on
 *                    the device, the merges and the flood's own long double moments are formed on the host from the
 *                    labelled voxels alone (visfd_hip_label_connected_graph_last_settled); results are the flood's bits
 *                    either way; default 0: such calls are handed to the flood
 *   watershed_host   1: visfd_hip_watershed[_dev] run the sequential flood on the host for calls without markers too (with
 *                    markers they always do); labels and lists are identical either way; default 0
 *   find_spheres_host 1: visfd_hip_find_spheres[_dev] walk the (query, sphere) pairs on the host (the walk of
 *                    visfd_hip_find_spheres_host) instead of launching the search kernel; ids are identical either way; default 0
 *   discard_overlap_host 1: visfd_hip_discard_overlapping_blobs_ctx / _dev run the host entry instead of the rounds on the
 *                    device (csrc/discard_overlap.hip); lists are identical either way; default 0
 *   discard_overlap_time 1: those two entries time their phases with stream events
 *                    (visfd_hip_discard_overlapping_blobs_last_times); default 0
 *   discard_overlap_max_rounds  rounds after which the host finishes such a list from the states reached; lists are
 *                    identical for every value; default 256
 *   voxelize_time    1: visfd_hip_voxelize_mesh[_dev] time their three phases with events
 *                    (visfd_hip_voxelize_last_times); default 0
 *   voxelize_bisect  tests: the voxeliser finds the sample behind every crossing by bisection with the exact sign, never
 *                    from its double-precision estimate; images are bit-identical either way; default 0
 *   close_surface_rtol_exp   k: visfd_hip_close_surface[_dev] stop their multigrid cycles when the residual's 2-norm is at
 *                    most 10^-k of the right-hand side's; default 5 (profiles/close_surface_time.txt)
 *   close_surface_max_cycles  ... or after this many cycles (the mask is still returned and
 *                    visfd_hip_close_surface_last reports the stop); default 20, twice the
 *                    most cycles the test cases take at the default rtol
 *   close_surface_time  1: those two entries time their three phases with events (visfd_hip_close_surface_last_times);
 *                    default 0
 *   isosurface_time  1: visfd_hip_isosurface[_dev] time their four phases with events (visfd_hip_isosurface_last_times);
 *                    default 0
 *   gauss_cfg, debug development aids */
int visfd_hip_set_option(visfd_hip_ctx* ctx, const char* name, int64_t value);
int visfd_hip_get_option(visfd_hip_ctx* ctx, const char* name, int64_t* value_out);
/* bytes of device workspace currently held by the context */
int64_t visfd_hip_workspace_bytes(visfd_hip_ctx* ctx);
/* TEST AID: waits for the context's stream, then fills every workspace slot the context holds with 0xFF bytes (NaN as
 * floats, huge as counters) and forgets what it had cached inside them (vote table, structuring element, filter table, median footprint), without freeing
 * anything.  No stage may depend on what a slot held before the call that uses it, so every result after this call is the
 * same as before it.  What live blob jobs have queued is fetched to the host first, as visfd_hip_trim does. */
int visfd_hip_debug_poison_workspace(visfd_hip_ctx* ctx);

/* ---- a1: filter taps (host arithmetic, long double) ------------------------------------------ */
/* GenFilterGauss1D<float>, lib/visfd/filter1d.hpp:409-460.  taps_out has 2*halfwidth+1 entries. */
int visfd_hip_gauss_taps(float sigma, int halfwidth, float* taps_out);
/* ratio = sqrt(-2 ln threshold) in float, bin/filter_mrc/filter3d_variants.hpp:513-518 */
float visfd_hip_ratio_from_threshold(float truncate_threshold);

/* ---- a4: ApplySeparable, lib/visfd/filter3d.hpp:686-1050 -------------------------------------- */
/* taps_d has 2*h_d+1 entries, centre at index h_d.  A_out (nullable) = product of the centre taps. */
int visfd_hip_separable3d(visfd_hip_ctx*, const float* src, float* dst, const float* mask,
                          int64_t nx, int64_t ny, int64_t nz,
                          const float* taps_x, int hx, const float* taps_y, int hy,
                          const float* taps_z, int hz, int normalize, float* A_out);
int visfd_hip_separable3d_dev(visfd_hip_ctx*, const float* src, float* dst, const float* mask,
                              int64_t nx, int64_t ny, int64_t nz,
                              const float* taps_x, int hx, const float* taps_y, int hy,
                              const float* taps_z, int hz, int normalize, float* A_out);

/* ---- a5: ApplyGauss(sigma[3], halfwidth[3]), lib/visfd/filter3d.hpp:1086-1124 ------------------ */
int visfd_hip_apply_gauss(visfd_hip_ctx*, const float* src, float* dst, const float* mask,
                          int64_t nx, int64_t ny, int64_t nz, const float sigma[3],
                          const int halfwidth[3], int normalize, float* A_out);
int visfd_hip_apply_gauss_dev(visfd_hip_ctx*, const float* src, float* dst, const float* mask,
                              int64_t nx, int64_t ny, int64_t nz, const float sigma[3],
                              const int halfwidth[3], int normalize, float* A_out);
/* halfwidth[d] = max(1, floor(sigma[d]*ratio)), lib/visfd/filter3d.hpp:1240-1247 */
int visfd_hip_gauss_halfwidths(const float sigma[3], float truncate_ratio, int halfwidth_out[3]);

/* ---- f4: LocalFluctuations (lib/visfd/filter3d.hpp:1698-1853) ---------------------------------- */
/* dst = sqrt(max(A * G((src - G(src))^2), 0)), G = ApplyGauss(sigma[3], truncate_ratio) with the same mask and
 * normalize flag, A = the central value of GenFilterGenGauss3D(sigma, exponent, truncate_ratio)
 * (filter3d.hpp:546-640, :1725, :1836).  Only exponent == 2 (the separable case) is provided here; src != dst.
 * visfd_hip_local_fluctuations_gen (below) takes any exponent. */
int visfd_hip_local_fluctuations(visfd_hip_ctx*, const float* src, float* dst, const float* mask,
                                 int64_t nx, int64_t ny, int64_t nz, const float sigma[3], float exponent,
                                 float truncate_ratio, int normalize);
int visfd_hip_local_fluctuations_dev(visfd_hip_ctx*, const float* src, float* dst, const float* mask,
                                     int64_t nx, int64_t ny, int64_t nz, const float sigma[3], float exponent,
                                     float truncate_ratio, int normalize);
/* LocalFluctuationsByRadius (filter3d.hpp:1897-1926; bin/filter_mrc/filter3d_variants.hpp:651-681), host arithmetic:
 * sigma = radius / (9 pi / 2)^(1/6); a negative truncate_ratio is replaced by (-log threshold)^(1/exponent). */
int visfd_hip_fluctuation_sigmas(const float radius[3], float exponent, float truncate_ratio,
                                 float truncate_threshold, float sigma_out[3], float* ratio_out);

/* ---- g1-g5: the general (non-separable) 3-D filter, Filter3D::Apply (lib/visfd/filter3d.hpp:37-530) ----------------
 * Tables are (2 hx + 1)(2 hy + 1)(2 hz + 1) floats, x fastest, entry H[jz][jy][jx] at ((jz + hz) * (2 hy + 1) + jy + hy) *
 * (2 hx + 1) + jx + hx.  The table makers are host arithmetic and take no context.  They write nothing when cap == 0
 * (count only), return VISFD_HIP_ECAPACITY when 0 < cap < *n, and always set *n to the entry count. */
/* halfwidth[d] = floor(width[d] * ratio); a negative ratio is first replaced by pow(-log(threshold), 1.0 / m_exp)
 * (bin/filter_mrc/filter3d_variants.hpp:99-103, lib/visfd/filter3d.hpp:631-633) */
int visfd_hip_gengauss3d_halfwidths(const float width[3], float m_exp, float truncate_ratio, float truncate_threshold,
                                    int halfwidth_out[3]);
/* GenFilterGenGauss3D(width, m_exp, truncate_halfwidth) (filter3d.hpp:546-601): exp(-r^m), r = sqrt((x/wx)^2 + (y/wy)^2 +
 * (z/wz)^2), entries below the smallest face value zeroed, divided by their float sum.  A_out (nullable) = centre entry. */
int visfd_hip_gengauss3d_table(const float width[3], float m_exp, const int halfwidth[3], float* table, int64_t cap,
                               int64_t* n, float* A_out);
/* GenFilterDogg3D(width_a, width_b, m, n, ratio, threshold) (filter3d_variants.hpp:284-345, :441-482): each generalised
 * Gaussian in its own window, the table's window (halfwidth_out) their per-axis maximum, entries A_entry - B_entry.
 * A_out, B_out (nullable): the two centre values. */
int visfd_hip_dogg3d_table(const float width_a[3], const float width_b[3], float m_exp, float n_exp, float truncate_ratio,
                           float truncate_threshold, int halfwidth_out[3], float* table, int64_t cap, int64_t* n,
                           float* A_out, float* B_out);
/* Filter3D::Apply (filter3d.hpp:81-198, :403-458): for every voxel i with mask(i) != 0 (or no mask)
 *   g = sum_j (H[j] * mask(i - j)) * src(i - j),   den = sum_j H[j] * mask(i - j)
 * over the senders i - j inside the image with mask != 0, j walked with jz outermost, then jy, then jx, each from -h to +h,
 * in float, multiply then add; dst = g, or g / den where `normalize` and den > 0.  den_out (nullable) receives den: the
 * reference's second Apply overload.  Bit-identical to the reference for finite src.
 * DEFINED HERE, undefined in the reference: a voxel with mask == 0 gets dst = 0 and den = 0 also when no denominator was
 * asked for (the reference dereferences a null pointer there, filter3d.hpp:182).
 * THE ONE DIVERGENCE: table entries equal to 0 may be dropped and senders with mask == 0 enter as zero factors, so a NaN
 * or Inf in src under a zero weight or outside the mask need not spread to its neighbours as it does in the reference
 * (which of the two kernels runs decides; for finite src both give the reference's bits).
 * A dst that overlaps src or mask is VISFD_HIP_EINVAL; so are negative half-widths.  `table` is a host array on both
 * faces; it is kept in the context's workspace and sent again only when it changes. */
int visfd_hip_filter3d(visfd_hip_ctx*, const float* src, float* dst, const float* mask, int64_t nx, int64_t ny, int64_t nz,
                       const float* table, const int halfwidth[3], int normalize, float* den_out);
int visfd_hip_filter3d_dev(visfd_hip_ctx*, const float* src, float* dst, const float* mask, int64_t nx, int64_t ny,
                           int64_t nz, const float* table, const int halfwidth[3], int normalize, float* den_out);
/* the kernel the context's last general-filter call ran: VISFD_HIP_FILTER3D_PATH_* (-1 before the first call).  The tiled
 * kernel takes every window whose source and mask patches, 2 * (64 + 2 hx) * (4 + 2 hy) floats, fit 48 KB of LDS; the
 * option filter3d_general forces the general one. */
#define VISFD_HIP_FILTER3D_PATH_GENERAL 0    /* filter3d_kernel: the non-zero entries walked one by one, no LDS */
#define VISFD_HIP_FILTER3D_PATH_TILED 1      /* filter3d_tiled_kernel: source planes staged in LDS, 8 output planes a thread */
int visfd_hip_filter3d_last_path(visfd_hip_ctx*, int* path);
/* HandleGGauss (bin/filter_mrc/handlers.cpp:167-187): the generalised Gaussian table above, applied.  A_out nullable. */
int visfd_hip_apply_ggauss(visfd_hip_ctx*, const float* src, float* dst, const float* mask, int64_t nx, int64_t ny,
                           int64_t nz, const float width[3], float m_exp, const int halfwidth[3], int normalize,
                           float* A_out);
int visfd_hip_apply_ggauss_dev(visfd_hip_ctx*, const float* src, float* dst, const float* mask, int64_t nx, int64_t ny,
                               int64_t nz, const float width[3], float m_exp, const int halfwidth[3], int normalize,
                               float* A_out);
/* HandleDogg (handlers.cpp:265-293): the difference-of-generalised-Gaussians table above, applied; never normalised. */
int visfd_hip_apply_dogg(visfd_hip_ctx*, const float* src, float* dst, const float* mask, int64_t nx, int64_t ny,
                         int64_t nz, const float width_a[3], const float width_b[3], float m_exp, float n_exp,
                         float truncate_ratio, float truncate_threshold, float* A_out, float* B_out);
int visfd_hip_apply_dogg_dev(visfd_hip_ctx*, const float* src, float* dst, const float* mask, int64_t nx, int64_t ny,
                             int64_t nz, const float width_a[3], const float width_b[3], float m_exp, float n_exp,
                             float truncate_ratio, float truncate_threshold, float* A_out, float* B_out);
/* LocalFluctuations for any exponent (filter3d.hpp:1698-1853): with W = the filter of GenFilterGenGauss3D(sigma, exponent,
 * floor(sigma * truncate_ratio)) times (float)(1.0 / A), A its centre entry: dst = sqrt(max(A * W((src - W(src))^2), 0)),
 * both W with the same mask and normalize flag.  Exponent 2 takes the separable path of visfd_hip_local_fluctuations. */
int visfd_hip_local_fluctuations_gen(visfd_hip_ctx*, const float* src, float* dst, const float* mask, int64_t nx,
                                     int64_t ny, int64_t nz, const float sigma[3], float exponent, float truncate_ratio,
                                     int normalize);
int visfd_hip_local_fluctuations_gen_dev(visfd_hip_ctx*, const float* src, float* dst, const float* mask, int64_t nx,
                                         int64_t ny, int64_t nz, const float sigma[3], float exponent,
                                         float truncate_ratio, int normalize);

/* ---- d1-d2: drawing (lib/visfd/draw.hpp:90-457) ------------------------------------------------------------------
 * Both are bit-identical to the reference for finite inputs. */
/* DrawSpheres (draw.hpp:238-457).  Every voxel of dst, masked or not, first becomes background * rescale + offset (two float
 * roundings) or, with background_normalize, ((background - ave) / stddev) * rms * rescale + offset, where ave and stddev are
 * the reference's float statistics of the background weighted by the mask (0 + offset when stddev is not > 0) and rms the
 * root mean square of `foreground`.  Then sphere i = 0 .. n-1 in list order overwrites the voxels with mask != 0 whose
 * squared integer distance r2 from the centre truncated to int satisfies rmin2 <= (float)r2 <= rmax2, rmax2 = (d/2)^2,
 * rmin2 = (d/2 - th)^2 when th > 0 and d/2 - th > 0, else 0, with foreground[i], divided under foreground_normalize by the
 * number of such voxels.  So the last sphere in list order wins every voxel it holds.
 * centers: 3 n floats (x, y, z per sphere, in voxels).  diameters, shell_thicknesses, foreground: n floats each or NULL for
 * the reference's defaults (diameter 0, thickness = radius: a solid sphere, foreground 1).  All four are HOST arrays on
 * both faces.  dst may be the background array itself; any other overlap of dst with background or mask is refused.
 * any_center_outside (nullable): set to 1 when a truncated centre lies outside the image (the reference's warning), else 0.
 * With background_normalize the statistics are computed on the host (the _dev face copies background and mask down for
 * them and waits for the stream); otherwise the _dev face is asynchronous.
 * Refused with VISFD_HIP_EINVAL, dst untouched: a null background (the reference dereferences it), n > 2^31 - 2, a centre
 * that is not finite or does not fit an int, a diameter that is not finite or whose Rs = ceil(d/2 - 0.5) has
 * 3 Rs^2 >= 2^31 (the reference's int arithmetic overflows there). */
int visfd_hip_draw_spheres(visfd_hip_ctx*, float* dst, const float* mask, const float* background, int64_t nx, int64_t ny,
                           int64_t nz, const float* centers, const float* diameters, const float* shell_thicknesses,
                           const float* foreground, int64_t n, float background_offset, float background_rescale,
                           int background_normalize, int foreground_normalize, int* any_center_outside);
int visfd_hip_draw_spheres_dev(visfd_hip_ctx*, float* dst, const float* mask, const float* background, int64_t nx,
                               int64_t ny, int64_t nz, const float* centers, const float* diameters,
                               const float* shell_thicknesses, const float* foreground, int64_t n, float background_offset,
                               float background_rescale, int background_normalize, int foreground_normalize,
                               int* any_center_outside);
/* With the option draw_time set: milliseconds the last DrawSpheres of the context spent in the zero fill of its owner volume,
 * in the scatter (with the counting pass of foreground_normalize) and in the resolve; -1 before the first timed call. */
int visfd_hip_draw_last_times(visfd_hip_ctx*, float ms[3]);
/* SimpleRegion<float> (draw.hpp:46-81) as a plain struct.  c: xmin, xmax, ymin, ymax, zmin, zmax of a rectangle, or
 * x0, y0, z0, r of a sphere (c[4], c[5] unused), in voxels. */
#define VISFD_HIP_REGION_RECT 0
#define VISFD_HIP_REGION_SPHERE 1
typedef struct visfd_hip_region {
  int32_t type;
  float c[6];
  float value;
} visfd_hip_region;
/* DrawRegions (draw.hpp:90-224): the regions act on dst in list order, on voxels with mask != 0 only.  A value that is
 * not negative (NaN included) is written; a negative one zeroes voxels that are > 0 when negative_means_subtract, and does
 * nothing otherwise.  When the first region is negative, negative_means_subtract is set and every unmasked voxel of dst is
 * 0, the unmasked voxels are first set to 1.  `regions` is a HOST array on both faces; the _dev face is asynchronous.
 * Refused: a sphere whose centre or radius is not finite, whose rounded centre does not fit an int or whose
 * Ri = ceil(r - 0.5) exceeds 32767. */
int visfd_hip_draw_regions(visfd_hip_ctx*, float* dst, const float* mask, int64_t nx, int64_t ny, int64_t nz,
                           const visfd_hip_region* regions, int64_t n, int negative_means_subtract);
int visfd_hip_draw_regions_dev(visfd_hip_ctx*, float* dst, const float* mask, int64_t nx, int64_t ny, int64_t nz,
                               const visfd_hip_region* regions, int64_t n, int negative_means_subtract);

/* ---- m1: grayscale morphology (lib/visfd/morphology.hpp:134-597) ------------------------------- */
#define VISFD_HIP_MORPH_DILATE 0          /* DilateSphere / Dilate                         morphology.hpp:134-172, 241-330 */
#define VISFD_HIP_MORPH_ERODE 1           /* ErodeSphere / Erode                           :188-229, 336-420 */
#define VISFD_HIP_MORPH_OPEN 2            /* OpenSphere: erode, then dilate                :431-468 */
#define VISFD_HIP_MORPH_CLOSE 3           /* CloseSphere: dilate, then erode               :475-510 */
#define VISFD_HIP_MORPH_TOP_HAT_WHITE 4   /* WhiteTopHatSphere: dst = dst - open(src)      :517-553 */
#define VISFD_HIP_MORPH_TOP_HAT_BLACK 5   /* BlackTopHatSphere: dst = close(src) - dst     :560-597 */
/* The structuring element of DilateSphere / ErodeSphere (morphology.hpp:254-316), host arithmetic: entries (dx, dy, dz)
 * in dxyz (3 ints each) and b, dz outermost, then dy, then dx.  *n = the number of entries; the first min(n, cap) are
 * written (cap == 0: count only; 0 < cap < n: VISFD_HIP_ECAPACITY).  ceil(max(radius, radius_max)) must be <= 128. */
int visfd_hip_sphere_structure(float radius, float radius_max, float bmax, int* dxyz, float* b, int64_t cap,
                               int64_t* n);
/* The flat ball (bmax == 0) as a threshold: offset (ix, iy, iz) is in the element exactly when ix^2 + iy^2 + iz^2 <= *t,
 * the largest integer whose double square root, rounded to float, is <= radius (the element's test is monotone in the
 * squared length, and its cube never cuts the ball).  Host arithmetic, no table; any finite radius >= 0. */
int visfd_hip_flat_ball_dsq_max(float radius, int64_t* t);
/* op = VISFD_HIP_MORPH_*, with the sphere element above.  The reference library's semantics: voxels with mask == 0 are
 * not written (dst keeps its values there); neighbours with mask == 0 or outside the image are skipped; the top-hats
 * read dst.  A dst that overlaps src or mask is VISFD_HIP_EINVAL.  The temporaries live in the context's workspace.
 * Flat elements made of symmetric X-runs of half-length <= 10 (every flat ball of radius < 11) run on the X-run kernel,
 * everything else on the general element walk; both give the reference's bits.
 * Two-level images (option morph_levels): with bmax == 0, radius finite and >= 0, radius_max finite, option morph_general
 * 0 and nx + ny + nz <= 46340, a source whose voxels with mask != 0 hold at most two distinct bit patterns, none a NaN
 * and the two comparing unequal (so not +0 / -0), needs no element: the flat ball is {d^2 <= visfd_hip_flat_ball_dsq_max
 * (radius)}, a threshold on the exact squared distance to the nearest voxel of a level (csrc/distance.hip).  A census
 * kernel decides (its few words are all the host reads back); the cost is O(voxels) at any radius, the element is neither
 * built nor uploaded, radii beyond 128 are accepted, and the bits are the element walk's.  A call that is not eligible
 * runs as described above, error codes included. */
int visfd_hip_morph_sphere(visfd_hip_ctx*, const float* src, float* dst, const float* mask,
                           int64_t nx, int64_t ny, int64_t nz, int op, float radius, float radius_max, float bmax);
int visfd_hip_morph_sphere_dev(visfd_hip_ctx*, const float* src, float* dst, const float* mask,
                               int64_t nx, int64_t ny, int64_t nz, int op, float radius, float radius_max, float bmax);
/* Dilate / Erode (op VISFD_HIP_MORPH_DILATE or _ERODE) with an arbitrary element of n entries: (dx, dy, dz) in dxyz
 * (3 ints each) and b, walked in the given order (host arrays on both faces). */
int visfd_hip_morph_table(visfd_hip_ctx*, const float* src, float* dst, const float* mask,
                          int64_t nx, int64_t ny, int64_t nz, int op, const int* dxyz, const float* b, int64_t n);
int visfd_hip_morph_table_dev(visfd_hip_ctx*, const float* src, float* dst, const float* mask,
                              int64_t nx, int64_t ny, int64_t nz, int op, const int* dxyz, const float* b, int64_t n);
/* the kernel the context's last morphology call ran: VISFD_HIP_MORPH_PATH_* (-1 before the first call) */
#define VISFD_HIP_MORPH_PATH_GENERAL 0    /* morph_kernel: the element walked entry by entry */
#define VISFD_HIP_MORPH_PATH_XRUNS 1      /* morph_runs_kernel: window maxima of X-runs, zero-sign fix-up of erosions */
#define VISFD_HIP_MORPH_PATH_LEVELS 2     /* csrc/morph_levels.hip: every step of the call a threshold on the distance map */
int visfd_hip_morph_last_path(visfd_hip_ctx*, int* path);

/* ---- m1b: the median filter, Median / MedianSphere (lib/visfd/filter3d.hpp:1577-1674) -------------- */
/* The reference's footprint loop does not terminate once a neighbour is skipped, so the semantics are stated here.
 * A voxel with mask == 0 is not written (dst keeps its value).  Any other voxel collects the source values at voxel +
 * entry for every footprint entry that lies inside the image and, with a mask, has mask != 0; duplicates count as often
 * as they appear and the centre need not be an entry.  With n values collected it gets the value of rank n / 2 (0-based,
 * ascending: the upper median for even n, what std::nth_element(begin, begin + n / 2, begin + n) leaves there), and
 * +0.0f when n == 0.  The order is total on bit patterns: a float with bits u has the key ~u if its sign bit is set, else
 * u | 0x80000000, and keys compare as unsigned integers -- operator< for finite values and infinities, -0 before +0, NaNs
 * by sign and payload below -inf or above +inf -- so every result is defined to the bit for every input.
 * Limits, which keep one launch bounded (beyond them: VISFD_HIP_EINVAL): radius >= 0 and ceil(radius) <= 16; a table has
 * 1 <= n <= 32768 entries with |d| <= 16 per axis; ny <= 262140 (65535 rows of workgroups of 4 voxels in y; nx and nz
 * only need to be below 2^30).  A dst that overlaps src or mask is VISFD_HIP_EINVAL. */
#define VISFD_HIP_MEDIAN_MAX_RADIUS 16
#define VISFD_HIP_MEDIAN_MAX_ENTRIES 32768
/* The footprint of MedianSphere (filter3d.hpp:1652-1662), host arithmetic: with Ri = ceil(radius), every (ix, iy, iz) of
 * [-Ri, Ri]^3 with (float)sqrt((double)(ix^2 + iy^2 + iz^2)) <= radius, iz outermost, then iy, then ix, 3 ints each.
 * *n = the number of entries; the first min(n, cap) are written (cap == 0: count only; 0 < cap < n:
 * VISFD_HIP_ECAPACITY). */
int visfd_hip_median_footprint(float radius, int* dxyz, int64_t cap, int64_t* n);
int visfd_hip_median_sphere(visfd_hip_ctx*, const float* src, float* dst, const float* mask,
                            int64_t nx, int64_t ny, int64_t nz, float radius);
int visfd_hip_median_sphere_dev(visfd_hip_ctx*, const float* src, float* dst, const float* mask,
                                int64_t nx, int64_t ny, int64_t nz, float radius);
/* an arbitrary footprint of n entries (dx, dy, dz), 3 ints each (a host array on both faces) */
int visfd_hip_median_table(visfd_hip_ctx*, const float* src, float* dst, const float* mask,
                           int64_t nx, int64_t ny, int64_t nz, const int* dxyz, int64_t n);
int visfd_hip_median_table_dev(visfd_hip_ctx*, const float* src, float* dst, const float* mask,
                               int64_t nx, int64_t ny, int64_t nz, const int* dxyz, int64_t n);
/* the kernel the context's last median call ran: VISFD_HIP_MEDIAN_PATH_* (-1 before the first call) */
#define VISFD_HIP_MEDIAN_PATH_GENERAL 0   /* median_general_kernel: neighbours from global memory, tested per entry */
#define VISFD_HIP_MEDIAN_PATH_TILED 1     /* median_tiled_kernel: 64 x 4 x 4 outputs and their bounding box in LDS (64 KiB:
                                           * balls up to radius 5) */
int visfd_hip_median_last_path(visfd_hip_ctx*, int* path);

/* ---- exact distance maps (bin/filter_mrc/handlers_unsupported.cpp:1393-1550: -distance-points, -distance-to-voxels) ---- */
/* The integer quantity behind both handlers, bit for bit:
 *     dsq(v) = min(cap, min over seeds s of |v - s|^2),   cap = (nx + ny + nz)^2   (the reference's start value)
 * Seeds are the voxels with mask != 0 (mask nullable) and lo <= src <= hi (a NaN voxel is never one; src nullable: no voxel
 * is) and the `npoints` listed points (x, y, z as int32 triples, ALWAYS A HOST ARRAY), which may lie anywhere, outside the
 * image too.  nx + ny + nz must be at most 46340 (beyond it cap overflows the reference's int): VISFD_HIP_EINVAL.
 * The device work is an exact separable Euclidean distance transform, O(voxels) whatever the number of seeds; only listed
 * or query points OUTSIDE the image cost O(voxels x such points).  Voxels are cubes: the float forms use one voxel width
 * (the reference uses voxel_width[0]); anisotropic voxels are not provided.
 *
 * visfd_hip_distance_sq[_dev]            dsq (int32, nz*ny*nx) from the seeds above
 * visfd_hip_distance_to_points[_dev]     dst = sqrtf((float)dsq * (w * w)), every step rounded to float, from the listed
 *                                        points alone, where mask != 0; dst keeps its value where mask == 0.  dst must not
 *                                        overlap mask (VISFD_HIP_EINVAL)
 * visfd_hip_distance_from_points[_dev]   the roles swapped: out[k] (HOST array of npoints floats on both faces) is the same
 *                                        float formula for the distance from listed point k to the nearest selected voxel
 *                                        (cap's distance when none is selected); returns with the stream idle */
#define VISFD_HIP_DISTANCE_MAX_DIM_SUM 46340
int visfd_hip_distance_sq(visfd_hip_ctx*, const float* src, const float* mask, int64_t nx, int64_t ny, int64_t nz,
                          float lo, float hi, const int32_t* points, int64_t npoints, int32_t* dsq);
int visfd_hip_distance_sq_dev(visfd_hip_ctx*, const float* src, const float* mask, int64_t nx, int64_t ny, int64_t nz,
                              float lo, float hi, const int32_t* points, int64_t npoints, int32_t* dsq);
int visfd_hip_distance_to_points(visfd_hip_ctx*, float* dst, const float* mask, int64_t nx, int64_t ny, int64_t nz,
                                 const int32_t* points, int64_t npoints, float voxel_width);
int visfd_hip_distance_to_points_dev(visfd_hip_ctx*, float* dst, const float* mask, int64_t nx, int64_t ny, int64_t nz,
                                     const int32_t* points, int64_t npoints, float voxel_width);
int visfd_hip_distance_from_points(visfd_hip_ctx*, const float* src, const float* mask, int64_t nx, int64_t ny, int64_t nz,
                                   float lo, float hi, const int32_t* points, int64_t npoints, float voxel_width,
                                   float* out);
int visfd_hip_distance_from_points_dev(visfd_hip_ctx*, const float* src, const float* mask, int64_t nx, int64_t ny,
                                       int64_t nz, float lo, float hi, const int32_t* points, int64_t npoints,
                                       float voxel_width, float* out);
/* what the context's last distance call ran: VISFD_HIP_DISTANCE_PATH_* (-1 before the first call) */
#define VISFD_HIP_DISTANCE_PATH_GENERAL 0     /* the brute-force walks (option distance_general) */
#define VISFD_HIP_DISTANCE_PATH_TRANSFORM 1   /* the separable transform: a row pass and two lower-envelope passes */
int visfd_hip_distance_last_path(visfd_hip_ctx*, int* path);

/* ---- m1c: image statistics and the intensity maps that end every filter_mrc run (bin/filter_mrc/filter_mrc.cpp:746-786,
 * handlers.cpp:1003-1081, lib/threshold/threshold.hpp, MrcSimple::Invert / Rescale01 / FindMinMaxMean) -------------- */
/* Statistics of the voxels with mask == NULL || mask != 0.
 *   count        how many voxels that is
 *   n_nonfinite  how many of them are NaN or +-inf; when this is not 0 the fields below are unspecified
 *   min, max     by the total order on bit patterns (-0 before +0)
 *   sum          the EXACT sum of the values, rounded once to double (round to nearest even): what Python's math.fsum
 *                returns.  The device adds integers -- per exponent field the mantissas of the positive and of the negative
 *                values in 64-bit words -- so the result depends neither on the launch geometry nor on arrival order; the
 *                host combines the 255 bins in multi-word integer arithmetic.
 *   order_free   1 when a double sum of the values is provably the same in EVERY order of additions: all values are
 *                multiples of 2^q and sum |x| < 2^(q + 53), so every partial sum of every order is a multiple of 2^q below
 *                2^(q + 53), hence a double, hence exact.  Then sum / count is bit for bit the mean FindMinMaxMean and
 *                Invert compute serially (mrc_simple.cpp:396-481).  0: not proven (a serial sum may round differently).
 * count == 0 gives sum = 0, min = max = 0 and order_free = 1. */
typedef struct visfd_hip_stats {
  int64_t count;
  int64_t n_nonfinite;
  double sum;
  float min, max;
  int32_t order_free;
  int32_t reserved;
} visfd_hip_stats;
int visfd_hip_image_stats(visfd_hip_ctx*, const float* src, const float* mask, int64_t n, visfd_hip_stats* out);
/* src and mask on the device, `out` on the host; returns with the stream idle */
int visfd_hip_image_stats_dev(visfd_hip_ctx*, const float* src, const float* mask, int64_t n, visfd_hip_stats* out);
/* the same bins filled by a plain host loop and the same combine: no context, no device */
int visfd_hip_image_stats_host(const float* src, const float* mask, int64_t n, visfd_hip_stats* out);

/* One pass that applies, per voxel and in the reference's order, the stages `p` switches on:
 *   1. invert      out = (float)(2.0 * ave - (double)out) where mask != 0                (MrcSimple::Invert)
 *   2. map         one of VISFD_HIP_MAP_*.  The threshold family READS `in` AND OVERWRITES out (so an inversion is lost, and so
 *                  is whatever a filter wrote to out: handlers.cpp:1044-1077); RESCALE acts on out: out * t[0], then + t[1],
 *                  each rounded to float
 *   3. mask_fill   out = masked_value where mask == 0                                    (filter_mrc.cpp:771-776)
 *   4. rescale01   out = rescale_a + ((rescale_b - rescale_a) * (out - dmin)) / (dmax - dmin), left to right in float, on
 *                  every voxel                                                           (MrcSimple::Rescale01)
 * The maps, with I = in[voxel], a, b, c, d = t[0..3], every operation rounded to float (threshold.hpp with Number = float):
 *   STEP      I > a ? out_b : out_a
 *   THRESH2   g = (I - a) / (b - a) when (a <= I && I < b) || (b < I && I <= a), else 1 when (I - a) * (b - a) > 0, else 0;
 *             out_a + g * (out_b - out_a).  Clipping is THRESH2 with out_a = a and out_b = b (not min(max(I, a), b): the
 *             bits differ)
 *   THRESH4   Threshold4 (threshold.hpp:117-169), including its early return of g itself when b == c == d; thresholds that
 *             are neither increasing nor decreasing (the reference asserts) give the first ramp's g
 *   RANGE     SelectIntensityRange: 1 or 0, out_a and out_b unused as in the reference (threshold.hpp:206-229)
 *   GAUSS     (float)(out_a + (double)(out_b - out_a) * exp(-0.5 * xr * xr)), xr = (I - a) / b in float, the rest in
 *             double.  The device's double exp may differ from the host library's in its last bit: results are within one
 *             float ulp of the reference's, everything else on this page is bit for bit.
 * in == out is allowed (in may be NULL when no threshold map is on: it is then not read); any other overlap of out with in
 * or mask is VISFD_HIP_EINVAL.  mask may be NULL: every voxel then counts as mask != 0.  Loads and stores are 16 bytes wide
 * where the arrays' addresses agree modulo 16, with a scalar head and tail; arrays need 4-byte alignment only.
 * stats_out (nullable): the statistics of what was written, under the mask when p->stats_mask, else of every voxel; the
 * call then returns with the stream idle (without it the _dev face only queues the kernel). */
#define VISFD_HIP_MAP_NONE 0
#define VISFD_HIP_MAP_STEP 1
#define VISFD_HIP_MAP_THRESH2 2
#define VISFD_HIP_MAP_THRESH4 3
#define VISFD_HIP_MAP_RANGE 4
#define VISFD_HIP_MAP_GAUSS 5
#define VISFD_HIP_MAP_RESCALE 6
typedef struct visfd_hip_intensity {
  int32_t invert;       /* stage 1 on / off */
  int32_t map;          /* stage 2: VISFD_HIP_MAP_* */
  int32_t mask_fill;    /* stage 3 on / off */
  int32_t rescale01;    /* stage 4 on / off */
  int32_t stats_mask;   /* stats_out: 1 under the mask, 0 of every voxel */
  int32_t reserved;
  double ave;           /* stage 1: the mean to invert about */
  float t[4];           /* stage 2: a, b, c, d (GAUSS: x0, sigma; RESCALE: factor, offset) */
  float out_a, out_b;   /* stage 2 */
  float masked_value;   /* stage 3 */
  float dmin, dmax;     /* stage 4 */
  float rescale_a, rescale_b;
  float reserved2;
} visfd_hip_intensity;
int visfd_hip_intensity_map(visfd_hip_ctx*, const float* in, float* out, const float* mask,
                            int64_t nx, int64_t ny, int64_t nz, const visfd_hip_intensity* p, visfd_hip_stats* stats_out);
int visfd_hip_intensity_map_dev(visfd_hip_ctx*, const float* in, float* out, const float* mask,
                                int64_t nx, int64_t ny, int64_t nz, const visfd_hip_intensity* p, visfd_hip_stats* stats_out);
/* the same stages by a plain host loop (the scalar functions of csrc/intensity.hpp compiled for the host): no context, no
 * device; stats_out as above */
int visfd_hip_intensity_map_host(const float* in, float* out, const float* mask, int64_t nx, int64_t ny, int64_t nz,
                                 const visfd_hip_intensity* p, visfd_hip_stats* stats_out);

/* ---- m2: local minima and maxima with plateaus, _FindExtrema (lib/visfd/morphology_implementation.hpp:57-515) ---- */
/* A plateau is a maximal set of voxels with mask != 0 joined through neighbour pairs of equal value (-0 == +0; a NaN
 * voxel is alone); its root is its first voxel in raster order.  It is a minimum unless a member has a lower existing
 * neighbour, a maximum unless a member has a higher one; a neighbour outside the image or with mask == 0 disqualifies
 * both unless allow_borders.  connectivity 1, 2, 3: the 6, 18, 26 neighbours with dx^2 + dy^2 + dz^2 <= connectivity
 * (the reference accepts larger values; here they are VISFD_HIP_EINVAL).  Images of 2^31 - 2 voxels and more are
 * VISFD_HIP_EINVAL too (the union-find word and the labels are 32-bit).
 * Lists (host arrays on both faces, each may be NULL): root index ix + nx * (iy + ny * iz), root value, voxels of the
 * plateau.  Minima with value <= minima_threshold ascending in (value, root index); maxima with value >=
 * maxima_threshold in exactly the reverse of ascending order (the reference's, ties included).  The thresholds are
 * taken as given: FindMaxima's replacement of +inf by -inf is the caller's (visfd_hip.hpp does it).
 * *n_min / *n_max always receive the list lengths.  A capacity of 0 writes nothing of that list; 0 < capacity < length:
 * VISFD_HIP_ECAPACITY and nothing but the counts is written.
 * labels (NULL: none; the device in the _dev face): the reference's aaaiDest as int32, numbered by position in the
 * sorted lists, maxima positive, minima negative (positive when only one kind is sought); voxels with mask == 0 are not
 * written.  The reference's numbering rules are kept.  labels must not overlap src or mask.
 * Further limits of the classification launch, VISFD_HIP_EINVAL as well: ny and nz at most 524280, and fewer than 2^24
 * tiles of 64 x 8 x 8 voxels, ceil(nx/64) * ceil(ny/8) * ceil(nz/8) (only very thin images of near 2^31 voxels get there).
 * Both faces return with the context's stream idle.  Temporaries: 9 bytes per voxel in the context's workspace, 12 bytes
 * per list entry and, with labels, 8 more per listed entry; the host face also stages src, mask and labels there (4 bytes
 * per voxel each).  A call that returns VISFD_HIP_ECAPACITY has done all of the device work, and the repeated call does
 * it again: give the lists room (visfd_hip.hpp and the Python binding start with max(65536, voxels / 32) entries). */
#define VISFD_HIP_EXTREMA_MAX_CONNECTIVITY 3
#define VISFD_HIP_EXTREMA_MAX_VOXELS 2147483645LL
#define VISFD_HIP_EXTREMA_MAX_NY_NZ 524280
int visfd_hip_find_extrema(visfd_hip_ctx*, const float* src, const float* mask, int64_t nx, int64_t ny, int64_t nz,
                           int find_minima, int find_maxima, float minima_threshold, float maxima_threshold,
                           int connectivity, int allow_borders,
                           int64_t* min_index, float* min_score, int64_t* min_nvoxels, int64_t min_cap, int64_t* n_min,
                           int64_t* max_index, float* max_score, int64_t* max_nvoxels, int64_t max_cap, int64_t* n_max,
                           int32_t* labels);
int visfd_hip_find_extrema_dev(visfd_hip_ctx*, const float* src, const float* mask, int64_t nx, int64_t ny, int64_t nz,
                               int find_minima, int find_maxima, float minima_threshold, float maxima_threshold,
                               int connectivity, int allow_borders,
                               int64_t* min_index, float* min_score, int64_t* min_nvoxels, int64_t min_cap, int64_t* n_min,
                               int64_t* max_index, float* max_score, int64_t* max_nvoxels, int64_t max_cap, int64_t* n_max,
                               int32_t* labels);

/* ---- m3: watershed segmentation, Watershed (lib/visfd/segmentation.hpp:65-559) --------------------------------------- */
/* Meyer's flood from the image's local minima (start_from_minima) or maxima, or from markers.  s = value, or -value when
 * starting from maxima; a voxel is eligible when mask != 0 and s <= SIGN * halt_threshold.  The seeds are the plateaus
 * that visfd_hip_find_extrema lists with that threshold and allow_borders, numbered 0 .. n-1 in its list order; basin k
 * is labelled k + 1.  With show_boundaries a voxel that meets an already labelled voxel of another basin becomes
 * boundary.  labels (int32) is written everywhere: basin numbers, label_boundary on boundaries, label_undefined on
 * unmasked voxels that are not eligible (or were never reached), and -1 where mask == 0 whatever label_undefined is (the
 * reference initialises its image to -1 and relabels unmasked voxels only).  DESIGN.md 4.8 states the result as a function
 * of each voxel's neighbourhood; without markers the context faces compute that on the device (csrc/watershed.hip).
 * markers (int32, NULL: none): the seeds are then the first voxel in raster order of each distinct positive label on a
 * voxel with mask != 0, numbered by first appearance, and basins get their marker's label back at the end (the reference's
 * relabelling with its quirks: unmapped labels become label_undefined).  Marked calls run the sequential flood on the
 * host on every face (the _dev face copies down and back and waits for the stream).
 * halt_threshold is taken as given: Watershed's replacement of +inf by -inf when starting from maxima is the caller's
 * (visfd_hip.hpp and filter_mrc do it).  connectivity 1, 2, 3 as for visfd_hip_find_extrema, whose size limits hold too.
 * basin_index / basin_score (host arrays on every face, each may be NULL): the seeds' voxel index ix + nx * (iy + ny * iz)
 * and value.  *n_basins receives the count on every return but VISFD_HIP_EINVAL and device failures (the image is refused
 * before its seeds are sought); basin_cap == 0 writes nothing of the lists; 0 < basin_cap < count: VISFD_HIP_ECAPACITY,
 * and nothing but the count is written (labels neither).
 * VISFD_HIP_EINVAL, labels untouched: an unmasked NaN voxel or a NaN threshold (the flood's heap order is then no strict
 * weak order); connectivity outside 1..3; the size limits; more than 2^24 basins (the reference carries the basin through a
 * float); labels overlapping src, mask or markers.
 * Both context faces return with the context's stream idle.  Temporaries of the device path: 10 bytes per voxel (kind,
 * link, carried basin, one byte of feeder marks and then boundary states) next to the 9 of the seed search, 4 bytes per basin; the host face stages src,
 * mask and labels (4 bytes per voxel each).  visfd_hip_watershed_host needs no context and no device. */
#define VISFD_HIP_WATERSHED_MAX_BASINS 16777216
int visfd_hip_watershed_host(const float* src, const float* mask, const int32_t* markers, int64_t nx, int64_t ny, int64_t nz,
                             float halt_threshold, int start_from_minima, int connectivity, int show_boundaries,
                             int32_t label_boundary, int32_t label_undefined, int32_t* labels,
                             int64_t* basin_index, float* basin_score, int64_t basin_cap, int64_t* n_basins);
int visfd_hip_watershed(visfd_hip_ctx*, const float* src, const float* mask, const int32_t* markers, int64_t nx, int64_t ny,
                        int64_t nz, float halt_threshold, int start_from_minima, int connectivity, int show_boundaries,
                        int32_t label_boundary, int32_t label_undefined, int32_t* labels,
                        int64_t* basin_index, float* basin_score, int64_t basin_cap, int64_t* n_basins);
int visfd_hip_watershed_dev(visfd_hip_ctx*, const float* src, const float* mask, const int32_t* markers, int64_t nx,
                            int64_t ny, int64_t nz, float halt_threshold, int start_from_minima, int connectivity,
                            int show_boundaries, int32_t label_boundary, int32_t label_undefined, int32_t* labels,
                            int64_t* basin_index, float* basin_score, int64_t basin_cap, int64_t* n_basins);
/* the context's last successful watershed call: out[0] the path it took, out[1] label rounds (launches of the propagation
 * kernel, the final unchanged one included), out[2] boundary rounds, out[3] basins; all -1 before the first call, rounds 0
 * on the host path */
#define VISFD_HIP_WATERSHED_PATH_HOST 0
#define VISFD_HIP_WATERSHED_PATH_DEVICE 1
int visfd_hip_watershed_last_stats(visfd_hip_ctx*, int64_t out[4]);

/* ---- a6: ApplyDog, lib/visfd/filter3d.hpp:1338-1402 -------------------------------------------- */
int visfd_hip_apply_dog(visfd_hip_ctx*, const float* src, float* dst, const float* mask,
                        int64_t nx, int64_t ny, int64_t nz, const float sigma_a[3],
                        const float sigma_b[3], const int halfwidth[3], float* A_out, float* B_out);
int visfd_hip_apply_dog_dev(visfd_hip_ctx*, const float* src, float* dst, const float* mask,
                            int64_t nx, int64_t ny, int64_t nz, const float sigma_a[3],
                            const float sigma_b[3], const int halfwidth[3], float* A_out,
                            float* B_out);

/* ---- a7: ApplyLog(sigma[3], delta, ratio), lib/visfd/filter3d.hpp:1428-1507 -------------------- */
int visfd_hip_apply_log(visfd_hip_ctx*, const float* src, float* dst, const float* mask,
                        int64_t nx, int64_t ny, int64_t nz, const float sigma[3],
                        float delta_sigma_over_sigma, float truncate_ratio, float* A_out,
                        float* B_out);
int visfd_hip_apply_log_dev(visfd_hip_ctx*, const float* src, float* dst, const float* mask,
                            int64_t nx, int64_t ny, int64_t nz, const float sigma[3],
                            float delta_sigma_over_sigma, float truncate_ratio, float* A_out,
                            float* B_out);

/* ---- a8: BlobDog, lib/visfd/feature.hpp:53-427 -------------------------------------------------- */
/* One record per detected blob.  ix,iy,iz are voxel indices (the reference stores them as floats,
 * feature.hpp:275-279); scale = index into blob_sigma[] of the blob's scale (ir-1 in the reference);
 * score = LoG value.  Lists are returned sorted by (scale, iz, iy, ix): the reference's in-memory
 * order depends on OpenMP scheduling (feature.hpp:310-345) and its callers sort anyway
 * (bin/filter_mrc/handlers.cpp:876-909). */
typedef struct visfd_hip_blob {
  int32_t ix, iy, iz;
  int32_t scale;
  float sigma; /* blob_sigma[scale] */
  float score;
} visfd_hip_blob;

/* aspect_ratio: NULL = {1,1,1}.  minima/maxima thresholds and use_threshold_ratios as
 * feature.hpp:72-74 (pass +INFINITY / -INFINITY to disable).  With ratios the thresholds are multiplied by the best
 * scores unconditionally, as the reference does (feature.hpp:369-372), so an infinite ratio is NOT "disabled":
 *   minima_threshold = +inf with a finite maxima ratio: no minimum is kept (inf * negative best = -inf);
 *   maxima_threshold = -inf: no maximum is ever recorded (feature.hpp:286-289: -inf * (-1) = +inf in every thread).
 * ONE FENCE: with BOTH sides infinite in ratio mode the reference keeps, of the minima, the first one each OpenMP
 * thread meets (its result depends on the thread count); this library returns all minima there (and no maxima).
 * NaN / Inf voxels propagate as in the reference (every comparison with a NaN is false in its scan, feature.hpp:245-304):
 * same lists (tests/test_gpu_parity.py::test_blob_detection_with_non_finite_voxels).
 * src and mask are HOST pointers in the first form, DEVICE pointers in the _dev form; the blob lists are always host
 * arrays of the given capacities.  Planes (nx * ny) of 2^29 voxels and more are VISFD_HIP_EINVAL (the scan addresses a
 * plane through one 2 GiB buffer descriptor). */
int visfd_hip_blob_dog(visfd_hip_ctx*, const float* src, const float* mask,
                       int64_t nx, int64_t ny, int64_t nz, const float* blob_sigma, int n_sigma,
                       const float* aspect_ratio, float delta_sigma_over_sigma,
                       float truncate_ratio, float minima_threshold, float maxima_threshold,
                       int use_threshold_ratios,
                       visfd_hip_blob* minima, int64_t minima_capacity, int64_t* n_minima,
                       visfd_hip_blob* maxima, int64_t maxima_capacity, int64_t* n_maxima);
int visfd_hip_blob_dog_dev(visfd_hip_ctx*, const float* src, const float* mask,
                           int64_t nx, int64_t ny, int64_t nz, const float* blob_sigma,
                           int n_sigma, const float* aspect_ratio, float delta_sigma_over_sigma,
                           float truncate_ratio, float minima_threshold, float maxima_threshold,
                           int use_threshold_ratios,
                           visfd_hip_blob* minima, int64_t minima_capacity, int64_t* n_minima,
                           visfd_hip_blob* maxima, int64_t maxima_capacity, int64_t* n_maxima);
/* The same detector in two halves, for hosts that have more work for the context's stream (ABI >= 9; no reference counterpart:
 * BlobDog is one call there).  `begin` queues every filter and scan and fetches the lists of all scales but the last few; `end`
 * fetches those, repeats scales whose buffers overflowed, merges, and hands the lists over exactly as visfd_hip_blob_dog_dev does.
 * Between the two the caller may queue other calls of the SAME context (a membrane stage): the device then goes from the last
 * scan straight into that work instead of idling through the host's list handling.  ANY call of the context is allowed
 * there -- larger volumes, another blob call or a second `begin`, visfd_hip_trim, changed options: a pending scan keeps the
 * buffers and capacities it was launched with, and whatever would free or overwrite those first fetches the job's
 * lists to the host (which waits for the job's scans; a membrane stage with a caller-supplied `dir` never does that).  src and
 * mask must stay unchanged until `end` returns.  VISFD_HIP_ECAPACITY from `end` leaves the job alive and returns the counts:
 * call `end` again with room for them; every other return value of `end` -- a refused argument included -- and
 * visfd_hip_blob_dog_abort free the job.  visfd_hip_destroy aborts the context's live jobs.  A handle that is not live
 * (ended, aborted, destroyed with its context) is never dereferenced: `end` answers VISFD_HIP_EINVAL, `abort` does nothing. */
typedef struct visfd_hip_blob_job visfd_hip_blob_job;
int visfd_hip_blob_dog_begin_dev(visfd_hip_ctx*, const float* src, const float* mask,
                                 int64_t nx, int64_t ny, int64_t nz, const float* blob_sigma,
                                 int n_sigma, const float* aspect_ratio, float delta_sigma_over_sigma,
                                 float truncate_ratio, float minima_threshold, float maxima_threshold,
                                 int use_threshold_ratios, visfd_hip_blob_job** job_out);
int visfd_hip_blob_dog_end(visfd_hip_blob_job* job,
                           visfd_hip_blob* minima, int64_t minima_capacity, int64_t* n_minima,
                           visfd_hip_blob* maxima, int64_t maxima_capacity, int64_t* n_maxima);
void visfd_hip_blob_dog_abort(visfd_hip_blob_job* job);
/* the context's live blob jobs: begun, and neither ended nor aborted */
int visfd_hip_blob_jobs_pending(visfd_hip_ctx* ctx);
/* BlobDogD's conversions, lib/visfd/feature.hpp:475 and :504 */
int visfd_hip_blob_diameters_to_sigmas(const float* diameters, int n, float* sigmas);
int visfd_hip_blob_sigmas_to_diameters(const float* sigmas, int n, float* diameters);

/* ---- f3: blob list post-processing (host-side; these take no context and touch no device) --------
 * Lists are three parallel arrays: crds[n][3] (x,y,z in voxels), diameters[n], scores[n]. */
enum {   /* SortCriteria, lib/visfd/visfd_utils.hpp:49-55 */
  VISFD_HIP_DO_NOT_SORT = 0,
  VISFD_HIP_SORT_DECREASING = 1,
  VISFD_HIP_SORT_INCREASING = 2,
  VISFD_HIP_SORT_DECREASING_MAGNITUDE = 3,
  VISFD_HIP_SORT_INCREASING_MAGNITUDE = 4
};
/* CalcSphereOverlap, lib/visfd/visfd_utils.hpp:95-118: volume shared by two spheres */
float visfd_hip_sphere_overlap(float rij, float ri, float rj);
/* SortBlobs, lib/visfd/feature.hpp:519-616: reorders the three arrays; `permutation` (nullable, n
 * entries) receives the original index of every new position.  Ties keep the reference's order:
 * (key, index) ascending, or exactly the reverse of that. */
int visfd_hip_sort_blobs(float* crds, float* diameters, float* scores, int64_t n, int sort_criteria,
                         int ascending_order, uint64_t* permutation);
/* DiscardMaskedBlobs, lib/visfd/feature.hpp:924-969: drops blobs whose centre voxel
 * floor(x+0.5) has mask == 0; *n is updated.  mask == NULL keeps everything.  A centre outside the
 * mask image is VISFD_HIP_EINVAL (the reference reads out of bounds). */
int visfd_hip_discard_masked_blobs(float* crds, float* diameters, float* scores, int64_t* n,
                                   const float* mask, int64_t nx, int64_t ny, int64_t nz);
/* DiscardOverlappingBlobs, lib/visfd/feature.hpp:720-913: sorts by `sort_criteria` (best first), then
 * keeps a blob unless an already-kept blob it meets in the coarse occupancy grid (cell = `scale`
 * voxels, reference default 6) is closer than (ri+rk)*min_radial_separation_ratio or overlaps more
 * than the given volume fractions (infinity disables a criterion).  *n is updated. */
int visfd_hip_discard_overlapping_blobs(float* crds, float* diameters, float* scores, int64_t* n,
                                        float min_radial_separation_ratio,
                                        float max_volume_overlap_large, float max_volume_overlap_small,
                                        int sort_criteria, int scale);
/* The same on a context's device (csrc/discard_overlap.hip): the reference's bits always, computed on the device for
 * every list outside the hand-over set.  The greedy walk is order-free -- a blob is kept exactly when no kept blob
 * BEFORE it in the sorted list both shares a cell of the occupancy grid with it and meets the discard criterion -- so
 * the device ranks the list (stable radix sort of score or |score|, ties as std::pair orders them), buckets the blobs by
 * centre cell and settles the recursion in rounds, one launch per round; the round count is the longest chain of
 * dependencies in the list.
 *   _ctx   host arrays, staged through the context's workspace
 *   _dev   device arrays, in place; *n (a HOST word) is read and written.  Both return with the stream idle.
 * The hand-over set, for which the call runs visfd_hip_discard_overlapping_blobs unchanged and says so: a non-finite
 * coordinate, diameter or score; a diameter < 0; n >= 2^31; bounds outside the int range; more than 2^27 cells in the
 * table or in the range of the centre cells.  A list that needs more rounds than the option discard_overlap_max_rounds
 * (default 256: a cap, random lists need a dozen) is finished by the host walk from the states reached, same bits.
 * Option discard_overlap_host (VISFD_HIP_DISCARD_OVERLAP_HOST) 1: both faces run the host entry. */
int visfd_hip_discard_overlapping_blobs_ctx(visfd_hip_ctx*, float* crds, float* diameters, float* scores, int64_t* n,
                                            float min_radial_separation_ratio, float max_volume_overlap_large,
                                            float max_volume_overlap_small, int sort_criteria, int scale);
int visfd_hip_discard_overlapping_blobs_dev(visfd_hip_ctx*, float* crds, float* diameters, float* scores, int64_t* n,
                                            float min_radial_separation_ratio, float max_volume_overlap_large,
                                            float max_volume_overlap_small, int sort_criteria, int scale);
/* the context's last _ctx / _dev call: info[0] path (VISFD_HIP_DISCARD_OVERLAP_PATH_*, -1 before the first call),
 * [1] reason (VISFD_HIP_DISCARD_OVERLAP_REASON_*), [2] rounds launched, [3] blobs in, [4] blobs kept, [5] pairs that
 * reached the discard criterion, [6] pairs that reached the exact cell test, [7] table cells */
#define VISFD_HIP_DISCARD_OVERLAP_PATH_DEVICE 0
#define VISFD_HIP_DISCARD_OVERLAP_PATH_HOST 1          /* option discard_overlap_host */
#define VISFD_HIP_DISCARD_OVERLAP_PATH_HANDED_OVER 2   /* the host entry, or the host walk from the device's states */
#define VISFD_HIP_DISCARD_OVERLAP_REASON_NONE 0
#define VISFD_HIP_DISCARD_OVERLAP_REASON_NONFINITE 1
#define VISFD_HIP_DISCARD_OVERLAP_REASON_NEGATIVE 2    /* a diameter < 0 */
#define VISFD_HIP_DISCARD_OVERLAP_REASON_COUNT 3       /* n >= 2^31 */
#define VISFD_HIP_DISCARD_OVERLAP_REASON_BOUNDS 4      /* bounds outside the int range */
#define VISFD_HIP_DISCARD_OVERLAP_REASON_CELLS 5       /* more than 2^27 cells */
#define VISFD_HIP_DISCARD_OVERLAP_REASON_ROUNDS 6      /* the round cap */
int visfd_hip_discard_overlapping_blobs_last(visfd_hip_ctx*, int64_t info[8]);
/* option discard_overlap_time: milliseconds between events on the stream of the last _ctx / _dev call: the reduction with
 * its wait, ranking and records, buckets, the rounds with their waits, compaction; -1 for a phase that did not run */
int visfd_hip_discard_overlapping_blobs_last_times(visfd_hip_ctx*, float ms[5]);

/* ---- f3, continued: FindSpheres and the supervised score thresholds ("-auto-thresh score -supervised POS NEG") ----
 * FindSpheres, lib/visfd/visfd_utils.hpp:271-359: for every query point the sphere of the list that holds it, the LAST
 * one when several do.  The reference paints every sphere into an integer table as large as the bounding box of the
 * queries and reads the queries off it; here nothing is painted: the answer is, per query, the largest index among the
 * spheres that contain it, an integer max-reduction over (query, sphere) pairs.  Exact, the reference's arithmetic:
 *   query q[d]    = (int)crds[i][d], a truncation toward zero (-0.5 becomes 0)
 *   centre c[d]   = (int)sphere_crds[i][d], also a truncation; centres may lie anywhere, negative included
 *   R             = max(0, (int)ceil(diameter / 2 - 0.5)): the division in float, the rest in double
 *   Rsqr          = max(0, (int)ceil(SQR(diameter / 2) - 0.5)): the square in float, the rest in double
 *   i contains q  iff |q - c| <= R on every axis and |q - c|^2 <= Rsqr (integers).  A diameter <= 1, negative ones
 *                 included, has R = 0: its sphere is the centre voxel, whatever Rsqr is
 *   ids[k]        = 1 + the largest containing index, 0 when no sphere contains query k
 * crds: n_crds x 3 floats, sphere_crds: n_spheres x 3 floats, sphere_diameters: n_spheres floats, ids: n_crds int64.
 * VISFD_HIP_EINVAL, ids untouched: a query whose truncation is negative (the reference reads outside its table), a
 * non-finite coordinate or diameter, R > VISFD_HIP_FIND_SPHERES_MAX_R, n_spheres >= 2^31, a null array with a non-zero
 * count.  n_crds == 0 and n_spheres == 0 are valid (nothing written; all zeros).  Coordinates beyond the int range
 * saturate (the reference's conversion is undefined there).
 *   visfd_hip_find_spheres_host   no context, no device: a walk over the pairs
 *   visfd_hip_find_spheres        host arrays, staged through the context's workspace; the search runs on the device
 *                                 (csrc/find_spheres.hip); what it checks it checks on the host, before anything is launched
 *   visfd_hip_find_spheres_dev    device arrays (ids: int64 on the device).  The values are checked by the two
 *                                 preparation launches, whose one flag word the call waits for; the search itself is
 *                                 asynchronous on the context's stream
 * Context option find_spheres_host (VISFD_HIP_FIND_SPHERES_HOST): the two context faces run the host walk instead. */
#define VISFD_HIP_FIND_SPHERES_MAX_R 46340
int visfd_hip_find_spheres_host(const float* crds, int64_t n_crds, const float* sphere_crds, const float* sphere_diameters,
                                int64_t n_spheres, int64_t* ids);
int visfd_hip_find_spheres(visfd_hip_ctx*, const float* crds, int64_t n_crds, const float* sphere_crds,
                           const float* sphere_diameters, int64_t n_spheres, int64_t* ids);
int visfd_hip_find_spheres_dev(visfd_hip_ctx*, const float* crds, int64_t n_crds, const float* sphere_crds,
                               const float* sphere_diameters, int64_t n_spheres, int64_t* ids);
/* what the context's last FindSpheres call ran: VISFD_HIP_FIND_SPHERES_PATH_* (-1 before the first call) */
#define VISFD_HIP_FIND_SPHERES_PATH_DEVICE 0
#define VISFD_HIP_FIND_SPHERES_PATH_HOST 1     /* option find_spheres_host */
int visfd_hip_find_spheres_last_path(visfd_hip_ctx*, int* path);

/* ChooseThreshold1D, lib/visfd/visfd_utils.hpp:373-516: the score threshold with the fewest misclassified training
 * data (accepted[i] != 0: a positive), the median one of those that tie; -+infinity when accepting or rejecting
 * everything is best.  is_lower_bound == 0: data BELOW the threshold are accepted.  Ties of the (score, index) sort and
 * the float / double steps of the midpoint are the reference's. */
int visfd_hip_choose_threshold_1d(const float* scores, const unsigned char* accepted, int64_t n, int is_lower_bound,
                                  float* threshold);
/* The four below take a NULLABLE context: with NULL the spheres are searched by visfd_hip_find_spheres_host, otherwise
 * by visfd_hip_find_spheres on that context.
 * _FindBlobScores, lib/visfd/feature_implementation.hpp:48-89: a copy of the blob list is sorted by
 * visfd_hip_sort_blobs(sort_criteria, ascending) -- increasing priority -- and searched; scores[k] is the score of the
 * blob that holds training point k (-infinity when none does), sphere_ids[k] (nullable) its position in the SORTED list
 * plus one (0: none). */
int visfd_hip_find_blob_scores(visfd_hip_ctx*, const float* training_crds, int64_t n_training, const float* blob_crds,
                               const float* blob_diameters, const float* blob_scores, int64_t n_blobs, int sort_criteria,
                               float* scores, int64_t* sphere_ids);
/* ChooseBlobScoreThresholds[Multi], lib/visfd/feature.hpp:988-1111, feature_implementation.hpp:136-457: the training
 * points (positives first, then negatives; set after set) that lie in a blob take that blob's score, the others are
 * dropped; the interval [*lower, *upper] is chosen lower bound first and upper bound first, and the attempt with no more
 * mistakes than the other is kept.  report[4] (nullable) = false positives, negatives, false negatives, positives: the
 * numbers of the reference's progress report.  No negative or no positive left after dropping: VISFD_HIP_EINVAL, with
 * the reference's message in visfd_hip_last_error.  The multi form takes the sets' arrays concatenated and their counts. */
int visfd_hip_choose_blob_score_thresholds(visfd_hip_ctx*, const float* blob_crds, const float* blob_diameters,
                                           const float* blob_scores, int64_t n_blobs, const float* pos_crds, int64_t n_pos,
                                           const float* neg_crds, int64_t n_neg, int sort_criteria, float* lower,
                                           float* upper, int64_t* report);
int visfd_hip_choose_blob_score_thresholds_multi(visfd_hip_ctx*, int64_t n_sets, const float* blob_crds,
                                                 const float* blob_diameters, const float* blob_scores,
                                                 const int64_t* n_blobs, const float* pos_crds, const int64_t* n_pos,
                                                 const float* neg_crds, const int64_t* n_neg, int sort_criteria,
                                                 float* lower, float* upper, int64_t* report);
/* DiscardBlobsByScoreSupervised, lib/visfd/feature.hpp:1124-1180: the thresholds as above, then the blobs with
 * lower <= score <= upper are kept in list order; *n is updated. */
int visfd_hip_discard_blobs_by_score_supervised(visfd_hip_ctx*, float* crds, float* diameters, float* scores, int64_t* n,
                                                const float* pos_crds, int64_t n_pos, const float* neg_crds, int64_t n_neg,
                                                int sort_criteria, float* lower, float* upper, int64_t* report);

/* ---- f1: LabelConnected, lib/visfd/connect.hpp:168-1427 (host-side: a sequential priority flood) ------
 * Clusters the voxels whose saliency passes `threshold_saliency` into connected "islands", growing from the
 * local saliency maxima (minima if start_from_saliency_maxima == 0) in order of decreasing saliency and merging
 * islands that touch.  labels[nz][ny][nx] receives 1..n_clusters (1 = largest when sort_by_size != 0, otherwise
 * ordered by the height of the seeding maximum) and `label_undefined` for unclustered voxels; voxels with
 * mask == 0 receive the value n_seeds + 1 as in the reference (connect.hpp:1401-1403 skips them).
 * direction (nullable, [nz][ny][nx][3]) and tensor (nullable, [nz][ny][nx][6] = xx,yy,zz,xy,yz,xz) switch on the
 * compatibility tests of connect.hpp:455-553 and :625-672 with the four cosine thresholds (values below -1
 * disable a test; with consider_dot_product_sign == 0 negative vector thresholds become 0).  When
 * standardize_directions != 0 (and signs are ignored) `direction` is rewritten in place with consistent,
 * outward-pointing signs (the reference's aaaafVectorStandardized aliasing its aaaafVector, as in
 * handlers.cpp:1985-2013).  Per-cluster outputs (each nullable; cluster_capacity entries): seed position
 * x,y,z in final cluster order; sizes and seed saliencies in the provisional (seed-height) order -- the
 * reference only permutes the positions (connect.hpp:1294-1348).  Every dimension must be >= 3.
 * The _ex form adds the reference's remaining optional arguments:
 *   voxel_weights [nz][ny][nx] (nullable): a cluster's "size" is the sum of its voxels' weights (connect.hpp:1154-1183);
 *   must-link constraints (connect.hpp:829-1045): n groups of locations (x,y,z, voxels; must_link_crds[total][3],
 *   must_link_group_sizes[n]); the clusters of the clustered voxels nearest to consecutive locations of a group are
 *   merged.  must_link_directions (nullable, one per location): 0 = the two surfaces face the same way, 1 = opposite,
 *   2 = decide from the angles their normals make with the joining line (DirectionPairType). */
int visfd_hip_label_connected(const float* saliency, int64_t* labels, const float* mask, int64_t nx, int64_t ny,
                              int64_t nz, float threshold_saliency, float* direction,
                              float threshold_vector_saliency, float threshold_vector_neighbor,
                              int consider_dot_product_sign, const float* tensor,
                              float threshold_tensor_saliency, float threshold_tensor_neighbor,
                              int tensor_is_positive_definite_near_target, int connectivity,
                              int64_t label_undefined, int sort_by_size, int standardize_directions,
                              int start_from_saliency_maxima, int64_t* n_clusters, float* cluster_maxima,
                              float* cluster_sizes, float* cluster_saliencies, int64_t cluster_capacity);
int visfd_hip_label_connected_ex(const float* saliency, int64_t* labels, const float* mask, int64_t nx, int64_t ny,
                              int64_t nz, float threshold_saliency, float* direction,
                              float threshold_vector_saliency, float threshold_vector_neighbor,
                              int consider_dot_product_sign, const float* tensor,
                              float threshold_tensor_saliency, float threshold_tensor_neighbor,
                              int tensor_is_positive_definite_near_target, int connectivity,
                              int64_t label_undefined, int sort_by_size, int standardize_directions,
                              int start_from_saliency_maxima, int64_t* n_clusters, float* cluster_maxima,
                              float* cluster_sizes, float* cluster_saliencies, int64_t cluster_capacity,
                                 const float* voxel_weights, const float* must_link_crds,
                                 const int64_t* must_link_group_sizes, int64_t must_link_ngroups,
                                 const int* must_link_directions);

/* visfd_hip_label_connected_ex with its SEED SEARCH on a context's device: the same arguments after the context (host
 * arrays), the same results bit for bit.  Only the seeds -- the plateau-aware extrema of the whole image, the part of the
 * call that looks at every voxel -- are found on the device, by the kernels of visfd_hip_find_extrema (saliency and mask
 * are staged through the workspace); the flood from them is the sequential one of the host, unchanged.  This is not a
 * device implementation of LabelConnected, and it reports no fallback reasons: DESIGN.md 4.13 says what stands in the way
 * of one and leaves the names such a face would take free.
 * Refused before anything is allocated or copied (VISFD_HIP_EINVAL): a null context or image, a dimension below 3, an
 * image of 2^31 voxels or more, connectivity < 1.  Where the device search does not reach -- connectivity above
 * VISFD_HIP_EXTREMA_MAX_CONNECTIVITY, more than VISFD_HIP_EXTREMA_MAX_VOXELS voxels, ny or nz above
 * VISFD_HIP_EXTREMA_MAX_NY_NZ, 2^24 tiles of 64 x 8 x 8 or more -- the host searches the seeds as well.
 * visfd_hip_label_connected_device_seeds_last: where the context's last successful call searched its seeds
 * (VISFD_HIP_CONNECT_SEEDS_*; -1 before the first) and, nullable, the length of the device's list (-1 on the host). */
#define VISFD_HIP_CONNECT_SEEDS_DEVICE 0
#define VISFD_HIP_CONNECT_SEEDS_HOST 1
int visfd_hip_label_connected_device_seeds(visfd_hip_ctx*, const float* saliency, int64_t* labels, const float* mask,
                                           int64_t nx, int64_t ny, int64_t nz, float threshold_saliency, float* direction,
                                           float threshold_vector_saliency, float threshold_vector_neighbor,
                                           int consider_dot_product_sign, const float* tensor,
                                           float threshold_tensor_saliency, float threshold_tensor_neighbor,
                                           int tensor_is_positive_definite_near_target, int connectivity,
                                           int64_t label_undefined, int sort_by_size, int standardize_directions,
                                           int start_from_saliency_maxima, int64_t* n_clusters, float* cluster_maxima,
                                           float* cluster_sizes, float* cluster_saliencies, int64_t cluster_capacity,
                                           const float* voxel_weights, const float* must_link_crds,
                                           const int64_t* must_link_group_sizes, int64_t must_link_ngroups,
                                           const int* must_link_directions);
int visfd_hip_label_connected_device_seeds_last(visfd_hip_ctx*, int* where, int64_t* n_seeds);

/* LabelConnected AS A GRAPH PROBLEM: a voxel is valid when it is unmasked and passes the saliency, tensor
 * and vector tests; two valid neighbours are joined when their neighbour tests pass in both directions; a cluster is a
 * connected component of that graph that holds a valid seed.  The arguments are those of
 * visfd_hip_label_connected_device_seeds.  What a successful call returns:
 *   - labels, n_clusters, cluster_maxima, cluster_sizes and cluster_saliencies: the same bits as
 *     visfd_hip_label_connected_ex on the same inputs (masked voxels get n_seeds + 1, as there);
 *   - with standardize_directions (and signs ignored), the direction of every voxel that ends up labelled: the same bits
 *     as after visfd_hip_label_connected_ex;
 *   - the direction of EVERY OTHER voxel, unlabelled or masked: bit for bit what the caller passed in.  This is where
 *     these entries differ from the four above: the flood also turns the directions of a halo of unlabelled voxels around
 *     every cluster, in a way its pop order decides, and the entries above reproduce that; these leave the halo alone.
 *     Nothing in this library reads those directions.
 * visfd_hip_label_connected_graph       host arrays; the work runs on the context's device (csrc/connect_graph.hip), except
 *                                       the vector test, which the host runs over the list of candidates the device compacts
 * visfd_hip_label_connected_graph_dev   saliency, mask, direction, tensor, labels (and voxel_weights) are device arrays, the
 *                                       per-cluster outputs host arrays; returns with the stream idle
 * visfd_hip_label_connected_graph_host  no context and no device: a serial walk of the same definition
 *                                       (its guard on the outward sum is count * max|term| * 2^-20; the device's is the
 *                                       looser count * B * 2^-20, B = max (|r_x| + |r_y| + |r_z|) * max|n_d|, so the device
 *                                       may report OUTWARD where the walk does not; the results agree either way)
 * Calls whose result the pop order does decide carry a reason (VISFD_HIP_CONNECT_REASON_*): both directed tests of a
 * pair of valid voxels disagree; an edge's dot product is exactly zero while standardising; a component's signs cannot
 * be made consistent; must-link constraints; voxel weights; a cluster's outward sum is too near zero for its sign to be
 * certain; connectivity above 3, an image the device's seed search does not take (VISFD_HIP_EXTREMA_MAX_*), or
 * 2^31 - 2 voxels or more (the union-find word is (index << 1) | sign).  Such a call is handed to the flood (from the
 * seeds already found; the _dev face on a staged copy), the labelled results are the flood's, and the directions of the
 * unlabelled and masked voxels are put back to their input bits, so the contract above holds on every path.
 * Refused before anything is allocated or copied (VISFD_HIP_EINVAL): what visfd_hip_label_connected_device_seeds refuses.
 * visfd_hip_label_connected_graph_last: what the context's last successful call did -- path (VISFD_HIP_CONNECT_GRAPH_*; -1
 * before the first), and, each nullable, the reason bits, the number of valid voxels and the number of candidates the
 * host's vector test looked at (0 without directions; both -1 where the call was handed over before counting).  With a
 * null context: the calling thread's last visfd_hip_label_connected_graph_host.
 * visfd_hip_label_connected_graph_last_settled: with the option connect_settle, MUST_LINK, WEIGHTS and OUTWARD are no reasons
 * for visfd_hip_label_connected_graph and _graph_dev (the other reasons hand over as before, and a must-link location
 * beyond 2^20 voxels from the origin, or 2^33 or more squared voxels from a corner of the image, is LIMITS); *settled gets
 * the bits of those three that the context's last device-path call settled itself -- OUTWARD only if a cluster's sum
 * was in doubt -- and 0 after a call that took the flood or ran with the option off.
 * visfd_hip_label_connected_graph_last_times: with the option connect_time, the milliseconds of the last device-path
 * call by stage: seed search, classify and compact, host vector test, edges and union-find, clusters, directions and
 * the last pass, copies to the device, copies to the host. */
#define VISFD_HIP_CONNECT_GRAPH_DEVICE 0
#define VISFD_HIP_CONNECT_GRAPH_HOST_GRAPH 1
#define VISFD_HIP_CONNECT_GRAPH_FLOOD 2
#define VISFD_HIP_CONNECT_REASON_ASYMMETRIC 1
#define VISFD_HIP_CONNECT_REASON_ZERO_DOT 2
#define VISFD_HIP_CONNECT_REASON_UNBALANCED 4
#define VISFD_HIP_CONNECT_REASON_MUST_LINK 8
#define VISFD_HIP_CONNECT_REASON_WEIGHTS 16
#define VISFD_HIP_CONNECT_REASON_OUTWARD 32
#define VISFD_HIP_CONNECT_REASON_LIMITS 64
int visfd_hip_label_connected_graph(visfd_hip_ctx*, const float* saliency, int64_t* labels, const float* mask,
                                    int64_t nx, int64_t ny, int64_t nz, float threshold_saliency, float* direction,
                                    float threshold_vector_saliency, float threshold_vector_neighbor,
                                    int consider_dot_product_sign, const float* tensor,
                                    float threshold_tensor_saliency, float threshold_tensor_neighbor,
                                    int tensor_is_positive_definite_near_target, int connectivity,
                                    int64_t label_undefined, int sort_by_size, int standardize_directions,
                                    int start_from_saliency_maxima, int64_t* n_clusters, float* cluster_maxima,
                                    float* cluster_sizes, float* cluster_saliencies, int64_t cluster_capacity,
                                    const float* voxel_weights, const float* must_link_crds,
                                    const int64_t* must_link_group_sizes, int64_t must_link_ngroups,
                                    const int* must_link_directions);
int visfd_hip_label_connected_graph_dev(visfd_hip_ctx*, const float* saliency, int64_t* labels, const float* mask,
                                        int64_t nx, int64_t ny, int64_t nz, float threshold_saliency, float* direction,
                                        float threshold_vector_saliency, float threshold_vector_neighbor,
                                        int consider_dot_product_sign, const float* tensor,
                                        float threshold_tensor_saliency, float threshold_tensor_neighbor,
                                        int tensor_is_positive_definite_near_target, int connectivity,
                                        int64_t label_undefined, int sort_by_size, int standardize_directions,
                                        int start_from_saliency_maxima, int64_t* n_clusters, float* cluster_maxima,
                                        float* cluster_sizes, float* cluster_saliencies, int64_t cluster_capacity,
                                        const float* voxel_weights, const float* must_link_crds,
                                        const int64_t* must_link_group_sizes, int64_t must_link_ngroups,
                                        const int* must_link_directions);
int visfd_hip_label_connected_graph_host(const float* saliency, int64_t* labels, const float* mask,
                                         int64_t nx, int64_t ny, int64_t nz, float threshold_saliency, float* direction,
                                         float threshold_vector_saliency, float threshold_vector_neighbor,
                                         int consider_dot_product_sign, const float* tensor,
                                         float threshold_tensor_saliency, float threshold_tensor_neighbor,
                                         int tensor_is_positive_definite_near_target, int connectivity,
                                         int64_t label_undefined, int sort_by_size, int standardize_directions,
                                         int start_from_saliency_maxima, int64_t* n_clusters, float* cluster_maxima,
                                         float* cluster_sizes, float* cluster_saliencies, int64_t cluster_capacity,
                                         const float* voxel_weights, const float* must_link_crds,
                                         const int64_t* must_link_group_sizes, int64_t must_link_ngroups,
                                         const int* must_link_directions);
int visfd_hip_label_connected_graph_last(visfd_hip_ctx*, int* path, unsigned* reasons, int64_t* n_valid,
                                         int64_t* n_undecided);
int visfd_hip_label_connected_graph_last_settled(visfd_hip_ctx*, unsigned* settled);
int visfd_hip_label_connected_graph_last_times(visfd_hip_ctx*, float ms[8]);

/* Principal eigenvector (eigenvector row 0 of ConvertFlatSym2Evects3 in the given order) of nvox flat tensors
 * [nvox][6] -> direction [nvox][3], computed on the HOST in the reference's arithmetic (the loop of
 * bin/filter_mrc/handlers.cpp:1935-1952); voxels with mask == 0 (mask nullable) are left untouched. */
int visfd_hip_principal_directions_host(const float* tensor, const float* mask, int64_t nvox, int order,
                                        float* direction);
/* Post-vote score lambda0 - lambda1 (bin/filter_mrc/handlers.cpp:1868-1888) of nvox flat tensors on the HOST in
 * the reference's arithmetic (the device kernel visfd_hip_tensor_saliency agrees to ~1e-7 relative only);
 * used before visfd_hip_label_connected, whose flood order and thresholds act on this number. */
int visfd_hip_tensor_saliency_host(const float* tensor, const float* mask, int64_t nvox, int order,
                                   float* saliency);

/* DiagonalizeFlatSym3 (lib/visfd/eigen3_simple.hpp:271-342) of n interleaved flat matrices [n][6] ->
 * [n][lambda0,lambda1,lambda2, shoemake0..2] on the HOST, bit-identical to the reference (the form a caller uses
 * per voxel inside their own loops; visfd_hip_diagonalize_flat_sym3 is the device batch). order 0/1. */
int visfd_hip_diagonalize_flat_sym3_host(const float* m6, float* out6, int64_t n, int eival_order);
/* ConvertFlatSym2Evects3<float> (lib/visfd/eigen3_simple.hpp:392-405; decode lib/visfd/lin3_utils.hpp:566-584):
 * one flat symmetric matrix -> eigenvalues and eigenvectors as rows (row-major 3x3), host. */
int visfd_hip_convert_flat_sym2_evects3_host(const float* m6, int eival_order, float* eivals3, float* eivects9);
/* DiagonalizeSym3<float> (lib/visfd/eigen3_simple.hpp:137-266) on the host: m9 = symmetric 3x3, row-major;
 * eivects9 = eigenvectors as rows; order 0..3 = INCREASING, DECREASING, INCREASING_ABS, DECREASING_ABS_EIVALS. */
int visfd_hip_diagonalize_sym3_f32_host(const float* m9, int order, float* eivals3, float* eivects9);
/* The oriented point cloud of a clustered surface (the -normals-file tail of HandleTV,
 * bin/filter_mrc/handlers.cpp:2039-2309), host-side.  voxel2cluster = the label volume as floats (what HandleTV
 * writes to its output image; NULL: export every unmasked voxel unchanged), direction = [nz][ny][nx][3]
 * (standardized), select_cluster = the label to export, curve_ds / find_ridge / max_distance_to_feature = the
 * reference's settings (defaults 0.2, 1, 1.3 voxels; settings.cpp:147-149).  crds/norms receive n_points x 3
 * floats each (capacity points; pass NULL pointers to only count). */
int visfd_hip_surface_points(const float* saliency, const float* voxel2cluster, const float* direction,
                             const float* mask, int64_t nx, int64_t ny, int64_t nz, int select_cluster,
                             const float voxel_width[3], float curve_ds, int find_ridge,
                             float max_distance_to_feature, float* crds, float* norms, int64_t capacity,
                             int64_t* n_points);
/* The same points from a context's device: the selection and its raster-order list, the walks along the normals and the
 * gather of the ridge snap's Hessians and gradients run as kernels (csrc/surface_points.hip); the 3x3 eigen solve of the
 * snap, its rejections and the voxel_width scaling run on the host over the compacted points.  Points, normals, count and
 * order are those of visfd_hip_surface_points bit for bit, provided every direction a walk meets has a finite, non-zero
 * length (where one has not, the host's own conversion of a NaN to an index is undefined: the device ends that walk as if
 * it had left the image, reads nothing out of range, and still returns VISFD_HIP_OK).
 *   _ctx  host arrays, direction [nz][ny][nx][3]; crds / norms host [capacity][3].
 *   _dev  device arrays, direction channel-planar [3][nz][ny][nx]; crds / norms [capacity][3] in device or host memory.
 * One call counts and fills: with crds == norms == NULL it only counts; otherwise, when the points do not fit,
 * *n_points holds the needed count, crds / norms are left unwritten and the call returns VISFD_HIP_ECAPACITY.  Every
 * dimension must be at least 3 and below 2^24 (positions are floats); the voxel count is not limited to 2^31.
 * A walk takes at most `surface_steps_cap` steps per direction on the device (option, default 256).  A call in which a
 * walk needs more, or in which a walked point rounds to a voxel outside the image, is handed over to
 * visfd_hip_surface_points (the _dev entry brings the volumes to the host for it); visfd_hip_surface_points_last says so. */
int visfd_hip_surface_points_ctx(visfd_hip_ctx*, const float* saliency, const float* voxel2cluster, const float* direction,
                                 const float* mask, int64_t nx, int64_t ny, int64_t nz, int select_cluster,
                                 const float voxel_width[3], float curve_ds, int find_ridge,
                                 float max_distance_to_feature, float* crds, float* norms, int64_t capacity,
                                 int64_t* n_points);
int visfd_hip_surface_points_dev(visfd_hip_ctx*, const float* saliency, const float* voxel2cluster, const float* direction,
                                 const float* mask, int64_t nx, int64_t ny, int64_t nz, int select_cluster,
                                 const float voxel_width[3], float curve_ds, int find_ridge,
                                 float max_distance_to_feature, float* crds, float* norms, int64_t capacity,
                                 int64_t* n_points);
#define VISFD_HIP_SURFACE_POINTS_PATH_DEVICE 0
#define VISFD_HIP_SURFACE_POINTS_PATH_HANDED_OVER 1
#define VISFD_HIP_SURFACE_POINTS_REASON_STEPS 1u    /* a walk reached surface_steps_cap */
#define VISFD_HIP_SURFACE_POINTS_REASON_BOUNDS 2u   /* a walked point rounds to a voxel outside the image */
/* The context's last _ctx / _dev call: out[0] the path, out[1] the reason bits of a hand-over, out[2] the selected voxels,
 * out[3] the points, out[4] the longest walk in steps (one direction; on the device path), out[5] the steps all walks of
 * the device path took together (the last, failing step of each direction and the second walk to the two positions
 * around the average included).  -1, 0, -1, -1, -1, -1 before the first call. */
int visfd_hip_surface_points_last(visfd_hip_ctx*, int64_t out[6]);
/* Under the option surface_points_time: milliseconds of the last device-path call: select and compact, walk, ridge
 * gather (events on the stream), host finish with the copies out (host clock); -1 for a stage that did not run. */
int visfd_hip_surface_points_last_times(visfd_hip_ctx*, float ms[4]);

/* ---- f4: BinArray3D / UnbinArray3D, lib/visfd/resample.hpp:53-166 -------------------------------------
 * Sizes are {nx, ny, nz}.  bin[d] = floor(size_big[d] / size_small[d]); `offset` (nullable) shifts the
 * binning window and must satisfy 0 <= offset[d] < bin[d] (VISFD_HIP_EINVAL otherwise, where the
 * reference throws; also when the shifted window would leave the source, which the reference only
 * asserts).  Bin: dst = float sum over the bin in z,y,x order / bin volume; source voxels
 * beyond size_dst*bin are dropped.  Unbin: dst[I] = src[clamp((I - offset) / bin)]. */
int visfd_hip_bin_array3d(visfd_hip_ctx*, const float* src, const int64_t size_src[3], float* dst,
                          const int64_t size_dst[3], const int* offset);
int visfd_hip_bin_array3d_dev(visfd_hip_ctx*, const float* src, const int64_t size_src[3], float* dst,
                              const int64_t size_dst[3], const int* offset);
int visfd_hip_unbin_array3d(visfd_hip_ctx*, const float* src, const int64_t size_src[3], float* dst,
                            const int64_t size_dst[3], const int* offset);
int visfd_hip_unbin_array3d_dev(visfd_hip_ctx*, const float* src, const int64_t size_src[3], float* dst,
                                const int64_t size_dst[3], const int* offset);

/* ---- a9: CalcHessian, lib/visfd/feature.hpp:1203-1348 ------------------------------------------- */
/* gradient (nullable): 3 channels; hessian: 6 channels (xx,yy,zz,xy,yz,xz).  Voxels with mask==0
 * are left untouched.  Returns VISFD_HIP_EINVAL if any dimension < 3 (feature.hpp:1260-1264). */
int visfd_hip_calc_hessian(visfd_hip_ctx*, const float* src, float* gradient, float* hessian,
                           const float* mask, int64_t nx, int64_t ny, int64_t nz, float sigma,
                           float truncate_ratio);
int visfd_hip_calc_hessian_dev(visfd_hip_ctx*, const float* src, float* gradient, float* hessian,
                               const float* mask, int64_t nx, int64_t ny, int64_t nz, float sigma,
                               float truncate_ratio);

/* ---- a10: DiagonalizeFlatSym3 (batched), lib/visfd/eigen3_simple.hpp:271-342 -------------------- */
/* n matrices of 6 floats -> n x [lambda0,lambda1,lambda2, shoemake0..2]. Host: interleaved;
 * device: channel-planar with stride n. */
int visfd_hip_diagonalize_flat_sym3(visfd_hip_ctx*, const float* m6, float* out6, int64_t n,
                                    int eival_order);
int visfd_hip_diagonalize_flat_sym3_dev(visfd_hip_ctx*, const float* m6, float* out6, int64_t n,
                                        int eival_order);

/* ---- a12 (first half): ridge saliency + principal direction ------------------------------------- */
/* The per-voxel loop of HandleTV, bin/filter_mrc/handlers.cpp:1640-1746 (SURFACE_RIDGE, no
 * background subtraction): saliency = (l0^2-l1^2)^2 (feature.hpp:1557-1560), direction = first
 * eigenvector after the float Shoemake round trip (eigen3_simple.hpp:392-405).  saliency is zero
 * where mask==0; direction is written only where mask!=0. */
int visfd_hip_hessian_saliency(visfd_hip_ctx*, const float* hessian, const float* mask,
                               int64_t nvox, int eival_order, float* saliency, float* direction);
int visfd_hip_hessian_saliency_dev(visfd_hip_ctx*, const float* hessian, const float* mask,
                                   int64_t nvox, int eival_order, float* saliency,
                                   float* direction);
/* Fused form (no materialised Hessian): Gaussian smoothing + 19-point stencil + eigen + score.
 * Equivalent to calc_hessian followed by hessian_saliency.  Device face only. */
int visfd_hip_ridge_saliency_dev(visfd_hip_ctx*, const float* src, const float* mask,
                                 int64_t nx, int64_t ny, int64_t nz, float sigma,
                                 float truncate_ratio, int eival_order, float* saliency,
                                 float* direction);
/* The same in two steps, for callers that threshold the saliency before they need directions (HandleTV,
 * handlers.cpp:1751-1797): visfd_hip_ridge_scores_dev smooths and scores every voxel and hands back the smoothed
 * volume (`smoothed`: caller's buffer of nvox floats, distinct from src and saliency);
 * visfd_hip_ridge_directions_dev writes the principal direction (3 planes) of the voxels whose saliency is non-zero
 * and leaves the others untouched.  Scores and directions are bit-identical to visfd_hip_ridge_saliency_dev's. */
int visfd_hip_ridge_scores_dev(visfd_hip_ctx*, const float* src, const float* mask, int64_t nx, int64_t ny,
                               int64_t nz, float sigma, float truncate_ratio, int eival_order, float* saliency,
                               float* smoothed);
int visfd_hip_ridge_directions_dev(visfd_hip_ctx*, const float* smoothed, int64_t nx, int64_t ny, int64_t nz,
                                   float sigma, int eival_order, const float* saliency, float* direction);
/* The optional PEAK-HEIGHT factor of the two score loops (`-membrane-background SIGMA_B`, alias `-detection-background`;
 * bin/filter_mrc/settings.cpp:2802-2825): background = ApplyGauss(image, SIGMA_B, floor(SIGMA_B * ratio), mask, normalize)
 * (handlers.cpp:1577-1592), and every score is multiplied by (image - background) in float (handlers.cpp:1698-1702).
 * visfd_hip_peak_background_dev computes the background volume; visfd_hip_ridge_scores_bg_dev is
 * visfd_hip_ridge_scores_dev with the factor applied to every score (background == NULL: no factor). */
int visfd_hip_peak_background_dev(visfd_hip_ctx*, const float* image, const float* mask, int64_t nx, int64_t ny, int64_t nz,
                                  float sigma_background, float truncate_ratio, int normalize, float* background);
int visfd_hip_ridge_scores_bg_dev(visfd_hip_ctx*, const float* src, const float* mask, int64_t nx, int64_t ny,
                                  int64_t nz, float sigma, float truncate_ratio, int eival_order, const float* background,
                                  float* saliency, float* smoothed);

/* ---- a12 (second half): global top-fraction threshold, handlers.cpp:1751-1797 -------------------- */
/* threshold = (floor(n_unmasked*fraction))-th largest unmasked saliency; every voxel with
 * saliency < threshold is zeroed in place.  threshold_out nullable. */
int visfd_hip_threshold_fraction(visfd_hip_ctx*, float* saliency, const float* mask, int64_t nvox,
                                 float fraction, float* threshold_out);
int visfd_hip_threshold_fraction_dev(visfd_hip_ctx*, float* saliency, const float* mask,
                                     int64_t nvox, float fraction, float* threshold_out);
/* building blocks for the multi-GPU (Z-slab) form of the same select: the order-preserving 32-bit
 * key of the float is split into three digits (round 0: bits 31..21, round 1: bits 20..10, round 2:
 * bits 9..0); each call returns this rank's 2048-bin histogram of digit `round` over unmasked
 * voxels whose higher digits equal `prefix` (right-aligned; 0 for round 0).  The caller sums the
 * histograms across ranks, walks them from the top to find the digit of the k-th largest key, and
 * finally applies the threshold with visfd_hip_apply_threshold_dev.
 * visfd_amd/slab.py holds the host logic. */
int visfd_hip_select_histogram_dev(visfd_hip_ctx*, const float* saliency, const float* mask,
                                   int64_t nvox, int round, uint32_t prefix,
                                   uint64_t* hist_host /* 2048 */, uint64_t* n_unmasked_host);
/* the same histogram written to DEVICE memory (2048 counters), asynchronous on the context's stream: multi-GPU callers
 * all-reduce it there (RCCL) and fetch the sum once per round */
int visfd_hip_select_histogram_todev(visfd_hip_ctx*, const float* saliency, const float* mask, int64_t nvox, int round,
                                     uint32_t prefix, uint64_t* hist_dev /* 2048, device */);
int visfd_hip_apply_threshold_dev(visfd_hip_ctx*, float* saliency, int64_t nvox, float threshold);

/* ---- a13+a14: TV3D::TVDenseStick, lib/visfd/feature.hpp:1645-1675,1711-2037,2217-2384 ------------ */
/* As instantiated by HandleTV (handlers.cpp:1821-1836): normalize=false, diagonalize=false.
 * tensor (6 channels) is zeroed where mask_dst!=0 (or everywhere if NULL) and left untouched
 * elsewhere.  detect_curves selects the curve vote field (feature.hpp:2317-2347). */
int visfd_hip_tv_dense_stick(visfd_hip_ctx*, const float* saliency, const float* direction,
                             float* tensor, const float* mask_src, const float* mask_dst,
                             int64_t nx, int64_t ny, int64_t nz, float sigma_tv, int exponent,
                             float cutoff_ratio, int detect_curves);
int visfd_hip_tv_dense_stick_dev(visfd_hip_ctx*, const float* saliency, const float* direction,
                                 float* tensor, const float* mask_src, const float* mask_dst,
                                 int64_t nx, int64_t ny, int64_t nz, float sigma_tv, int exponent,
                                 float cutoff_ratio, int detect_curves);
/* Z-slab form for multi-GPU runs: the arrays cover planes [z_lo, z_lo+nz_local) of a volume whose
 * true height is nz_global; receivers are computed for planes [z_out0, z_out1) (global indices) and
 * senders outside the supplied planes are treated as absent (so the caller must supply
 * halfwidth ghost planes on interior faces). */
int visfd_hip_tv_dense_stick_slab_dev(visfd_hip_ctx*, const float* saliency, const float* direction,
                                      float* tensor, const float* mask_src, const float* mask_dst,
                                      int64_t nx, int64_t ny, int64_t nz_local, int64_t z_out0,
                                      int64_t z_out1, float sigma_tv, int exponent,
                                      float cutoff_ratio, int detect_curves);
/* The denominators of TVDenseStick(normalize=true) with a source mask (feature.hpp:1761-1822, 2376-2382):
 * den[voxel] = sum of w(j) * mask_src(sender) over the votes the voxel receives, added in vote order; voxels with
 * mask_dst == 0 keep the caller's value.  Host pointers.  include/visfd_hip.hpp divides the tensors by it exactly as
 * the reference does. */
int visfd_hip_tv_weight_sum(visfd_hip_ctx*, const float* saliency, float* den, const float* mask_src, const float* mask_dst,
                            int64_t nx, int64_t ny, int64_t nz, float sigma_tv, float cutoff_ratio);
/* halfwidth of the vote window, floor(sigma_tv*cutoff) (feature.hpp:1671); tables (nullable):
 * w[(2h+1)^3], rhat[(2h+1)^3][3] as built by filter3d.hpp:546-601 and feature.hpp:2468-2482. */
int visfd_hip_tv_tables(float sigma_tv, float cutoff_ratio, int* halfwidth_out, float* w,
                        float* rhat);

/* ---- a15: post-voting score, bin/filter_mrc/handlers.cpp:1870-1892 ------------------------------ */
/* saliency[v] = lambda0 - lambda1 of the diagonalised vote tensor where mask != 0; untouched elsewhere */
int visfd_hip_tensor_saliency(visfd_hip_ctx*, const float* tensor, const float* mask, int64_t nvox,
                              int eival_order, float* saliency_inout);
int visfd_hip_tensor_saliency_dev(visfd_hip_ctx*, const float* tensor, const float* mask,
                                  int64_t nvox, int eival_order, float* saliency_inout);
/* with the peak-height factor (handlers.cpp:1883-1887): score *= image - background (both NULL: no factor) */
int visfd_hip_tensor_saliency_bg_dev(visfd_hip_ctx*, const float* tensor, const float* mask, int64_t nvox, int eival_order,
                                     const float* image, const float* background, float* saliency_inout);

/* ---- a9+a10+a11+a12+a14+a15 in one call: the compute section of HandleTV ------------------------- */
/* bin/filter_mrc/handlers.cpp:1618-1892 for SURFACE_RIDGE (the _bg forms add the optional peak-height factor of
 * handlers.cpp:1577-1605,1698-1702,1883-1887: sigma_background > 0 multiplies both scores by image - background):
 * CalcHessian (feature.hpp:1203) -> per-voxel eigen/score/direction loop (handlers.cpp:1645-1746) ->
 * saliency threshold (handlers.cpp:1751-1797: top `best_fraction` of unmasked voxels when
 * best_fraction >= 0, else the absolute value `threshold_abs`) -> TV3D::TVDenseStick when sigma_tv > 0
 * (handlers.cpp:1821-1836, normalize=false) -> post-voting score (handlers.cpp:1870-1892).
 * saliency_out: 1 channel (zero where mask == 0 before voting; voxels with mask == 0 keep that zero).
 * tensor_out (nullable): 6 channels, interleaved on the host face / planar on the device face; this is
 * what `-save-progress` writes as <base>_tensor_{0..5}.rec (handlers.cpp:1897-1922).
 * direction_out (nullable): principal direction, 3 channels. threshold_out (nullable). */
int visfd_hip_membrane_detect(visfd_hip_ctx*, const float* src, const float* mask,
                              int64_t nx, int64_t ny, int64_t nz, float sigma, float truncate_ratio,
                              int eival_order, float best_fraction, float threshold_abs, float sigma_tv,
                              int tv_exponent, float tv_cutoff_ratio, float* saliency_out,
                              float* tensor_out, float* direction_out, float* threshold_out);
int visfd_hip_membrane_detect_dev(visfd_hip_ctx*, const float* src, const float* mask,
                                  int64_t nx, int64_t ny, int64_t nz, float sigma, float truncate_ratio,
                                  int eival_order, float best_fraction, float threshold_abs,
                                  float sigma_tv, int tv_exponent, float tv_cutoff_ratio,
                                  float* saliency_out, float* tensor_out, float* direction_out,
                                  float* threshold_out);
int visfd_hip_membrane_detect_bg(visfd_hip_ctx*, const float* src, const float* mask,
                                 int64_t nx, int64_t ny, int64_t nz, float sigma, float truncate_ratio,
                                 int eival_order, float best_fraction, float threshold_abs, float sigma_tv,
                                 int tv_exponent, float tv_cutoff_ratio, float sigma_background, int normalize_background,
                                 float* saliency_out, float* tensor_out, float* direction_out, float* threshold_out);
int visfd_hip_membrane_detect_bg_dev(visfd_hip_ctx*, const float* src, const float* mask,
                                     int64_t nx, int64_t ny, int64_t nz, float sigma, float truncate_ratio,
                                     int eival_order, float best_fraction, float threshold_abs,
                                     float sigma_tv, int tv_exponent, float tv_cutoff_ratio, float sigma_background,
                                     int normalize_background, float* saliency_out, float* tensor_out, float* direction_out,
                                     float* threshold_out);
/* The same stage (fraction cut, sigma_tv > 0) with every volume the caller's, all device memory: `scratch` receives the
 * smoothed image, `background` (NULL unless sigma_background > 0) the background of the peak-height factor, saliency,
 * direction (3 planes) and tensor (6 planes) the results.  Voxels of `direction_out` whose score did not survive the cut
 * keep what they held. */
int visfd_hip_membrane_stage_dev(visfd_hip_ctx*, const float* src, const float* mask, int64_t nx, int64_t ny, int64_t nz,
                                 float sigma, float truncate_ratio, int eival_order, float best_fraction, float sigma_tv,
                                 int tv_exponent, float tv_cutoff_ratio, float sigma_background, int normalize_background,
                                 float* background, float* scratch, float* saliency_out, float* direction_out,
                                 float* tensor_out, float* threshold_out);
/* Test aids: the two consumers of a saliency volume that has NOT been cut.  thr_dev: one float in device memory (a voxel
 * counts if !(s < *thr_dev) && s != 0), or NULL for a volume that has been cut.  The lists of the whole volume for vote
 * windows of half-width h (mode 0, 2: saliencies times 1/4, 1/2; 1: as they are; fold: the folded records) come back in
 * HOST arrays: rows (nz (ny + 1) ceil(nx / 16) words: list (z, tx) is [rows[(z (ny + 1) + ny) ntx + tx], rows[z (ny + 1) ntx + tx])),
 * entries (4 floats each) and positions.  *nrows and *total are set in any case; an array that is too small stays as it was. */
int visfd_hip_debug_ridge_directions_thr_dev(visfd_hip_ctx*, const float* smoothed, int64_t nx, int64_t ny, int64_t nz,
                                             float sigma, int eival_order, const float* saliency, const float* thr_dev,
                                             float* direction_out);
int visfd_hip_debug_tv_lists_dev(visfd_hip_ctx*, const float* saliency, const float* direction, const float* thr_dev, int64_t nx,
                                 int64_t ny, int64_t nz, int h, int mode, int fold, uint32_t* rows, int64_t rows_cap, float* entries,
                                 uint32_t* positions, int64_t entries_cap, int64_t* nrows, int64_t* total, uint32_t* flags);

/* ---- Z-slab helpers for the separable filter (multi-GPU) -------------------------- */
/* Same as apply_gauss_dev on a slab: arrays hold planes [z_lo, z_lo+nz_local) of a volume of height
 * nz_global; planes outside the slab are treated as outside the image ONLY at the true faces
 * (z_lo==0 / z_lo+nz_local==nz_global); the unmasked normaliser uses global coordinates
 * (filter3d.hpp:1004-1021).  Output planes within halfwidth[2] of an interior slab face are
 * invalid and must be discarded by the caller (they are ghost planes). */
int visfd_hip_apply_gauss_slab_dev(visfd_hip_ctx*, const float* src, float* dst,
                                   int64_t nx, int64_t ny, int64_t nz_local, int64_t z_lo,
                                   int64_t nz_global, const float sigma[3], const int halfwidth[3],
                                   int normalize, float* A_out);

/* ---- e: Z-slab runs across the GPUs of one node ------------------------------------------------------
 * The reference is single-process (OpenMP only): there is no reference interface to cite here.  These entry points are
 * what a host started once per GPU calls so that a volume larger than one GPU's HBM -- or simply more throughput -- runs on
 * the GPUs of a node: planes [z0, z1) of the volume per rank plus `ghost` planes on each INTERIOR face, halos exchanged
 * point-to-point with the two Z-neighbours only (RCCL send/recv over one xGMI link each, on a transfer stream of the
 * slab's own, overlapping the votes of the interior planes), three all-reduces of 2048 counters for the exact global
 * top-fraction threshold.  Outputs of owned planes are bit-identical to the single-volume run (exact kernels).
 * Volumes are DEVICE pointers of the local shape [nz_local][ny][nx]; everything is queued on the context's stream. */
typedef struct visfd_hip_slab visfd_hip_slab;
/* A transport other than RCCL (tests; MPI hosts).  Pointers are DEVICE pointers; work must be ordered on `stream`
 * (a hipStream_t) or complete on return.  Every callback returns 0 on success. */
typedef struct visfd_hip_transport {
  /* send `bytes` from sendbuf to rank `peer` and receive as many from it into recvbuf (a paired exchange); `peer` is a
   * Z-neighbour, or the rank itself when visfd_hip_slab_selftest calls */
  int (*sendrecv)(void* user, int peer, const void* sendbuf, void* recvbuf, size_t bytes, void* stream);
  /* sum `count` uint64 counters over all ranks, in place */
  int (*allreduce_sum_u64)(void* user, uint64_t* buf, size_t count, void* stream);
  int (*group_start)(void* user);   /* optional (may be NULL): brackets the sendrecv calls of one halo exchange */
  int (*group_end)(void* user);
  void* user;
} visfd_hip_transport;
/* RCCL: rank 0 obtains a 128-byte id (ncclGetUniqueId), the host hands it to every rank by its own means (a file, MPI,
 * torch.distributed ...), every rank creates its slab with it (ncclCommInitRank).  librccl.so is loaded at run time. */
int visfd_hip_slab_unique_id(void* id_out_128_bytes);
/* 1 if librccl.so can be loaded in this process (no error is set otherwise): lets every rank agree BEFORE any of them
 * enters ncclCommInitRank, which would block for ever if one rank could not follow */
int visfd_hip_slab_rccl_available(void);
int visfd_hip_slab_create_rccl(visfd_hip_ctx*, const void* unique_id_128_bytes /* may be NULL when world == 1 */, int rank,
                               int world, int64_t nz_global, int ghost, visfd_hip_slab** out);
int visfd_hip_slab_create_custom(visfd_hip_ctx*, const visfd_hip_transport*, int rank, int world, int64_t nz_global,
                                 int ghost, visfd_hip_slab** out);
/* Both refuse (VISFD_HIP_EINVAL) when world > 1 and the THINNEST slab, nz_global / world planes, is thinner than `ghost`:
 * the answer is the same on every rank, so no rank goes on into a collective that the others never join. */
int visfd_hip_slab_destroy(visfd_hip_slab*);
/* out = {z0, z1, lo, hi, own0, own1, nz_local}: owned planes [z0, z1) and stored planes [lo, hi) of the volume; the owned
 * planes are [own0, own1) of the local array */
int visfd_hip_slab_layout(visfd_hip_slab*, int64_t out[7]);
/* The transport's smoke test: a grouped send/receive of `count` floats from this rank to itself on the transfer stream and
 * an all-reduce of 2048 counters, both verified.  A slab created with world == 1 AND an id owns a one-rank RCCL communicator:
 * that is what a one-GPU box can run of the RCCL path (run-time loading, call signatures, stream ordering). */
int visfd_hip_slab_selftest(visfd_hip_slab*, int64_t count);
/* workgroup slots the voting grid leaves free for the transport's kernels while a halo is in flight (default 64) */
int visfd_hip_slab_set_reserve(visfd_hip_slab*, int reserve_workgroups);
/* fill the ghost planes of `nvol` volumes within `depth` planes of the owned range (one group of sends/receives) */
int visfd_hip_slab_exchange_dev(visfd_hip_slab*, float* const* volumes, int nvol, int64_t nx, int64_t ny, int depth);
/* HandleTV (bin/filter_mrc/handlers.cpp:1501-1892) on one slab: ridge scores, GLOBAL top-fraction threshold, directions,
 * halo of (saliency, direction), votes (interior planes beside the transfer), post-vote score.  dirs: 3 planar channels,
 * tensor: 6, scratch: one volume.  Valid results: the owned planes of sal and tensor.  src_halo_ready != 0: the caller has
 * already exchanged src's ghost planes at least floor(sigma * ratio) + 1 deep in this step. */
int visfd_hip_membrane_detect_slab_dev(visfd_hip_slab*, float* src, float* sal, float* dirs, float* tensor, float* scratch,
                                       int64_t nx, int64_t ny, float sigma, float truncate_ratio, int eival_order,
                                       float best_fraction, float sigma_tv, int exponent, float tv_truncate_ratio,
                                       int src_halo_ready, float* threshold_out);
/* The same for a host whose volume lives in HOST memory (filter_mrc started once per GPU, `-slab`): src_owned / sal_owned
 * are the rank's OWNED planes [z0, z1) only ([z1-z0][ny][nx]); tensor_owned (may be NULL) receives six interleaved floats per
 * owned voxel, as visfd_hip_membrane_detect returns them.  Device arrays (12 slab volumes) live for the call only. */
int visfd_hip_membrane_detect_slab(visfd_hip_slab*, const float* src_owned, int64_t nx, int64_t ny, float sigma,
                                   float truncate_ratio, int eival_order, float best_fraction, float sigma_tv, int exponent,
                                   float tv_truncate_ratio, float* sal_owned, float* tensor_owned, float* threshold_out);
/* The slab forms with the peak-height factor (sigma_background > 0; `background`: one more slab volume on the device face).
 * The ghost depth must cover floor(sigma_background * truncate_ratio) as well. */
int visfd_hip_membrane_detect_slab_bg_dev(visfd_hip_slab*, float* src, float* sal, float* dirs, float* tensor, float* scratch,
                                          float* background, int64_t nx, int64_t ny, float sigma, float truncate_ratio,
                                          int eival_order, float best_fraction, float sigma_tv, int exponent,
                                          float tv_truncate_ratio, float sigma_background, int normalize_background,
                                          int src_halo_ready, float* threshold_out);
int visfd_hip_membrane_detect_slab_bg(visfd_hip_slab*, const float* src_owned, int64_t nx, int64_t ny, float sigma,
                                      float truncate_ratio, int eival_order, float best_fraction, float sigma_tv, int exponent,
                                      float tv_truncate_ratio, float sigma_background, int normalize_background,
                                      float* sal_owned, float* tensor_owned, float* threshold_out);
/* BlobDog (lib/visfd/feature.hpp:53-427) on one slab with absolute thresholds: blobs of the OWNED planes only, iz as
 * GLOBAL plane index.  The host merges the ranks' lists (and applies ratio thresholds, which need the global best). */
int visfd_hip_blob_dog_slab_dev(visfd_hip_slab*, float* src, int64_t nx, int64_t ny, const float* blob_sigma, int n_sigma,
                                float delta_sigma_over_sigma, float truncate_ratio, float minima_threshold,
                                float maxima_threshold, int src_halo_ready,
                                visfd_hip_blob* minima, int64_t minima_capacity, int64_t* n_minima,
                                visfd_hip_blob* maxima, int64_t maxima_capacity, int64_t* n_maxima);
/* The halo depth the slab blob stage exchanges (and the least ghost depth it accepts): the Z half-width of the widest LoG
 * in the kernels' own float arithmetic (sigma_b = (float)(sigma * (1 + delta/2)), floor(truncate_ratio * sigma_b) as a float
 * product; lib/visfd/filter3d.hpp:1451-1464) plus the one plane the 26-neighbour scan reads beyond it. */
int visfd_hip_blob_halo_depth(const float* blob_sigma, int n_sigma, float delta_sigma_over_sigma, float truncate_ratio,
                              int* depth_out);
/* Host-memory faces for a host that runs one process per GPU (`filter_mrc -gauss|-blob ... -slab`): the rank's OWNED planes
 * [z1-z0][ny][nx] in, the owned planes of the filtered volume / the blobs of the owned planes (iz GLOBAL) out.  A blob list that
 * does not fit returns VISFD_HIP_ECAPACITY with the needed counts in n_minima / n_maxima; the retry is local. */
int visfd_hip_apply_gauss_slab(visfd_hip_slab*, const float* src_owned, int64_t nx, int64_t ny, const float sigma[3],
                               const int halfwidth[3], int normalize, float* dst_owned, float* A_out);
int visfd_hip_blob_dog_slab(visfd_hip_slab*, const float* src_owned, int64_t nx, int64_t ny, const float* blob_sigma, int n_sigma,
                            float delta_sigma_over_sigma, float truncate_ratio, float minima_threshold, float maxima_threshold,
                            visfd_hip_blob* minima, int64_t minima_capacity, int64_t* n_minima,
                            visfd_hip_blob* maxima, int64_t maxima_capacity, int64_t* n_maxima);

/* ---- voxelising a closed triangle mesh (bin/voxelize_mesh/voxelize_mesh.py) -----------------------------
 * The reference asks vtk which grid samples lie inside the surface; here the answer is defined exactly, in integers.
 *
 * Quantisation (host, IEEE double, in this order): t = (double)v[d] / voxel_width; t = t - origin[d]; t = t * 1024.0;
 * q = nearbyint(t) (ties to even) as int32: 1/1024 voxel units.  origin: the position of voxel 0, in voxels.
 * VISFD_HIP_EINVAL for a non-finite vertex, |q| > 2^29, voxel_width zero or not finite.
 *
 * Inside rule.  Rays run along x; sample (ix, iy, iz) is the point 1024 * (ix, iy, iz); u = y, v = z.  For a triangle with
 * quantised vertices A, B, C: area2 = (Bu-Au)(Cv-Av) - (Bv-Av)(Cu-Au); triangles with area2 == 0 are skipped; s =
 * sign(area2).  For a directed edge a->b and the sample's (pu, pv): E = (bu-au)(pv-av) - (bv-av)(pu-au); sigma = sign(E) if
 * E != 0, else -sign(bv-av) if that is not 0, else sign(bu-au) (the sample moved by (+eps, +eps^2)).  The triangle covers row
 * (iy, iz) iff sigma of AB, BC and CA all equal s.  Its crossing is the rational x_c = Ax - (Ny (pu-Ay) + Nz (pv-Az)) / Nx
 * with N = (B-A) x (C-A); k = floor(x_c / 1024) + 1 clamped to [0, nx].  inside(ix, iy, iz) is the parity of the
 * crossings of row (iy, iz) with k <= ix.  dst: float32 [nz][ny][nx], 1.0 inside and 0.0 outside.
 *
 * vertices: float[n_vertices][3] (x, y, z) and triangles: int32[n_triangles][3] are HOST arrays on both faces; dst is a
 * host pointer in the first form and a device pointer in the _dev form.  Both return with the stream idle.
 * check_closed != 0: a mesh with boundary or non-manifold edges (visfd_hip_mesh_edges_host) is VISFD_HIP_EINVAL and the
 * message names the counts.  Also VISFD_HIP_EINVAL: a triangle index out of range, images of 2^31 voxels or more,
 * nx >= 2^19. */
int visfd_hip_voxelize_mesh(visfd_hip_ctx*, const float* vertices, int64_t n_vertices, const int32_t* triangles,
                            int64_t n_triangles, double voxel_width, const double origin[3], int64_t nx, int64_t ny,
                            int64_t nz, int check_closed, float* dst);
int visfd_hip_voxelize_mesh_dev(visfd_hip_ctx*, const float* vertices, int64_t n_vertices, const int32_t* triangles,
                                int64_t n_triangles, double voxel_width, const double origin[3], int64_t nx, int64_t ny,
                                int64_t nz, int check_closed, float* dst);
/* The last voxelisation of the context: crossings (covered (triangle, row) pairs of rows inside the image), skipped
 * triangles (area2 == 0), odd_rows (rows whose total crossing parity is odd: 0 for every closed mesh), inside voxels;
 * -1 each before the first call. */
int visfd_hip_voxelize_last(visfd_hip_ctx*, int64_t stats[4]);
/* option voxelize_time: milliseconds the last voxelisation spent zeroing its toggle words, in the scatter over the
 * triangles, and in the fill of the image */
int visfd_hip_voxelize_last_times(visfd_hip_ctx*, float ms[3]);
/* the quantisation above: q receives int32[n_vertices][3] */
int visfd_hip_voxelize_quantize_host(const float* vertices, int64_t n_vertices, double voxel_width, const double origin[3],
                                     int32_t* q);
/* The census of undirected edges: those used by exactly one triangle (boundary) and by more than two (non-manifold).
 * VISFD_HIP_EINVAL for an index outside [0, n_vertices). */
int visfd_hip_mesh_edges_host(const int32_t* triangles, int64_t n_triangles, int64_t n_vertices, int64_t* boundary_edges,
                              int64_t* nonmanifold_edges);

/* ---- closing an oriented point cloud into a mask ----------------------------------------------------------
 * No counterpart in the reference: its Example 3 writes the cloud with -normals-file, closes it with an external surface
 * reconstruction program, and voxelises the mesh for the next run's -mask.  Here the mask is computed on the voxel grid, as
 * the grid form of Poisson surface reconstruction.  The result is defined as follows.
 *
 * Inputs.  n points p_i (float[n][3], x y z, in voxel coordinates: voxel (ix, iy, iz) is the node at that coordinate), their
 * normals n_i (float[n][3]), the image size nx, ny, nz >= 3, pad >= 0 (the equation is solved on the box that is the image
 * grown by pad nodes on every face: Nd = nd + 2 pad nodes per axis, each at most 65535), and the orientation
 * (VISFD_HIP_CLOSE_OUTWARD: the normals point out of the solid, _INWARD, or _AUTO).
 *
 * 1. Splat (exact, independent of order).  A point is USED when its six floats are finite, no |n_d| exceeds 2^30 (so that
 *    no contribution leaves int64), and its cell floor(p) .. floor(p) + 1 lies inside the box; the others are counted as
 *    skipped.  In double: f_d = (double)p_d - floor((double)p_d); a corner's weight is (wx * wy) * wz with w = f or 1 - f;
 *    its contribution to channel d is llrint((weight * (double)n_d) * 2^24), ties to even.  Contributions are added as
 *    64-bit integers into three int64 volumes acc[d][Nz][Ny][Nx].  V_d = (float)((double)acc_d * 2^-24).
 * 2. Right-hand side, in float: b = ((0.5 (Vx[x+1] - Vx[x-1]) + 0.5 (Vy[y+1] - Vy[y-1])) + 0.5 (Vz[z+1] - Vz[z-1])), V = 0
 *    outside the box.
 * 3. chi solves Laplace(chi) = b with the 7-point Laplacian at unit spacing, chi = 0 outside the box: float32 multigrid
 *    V-cycles on the device, stopped when |b - Laplace(chi)|_2 <= rtol |b|_2 (rtol = 10^-close_surface_rtol_exp), the norm
 *    being that of the iterate the call returns, or after close_surface_max_cycles cycles.  Every reduction has a fixed
 *    order: a call gives the same bits on every run.  The float64 solve of tests/close_surface_np.py is the yardstick.
 * 4. Level: iso = (the sum over the used points, in double and in a fixed order, of chi interpolated trilinearly at p_i with
 *    the weights of step 1) / n_used.
 * 5. Mask over the image (the pad is dropped), float32 [nz][ny][nx] of 0 and 1 like visfd_hip_voxelize_mesh's:
 *    outward: 1 where (double)chi < iso; inward: 1 where (double)chi > iso; auto: whichever of the two sets holds fewer
 *    nodes on the six faces of the padded box, outward on a tie.
 * chi_out (nullable): float32 [nz][ny][nx], chi over the image.
 *
 * A call in which no point is used (n == 0 included) succeeds with a mask of zeros.  VISFD_HIP_EINVAL, before anything is
 * allocated: a null context or mask, a dimension below 3, a negative pad or n, n > 0 with a null array, an unknown
 * orientation, a padded dimension above 65535.  points, normals, mask and chi_out are host arrays in the first form and
 * device arrays in the _dev form, where an output that overlaps a list or the other output is VISFD_HIP_EINVAL too.  Both return with the stream idle. */
#define VISFD_HIP_CLOSE_OUTWARD 0
#define VISFD_HIP_CLOSE_INWARD 1
#define VISFD_HIP_CLOSE_AUTO 2
#define VISFD_HIP_CLOSE_STOP_RTOL 0   /* the residual test was met */
#define VISFD_HIP_CLOSE_STOP_CAP 1    /* close_surface_max_cycles cycles were run first */
#define VISFD_HIP_CLOSE_STOP_NONE 2   /* nothing to solve: no used point, or a right-hand side of zeros */
int visfd_hip_close_surface(visfd_hip_ctx*, const float* points, const float* normals, int64_t n, int64_t nx, int64_t ny,
                            int64_t nz, int64_t pad, int orientation, float* mask, float* chi_out);
int visfd_hip_close_surface_dev(visfd_hip_ctx*, const float* points, const float* normals, int64_t n, int64_t nx, int64_t ny,
                                int64_t nz, int64_t pad, int orientation, float* mask, float* chi_out);
/* Step 1 alone: acc receives int64[3][Nz][Ny][Nx] (a host array, in the _dev form a device array like the lists), counts
 * (nullable, host) the used and the skipped points.  Refusals as above (acc in the place of mask). */
int visfd_hip_close_surface_splat(visfd_hip_ctx*, const float* points, const float* normals, int64_t n, int64_t nx, int64_t ny,
                                  int64_t nz, int64_t pad, int64_t* acc, int64_t counts[2]);
int visfd_hip_close_surface_splat_dev(visfd_hip_ctx*, const float* points, const float* normals, int64_t n, int64_t nx,
                                      int64_t ny, int64_t nz, int64_t pad, int64_t* acc, int64_t counts[2]);
/* The same integers by a serial walk on the host: no context, no device. */
int visfd_hip_close_surface_splat_host(const float* points, const float* normals, int64_t n, int64_t nx, int64_t ny, int64_t nz,
                                       int64_t pad, int64_t* acc, int64_t counts[2]);
/* The last visfd_hip_close_surface[_dev] of the context.  stats: used points, skipped points, cycles run, the stop
 * (VISFD_HIP_CLOSE_STOP_*), the orientation taken (VISFD_HIP_CLOSE_OUTWARD or _INWARD), 1 when the mask holds a voxel on a
 * face of the image (a surface cut by the border: pad), else 0; -1 each before the first call.
 * values: the final |b - Laplace(chi)| / |b|, and iso. */
int visfd_hip_close_surface_last(visfd_hip_ctx*, int64_t stats[6], double values[2]);
/* option close_surface_time: milliseconds of the last call's splat with the right-hand side, its solve, and its level
 * and cut */
int visfd_hip_close_surface_last_times(visfd_hip_ctx*, float ms[3]);

/* ---- the closed triangle mesh of a level set -------------------------------------------------------------
 * No counterpart in the reference, whose Example 3 takes its mesh from an external reconstruction program.  The mesh is
 * defined to the bit, by marching tetrahedra on the Kuhn split of every grid cell.
 *
 * Inputs.  vol: float32 [nz][ny][nx], every dimension >= 1; iso: a double; side: VISFD_HIP_ISO_BELOW (a node is inside iff
 * (double)v < iso) or VISFD_HIP_ISO_ABOVE (inside iff (double)v > iso).  A NaN node is never inside.
 *
 * Grid.  The image nodes are surrounded by one layer of border nodes (coordinates -1 and n_d), which are always outside:
 * that caps every solid the image border cuts.  Cells have lower corners from -1 to n_d - 1 on each axis.  A cell is split
 * into the 6 tetrahedra 0, e_a, e_a + e_b, e_a + e_b + e_c for the permutations (a, b, c) of the axes in lexicographic
 * order xyz, xzy, yxz, yzx, zxy, zyx: that order is the tet index 0..5 and the corner order within a tet.  Every tet edge
 * runs from a node to the node at + dir; the 7 directions, in this order the edge class 0..6, are (1,0,0) (0,1,0) (0,0,1)
 * (1,1,0) (0,1,1) (1,0,1) (1,1,1).
 *
 * Vertices.  One per edge whose two ends differ in insideness.  a: the lower end, b = a + dir.  With both ends image nodes,
 * in double: t = (iso - (double)v_a) / ((double)v_b - (double)v_a); a non-finite t becomes 0.5; t is clamped to
 * [1/64, 63/64].  With a border node at one end t = 0.5.  Coordinate d is (float)((double)a_d + t) where dir_d = 1 and
 * (float)a_d elsewhere; no fused multiply-add changes these.  The clamp keeps a vertex quantised to 1/1024 voxel (the
 * voxeliser above) off the nodes.  Vertices are in voxel coordinates, listed in ascending order of key(a) * 7 + class,
 * key(a) = ((a_z + 1)(ny + 1) + (a_y + 1))(nx + 1) + (a_x + 1).
 *
 * Triangles.  Per tet, I and O: its inside and outside corners in tet corner order; e(i, o): the vertex on that edge.
 * |I| = 1: the polygon [e(I0, o) for o in O]; |I| = 3: [e(i, O0) for i in I]; |I| = 2: [e(I0,O0), e(I0,O1), e(I1,O1),
 * e(I1,O0)].  With the vertices at the edge midpoints, if (P1 - P0) x (P2 - P0) points from the mean of the outside corners
 * towards the mean of the inside corners, the whole list is reversed: normals point out of the solid.  (P0, P1, P2) is
 * emitted, and for a quad (P0, P2, P3) too.  Triangles are listed in order of (cell key, tet index, first / second);
 * indices are int32.  The mesh is closed and edge-manifold by construction.
 *
 * Outputs: vertices float[vertices_cap][3] (x, y, z), triangles int32[triangles_cap][3]; *n_vertices and *n_triangles are
 * always set.  A null array is not written (both null: the count query).  An array whose capacity is below its count is left
 * exactly as it was and the call returns VISFD_HIP_ECAPACITY; the other array is still written.
 * VISFD_HIP_EINVAL, nothing written: a null context, volume or count pointer, a dimension < 1 (or >= 2^31 - 2), an unknown
 * side, a non-finite iso, a negative capacity, more than 2^31 - 1 vertices; on the device face outputs that overlap the
 * volume or each other.  vol and the arrays are host memory in the first form, device memory in the _dev form; both return
 * with the stream idle.  Two calls write the same bytes. */
#define VISFD_HIP_ISO_BELOW 0
#define VISFD_HIP_ISO_ABOVE 1
int visfd_hip_isosurface(visfd_hip_ctx*, const float* vol, int64_t nx, int64_t ny, int64_t nz, double iso, int side,
                         float* vertices, int64_t vertices_cap, int32_t* triangles, int64_t triangles_cap, int64_t* n_vertices,
                         int64_t* n_triangles);
int visfd_hip_isosurface_dev(visfd_hip_ctx*, const float* vol, int64_t nx, int64_t ny, int64_t nz, double iso, int side,
                             float* vertices, int64_t vertices_cap, int32_t* triangles, int64_t triangles_cap,
                             int64_t* n_vertices, int64_t* n_triangles);
/* The same mesh by a serial walk on the host: no context, no device. */
int visfd_hip_isosurface_host(const float* vol, int64_t nx, int64_t ny, int64_t nz, double iso, int side, float* vertices,
                              int64_t vertices_cap, int32_t* triangles, int64_t triangles_cap, int64_t* n_vertices,
                              int64_t* n_triangles);
/* The last visfd_hip_isosurface[_dev] of the context: vertices, triangles, inside nodes, 1 if an inside node lies on a face
 * of the image (the border layer capped the solid there) else 0; -1 each before the first call. */
int visfd_hip_isosurface_last(visfd_hip_ctx*, int64_t stats[4]);
/* option isosurface_time: milliseconds of the last call's classification, its scan with the host's read of the totals, its
 * vertex pass and its triangle pass (-1: the phase did not run) */
int visfd_hip_isosurface_last_times(visfd_hip_ctx*, float ms[4]);

#ifdef __cplusplus
}
#endif
#endif /* VISFD_HIP_H */
