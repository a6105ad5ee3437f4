// common.hpp -- context, workspace and error plumbing shared by the HIP translation units.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/visfd_hip.h"

namespace vh {

typedef int64_t i64;

// ---- error reporting -------------------------------------------------------------------------
void set_error(const std::string& msg);
int fail(int code, const std::string& msg);

#define VH_HIP(expr)                                                                         \
  do {                                                                                       \
    hipError_t _e = (expr);                                                                  \
    if (_e != hipSuccess)                                                                    \
      return vh::fail(_e == hipErrorOutOfMemory ? VISFD_HIP_ENOMEM : VISFD_HIP_EDEVICE,      \
                      std::string(#expr) + ": " + hipGetErrorString(_e));                    \
  } while (0)

#define VH_TRY(expr)           \
  do {                         \
    int _rc = (expr);          \
    if (_rc != VISFD_HIP_OK) return _rc; \
  } while (0)

#define VH_REQUIRE(cond, msg) \
  do {                        \
    if (!(cond)) return vh::fail(VISFD_HIP_EINVAL, msg); \
  } while (0)

// ---- workspace: named slots that only grow; freed by visfd_hip_trim/destroy -------------------
enum Slot {
  WS_A = 0, WS_B, WS_C, WS_D,      // full-volume float scratch
  WS_DEN_A, WS_DEN_B,              // masked-normalisation denominators
  WS_NORM,                         // Dx|Dy|Dz normaliser lines
  WS_LOG0, WS_LOG1, WS_LOG2,       // rolling LoG volumes of the blob detector
  WS_CAND, WS_COUNTER,             // candidate list + counters
  WS_SCANCNT,                      // counters of the pipelined blob scan: theirs alone (a scan's counts are read by the host after later stages
                                   // may have been queued, visfd_hip_blob_dog_begin_dev / _end)
  WS_HIST,                         // radix-select histograms
  WS_TVTAB,                        // tensor-voting lookup table
  WS_TVAUX,                        // tensor-voting auxiliaries
  WS_TVSCRATCH,                    // tensor voting: per-workgroup rings of compacted sender planes (exact kernel) / the launch's sender lists
  WS_TVLIST,                       // tolerance-mode tensor voting: row offsets of the sender lists
  WS_H2D_0, WS_H2D_1, WS_H2D_2, WS_H2D_3, WS_H2D_4,  // staging for the host-pointer face
  WS_MORPH_TAB,                    // morphology: the structuring element on the device (its slot key: the same ints)
  WS_MORPH_SRC,                    // morphology: the source with masked voxels replaced by NaN
  WS_MORPH_TMP,                    // morphology: the intermediate image of open / close / the top-hats
  WS_EXT_FLAGS,                    // extrema: one byte of neighbour facts per voxel (csrc/extrema.hip)
  WS_EXT_PARENT,                   // extrema: the union-find word of every voxel (int32)
  WS_EXT_COUNT,                    // extrema: voxels per plateau, at the plateau's root (int32 per voxel)
  WS_EXT_COUNTERS,                 // extrema: the two list lengths
  WS_EXT_LIST,                     // extrema: the unsorted lists (index, score, voxels)
  WS_EXT_RANKS,                    // extrema: listed roots in raster order and their sorted positions, for the label image
  WS_F3D_TAB,                      // general 3-D filter: the table's non-zero entries on the device (its slot key: window, nx, ny and the raw table)
  WS_DRAW_OWNER,                   // DrawSpheres: the owner volume, one uint32 per voxel: the last sphere that holds it, plus one (csrc/draw.hip)
  WS_DRAW_TAB,                     // DrawSpheres: per-sphere values, counts, clipped boxes and running row counts; DrawRegions: its one flag
  WS_WSH_KIND,                     // watershed: one byte per voxel: ineligible / interior / chain / join, and what the merge pass adds (csrc/watershed.hip)
  WS_WSH_LINK,                     // watershed: union-find parent or down pointer (int32), then the voxel's node; reused for the qualifying-neighbour bits
  WS_WSH_C,                        // watershed: the carried basin (int32 per voxel)
  WS_WSH_STATE,                    // watershed: boundary state, one byte per voxel
  WS_WSH_SEEDS,                    // watershed: the seeds' root indices in list order
  WS_WSH_FLAGS,                    // watershed: the NaN flag and the per-round change flag
  WS_MEDIAN_TAB,                   // median filter: the footprint on the device (its slot key: the same ints); csrc/median.hip
  WS_INTENSITY,                    // image statistics: the integer bins of one pass (csrc/intensity.hip), zeroed by every call that uses them
  WS_DIST_DSQ,                     // distance maps: the int32 squared distances behind the float outputs (csrc/distance.hip)
  WS_DIST_STACK,                   // distance maps: the envelope passes' stacks, per wave [entry][lane] of int2
  WS_DIST_POINTS,                  // distance maps: the listed points that can matter; query points and their results
  WS_FS_RECORDS,                   // FindSpheres: one 16-byte record (cx, cy, cz, Rsqr) per sphere, padded to whole passes (csrc/find_spheres.hip)
  WS_FS_QUERIES,                   // FindSpheres: the truncated queries, padded to whole batches, and the flag word of the two preparation launches
  WS_CG_WORD,                      // LabelConnected as a graph (csrc/connect_graph.hip): the parity union-find word of every voxel (uint32)
  WS_CG_AUX,                       // ... per voxel, meaningful at roots: the lowest seed rank, then the cluster number and the anchor's sign (int32)
  WS_CG_LIST,                      // ... the listed voxels' indices, then their cluster number and sign (2 x int32 per entry)
  WS_CG_REC,                       // ... the listed voxels' Hessians and directions for the host's vector test (9 floats per entry), then its bits
  WS_CG_SEEDS,                     // ... the ranked seeds, their roots, signs and numbers (4 x int32 per seed)
  WS_CG_CLUSTER,                   // ... per cluster: size, coordinate sums, centre of mass, outward sum, final label, bound (10 x 8 bytes)
  WS_CG_COUNTERS,                  // ... the two list lengths and the reason flags
  WS_CG_SETTLE,                    // ... option connect_settle: the gathered voxels (index, code, direction, weight: 6 x 4 bytes per entry)
  WS_CG_LINKS,                     // ... option connect_settle: per must-link location its rounded position, nearest-voxel key, code and direction
  WS_OVL_LIST,                     // DiscardOverlappingBlobs (csrc/discard_overlap.hip): the per-blob arrays: sort keys and values, records in sorted and
                                   // in bucket order, sorted scores, states, the two lists of undecided blobs
  WS_OVL_CELLS,                    // ... the buckets' offsets, one word per centre cell plus one
  WS_OVL_TEMP,                     // ... the reduction words, the counters, and the sort's and the scan's temporary storage
  WS_VOX_TOGGLE,                   // VoxelizeMesh (csrc/voxelize.hip): the toggle volume, nx + 1 bits per row (iy, iz) in 32-bit words
  WS_VOX_MESH,                     // ... the quantised vertices, the triangles, the tiled triangles' ids and running item counts, the counters
  WS_SP_BITS,                      // surface points (csrc/surface_points.hip): one selection bit per voxel, a byte per 8 voxels
  WS_SP_CHUNKS,                    // ... per workgroup chunk its count (uint32) and its list offset (uint64); the counters; the table of arc lengths
  WS_SP_LIST,                      // ... the selected voxels' linear indices in raster order (int64)
  WS_SP_OUT,                       // ... per listed voxel its position and its normal (2 x 3 floats), then the ridge records (9 floats)
  WS_SP_SCRATCH,                   // ... the backward weights of one batch of walks, [step][lane]
  WS_CS_ACC,                       // close_surface (csrc/close_surface.hip): the three int64 volumes of the splat over the padded box
  WS_CS_GRID,                      // ... per multigrid level the two iterates and the right-hand side (rows padded to a multiple of 4 floats)
  WS_CS_AUX,                       // ... the workgroups' partial sums (double), the three totals, the counters
  WS_ISO_TAB,                      // isosurface (csrc/isosurface.hip): the polygon tables of the 6 tets (their slot key: a version string)
  WS_ISO_CODE,                     // ... one byte per lower node: the insideness of its cell's 8 corners
  WS_ISO_CHUNKS,                   // ... per workgroup chunk its offsets (2 x uint64) and its counts (4 x uint32), then the 4 totals
  WS_ISO_FIRST,                    // ... every lower node's first vertex id (int32)
  WS_ISO_OUT,                      // ... the host-pointer face's vertices and triangles
  WS_SELECT,                       // radix select with the digit picked on the device: its state block (SelectState), and behind it the words
                                   // the queued membrane stage reads back with it (StageReadback) -- theirs alone, no pending scan owns any
  WS_NSLOTS
};

struct BlobJob;   // blob_job.hip: one visfd_hip_blob_dog_begin_dev that has not been ended or aborted yet

}  // namespace vh

// Tuning and test switches: read ONCE from the environment when the context is created (VISFD_HIP_<NAME>) and
// changed afterwards only through visfd_hip_set_option -- no getenv on any hot path.
struct visfd_hip_options {
  int gauss_3pass = 0;      // 1: the separable filter always takes its three single-axis passes
  int gauss_cfg = 0;        // development aid, kept for set/get: currently selects nothing
  int gauss_wg_per_cu = 2;  // workgroups per CU the single-sweep filter cuts the volume into
  int log_pair = 1;         // both Gaussians of an unmasked DoG/LoG scale in two shared launches (csrc/gauss_pair.hip): 0 never,
                            // 1 for the half-widths its table lists, 2 wherever it applies
  int log_pair_chunk = 0;   // march length of those launches along z and y (0: default); tests put chunk seams into small volumes
  int membrane_queue = 1;   // the membrane stage queued in one go (csrc/api.hip: membrane_stage): the select's digits picked on the device, no
                            // threshold pass, one wait per stage with the direction kernel queued behind it; 0: a host walk after every
                            // select round, the threshold pass, a wait for the lists' total.  The bits are the same either way.
                            // (The slab stage's select is always the queued one: a host walk would have to fetch the ranks' sums)
  int tv_dense = 0;         // 1: tensor voting by the baseline kernel (csrc/tv.hip)
  int tv_fma = 0;           // 1: TOLERANCE MODE of tensor voting: fused multiply-adds, results within 1e-5 of the field's scale
                            //    instead of bit-identical (surfaces, exponent 2 or 4; everything else stays exact)
  int gauss_fma = 0;        // 1: TOLERANCE MODE of the single-sweep Gaussian (plain ApplyGauss only; DoG/LoG stay exact)
  int eig_f32 = 0;          // 1: TOLERANCE MODE of the device eigen solver: its one angle (atan2, sin, cos) in single precision --
                            //    eigenvalues and scores move by ~1 float ulp (eigen3.hpp); 0: the reference's double-precision angle
  int tv_zrun = 0;          // receiver planes per unit of work (0: default)
  int tv_no_replay = 0;     // 1: list every sender plane again for every receiver plane (nothing reused from the rings)
  int tv_exact_tiled = 0;   // 1: exact tensor voting always on tv_tiled.hip (the round-2 kernel), never on the exact form of tv_box.hip
  int tv_no_fold = 0;       // tests: tolerance-mode voting never folds the saliency into the listed normals (tv_box.hip: vote_fma)
  int tv_poison = 0;        // tests: NaN bit patterns in LDS, ring memory and the output before tensor voting runs (tv_box.hip)
  int tv_reserve_wg = 0;    // workgroup slots the persistent voting grid leaves free (slab runs: the halo transport's kernels)
  int tv_max_wg = 0;        // cap on the persistent grid (0: fill the chip); tests use it to make workgroups claim many units
  int64_t blob_test_cap = 0;   // pretend the pipelined blob scan's buffers hold this many entries (0: off)
  int morph_general = 0;    // 1: morphology always on the general element walk (csrc/morph.hip), never on the flat X-run path
  int morph_levels = 1;     // flat balls on images of at most two levels as a threshold on the distance map (csrc/morph_levels.hip):
                            // 0 never, 1 when eligible and ceil(radius) > 10 or radius >= 5 (R0, profiles/morph_levels_time.txt), 2 whenever eligible
  int filter3d_general = 0; // 1: the general 3-D filter always on the entry walk (csrc/filter3d.hip), never on the tiled kernel
  int median_general = 0;   // 1: the median filter always on the general footprint walk (csrc/median.hip), never on the LDS-tiled kernel
  int distance_general = 0; // 1: distance maps by the brute-force walks (csrc/distance.hip), never by the separable transform
  int discard_overlap_host = 0;   // 1: visfd_hip_discard_overlapping_blobs_ctx / _dev run the host entry (csrc/blob_post.cpp), never the rounds on the device
  int discard_overlap_time = 0;   // 1: those two time their phases with events on the stream (visfd_hip_discard_overlapping_blobs_last_times; tools/discard_overlap_time.py)
  int discard_overlap_max_rounds = 256;   // rounds of csrc/discard_overlap.hip after which the host finishes the list from the states so far (a cap, not a tuning knob)
  int find_spheres_host = 0; // 1: FindSpheres walks the pairs on the host (csrc/find_spheres.hip), never launches the search kernel
  int watershed_host = 0;   // 1: the watershed runs the sequential host flood without markers too (csrc/watershed_host.cpp)
  int stats_blocks = 0;     // workgroups of the statistics / intensity-map kernel (csrc/intensity.hip); 0: eight per CU
  int connect_time = 0;     // 1: visfd_hip_label_connected_graph[_dev] time their stages on the host clock and wait for each (tools/connect_graph_time.py)
  int connect_settle = 0;   // 1: visfd_hip_label_connected_graph[_dev] settle must-links, voxel weights and doubtful outward sums on the
                            //    device path instead of handing the call to the flood (csrc/connect_graph.hip)
  int draw_time = 0;        // 1: DrawSpheres times its zero fill, scatter and resolve with events and waits for them (tools/draw_time.py)
  int voxelize_bisect = 0;  // tests: VoxelizeMesh finds every crossing's sample by bisection with the exact sign, never from the double estimate
  int voxelize_time = 0;    // 1: VoxelizeMesh times its zero fill, scatter and fill with events (tools/voxelize_time.py)
  int surface_steps_cap = 256;   // visfd_hip_surface_points_ctx / _dev: steps a walk may take per direction on the device; a call in which
                            //    a walk needs more is finished by the host entry.  One float of scratch per step and lane of a batch:
                            //    256 steps x 262144 lanes = 256 MiB (csrc/surface_points.hip).  Clamped to 1..65536
  int surface_points_time = 0;   // 1: those two time their stages (visfd_hip_surface_points_last_times; tools/surface_points_time.py)
  int close_surface_rtol_exp = 5;   // close_surface stops its cycles when |b - Laplace(chi)| <= 10^-k |b| (profiles/close_surface_time.txt)
  int close_surface_max_cycles = 20;   // ... or after this many cycles: the mask is still returned, visfd_hip_close_surface_last says which
  int close_surface_time = 0;   // 1: close_surface times its splat, solve and cut with events (visfd_hip_close_surface_last_times; tools/close_surface_time.py)
  int isosurface_time = 0;   // 1: visfd_hip_isosurface[_dev] time their four phases with events (visfd_hip_isosurface_last_times; tools/isosurface_time.py)
  int debug = 0;
};

struct visfd_hip_ctx {
  visfd_hip_options opt;
  int device = 0;
  hipStream_t stream = nullptr;
  bool own_stream = false;
  void* slot_ptr[vh::WS_NSLOTS] = {};
  size_t slot_bytes[vh::WS_NSLOTS] = {};
  std::vector<unsigned char> slot_key[vh::WS_NSLOTS];   // what a slot's contents were built from (ws_holds / ws_put); empty: nothing remembered
  int num_cus = 256;
  hipStream_t aux_stream = nullptr;   // host copies that must not queue behind the main stream's kernels
  void* stage_pinned = nullptr;       // the queued membrane stage's one readback (StageReadback, pinned host memory) and the event
  hipEvent_t stage_event = nullptr;   // behind its copy; both made by the first such stage, gone with the context
  int morph_last_path = -1;           // the kernel the last morphology call ran (VISFD_HIP_MORPH_PATH_*)
  struct {                            // of the filter table expanded into slot WS_F3D_TAB, valid only while that slot's key holds:
    int64_t n = 0, ncols = 0;         // the number of its non-zero entries, of the columns (jy, jx) that hold one,
    float den = 0.0f;                 // and the entries' float sum in order
  } f3d;
  int f3d_last_path = -1;             // the kernel the last general-filter call ran (VISFD_HIP_FILTER3D_PATH_*)
  int median_last_path = -1;          // the kernel the last median call ran (VISFD_HIP_MEDIAN_PATH_*)
  int distance_last_path = -1;        // what the last distance call ran (VISFD_HIP_DISTANCE_PATH_*)
  int find_spheres_last_path = -1;    // what the last FindSpheres call ran (VISFD_HIP_FIND_SPHERES_PATH_*)
  int64_t discard_overlap_last[8] = {-1, 0, 0, 0, 0, 0, 0, 0};   // the last visfd_hip_discard_overlapping_blobs_ctx / _dev (visfd_hip_discard_overlapping_blobs_last)
  float discard_overlap_ms[5] = {-1.0f, -1.0f, -1.0f, -1.0f, -1.0f};   // option discard_overlap_time: reduction, ranking and records, buckets, rounds, compaction
  float draw_ms[3] = {-1.0f, -1.0f, -1.0f};   // option draw_time: zero fill, scatter (with count and values), resolve of the last DrawSpheres
  int64_t voxelize_stats[4] = {-1, -1, -1, -1};   // the last VoxelizeMesh: crossings, skipped triangles, odd rows, inside voxels
  float voxelize_ms[3] = {-1.0f, -1.0f, -1.0f};   // option voxelize_time: zero fill, scatter, fill of the last VoxelizeMesh
  int64_t surface_points_last[6] = {-1, 0, -1, -1, -1, -1};   // the last visfd_hip_surface_points_ctx / _dev: path, reasons, selected voxels, points, longest walk, steps taken
  float surface_points_ms[4] = {-1.0f, -1.0f, -1.0f, -1.0f};   // option surface_points_time: select and compact, walk, ridge gather, host finish and copies
  int64_t close_surface_last[6] = {-1, -1, -1, -1, -1, -1};   // the last close_surface: used and skipped points, cycles, stop reason, orientation taken, mask on a face
  double close_surface_values[2] = {0.0, 0.0};   // ... its final residual ratio and its level iso
  float close_surface_ms[3] = {-1.0f, -1.0f, -1.0f};   // option close_surface_time: splat and right-hand side, solve, level and cut
  int64_t isosurface_last[4] = {-1, -1, -1, -1};   // the last visfd_hip_isosurface[_dev]: vertices, triangles, inside nodes, 1 if the image border cut the solid
  float isosurface_ms[4] = {-1.0f, -1.0f, -1.0f, -1.0f};   // option isosurface_time: classify, scan and the host's read of the totals, vertices, triangles
  int64_t wsh_stats[4] = {-1, -1, -1, -1};   // the last watershed call: path, label rounds, boundary rounds, basins
  int64_t connect_seeds[2] = {-1, -1};       // the last visfd_hip_label_connected_device_seeds: where the seeds were searched, how many (csrc/connect_seeds.hip)
  int64_t connect_graph[4] = {-1, 0, -1, -1};   // the last visfd_hip_label_connected_graph[_dev]: path, reasons, valid voxels, candidates of the host's vector test
  unsigned connect_graph_settled = 0;        // option connect_settle: the reason bits the last device-path call settled itself
  float connect_graph_ms[8] = {-1.0f, -1.0f, -1.0f, -1.0f, -1.0f, -1.0f, -1.0f, -1.0f};   // option connect_time: its stages (csrc/connect_graph.hip: MS_*)
  std::vector<vh::BlobJob*> blob_jobs;   // the context's live blob jobs (blob_job.hip)
};

namespace vh {

// Collects every scan that live blob jobs of the context (all but `except`) have queued and not fetched yet into the jobs'
// host lists; afterwards those jobs hold no pointer into the workspace.  Called before anything frees, reallocates or
// overwrites the buffers a pending scan writes to (WS_CAND, WS_SCANCNT): ws_get when one of them grows, visfd_hip_trim,
// and every scan launched for another job.  With nothing pending -- the usual case -- it is a loop over an empty list.
int blob_jobs_drain(visfd_hip_ctx* ctx, const BlobJob* except = nullptr);
void blob_jobs_abort(visfd_hip_ctx* ctx);   // visfd_hip_destroy: the context's jobs go with it (their handles then name no live job)

// returns a device buffer of at least `bytes` bytes in slot `s` (contents undefined)
int ws_get(visfd_hip_ctx* ctx, Slot s, size_t bytes, void** out);
template <typename T>
inline int ws(visfd_hip_ctx* ctx, Slot s, size_t count, T** out) {
  void* p = nullptr;
  int rc = ws_get(ctx, s, count * sizeof(T), &p);
  *out = static_cast<T*>(p);
  return rc;
}
// A table a stage keeps in its slot between calls.  ws_holds: the slot's contents were built from these key bytes -- host
// compares only, so a hit queues nothing and never waits for the stream.  ws_put: `bytes` of host memory into the slot
// under that key.  ws_get, visfd_hip_trim and visfd_hip_debug_poison_workspace drop the key where the contents go.
bool ws_holds(const visfd_hip_ctx* ctx, Slot s, const void* key, size_t key_bytes);
int ws_put(visfd_hip_ctx* ctx, Slot s, const void* key, size_t key_bytes, const void* host, size_t bytes);

inline int check_dims(i64 nx, i64 ny, i64 nz) {
  if (nx <= 0 || ny <= 0 || nz <= 0) return fail(VISFD_HIP_EINVAL, "image dimensions must be positive");
  return VISFD_HIP_OK;
}
// two byte ranges share a byte (a null pointer shares none)
inline bool overlap_bytes(const void* a, size_t na, const void* b, size_t nb) {
  const char* p = static_cast<const char*>(a);
  const char* q = static_cast<const char*>(b);
  return p && q && p < q + nb && q < p + na;
}
inline bool overlaps(const float* a, const float* b, i64 n) { return overlap_bytes(a, sizeof(float) * n, b, sizeof(float) * n); }
inline int check_dims32(i64 nx, i64 ny, i64 nz) {   // for the kernels that index a volume with 32-bit coordinates
  if (nx >= (1LL << 31) || ny >= (1LL << 31) || nz >= (1LL << 31)) return fail(VISFD_HIP_EINVAL, "dimension too large");
  return VISFD_HIP_OK;
}
// what a filter that cannot run in place says first about its arrays: `who` cannot, `tag` starts the mask's message
inline int check_out_of_place(const visfd_hip_ctx* ctx, const float* src, const float* dst, const float* mask, i64 nx, i64 ny,
                              i64 nz, const char* who, const char* tag) {
  VH_REQUIRE(ctx && src && dst, "null argument");
  VH_TRY(check_dims(nx, ny, nz));
  VH_REQUIRE(!overlaps(src, dst, nx * ny * nz), std::string(who) + " cannot run in place (dst overlaps src)");
  VH_REQUIRE(!overlaps(mask, dst, nx * ny * nz), std::string(tag) + ": dst overlaps mask");
  return VISFD_HIP_OK;
}

// Events on a stream at the boundaries of a call's N phases, for the *_time options: mark(k) is the boundary before
// phase k, mark(N) the end.  Events are created when first marked and go with the clock, whichever way the call returns.
template <int N>
struct PhaseClock {
  hipStream_t st = nullptr;
  bool on = false;
  hipEvent_t ev[N + 1] = {};
  bool set[N + 1] = {};
  void start(hipStream_t s, bool enabled) {
    st = s;
    on = enabled;
    mark(0);
  }
  void mark(int k) {   // marked again, the later one counts
    if (!on) return;
    if (!ev[k] && hipEventCreate(&ev[k]) != hipSuccess) { ev[k] = nullptr; return; }
    set[k] = hipEventRecord(ev[k], st) == hipSuccess;
  }
  // the stream is idle; a phase that did not run has -1
  void read(float* ms) {
    for (int k = 0; k < N; k++) {
      ms[k] = -1.0f;
      if (!on || !set[k]) continue;
      int e = k + 1;
      while (e <= N && !set[e]) e++;
      if (e <= N && hipEventElapsedTime(&ms[k], ev[k], ev[e]) != hipSuccess) ms[k] = -1.0f;
    }
  }
  ~PhaseClock() {
    for (hipEvent_t e : ev)
      if (e) (void)hipEventDestroy(e);
  }
};

// blob_post.cpp: steps 2 to 4 of DiscardOverlappingBlobs (bounds, the greedy walk over the occupancy grid, compaction) on a
// list that is sorted already; `states` (nullable): what the device's rounds have decided, one OVERLAP_* byte per blob
enum : unsigned char { OVERLAP_UNDECIDED = 0, OVERLAP_KEPT = 1, OVERLAP_DISCARDED = 2 };
void overlap_walk_sorted(float* crds, float* diameters, float* scores, int64_t* n_inout, const unsigned char* states,
                         float min_radial_separation_ratio, float max_volume_overlap_large, float max_volume_overlap_small,
                         int scale);

// ---- taps carried in the kernel-argument segment (scalar loads, SGPR operands) ---------------
constexpr int MAX_HALFWIDTH = 64;
struct Taps {
  float t[2 * MAX_HALFWIDTH + 1];  // t[j + h], j = -h..h
  int h;
};

// host-side arithmetic (taps.cpp)
void host_gauss_taps(float sigma, int h, float* t);
void host_conv_ones(i64 n, const float* t, int h, float* out);  // filter applied to a line of ones
int host_iso_halfwidth(float sigma, float ratio);   // the isotropic Gaussian's: what gauss_iso_dev runs and the slab stage sizes halos by
int host_tv_halfwidth(float sigma, float cutoff);
void host_tv_tables(float sigma, int h, float* w, float* rhat);
float host_gengauss3d_peak(const float width[3], float m_exp, float ratio);
void host_gengauss3d_table(const float width[3], float m_exp, const int hw[3], float* table_out, float* A_out);
void host_gengauss3d_halfwidths(const float width[3], float m_exp, float ratio, float threshold, int hw[3]);
i64 host_dogg3d_table(const float width_a[3], const float width_b[3], float m_exp, float n_exp, float ratio,
                      float threshold, int hw[3], float* table_out, i64 cap, float* A_out, float* B_out);
i64 host_sphere_structure(float radius, float radius_max, float bmax, int* dxyz, float* b, i64 cap);

// ---- device stages (each in its own .hip; all asynchronous on ctx->stream) -------------------
// The optional tail of a Gaussian call.  With a minuend, dst receives (minuend - G(src)) * log_scale -- the DoG/LoG
// epilogue, applied on every route by the launch that writes dst, which may be the minuend itself.
struct GaussOpts {
  float* A_out = nullptr;          // the filter's peak weight (filter3d.hpp:1044-1046)
  const float* minuend = nullptr;
  float log_scale = 1.0f;
  bool fma = false;                // tolerance mode (option gauss_fma) for callers whose output is a float field; ignored with a minuend
  i64 z_lo = 0, nz_global = 0;     // Z-slab placement of a multi-GPU run: the arrays hold planes [z_lo, z_lo + nz) of nz_global; 0: the whole volume
};
int dev_separable3d(visfd_hip_ctx* ctx, const float* src, float* dst, const float* mask, i64 nx, i64 ny, i64 nz,
                    const float* tx, int hx, const float* ty, int hy, const float* tz, int hz, bool normalize,
                    const GaussOpts& o = {});

// What a Gaussian launch carries below the tap-building level: gauss.hip fills one per call and routes it to the three
// single-axis passes or, through the one entry point per compiled half-width, to the single sweep (gauss_fused.hip).
struct GaussRequest {
  const float* src;
  float* dst;
  i64 nx, ny, nz;
  Taps tx, ty, tz;
  const float *Dx, *Dy, *Dz;   // boundary normaliser lines (null without the box normaliser); Dz is indexed by iz + dz_offset
  i64 dz_offset;
  bool normalize;              // divide by (Dx*Dy)*Dz
  bool zpass;                  // single sweep: false runs the Y and X passes only (tz is then not looked at)
  const float* minuend;        // DoG/LoG epilogue, see GaussOpts
  float log_scale;
  bool fma;
  const float* numer;          // Y/X sweep of a mask denominator: dst = numer / result where result > 0, numer elsewhere
};

// A route returns VISFD_HIP_OK, an error, or GAUSS_DECLINED: nothing launched, the caller takes the next route.
constexpr int GAUSS_DECLINED = -1;
// gauss.hip: the boundary normaliser lines Dx | Dy | Dz of one filter into D (nx + ny + nz floats), on the device
int dev_norm_lines(visfd_hip_ctx* ctx, float* D, i64 nx, i64 ny, i64 nz, const Taps& tx, const Taps& ty, const Taps& tz);

// gauss_pair.hip: dst = (G_a(src) - G_b(src)) * scale, unmasked and normalised, both filters in two shared launches.
// a[d], b[d]: the taps of the two filters along x, y, z; dst may be src.  Declines what it does not cover.
struct LogPairRequest {
  const float* src;
  float* dst;
  i64 nx, ny, nz;
  Taps a[3], b[3];
  float scale;
  i64 z_lo, nz_global;   // Z-slab placement, as in GaussOpts
};
int log_pair_route(visfd_hip_ctx* ctx, const LogPairRequest& rq);

// api.hip: the Gaussian from sigmas and half-widths, and ApplyLog
int gauss_dev(visfd_hip_ctx* ctx, const float* src, float* dst, const float* mask, i64 nx, i64 ny, i64 nz,
              const float sigma[3], const int hw[3], bool normalize, const GaussOpts& o = {});
struct LogPlan {
  float sa[3], sb[3], scale;
  int hw[3];
};
LogPlan plan_log(const float sigma[3], float delta, float ratio);
int log_dev(visfd_hip_ctx* ctx, const float* src, float* dst, const float* mask, i64 nx, i64 ny, i64 nz,
            const float sigma[3], float delta, float ratio, float* A, float* B);
// LocalFluctuations element-wise steps (filter3d.hpp:1776-1790 and :1819-1846)
int dev_sub_square(visfd_hip_ctx* ctx, const float* a, const float* b, float* out, i64 n);   // out = (a-b)*(a-b)
int dev_scale_clamp_sqrt(visfd_hip_ctx* ctx, float* a_inout, i64 n, float scale);           // a = sqrt(max(a*scale, 0))

// What a queued scan of the pipelined form writes to, as decided when it was launched: blob_scan_collect reads these and
// nothing of the context's current state (slot sizes and options may have changed since).
struct ScanPending {
  const unsigned long long* counters = nullptr;   // [0]: candidates, [1]: verified
  const void* survivors = nullptr;
  size_t cap_idx = 0, cap_out = 0;
};
// `owner`: the job the scan belongs to (the pending scans of every other job of the context are collected first: the
// buffer sets are shared)
int blob_scan_launch(visfd_hip_ctx* ctx, const BlobJob* owner, int set, hipEvent_t done, const float* lo, const float* mid,
                     const float* hi, const float* mask, i64 nx, i64 ny, i64 nz, float min_thr, float max_thr,
                     ScanPending* pending);
int blob_scan_collect(visfd_hip_ctx* ctx, const ScanPending& pending, hipEvent_t done, hipStream_t aux, i64 nx, i64 ny,
                      int scale_index,
                      float sigma, std::vector<visfd_hip_blob>* minima, std::vector<visfd_hip_blob>* maxima,
                      bool* overflow);
int dev_blob_scan(visfd_hip_ctx* ctx, const float* lo, const float* mid, const float* hi,
                  const float* mask, i64 nx, i64 ny, i64 nz, int scale_index, float sigma,
                  float min_thr, float max_thr, bool want_min, bool want_max,
                  std::vector<visfd_hip_blob>* minima, std::vector<visfd_hip_blob>* maxima);

int dev_hessian(visfd_hip_ctx* ctx, const float* smoothed, const float* mask, i64 nx, i64 ny, i64 nz,
                float sigma, float* grad_planar, float* hess_planar);
int dev_hessian_saliency(visfd_hip_ctx* ctx, const float* hess_planar, const float* mask, i64 nvox,
                         int order, float* saliency, float* dir_planar);
int dev_ridge_saliency_fused(visfd_hip_ctx* ctx, const float* smoothed, const float* mask, i64 nx,
                             i64 ny, i64 nz, float sigma, int order, float* saliency,
                             float* dir_planar);
// peak_img / peak_bg (nullable pair): score *= peak_img - peak_bg, the reference's optional peak-height factor
// (bin/filter_mrc/handlers.cpp:1698-1702 and :1883-1887, `-membrane-background`)
int dev_ridge_score(visfd_hip_ctx* ctx, const float* smoothed, const float* mask, i64 nx, i64 ny, i64 nz,
                    float sigma, int order, float* saliency, const float* peak_img = nullptr, const float* peak_bg = nullptr);
// thr_dev (nullable, device memory): the saliency volume has not been cut; a voxel survives if !(s < *thr_dev) && s != 0 --
// the voxels dev_apply_threshold followed by s != 0 keeps
int dev_ridge_directions(visfd_hip_ctx* ctx, const float* smoothed, const float* saliency, i64 nx, i64 ny, i64 nz,
                         float sigma, int order, float* dir_planar, const float* thr_dev = nullptr);
int dev_diagonalize(visfd_hip_ctx* ctx, const float* m6_planar, float* out6_planar, i64 n, int order);
int dev_tensor_saliency(visfd_hip_ctx* ctx, const float* tensor_planar, const float* mask, i64 nvox,
                        int order, float* saliency, const float* peak_img = nullptr, const float* peak_bg = nullptr);

int dev_select_histogram(visfd_hip_ctx* ctx, const float* sal, const float* mask, i64 nvox, int pass,
                         uint32_t prefix, uint64_t* hist_host, uint64_t* n_unmasked_host);
int dev_select_histogram_todev(visfd_hip_ctx* ctx, const float* sal, const float* mask, i64 nvox, int pass, uint32_t prefix,
                               uint64_t* hist);
// The select with no host step between its rounds (select.hip: pick_kernel): what the device keeps of it.
enum : uint32_t { SELECT_NO_VOXEL = 1u, SELECT_INCONSISTENT = 2u };
struct SelectState {
  uint32_t prefix;   // the digits picked so far, right-aligned; after round 2 the order key of the threshold
  uint32_t flag;     // 0, or why there is no threshold (SELECT_*)
  uint64_t k;        // the rank left inside the picked bins
  uint64_t n;        // round 0's total: the unmasked voxels
  float thr;         // after round 2: the threshold (+inf with a flag)
  uint32_t pad;
};
// What the queued membrane stage reads back in its one copy (slot WS_SELECT holds the same layout on the device)
struct StageReadback {
  SelectState sel;
  unsigned long long list_total;   // tv_list.hip: the sender lists' length
  unsigned list_flags, pad;        // ... and what their count pass saw (TVL_*)
};
// A select over the ranks of a slab run: called after each round's histogram_kernel and before its pick_kernel, it sums
// the `count` counters over the ranks, in place, ordered on `stream` (the context's); returns a VISFD_HIP_* code.  Every
// rank then picks from the same sums, so every rank picks the same digit, and round 0's total is the global n.
struct SelectReduce {
  int (*sum)(void* user, uint64_t* hist, size_t count, hipStream_t stream);
  void* user;
};
int dev_select_queue(visfd_hip_ctx* ctx, const float* sal, const float* mask, i64 nvox, float fraction, SelectState* state_dev,
                     const SelectReduce* reduce = nullptr);
int select_result(const SelectState& s, float* thr_out);   // the state read back: the threshold, or the select's error
int select_rank_check(uint64_t n, float fraction);         // the select's VISFD_HIP_EINVAL, from n alone (no mask: n is known before round 0)
int dev_apply_threshold(visfd_hip_ctx* ctx, float* sal, i64 nvox, float thr);
// the queued form whatever the option says (the slab stage); dev_threshold_fraction takes it under membrane_queue
int dev_threshold_queued(visfd_hip_ctx* ctx, float* sal, const float* mask, i64 nvox, float fraction, float* thr_out,
                         const SelectReduce* reduce = nullptr);
int dev_threshold_fraction(visfd_hip_ctx* ctx, float* sal, const float* mask, i64 nvox, float fraction,
                           float* thr_out);

int dev_tv_dense_stick(visfd_hip_ctx* ctx, const float* sal, const float* dir_planar,
                       float* tensor_planar, const float* mask_src, const float* mask_dst, i64 nx,
                       i64 ny, i64 nz, i64 z_out0, i64 z_out1, float sigma_tv, int exponent,
                       float cutoff, bool curves);

int dev_tv_weight_sum(visfd_hip_ctx* ctx, const float* sal, float* den, const float* mask_src, const float* mask_dst, i64 nx,
                      i64 ny, i64 nz, float sigma_tv, float cutoff);

// A structuring element as the morphology kernels see it (the entries themselves are in slot WS_MORPH_TAB).
// runs: every b is +0.0f and every (dy, dz) row of the element is one symmetric X-run [-L, L], |dy|, |dz|, L <= R <=
// MORPH_RUN_MAX_R; run_len[(dz + R) * (2R + 1) + dy + R] = L, or -1 where the row is not in the element.
constexpr int MORPH_RUN_MAX_R = 10;
struct MorphElem {
  i64 n = 0;
  int lo[3] = {0, 0, 0}, hi[3] = {0, 0, 0};
  bool flat = true;
  bool runs = false;
  int R = 0;
  signed char run_len[(2 * MORPH_RUN_MAX_R + 1) * (2 * MORPH_RUN_MAX_R + 1)];
};

// morph.hip: Dilate / Erode with a structuring element already in WS_MORPH_TAB.  el.runs selects the X-run kernel
// (window maxima per row, then a zero-sign fix-up of flat erosions in element order), otherwise the element walk.
// Neighbours come from `src`, whose excluded voxels the caller has made NaN (a NaN candidate never wins, exactly like a
// skipped one).  Voxels with mask == 0 are left untouched, or set to NaN when nan_masked (an intermediate image).
// epi: 0 dst = result, 1 dst = dst - result (white top-hat), 2 dst = result - dst (black top-hat).
// Returns the path it took in *path (VISFD_HIP_MORPH_PATH_*).
int dev_morph_table(visfd_hip_ctx* ctx, const float* src, float* dst, const float* mask, i64 nx, i64 ny, i64 nz,
                    const MorphElem& el, bool dilate, int epi, bool nan_masked, int* path);
// out = (mask == 0) ? NaN : src
int dev_nan_masked(visfd_hip_ctx* ctx, const float* src, const float* mask, float* out, i64 n);
// the orchestration (tail of morph.hip): an element into WS_MORPH_TAB (`el` describes it), and one op with it
int morph_put_table(visfd_hip_ctx* ctx, const int* dxyz, const float* b, i64 n, MorphElem* el);
int morph_run(visfd_hip_ctx* ctx, const float* src, float* dst, const float* mask, i64 nx, i64 ny, i64 nz, int op,
              MorphElem el);

// morph_levels.hip: flat balls on images of at most two levels.  The ball of DilateSphere with bmax == 0 is {d^2 <= T}:
// host_flat_ball_dsq_max is T, the largest integer whose double square root, rounded to float, is <= radius (radius
// finite and >= 0).  morph_levels_try decides whether a visfd_hip_morph_sphere[_dev] call is eligible (options, radii,
// dimensions, then the level census on the device) and, if so, runs it and sets *taken; otherwise it changes nothing.
i64 host_flat_ball_dsq_max(float radius);
constexpr float MORPH_LEVELS_R0 = 5.0f;   // option morph_levels = 1: the path is taken from this radius on (profiles/morph_levels_time.txt)
int morph_levels_try(visfd_hip_ctx* ctx, const float* src, float* dst, const float* mask, i64 nx, i64 ny, i64 nz, int op,
                     float radius, float radius_max, float bmax, bool* taken);
// What the last pass of the transform writes on that path instead of the squared distance, at voxels with mask != 0
// (the others: NaN when nan_masked, else untouched): v = dsq <= t ? near : far (bit patterns), then dst = v, dst - v
// (epi 1) or v - dst (epi 2) as morph.hip's epilogue does.
struct LevelsEpilogue {
  float* dst;
  const float* mask;
  int t;
  unsigned near_bits, far_bits;
  int epi, nan_masked;
};
// distance.hip: the row pass and the y pass of the transform into dsq with the voxels `src == level` (mask != 0) as
// seeds, then the z pass with that epilogue; dsq is scratch afterwards.  nx + ny + nz <= 46340.
int dev_distance_levels(visfd_hip_ctx* ctx, const float* src, const float* mask, i64 nx, i64 ny, i64 nz, float level,
                        int32_t* dsq, const LevelsEpilogue& e);

// median.hip: a footprint as the median kernels see it (the entries themselves are in slot WS_MEDIAN_TAB): the entry
// count, the bounding box of the offsets and the extent W x H x D of the tiled kernel's LDS image for that box.
struct MedianTab {
  i64 n = 0;
  int lo[3] = {0, 0, 0}, hi[3] = {0, 0, 0};
  int W = 0, H = 0, D = 0;
};
// a footprint of n entries (dx, dy, dz; host array) into WS_MEDIAN_TAB (`mt` describes it), and the median of src with it:
// voxels with mask == 0 are left untouched, neighbours outside the image or with mask == 0 are not collected, a voxel
// that collects nothing gets +0.0f.  The route is the LDS-tiled kernel where the bounding box fits its budget and the
// option median_general is off, else the general walk (ctx->median_last_path says which).
int median_put_table(visfd_hip_ctx* ctx, const int* dxyz, i64 n, MedianTab* mt);
int median_run(visfd_hip_ctx* ctx, const float* src, float* dst, const float* mask, i64 nx, i64 ny, i64 nz,
               const MedianTab& mt);

// distance.hip: dsq = min((nx + ny + nz)^2, squared distance to the nearest seed), int32 on the device.  Seeds: the voxels
// with mask != 0 and lo <= src <= hi (src nullable: none) and the `npoints` listed points (x, y, z; HOST array; anywhere).
// The separable transform, or the brute-force walks under the option distance_general (ctx->distance_last_path).
int dev_distance_sq(visfd_hip_ctx* ctx, const float* src, const float* mask, i64 nx, i64 ny, i64 nz, float lo, float hi,
                    const int32_t* points, i64 npoints, int32_t* dsq);

// filter3d.hip: Filter3D::Apply with an arbitrary table of (2 hx + 1)(2 hy + 1)(2 hz + 1) entries (x fastest), on device
// arrays.  dst = sum_j (H[j] * mask[i - j]) * src[i - j] in the reference's order, divided by den = sum_j H[j] * mask[i - j]
// where `normalize` and den > 0; den_out (nullable) receives den.  Voxels with mask == 0 get dst = 0 and den = 0.
int dev_filter3d(visfd_hip_ctx* ctx, const float* src, float* dst, const float* mask, i64 nx, i64 ny, i64 nz,
                 const float* table, const int hw[3], bool normalize, float* den_out);

// extrema.hip: plateau-aware minima and maxima (visfd_hip_find_extrema[_dev], include/visfd_hip.h)
struct ExtremaArgs {
  const float* src;
  const float* mask;
  i64 nx, ny, nz;
  int find_minima, find_maxima;
  float minima_threshold, maxima_threshold;
  int connectivity, allow_borders;
  int64_t *min_index, *min_nvoxels, *max_index, *max_nvoxels;
  float *min_score, *max_score;
  int64_t min_cap, max_cap;
  int64_t *n_min, *n_max;
  int32_t* labels;
};
// everything that can be said without a device, the context last
int extrema_check_args(const visfd_hip_ctx* ctx, const ExtremaArgs& a);
// src, mask, labels on the device; the lists on the host.  Returns with the stream idle.
int dev_find_extrema(visfd_hip_ctx* ctx, const ExtremaArgs& a);

// The watershed's seeds: the whole sorted list of one kind of extremum (borders allowed), the plateaus' roots and values.
// Returns with the stream idle.
int dev_extrema_seeds(visfd_hip_ctx* ctx, const float* src, const float* mask, i64 nx, i64 ny, i64 nz, bool minima,
                      float threshold, int connectivity, std::vector<int>* index, std::vector<float>* score);

// resample.hip (sizes are {nx, ny, nz}; offset nullable)
int dev_bin_array3d(visfd_hip_ctx* ctx, const float* src, const int64_t size_src[3], float* dst,
                    const int64_t size_dst[3], const int* offset);
int dev_unbin_array3d(visfd_hip_ctx* ctx, const float* src, const int64_t size_src[3], float* dst,
                      const int64_t size_dst[3], const int* offset);

// layout helpers for the host-pointer face
int dev_interleaved_to_planar(visfd_hip_ctx* ctx, const float* aos, float* planar, i64 n, int channels);
int dev_planar_to_interleaved(visfd_hip_ctx* ctx, const float* planar, float* aos, i64 n, int channels,
                              const float* mask /*nullable: only where mask!=0*/);

// How the host-pointer entry points move the caller's arrays through the workspace slots: every copy is asynchronous on
// ctx->stream, and `down` ends with the call's synchronisation.
struct Stage {
  visfd_hip_ctx* ctx;
  size_t n;   // voxels; an array has channels * n floats

  // channels * n floats in slot s, filled from the caller's array unless `fill` is null
  int out(Slot s, float** dev, int channels = 1, const float* fill = nullptr) const {
    VH_TRY(ws(ctx, s, channels * n, dev));
    if (fill) VH_HIP(hipMemcpyAsync(*dev, fill, sizeof(float) * channels * n, hipMemcpyHostToDevice, ctx->stream));
    return VISFD_HIP_OK;
  }
  // a nullable host array into slot s: a null one takes no memory and gives a null device pointer
  int up(Slot s, const float* host, float** dev, int channels = 1) const {
    *dev = nullptr;
    return host ? out(s, dev, channels, host) : VISFD_HIP_OK;
  }
  int down(float* host, const float* dev, int channels = 1) const {
    VH_HIP(hipMemcpyAsync(host, dev, sizeof(float) * channels * n, hipMemcpyDeviceToHost, ctx->stream));
    VH_HIP(hipStreamSynchronize(ctx->stream));
    return VISFD_HIP_OK;
  }
  // an interleaved host array into slot s_aos and, channel by channel, into slot s_planar
  int up_planar(Slot s_aos, Slot s_planar, const float* host, int channels, float** planar, float** aos = nullptr) const {
    float* a = nullptr;
    VH_TRY(out(s_aos, &a, channels, host));
    VH_TRY(out(s_planar, planar, channels));
    if (aos) *aos = a;
    return dev_interleaved_to_planar(ctx, a, *planar, (i64)n, channels);
  }
  // planar channels back to the caller's interleaved array through the device buffer `aos`.  keep: the caller's values
  // go up first, so that voxels with mask == 0 (which the interleave skips) come back as they were
  int down_interleaved(float* host, const float* planar, float* aos, int channels, const float* mask, bool keep) const {
    if (keep) VH_HIP(hipMemcpyAsync(aos, host, sizeof(float) * channels * n, hipMemcpyHostToDevice, ctx->stream));
    VH_TRY(dev_planar_to_interleaved(ctx, planar, aos, (i64)n, channels, mask));
    return down(host, aos, channels);
  }
};

// The commonest face: the checks every such face starts with (those that have checked more already pass them again), src
// and mask up (slots WS_H2D_0 and _1), dst reserved in WS_H2D_2 -- filled from the caller's array when the stage leaves
// some of its voxels alone or reads it (dst_up) -- `run(src, dst, mask)` on the device copies, and dst down.
template <typename Run>
int stage_filter(visfd_hip_ctx* ctx, const float* src, float* dst, const float* mask, i64 nx, i64 ny, i64 nz, bool dst_up,
                 Run run) {
  VH_REQUIRE(ctx && src && dst, "null argument");
  VH_HIP(hipSetDevice(ctx->device));
  VH_TRY(check_dims(nx, ny, nz));
  const Stage st = {ctx, (size_t)(nx * ny * nz)};
  float *ds, *dm, *dd;
  VH_TRY(st.up(WS_H2D_0, src, &ds));
  VH_TRY(st.up(WS_H2D_1, mask, &dm));
  VH_TRY(st.out(WS_H2D_2, &dd, 1, dst_up ? dst : nullptr));
  VH_TRY(run(ds, dd, dm));
  return st.down(dst, dd);
}

inline unsigned grid_for(i64 n, int block, i64 cap = (i64)1 << 30) {
  i64 g = (n + block - 1) / block;
  if (g > cap) g = cap;
  if (g < 1) g = 1;
  return (unsigned)g;
}

}  // namespace vh
