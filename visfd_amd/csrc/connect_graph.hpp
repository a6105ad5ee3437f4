// connect_graph.hpp -- LabelConnected as a graph problem (tests/connect_graph_np.py): what the host walk
// (connect_graph_host.cpp) and the device path (connect_graph.hip) share.
//
//   valid voxel      unmasked, passes the saliency threshold, the tensor test and the vector test
//   compatible edge  two valid neighbours whose neighbour tests pass in both directions
//   cluster          a connected component of (valid voxels, compatible edges) that holds a valid seed
//
// The per-voxel and per-pair arithmetic below is that of connect.cpp's flood (its pop loop), operand order kept, plain
// IEEE float without contraction; it is compiled for the host and for the device from this one text.  The principal
// eigenvector of the vector test is the exception: it is only ever computed on the host (vector_test below), because the
// device's libm moves it in the last place -- and by anything near a degenerate Hessian -- so no margin on the comparison
// would make a device verdict safe.
#pragma once

#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <vector>

#include "../../include/visfd_hip.h"

namespace vh {
namespace cg {

#define VH_CG_HD __host__ __device__ __forceinline__

// The union-find word of a voxel: (parent index << 1) | sign of the voxel relative to that parent.  A root points at
// itself with sign 0; NOT_VALID marks a voxel that is no vertex of the graph.  (index << 1) | 1 must stay below NOT_VALID,
// so an image may have at most 2^31 - 1 voxels; the entries hand over from 2^31 - 2 (VISFD_HIP_CONNECT_REASON_LIMITS).
constexpr unsigned NOT_VALID = 0xffffffffu;
constexpr int64_t MAX_VOXELS = ((int64_t)1 << 31) - 3;
constexpr int NO_SEED = 0x7fffffff;

struct Params {
  int nx, ny, nz;
  float thr, tvs, tvn, tts, ttn;   // saliency, vector (voxel, neighbour), tensor (voxel, neighbour); tvs, tvn clamped when unsigned
  float SIGN;                      // -1 from maxima, +1 from minima
  int signs, standardize, flip_hessian, has_t, has_v;
  int noff;
  int off[13][3];                  // the forward half of the neighbourhood (dx, dy, dz), raster order after the centre
};

inline int forward_offsets(int connectivity, int off[13][3]) {   // connectivity 1..3
  int k = 0;
  for (int dz = 0; dz <= 1; dz++)
    for (int dy = -1; dy <= 1; dy++)
      for (int dx = -1; dx <= 1; dx++) {
        if (dx * dx + dy * dy + dz * dz > connectivity) continue;
        if (dz == 0 && (dy < 0 || (dy == 0 && dx <= 0))) continue;
        off[k][0] = dx; off[k][1] = dy; off[k][2] = dz;
        k++;
      }
  return k;
}

// the value the reference's TraceProductSym3 returns (connect.cpp's header comment)
VH_CG_HD float trace_product(const float* a, const float* b) {
  return a[0] * b[0] + a[0] * b[1] + a[1] * b[2] + a[1] * b[0] + a[1] * b[1] + a[2] * b[2] + a[2] * b[1] + a[2] * b[2] +
         a[0] * b[0];
}
VH_CG_HD float frobenius(const float* a) { return sqrtf(trace_product(a, a)); }   // correctly rounded on both sides
VH_CG_HD float dot3(const float* a, const float* b) { return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]; }
VH_CG_HD float sqr(float x) { return x * x; }

// visfd_utils.hpp:528-616 as connect.cpp's hessian_fd has it, flat (xx, yy, zz, xy, yz, xz), with the sign flip of the pop loop
VH_CG_HD void hessian6(const Params& p, const float* S, int ix, int iy, int iz, float H[6]) {
  if (ix == 0) ix++; else if (ix == p.nx - 1) ix--;
  if (iy == 0) iy++; else if (iy == p.ny - 1) iy--;
  if (iz == 0) iz++; else if (iz == p.nz - 1) iz--;
  const int64_t sy = p.nx, sz = (int64_t)p.nx * p.ny;
  const float* c = S + ((int64_t)iz * p.ny + iy) * p.nx + ix;
#define VH_CG_S(dx, dy, dz) c[(dx) + (dy) * sy + (dz) * sz]
  H[0] = (VH_CG_S(1, 0, 0) + VH_CG_S(-1, 0, 0) - 2 * VH_CG_S(0, 0, 0));
  H[1] = (VH_CG_S(0, 1, 0) + VH_CG_S(0, -1, 0) - 2 * VH_CG_S(0, 0, 0));
  H[2] = (VH_CG_S(0, 0, 1) + VH_CG_S(0, 0, -1) - 2 * VH_CG_S(0, 0, 0));
  H[3] = (float)(0.25 * (VH_CG_S(1, 1, 0) + VH_CG_S(-1, -1, 0) - VH_CG_S(1, -1, 0) - VH_CG_S(-1, 1, 0)));
  H[4] = (float)(0.25 * (VH_CG_S(0, 1, 1) + VH_CG_S(0, -1, -1) - VH_CG_S(0, 1, -1) - VH_CG_S(0, -1, 1)));
  H[5] = (float)(0.25 * (VH_CG_S(1, 0, 1) + VH_CG_S(-1, 0, -1) - VH_CG_S(-1, 0, 1) - VH_CG_S(1, 0, -1)));
#undef VH_CG_S
  if (p.flip_hessian)
    for (int k = 0; k < 6; k++) H[k] *= -1.0f;
}

// threshold and mask: the two tests that need nothing but the voxel's own words (NaNs behave as in the flood)
VH_CG_HD bool passes_threshold(const Params& p, const float* S, const float* M, int64_t i) {
  if (S[i] * p.SIGN > p.thr * p.SIGN) return false;
  return !(M && M[i] == 0.0f);
}
VH_CG_HD bool passes_tensor(const Params& p, const float H[6], const float* t) {
  return !(trace_product(H, t) < p.tts * frobenius(H) * frobenius(t));
}

// the neighbour test as the flood evaluates it when voxel i is popped and looks at its unmasked neighbour j
VH_CG_HD bool passes_neighbour(const Params& p, const float* T, const float* V, int64_t i, int64_t j) {
  if (!T) return true;   // both tests sit under "if tensor" (connect.hpp:625-672)
  const float* ti = T + 6 * i;
  const float* tj = T + 6 * j;
  if (trace_product(ti, tj) < (p.ttn * frobenius(ti) * frobenius(tj))) return false;
  if (V) {
    const float* vi = V + 3 * i;
    const float* vj = V + 3 * j;
    if (p.signs) {   // quirk kept: the signed form uses the tensor threshold
      if (dot3(vi, vj) < (p.ttn * sqrtf(dot3(vi, vi)) * sqrtf(dot3(vj, vj)))) return false;
    } else {
      if (sqr(dot3(vi, vj)) < (sqr(p.tvn) * dot3(vi, vi) * dot3(vj, vj))) return false;
    }
  }
  return true;
}

// ---- host side (connect_graph_host.cpp) --------------------------------------------------------------------------------------

// the arguments of visfd_hip_label_connected_ex
struct Call {
  const float* saliency;
  int64_t* labels;
  const float* mask;
  int64_t nx, ny, nz;
  float threshold_saliency;
  float* direction;
  float threshold_vector_saliency, threshold_vector_neighbor;
  int consider_dot_product_sign;
  const float* tensor;
  float threshold_tensor_saliency, threshold_tensor_neighbor;
  int tensor_is_positive_definite_near_target, connectivity;
  int64_t label_undefined;
  int sort_by_size, standardize_directions, start_from_saliency_maxima;
  int64_t* n_clusters;
  float *cluster_maxima, *cluster_sizes, *cluster_saliencies;
  int64_t cluster_capacity;
  const float* voxel_weights;
  const float* must_link_crds;
  const int64_t* must_link_group_sizes;
  int64_t must_link_ngroups;
  const int* must_link_directions;
};

struct Last {   // what visfd_hip_label_connected_graph_last reports
  int path = -1;
  unsigned reasons = 0;
  int64_t n_valid = -1, n_undecided = -1;
};

Params make_params(const Call& c);
// MUST_LINK, WEIGHTS, LIMITS: what is known before any work starts (device: the seed search's limits too)
unsigned early_reasons(const Call& c, bool device);

// The vector test over a candidate list: H[k][6] (sign flip applied), v[k][3] -> bit k of pass[k / 32] (set: passes).
void vector_test(const Params& p, int order, const float* H, const float* v, int64_t count, unsigned* pass);

// Provisional numbering from the ranked seeds: seed_root[k] (the root of seed k's component, -1 where the seed is no valid
// voxel) -> prov_of_seed[k] (the component's number where seed k is its anchor, else -1) and `deepest` (anchor rank by number).
void number_clusters(const std::vector<int>& seed_root, std::vector<int>* prov_of_seed, std::vector<int64_t>* deepest);

// From integer sizes: the final order (perm[k] = provisional number of final cluster k, inv its inverse) and the three
// per-cluster lists with the flood's deepest / perm quirk.  VISFD_HIP_ECAPACITY as the flood.
int finish_lists(const Call& c, const std::vector<int>& seed_index, const std::vector<float>& seed_score,
                 const std::vector<int64_t>& deepest, const std::vector<uint64_t>& sizes, std::vector<int64_t>* inv);

// the same from the flood's float sizes (voxel weights: the sizes are sums of weights)
int finish_lists(const Call& c, const std::vector<int>& seed_index, const std::vector<float>& seed_score,
                 const std::vector<int64_t>& deepest, const std::vector<float>& sizes, std::vector<int64_t>* inv);

// ---- option connect_settle (device path only): what the host does from small arrays and from the labelled voxels -------------
// The must-link locations as the flood rounds them, three ints per location in group order.  LIMITS where a location is
// 2^20 voxels or more from the origin or could be 2^33 squared voxels or more from a voxel of the image: the device's
// search key is (squared distance << 31) | voxel index.
unsigned link_locations(const Call& c, std::vector<int>* want);

struct LinkContact {   // the labelled voxel nearest to a location
  int index;           // its voxel index
  int code;            // (provisional cluster << 1) | its sign relative to the cluster's anchor
  float n[3];          // its direction as it came in (zeros without directions)
};
// The flood's must-link block (connect.cpp) on cluster-level state: map[k] = (the provisional cluster that absorbed k, k
// itself where none did) << 1 | whether k's voxels are negated on top of their sign to k's anchor.  Returns ZERO_DOT
// where a contact's deciding quantity is a zero, which the flood reads by basin polarities the graph does not have.
unsigned merge_links(const Call& c, bool standardize, const std::vector<LinkContact>& contact, size_t n_clusters,
                     std::vector<int>* map);

struct SettleVoxel {   // one labelled voxel gathered by the device, in no order
  int index, cluster;
  float n[3];          // direction with the sign to the anchor (and a must-link's negation) applied
  float w;
};
// Orders the voxels by index and runs the flood's own statements over them (connect_host.hpp: cluster_moments).
void settle_moments(const Call& c, std::vector<SettleVoxel>* voxels, size_t n_clusters, bool weighted, bool standardize,
                    std::vector<long double>* sizes, std::vector<long double>* sum_dot);

// The flood (connect.cpp) for a call whose result the pop order decides, the contract of the graph entries kept: the
// directions of voxels that end up unlabelled or are masked are put back to their input bits.  seed_index / seed_score: the
// ranked seeds where they are known already (both or neither).
int flood_keeping_unlabelled(const Call& c, const std::vector<int>* seed_index, const std::vector<float>* seed_score);

// the serial walk of the definition; *last says what it did
int host_walk(const Call& c, Last* last);
Last& host_last();   // the calling thread's last successful visfd_hip_label_connected_graph_host

}  // namespace cg
}  // namespace vh
