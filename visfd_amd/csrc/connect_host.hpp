// connect_host.hpp -- the sequential flood of LabelConnected (connect.cpp) as connect_seeds.hip calls it.
#pragma once

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <thread>
#include <vector>

namespace vh {

// null image, dimensions below 3 or too large for 32-bit voxel indices, connectivity < 1: VISFD_HIP_EINVAL
int label_connected_check_args(const float* saliency, const int64_t* labels, int64_t nx, int64_t ny, int64_t nz,
                               int connectivity);

// visfd_hip_label_connected_ex (include/visfd_hip.h) on host arrays.  given_index / given_score (both or neither): the
// seeds -- the plateau-aware extrema of the saliency that pass the threshold, as voxel indices and values in the
// reference's ranked order -- when the caller has found them already; otherwise the flood searches them itself.
int host_label_connected(const float* saliency, int64_t* labels, const float* mask, int64_t nx, int64_t ny, int64_t nz,
                         float threshold_saliency, float* direction, float threshold_vector_saliency,
                         float threshold_vector_neighbor, int consider_dot_product_sign, const float* tensor,
                         float threshold_tensor_saliency, float threshold_tensor_neighbor,
                         int tensor_is_positive_definite_near_target, int connectivity, int64_t label_undefined,
                         int sort_by_size, int standardize_directions, int start_from_saliency_maxima,
                         int64_t* n_clusters, float* cluster_maxima, float* cluster_sizes, float* cluster_saliencies,
                         int64_t cluster_capacity, const float* voxel_weights, const float* must_link_crds,
                         const int64_t* must_link_group_sizes, int64_t must_link_ngroups, const int* must_link_directions,
                         const std::vector<int>* given_index, const std::vector<float>* given_score);

// the ranked seed list the flood would search for itself (plateau-aware extrema that pass the threshold)
void host_find_seeds(const float* saliency, const float* mask, int64_t nx, int64_t ny, int64_t nz, bool seek_minima,
                     float threshold, int connectivity, std::vector<int>* index, std::vector<float>* score);

// connect.cpp: the host finish of the device path of the surface points (surface_points.hip).  Per walked point k,
// rec[9k..] holds the Hessian (xx, yy, zz, xy, yz, xz) and the gradient of the saliency at round(xyz[3k..]).  Runs the
// ridge snap of visfd_hip_surface_points (the same text) on each, compacts xyz / nrm in place with the order kept, and
// returns the number of points that stay.
int64_t host_surface_ridge_finish(float* xyz, float* nrm, const float* rec, int64_t n, const int size[3],
                                  const float voxel_width[3], float max_distance_to_feature);

// ---- text that the flood (connect.cpp) and the settle paths of the graph entries (connect_graph_host.cpp) both run, so
// that the two cannot drift apart: every statement below is the flood's, operand order and types kept.

// The must-link contact test (connect.hpp:940-1010): from the two contact voxels' directions and positions, the quantity
// that decides whether they face compatibly, and the rule it is read by (must_link_match).  how: 0 same, 1 opposite,
// 2 inferred from the angles the normals make with the line that joins the voxels.
inline int must_link_decider(const float* n_i, const float* n_j, const int ri[3], const int rj[3], int how, float* value) {
  const float dot_ij = n_i[0] * n_j[0] + n_i[1] * n_j[1] + n_i[2] * n_j[2];
  if (how == 0) { *value = dot_ij; return 0; }
  if (how == 1) { *value = dot_ij; return 1; }
  float r_ij[3] = {(float)(ri[0] - rj[0]), (float)(ri[1] - rj[1]), (float)(ri[2] - rj[2])};
  {   // Normalize3 (lin3_utils.hpp:143-155)
    const float len = std::sqrt(r_ij[0] * r_ij[0] + r_ij[1] * r_ij[1] + r_ij[2] * r_ij[2]);
    if (len > 0) { const float inv = (float)(1.0 / (double)len); for (int d = 0; d < 3; d++) r_ij[d] *= inv; }
    else { r_ij[0] = 1.0f; r_ij[1] = 0.0f; r_ij[2] = 0.0f; }
  }
  const float ni_dot_rij = n_i[0] * r_ij[0] + n_i[1] * r_ij[1] + n_i[2] * r_ij[2];
  const float nj_dot_rij = n_j[0] * r_ij[0] + n_j[1] * r_ij[1] + n_j[2] * r_ij[2];
  const float theta0 = (float)(M_PI / 4);
  const float theta_i = std::asin(std::abs(ni_dot_rij)), theta_j = std::asin(std::abs(nj_dot_rij));
  if (theta_i < theta0 && theta_j < theta0) { *value = dot_ij; return 0; }
  *value = ni_dot_rij * nj_dot_rij;
  return 2;
}
inline bool must_link_match(int rule, float value) { return rule == 0 ? value > 0 : rule == 1 ? value < 0 : value <= 0; }

// Cluster sizes and outward sums (connect.hpp:1154-1290).  walk(f) calls f(x, y, z, k, n, w) for every labelled voxel in
// raster order: its position, cluster, direction (three floats, polarity applied; null where not standardising) and
// weight (looked at only when `weighted`).  sizes[k]: the number of voxels or the sum of their weights; with
// `standardize`, sum_dot[k]: the sum of (r - r_com) . n whose sign decides the outward flip.  A cluster whose weights
// sum to zero gets the centre of mass 0 / 0 and a sum that is not below zero, here as in the reference.
template <typename Walk>
void cluster_moments(Walk walk, size_t n_clusters, bool weighted, bool standardize, std::vector<long double>* sizes_out,
                     std::vector<long double>* sum_dot_out) {
  std::vector<long double> sizes(n_clusters, 0.0L);
  walk([&](int, int, int, int64_t k, const float*, float w) { sizes[(size_t)k] += weighted ? (long double)w : 1.0L; });
  std::vector<long double> sum_dot(n_clusters, 0.0L);
  if (standardize) {
    std::vector<long double> com(3 * n_clusters, 0.0L);
    walk([&](int x, int y, int z, int64_t k, const float*, float w) {
      if (weighted) {   // connect.hpp:1211-1224: int * float products in float, summed in long double
        com[3 * (size_t)k] += x * w; com[3 * (size_t)k + 1] += y * w; com[3 * (size_t)k + 2] += z * w;
      } else {
        com[3 * (size_t)k] += x; com[3 * (size_t)k + 1] += y; com[3 * (size_t)k + 2] += z;
      }
    });
    for (size_t k = 0; k < n_clusters; k++)
      for (int d = 0; d < 3; d++) com[3 * k + d] /= sizes[k];
    walk([&](int x, int y, int z, int64_t k, const float* n, float w) {
      const float r[3] = {(float)(x - com[3 * (size_t)k]), (float)(y - com[3 * (size_t)k + 1]), (float)(z - com[3 * (size_t)k + 2])};
      long double delta_sum = (long double)(r[0] * n[0] + r[1] * n[1] + r[2] * n[2]);
      if (weighted) delta_sum *= w;
      sum_dot[(size_t)k] += delta_sum;
    });
  }
  sizes_out->swap(sizes);
  sum_dot_out->swap(sum_dot);
}

// work(lo, hi) over [0, nvox) split across the host's cores, 16 threads at the most (independent voxels only)
template <typename F>
void parallel_voxels(int64_t nvox, F work) {
  unsigned nt = std::thread::hardware_concurrency();
  if (nt < 1) nt = 1;
  if (nt > 16) nt = 16;
  if ((int64_t)nt > nvox / 4096 + 1) nt = (unsigned)(nvox / 4096 + 1);
  std::vector<std::thread> pool;
  const int64_t chunk = (nvox + nt - 1) / nt;
  for (unsigned t = 1; t < nt; t++)
    pool.emplace_back(work, std::min<int64_t>(nvox, t * chunk), std::min<int64_t>(nvox, (t + 1) * chunk));
  work(0, std::min<int64_t>(nvox, chunk));
  for (size_t t = 0; t < pool.size(); t++) pool[t].join();
}

}  // namespace vh
