// connect_host.hpp -- the sequential flood of LabelConnected (connect.cpp) as connect_seeds.hip calls it.
#pragma once

#include <algorithm>
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
