// connect_seeds.hip -- LabelConnected (reference lib/visfd/connect.hpp:168-1427) with its seed search on the device.
//
// This file holds no kernel of its own and does NOT move the flood to the device.  LabelConnected is two things in a row:
// a search of the whole image for its seeds -- the plateau-aware local maxima (or minima) of the saliency,
// lib/visfd/morphology_implementation.hpp:57-515 -- and a priority flood from those seeds over the few per cent of voxels
// that pass the threshold.  The search looks at every voxel and all of its neighbours and has no order in it; it is what
// extrema.hip already computes, root voxels, values, ranking and ties included.  The entry point here stages saliency
// and mask, takes the ranked list from those kernels and hands it to the sequential flood of connect.cpp; labels, lists
// and directions are connect.cpp's, bit for bit.  DESIGN.md 4.13 says what stands between the flood and a device.
//
// connect.cpp's own search is used where extrema.hip does not reach: connectivity above 3, or an image beyond
// VISFD_HIP_EXTREMA_MAX_VOXELS / _MAX_NY_NZ / 2^24 - 1 tiles.  visfd_hip_label_connected_device_seeds_last says which ran.
#include <limits>

#include "common.hpp"
#include "connect_host.hpp"
#include "tile.hpp"

namespace vh {
namespace {

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

bool search_fits_device(const Call& c) {
  return c.connectivity <= VISFD_HIP_EXTREMA_MAX_CONNECTIVITY && c.nx * c.ny * c.nz <= VISFD_HIP_EXTREMA_MAX_VOXELS &&
         c.ny <= VISFD_HIP_EXTREMA_MAX_NY_NZ && c.nz <= VISFD_HIP_EXTREMA_MAX_NY_NZ &&
         tile_count(c.nx, c.ny, c.nz) < ((i64)1 << 24);
}

// c's arrays on the host; dev_saliency / dev_mask: the same image on the device (null: the host search)
int flood(visfd_hip_ctx* ctx, const Call& c, const float* dev_saliency, const float* dev_mask) {
  std::vector<int> index;
  std::vector<float> score;
  const bool on_device = dev_saliency != nullptr;
  if (on_device) {
    const bool minima = c.start_from_saliency_maxima == 0;
    float thr = c.threshold_saliency;   // morphology_implementation.hpp:774-775: no threshold for maxima is -infinity
    if (!minima && thr == std::numeric_limits<float>::infinity()) thr = -std::numeric_limits<float>::infinity();
    VH_TRY(dev_extrema_seeds(ctx, dev_saliency, dev_mask, c.nx, c.ny, c.nz, minima, thr, c.connectivity, &index, &score));
  }
  VH_TRY(host_label_connected(c.saliency, c.labels, c.mask, c.nx, c.ny, c.nz, c.threshold_saliency, c.direction,
                              c.threshold_vector_saliency, c.threshold_vector_neighbor, c.consider_dot_product_sign,
                              c.tensor, c.threshold_tensor_saliency, c.threshold_tensor_neighbor,
                              c.tensor_is_positive_definite_near_target, c.connectivity, c.label_undefined, c.sort_by_size,
                              c.standardize_directions, c.start_from_saliency_maxima, c.n_clusters, c.cluster_maxima,
                              c.cluster_sizes, c.cluster_saliencies, c.cluster_capacity, c.voxel_weights, c.must_link_crds,
                              c.must_link_group_sizes, c.must_link_ngroups, c.must_link_directions,
                              on_device ? &index : nullptr, on_device ? &score : nullptr));
  ctx->connect_seeds[0] = on_device ? VISFD_HIP_CONNECT_SEEDS_DEVICE : VISFD_HIP_CONNECT_SEEDS_HOST;
  ctx->connect_seeds[1] = on_device ? (int64_t)index.size() : -1;
  return VISFD_HIP_OK;
}

}  // namespace
}  // namespace vh

using namespace vh;

extern "C" {

int visfd_hip_label_connected_device_seeds(visfd_hip_ctx* ctx, const float* saliency, int64_t* labels, const float* mask,
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
                                           const int* must_link_directions) {
  VH_REQUIRE(ctx, "null context");
  VH_TRY(label_connected_check_args(saliency, labels, nx, ny, nz, connectivity));   // before any allocation
  const Call c = {saliency, labels, mask, nx, ny, nz, threshold_saliency, direction, threshold_vector_saliency,
                  threshold_vector_neighbor, consider_dot_product_sign, tensor, threshold_tensor_saliency,
                  threshold_tensor_neighbor, tensor_is_positive_definite_near_target, connectivity, label_undefined,
                  sort_by_size, standardize_directions, start_from_saliency_maxima, n_clusters, cluster_maxima,
                  cluster_sizes, cluster_saliencies, cluster_capacity, voxel_weights, must_link_crds, must_link_group_sizes,
                  must_link_ngroups, must_link_directions};
  if (!search_fits_device(c)) return flood(ctx, c, nullptr, nullptr);
  VH_HIP(hipSetDevice(ctx->device));
  const Stage st = {ctx, (size_t)(nx * ny * nz)};
  float *ds, *dm;
  VH_TRY(st.up(WS_H2D_0, saliency, &ds));
  VH_TRY(st.up(WS_H2D_1, mask, &dm));
  return flood(ctx, c, ds, dm);   // the search waits for the stream before it reads its lists
}

int visfd_hip_label_connected_device_seeds_last(visfd_hip_ctx* ctx, int* where, int64_t* n_seeds) {
  VH_REQUIRE(ctx && where, "null argument");
  *where = (int)ctx->connect_seeds[0];
  if (n_seeds) *n_seeds = ctx->connect_seeds[1];
  return VISFD_HIP_OK;
}

}  // extern "C"
