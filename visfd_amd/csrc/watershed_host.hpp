// watershed_host.hpp -- the sequential watershed (watershed_host.cpp).  Plain C++: no HIP, no context, so that the flood
// can also be built into a stand-alone program.
#pragma once

#include <cstdint>
#include <string>
#include <vector>

namespace vh {

struct WatershedArgs {
  const float* src;
  const float* mask;          // nullable
  const int32_t* markers;     // nullable
  int64_t nx, ny, nz;
  float halt_threshold;
  int start_from_minima, connectivity, show_boundaries;
  int32_t label_boundary, label_undefined;
  int32_t* labels;
  int64_t* basin_index;       // the lists: host arrays on every face, each nullable
  float* basin_score;
  int64_t basin_cap;
  int64_t* n_basins;
};

// The reference's Meyer flood (lib/visfd/segmentation.hpp:65-559) on host arrays, from the image's own minima or maxima or
// from markers.  Writes a.labels (every voxel), the basin lists under the capacity protocol and *a.n_basins; the
// arguments have been checked (watershed_check_args).  Returns a VISFD_HIP_* code; on failure *err says why and labels
// is untouched.
int host_watershed(const WatershedArgs& a, std::string* err);

// true when a voxel with mask != 0 holds a NaN
bool host_any_unmasked_nan(const float* src, const float* mask, int64_t n);

}  // namespace vh
