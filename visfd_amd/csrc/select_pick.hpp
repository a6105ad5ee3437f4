// select_pick.hpp -- the two host/device steps of the radix select (select.hip): the rank the reference reads, and the walk
// that picks one digit from a histogram.  Plain C++ (tests/select_pick_check.cpp compiles it with g++), __host__ __device__
// under hipcc: pick_kernel and the host walk of dev_threshold_fraction run THIS code and nothing else does (select_rank_check
// is select_rank's verdict before anything is queued).  The slab stage has no select of its own: it is pick_kernel on the
// ranks' summed counters.
#pragma once

#include <cmath>
#include <cstdint>

#if defined(__HIPCC__)
#define VH_SELECT_HD __host__ __device__
#else
#define VH_SELECT_HD
#endif

namespace vh {

// i = floor(n_voxels * fraction): size_t -> float, a single-precision product (handlers.cpp:1781).  False where the
// reference would read past its array (no voxel, or i >= n).
VH_SELECT_HD inline bool select_rank(uint64_t n, float fraction, uint64_t* k) {
  const float prod = (float)n * fraction;
  *k = (uint64_t)floorf(prod);
  return n != 0 && *k < n;
}

// Walk a histogram of `nbins` counters from the largest key down; returns the bin holding the k-th largest (0-based)
// element and rewrites k to the rank inside that bin; -1 if the counters hold no more than k elements.
VH_SELECT_HD inline int select_pick_bin(const uint64_t* h, int nbins, uint64_t* k) {
  uint64_t seen = 0;
  for (int b = nbins - 1; b >= 0; b--) {
    if (seen + h[b] > *k) { *k -= seen; return b; }
    seen += h[b];
  }
  return -1;
}

}  // namespace vh
