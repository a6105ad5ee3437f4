// watershed_host.cpp -- the reference's watershed on the host, statement for statement: Meyer's flood from a priority queue
// (lib/visfd/segmentation.hpp:220-549), seeded with the image's own minima or maxima (_FindExtrema with borders allowed)
// or with the caller's markers (:155-199).  It is the only path for markers -- whole lakes then flood downhill in heap
// order, which is serial -- and the cross-check of the kernels in watershed.hip (option watershed_host).
//
// The queue is keyed on (-s, basin, x, y, z) with s = SIGN * value and has no insertion counter, so its order depends on
// its contents only.  The reference carries the basin through a float on the way out of the queue (:334); with at most
// 2^24 basins, which the caller has checked, that changes nothing and integers are used here.  Nothing in this file needs
// a device or the library's context.
#include "watershed_host.hpp"

#include <algorithm>
#include <array>
#include <cmath>
#include <limits>
#include <map>
#include <queue>
#include <set>
#include <tuple>

#include "../../include/visfd_hip.h"

namespace vh {

namespace {

typedef int64_t i64;

struct Offsets {
  std::vector<std::array<int, 3> > d;   // (dx, dy, dz), dz outermost as the reference builds them (:97-112)
  explicit Offsets(int connectivity) {
    const int r = (int)std::floor(std::sqrt((double)connectivity));
    for (int jz = -r; jz <= r; jz++)
      for (int jy = -r; jy <= r; jy++)
        for (int jx = -r; jx <= r; jx++) {
          if ((jx == 0 && jy == 0 && jz == 0) || jx * jx + jy * jy + jz * jz > connectivity) continue;
          d.push_back({{jx, jy, jz}});
        }
  }
};

// Seeds of the unmarked case: the roots (first voxels in raster order) of the plateaus that are minima (maxima) and pass
// the threshold, ascending in (value, raster position), reversed for maxima (morphology_implementation.hpp:57-515).
void plateau_seeds(const WatershedArgs& a, const Offsets& nb, std::vector<i64>* index, std::vector<float>* score) {
  const int nx = (int)a.nx, ny = (int)a.ny, nz = (int)a.nz;
  const i64 n = a.nx * a.ny * a.nz;
  const bool minima = a.start_from_minima != 0;
  std::vector<unsigned char> seen((size_t)n, 0);
  std::vector<i64> plateau;
  std::vector<std::pair<float, i64> > found;   // (value, root)
  for (i64 c0 = 0; c0 < n; c0++) {
    if ((a.mask && a.mask[c0] == 0.0f) || seen[(size_t)c0]) continue;
    bool extremum = true;
    plateau.assign(1, c0);
    seen[(size_t)c0] = 1;
    const float v = a.src[c0];
    for (size_t head = 0; head < plateau.size(); head++) {
      const i64 c = plateau[head];
      const int x = (int)(c % nx), y = (int)((c / nx) % ny), z = (int)(c / ((i64)nx * ny));
      for (size_t j = 0; j < nb.d.size(); j++) {
        const int xx = x + nb.d[j][0], yy = y + nb.d[j][1], zz = z + nb.d[j][2];
        if (xx < 0 || xx >= nx || yy < 0 || yy >= ny || zz < 0 || zz >= nz) continue;
        const i64 cj = ((i64)zz * ny + yy) * nx + xx;
        if (a.mask && a.mask[cj] == 0.0f) continue;
        const float vj = a.src[cj];
        if (vj == v) {
          if (!seen[(size_t)cj]) {
            seen[(size_t)cj] = 1;
            plateau.push_back(cj);
          }
        } else if (minima ? vj < v : vj > v) {
          extremum = false;
        }
      }
    }
    if (extremum && (minima ? v <= a.halt_threshold : v >= a.halt_threshold)) found.push_back(std::make_pair(v, c0));
  }
  std::sort(found.begin(), found.end(), [](const std::pair<float, i64>& p, const std::pair<float, i64>& q) {
    if (p.first < q.first) return true;
    if (q.first < p.first) return false;
    return p.second < q.second;
  });
  if (!minima) std::reverse(found.begin(), found.end());
  for (size_t k = 0; k < found.size(); k++) {
    index->push_back(found[k].second);
    score->push_back(found[k].first);
  }
}

}  // namespace

bool host_any_unmasked_nan(const float* src, const float* mask, int64_t n) {
  for (i64 i = 0; i < n; i++)
    if (src[i] != src[i] && !(mask && mask[i] == 0.0f)) return true;
  return false;
}

int host_watershed(const WatershedArgs& a, std::string* err) {
  const int nx = (int)a.nx, ny = (int)a.ny, nz = (int)a.nz;
  const i64 n = a.nx * a.ny * a.nz;
  const Offsets nb(a.connectivity);
  const float SIGN = a.start_from_minima ? 1.0f : -1.0f;
  const float halt = a.halt_threshold * SIGN;
  const i64 WATERSHED_BOUNDARY = 0, UNDEFINED = -1;

  std::vector<i64> seed;
  std::vector<float> seed_score;
  i64 max_label = 0;
  if (a.markers) {   // :155-199: the first voxel of each distinct positive label, in raster order
    std::set<i64> so_far;
    for (i64 c = 0; c < n; c++) {
      if (a.mask && a.mask[c] == 0.0f) continue;
      const i64 label = a.markers[c];
      if (label > 0 && so_far.insert(label).second) {
        max_label = std::max(max_label, label);
        seed.push_back(c);
        seed_score.push_back(a.src[c]);
      }
    }
  } else {
    plateau_seeds(a, nb, &seed, &seed_score);
    max_label = (i64)seed.size();
  }
  const i64 nseeds = (i64)seed.size();
  if (a.n_basins) *a.n_basins = nseeds;
  if (nseeds > VISFD_HIP_WATERSHED_MAX_BASINS) {
    *err = "watershed: more than 2^24 basins (the reference's labels are not exact beyond that)";
    return VISFD_HIP_EINVAL;
  }
  if (a.basin_cap > 0 && a.basin_cap < nseeds) {
    *err = "watershed: the basin list is too small";
    return VISFD_HIP_ECAPACITY;
  }
  if (a.basin_cap > 0)
    for (i64 k = 0; k < nseeds; k++) {
      if (a.basin_index) a.basin_index[k] = seed[(size_t)k];
      if (a.basin_score) a.basin_score[k] = seed_score[(size_t)k];
    }

  const i64 QUEUED = max_label + 1;
  std::vector<i64> dest((size_t)n, UNDEFINED);
  typedef std::tuple<float, i64, std::array<int, 3> > Entry;
  std::priority_queue<Entry> q;
  for (i64 k = 0; k < nseeds; k++) {
    const i64 c = seed[(size_t)k];
    const std::array<int, 3> at = {{(int)(c % nx), (int)((c / nx) % ny), (int)(c / ((i64)nx * ny))}};
    q.push(Entry(-(seed_score[(size_t)k] * SIGN), k, at));
    dest[(size_t)c] = QUEUED;
  }
  while (!q.empty()) {
    const Entry p = q.top();
    q.pop();
    const float score = -std::get<0>(p);
    const i64 basin = std::get<1>(p);
    const int x = std::get<2>(p)[0], y = std::get<2>(p)[1], z = std::get<2>(p)[2];
    const i64 c = ((i64)z * ny + y) * nx + x;
    if (score > halt || (a.mask && a.mask[c] == 0.0f)) {
      dest[(size_t)c] = UNDEFINED;
      continue;
    }
    dest[(size_t)c] = basin + 1;
    for (size_t j = 0; j < nb.d.size(); j++) {
      const int xx = x + nb.d[j][0], yy = y + nb.d[j][1], zz = z + nb.d[j][2];
      if (zz < 0 || zz >= nz || yy < 0 || yy >= ny || xx < 0 || xx >= nx) continue;
      const i64 cj = ((i64)zz * ny + yy) * nx + xx;
      if (a.mask && a.mask[cj] == 0.0f) continue;
      const i64 dj = dest[(size_t)cj];
      if (dj == WATERSHED_BOUNDARY || dj == QUEUED) continue;
      if (dj == UNDEFINED) {
        dest[(size_t)cj] = QUEUED;
        const std::array<int, 3> at = {{xx, yy, zz}};
        q.push(Entry(-(a.src[cj] * SIGN), basin, at));
      } else if (dj != dest[(size_t)c] && a.show_boundaries) {
        dest[(size_t)c] = WATERSHED_BOUNDARY;   // the later of two voxels of different basins, the shallower one
      }
    }
  }

  const i64 label_boundary = a.label_boundary, label_undefined = a.label_undefined;
  if (label_boundary != WATERSHED_BOUNDARY)
    for (i64 c = 0; c < n; c++)
      if (!(a.mask && a.mask[c] == 0.0f) && dest[(size_t)c] == WATERSHED_BOUNDARY) dest[(size_t)c] = label_boundary;
  if (label_undefined != UNDEFINED)
    for (i64 c = 0; c < n; c++)
      if (!(a.mask && a.mask[c] == 0.0f) && dest[(size_t)c] == UNDEFINED) dest[(size_t)c] = label_undefined;
  if (a.markers) {   // :519-549: basin numbers back to the caller's labels; the first scan reads masked voxels too
    std::map<i64, i64> old2new;
    for (i64 c = 0; c < n; c++) {
      const i64 label_old = dest[(size_t)c], label_new = a.markers[c];
      if (label_new > 0 && label_old != label_boundary && label_old != label_undefined) old2new[label_old] = label_new;
    }
    for (i64 c = 0; c < n; c++) {
      if (a.mask && a.mask[c] == 0.0f) continue;
      const i64 d = dest[(size_t)c];
      if (d == label_boundary || d == label_undefined) continue;
      const std::map<i64, i64>::const_iterator it = old2new.find(d);
      dest[(size_t)c] = it != old2new.end() ? it->second : label_undefined;
    }
  }
  for (i64 c = 0; c < n; c++) a.labels[c] = (int32_t)dest[(size_t)c];
  return VISFD_HIP_OK;
}

}  // namespace vh
