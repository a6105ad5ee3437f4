// blob_post.cpp -- blob list post-processing: sorting by score, discarding blobs
// whose centres are masked out, greedy non-max suppression of overlapping blobs, and (second half of the file) the score
// thresholds chosen from training points.
//
// These are short sequential host algorithms in the reference as well (lib/visfd/feature.hpp:519-616,
// :720-913, :924-969; sphere overlap lib/visfd/visfd_utils.hpp:95-118); the greedy suppression's
// result depends on the visiting order and on WHICH earlier blobs a blob is compared with, so both
// are reproduced exactly:
//   * order: blobs are ranked by (key, original index) tuples, key = score or |score|, ascending,
//     or the exact reverse of that ranking for descending (so ties then go to the LARGER index);
//   * candidates: a kept blob k is compared with blob i only if the two meet in a coarse occupancy
//     grid (cell = `scale` voxels; a blob occupies the cells within ceil(r/scale)+1 of its centre
//     cell).  The grid origin/extents come from integer-truncated bounds of all blobs.
// Arithmetic types follow the reference expression by expression (float unless a double constant
// such as M_PI enters; see each line).
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <limits>
#include <utility>
#include <vector>

#include "common.hpp"

namespace {

using vh::i64;

// lib/visfd/visfd_utils.hpp:95-118 (Scalar = float; constants with M_PI are double)
float sphere_overlap(float rij, float Ri, float Rj) {
  if (Ri > Rj) std::swap(Ri, Rj);
  if (rij <= Ri) return (float)((4 * M_PI / 3) * Ri * Ri * Ri);  // (double * float) * float * float
  const float xi = (float)(0.5 * (1.0 / rij) * (rij * rij + Ri * Ri - Rj * Rj));
  const float xj = (float)(0.5 * (1.0 / rij) * (rij * rij + Rj * Rj - Ri * Ri));
  const float qi = xi / Ri, qj = xj / Rj;
  const float ti = Ri * Ri * Ri * (2 - qi * (3 - qi * qi));
  const float tj = Rj * Rj * Rj * (2 - qj * (3 - qj * qj));
  return (float)((M_PI / 3) * (ti + tj));
}

// Ranking of lib/visfd/feature.hpp:519-616: returns order[] with order[rank] = original index.
void rank_blobs(const float* scores, i64 n, int criteria, bool ascending_order, std::vector<i64>* order) {
  bool ascending = ascending_order, magnitude = false;
  switch (criteria) {
    case VISFD_HIP_SORT_DECREASING: break;
    case VISFD_HIP_SORT_INCREASING: ascending = !ascending; break;
    case VISFD_HIP_SORT_DECREASING_MAGNITUDE: magnitude = true; break;
    case VISFD_HIP_SORT_INCREASING_MAGNITUDE: magnitude = true; ascending = !ascending; break;
    default: break;
  }
  std::vector<std::pair<float, i64> > key((size_t)n);
  for (i64 i = 0; i < n; i++) key[(size_t)i] = std::make_pair(magnitude ? std::fabs(scores[i]) : scores[i], i);
  std::sort(key.begin(), key.end());                  // (key, index) lexicographic
  if (!ascending) std::reverse(key.begin(), key.end());  // == sorting through reverse iterators
  order->resize((size_t)n);
  for (i64 i = 0; i < n; i++) (*order)[(size_t)i] = key[(size_t)i].second;
}

void permute(const std::vector<i64>& order, float* crds, float* diameters, float* scores) {
  const size_t n = order.size();
  std::vector<float> c(crds, crds + 3 * n), d(diameters, diameters + n), s(scores, scores + n);
  for (size_t i = 0; i < n; i++) {
    const size_t j = (size_t)order[i];
    crds[3 * i] = c[3 * j]; crds[3 * i + 1] = c[3 * j + 1]; crds[3 * i + 2] = c[3 * j + 2];
    diameters[i] = d[j];
    scores[i] = s[j];
  }
}

}  // namespace

extern "C" {

float visfd_hip_sphere_overlap(float rij, float ri, float rj) { return sphere_overlap(rij, ri, rj); }

int visfd_hip_sort_blobs(float* crds, float* diameters, float* scores, int64_t n, int sort_criteria,
                         int ascending_order, uint64_t* permutation) {
  if (n < 0 || (n > 0 && (!crds || !diameters || !scores))) return vh::fail(VISFD_HIP_EINVAL, "sort_blobs: null list");
  if (sort_criteria == VISFD_HIP_DO_NOT_SORT) {   // the reference's dispatcher falls through: nothing happens
    return VISFD_HIP_OK;
  }
  if (sort_criteria < 0 || sort_criteria > VISFD_HIP_SORT_INCREASING_MAGNITUDE)
    return vh::fail(VISFD_HIP_EINVAL, "sort_blobs: unknown sort criteria");
  if (n == 0) return VISFD_HIP_OK;
  std::vector<i64> order;
  rank_blobs(scores, n, sort_criteria, ascending_order != 0, &order);
  if (permutation)
    for (i64 i = 0; i < n; i++) permutation[i] = (uint64_t)order[(size_t)i];
  permute(order, crds, diameters, scores);
  return VISFD_HIP_OK;
}

int visfd_hip_discard_masked_blobs(float* crds, float* diameters, float* scores, int64_t* n_inout,
                                   const float* mask, int64_t nx, int64_t ny, int64_t nz) {
  if (!n_inout || *n_inout < 0) return vh::fail(VISFD_HIP_EINVAL, "discard_masked_blobs: bad count");
  if (!mask) return VISFD_HIP_OK;   // feature.hpp:951: nothing is discarded without a mask
  const i64 n = *n_inout;
  i64 kept = 0;
  for (i64 i = 0; i < n; i++) {
    // centre voxel = floor(x + 0.5) evaluated in double (feature.hpp:948-950)
    const i64 ix = (i64)std::floor((double)crds[3 * i] + 0.5);
    const i64 iy = (i64)std::floor((double)crds[3 * i + 1] + 0.5);
    const i64 iz = (i64)std::floor((double)crds[3 * i + 2] + 0.5);
    if (ix < 0 || ix >= nx || iy < 0 || iy >= ny || iz < 0 || iz >= nz)
      return vh::fail(VISFD_HIP_EINVAL, "discard_masked_blobs: a blob centre lies outside the mask image");
    if (mask[(iz * ny + iy) * nx + ix] == 0.0f) continue;
    if (kept != i) {
      std::memmove(crds + 3 * kept, crds + 3 * i, 3 * sizeof(float));
      diameters[kept] = diameters[i];
      scores[kept] = scores[i];
    }
    kept++;
  }
  *n_inout = kept;
  return VISFD_HIP_OK;
}

int visfd_hip_discard_overlapping_blobs(float* crds, float* diameters, float* scores, int64_t* n_inout,
                                        float min_radial_separation_ratio, float max_volume_overlap_large,
                                        float max_volume_overlap_small, int sort_criteria, int scale) {
  if (!n_inout || *n_inout < 0) return vh::fail(VISFD_HIP_EINVAL, "discard_overlapping_blobs: bad count");
  if (scale < 1) return vh::fail(VISFD_HIP_EINVAL, "discard_overlapping_blobs: scale must be >= 1");
  const i64 n = *n_inout;
  if (n == 0) return VISFD_HIP_OK;
  // 1. best blobs first (feature.hpp:737-743: ascending_order = false)
  VH_TRY(visfd_hip_sort_blobs(crds, diameters, scores, n, sort_criteria, 0, nullptr));
  vh::overlap_walk_sorted(crds, diameters, scores, n_inout, nullptr, min_radial_separation_ratio, max_volume_overlap_large,
                          max_volume_overlap_small, scale);
  return VISFD_HIP_OK;
}

}  // extern "C"

// Steps 2 to 4 of DiscardOverlappingBlobs on a list that is sorted already.  `states` (nullable, one byte per blob) is
// what rounds on the device have decided so far (csrc/discard_overlap.hip): a kept blob enters the grid untested, a
// discarded one is skipped, an undecided one is tested as always.  Without states every blob is undecided.
void vh::overlap_walk_sorted(float* crds, float* diameters, float* scores, int64_t* n_inout, const unsigned char* states,
                             float min_radial_separation_ratio, float max_volume_overlap_large,
                             float max_volume_overlap_small, int scale) {
  const i64 n = *n_inout;
  // 2. integer bounds of all blobs (feature.hpp:756-768); float -> int conversions truncate
  int bmin[3] = {0, 0, 0}, bmax[3] = {-1, -1, -1};
  for (i64 i = 0; i < n; i++)
    for (int d = 0; d < 3; d++) {
      const float reff = std::ceil(diameters[i] / 2);
      const float c = crds[3 * i + d];
      if ((c - reff < (float)bmin[d]) || (bmin[d] > bmax[d])) bmin[d] = (int)(c - reff);
      if ((c + reff > (float)bmax[d]) || (bmin[d] > bmax[d])) bmax[d] = (int)(c + reff);
    }
  int tsz[3];
  for (int d = 0; d < 3; d++) tsz[d] = (1 + bmax[d] - bmin[d]) / scale;
  const bool has_grid = tsz[0] > 0 && tsz[1] > 0 && tsz[2] > 0;

  // 3. occupancy grid: for every cell the kept blobs (sorted positions) that reach it
  std::vector<std::vector<uint32_t> > cells(has_grid ? (size_t)tsz[0] * tsz[1] * tsz[2] : 0);
  std::vector<i64> keep;
  keep.reserve((size_t)n);
  for (i64 i = 0; i < n; i++) {
    const float reff_ = diameters[i] / 2;
    const float Reff_ = reff_ / scale;
    const int Reff = (int)std::ceil(Reff_) + 1;
    const int Reffsq = Reff * Reff;
    const float ix = crds[3 * i], iy = crds[3 * i + 1], iz = crds[3 * i + 2];
    const int C[3] = {(int)std::floor((ix - bmin[0]) / scale), (int)std::floor((iy - bmin[1]) / scale),
                      (int)std::floor((iz - bmin[2]) / scale)};
    const unsigned char state = states ? states[i] : (unsigned char)vh::OVERLAP_UNDECIDED;
    if (state == vh::OVERLAP_DISCARDED) continue;
    bool discard = false;
    auto for_cells = [&](auto&& fn) {   // the blob's cells inside the table, fn returns false to stop
      if (!has_grid) return;
      for (int Jz = -Reff; Jz <= Reff; Jz++) {
        const int z = C[2] + Jz;
        if (z < 0 || z >= tsz[2]) continue;
        for (int Jy = -Reff; Jy <= Reff; Jy++) {
          const int y = C[1] + Jy;
          if (y < 0 || y >= tsz[1]) continue;
          for (int Jx = -Reff; Jx <= Reff; Jx++) {
            const int x = C[0] + Jx;
            if (x < 0 || x >= tsz[0]) continue;
            if (Jx * Jx + Jy * Jy + Jz * Jz > Reffsq) continue;
            if (!fn(cells[((size_t)z * tsz[1] + y) * tsz[0] + x])) return;
          }
        }
      }
    };
    if (state != vh::OVERLAP_KEPT) for_cells([&](std::vector<uint32_t>& cell) {
      for (uint32_t k : cell) {
        const float kx = crds[3 * k], ky = crds[3 * k + 1], kz = crds[3 * k + 2];
        const float rik = std::sqrt((ix - kx) * (ix - kx) + (iy - ky) * (iy - ky) + (iz - kz) * (iz - kz));
        const float ri = diameters[i] / 2, rk = diameters[k] / 2;
        const float vol = sphere_overlap(rik, ri, rk);
        if (rik < (ri + rk) * min_radial_separation_ratio) discard = true;
        const float vi = (float)((4 * M_PI / 3) * (ri * ri * ri));
        const float vk = (float)((4 * M_PI / 3) * (rk * rk * rk));
        float v_large = vi, v_small = vk;
        if (vk > vi) { v_large = vk; v_small = vi; }
        if ((vol / v_small > max_volume_overlap_small) || (vol / v_large > max_volume_overlap_large)) discard = true;
      }
      return !discard;
    });
    if (discard) continue;
    keep.push_back(i);
    for_cells([&](std::vector<uint32_t>& cell) { cell.push_back((uint32_t)i); return true; });
  }
  // 4. compact the kept blobs (ascending positions: in place is safe)
  for (size_t j = 0; j < keep.size(); j++) {
    const i64 i = keep[j];
    if ((i64)j != i) {
      std::memmove(crds + 3 * j, crds + 3 * i, 3 * sizeof(float));
      diameters[j] = diameters[i];
      scores[j] = scores[i];
    }
  }
  *n_inout = (int64_t)keep.size();
}

// ---- the supervised score thresholds: visfd_utils.hpp:373-516, feature_implementation.hpp:48-457, feature.hpp:643-697,
//      :988-1180.  Short sequential host logic; the one search over (training point, blob) pairs is FindSpheres
//      (find_spheres.hip), on the device when a context is passed.
namespace {

// ChooseThreshold1D.  (score, index) tuples sorted ascending, or descending through reverse iterators (ties then go to
// the LARGER index first); the mistake count starts at Nn -- everything accepted -- and moves by one per datum; of the
// positions that reach the minimum the median entry is taken.
float choose_threshold_1d(const std::vector<float>& scores, const std::vector<unsigned char>& accepted, bool lower_bound) {
  const i64 N = (i64)scores.size();
  i64 Nn = 0;
  for (i64 i = 0; i < N; i++) Nn += accepted[(size_t)i] ? 0 : 1;
  const float SGN = lower_bound ? 1.0f : -1.0f;
  std::vector<std::pair<float, i64> > key((size_t)N);
  for (i64 i = 0; i < N; i++) key[(size_t)i] = std::make_pair(scores[(size_t)i], i);
  if (lower_bound) std::sort(key.begin(), key.end());
  else std::sort(key.rbegin(), key.rend());
  i64 min_mistakes = Nn, mistakes = Nn;
  for (i64 i = 0; i < N; i++) {
    mistakes += accepted[(size_t)key[(size_t)i].second] ? 1 : -1;
    if (mistakes < min_mistakes) min_mistakes = mistakes;
  }
  std::vector<i64> at_min;
  mistakes = Nn;
  for (i64 i = -1; i < N; i++) {
    if (i >= 0) mistakes += accepted[(size_t)key[(size_t)i].second] ? 1 : -1;
    if (mistakes == min_mistakes) at_min.push_back(i);
  }
  const i64 it = at_min[at_min.size() / 2];
  // the order of the two tests is the reference's: with N == 0 both hold and the first wins
  if (it == -1) return -SGN * std::numeric_limits<float>::infinity();
  if (it == N - 1) return SGN * std::numeric_limits<float>::infinity();
  // 0.5 * (a + b): the sum in float, the product with the double literal in double, stored as float
  return (float)(0.5 * (key[(size_t)it].first + key[(size_t)it + 1].first));
}

struct Interval {
  float lower, upper;
  i64 false_pos, n_neg, false_neg, n_pos;
};

// _ChooseThresholdInterval: lower bound first, then upper bound first; each second threshold is chosen among the data the
// first one keeps (>= / <=); "<=" between the two mistake counts keeps the first attempt on a tie.
Interval choose_interval(const std::vector<float>& s, const std::vector<unsigned char>& acc) {
  const size_t N = s.size();
  auto second = [&](float first, bool first_is_lower) {
    std::vector<float> rs;
    std::vector<unsigned char> ra;
    for (size_t i = 0; i < N; i++)
      if (first_is_lower ? s[i] >= first : s[i] <= first) { rs.push_back(s[i]); ra.push_back(acc[i]); }
    return choose_threshold_1d(rs, ra, !first_is_lower);
  };
  auto mistakes = [&](float lo, float hi) {
    i64 m = 0;
    for (size_t i = 0; i < N; i++) m += ((acc[i] != 0) != (s[i] >= lo && s[i] <= hi)) ? 1 : 0;
    return m;
  };
  const float lo1 = choose_threshold_1d(s, acc, true), hi1 = second(lo1, true);
  const float hi2 = choose_threshold_1d(s, acc, false), lo2 = second(hi2, false);
  Interval r;
  if (mistakes(lo1, hi1) <= mistakes(lo2, hi2)) { r.lower = lo1; r.upper = hi1; }
  else { r.lower = lo2; r.upper = hi2; }
  r.false_pos = r.false_neg = r.n_neg = r.n_pos = 0;
  for (size_t i = 0; i < N; i++) {
    const bool in = s[i] >= r.lower && s[i] <= r.upper;
    if (in && !acc[i]) r.false_pos++;
    if (!in && acc[i]) r.false_neg++;
    if (acc[i]) r.n_pos++; else r.n_neg++;
  }
  return r;
}

int find_spheres_with(visfd_hip_ctx* ctx, const float* crds, i64 n_crds, const float* sc, const float* sd, i64 n_spheres,
                      int64_t* ids) {
  return ctx ? visfd_hip_find_spheres(ctx, crds, n_crds, sc, sd, n_spheres, ids)
             : visfd_hip_find_spheres_host(crds, n_crds, sc, sd, n_spheres, ids);
}

int check_list(const float* c, const float* d, const float* s, i64 n, const char* what) {
  if (n < 0 || (n > 0 && (!c || !d || !s)))
    return vh::fail(VISFD_HIP_EINVAL, std::string(what) + ": null list");
  return VISFD_HIP_OK;
}

// _FindBlobScores
int find_blob_scores(visfd_hip_ctx* ctx, const float* tcrds, i64 nt, const float* bc, const float* bd, const float* bs, i64 nb,
                     int criteria, float* scores, int64_t* ids) {
  if (criteria < 0 || criteria > VISFD_HIP_SORT_INCREASING_MAGNITUDE)
    return vh::fail(VISFD_HIP_EINVAL, "find_blob_scores: unknown sort criteria");
  std::vector<float> c(bc, bc + 3 * nb), d(bd, bd + nb), s(bs, bs + nb);
  VH_TRY(visfd_hip_sort_blobs(c.data(), d.data(), s.data(), nb, criteria, 1, nullptr));   // increasing priority
  std::vector<int64_t> which((size_t)nt);
  VH_TRY(find_spheres_with(ctx, tcrds, nt, c.data(), d.data(), nb, which.data()));
  for (i64 i = 0; i < nt; i++) {
    scores[i] = which[(size_t)i] ? s[(size_t)which[(size_t)i] - 1] : -std::numeric_limits<float>::infinity();
    if (ids) ids[i] = which[(size_t)i];
  }
  return VISFD_HIP_OK;
}

// _ComplainIfTrainingDataEmpty, feature_implementation.hpp:101-116 (the texts verbatim)
int complain_if_empty(i64 Nn, i64 Np) {
  if (Nn == 0)
    return vh::fail(VISFD_HIP_EINVAL,
                    "Error: Empty list of negative training examples.\n"
                    "       Either you have provided no examples of data that you want to discard\n"
                    "          (IE. Your file of negative training examples is empty),\n"
                    "       OR none of the examples that you provided are sufficiently close to ANY\n"
                    "       of the blobs in the list of blobs that you are considering discarding.\n"
                    "       Either provide more negative training examples, or specify your\n"
                    "       selection threshold(s) manually.\n");
  if (Np == 0)
    return vh::fail(VISFD_HIP_EINVAL,
                    "Error: Empty list of positive training examples.\n"
                    "       Either you have provided no examples of data that you want to keep\n"
                    "          (IE. Your file of positive training examples is empty),\n"
                    "       OR none of the examples that you provided are sufficiently close to ANY\n"
                    "       of the blobs in the list of blobs that you are considering discarding.\n"
                    "       Either provide more positive training examples, or specify your\n"
                    "       selection threshold(s) manually.\n");
  return VISFD_HIP_OK;
}

// _ChooseBlobScoreThresholdsMulti (one set: _ChooseBlobScoreThresholds): per set positives first, then negatives; the
// points no blob holds are dropped; the sets' survivors are concatenated in order
int choose_thresholds(visfd_hip_ctx* ctx, i64 n_sets, const float* bc, const float* bd, const float* bs, const int64_t* nb,
                      const float* pc, const int64_t* np, const float* nc, const int64_t* nn, int criteria, Interval* out) {
  std::vector<float> scores;
  std::vector<unsigned char> accepted;
  i64 ob = 0, op = 0, on = 0;
  for (i64 I = 0; I < n_sets; I++) {
    VH_TRY(check_list(bc, bd, bs, nb[I], "choose_blob_score_thresholds"));
    if (np[I] < 0 || nn[I] < 0 || (np[I] > 0 && !pc) || (nn[I] > 0 && !nc))
      return vh::fail(VISFD_HIP_EINVAL, "choose_blob_score_thresholds: null training list");
    const i64 nt = np[I] + nn[I];
    std::vector<float> t((size_t)(3 * nt)), ts((size_t)nt);
    std::vector<int64_t> which((size_t)nt);
    if (np[I] > 0) std::memcpy(t.data(), pc + 3 * op, sizeof(float) * 3 * (size_t)np[I]);
    if (nn[I] > 0) std::memcpy(t.data() + 3 * np[I], nc + 3 * on, sizeof(float) * 3 * (size_t)nn[I]);
    VH_TRY(find_blob_scores(ctx, t.data(), nt, bc + 3 * ob, bd + ob, bs + ob, nb[I], criteria, ts.data(), which.data()));
    for (i64 i = 0; i < nt; i++)
      if (which[(size_t)i] != 0) {   // FindBlobScores, feature.hpp:684-690
        scores.push_back(ts[(size_t)i]);
        accepted.push_back(i < np[I] ? 1 : 0);
      }
    ob += nb[I]; op += np[I]; on += nn[I];
  }
  i64 Np = 0;
  for (unsigned char a : accepted) Np += a;
  VH_TRY(complain_if_empty((i64)accepted.size() - Np, Np));
  *out = choose_interval(scores, accepted);
  return VISFD_HIP_OK;
}

void give(const Interval& r, float* lower, float* upper, int64_t* report) {
  if (lower) *lower = r.lower;
  if (upper) *upper = r.upper;
  if (report) { report[0] = r.false_pos; report[1] = r.n_neg; report[2] = r.false_neg; report[3] = r.n_pos; }
}

}  // namespace

extern "C" {

int visfd_hip_choose_threshold_1d(const float* scores, const unsigned char* accepted, int64_t n, int is_lower_bound,
                                  float* threshold) {
  if (n < 0 || !threshold || (n > 0 && (!scores || !accepted)))
    return vh::fail(VISFD_HIP_EINVAL, "choose_threshold_1d: null argument");
  *threshold = choose_threshold_1d(std::vector<float>(scores, scores + n), std::vector<unsigned char>(accepted, accepted + n),
                                   is_lower_bound != 0);
  return VISFD_HIP_OK;
}

int visfd_hip_find_blob_scores(visfd_hip_ctx* ctx, const float* training_crds, int64_t n_training, const float* blob_crds,
                               const float* blob_diameters, const float* blob_scores, int64_t n_blobs, int sort_criteria,
                               float* scores, int64_t* sphere_ids) {
  VH_TRY(check_list(blob_crds, blob_diameters, blob_scores, n_blobs, "find_blob_scores"));
  if (n_training < 0 || (n_training > 0 && (!training_crds || !scores)))
    return vh::fail(VISFD_HIP_EINVAL, "find_blob_scores: null training list");
  return find_blob_scores(ctx, training_crds, n_training, blob_crds, blob_diameters, blob_scores, n_blobs, sort_criteria,
                          scores, sphere_ids);
}

int visfd_hip_choose_blob_score_thresholds_multi(visfd_hip_ctx* ctx, int64_t n_sets, const float* blob_crds,
                                                 const float* blob_diameters, const float* blob_scores,
                                                 const int64_t* n_blobs, const float* pos_crds, const int64_t* n_pos,
                                                 const float* neg_crds, const int64_t* n_neg, int sort_criteria,
                                                 float* lower, float* upper, int64_t* report) {
  if (n_sets < 0 || (n_sets > 0 && (!n_blobs || !n_pos || !n_neg)))
    return vh::fail(VISFD_HIP_EINVAL, "choose_blob_score_thresholds_multi: null counts");
  Interval r;
  VH_TRY(choose_thresholds(ctx, n_sets, blob_crds, blob_diameters, blob_scores, n_blobs, pos_crds, n_pos, neg_crds, n_neg,
                           sort_criteria, &r));
  give(r, lower, upper, report);
  return VISFD_HIP_OK;
}

int visfd_hip_choose_blob_score_thresholds(visfd_hip_ctx* ctx, const float* blob_crds, const float* blob_diameters,
                                           const float* blob_scores, int64_t n_blobs, const float* pos_crds, int64_t n_pos,
                                           const float* neg_crds, int64_t n_neg, int sort_criteria, float* lower,
                                           float* upper, int64_t* report) {
  return visfd_hip_choose_blob_score_thresholds_multi(ctx, 1, blob_crds, blob_diameters, blob_scores, &n_blobs, pos_crds,
                                                      &n_pos, neg_crds, &n_neg, sort_criteria, lower, upper, report);
}

int visfd_hip_discard_blobs_by_score_supervised(visfd_hip_ctx* ctx, float* crds, float* diameters, float* scores,
                                                int64_t* n_inout, const float* pos_crds, int64_t n_pos,
                                                const float* neg_crds, int64_t n_neg, int sort_criteria, float* lower,
                                                float* upper, int64_t* report) {
  if (!n_inout || *n_inout < 0) return vh::fail(VISFD_HIP_EINVAL, "discard_blobs_by_score_supervised: bad count");
  const i64 n = *n_inout;
  Interval r;
  VH_TRY(choose_thresholds(ctx, 1, crds, diameters, scores, &n, pos_crds, &n_pos, neg_crds, &n_neg, sort_criteria, &r));
  give(r, lower, upper, report);
  i64 kept = 0;
  for (i64 i = 0; i < n; i++) {
    if (!(scores[i] >= r.lower && scores[i] <= r.upper)) continue;
    if (kept != i) {
      std::memmove(crds + 3 * kept, crds + 3 * i, 3 * sizeof(float));
      diameters[kept] = diameters[i];
      scores[kept] = scores[i];
    }
    kept++;
  }
  *n_inout = kept;
  return VISFD_HIP_OK;
}

}  // extern "C"
