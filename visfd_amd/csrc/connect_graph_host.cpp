// connect_graph_host.cpp -- the host pieces of LabelConnected as a graph problem (connect_graph.hpp): the
// serial walk of the definition (visfd_hip_label_connected_graph_host), and what the device path (connect_graph.hip)
// leaves to the host: the vector test over its candidate list, the numbering of the clusters from small arrays, and the
// hand-over to the flood of connect.cpp for calls whose result the pop order decides.
#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <unordered_map>
#include <utility>

#include "common.hpp"
#include "connect_graph.hpp"
#include "connect_host.hpp"
#include "eigen3.hpp"

namespace vh {
namespace cg {

Params make_params(const Call& c) {
  Params p = {};
  p.nx = (int)c.nx; p.ny = (int)c.ny; p.nz = (int)c.nz;
  p.signs = c.consider_dot_product_sign != 0;
  p.has_t = c.tensor != nullptr;
  p.has_v = c.direction != nullptr;
  p.standardize = p.has_v && c.standardize_directions && !p.signs;
  const bool from_max = c.start_from_saliency_maxima != 0;
  p.flip_hessian = (c.tensor_is_positive_definite_near_target != 0) == from_max;
  p.SIGN = from_max ? -1.0f : 1.0f;
  p.thr = c.threshold_saliency;
  p.tvs = c.threshold_vector_saliency;
  p.tvn = c.threshold_vector_neighbor;
  if (!p.signs) {   // connect.hpp:207-216: a negative threshold means "do not compare"
    if (p.tvs < 0) p.tvs = 0.0f;
    if (p.tvn < 0) p.tvn = 0.0f;
  }
  p.tts = c.threshold_tensor_saliency;
  p.ttn = c.threshold_tensor_neighbor;
  p.noff = c.connectivity <= 3 ? forward_offsets(c.connectivity, p.off) : 0;
  return p;
}

unsigned early_reasons(const Call& c, bool device) {
  unsigned r = 0;
  if (c.must_link_crds && c.must_link_ngroups > 0) r |= VISFD_HIP_CONNECT_REASON_MUST_LINK;
  if (c.voxel_weights) r |= VISFD_HIP_CONNECT_REASON_WEIGHTS;
  const int64_t n = c.nx * c.ny * c.nz;
  if (c.connectivity > 3 || n > MAX_VOXELS) r |= VISFD_HIP_CONNECT_REASON_LIMITS;
  if (device && (n > VISFD_HIP_EXTREMA_MAX_VOXELS || c.ny > VISFD_HIP_EXTREMA_MAX_NY_NZ || c.nz > VISFD_HIP_EXTREMA_MAX_NY_NZ))
    r |= VISFD_HIP_CONNECT_REASON_LIMITS;
  return r;
}

namespace {

// connect.cpp's pop loop, the "if (V)" block: the principal eigenvector of the saliency's Hessian against the direction
inline bool vector_ok(const Params& p, int order, const float* H, const float* v) {
  float d6[6], e0[3];
  vh::eig::diagonalize_flat(H, order, d6);
  vh::eig::shoemake_row0(d6 + 3, e0);
  if (p.signs) return !(dot3(e0, v) < (p.tvs * std::sqrt(dot3(e0, e0)) * std::sqrt(dot3(v, v))));
  return !(sqr(dot3(e0, v)) < (sqr(p.tvs) * dot3(e0, e0) * dot3(v, v)));
}

inline int eigen_order(const Call& c) {   // connect.hpp:197-201
  return c.start_from_saliency_maxima ? VISFD_HIP_DECREASING_EIVALS : VISFD_HIP_INCREASING_EIVALS;
}

// Serial parity union-find over the words of connect_graph.hpp.  A voxel's sign relative to an ancestor is the XOR of
// the signs along the path, so compressing a path to the root stores (root, that XOR).
struct Parity {
  unsigned* w;
  int find(int x, int* sign) {
    int r = x, acc = 0;
    while ((int)(w[r] >> 1) != r) { acc ^= (int)(w[r] & 1u); r = (int)(w[r] >> 1); }
    *sign = acc;
    while ((int)(w[x] >> 1) != r) {   // second walk: every node on the way gets (root, its own XOR to the root)
      const unsigned old = w[x];
      w[x] = ((unsigned)r << 1) | (unsigned)acc;
      acc ^= (int)(old & 1u);
      x = (int)(old >> 1);
    }
    return r;
  }
  bool unite(int a, int b, int sign) {   // false: already joined with the other relative sign
    int pa, pb;
    int ra = find(a, &pa), rb = find(b, &pb);
    if (ra == rb) return (pa ^ pb) == sign;
    if (ra > rb) std::swap(ra, rb);
    w[rb] = ((unsigned)ra << 1) | (unsigned)(pa ^ pb ^ sign);   // towards the smaller index, as on the device
    return true;
  }
};

thread_local Last g_host_last;

}  // namespace

void vector_test(const Params& p, int order, const float* H, const float* v, int64_t count, unsigned* pass) {
  const int64_t words = (count + 31) / 32;
  parallel_voxels(words, [&](int64_t lo, int64_t hi) {
    for (int64_t wd = lo; wd < hi; wd++) {
      unsigned bits = 0;
      const int64_t end = std::min<int64_t>(count, 32 * wd + 32);
      for (int64_t k = 32 * wd; k < end; k++)
        if (vector_ok(p, order, H + 6 * k, v + 3 * k)) bits |= 1u << (k & 31);
      pass[wd] = bits;
    }
  });
}

void number_clusters(const std::vector<int>& seed_root, std::vector<int>* prov_of_seed, std::vector<int64_t>* deepest) {
  std::vector<std::pair<int, int> > by_root;   // (root, rank) of the valid seeds
  for (size_t k = 0; k < seed_root.size(); k++)
    if (seed_root[k] >= 0) by_root.push_back(std::make_pair(seed_root[k], (int)k));
  std::sort(by_root.begin(), by_root.end());
  prov_of_seed->assign(seed_root.size(), -1);
  for (size_t k = 0; k < by_root.size(); k++)
    if (k == 0 || by_root[k].first != by_root[k - 1].first) (*prov_of_seed)[(size_t)by_root[k].second] = 0;   // an anchor
  deepest->clear();
  for (size_t k = 0; k < seed_root.size(); k++)
    if ((*prov_of_seed)[k] == 0) {
      (*prov_of_seed)[k] = (int)deepest->size();
      deepest->push_back((int64_t)k);
    }
}

int finish_lists(const Call& c, const std::vector<int>& seed, const std::vector<float>& seed_score,
                 const std::vector<int64_t>& deepest, const std::vector<uint64_t>& sizes, std::vector<int64_t>* inv) {
  std::vector<float> as_float(sizes.size());   // an integer below 2^64 rounds to float as its long double does
  for (size_t k = 0; k < sizes.size(); k++) as_float[k] = (float)sizes[k];
  return finish_lists(c, seed, seed_score, deepest, as_float, inv);
}

unsigned link_locations(const Call& c, std::vector<int>* want) {
  want->clear();
  if (!(c.must_link_crds && c.must_link_ngroups > 0 && c.must_link_group_sizes)) return 0;
  unsigned reasons = 0;
  const int64_t dim[3] = {c.nx, c.ny, c.nz};
  int64_t at = 0;
  for (int64_t grp = 0; grp < c.must_link_ngroups; grp++)
    for (int64_t loc = 0; loc < c.must_link_group_sizes[grp]; loc++, at++) {
      long double reach = 0.0L;
      for (int d = 0; d < 3; d++) {
        const float crd = c.must_link_crds[3 * at + d];
        if (!(std::fabs(crd) < 1048576.0f)) { reasons |= VISFD_HIP_CONNECT_REASON_LIMITS; want->push_back(0); continue; }
        const int w = (int)std::floor(crd + 0.5);   // connect.cpp's rounding
        want->push_back(w);
        const long double far = (long double)std::max<int64_t>(std::llabs((long long)w), std::llabs((long long)(w - (dim[d] - 1))));
        reach += far * far;
      }
      if (reach >= 8589934592.0L) reasons |= VISFD_HIP_CONNECT_REASON_LIMITS;   // 2^33
    }
  return reasons;
}

unsigned merge_links(const Call& c, bool standardize, const std::vector<LinkContact>& contact, size_t n_clusters,
                     std::vector<int>* map) {
  std::vector<int> cur(n_clusters);            // the cluster a provisional cluster belongs to by now: the smallest number in it
  std::vector<signed char> q(n_clusters, 1);   // whether its voxels have been negated since
  for (size_t k = 0; k < n_clusters; k++) cur[k] = (int)k;
  unsigned reasons = 0;
  int64_t at = 0;
  for (int64_t grp = 0; grp < c.must_link_ngroups; grp++) {
    const LinkContact* prev = nullptr;
    for (int64_t loc = 0; loc < c.must_link_group_sizes[grp]; loc++, at++) {
      const LinkContact& now = contact[(size_t)at];
      const int pi = now.code >> 1;
      if (prev && cur[(size_t)pi] != cur[(size_t)(prev->code >> 1)]) {
        const int pj = prev->code >> 1;
        const int keep = std::min(cur[(size_t)pi], cur[(size_t)pj]), gone = std::max(cur[(size_t)pi], cur[(size_t)pj]);
        bool negate = false;
        if (standardize) {
          // F = the direction oriented to its provisional anchor, times q: what the flood's n * polarity is at this point.
          // The flood decides from n = F * polarity; the polarities multiply out of every rule (negation commutes with
          // float rounding) except at a zero, where the side the flood takes depends on them.
          float fi[3], fj[3];
          const bool ni = ((now.code & 1) != 0) != (q[(size_t)pi] < 0), nj = ((prev->code & 1) != 0) != (q[(size_t)pj] < 0);
          for (int d = 0; d < 3; d++) { fi[d] = ni ? now.n[d] * -1.0f : now.n[d]; fj[d] = nj ? prev->n[d] * -1.0f : prev->n[d]; }
          const int ri[3] = {(int)(now.index % c.nx), (int)((now.index / c.nx) % c.ny), (int)(now.index / (c.nx * c.ny))};
          const int rj[3] = {(int)(prev->index % c.nx), (int)((prev->index / c.nx) % c.ny), (int)(prev->index / (c.nx * c.ny))};
          float decides;
          const int rule = must_link_decider(fi, fj, ri, rj, c.must_link_directions ? c.must_link_directions[at] : 2, &decides);
          if (decides == 0.0f || decides != decides) reasons |= VISFD_HIP_CONNECT_REASON_ZERO_DOT;
          negate = !must_link_match(rule, decides);
        }
        for (size_t k = 0; k < n_clusters; k++)
          if (cur[k] == gone) {
            cur[k] = keep;
            if (negate) q[k] = (signed char)-q[k];
          }
      }
      prev = &now;
    }
  }
  map->resize(n_clusters);
  for (size_t k = 0; k < n_clusters; k++) (*map)[k] = (cur[k] << 1) | (q[k] < 0 ? 1 : 0);
  return reasons;
}

void settle_moments(const Call& c, std::vector<SettleVoxel>* voxels, size_t n_clusters, bool weighted, bool standardize,
                    std::vector<long double>* sizes, std::vector<long double>* sum_dot) {
  std::sort(voxels->begin(), voxels->end(), [](const SettleVoxel& a, const SettleVoxel& b) { return a.index < b.index; });
  const int nx = (int)c.nx, ny = (int)c.ny;
  cluster_moments(
      [&](auto&& f) {
        for (const SettleVoxel& v : *voxels) f(v.index % nx, (v.index / nx) % ny, v.index / (nx * ny), (int64_t)v.cluster, v.n, v.w);
      },
      n_clusters, weighted, standardize, sizes, sum_dot);
}

int finish_lists(const Call& c, const std::vector<int>& seed, const std::vector<float>& seed_score,
                 const std::vector<int64_t>& deepest, const std::vector<float>& sizes, std::vector<int64_t>* inv) {
  const int64_t n_clusters = (int64_t)deepest.size();
  std::vector<int64_t> perm((size_t)n_clusters);
  inv->resize((size_t)n_clusters);
  for (int64_t k = 0; k < n_clusters; k++) perm[(size_t)k] = (*inv)[(size_t)k] = k;
  if (c.sort_by_size && n_clusters > 0) {   // connect.hpp:1322-1365: (float size, id) descending = reverse of ascending
    std::vector<std::pair<float, int64_t> > key((size_t)n_clusters);
    for (int64_t k = 0; k < n_clusters; k++) key[(size_t)k] = std::make_pair((float)sizes[(size_t)k], k);
    std::sort(key.begin(), key.end());
    std::reverse(key.begin(), key.end());
    for (int64_t k = 0; k < n_clusters; k++) { perm[(size_t)k] = key[(size_t)k].second; (*inv)[(size_t)key[(size_t)k].second] = k; }
  }
  if (c.n_clusters) *c.n_clusters = n_clusters;
  if (c.cluster_maxima || c.cluster_sizes || c.cluster_saliencies) {
    if (c.cluster_capacity < n_clusters) return vh::fail(VISFD_HIP_ECAPACITY, "label_connected: cluster arrays too small");
    for (int64_t k = 0; k < n_clusters; k++) {
      // quirk kept (connect.cpp): only the seed list follows the size ordering
      const int64_t cm = seed[(size_t)deepest[(size_t)perm[(size_t)k]]];
      if (c.cluster_maxima) {
        c.cluster_maxima[3 * k] = (float)(cm % c.nx);
        c.cluster_maxima[3 * k + 1] = (float)((cm / c.nx) % c.ny);
        c.cluster_maxima[3 * k + 2] = (float)(cm / (c.nx * c.ny));
      }
      if (c.cluster_sizes) c.cluster_sizes[k] = (float)sizes[(size_t)k];
      if (c.cluster_saliencies) c.cluster_saliencies[k] = seed_score[(size_t)deepest[(size_t)k]];   // the seed's own value
    }
  }
  return VISFD_HIP_OK;
}

int flood_keeping_unlabelled(const Call& c, const std::vector<int>* seed_index, const std::vector<float>* seed_score) {
  const int64_t n = c.nx * c.ny * c.nz;
  const bool rewrites = c.direction && c.standardize_directions && !c.consider_dot_product_sign;
  std::vector<float> before;
  if (rewrites) before.assign(c.direction, c.direction + 3 * n);
  // the flood runs with 0 for "undefined": no cluster number and no masked voxel's n_seeds + 1 is 0, so the unlabelled
  // voxels can be told apart whatever the caller's label_undefined is
  const int rc = host_label_connected(c.saliency, c.labels, c.mask, c.nx, c.ny, c.nz, c.threshold_saliency, c.direction,
                              c.threshold_vector_saliency, c.threshold_vector_neighbor, c.consider_dot_product_sign, c.tensor,
                              c.threshold_tensor_saliency, c.threshold_tensor_neighbor,
                              c.tensor_is_positive_definite_near_target, c.connectivity, 0, c.sort_by_size,
                              c.standardize_directions, c.start_from_saliency_maxima, c.n_clusters, c.cluster_maxima,
                              c.cluster_sizes, c.cluster_saliencies, c.cluster_capacity, c.voxel_weights, c.must_link_crds,
                              c.must_link_group_sizes, c.must_link_ngroups, c.must_link_directions, seed_index, seed_score);
  // lists too small: the flood has written its labels and directions all the same, as the graph path does on that status
  if (rc != VISFD_HIP_OK && rc != VISFD_HIP_ECAPACITY) return rc;
  for (int64_t i = 0; i < n; i++) {
    const bool masked = c.mask && c.mask[i] == 0.0f;
    if (!masked && c.labels[i] != 0) continue;
    if (rewrites) std::memcpy(c.direction + 3 * i, before.data() + 3 * i, 3 * sizeof(float));
    if (!masked) c.labels[i] = c.label_undefined;
  }
  return rc;
}

int host_walk(const Call& c, Last* last) {
  *last = Last();
  unsigned reasons = early_reasons(c, false);
  if (reasons) {
    const int rc = flood_keeping_unlabelled(c, nullptr, nullptr);
    if (rc != VISFD_HIP_OK && rc != VISFD_HIP_ECAPACITY) return rc;
    last->path = VISFD_HIP_CONNECT_GRAPH_FLOOD;
    last->reasons = reasons;
    return rc;
  }
  const Params p = make_params(c);
  const int64_t n = c.nx * c.ny * c.nz;
  const float* S = c.saliency;
  const float* M = c.mask;
  const float* T = c.tensor;
  float* V = c.direction;
  const int order = eigen_order(c);
  const int64_t plane = c.nx * c.ny;

  // ---- valid voxels (independent of one another: split over the cores)
  std::vector<unsigned> word((size_t)n);
  std::atomic<int64_t> n_valid(0), n_undecided(0);
  parallel_voxels(n, [&](int64_t lo, int64_t hi) {
    int64_t valid = 0, undecided = 0;
    for (int64_t i = lo; i < hi; i++) {
      word[(size_t)i] = NOT_VALID;
      if (!passes_threshold(p, S, M, i)) continue;
      if (T || V) {
        float H[6];
        hessian6(p, S, (int)(i % c.nx), (int)((i / c.nx) % c.ny), (int)(i / plane), H);
        if (T && !passes_tensor(p, H, T + 6 * i)) continue;
        if (V) {
          undecided++;
          if (!vector_ok(p, order, H, V + 3 * i)) continue;
        }
      }
      word[(size_t)i] = (unsigned)i << 1;
      valid++;
    }
    n_valid += valid;
    n_undecided += undecided;
  });
  last->n_valid = n_valid;
  last->n_undecided = n_undecided;

  std::vector<int> seed;
  std::vector<float> seed_score;
  host_find_seeds(S, M, c.nx, c.ny, c.nz, !c.start_from_saliency_maxima, c.threshold_saliency, c.connectivity, &seed, &seed_score);
  const int64_t nseeds = (int64_t)seed.size();

  // ---- compatible edges
  Parity uf = {word.data()};
  for (int64_t i = 0; i < n; i++) {
    if (word[(size_t)i] == NOT_VALID) continue;
    const int x = (int)(i % c.nx), y = (int)((i / c.nx) % c.ny), z = (int)(i / plane);
    for (int k = 0; k < p.noff; k++) {
      const int xx = x + p.off[k][0], yy = y + p.off[k][1], zz = z + p.off[k][2];
      if (xx < 0 || xx >= p.nx || yy < 0 || yy >= p.ny || zz >= p.nz) continue;
      const int64_t j = ((int64_t)zz * c.ny + yy) * c.nx + xx;
      if (word[(size_t)j] == NOT_VALID) continue;
      const bool fwd = passes_neighbour(p, T, V, i, j), bwd = passes_neighbour(p, T, V, j, i);
      if (fwd != bwd) reasons |= VISFD_HIP_CONNECT_REASON_ASYMMETRIC;
      if (!(fwd && bwd)) continue;
      int sign = 0;
      if (p.standardize) {
        const float d = dot3(V + 3 * i, V + 3 * j);
        if (d == 0.0f) reasons |= VISFD_HIP_CONNECT_REASON_ZERO_DOT;
        sign = d < 0.0f;
      }
      if (!uf.unite((int)i, (int)j, sign)) reasons |= VISFD_HIP_CONNECT_REASON_UNBALANCED;
    }
  }

  // ---- clusters: the components that hold a valid seed, numbered by their lowest-ranked one (its anchor)
  std::vector<int> seed_root((size_t)nseeds, -1), seed_sign((size_t)nseeds, 0), prov_of_seed;
  std::vector<int64_t> deepest, inv;
  std::unordered_map<int, int> of_root;   // root -> (provisional number << 1) | the anchor's sign to the root
  std::vector<uint64_t> sizes;
  std::vector<int64_t> sums;
  // (a call that has a reason by now is walked to the end all the same, so that every reason it has is reported)
  for (int64_t k = 0; k < nseeds; k++)
    if (word[(size_t)seed[(size_t)k]] != NOT_VALID) seed_root[(size_t)k] = uf.find(seed[(size_t)k], &seed_sign[(size_t)k]);
  number_clusters(seed_root, &prov_of_seed, &deepest);
  for (int64_t k = 0; k < nseeds; k++)
    if (prov_of_seed[(size_t)k] >= 0) of_root[seed_root[(size_t)k]] = (prov_of_seed[(size_t)k] << 1) | seed_sign[(size_t)k];
  const size_t nc = deepest.size();
  sizes.assign(nc, 0);
  sums.assign(3 * nc, 0);
  // labels as scratch: (provisional number << 1) | sign relative to the anchor, -1 for every other voxel
  int last_root = -1, last_code = -1;
  for (int64_t i = 0; i < n; i++) {
    c.labels[i] = -1;
    if (word[(size_t)i] == NOT_VALID) continue;
    int sign;
    const int r = uf.find((int)i, &sign);
    if (r != last_root) {
      const std::unordered_map<int, int>::const_iterator it = of_root.find(r);
      last_root = r;
      last_code = it == of_root.end() ? -1 : it->second;
    }
    if (last_code < 0) continue;
    const int k = last_code >> 1;
    c.labels[i] = ((int64_t)k << 1) | (int64_t)(sign ^ (last_code & 1));
    sizes[(size_t)k]++;
    sums[3 * (size_t)k] += i % c.nx;
    sums[3 * (size_t)k + 1] += (i / c.nx) % c.ny;
    sums[3 * (size_t)k + 2] += i / plane;
  }

  // ---- outward orientation (connect.cpp's last block): the sign of sum (r - r_com) . n per cluster, taken only where the
  // rounding of the terms cannot decide it (tests/connect_graph_np.py: OUTWARD_GUARD).  The guard here is the
  // restatement's, count * max|term| * 2^-20, not the device's derived count * B * 2^-20 (connect_graph.hip): this walk forms
  // every term exactly as the flood does, so any guard serves it, and with the restatement's its reasons can be checked
  // against the restatement call by call.  B >= max|term|, so the device may hand over a call that this walk keeps.
  std::vector<char> flip(deepest.size(), 0);
  if (p.standardize) {
    const size_t nc = deepest.size();
    std::vector<long double> sum(nc, 0.0L);
    std::vector<float> biggest(nc, 0.0f);
    for (int64_t i = 0; i < n; i++) {
      if (c.labels[i] < 0) continue;
      const size_t k = (size_t)(c.labels[i] >> 1);
      const float pol = (c.labels[i] & 1) ? -1.0f : 1.0f;
      const int x = (int)(i % c.nx), y = (int)((i / c.nx) % c.ny), z = (int)(i / plane);
      const long double size = (long double)sizes[k];
      const float r[3] = {(float)(x - (long double)sums[3 * k] / size), (float)(y - (long double)sums[3 * k + 1] / size),
                          (float)(z - (long double)sums[3 * k + 2] / size)};
      const float v[3] = {V[3 * i] * pol, V[3 * i + 1] * pol, V[3 * i + 2] * pol};
      const float term = dot3(r, v);
      sum[k] += (long double)term;
      if (std::fabs(term) > biggest[k]) biggest[k] = std::fabs(term);
    }
    for (size_t k = 0; k < nc; k++) {
      const double bound = (double)sizes[k] * (double)biggest[k] * 9.5367431640625e-07;   // 2^-20
      if (bound > 0 && !(std::fabs((double)sum[k]) > bound)) reasons |= VISFD_HIP_CONNECT_REASON_OUTWARD;
      flip[k] = sum[k] < 0.0L;
    }
  }

  if (reasons) {   // the pop order decides: the flood, from the seeds found above
    const int rc = flood_keeping_unlabelled(c, &seed, &seed_score);
    if (rc != VISFD_HIP_OK && rc != VISFD_HIP_ECAPACITY) return rc;
    last->path = VISFD_HIP_CONNECT_GRAPH_FLOOD;
    last->reasons = reasons;
    return rc;
  }

  const int rc = finish_lists(c, seed, seed_score, deepest, sizes, &inv);
  for (int64_t i = 0; i < n; i++) {
    if (c.labels[i] < 0) {
      c.labels[i] = (M && M[i] == 0.0f) ? nseeds + 1 : c.label_undefined;
      continue;
    }
    const size_t k = (size_t)(c.labels[i] >> 1);
    if (p.standardize) {
      if (c.labels[i] & 1) { V[3 * i] *= -1.0f; V[3 * i + 1] *= -1.0f; V[3 * i + 2] *= -1.0f; }
      if (flip[k]) { V[3 * i] *= -1.0f; V[3 * i + 1] *= -1.0f; V[3 * i + 2] *= -1.0f; }
    }
    c.labels[i] = inv[k] + 1;
  }
  last->path = VISFD_HIP_CONNECT_GRAPH_HOST_GRAPH;
  return rc;
}

Last& host_last() { return g_host_last; }

}  // namespace cg
}  // namespace vh

extern "C" int visfd_hip_label_connected_graph_host(
    const float* saliency, int64_t* labels, const float* mask, int64_t nx, int64_t ny, int64_t nz, float threshold_saliency,
    float* direction, float threshold_vector_saliency, float threshold_vector_neighbor, int consider_dot_product_sign,
    const float* tensor, float threshold_tensor_saliency, float threshold_tensor_neighbor,
    int tensor_is_positive_definite_near_target, int connectivity, int64_t label_undefined, int sort_by_size,
    int standardize_directions, int start_from_saliency_maxima, int64_t* n_clusters, float* cluster_maxima,
    float* cluster_sizes, float* cluster_saliencies, int64_t cluster_capacity, const float* voxel_weights,
    const float* must_link_crds, const int64_t* must_link_group_sizes, int64_t must_link_ngroups,
    const int* must_link_directions) {
  VH_TRY(vh::label_connected_check_args(saliency, labels, nx, ny, nz, connectivity));   // before any allocation
  const vh::cg::Call c = {saliency, labels, mask, nx, ny, nz, threshold_saliency, direction, threshold_vector_saliency,
                          threshold_vector_neighbor, consider_dot_product_sign, tensor, threshold_tensor_saliency,
                          threshold_tensor_neighbor, tensor_is_positive_definite_near_target, connectivity, label_undefined,
                          sort_by_size, standardize_directions, start_from_saliency_maxima, n_clusters, cluster_maxima,
                          cluster_sizes, cluster_saliencies, cluster_capacity, voxel_weights, must_link_crds,
                          must_link_group_sizes, must_link_ngroups, must_link_directions};
  vh::cg::Last last;
  const int rc = vh::cg::host_walk(c, &last);
  if (rc == VISFD_HIP_OK || rc == VISFD_HIP_ECAPACITY) vh::cg::host_last() = last;
  return rc;
}
