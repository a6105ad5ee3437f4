// connect_graph.hip -- LabelConnected as a graph problem on the device (the definition and the shared
// arithmetic: connect_graph.hpp; the host pieces: connect_graph_host.cpp).
//
//   (a) classify   one sweep: mask, threshold, and where both pass the 19-point Hessian against the vote tensor;
//                  the survivors are compacted into a list (a second sweep over the 4-byte words, once their number is known)
//   (b) vector     the list's Hessians and directions go to the host, which runs the vector test with its own eigen code
//                  and returns one bit per entry (connect_graph.hpp says why this stage cannot run here)
//   (c) edges      per listed voxel and forward offset both directed neighbour tests; compatible pairs are united in a
//                  lock-free union-find whose words carry the voxel's sign relative to its parent
//   (d) clusters   the ranked seeds of extrema.hip: atomicMin of the rank at each valid seed's root; the host numbers
//                  the anchors; sizes and coordinate sums are integer atomics
//   (e) directions sign = parity to the root XOR the anchor's; the outward sum in fp64 with its bound; one last pass
//                  writes labels and directions of the labelled voxels
//
// A call whose result the pop order decides (the reason bits of include/visfd_hip.h) is handed to the flood of
// connect.cpp, from the seeds found here; the directions of unlabelled voxels are then put back, so the contract is the
// same on every path.
// Option connect_settle: must-links (nearest labelled voxel per location here, the merges on the host between (d) and
// (e)), voxel weights and doubtful outward sums (the labelled voxels gathered for the host, which runs the flood's own
// statements over them: connect_host.hpp) are then no reasons.
#include <chrono>
#include <limits>

#include "common.hpp"
#include "connect_graph.hpp"
#include "connect_host.hpp"
#include "tile.hpp"
#include "wave.hpp"

namespace vh {
namespace cg {
namespace {

constexpr int BLOCK = 256;

// ---- the parity union-find ----------------------------------------------------------------------------------------------
// word[v] = (parent << 1) | sign of v relative to that parent; a root holds (v << 1).  The invariant everything rests on:
// once v has a parent, every word v ever holds is a pair (a, s) where a is an ancestor of v in the final forest and s is
// v's sign relative to a -- and that sign never changes, because the sign between two voxels of one tree is fixed by the
// first path that joined them (a later edge that disagrees changes nothing: it raises UNBALANCED).  Roots are hooked only
// by a compare-and-swap from their own word (v << 1), towards a smaller index, so there are no cycles and a root is hooked
// once.  A non-root's word is only ever replaced by another such pair (path halving below).  A word read late (another
// CU's copy) is therefore an older TRUE statement: a find may take more steps or end at a voxel that has stopped being a
// root, never at a wrong sign; the compare-and-swap, which acts on memory, is what decides whether a root still is one.
__device__ __forceinline__ unsigned ld_word(const unsigned* p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// an ancestor of x that was a root when read, and x's sign relative to it; every second link on the way is shortened to
// (grandparent, sign to the grandparent) -- the XOR of two true statements
__device__ __forceinline__ int find_sign(unsigned* word, int x, int* sign) {
  int acc = 0;
  for (;;) {
    const unsigned wx = ld_word(word + x);
    const int p = (int)(wx >> 1);
    if (p == x) break;
    const unsigned wp = ld_word(word + p);
    const int gp = (int)(wp >> 1);
    if (gp == p) {
      acc ^= (int)(wx & 1u);
      x = p;
      break;
    }
    const unsigned shortened = ((unsigned)gp << 1) | ((wx ^ wp) & 1u);
    __hip_atomic_store(word + x, shortened, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // x has a parent: no hook can be aimed at it
    acc ^= (int)(shortened & 1u);
    x = gp;
  }
  *sign = acc;
  return x;
}

// x and y belong together with relative sign rel
__device__ __forceinline__ void unite_sign(unsigned* word, int x, int y, int rel, unsigned* flags) {
  for (;;) {
    int sx, sy;
    const int rx = find_sign(word, x, &sx), ry = find_sign(word, y, &sy);
    const int r = sx ^ sy ^ rel;   // the sign between the two ancestors
    if (rx == ry) {
      if (r) atomicOr(flags, (unsigned)VISFD_HIP_CONNECT_REASON_UNBALANCED);
      return;
    }
    const int a = rx > ry ? rx : ry, b = rx > ry ? ry : rx;
    const unsigned own = (unsigned)a << 1;
    const unsigned old = atomicCAS(word + a, own, ((unsigned)b << 1) | (unsigned)r);
    if (old == own) return;
    // a was hooked in the meantime: old = (q, s) says a = s relative to q, so what is left to join is q and b with s ^ r
    x = (int)(old >> 1);
    y = b;
    rel = (int)(old & 1u) ^ r;
  }
}

// ---- (a) ----------------------------------------------------------------------------------------------------------------
// four voxels per thread: 16-byte loads of saliency and mask, a 16-byte store of the words and two of the labels (vec: all
// four arrays are 16-byte aligned); the Hessian and the tensor are read only where mask and threshold pass
__global__ void __launch_bounds__(BLOCK)
classify_kernel(Params p, const float* __restrict__ S, const float* __restrict__ M, const float* __restrict__ T,
                unsigned* __restrict__ word, int64_t* __restrict__ labels, int64_t n, int64_t label_masked,
                int64_t label_undefined, int vec, unsigned long long* __restrict__ counters) {
  const int64_t i0 = 4 * ((int64_t)blockIdx.x * BLOCK + threadIdx.x);
  if (i0 >= n) return;
  float s[4], m[4] = {1.0f, 1.0f, 1.0f, 1.0f};
  const int cnt = n - i0 < 4 ? (int)(n - i0) : 4;
  if (vec && cnt == 4) {
    const float4 sv = *reinterpret_cast<const float4*>(S + i0);
    s[0] = sv.x; s[1] = sv.y; s[2] = sv.z; s[3] = sv.w;
    if (M) {
      const float4 mv = *reinterpret_cast<const float4*>(M + i0);
      m[0] = mv.x; m[1] = mv.y; m[2] = mv.z; m[3] = mv.w;
    }
  } else {
    for (int k = 0; k < cnt; k++) {
      s[k] = S[i0 + k];
      if (M) m[k] = M[i0 + k];
    }
  }
  unsigned w[4];
  int64_t lab[4];
  unsigned found = 0;
  const int64_t plane = (int64_t)p.nx * p.ny;
  for (int k = 0; k < cnt; k++) {
    const int64_t i = i0 + k;
    const bool masked = m[k] == 0.0f;
    lab[k] = masked ? label_masked : label_undefined;
    w[k] = NOT_VALID;
    if (masked || s[k] * p.SIGN > p.thr * p.SIGN) continue;
    if (T) {
      float H[6];
      hessian6(p, S, (int)(i % p.nx), (int)((i / p.nx) % p.ny), (int)(i / plane), H);
      if (!passes_tensor(p, H, T + 6 * i)) continue;
    }
    w[k] = (unsigned)i << 1;
    found++;
  }
  if (vec && cnt == 4) {
    *reinterpret_cast<uint4*>(word + i0) = make_uint4(w[0], w[1], w[2], w[3]);
    *reinterpret_cast<longlong2*>(labels + i0) = make_longlong2(lab[0], lab[1]);
    *reinterpret_cast<longlong2*>(labels + i0 + 2) = make_longlong2(lab[2], lab[3]);
  } else {
    for (int k = 0; k < cnt; k++) {
      word[i0 + k] = w[k];
      labels[i0 + k] = lab[k];
    }
  }
  if (found) atomicAdd(counters, (unsigned long long)found);
}

// the listed voxels in no particular order (nothing downstream depends on it); with directions, their Hessian and direction
__global__ void __launch_bounds__(BLOCK)
gather_kernel(Params p, const float* __restrict__ S, const float* __restrict__ V, const unsigned* __restrict__ word,
              int64_t n, int* __restrict__ list, int* __restrict__ aux, float* __restrict__ recH, float* __restrict__ recV,
              unsigned long long cap, unsigned long long* __restrict__ counters) {
  const int64_t i0 = 4 * ((int64_t)blockIdx.x * BLOCK + threadIdx.x);
  if (i0 >= n) return;
  const int cnt = n - i0 < 4 ? (int)(n - i0) : 4;
  unsigned w[4];
  if (cnt == 4) {   // word comes from the workspace: aligned
    const uint4 wv = *reinterpret_cast<const uint4*>(word + i0);
    w[0] = wv.x; w[1] = wv.y; w[2] = wv.z; w[3] = wv.w;
  } else {
    for (int k = 0; k < cnt; k++) w[k] = word[i0 + k];
  }
  const int64_t plane = (int64_t)p.nx * p.ny;
  for (int k = 0; k < cnt; k++) {
    if (w[k] == NOT_VALID) continue;
    const int64_t i = i0 + k;
    const unsigned long long slot = atomicAdd(counters + 1, 1ull);
    if (slot >= cap) continue;   // cannot happen: cap is what classify_kernel counted
    list[slot] = (int)i;
    aux[i] = NO_SEED;
    if (V) {
      float H[6];
      hessian6(p, S, (int)(i % p.nx), (int)((i / p.nx) % p.ny), (int)(i / plane), H);
      for (int c = 0; c < 6; c++) recH[6 * slot + c] = H[c];
      for (int c = 0; c < 3; c++) recV[3 * slot + c] = V[3 * i + c];
    }
  }
}

// ---- (b): the host's verdicts -------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(BLOCK)
reject_kernel(const int* __restrict__ list, const unsigned* __restrict__ pass, int64_t count, unsigned* __restrict__ word) {
  const int64_t k = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
  if (k >= count) return;
  if (!((pass[k >> 5] >> (k & 31)) & 1u)) word[list[k]] = NOT_VALID;
}

// ---- (c) ----------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(BLOCK)
edges_kernel(Params p, const float* __restrict__ T, const float* __restrict__ V, const int* __restrict__ list, int64_t count,
             unsigned* word, unsigned* flags) {
  const int64_t k = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
  if (k >= count) return;
  const int i = list[k];
  if (ld_word(word + i) == NOT_VALID) return;   // validity was settled before this launch and does not change in it
  const int x = i % p.nx, y = (i / p.nx) % p.ny, z = i / (p.nx * p.ny);
  unsigned reasons = 0;
  for (int o = 0; o < p.noff; o++) {
    const int xx = x + p.off[o][0], yy = y + p.off[o][1], zz = z + p.off[o][2];
    if (xx < 0 || xx >= p.nx || yy < 0 || yy >= p.ny || zz >= p.nz) continue;
    const int j = (zz * p.ny + yy) * p.nx + xx;
    if (ld_word(word + j) == NOT_VALID) continue;
    const bool fwd = passes_neighbour(p, T, V, i, j), bwd = passes_neighbour(p, T, V, j, i);
    if (fwd != bwd) reasons |= VISFD_HIP_CONNECT_REASON_ASYMMETRIC;
    if (!(fwd && bwd)) continue;
    int sign = 0;
    if (p.standardize) {
      const float d = dot3(V + 3 * (int64_t)i, V + 3 * (int64_t)j);
      if (d == 0.0f) reasons |= VISFD_HIP_CONNECT_REASON_ZERO_DOT;
      sign = d < 0.0f;
    }
    unite_sign(word, i, j, sign, flags);
  }
  if (reasons) atomicOr(flags, reasons);
}

// ---- (d) ----------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(BLOCK)
seed_root_kernel(const int* __restrict__ seed, int64_t nseeds, unsigned* word, int* aux, int* __restrict__ seed_root,
                 int* __restrict__ seed_sign) {
  const int64_t k = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
  if (k >= nseeds) return;
  const int c = seed[k];
  int root = -1, sign = 0;
  if (ld_word(word + c) != NOT_VALID) {
    root = find_sign(word, c, &sign);   // the unions are complete: this is the root
    atomicMin(aux + root, (int)k);
  }
  seed_root[k] = root;
  seed_sign[k] = sign;
}

// code[k]: -1 for a seed that is no valid voxel, else (anchor of its component << 1) | sign to the root
__global__ void __launch_bounds__(BLOCK)
seed_anchor_kernel(int64_t nseeds, const int* __restrict__ aux, const int* __restrict__ seed_root,
                   const int* __restrict__ seed_sign, int* __restrict__ code) {
  const int64_t k = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
  if (k >= nseeds) return;
  const int r = seed_root[k];
  code[k] = r < 0 ? -1 : (((aux[r] == (int)k) ? 1 : 0) << 1) | seed_sign[k];
}

// aux[root] = (provisional number << 1) | the anchor's sign to the root; roots without a valid seed keep NO_SEED
__global__ void __launch_bounds__(BLOCK)
seed_number_kernel(int64_t nseeds, const int* __restrict__ prov, const int* __restrict__ seed_root,
                   const int* __restrict__ seed_sign, int* __restrict__ aux) {
  const int64_t k = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
  if (k >= nseeds) return;
  if (prov[k] >= 0) aux[seed_root[k]] = (prov[k] << 1) | seed_sign[k];
}

// res[k] = (provisional number << 1) | sign relative to the anchor, -1 where the listed voxel stays unlabelled; per cluster
// the voxel count and the three coordinate sums, integers (one atomic per wave where the wave's voxels share a cluster;
// sizes null: res alone)
__global__ void __launch_bounds__(BLOCK)
census_kernel(Params p, const int* __restrict__ list, int64_t count, unsigned* word, const int* __restrict__ aux,
              int* __restrict__ res, unsigned long long* __restrict__ sizes, unsigned long long* __restrict__ sums) {
  const int64_t k = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
  int prov = -1;
  unsigned long long x = 0, y = 0, z = 0;
  if (k < count) {
    const int i = list[k];
    int code = -1;
    if (ld_word(word + i) != NOT_VALID) {
      int sign;
      const int a = aux[find_sign(word, i, &sign)];
      if (a != NO_SEED) code = a ^ sign;   // (number << 1) | (anchor's sign ^ this voxel's sign)
    }
    res[k] = code;
    if (code >= 0) {
      prov = code >> 1;
      x = (unsigned)(i % p.nx); y = (unsigned)((i / p.nx) % p.ny); z = (unsigned)(i / (p.nx * p.ny));
    }
  }
  if (!sizes) return;   // option connect_settle with voxel weights: the host forms the moments (the same for every thread)
  // no lane has left: a lane past the list holds nothing (prov < 0) and adds zeros
  int common;
  if (wave_agree(prov, &common)) {
    const unsigned long long c = wave_sum<unsigned long long>(prov >= 0 ? 1ull : 0ull);
    x = wave_sum(x); y = wave_sum(y); z = wave_sum(z);
    if (wave_lane() == 0 && common >= 0) {
      atomicAdd(sizes + common, c);
      atomicAdd(sums + 3 * common, x); atomicAdd(sums + 3 * common + 1, y); atomicAdd(sums + 3 * common + 2, z);
    }
  } else if (prov >= 0) {
    atomicAdd(sizes + prov, 1ull);
    atomicAdd(sums + 3 * prov, x); atomicAdd(sums + 3 * prov + 1, y); atomicAdd(sums + 3 * prov + 2, z);
  }
}

// ---- (e) ----------------------------------------------------------------------------------------------------------------
// Per cluster: sum of dot3((float)(r - com), n) in fp64, B = max (|r_x| + |r_y| + |r_z|) * max|n_d| as float bits (the
// values are not negative, so the bits order like the values), and whether any term is not an exact zero.
__global__ void __launch_bounds__(BLOCK)
outward_kernel(Params p, const float* __restrict__ V, const int* __restrict__ list, const int* __restrict__ res,
               int64_t count, const double* __restrict__ com, double* __restrict__ sum, unsigned* __restrict__ B,
               unsigned* __restrict__ any) {
  const int64_t k = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
  int prov = -1;
  double term = 0.0;
  float bound = 0.0f;
  bool nonzero = false;
  if (k < count && res[k] >= 0) {
    prov = res[k] >> 1;
    const int i = list[k];
    const float pol = (res[k] & 1) ? -1.0f : 1.0f;
    const int x = i % p.nx, y = (i / p.nx) % p.ny, z = i / (p.nx * p.ny);
    const float r[3] = {(float)(x - com[3 * prov]), (float)(y - com[3 * prov + 1]), (float)(z - com[3 * prov + 2])};
    const float v[3] = {V[3 * (int64_t)i] * pol, V[3 * (int64_t)i + 1] * pol, V[3 * (int64_t)i + 2] * pol};
    const float t = dot3(r, v);
    term = (double)t;
    bound = (fabsf(r[0]) + fabsf(r[1]) + fabsf(r[2])) * fmaxf(fabsf(v[0]), fmaxf(fabsf(v[1]), fabsf(v[2])));
    nonzero = !(t == 0.0f);
  }
  // one atomic of each kind per wave where the wave's voxels share a cluster (a lane that holds nothing adds 0, 0, false)
  int common;
  if (wave_agree(prov, &common)) {
    term = wave_sum(term);   // fp64: the butterfly's order fixes the bits
    unsigned bits = __float_as_uint(bound);
    for (int o = 32; o > 0; o >>= 1) {
      const unsigned other = __shfl_xor(bits, o);
      bits = other > bits ? other : bits;
    }
    const bool some = __ballot(nonzero) != 0;
    if (wave_lane() == 0 && common >= 0) {
      atomicAdd(sum + common, term);
      atomicMax(B + common, bits);
      if (some) atomicOr(any + common, 1u);
    }
  } else if (prov >= 0) {
    atomicAdd(sum + prov, term);
    atomicMax(B + prov, __float_as_uint(bound));
    if (nonzero) atomicOr(any + prov, 1u);
  }
}

// labels and directions of the labelled voxels; final[prov] = (final label << 1) | outward flip
__global__ void __launch_bounds__(BLOCK)
write_kernel(const int* __restrict__ list, const int* __restrict__ res, int64_t count, const int64_t* __restrict__ final,
             int standardize, int64_t* __restrict__ labels, float* __restrict__ V) {
  const int64_t k = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
  if (k >= count || res[k] < 0) return;
  const int64_t i = list[k];
  const int64_t f = final[res[k] >> 1];
  labels[i] = f >> 1;
  if (standardize) {   // the flood's two multiplications (polarity, then the outward flip), each only where it is -1
    float v[3] = {V[3 * i], V[3 * i + 1], V[3 * i + 2]};
    if (res[k] & 1) for (int c = 0; c < 3; c++) v[c] *= -1.0f;
    if (f & 1) for (int c = 0; c < 3; c++) v[c] *= -1.0f;
    for (int c = 0; c < 3; c++) V[3 * i + c] = v[c];
  }
}

// ---- option connect_settle: must-links, voxel weights and doubtful outward sums without the flood ----------------------------
constexpr int LINK_BATCH = 32;   // locations per pass over a workgroup's voxels
constexpr int LINK_ITEMS = 4;    // listed voxels per thread
constexpr unsigned long long NO_KEY = ~0ull;

// FindNearestVoxel over the labelled voxels, for every must-link location at once: keys[l] = min of
// (squared distance << 31) | voxel index, so among the closest the first in scan order wins, as "strictly closer wins"
// does in the flood's scan.  want[l][3]: the location as the flood rounds it; the host has made sure that no squared
// distance reaches 2^33.  Each thread keeps its voxels in registers and walks the locations, which are the same for the
// whole wave; a wave's minimum goes to LDS, and a workgroup sends one atomic per location.
__global__ void __launch_bounds__(BLOCK)
nearest_kernel(Params p, const int* __restrict__ list, const int* __restrict__ res, int64_t count, const int* __restrict__ want,
               int nloc, unsigned long long* __restrict__ keys) {
  __shared__ unsigned long long best[LINK_BATCH];
  int idx[LINK_ITEMS], x[LINK_ITEMS], y[LINK_ITEMS], z[LINK_ITEMS];
  const int64_t base = (int64_t)blockIdx.x * (BLOCK * LINK_ITEMS) + threadIdx.x;
  for (int j = 0; j < LINK_ITEMS; j++) {
    const int64_t k = base + (int64_t)j * BLOCK;
    idx[j] = -1;
    x[j] = y[j] = z[j] = 0;
    if (k < count && res[k] >= 0) {
      const int i = list[k];
      idx[j] = i;
      x[j] = i % p.nx; y[j] = (i / p.nx) % p.ny; z[j] = i / (p.nx * p.ny);
    }
  }
  for (int l0 = 0; l0 < nloc; l0 += LINK_BATCH) {
    const int lend = nloc - l0 < LINK_BATCH ? nloc - l0 : LINK_BATCH;
    if (threadIdx.x < LINK_BATCH) best[threadIdx.x] = NO_KEY;
    __syncthreads();
    for (int l = 0; l < lend; l++) {
      const long long wx = want[3 * (l0 + l)], wy = want[3 * (l0 + l) + 1], wz = want[3 * (l0 + l) + 2];
      unsigned long long key = NO_KEY;
      for (int j = 0; j < LINK_ITEMS; j++) {
        if (idx[j] < 0) continue;
        const long long dx = wx - x[j], dy = wy - y[j], dz = wz - z[j];
        const unsigned long long cand = ((unsigned long long)(dx * dx + dy * dy + dz * dz) << 31) | (unsigned long long)idx[j];
        key = cand < key ? cand : key;
      }
      key = wave_min(key);   // the loops over l0 and l are the same for every thread; a lane without voxels holds NO_KEY
      if (wave_lane() == 0 && key != NO_KEY) atomicMin(&best[l], key);
    }
    __syncthreads();
    if ((int)threadIdx.x < lend && best[threadIdx.x] != NO_KEY) atomicMin(keys + l0 + threadIdx.x, best[threadIdx.x]);
    __syncthreads();
  }
}

// per location: the nearest voxel's code ((provisional number << 1) | sign to the anchor) and its direction as it came in
__global__ void __launch_bounds__(BLOCK)
link_fetch_kernel(int nloc, const unsigned long long* __restrict__ keys, unsigned* word, const int* __restrict__ aux,
                  const float* __restrict__ V, int* __restrict__ code, float* __restrict__ dir) {
  const int l = blockIdx.x * BLOCK + threadIdx.x;
  if (l >= nloc) return;
  int cd = -1;
  float v[3] = {0.0f, 0.0f, 0.0f};
  if (keys[l] != NO_KEY) {
    const int i = (int)(keys[l] & 0x7fffffffull);
    int sign;
    const int a = aux[find_sign(word, i, &sign)];
    if (a != NO_SEED) cd = a ^ sign;
    if (V) for (int c = 0; c < 3; c++) v[c] = V[3 * (int64_t)i + c];
  }
  code[l] = cd;
  for (int c = 0; c < 3; c++) dir[3 * l + c] = v[c];
}

// after the merges: map[k] = (the number cluster k's voxels carry from here on << 1) | whether they are negated
__global__ void __launch_bounds__(BLOCK)
remap_kernel(int64_t count, const int* __restrict__ map, int* __restrict__ res) {
  const int64_t k = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
  if (k >= count || res[k] < 0) return;
  res[k] = map[res[k] >> 1] ^ (res[k] & 1);
}

// The labelled voxels of the clusters the host has to walk itself (wanted[k] != 0; null: all of them), compacted: voxel
// index, cluster, the direction write_kernel would give it before the outward flip, and the weight where the weights are
// on the device.  One atomic per wave; the order is whatever the waves make it, the host sorts by index.
__global__ void __launch_bounds__(BLOCK)
settle_gather_kernel(const int* __restrict__ list, const int* __restrict__ res, int64_t count,
                     const unsigned char* __restrict__ wanted, const float* __restrict__ V, const float* __restrict__ W,
                     unsigned long long cap, unsigned long long* __restrict__ counter, int* __restrict__ out_index,
                     int* __restrict__ out_cluster, float* __restrict__ out_n, float* __restrict__ out_w) {
  const int64_t k = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
  const bool has = k < count && res[k] >= 0 && (!wanted || wanted[res[k] >> 1]);
  const unsigned long long holders = __ballot(has);
  if (!holders) return;
  const int lane = wave_lane(), leader = wave_leader(holders);
  unsigned long long first = 0;
  if (lane == leader) first = atomicAdd(counter, (unsigned long long)__popcll(holders));
  first = __shfl(first, leader);
  if (!has) return;
  const unsigned long long slot = first + (unsigned long long)wave_rank(holders, lane);
  if (slot >= cap) return;   // cannot happen: cap is the number of such voxels, or the length of the list
  const int64_t i = list[k];
  out_index[slot] = (int)i;
  out_cluster[slot] = res[k] >> 1;
  float v[3] = {0.0f, 0.0f, 0.0f};
  if (V) {
    for (int c = 0; c < 3; c++) v[c] = V[3 * i + c];
    if (res[k] & 1) for (int c = 0; c < 3; c++) v[c] *= -1.0f;
  }
  for (int c = 0; c < 3; c++) out_n[3 * slot + c] = v[c];
  out_w[slot] = W ? W[i] : 1.0f;
}

// ---- orchestration --------------------------------------------------------------------------------------------------------
struct DevArrays {
  const float* S;
  const float* M;
  float* V;
  const float* T;
  int64_t* labels;
  const float* W;        // voxel weights on the device (the _dev face), or
  const float* W_host;   // on the host (the host-array face looks up the gathered voxels' weights there); both null: none
};

enum { MS_SEEDS = 0, MS_CLASSIFY, MS_VECTOR, MS_EDGES, MS_CLUSTERS, MS_DIRECTIONS, MS_COPY_IN, MS_COPY_OUT, MS_COUNT };

struct Clock {   // option connect_time: wall time per stage, the stream drained at every mark
  visfd_hip_ctx* ctx;
  bool on;
  std::chrono::steady_clock::time_point t;
  int start() {
    if (!on) return VISFD_HIP_OK;
    for (int k = 0; k < MS_COUNT; k++) ctx->connect_graph_ms[k] = 0.0f;
    t = std::chrono::steady_clock::now();
    return VISFD_HIP_OK;
  }
  int mark(int stage) {
    if (!on) return VISFD_HIP_OK;
    VH_HIP(hipStreamSynchronize(ctx->stream));
    const std::chrono::steady_clock::time_point now = std::chrono::steady_clock::now();
    ctx->connect_graph_ms[stage] += std::chrono::duration<float, std::milli>(now - t).count();
    t = now;
    return VISFD_HIP_OK;
  }
};

inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

template <typename T>
int to_host(visfd_hip_ctx* ctx, T* host, const T* dev, size_t count) {
  VH_HIP(hipMemcpyAsync(host, dev, sizeof(T) * count, hipMemcpyDeviceToHost, ctx->stream));
  VH_HIP(hipStreamSynchronize(ctx->stream));
  return VISFD_HIP_OK;
}
template <typename T>
int to_dev(visfd_hip_ctx* ctx, T* dev, const T* host, size_t count) {   // small arrays of locals: waited for
  VH_HIP(hipMemcpyAsync(dev, host, sizeof(T) * count, hipMemcpyHostToDevice, ctx->stream));
  VH_HIP(hipStreamSynchronize(ctx->stream));
  return VISFD_HIP_OK;
}

bool search_fits(const Call& c);
int search_seeds(visfd_hip_ctx* ctx, const Call& c, const float* dev_saliency, const float* dev_mask, std::vector<int>* seed,
                 std::vector<float>* score);

// The labelled voxels of the wanted clusters (null: all), for the host's walk.  cap: how many there can be; counter: a
// word of the call's counters.
int gather_for_host(visfd_hip_ctx* ctx, const DevArrays& d, const int* list, const int* res, int64_t count,
                    const unsigned char* wanted, size_t nc, unsigned long long cap, unsigned long long* counter,
                    std::vector<SettleVoxel>* vox) {
  vox->clear();
  if (nc == 0 || count == 0 || cap == 0) return VISFD_HIP_OK;
  hipStream_t st = ctx->stream;
  int* buf;
  const size_t wanted_words = (nc + 3) / 4;
  VH_TRY(ws(ctx, WS_CG_SETTLE, (size_t)(6 * cap) + wanted_words, &buf));
  int *out_index = buf, *out_cluster = buf + cap;
  float *out_n = reinterpret_cast<float*>(buf + 2 * cap), *out_w = reinterpret_cast<float*>(buf + 5 * cap);
  unsigned char* dev_wanted = nullptr;
  if (wanted) {
    dev_wanted = reinterpret_cast<unsigned char*>(buf + 6 * cap);
    VH_TRY(to_dev(ctx, dev_wanted, wanted, nc));
  }
  VH_HIP(hipMemsetAsync(counter, 0, sizeof(unsigned long long), st));
  settle_gather_kernel<<<grid_for(count, BLOCK), BLOCK, 0, st>>>(list, res, count, dev_wanted, d.V, d.W, cap, counter, out_index,
                                                                 out_cluster, out_n, out_w);
  VH_HIP(hipGetLastError());
  unsigned long long m = 0;
  VH_TRY(to_host(ctx, &m, counter, 1));
  if (m > cap) m = cap;
  if (m == 0) return VISFD_HIP_OK;
  std::vector<int> hi(2 * (size_t)m);
  std::vector<float> hn(3 * (size_t)m), hw((size_t)m);
  VH_TRY(to_host(ctx, hi.data(), out_index, (size_t)m));
  VH_TRY(to_host(ctx, hi.data() + m, out_cluster, (size_t)m));
  VH_TRY(to_host(ctx, hn.data(), out_n, 3 * (size_t)m));
  if (d.W) VH_TRY(to_host(ctx, hw.data(), out_w, (size_t)m));
  vox->resize((size_t)m);
  for (size_t k = 0; k < (size_t)m; k++) {
    SettleVoxel& v = (*vox)[k];
    v.index = hi[k];
    v.cluster = hi[m + k];
    for (int a = 0; a < 3; a++) v.n[a] = hn[3 * k + a];
    v.w = d.W ? hw[k] : d.W_host ? d.W_host[v.index] : 1.0f;
  }
  return VISFD_HIP_OK;
}

// Must-links (option connect_settle), after the provisional clusters are numbered: the nearest labelled voxel of every
// location on the device, the merges on the host (connect_graph_host.cpp: merge_links), then res, deepest, sizes and sums
// speak of the merged clusters.  *reasons: ZERO_DOT where a contact cannot be decided without the flood.
int settle_links(visfd_hip_ctx* ctx, const Call& c, const Params& p, const DevArrays& d, const int* list, int* res,
                 int64_t count, unsigned* word, const int* aux, unsigned long long* cl, std::vector<int64_t>* deepest,
                 std::vector<uint64_t>* sizes, std::vector<int64_t>* sums, unsigned* reasons) {
  if (!c.must_link_group_sizes) return fail(VISFD_HIP_EINVAL, "label_connected: must-link group sizes missing");
  std::vector<int> want;
  link_locations(c, &want);   // its limits were looked at before any work started
  const int nloc = (int)(want.size() / 3);
  if (nloc == 0) return VISFD_HIP_OK;
  const size_t nc = deepest->size();
  if (nc == 0)   // the flood's FindNearestVoxel over an empty set (connect.cpp)
    return fail(VISFD_HIP_EINVAL, "Error: No voxels clustered. Empty image. Your cluster criteria are too strict.\n"
                                  "       (Attempting the find the nearest voxel from an empty set.)\n");
  hipStream_t st = ctx->stream;
  unsigned long long* keys;   // keys | want[3] | code | direction[3]
  VH_TRY(ws(ctx, WS_CG_LINKS, (size_t)nloc * 5 + (nc + 1) / 2, &keys));   // 8 + 12 + 4 + 12 of 40 bytes per location; the map
  int* dev_want = reinterpret_cast<int*>(keys + nloc);
  int* dev_code = dev_want + 3 * nloc;
  float* dev_dir = reinterpret_cast<float*>(dev_code + nloc);
  int* dev_map = reinterpret_cast<int*>(keys + (size_t)nloc * 5);
  VH_HIP(hipMemsetAsync(keys, 0xff, sizeof(unsigned long long) * nloc, st));
  VH_TRY(to_dev(ctx, dev_want, want.data(), want.size()));
  nearest_kernel<<<grid_for(count, BLOCK * LINK_ITEMS), BLOCK, 0, st>>>(p, list, res, count, dev_want, nloc, keys);
  link_fetch_kernel<<<grid_for(nloc, BLOCK), BLOCK, 0, st>>>(nloc, keys, word, aux, d.V, dev_code, dev_dir);
  VH_HIP(hipGetLastError());
  std::vector<unsigned long long> host_keys((size_t)nloc);
  std::vector<int> host_code((size_t)nloc);
  std::vector<float> host_dir(3 * (size_t)nloc);
  VH_TRY(to_host(ctx, host_keys.data(), keys, (size_t)nloc));
  VH_TRY(to_host(ctx, host_code.data(), dev_code, (size_t)nloc));
  VH_TRY(to_host(ctx, host_dir.data(), dev_dir, 3 * (size_t)nloc));
  std::vector<LinkContact> contact((size_t)nloc);
  for (int l = 0; l < nloc; l++) {
    if (host_keys[(size_t)l] == NO_KEY || host_code[(size_t)l] < 0) return fail(VISFD_HIP_EDEVICE, "label_connected_graph: a must-link location found no labelled voxel");
    contact[(size_t)l].index = (int)(host_keys[(size_t)l] & 0x7fffffffull);
    contact[(size_t)l].code = host_code[(size_t)l];
    for (int a = 0; a < 3; a++) contact[(size_t)l].n[a] = host_dir[3 * (size_t)l + a];
  }
  std::vector<int> map;
  *reasons |= merge_links(c, p.standardize != 0, contact, nc, &map);
  if (*reasons) return VISFD_HIP_OK;
  // the survivors in rank order; the sizes and sums of what they absorbed
  std::vector<int> number(nc, -1);
  std::vector<int64_t> kept;
  for (size_t k = 0; k < nc; k++)
    if ((size_t)(map[k] >> 1) == k) { number[k] = (int)kept.size(); kept.push_back((*deepest)[k]); }
  std::vector<uint64_t> msizes(kept.size(), 0);
  std::vector<int64_t> msums(3 * kept.size(), 0);
  for (size_t k = 0; k < nc; k++) {
    const int to = number[(size_t)(map[k] >> 1)];
    msizes[(size_t)to] += (*sizes)[k];
    for (int a = 0; a < 3; a++) msums[3 * (size_t)to + a] += (*sums)[3 * k + a];
    map[k] = (to << 1) | (map[k] & 1);
  }
  VH_TRY(to_dev(ctx, dev_map, map.data(), nc));
  remap_kernel<<<grid_for(count, BLOCK), BLOCK, 0, st>>>(count, dev_map, res);
  VH_HIP(hipGetLastError());
  VH_HIP(hipMemsetAsync(cl, 0, 10 * nc * sizeof(unsigned long long), st));   // stage (e) lays the merged clusters out anew
  deepest->swap(kept);
  sizes->swap(msizes);
  sums->swap(msums);
  return VISFD_HIP_OK;
}

// The device path on device arrays.  c: the call (its array pointers are not looked at); the lists go to c's host arrays.
// *reasons != 0 on return: nothing final was written (labels hold the background fill), the caller hands over to the flood
// with `seed` / `score`.
// settle (option connect_settle): must-links, voxel weights and doubtful outward sums are no reasons; *settled gets the
// bits of those that this call dealt with itself.
int run_device(visfd_hip_ctx* ctx, const Call& c, const DevArrays& d, Clock& clk, std::vector<int>* seed,
               std::vector<float>* score, Last* last, unsigned* reasons, bool settle, unsigned* settled) {
  const Params p = make_params(c);
  *settled = 0;
  const bool weighted = settle && (d.W || d.W_host);
  const bool linked = settle && c.must_link_crds && c.must_link_ngroups > 0;
  const int64_t n = c.nx * c.ny * c.nz;
  hipStream_t st = ctx->stream;
  const bool minima = c.start_from_saliency_maxima == 0;
  VH_TRY(search_seeds(ctx, c, d.S, d.M, seed, score));
  const int64_t nseeds = (int64_t)seed->size();
  VH_TRY(clk.mark(MS_SEEDS));

  unsigned* word;
  int* aux;
  unsigned long long* counters;   // [0] classified, [1] listed, [2] the reason flags (low word)
  VH_TRY(ws(ctx, WS_CG_WORD, (size_t)n, &word));
  VH_TRY(ws(ctx, WS_CG_AUX, (size_t)n, &aux));
  VH_TRY(ws(ctx, WS_CG_COUNTERS, 4, &counters));
  unsigned* flags = reinterpret_cast<unsigned*>(counters + 2);
  VH_HIP(hipMemsetAsync(counters, 0, 4 * sizeof(unsigned long long), st));

  // (a)
  const unsigned sweep = grid_for((n + 3) / 4, BLOCK);
  const int vec = aligned16(d.S) && aligned16(d.M) && aligned16(d.labels);
  classify_kernel<<<sweep, BLOCK, 0, st>>>(p, d.S, d.M, d.T, word, d.labels, n, nseeds + 1, c.label_undefined, vec, counters);
  VH_HIP(hipGetLastError());
  unsigned long long count_u = 0;
  VH_TRY(to_host(ctx, &count_u, counters, 1));
  const int64_t count = (int64_t)count_u;
  int* list;
  float* rec = nullptr;
  unsigned* pass = nullptr;
  VH_TRY(ws(ctx, WS_CG_LIST, (size_t)(2 * count), &list));
  int* res = list + count;
  if (d.V) {
    VH_TRY(ws(ctx, WS_CG_REC, (size_t)(9 * count + (count + 31) / 32), &rec));
    pass = reinterpret_cast<unsigned*>(rec + 9 * count);
  }
  if (count > 0) {
    gather_kernel<<<sweep, BLOCK, 0, st>>>(p, d.S, d.V, word, n, list, aux, rec, rec ? rec + 6 * count : nullptr, count_u,
                                           counters);
    VH_HIP(hipGetLastError());
  }
  VH_TRY(clk.mark(MS_CLASSIFY));

  // (b)
  int64_t n_valid = count;
  last->n_undecided = 0;
  if (d.V && count > 0) {
    std::vector<float> host_rec((size_t)(9 * count));
    std::vector<unsigned> host_pass((size_t)((count + 31) / 32));
    VH_TRY(to_host(ctx, host_rec.data(), rec, host_rec.size()));
    VH_TRY(clk.mark(MS_COPY_OUT));
    vector_test(p, minima ? VISFD_HIP_INCREASING_EIVALS : VISFD_HIP_DECREASING_EIVALS, host_rec.data(),
                host_rec.data() + 6 * count, count, host_pass.data());
    n_valid = 0;
    for (size_t k = 0; k < host_pass.size(); k++) n_valid += __builtin_popcount(host_pass[k]);
    VH_TRY(clk.mark(MS_VECTOR));
    VH_TRY(to_dev(ctx, pass, host_pass.data(), host_pass.size()));
    VH_TRY(clk.mark(MS_COPY_IN));
    reject_kernel<<<grid_for(count, BLOCK), BLOCK, 0, st>>>(list, pass, count, word);
    VH_HIP(hipGetLastError());
    VH_TRY(clk.mark(MS_VECTOR));
    last->n_undecided = count;
  }
  last->n_valid = n_valid;

  // (c)
  if (count > 0) {
    edges_kernel<<<grid_for(count, BLOCK), BLOCK, 0, st>>>(p, d.T, d.V, list, count, word, flags);
    VH_HIP(hipGetLastError());
  }
  unsigned long long flag_word = 0;
  VH_TRY(to_host(ctx, &flag_word, counters + 2, 1));
  VH_TRY(clk.mark(MS_EDGES));
  *reasons = (unsigned)flag_word;
  if (nseeds >= ((int64_t)1 << 30)) *reasons |= VISFD_HIP_CONNECT_REASON_LIMITS;   // (number << 1) | sign is an int
  if (*reasons) return VISFD_HIP_OK;

  // (d)
  std::vector<int64_t> deepest, inv;
  std::vector<uint64_t> sizes;
  std::vector<int64_t> sums;
  int* dseed = nullptr;
  if (nseeds > 0 && count > 0) {
    VH_TRY(ws(ctx, WS_CG_SEEDS, (size_t)(4 * nseeds), &dseed));
    int *seed_root = dseed + nseeds, *seed_sign = dseed + 2 * nseeds, *code = dseed + 3 * nseeds;
    VH_TRY(to_dev(ctx, dseed, seed->data(), (size_t)nseeds));
    const unsigned g = grid_for(nseeds, BLOCK);
    seed_root_kernel<<<g, BLOCK, 0, st>>>(dseed, nseeds, word, aux, seed_root, seed_sign);
    seed_anchor_kernel<<<g, BLOCK, 0, st>>>(nseeds, aux, seed_root, seed_sign, code);
    VH_HIP(hipGetLastError());
    std::vector<int> host_code((size_t)nseeds);
    VH_TRY(to_host(ctx, host_code.data(), code, (size_t)nseeds));
    for (int64_t k = 0; k < nseeds; k++) {   // the anchors in rank order are the provisional clusters
      const bool anchor = host_code[(size_t)k] >= 0 && (host_code[(size_t)k] & 2);
      host_code[(size_t)k] = anchor ? (int)deepest.size() : -1;
      if (anchor) deepest.push_back(k);
    }
    VH_TRY(to_dev(ctx, code, host_code.data(), (size_t)nseeds));
    seed_number_kernel<<<g, BLOCK, 0, st>>>(nseeds, code, seed_root, seed_sign, aux);
    VH_HIP(hipGetLastError());
  }
  size_t nc = deepest.size();
  sizes.assign(nc, 0);
  sums.assign(3 * nc, 0);
  // per cluster: sizes | sums[3] (u64) | com[3] | sum (double) | final (int64) | B | any (unsigned)
  unsigned long long* cl = nullptr;
  if (nc > 0) {
    VH_TRY(ws(ctx, WS_CG_CLUSTER, 10 * nc, &cl));
    VH_HIP(hipMemsetAsync(cl, 0, 10 * nc * sizeof(unsigned long long), st));
    census_kernel<<<grid_for(count, BLOCK), BLOCK, 0, st>>>(p, list, count, word, aux, res, weighted ? nullptr : cl, cl + nc);
    VH_HIP(hipGetLastError());
    if (!weighted) {
      std::vector<unsigned long long> host_cl(4 * nc);
      VH_TRY(to_host(ctx, host_cl.data(), cl, 4 * nc));
      for (size_t k = 0; k < nc; k++) sizes[k] = host_cl[k];
      for (size_t k = 0; k < 3 * nc; k++) sums[k] = (int64_t)host_cl[nc + k];
    }
  }
  if (linked) {
    VH_TRY(settle_links(ctx, c, p, d, list, res, count, word, aux, cl, &deepest, &sizes, &sums, reasons));
    if (*reasons) return clk.mark(MS_CLUSTERS);
    *settled |= VISFD_HIP_CONNECT_REASON_MUST_LINK;
    nc = deepest.size();
  }
  VH_TRY(clk.mark(MS_CLUSTERS));

  // (e)
  std::vector<char> flip(nc, 0);
  std::vector<float> weight_sizes;
  if (weighted) {   // sizes, centres of mass and outward sums from the weights: the flood's statements over the labelled voxels
    std::vector<long double> wsize, wsum;
    std::vector<SettleVoxel> vox;
    VH_TRY(gather_for_host(ctx, d, list, res, count, nullptr, nc, (unsigned long long)count, counters + 3, &vox));
    settle_moments(c, &vox, nc, true, p.standardize != 0, &wsize, &wsum);
    weight_sizes.resize(nc);
    for (size_t k = 0; k < nc; k++) {
      weight_sizes[k] = (float)wsize[k];
      flip[k] = p.standardize && wsum[k] < 0.0L;
    }
    *settled |= VISFD_HIP_CONNECT_REASON_WEIGHTS;
  } else if (p.standardize && nc > 0) {
    double* com = reinterpret_cast<double*>(cl + 4 * nc);
    double* sum = reinterpret_cast<double*>(cl + 7 * nc);
    unsigned* B = reinterpret_cast<unsigned*>(cl + 9 * nc);
    unsigned* any = B + nc;
    std::vector<double> host_com(3 * nc);
    for (size_t k = 0; k < nc; k++)
      for (int a = 0; a < 3; a++) host_com[3 * k + a] = (double)((long double)sums[3 * k + a] / (long double)sizes[k]);
    VH_TRY(to_dev(ctx, com, host_com.data(), 3 * nc));
    outward_kernel<<<grid_for(count, BLOCK), BLOCK, 0, st>>>(p, d.V, list, res, count, com, sum, B, any);
    VH_HIP(hipGetLastError());
    std::vector<double> host_sum(nc);
    std::vector<unsigned> host_b(2 * nc);
    std::vector<size_t> doubtful;
    VH_TRY(to_host(ctx, host_sum.data(), sum, nc));
    VH_TRY(to_host(ctx, host_b.data(), B, 2 * nc));
    for (size_t k = 0; k < nc; k++) {
      if (!host_b[nc + k]) continue;   // every term an exact zero: the sum is an exact zero, no flip
      float bk;
      std::memcpy(&bk, &host_b[k], sizeof(float));
      // A device term differs from the flood's by less than 2^-21 B (r is rounded twice: one float ulp per component) and
      // the fp64 accumulation adds count * 2^-53: the sign is the flood's wherever |sum| > count * 2^-20 * B.
      if (!(std::fabs(host_sum[k]) > (double)sizes[k] * 9.5367431640625e-07 * (double)bk)) {
        if (settle) doubtful.push_back(k);
        else *reasons |= VISFD_HIP_CONNECT_REASON_OUTWARD;
      }
      flip[k] = host_sum[k] < 0.0;
    }
    if (*reasons) return clk.mark(MS_DIRECTIONS);
    if (!doubtful.empty()) {   // the flood's own sum for these clusters, from their voxels in raster order: no guard needed
      std::vector<unsigned char> wanted(nc, 0);
      unsigned long long cap = 0;
      for (size_t k : doubtful) { wanted[k] = 1; cap += sizes[k]; }
      std::vector<long double> fsize, fsum;
      std::vector<SettleVoxel> vox;
      VH_TRY(gather_for_host(ctx, d, list, res, count, wanted.data(), nc, cap, counters + 3, &vox));
      settle_moments(c, &vox, nc, false, true, &fsize, &fsum);
      for (size_t k : doubtful) flip[k] = fsum[k] < 0.0L;
      *settled |= VISFD_HIP_CONNECT_REASON_OUTWARD;
    }
  }
  const int rc = weighted ? finish_lists(c, *seed, *score, deepest, weight_sizes, &inv)
                          : finish_lists(c, *seed, *score, deepest, sizes, &inv);
  if (nc > 0) {
    int64_t* final = reinterpret_cast<int64_t*>(cl + 8 * nc);
    std::vector<int64_t> host_final(nc);
    for (size_t k = 0; k < nc; k++) host_final[k] = ((inv[k] + 1) << 1) | (int64_t)flip[k];
    VH_TRY(to_dev(ctx, final, host_final.data(), nc));
    write_kernel<<<grid_for(count, BLOCK), BLOCK, 0, st>>>(list, res, count, final, p.standardize, d.labels, d.V);
    VH_HIP(hipGetLastError());
  }
  VH_HIP(hipStreamSynchronize(st));
  VH_TRY(clk.mark(MS_DIRECTIONS));
  return rc;
}

int record(visfd_hip_ctx* ctx, const Last& last, unsigned settled = 0) {
  ctx->connect_graph_settled = last.path == VISFD_HIP_CONNECT_GRAPH_DEVICE ? settled : 0;
  ctx->connect_graph[0] = last.path;
  ctx->connect_graph[1] = (int64_t)last.reasons;
  ctx->connect_graph[2] = last.n_valid;
  ctx->connect_graph[3] = last.n_undecided;
  return VISFD_HIP_OK;
}

// the image and the connectivity are within the reach of the device's seed search (extrema.hip)
bool search_fits(const Call& c) {
  return c.connectivity <= VISFD_HIP_EXTREMA_MAX_CONNECTIVITY && c.nx * c.ny * c.nz <= VISFD_HIP_EXTREMA_MAX_VOXELS &&
         c.ny <= VISFD_HIP_EXTREMA_MAX_NY_NZ && c.nz <= VISFD_HIP_EXTREMA_MAX_NY_NZ &&
         tile_count(c.nx, c.ny, c.nz) < ((i64)1 << 24);
}
unsigned reasons_before_work(const Call& c, bool settle) {
  unsigned r = early_reasons(c, true);
  if (settle) {   // option connect_settle: no reasons, but the device's nearest-voxel search has its reach
    r &= ~(unsigned)(VISFD_HIP_CONNECT_REASON_MUST_LINK | VISFD_HIP_CONNECT_REASON_WEIGHTS);
    std::vector<int> want;
    r |= link_locations(c, &want);
  }
  if (!search_fits(c)) r |= VISFD_HIP_CONNECT_REASON_LIMITS;
  return r;
}
int search_seeds(visfd_hip_ctx* ctx, const Call& c, const float* dev_saliency, const float* dev_mask, std::vector<int>* seed,
                 std::vector<float>* score) {
  const bool minima = c.start_from_saliency_maxima == 0;
  float thr = c.threshold_saliency;   // morphology_implementation.hpp:774-775: no threshold for maxima is -infinity
  if (!minima && thr == std::numeric_limits<float>::infinity()) thr = -std::numeric_limits<float>::infinity();
  return dev_extrema_seeds(ctx, dev_saliency, dev_mask, c.nx, c.ny, c.nz, minima, thr, c.connectivity, seed, score);
}

}  // namespace
}  // namespace cg
}  // namespace vh

using namespace vh;
using namespace vh::cg;

extern "C" {

int visfd_hip_label_connected_graph(visfd_hip_ctx* ctx, const float* saliency, int64_t* labels, const float* mask, int64_t nx,
                                    int64_t ny, int64_t nz, float threshold_saliency, float* direction,
                                    float threshold_vector_saliency, float threshold_vector_neighbor,
                                    int consider_dot_product_sign, const float* tensor, float threshold_tensor_saliency,
                                    float threshold_tensor_neighbor, int tensor_is_positive_definite_near_target,
                                    int connectivity, int64_t label_undefined, int sort_by_size, int standardize_directions,
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
  Last last;
  const bool settle = ctx->opt.connect_settle != 0;
  unsigned settled = 0;
  unsigned reasons = reasons_before_work(c, settle);
  VH_HIP(hipSetDevice(ctx->device));
  const size_t n = (size_t)(nx * ny * nz);
  const Stage stg = {ctx, n};
  float *ds, *dm, *dv, *dt;
  int64_t* dl;
  std::vector<int> seed;
  std::vector<float> score;
  if (reasons) {   // known before any work starts: the flood as visfd_hip_label_connected_device_seeds runs it
    const bool on_device = search_fits(c);
    if (on_device) {
      VH_TRY(stg.up(WS_H2D_0, saliency, &ds));
      VH_TRY(stg.up(WS_H2D_1, mask, &dm));
      VH_TRY(search_seeds(ctx, c, ds, dm, &seed, &score));
    }
    const int frc = flood_keeping_unlabelled(c, on_device ? &seed : nullptr, on_device ? &score : nullptr);
    if (frc != VISFD_HIP_OK && frc != VISFD_HIP_ECAPACITY) return frc;
    last.path = VISFD_HIP_CONNECT_GRAPH_FLOOD;
    last.reasons = reasons;
    record(ctx, last);
    return frc;
  }
  Clock clk = {ctx, ctx->opt.connect_time != 0, {}};
  VH_TRY(clk.start());
  VH_TRY(stg.up(WS_H2D_0, saliency, &ds));
  VH_TRY(stg.up(WS_H2D_1, mask, &dm));
  VH_TRY(stg.up(WS_H2D_2, direction, &dv, 3));
  VH_TRY(stg.up(WS_H2D_3, tensor, &dt, 6));
  VH_TRY(ws(ctx, WS_H2D_4, n, &dl));
  VH_TRY(clk.mark(MS_COPY_IN));
  const DevArrays d = {ds, dm, dv, dt, dl, nullptr, voxel_weights};
  const int rc = run_device(ctx, c, d, clk, &seed, &score, &last, &reasons, settle, &settled);
  if (rc != VISFD_HIP_OK && rc != VISFD_HIP_ECAPACITY) return rc;
  if (reasons) {
    const int frc = flood_keeping_unlabelled(c, &seed, &score);
    if (frc != VISFD_HIP_OK && frc != VISFD_HIP_ECAPACITY) return frc;
    last.path = VISFD_HIP_CONNECT_GRAPH_FLOOD;
    last.reasons = reasons;
    record(ctx, last);
    return frc;
  }
  VH_HIP(hipMemcpyAsync(labels, dl, sizeof(int64_t) * n, hipMemcpyDeviceToHost, ctx->stream));
  if (direction && standardize_directions && !consider_dot_product_sign)
    VH_HIP(hipMemcpyAsync(direction, dv, sizeof(float) * 3 * n, hipMemcpyDeviceToHost, ctx->stream));
  VH_HIP(hipStreamSynchronize(ctx->stream));
  VH_TRY(clk.mark(MS_COPY_OUT));
  last.path = VISFD_HIP_CONNECT_GRAPH_DEVICE;
  record(ctx, last, settled);
  return rc;
}

int visfd_hip_label_connected_graph_dev(visfd_hip_ctx* ctx, const float* saliency, int64_t* labels, const float* mask,
                                        int64_t nx, int64_t ny, int64_t nz, float threshold_saliency, float* direction,
                                        float threshold_vector_saliency, float threshold_vector_neighbor,
                                        int consider_dot_product_sign, const float* tensor, float threshold_tensor_saliency,
                                        float threshold_tensor_neighbor, int tensor_is_positive_definite_near_target,
                                        int connectivity, int64_t label_undefined, int sort_by_size,
                                        int standardize_directions, int start_from_saliency_maxima, int64_t* n_clusters,
                                        float* cluster_maxima, float* cluster_sizes, float* cluster_saliencies,
                                        int64_t cluster_capacity, const float* voxel_weights, const float* must_link_crds,
                                        const int64_t* must_link_group_sizes, int64_t must_link_ngroups,
                                        const int* must_link_directions) {
  VH_REQUIRE(ctx, "null context");
  VH_TRY(label_connected_check_args(saliency, labels, nx, ny, nz, connectivity));   // before any allocation
  Call c = {saliency, labels, mask, nx, ny, nz, threshold_saliency, direction, threshold_vector_saliency,
            threshold_vector_neighbor, consider_dot_product_sign, tensor, threshold_tensor_saliency, threshold_tensor_neighbor,
            tensor_is_positive_definite_near_target, connectivity, label_undefined, sort_by_size, standardize_directions,
            start_from_saliency_maxima, n_clusters, cluster_maxima, cluster_sizes, cluster_saliencies, cluster_capacity,
            voxel_weights, must_link_crds, must_link_group_sizes, must_link_ngroups, must_link_directions};
  VH_HIP(hipSetDevice(ctx->device));
  Clock clk = {ctx, ctx->opt.connect_time != 0, {}};
  VH_TRY(clk.start());
  Last last;
  std::vector<int> seed;
  std::vector<float> score;
  const bool settle = ctx->opt.connect_settle != 0;
  unsigned settled = 0;
  unsigned reasons = reasons_before_work(c, settle);
  int rc = VISFD_HIP_OK;
  bool have_seeds = false;
  if (reasons) {
    if ((have_seeds = search_fits(c))) VH_TRY(search_seeds(ctx, c, saliency, mask, &seed, &score));
  } else {
    have_seeds = true;
    const DevArrays d = {saliency, mask, direction, tensor, labels, voxel_weights, nullptr};
    rc = run_device(ctx, c, d, clk, &seed, &score, &last, &reasons, settle, &settled);
    if (rc != VISFD_HIP_OK && rc != VISFD_HIP_ECAPACITY) return rc;
    if (!reasons) {
      last.path = VISFD_HIP_CONNECT_GRAPH_DEVICE;
      record(ctx, last, settled);
      return rc;
    }
  }
  // the flood on a staged copy (voxel weights, where given, are a device array like the image)
  const size_t n = (size_t)(nx * ny * nz);
  std::vector<float> hs(n), hm, hv, ht, hw;
  std::vector<int64_t> hl(n);
  VH_HIP(hipMemcpyAsync(hs.data(), saliency, sizeof(float) * n, hipMemcpyDeviceToHost, ctx->stream));
  if (mask) { hm.resize(n); VH_HIP(hipMemcpyAsync(hm.data(), mask, sizeof(float) * n, hipMemcpyDeviceToHost, ctx->stream)); }
  if (direction) { hv.resize(3 * n); VH_HIP(hipMemcpyAsync(hv.data(), direction, sizeof(float) * 3 * n, hipMemcpyDeviceToHost, ctx->stream)); }
  if (tensor) { ht.resize(6 * n); VH_HIP(hipMemcpyAsync(ht.data(), tensor, sizeof(float) * 6 * n, hipMemcpyDeviceToHost, ctx->stream)); }
  if (voxel_weights) { hw.resize(n); VH_HIP(hipMemcpyAsync(hw.data(), voxel_weights, sizeof(float) * n, hipMemcpyDeviceToHost, ctx->stream)); }
  VH_HIP(hipStreamSynchronize(ctx->stream));
  c.saliency = hs.data();
  c.labels = hl.data();
  c.mask = mask ? hm.data() : nullptr;
  c.direction = direction ? hv.data() : nullptr;
  c.tensor = tensor ? ht.data() : nullptr;
  c.voxel_weights = voxel_weights ? hw.data() : nullptr;
  const int frc = flood_keeping_unlabelled(c, have_seeds ? &seed : nullptr, have_seeds ? &score : nullptr);
  if (frc != VISFD_HIP_OK && frc != VISFD_HIP_ECAPACITY) return frc;
  VH_HIP(hipMemcpyAsync(labels, hl.data(), sizeof(int64_t) * n, hipMemcpyHostToDevice, ctx->stream));
  if (direction) VH_HIP(hipMemcpyAsync(direction, hv.data(), sizeof(float) * 3 * n, hipMemcpyHostToDevice, ctx->stream));
  VH_HIP(hipStreamSynchronize(ctx->stream));
  last.path = VISFD_HIP_CONNECT_GRAPH_FLOOD;
  last.reasons = reasons;
  record(ctx, last);
  return frc;
}

int visfd_hip_label_connected_graph_last(visfd_hip_ctx* ctx, int* path, unsigned* reasons, int64_t* n_valid,
                                         int64_t* n_undecided) {
  VH_REQUIRE(path, "null argument");
  Last last;
  if (ctx) {
    last.path = (int)ctx->connect_graph[0];
    last.reasons = (unsigned)ctx->connect_graph[1];
    last.n_valid = ctx->connect_graph[2];
    last.n_undecided = ctx->connect_graph[3];
  } else {
    last = host_last();
  }
  *path = last.path;
  if (reasons) *reasons = last.reasons;
  if (n_valid) *n_valid = last.n_valid;
  if (n_undecided) *n_undecided = last.n_undecided;
  return VISFD_HIP_OK;
}

int visfd_hip_label_connected_graph_last_settled(visfd_hip_ctx* ctx, unsigned* settled) {
  VH_REQUIRE(ctx && settled, "null argument");
  *settled = ctx->connect_graph_settled;
  return VISFD_HIP_OK;
}

int visfd_hip_label_connected_graph_last_times(visfd_hip_ctx* ctx, float ms[8]) {
  VH_REQUIRE(ctx && ms, "null argument");
  for (int k = 0; k < 8; k++) ms[k] = ctx->connect_graph_ms[k];
  return VISFD_HIP_OK;
}

}  // extern "C"
