// union_find.hpp -- the lock-free union-find over voxel indices that the plateau search (extrema.hip) and the watershed
// (watershed.hip) share.  parent[] holds one int per voxel; a root points at itself.  Roots are hooked with atomicMin towards
// the smaller linear index, so a set's surviving representative is its first voxel in raster order.  Parent pointers only
// ever decrease, so there are no cycles, and a pointer read late (another CU's L1 is not refreshed) is an older link of
// the same final set: finds still terminate and unions still end in one tree.
#pragma once

#include <hip/hip_runtime.h>

namespace vh {

__device__ __forceinline__ int ld_parent(const int* p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// the root of x's tree; every second link on the way is shortened to its grandparent (atomicMin: a link only ever moves
// to a smaller index, and never away from a smaller one that a concurrent hook has just put there)
__device__ __forceinline__ int find_halving(int* parent, int x) {
  for (;;) {
    const int p = ld_parent(parent + x);
    if (p == x) return x;
    const int gp = ld_parent(parent + p);
    if (gp == p) return p;
    atomicMin(parent + x, gp);
    x = gp;
  }
}

__device__ __forceinline__ void unite(int* parent, int a, int b) {
  for (;;) {
    a = find_halving(parent, a);
    b = find_halving(parent, b);
    if (a == b) return;
    if (a < b) {
      const int t = a;
      a = b;
      b = t;
    }
    const int old = atomicMin(parent + a, b);   // a > b: hook a under b if a still is a root
    if (old == a) return;
    a = old;   // a had a parent already (now min(old, b)): what is left to join is old's tree and b's
  }
}

}  // namespace vh
