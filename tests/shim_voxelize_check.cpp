// VoxelizeMesh of the C++ drop-in (include/visfd_hip.hpp) on the off-grid box of tests/voxelize_cases.py in a 20 x 17 x 13
// image: prints the number of inside voxels (13 * 13 * 6 = 1014), the same box in physical units with an origin, and checks
// that the box without one face is refused unless check_closed is off.  tests/test_voxelize.py compiles it with
// -Wall -Werror, tests/test_voxelize_gpu.py runs it.
#include <array>
#include <cstdio>
#include <vector>

#include "visfd_hip.hpp"

using namespace visfd;
using std::array;
using std::vector;

static long count(float*** a, const int size[3]) {
  long n = 0;
  for (int iz = 0; iz < size[2]; iz++)
    for (int iy = 0; iy < size[1]; iy++)
      for (int ix = 0; ix < size[0]; ix++) {
        if (a[iz][iy][ix] != 0.0f && a[iz][iy][ix] != 1.0f) return -1;
        n += a[iz][iy][ix] == 1.0f;
      }
  return n;
}

int main() {
  const int size[3] = {20, 17, 13};
  const float lo[3] = {2.3f, 1.7f, 3.1f}, hi[3] = {15.6f, 14.2f, 9.9f};
  vector<array<float, 3> > v;
  for (int i = 0; i < 8; i++) v.push_back(array<float, 3>{{i & 1 ? hi[0] : lo[0], i & 2 ? hi[1] : lo[1], i & 4 ? hi[2] : lo[2]}});
  const int quads[6][4] = {{0, 2, 6, 4}, {1, 5, 7, 3}, {0, 4, 5, 1}, {2, 3, 7, 6}, {0, 1, 3, 2}, {4, 6, 7, 5}};
  vector<array<int, 3> > t;
  for (int f = 0; f < 6; f++) {
    t.push_back(array<int, 3>{{quads[f][0], quads[f][1], quads[f][2]}});
    t.push_back(array<int, 3>{{quads[f][0], quads[f][2], quads[f][3]}});
  }
  float*** dest = Alloc3D<float>(size);
  VoxelizeMesh(nullptr, size, v, t, dest);
  std::printf("inside %ld\n", count(dest, size));

  // the same box moved by one voxel along x through the origin, in units of half a voxel
  vector<array<float, 3> > v2(v);
  for (size_t i = 0; i < v2.size(); i++)
    for (int d = 0; d < 3; d++) v2[i][d] *= 0.5f;
  const double origin[3] = {1.0, 0.0, 0.0};
  VoxelizeMesh(nullptr, size, v2, t, dest, 0.5, origin);
  std::printf("shifted inside %ld first %d\n", count(dest, size), (int)dest[4][2][2]);

  vector<array<int, 3> > open(t.begin(), t.begin() + 2);
  open.insert(open.end(), t.begin() + 4, t.end());
  bool refused = false;
  try { VoxelizeMesh(nullptr, size, v, open, dest); } catch (VisfdErr&) { refused = true; }
  if (!refused) return 7;
  VoxelizeMesh(nullptr, size, v, open, dest, 1.0, nullptr, false);
  int64_t stats[4];
  if (visfd_hip_voxelize_last(hip_detail::context(), stats) != VISFD_HIP_OK) return 8;
  std::printf("open odd rows %ld\n", (long)stats[2]);
  Dealloc3D(dest);
  std::printf("shim voxelize check ok\n");
  return 0;
}
