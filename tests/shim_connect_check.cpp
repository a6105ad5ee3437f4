// Compiled and run by tests/test_connect_gpu.py: LabelConnected through the reference's signature (host) and
// LabelConnectedDeviceSeeds (seeds searched on a context's device) must give the same labels, lists and directions.
#include <cmath>
#include <cstdio>
#include <cstring>

#include "visfd_hip.hpp"

using namespace visfd;

int main() {
  int size[3] = {70, 20, 12};   // crosses the 64-voxel tile edge of the device search
  const size_t n = (size_t)size[0] * size[1] * size[2];
  float*** sal = Alloc3D<float>(size);
  ptrdiff_t*** lab_host = Alloc3D<ptrdiff_t>(size);
  ptrdiff_t*** lab_ctx = Alloc3D<ptrdiff_t>(size);
  std::array<float, 3>*** dir = Alloc3D<std::array<float, 3> >(size);
  std::array<float, 3>*** std_host = Alloc3D<std::array<float, 3> >(size);
  std::array<float, 3>*** std_ctx = Alloc3D<std::array<float, 3> >(size);
  unsigned s = 12345u;
  for (int z = 0; z < size[2]; z++)
    for (int y = 0; y < size[1]; y++)
      for (int x = 0; x < size[0]; x++) {
        s = s * 1664525u + 1013904223u;
        const bool sheet = (z == 3 || z == 8) && y > 1 && y < 18 && x > 1;
        sal[z][y][x] = sheet ? 2.0f + (float)((s >> 8) % 5) : 0.0f;   // five levels: plateaus, some across the tile edge
        const float sign = (s & 0x80000u) ? -1.0f : 1.0f;              // the arbitrary sign of an eigenvector
        dir[z][y][x] = {{0.1f * sign, 0.0f, sign}};
      }
  std::vector<std::array<float, 3> > cm_host, cm_ctx;
  std::vector<float> cs_host, cs_ctx, csal_host, csal_ctx;
  const float ninf = -std::numeric_limits<float>::infinity();
  const size_t k_host = LabelConnected(size, sal, lab_host, nullptr, 1.0f, dir, ninf, 0.5f, false, nullptr, ninf, ninf, true, 2,
                                       (ptrdiff_t)-1, &cm_host, &cs_host, &csal_host, SORT_BY_SIZE, nullptr, std_host);
  visfd_hip_ctx* ctx = hip_detail::context();
  const size_t k_ctx = LabelConnectedDeviceSeeds(ctx, size, sal, lab_ctx, nullptr, 1.0f, dir, ninf, 0.5f, false, nullptr, ninf,
                                                 ninf, true, 2, (ptrdiff_t)-1, &cm_ctx, &cs_ctx, &csal_ctx, SORT_BY_SIZE,
                                                 nullptr, std_ctx);
  int where = -1;
  int64_t seeds = -1;
  hip_detail::check(visfd_hip_label_connected_device_seeds_last(ctx, &where, &seeds));
  std::printf("clusters %zu %zu seeds searched %d found %lld\n", k_host, k_ctx, where, (long long)seeds);
  if (k_host != 2 || k_ctx != k_host) return 1;
  if (where != VISFD_HIP_CONNECT_SEEDS_DEVICE || seeds < 2) return 2;
  if (std::memcmp(&lab_host[0][0][0], &lab_ctx[0][0][0], n * sizeof(ptrdiff_t)) != 0) return 3;
  if (std::memcmp(&std_host[0][0][0], &std_ctx[0][0][0], n * 3 * sizeof(float)) != 0) return 4;
  if (cm_host != cm_ctx || cs_host != cs_ctx || csal_host != csal_ctx) return 5;
  std::printf("shim connect check ok\n");
  return 0;
}
