// Compiled and run by tests/test_connect_graph_contract.py (no GPU): LabelConnectedGraph with a null context -- the serial
// host walk of visfd_hip_label_connected_graph_host -- against the reference-signature LabelConnected (the flood).  Labels,
// lists and the directions of labelled voxels must be the flood's bits, the directions of all other voxels the input's;
// a call with a must-link must be handed to the flood and say so.
#include <cmath>
#include <cstdio>
#include <cstring>

#include "visfd_hip.hpp"

using namespace visfd;

int main() {
  int size[3] = {70, 20, 12};
  const size_t n = (size_t)size[0] * size[1] * size[2];
  float*** sal = Alloc3D<float>(size);
  ptrdiff_t*** lab_flood = Alloc3D<ptrdiff_t>(size);
  ptrdiff_t*** lab_graph = Alloc3D<ptrdiff_t>(size);
  std::array<float, 3>*** dir = Alloc3D<std::array<float, 3> >(size);
  std::array<float, 3>*** std_flood = Alloc3D<std::array<float, 3> >(size);
  std::array<float, 3>*** std_graph = Alloc3D<std::array<float, 3> >(size);
  unsigned s = 12345u;
  for (int z = 0; z < size[2]; z++)
    for (int y = 0; y < size[1]; y++)
      for (int x = 0; x < size[0]; x++) {
        s = s * 1664525u + 1013904223u;
        const bool sheet = (z == 3 || z == 8) && y > 1 && y < 18 && x > 1;
        sal[z][y][x] = sheet ? 2.0f + (float)((s >> 8) % 5) : 0.0f;   // five levels: plateaus and many seeds per sheet
        const float sign = (s & 0x80000u) ? -1.0f : 1.0f;              // the arbitrary sign of an eigenvector
        // normals that fan out from a line far below the sheets, so that a sheet's outward sum is far from zero
        const float fx = 0.02f * (float)(x - 35), fy = 0.02f * (float)(y - 10);
        dir[z][y][x] = {{fx * sign, fy * sign, sign}};
      }
  const float ninf = -std::numeric_limits<float>::infinity();
  for (int round = 0; round < 2; round++) {
    std::vector<std::vector<std::array<float, 3> > > must_link;
    if (round == 1) must_link.push_back({{{10.0f, 5.0f, 3.0f}}, {{40.0f, 12.0f, 8.0f}}});   // joins the two sheets
    std::vector<std::array<float, 3> > cm_flood, cm_graph;
    std::vector<float> cs_flood, cs_graph, csal_flood, csal_graph;
    const size_t k_flood = LabelConnected(size, sal, lab_flood, nullptr, 1.0f, dir, ninf, 0.5f, false, nullptr, ninf, ninf, true,
                                          2, (ptrdiff_t)-1, &cm_flood, &cs_flood, &csal_flood, SORT_BY_SIZE, nullptr, std_flood,
                                          round ? &must_link : nullptr);
    const size_t k_graph = LabelConnectedGraph(nullptr, size, sal, lab_graph, nullptr, 1.0f, dir, ninf, 0.5f, false, nullptr,
                                               ninf, ninf, true, 2, (ptrdiff_t)-1, &cm_graph, &cs_graph, &csal_graph,
                                               SORT_BY_SIZE, nullptr, std_graph, round ? &must_link : nullptr);
    int path = -1;
    unsigned reasons = 0;
    int64_t n_valid = -1, n_undecided = -1;
    hip_detail::check(visfd_hip_label_connected_graph_last(nullptr, &path, &reasons, &n_valid, &n_undecided));
    std::printf("round %d: clusters %zu %zu path %d reasons %u valid %lld undecided %lld\n", round, k_flood, k_graph, path,
                reasons, (long long)n_valid, (long long)n_undecided);
    if (k_flood != (round ? 1u : 2u) || k_graph != k_flood) return 1;
    if (round == 0 && (path != VISFD_HIP_CONNECT_GRAPH_HOST_GRAPH || reasons != 0 || n_valid != n_undecided || n_valid < 2000)) return 2;
    if (round == 1 && (path != VISFD_HIP_CONNECT_GRAPH_FLOOD || reasons != VISFD_HIP_CONNECT_REASON_MUST_LINK)) return 2;
    if (std::memcmp(&lab_flood[0][0][0], &lab_graph[0][0][0], n * sizeof(ptrdiff_t)) != 0) return 3;
    if (cm_flood != cm_graph || cs_flood != cs_graph || csal_flood != csal_graph) return 4;
    size_t halo = 0;
    for (int z = 0; z < size[2]; z++)
      for (int y = 0; y < size[1]; y++)
        for (int x = 0; x < size[0]; x++) {
          const bool labelled = lab_flood[z][y][x] != -1;
          const std::array<float, 3>& want = labelled ? std_flood[z][y][x] : dir[z][y][x];
          if (std::memcmp(&want, &std_graph[z][y][x], sizeof(want)) != 0) return 5;
          if (!labelled && std::memcmp(&std_flood[z][y][x], &dir[z][y][x], sizeof(want)) != 0) halo++;
        }
    std::printf("round %d: the flood turned %zu unlabelled voxels, the graph entry none\n", round, halo);
  }
  Dealloc3D(sal);
  Dealloc3D(lab_flood);
  Dealloc3D(lab_graph);
  Dealloc3D(dir);
  Dealloc3D(std_flood);
  Dealloc3D(std_graph);
  std::printf("shim connect graph check ok\n");
  return 0;
}
