// DrawSpheres and DrawRegions of the C++ drop-in (include/visfd_hip.hpp), called with the reference's signatures and
// default arguments (lib/visfd/draw.hpp:46-81, :90-95, :238-251).  Reads DIR/in.bin (nx ny nz, then image and mask as float32
// volumes), writes DIR/out.bin: one record per result (32-byte tag, int64 count, floats) and DIR/progress.txt (the
// pReportProgress text); tests/test_draw_gpu.py compares them with the numpy restatement.
#include <array>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <string>
#include <vector>

#include "visfd_hip.hpp"

using namespace visfd;
using std::array;
using std::vector;

static void put(FILE* f, const char* tag, const float* a, size_t n) {
  char t[32] = {0};
  std::strncpy(t, tag, 31);
  const int64_t m = (int64_t)n;
  std::fwrite(t, 1, 32, f);
  std::fwrite(&m, 8, 1, f);
  std::fwrite(a, 4, n, f);
}

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  const std::string dir = argv[1];
  FILE* in = std::fopen((dir + "/in.bin").c_str(), "rb");
  if (!in) return 3;
  int size[3];
  if (std::fread(size, 4, 3, in) != 3) return 4;
  const size_t n = (size_t)size[0] * size[1] * size[2];
  float*** image = Alloc3D<float>(size);
  float*** mask = Alloc3D<float>(size);
  float*** dest = Alloc3D<float>(size);
  if (std::fread(&image[0][0][0], 4, n, in) != n || std::fread(&mask[0][0][0], 4, n, in) != n) return 5;
  std::fclose(in);
  FILE* out = std::fopen((dir + "/out.bin").c_str(), "wb");
  if (!out) return 6;
  std::ofstream progress((dir + "/progress.txt").c_str());

  vector<array<float, 3> > centers;
  const float c[5][3] = {{4.2f, 5.0f, 6.9f}, {9.0f, 8.0f, 3.0f}, {-0.7f, 3.0f, 4.0f}, {30.0f, 3.0f, 4.0f}, {7.5f, 6.1f, 7.0f}};
  for (int i = 0; i < 5; i++) centers.push_back(array<float, 3>{{c[i][0], c[i][1], c[i][2]}});
  vector<float> diameters, thicknesses, scores;
  const float d[5] = {7.0f, 0.0f, 5.0f, 6.0f, 6.0f}, th[5] = {1.0f, 1.0f, 9.0f, 1.0f, 0.0f}, s[5] = {1.5f, -2.0f, 3.0f, 4.0f, 5.5f};
  diameters.assign(d, d + 5); thicknesses.assign(th, th + 5); scores.assign(s, s + 5);

  // every default argument but the background: single voxels of brightness 1
  DrawSpheres<float>(size, dest, nullptr, centers, nullptr, nullptr, nullptr, image);
  put(out, "defaults", &dest[0][0][0], n);
  // every argument, with the progress text and the outside-the-image warning
  DrawSpheres(size, dest, mask, centers, &diameters, &thicknesses, &scores, image, 0.25f, 0.5f, true, true, &progress);
  put(out, "all_arguments", &dest[0][0][0], n);
  // in place, diameters only
  std::memcpy(&dest[0][0][0], &image[0][0][0], 4 * n);
  DrawSpheres<float>(size, dest, nullptr, centers, &diameters, nullptr, nullptr, dest, 1.0f);
  put(out, "in_place", &dest[0][0][0], n);
  // a null background is an error, not a crash
  bool refused = false;
  try { DrawSpheres<float>(size, dest, nullptr, centers); } catch (VisfdErr&) { refused = true; }
  if (!refused) return 7;

  SimpleRegion<float> empty;   // the default region: an inverted rectangle of value 1
  if (empty.type != SimpleRegion<float>::RECT || empty.value != 1 || empty.data.rect.xmax != -1) return 8;
  vector<SimpleRegion<float> > regions;
  SimpleRegion<float> r;
  r.type = SimpleRegion<float>::SPHERE; r.value = -1;
  r.data.sphere.x0 = 6; r.data.sphere.y0 = 6; r.data.sphere.z0 = 5; r.data.sphere.r = 3.5f;
  regions.push_back(r);
  regions.push_back(empty);
  r.type = SimpleRegion<float>::RECT; r.value = 2.5f;
  r.data.rect.xmin = 1; r.data.rect.xmax = 4.4f; r.data.rect.ymin = 0; r.data.rect.ymax = 30; r.data.rect.zmin = 2; r.data.rect.zmax = 3;
  regions.push_back(r);
  std::memset(&dest[0][0][0], 0, 4 * n);
  DrawRegions(size, dest, static_cast<const float* const* const*>(nullptr), regions, true);   // as filter_mrc.cpp:280 calls it
  put(out, "regions_subtract", &dest[0][0][0], n);
  std::memcpy(&dest[0][0][0], &image[0][0][0], 4 * n);
  DrawRegions<float>(size, dest, mask, regions);                                               // the default: no subtraction
  put(out, "regions_default", &dest[0][0][0], n);

  std::fclose(out);
  Dealloc3D(image); Dealloc3D(mask); Dealloc3D(dest);
  std::printf("shim draw check ok\n");
  return 0;
}
