// The median functions of the C++ drop-in (include/visfd_hip.hpp), called with the reference's signatures
// (lib/visfd/filter3d.hpp:1577-1674).  Reads DIR/in.bin (nx ny nz, then src, mask, dest0 as float32 volumes), writes
// DIR/out.bin: one record per call (32-byte tag, int64 count, floats); tests/test_median_gpu.py checks them.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <iostream>
#include <string>
#include <tuple>
#include <vector>

#include "visfd_hip.hpp"

using namespace visfd;

static void put(FILE* f, const char* tag, float*** a, size_t n) {
  char t[32] = {0};
  std::strncpy(t, tag, 31);
  const int64_t m = (int64_t)n;
  std::fwrite(t, 1, 32, f);
  std::fwrite(&m, 8, 1, f);
  std::fwrite(&a[0][0][0], 4, n, f);
}

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  const std::string dir = argv[1];
  FILE* in = std::fopen((dir + "/in.bin").c_str(), "rb");
  if (!in) return 3;
  int size[3];
  if (std::fread(size, 4, 3, in) != 3) return 4;
  const size_t n = (size_t)size[0] * size[1] * size[2];
  float*** src = Alloc3D<float>(size);
  float*** mask = Alloc3D<float>(size);
  float*** dest0 = Alloc3D<float>(size);
  float*** dest = Alloc3D<float>(size);
  if (std::fread(&src[0][0][0], 4, n, in) != n || std::fread(&mask[0][0][0], 4, n, in) != n ||
      std::fread(&dest0[0][0][0], 4, n, in) != n)
    return 5;
  std::fclose(in);
  FILE* out = std::fopen((dir + "/out.bin").c_str(), "wb");
  if (!out) return 6;
  auto fresh = [&]() { std::memcpy(&dest[0][0][0], &dest0[0][0][0], 4 * n); };
  fresh(); MedianSphere(2.5f, size, src, dest);                  put(out, "sphere", dest, n);
  fresh(); MedianSphere(1.5f, size, src, dest, mask);            put(out, "sphere_mask", dest, n);
  fresh(); MedianSphere(2.0f, size, src, dest, mask, &std::cerr); put(out, "sphere_mask_report", dest, n);
  std::vector<std::tuple<int, int, int> > fp;
  fp.push_back(std::make_tuple(0, 0, 0));
  fp.push_back(std::make_tuple(2, -1, 0));
  fp.push_back(std::make_tuple(2, -1, 0));
  fp.push_back(std::make_tuple(-1, 0, 1));
  fp.push_back(std::make_tuple(0, 3, -2));
  fresh(); Median(fp, size, src, dest);                          put(out, "table", dest, n);
  fresh(); Median(fp, size, src, dest, mask);                    put(out, "table_mask", dest, n);
  std::fclose(out);
  Dealloc3D(src); Dealloc3D(mask); Dealloc3D(dest0); Dealloc3D(dest);
  std::printf("shim median check ok\n");
  return 0;
}
