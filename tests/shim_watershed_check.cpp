// visfd::Watershed of the C++ drop-in (include/visfd_hip.hpp), called with the reference's signature and defaults
// (lib/visfd/segmentation.hpp:65-82).  Reads DIR/in.bin (nx ny nz, then src, mask and markers as float32 volumes), writes
// DIR/out.bin: one record per result (32-byte tag, int64 count, doubles -- every label, coordinate and float score is exact
// in a double); tests/test_watershed_gpu.py checks them against the sequential flood.
#include <array>
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <iostream>
#include <limits>
#include <string>
#include <vector>

#include "visfd_hip.hpp"

using namespace visfd;

template <typename T>
static void put(FILE* f, const std::string& tag, const std::vector<T>& v) {
  char t[32] = {0};
  std::strncpy(t, tag.c_str(), 31);
  const int64_t m = (int64_t)v.size();
  std::fwrite(t, 1, 32, f);
  std::fwrite(&m, 8, 1, f);
  for (size_t k = 0; k < v.size(); k++) {
    const double d = (double)v[k];
    std::fwrite(&d, 8, 1, f);
  }
}

template <typename C>
static void put_crds(FILE* f, const std::string& tag, const std::vector<std::array<C, 3> >& c) {
  std::vector<double> flat;
  for (size_t k = 0; k < c.size(); k++)
    for (int d = 0; d < 3; d++) flat.push_back((double)c[k][d]);
  put(f, tag, flat);
}

template <typename L>
static void put_image(FILE* f, const std::string& tag, L*** a, size_t n) {
  put(f, tag, std::vector<L>(&a[0][0][0], &a[0][0][0] + n));
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
  float*** mk = Alloc3D<float>(size);
  if (std::fread(&src[0][0][0], 4, n, in) != n || std::fread(&mask[0][0][0], 4, n, in) != n ||
      std::fread(&mk[0][0][0], 4, n, in) != n)
    return 5;
  std::fclose(in);
  FILE* out = std::fopen((dir + "/out.bin").c_str(), "wb");
  if (!out) return 6;

  {  // every default: minima, 6 neighbours, boundaries 0, no threshold, no mask; labels as ptrdiff_t, filled with 9 first
    std::ptrdiff_t*** lab = Alloc3D<std::ptrdiff_t>(size);
    for (size_t i = 0; i < n; i++) (&lab[0][0][0])[i] = 9;
    float const* const* const* none = nullptr;
    const size_t nb = Watershed<std::ptrdiff_t, float>(size, src, lab, none);
    put(out, "default_n", std::vector<size_t>(1, nb));
    put_image(out, "default_labels", lab, n);
    Dealloc3D(lab);
  }
  {  // maxima with the default threshold (+inf means none), mask, 26 neighbours, lists, labels as int
    int*** lab = Alloc3D<int>(size);
    std::vector<std::array<int, 3> > crds;
    std::vector<float> scores;
    int const* const* const* no_markers = nullptr;
    const size_t nb = Watershed(size, src, lab, mask, no_markers, std::numeric_limits<float>::infinity(), false, 3, true, 0, -1,
                                &crds, &scores, &std::cerr);
    put(out, "maxima_n", std::vector<size_t>(1, nb));
    put_image(out, "maxima_labels", lab, n);
    put_crds(out, "maxima_crds", crds);
    put(out, "maxima_scores", scores);
    Dealloc3D(lab);
  }
  {  // a threshold, hidden boundaries, other labels for boundary and undefined, labels as short
    short*** lab = Alloc3D<short>(size);
    short const* const* const* no_markers = nullptr;
    std::vector<std::array<float, 3> > crds;
    Watershed(size, src, lab, mask, no_markers, 3.0f, true, 2, false, (short)-4, (short)-7, &crds);
    put_image(out, "hidden_labels", lab, n);
    put_crds(out, "hidden_crds", crds);
    Watershed(size, src, lab, mask, no_markers, 3.0f, true, 2, true, (short)-4, (short)-7, &crds);
    put_image(out, "shown_labels", lab, n);
    Dealloc3D(lab);
  }
  {  // markers (long), through the host flood
    long*** lab = Alloc3D<long>(size);
    long*** markers = Alloc3D<long>(size);
    for (size_t i = 0; i < n; i++) (&markers[0][0][0])[i] = (long)(&mk[0][0][0])[i];
    std::vector<std::array<double, 3> > crds;
    std::vector<float> scores;
    const size_t nb = Watershed(size, src, lab, mask, static_cast<long const* const* const*>(markers), 5.0f, true, 1, true,
                                0L, -1L, &crds, &scores);
    put(out, "markers_n", std::vector<size_t>(1, nb));
    put_image(out, "markers_labels", lab, n);
    put_crds(out, "markers_crds", crds);
    put(out, "markers_scores", scores);
    Dealloc3D(lab);
    Dealloc3D(markers);
  }
  std::fclose(out);
  Dealloc3D(src);
  Dealloc3D(mask);
  Dealloc3D(mk);
  std::printf("shim watershed check ok\n");
  return 0;
}
