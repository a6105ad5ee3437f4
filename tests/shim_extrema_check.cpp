// The extrema functions of the C++ drop-in (include/visfd_hip.hpp), called with the reference's signatures
// (lib/visfd/morphology.hpp:56-118, morphology_implementation.hpp:57-796).  Reads DIR/in.bin (nx ny nz, then src and mask
// as float32 volumes), writes DIR/out.bin: one record per result (32-byte tag, int64 count, doubles -- every index,
// count, label and float score is exact in a double); tests/test_extrema_gpu.py checks them against the restatement.
#include <array>
#include <cstdint>
#include <cstdio>
#include <cstring>
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
  if (std::fread(&src[0][0][0], 4, n, in) != n || std::fread(&mask[0][0][0], 4, n, in) != n) return 5;
  std::fclose(in);
  FILE* out = std::fopen((dir + "/out.bin").c_str(), "wb");
  if (!out) return 6;
  const float inf = std::numeric_limits<float>::infinity();

  {  // FindMinima: defaults, labels as float, filled with 9 first (masked voxels keep it)
    float*** lab = Alloc3D<float>(size);
    for (size_t i = 0; i < n; i++) (&lab[0][0][0])[i] = 9.0f;
    std::vector<std::array<float, 3> > crds;
    std::vector<float> scores;
    std::vector<size_t> nvox;
    const size_t found = FindMinima(size, src, mask, crds, scores, nvox, inf, 3, true, lab);
    if (found != crds.size()) return 7;
    put_crds(out, "minima_crds", crds); put(out, "minima_scores", scores); put(out, "minima_nvoxels", nvox);
    put_image(out, "minima_labels", lab, n);
    Dealloc3D(lab);
  }
  {  // FindMaxima: a threshold of +inf (the default) means none; connectivity 1, no borders, integer coordinates and labels
    int*** lab = Alloc3D<int>(size);
    std::memset(&lab[0][0][0], 0, 4 * n);
    std::vector<std::array<int, 3> > crds;
    std::vector<float> scores;
    std::vector<int> nvox;
    float const* const* const* no_mask = nullptr;
    const size_t found = FindMaxima(size, src, no_mask, crds, scores, nvox, inf, 1, false, lab);
    if (found != crds.size()) return 8;
    put_crds(out, "maxima_crds", crds); put(out, "maxima_scores", scores); put(out, "maxima_nvoxels", nvox);
    put_image(out, "maxima_labels", lab, n);
    Dealloc3D(lab);
  }
  {  // both lists, linear indices, thresholds, connectivity 2, labels as short
    short*** lab = Alloc3D<short>(size);
    std::memset(&lab[0][0][0], 0, 2 * n);
    std::vector<size_t> imin, imax, nmin, nmax;
    std::vector<float> smin, smax;
    const size_t found = _FindExtrema(size, src, mask, &imin, &imax, &smin, &smax, &nmin, &nmax, 1.0f, 5.0f, 2, true, lab);
    if (found != imin.size() + imax.size()) return 9;
    put(out, "both_min_index", imin); put(out, "both_min_scores", smin); put(out, "both_min_nvoxels", nmin);
    put(out, "both_max_index", imax); put(out, "both_max_scores", smax); put(out, "both_max_nvoxels", nmax);
    put_image(out, "both_labels", lab, n);
    Dealloc3D(lab);
  }
  {  // both lists, coordinates; only the maxima sought (null minima list), no label image
    std::vector<std::array<double, 3> > cmax;
    std::vector<std::array<double, 3> >* none = nullptr;
    std::vector<float> smax;
    std::vector<float>* none_scores = nullptr;
    std::vector<long> nmax;
    std::vector<long>* none_nvox = nullptr;
    float*** no_labels = nullptr;
    _FindExtrema(size, src, mask, none, &cmax, none_scores, &smax, none_nvox, &nmax, inf, 4.0f, 3, true, no_labels);
    put_crds(out, "maxonly_crds", cmax); put(out, "maxonly_scores", smax); put(out, "maxonly_nvoxels", nmax);
  }
  std::fclose(out);
  Dealloc3D(src); Dealloc3D(mask);
  std::printf("shim extrema check ok\n");
  return 0;
}
