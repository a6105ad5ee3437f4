// The general 3-D filter of the C++ drop-in (include/visfd_hip.hpp), called with the reference's signatures
// (lib/visfd/filter3d.hpp: Filter3D :37-530, GenFilterGenGauss3D :546-638, LocalFluctuations :1698-1853).  Reads DIR/in.bin
// (nx ny nz, then src and mask as float32 volumes), writes DIR/out.bin: one record per result (32-byte tag, int64 count,
// floats); tests/test_filter3d_gpu.py compares them with the numpy restatement.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <utility>

#include "visfd_hip.hpp"

using namespace visfd;

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
  float*** src = Alloc3D<float>(size);
  float*** mask = Alloc3D<float>(size);
  float*** dest = Alloc3D<float>(size);
  float*** den = Alloc3D<float>(size);
  if (std::fread(&src[0][0][0], 4, n, in) != n || std::fread(&mask[0][0][0], 4, n, in) != n) return 5;
  std::fclose(in);
  FILE* out = std::fopen((dir + "/out.bin").c_str(), "wb");
  if (!out) return 6;

  // a generalised Gaussian from half-widths, and from a ratio: floor(2 * (2.2, 1.1, 0.6)) = (4, 2, 1)
  const float width[3] = {2.2f, 1.1f, 0.6f};
  const int hw[3] = {4, 2, 1};
  float A = 0, A2 = 0;
  Filter3D<float, int> f = GenFilterGenGauss3D(width, 1.5f, hw, &A);
  Filter3D<float, int> f2 = GenFilterGenGauss3D(width, 1.5f, 2.0f, &A2);
  if (f2.halfwidth[0] != 4 || f2.halfwidth[1] != 2 || f2.halfwidth[2] != 1 || f.array_size[0] != 9 || A != A2 ||
      A != f.aaafH[0][0][0] || f.aaafH[-1][2][-4] != f2.aaafH[-1][2][-4])
    return 7;
  put(out, "table", f.flat_table(), 9 * 5 * 3);
  f.Apply(size, src, dest, nullptr, true);               put(out, "ggauss_norm", &dest[0][0][0], n);
  f.Apply(size, src, dest, mask, true);                  put(out, "ggauss_mask_norm", &dest[0][0][0], n);
  f.Apply(size, src, dest, mask, den);                   put(out, "ggauss_mask_raw", &dest[0][0][0], n);
                                                         put(out, "ggauss_mask_den", &den[0][0][0], n);
  // a table of the caller's own, filled through aaafH; copy, move and assignment keep it
  const int hq[3] = {1, 0, 2};
  Filter3D<float, int> q(hq);
  for (int jz = -2; jz <= 2; jz++)
    for (int jx = -1; jx <= 1; jx++) q.aaafH[jz][0][jx] = 0.25f * jz - 0.5f * jx + 0.125f;
  Filter3D<float, int> q2(q);
  Filter3D<float, int> q3;
  q3 = q2;
  Filter3D<float, int> q4(std::move(q2));
  q.MultiplyScalar(0.0f);                                // the copies are their own
  q4.AddScalar(1.0f);
  q4.AddScalar(-1.0f);
  q3.Apply(size, src, dest, nullptr, false);             put(out, "own_table", &dest[0][0][0], n);
  q4.Apply(size, src, dest, nullptr, false);             put(out, "own_table_moved", &dest[0][0][0], n);
  const float sums[4] = {q3.Sum(), q3.SumSqr(), q3.Average(), q3.AverageSqr()};
  put(out, "sums", sums, 4);
  Filter3D<float, int> g(f);
  g.MultiplyScalar(3.0f);
  g.Normalize();
  put(out, "renormalized", g.flat_table(), 9 * 5 * 3);

  float sigma[3] = {1.4f, 1.4f, 1.4f};
  LocalFluctuations(size, src, dest, mask, sigma, 6.0f, 1.5f, true);
  put(out, "fluct_m6_mask", &dest[0][0][0], n);
  const float radius[3] = {3.0f, 3.0f, 3.0f};
  LocalFluctuationsByRadius(size, src, dest, nullptr, radius, 4.0f, 1.3f, true);
  put(out, "fluct_radius_m4", &dest[0][0][0], n);
  std::fclose(out);
  Dealloc3D(src); Dealloc3D(mask); Dealloc3D(dest); Dealloc3D(den);
  std::printf("shim filter3d check ok\n");
  return 0;
}
