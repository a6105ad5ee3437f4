// MRC input/output of filter_mrc, written from the MRC2014 layout description (1024-byte header: nx,ny,nz,mode,
// start[3], m[3], cella[3], cellb[3], mapc/r/s, dmin,dmax,dmean, ispg, nsymbt, ..., "MAP ", machst);
// signed-byte rule as the reference applies it (mrc_header.cpp:49-75, mrc_simple.cpp:186-192).
// Part of filter_mrc.cpp's one translation unit (hence the unnamed namespace).
#pragma once
#include <algorithm>
#include <cstdint>
#include <cstring>
#include <fstream>
#include <string>
#include <vector>

#include "../../include/visfd_hip.hpp"

namespace {

using namespace visfd;
using std::string;
using std::vector;

struct Mrc {
  int32_t nx = 0, ny = 0, nz = 0, mode = 2;
  float cella[3] = {0, 0, 0};
  unsigned char raw_header[1024];
  float*** a = nullptr;  // [iz][iy][ix], contiguous
  bool loaded = false;

  ~Mrc() { Dealloc3D(a); }

  void alloc(int x, int y, int z) {
    Dealloc3D(a);
    nx = x; ny = y; nz = z;
    int size[3] = {nx, ny, nz};
    a = Alloc3D<float>(size);
  }
  float* data() { return &a[0][0][0]; }
  size_t nvox() const { return (size_t)nx * ny * nz; }
  void swap(Mrc& o) {
    std::swap(nx, o.nx); std::swap(ny, o.ny); std::swap(nz, o.nz); std::swap(mode, o.mode);
    std::swap(a, o.a); std::swap(loaded, o.loaded);
    for (int d = 0; d < 3; d++) std::swap(cella[d], o.cella[d]);
    unsigned char t[1024];
    std::memcpy(t, raw_header, 1024); std::memcpy(raw_header, o.raw_header, 1024); std::memcpy(o.raw_header, t, 1024);
  }

  void read(const string& path) {
    std::ifstream f(path.c_str(), std::ios::binary);
    if (!f) throw VisfdErr("Error: Unable to open \"" + path + "\" for reading.\n");
    f.read(reinterpret_cast<char*>(raw_header), 1024);
    if (!f) throw VisfdErr("Error: \"" + path + "\" is too short to be an MRC file.\n");
    int32_t w[256];
    std::memcpy(w, raw_header, 1024);
    float fw[256];
    std::memcpy(fw, raw_header, 1024);
    const int x = w[0], y = w[1], z = w[2];
    mode = w[3];
    if (x <= 0 || y <= 0 || z <= 0) throw VisfdErr("Error: bad image size in \"" + path + "\"\n");
    for (int d = 0; d < 3; d++) cella[d] = fw[10 + d];
    bool signed_bytes = true;
    if (path.size() > 4 && path.substr(path.size() - 4) == ".rec") signed_bytes = false;
    if (mode == 0 && w[38] == 1146047817) signed_bytes = (w[39] & 1) != 0;  // IMOD stamp + flag bit 0
    const int32_t nsymbt = w[23];
    if (nsymbt > 0) f.seekg(nsymbt, std::ios::cur);
    alloc(x, y, z);
    const size_t n = nvox();
    float* out = data();
    if (mode == 2) {
      f.read(reinterpret_cast<char*>(out), (std::streamsize)(n * 4));
    } else if (mode == 0) {
      vector<unsigned char> buf(n);
      f.read(reinterpret_cast<char*>(buf.data()), (std::streamsize)n);
      for (size_t i = 0; i < n; i++) out[i] = signed_bytes ? (float)(int8_t)buf[i] : (float)buf[i];
    } else if (mode == 1 || mode == 6) {
      vector<uint16_t> buf(n);
      f.read(reinterpret_cast<char*>(buf.data()), (std::streamsize)(n * 2));
      for (size_t i = 0; i < n; i++) out[i] = (mode == 1) ? (float)(int16_t)buf[i] : (float)buf[i];
    } else {
      throw VisfdErr("Error: unsupported MRC mode in \"" + path + "\" (supported: 0, 1, 2, 6)\n");
    }
    if (!f) throw VisfdErr("Error: \"" + path + "\" ended before all voxels were read.\n");
    loaded = true;
  }

  // the header and the cell size of another image of the same grid
  void copy_header_from(const Mrc& o) {
    std::memcpy(raw_header, o.raw_header, 1024);
    for (int d = 0; d < 3; d++) cella[d] = o.cella[d];
  }

  // header of `like` (cell size, origin, labels) with mode 2 and fresh statistics
  void write(const string& path, const Mrc& like) {
    unsigned char h[1024];
    std::memcpy(h, like.raw_header, 1024);
    int32_t w[256];
    std::memcpy(w, h, 1024);
    float fw[256];
    std::memcpy(fw, h, 1024);
    if (nx != w[0] || ny != w[1] || nz != w[2]) {   // resized by binning: grid and cell follow the new size
      w[7] = nx; w[8] = ny; w[9] = nz;
      std::memcpy(&w[10], like.cella, 12);
    }
    w[0] = nx; w[1] = ny; w[2] = nz; w[3] = 2;
    w[23] = 0;  // no extended header
    const size_t n = nvox();
    const float* p = &a[0][0][0];
    double sum = 0;
    float lo = p[0], hi = p[0];
    for (size_t i = 0; i < n; i++) { sum += p[i]; lo = std::min(lo, p[i]); hi = std::max(hi, p[i]); }
    std::memcpy(h, w, 96);
    fw[19] = lo; fw[20] = hi; fw[21] = (float)(sum / (double)n);
    std::memcpy(h + 76, &fw[19], 12);
    std::ofstream f(path.c_str(), std::ios::binary);
    if (!f) throw VisfdErr("Error: Unable to open \"" + path + "\" for writing.\n");
    f.write(reinterpret_cast<const char*>(h), 1024);
    f.write(reinterpret_cast<const char*>(p), (std::streamsize)(n * 4));
  }
};

}  // namespace
