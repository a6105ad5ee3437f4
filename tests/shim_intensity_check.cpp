// The intensity maps through include/visfd_hip.hpp, for tests/test_intensity.py (mode "host": the scalar functions under
// their reference names, compiled by the host compiler; no device) and tests/test_intensity_gpu.py (mode "gpu":
// visfd::IntensityMap and visfd::ImageStats on the process's context).
// usage: shim_intensity_check MODE IN OUT.  IN: int32 nx, ny, nz, has_mask; a visfd_hip_intensity; in, out and mask
// volumes (float32).  OUT: the new out volume; in mode "gpu" the visfd_hip_stats of the pass and of visfd::ImageStats of
// the new volume behind it.
#include <cstdio>
#include <cstring>
#include <fstream>
#include <iostream>
#include <vector>

#include "visfd_hip.hpp"

using namespace visfd;

static float host_voxel(const visfd_hip_intensity& p, float vin, float vout, bool in_mask) {
  visfd_hip_intensity q = p;
  float v = vout;
  if (p.invert && in_mask) v = vh_intensity::invert(v, p.ave);
  switch (p.map) {   // the threshold family by its reference names
    case VISFD_HIP_MAP_STEP: v = vin > p.t[0] ? p.out_b : p.out_a; break;
    case VISFD_HIP_MAP_THRESH2: v = Threshold2(vin, p.t[0], p.t[1], p.out_a, p.out_b); break;
    case VISFD_HIP_MAP_THRESH4: v = Threshold4(vin, p.t[0], p.t[1], p.t[2], p.t[3], p.out_a, p.out_b); break;
    case VISFD_HIP_MAP_RANGE: v = SelectIntensityRange(vin, p.t[0], p.t[1], p.out_a, p.out_b); break;
    case VISFD_HIP_MAP_GAUSS: v = SelectIntensityRangeGauss(vin, p.t[0], p.t[1], p.out_a, p.out_b); break;
    default: break;
  }
  q.invert = 0;
  if (p.map != VISFD_HIP_MAP_RESCALE) q.map = VISFD_HIP_MAP_NONE;
  return vh_intensity::apply(q, vin, v, in_mask);   // rescale, mask fill, Rescale01
}

int main(int argc, char** argv) {
  if (argc != 4) return 2;
  const std::string mode = argv[1];
  std::ifstream f(argv[2], std::ios::binary);
  int32_t hdr[4];
  visfd_hip_intensity p;
  f.read(reinterpret_cast<char*>(hdr), sizeof(hdr));
  f.read(reinterpret_cast<char*>(&p), sizeof(p));
  const int size[3] = {hdr[0], hdr[1], hdr[2]};
  const size_t n = (size_t)size[0] * size[1] * size[2];
  float*** in = Alloc3D<float>(size);
  float*** out = Alloc3D<float>(size);
  float*** mask = hdr[3] ? Alloc3D<float>(size) : nullptr;
  f.read(reinterpret_cast<char*>(&in[0][0][0]), n * 4);
  f.read(reinterpret_cast<char*>(&out[0][0][0]), n * 4);
  if (mask) f.read(reinterpret_cast<char*>(&mask[0][0][0]), n * 4);
  if (!f) return 3;
  std::ofstream o(argv[3], std::ios::binary);
  try {
    if (mode == "host") {
      float* po = &out[0][0][0];
      const float* pi = &in[0][0][0];
      for (size_t i = 0; i < n; i++) po[i] = host_voxel(p, pi[i], po[i], !mask || (&mask[0][0][0])[i] != 0.0f);
      o.write(reinterpret_cast<const char*>(po), n * 4);
    } else {
      visfd_hip_stats st;
      IntensityMap(size, in, out, mask, p, &st);
      const visfd_hip_stats st2 = ImageStats(size, out, p.stats_mask ? mask : nullptr);
      o.write(reinterpret_cast<const char*>(&out[0][0][0]), n * 4);
      o.write(reinterpret_cast<const char*>(&st), sizeof(st));
      o.write(reinterpret_cast<const char*>(&st2), sizeof(st2));
    }
  } catch (std::exception& e) {
    std::cerr << e.what() << std::endl;
    return 1;
  }
  Dealloc3D(in);
  Dealloc3D(out);
  Dealloc3D(mask);
  return o ? 0 : 4;
}
