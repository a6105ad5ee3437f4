// visfd_hip.hpp -- the visfd:: template API of the hot path, re-created on top of the C ABI
// (include/visfd_hip.h, libvisfd_hip.so).  Header-only, C++11, no dependency on the reference.
//
// A program written against the reference's headers for this path keeps compiling when it
// includes this file instead of <visfd.hpp>: the functions below have the reference's names,
// argument order, argument meaning and error behaviour (they throw visfd::VisfdErr), and take
// the same `float***` arrays indexed [iz][iy][ix].  The arrays must be CONTIGUOUS, as produced by
// visfd::Alloc3D (lib/visfd/alloc3d.hpp:25-67) or MrcSimple: &a[0][0][0] is handed to the C ABI.
//
// Reference signatures mirrored (file:line under the reference root):
//   ApplyGauss   lib/visfd/filter3d.hpp:1086-1097, :1161-1173, :1226-1237, :1297-1308
//                bin/filter_mrc/filter3d_variants.hpp:500-528 (ratio OR threshold)
//   ApplyDog     lib/visfd/filter3d.hpp:1338-1351          ApplyLog  :1428-1441, :1531-1544
//   ApplySeparable lib/visfd/filter3d.hpp:686-695  (with GenFilterGauss1D, filter1d.hpp:409)
//   BlobDog      lib/visfd/feature.hpp:53-77               BlobDogD  :446-470
//   CalcHessian  lib/visfd/feature.hpp:1203-1219
//   TV3D         lib/visfd/feature.hpp:1645-1647, TVDenseStick :1711-1901 (with its normalize / diagonalize_dest steps)
//   BlobDogNM / _BlobDogNM  bin/filter_mrc/feature_variants.hpp:393-580
//   Alloc3D / Dealloc3D  lib/visfd/alloc3d.hpp:25, :75
//   Watershed    lib/visfd/segmentation.hpp:65-82
//   Filter3D     lib/visfd/filter3d.hpp:37-530;  GenFilterGenGauss3D :546-638;  LocalFluctuations[ByRadius] :1698-1926
//   CompactMultiChannelImage3D  lib/visfd/multichannel_image3d.hpp:41-204
//   Threshold2, Threshold4, SelectIntensityRange, SelectIntensityRangeGauss  lib/threshold/threshold.hpp:52-258
//   VoxelizeMesh  what bin/voxelize_mesh/voxelize_mesh.py computes with vtk (no C++ counterpart in the reference)
//   CloseSurface  an oriented point cloud closed into a mask on the grid (no counterpart in the reference, whose workflow
//                 leaves this step to an external surface reconstruction program; visfd_hip.h states the definition)
//   IsoSurface    the closed triangle mesh of a level set by marching tetrahedra (no counterpart in the reference, whose
//                 workflow takes its mesh from that external program; visfd_hip.h states the definition)
// Only Scalar = float is provided (the hot path and the CLI use float throughout).
#ifndef VISFD_HIP_HPP
#define VISFD_HIP_HPP

#include <array>
#include <cmath>
#include <cstddef>
#include <cstdlib>
#include <exception>
#include <limits>
#include <ostream>
#include <string>
#include <tuple>
#include <type_traits>
#include <utility>
#include <vector>

#include "visfd_hip.h"
#include "../visfd_amd/csrc/intensity.hpp"   // the scalar intensity maps, shared with the kernels

namespace visfd {

// lib/visfd/err_visfd.hpp:15-22
class VisfdErr : public std::exception {
  std::string msg;
 public:
  VisfdErr(const char* description) : msg(description) {}
  VisfdErr(std::string description) : msg(description) {}
  virtual const char* what() const throw() { return msg.c_str(); }
  virtual ~VisfdErr() throw() {}
};

namespace hip_detail {

// One process-wide context (device 0 unless VISFD_HIP_DEVICE is set), created on first use.
inline visfd_hip_ctx* context() {
  static visfd_hip_ctx* ctx = nullptr;
  if (!ctx) {
    int dev = 0;
    if (const char* e = std::getenv("VISFD_HIP_DEVICE")) dev = std::atoi(e);
    if (visfd_hip_create(dev, nullptr, &ctx) != VISFD_HIP_OK)
      throw VisfdErr(std::string("visfd_hip: ") + visfd_hip_last_error());
  }
  return ctx;
}
inline void check(int rc) {
  if (rc != VISFD_HIP_OK) throw VisfdErr(std::string("visfd_hip: ") + visfd_hip_last_error());
}
template <typename T>
inline T* flat(T* const* const* a) { return a ? &a[0][0][0] : nullptr; }
inline const float* flat(float const* const* const* a) { return a ? &a[0][0][0] : nullptr; }
inline void require_contiguous(float const* const* const* a, const int size[3]) {
  if (!a) return;
  const float* base = &a[0][0][0];
  const size_t nx = size[0], ny = size[1];
  if (&a[size[2] - 1][size[1] - 1][0] != base + ((size_t)(size[2] - 1) * ny + (size[1] - 1)) * nx)
    throw VisfdErr("visfd_hip: 3-D arrays must be contiguous (allocate them with Alloc3D)");
}

}  // namespace hip_detail

// ---- lib/visfd/alloc3d.hpp ------------------------------------------------------------------
template <typename Entry, typename Integer>
Entry*** Alloc3D(const Integer size[3]) {
  const size_t nx = size[0], ny = size[1], nz = size[2];
  Entry*** a = new Entry**[nz];
  Entry** rows = new Entry*[nz * ny];
  Entry* data = new Entry[nz * ny * nx];
  for (size_t iz = 0; iz < nz; iz++) {
    a[iz] = rows + iz * ny;
    for (size_t iy = 0; iy < ny; iy++) a[iz][iy] = data + (iz * ny + iy) * nx;
  }
  return a;
}
template <typename Entry>
void Dealloc3D(Entry*** a) {
  if (a) {
    delete[] a[0][0];
    delete[] a[0];
    delete[] a;
  }
}

// ---- lib/visfd/multichannel_image3d.hpp:41-204 ------------------------------------------------------
// One pointer per voxel (nullptr where mask == 0) into one compact array of n_good_voxels * channels numbers in scan
// order: the container HandleTV keeps its Hessians and vote tensors in (bin/filter_mrc/handlers.cpp:1564-1565).
template <typename Scalar>
class CompactMultiChannelImage3D {
  // Written for this shim (only the public face -- aaaafI, nchannels(), the constructors, Resize -- follows the reference):
  // the channel values of the unmasked voxels live in one std::vector in scan order, and `aaaafI` is an Alloc3D table of
  // pointers into it that a single pass binds with a running cursor.
  std::vector<Scalar> values_;
  int channels_;
  int dims_[3];

  static bool masked_out(Scalar const* const* const* mask, int iz, int iy, int ix) { return mask && mask[iz][iy][ix] == 0.0; }

  void release() {
    if (aaaafI) Dealloc3D(aaaafI);
    aaaafI = nullptr;
    values_.clear();
    values_.shrink_to_fit();
  }
  // (re)build the pointer table over values_: voxel by voxel in scan order, unmasked voxels take consecutive records
  template <typename Keep>
  void bind(Keep keep) {
    aaaafI = Alloc3D<Scalar*>(dims_);
    Scalar* cursor = values_.empty() ? nullptr : &values_[0];
    for (int iz = 0; iz < dims_[2]; iz++)
      for (int iy = 0; iy < dims_[1]; iy++)
        for (int ix = 0; ix < dims_[0]; ix++) {
          const bool k = keep(iz, iy, ix);
          aaaafI[iz][iy][ix] = k ? cursor : nullptr;
          if (k) cursor += channels_;
        }
  }

 public:
  Scalar**** aaaafI;   // a 3-D array of pointers into the compact array (nullptr where the mask is zero)

  int nchannels() { return channels_; }
  explicit CompactMultiChannelImage3D(int set_n_channels_per_voxel) : channels_(set_n_channels_per_voxel), aaaafI(nullptr) {
    dims_[0] = dims_[1] = dims_[2] = 0;
  }
  CompactMultiChannelImage3D(int set_n_channels_per_voxel, int const set_image_size[3],
                             Scalar const* const* const* aaafMask = nullptr, std::ostream* pReportProgress = nullptr)
      : channels_(set_n_channels_per_voxel), aaaafI(nullptr) {
    dims_[0] = dims_[1] = dims_[2] = 0;
    Resize(set_image_size, aaafMask, pReportProgress);
  }
  void Resize(int const set_image_size[3], Scalar const* const* const* aaafMask = nullptr,
              std::ostream* pReportProgress = nullptr) {
    release();
    for (int d = 0; d < 3; d++) dims_[d] = set_image_size[d];
    size_t kept = 0;
    for (int iz = 0; iz < dims_[2]; iz++)
      for (int iy = 0; iy < dims_[1]; iy++)
        for (int ix = 0; ix < dims_[0]; ix++) kept += masked_out(aaafMask, iz, iy, ix) ? 0 : 1;
    if (pReportProgress)
      *pReportProgress << " -- allocating " << channels_ << " channels for " << kept << " of "
                       << (size_t)dims_[0] * dims_[1] * dims_[2] << " voxels\n";
    values_.assign(kept * (size_t)channels_, Scalar());
    bind([&](int iz, int iy, int ix) { return !masked_out(aaafMask, iz, iy, ix); });
  }
  ~CompactMultiChannelImage3D() { release(); }
  CompactMultiChannelImage3D(const CompactMultiChannelImage3D<Scalar>& source)
      : values_(source.values_), channels_(source.channels_), aaaafI(nullptr) {
    for (int d = 0; d < 3; d++) dims_[d] = source.dims_[d];
    if (!source.aaaafI) return;
    Scalar**** const theirs = source.aaaafI;
    bind([&](int iz, int iy, int ix) { return theirs[iz][iy][ix] != nullptr; });   // same voxels, same order: same records
  }
  void swap(CompactMultiChannelImage3D<Scalar>& other) {
    values_.swap(other.values_);   // (a vector's buffer moves with it: both pointer tables stay valid)
    std::swap(channels_, other.channels_);
    for (int d = 0; d < 3; d++) std::swap(dims_[d], other.dims_[d]);
    std::swap(aaaafI, other.aaaafI);
  }
  CompactMultiChannelImage3D(CompactMultiChannelImage3D<Scalar>&& other) : channels_(other.channels_), aaaafI(nullptr) {
    dims_[0] = dims_[1] = dims_[2] = 0;
    this->swap(other);
  }
  CompactMultiChannelImage3D<Scalar>& operator=(CompactMultiChannelImage3D<Scalar> source) {
    this->swap(source);
    return *this;
  }
};

// ---- lib/visfd/filter1d.hpp:26-390 (the fields the hot path's callers touch) -------------------
template <typename Scalar, typename Integer>
class Filter1D {
 public:
  std::vector<Scalar> storage;
  Scalar* afH;        // indexable from -halfwidth .. +halfwidth
  Integer halfwidth;
  Integer array_size;
  Filter1D() : afH(nullptr), halfwidth(-1), array_size(-1) {}
  explicit Filter1D(Integer h) { Resize(h); }
  Filter1D(const Filter1D& o) : storage(o.storage), halfwidth(o.halfwidth), array_size(o.array_size) {
    afH = storage.empty() ? nullptr : storage.data() + halfwidth;
  }
  Filter1D& operator=(const Filter1D& o) {
    storage = o.storage; halfwidth = o.halfwidth; array_size = o.array_size;
    afH = storage.empty() ? nullptr : storage.data() + halfwidth;
    return *this;
  }
  void Resize(Integer h) {
    halfwidth = h;
    array_size = 2 * h + 1;
    storage.assign((size_t)array_size, (Scalar)-1.0e38);
    afH = storage.data() + h;
  }
};

// lib/visfd/filter1d.hpp:409-460
inline Filter1D<float, int> GenFilterGauss1D(float sigma, int halfwidth, std::ostream* = nullptr) {
  Filter1D<float, int> f(halfwidth);
  hip_detail::check(visfd_hip_gauss_taps(sigma, halfwidth, f.storage.data()));
  return f;
}

// ---- lib/visfd/filter3d.hpp:686-695 ---------------------------------------------------------------
inline float ApplySeparable(int const image_size[3], float const* const* const* aaafSource,
                            float*** aaafDest, float const* const* const* aaafMask,
                            Filter1D<float, int> aFilter[3], bool normalize = true,
                            std::ostream* pReportProgress = nullptr) {
  hip_detail::require_contiguous(aaafSource, image_size);
  hip_detail::require_contiguous(aaafDest, image_size);
  hip_detail::require_contiguous(aaafMask, image_size);
  if (pReportProgress) *pReportProgress << "  progress: Applying Z, Y, X filters on the GPU" << std::endl;
  float A = 0;
  hip_detail::check(visfd_hip_separable3d(
      hip_detail::context(), hip_detail::flat(aaafSource), hip_detail::flat(aaafDest),
      hip_detail::flat(aaafMask), image_size[0], image_size[1], image_size[2],
      aFilter[0].storage.data(), aFilter[0].halfwidth, aFilter[1].storage.data(), aFilter[1].halfwidth,
      aFilter[2].storage.data(), aFilter[2].halfwidth, normalize ? 1 : 0, &A));
  return A;
}

// ---- ApplyGauss: lib/visfd/filter3d.hpp:1086 (sigma[3], halfwidth[3]) --------------------------------
inline float ApplyGauss(const int image_size[3], float const* const* const* aaafSource, float*** aaafDest,
                        float const* const* const* aaafMask, float const sigma[3],
                        const int truncate_halfwidth[3], bool normalize = true,
                        std::ostream* pReportProgress = nullptr) {
  hip_detail::require_contiguous(aaafSource, image_size);
  hip_detail::require_contiguous(aaafDest, image_size);
  hip_detail::require_contiguous(aaafMask, image_size);
  if (pReportProgress) *pReportProgress << "  progress: Applying Z, Y, X filters on the GPU" << std::endl;
  float A = 0;
  hip_detail::check(visfd_hip_apply_gauss(hip_detail::context(), hip_detail::flat(aaafSource),
                                          hip_detail::flat(aaafDest), hip_detail::flat(aaafMask),
                                          image_size[0], image_size[1], image_size[2], sigma,
                                          truncate_halfwidth, normalize ? 1 : 0, &A));
  return A;
}
// :1161 (sigma, halfwidth)
inline float ApplyGauss(const int image_size[3], float const* const* const* src, float*** dest,
                        float const* const* const* mask, float sigma, int truncate_halfwidth,
                        bool normalize = true, std::ostream* pReportProgress = nullptr) {
  const float s[3] = {sigma, sigma, sigma};
  const int hw[3] = {truncate_halfwidth, truncate_halfwidth, truncate_halfwidth};
  return ApplyGauss(image_size, src, dest, mask, s, hw, normalize, pReportProgress);
}
// :1226 (sigma[3], truncate_ratio)
inline float ApplyGauss(const int image_size[3], float const* const* const* src, float*** dest,
                        float const* const* const* mask, const float sigma[3], float truncate_ratio = 2.5,
                        bool normalize = true, std::ostream* pReportProgress = nullptr) {
  int hw[3];
  hip_detail::check(visfd_hip_gauss_halfwidths(sigma, truncate_ratio, hw));
  return ApplyGauss(image_size, src, dest, mask, sigma, hw, normalize, pReportProgress);
}
// :1297 (sigma, truncate_ratio).  The reference falls off the end of this overload without a return
// statement (filter3d.hpp:1309-1319); here it returns the A coefficient like its siblings.
inline float ApplyGauss(const int image_size[3], float const* const* const* src, float*** dest,
                        float const* const* const* mask, float sigma, float truncate_ratio = 2.5,
                        bool normalize = true, std::ostream* pReportProgress = nullptr) {
  const float s[3] = {sigma, sigma, sigma};
  return ApplyGauss(image_size, src, dest, mask, s, truncate_ratio, normalize, pReportProgress);
}
// bin/filter_mrc/filter3d_variants.hpp:500-528 (ratio, or threshold when ratio <= 0)
inline float ApplyGauss(const int image_size[3], float const* const* const* src, float*** dest,
                        float const* const* const* mask, const float sigma[3], float filter_truncate_ratio,
                        float filter_truncate_threshold, bool normalize = true,
                        std::ostream* pReportProgress = nullptr) {
  if (filter_truncate_ratio <= 0) filter_truncate_ratio = visfd_hip_ratio_from_threshold(filter_truncate_threshold);
  return ApplyGauss(image_size, src, dest, mask, sigma, filter_truncate_ratio, normalize, pReportProgress);
}

// ---- ApplyDog: lib/visfd/filter3d.hpp:1338-1351 -------------------------------------------------------
inline void ApplyDog(const int image_size[3], float const* const* const* src, float*** dest,
                     float const* const* const* mask, float const sigma_a[3], float const sigma_b[3],
                     const int truncate_halfwidth[3], float* pA = nullptr, float* pB = nullptr,
                     std::ostream* = nullptr) {
  hip_detail::require_contiguous(src, image_size);
  hip_detail::require_contiguous(dest, image_size);
  hip_detail::require_contiguous(mask, image_size);
  hip_detail::check(visfd_hip_apply_dog(hip_detail::context(), hip_detail::flat(src), hip_detail::flat(dest),
                                        hip_detail::flat(mask), image_size[0], image_size[1], image_size[2],
                                        sigma_a, sigma_b, truncate_halfwidth, pA, pB));
}

// ---- ApplyLog: lib/visfd/filter3d.hpp:1428-1441 and :1531-1544 ----------------------------------------
inline void ApplyLog(const int image_size[3], float const* const* const* src, float*** dest,
                     float const* const* const* mask, const float sigma[3],
                     float delta_sigma_over_sigma = 0.02, float truncate_ratio = 2.5, float* pA = nullptr,
                     float* pB = nullptr, std::ostream* = nullptr) {
  hip_detail::require_contiguous(src, image_size);
  hip_detail::require_contiguous(dest, image_size);
  hip_detail::require_contiguous(mask, image_size);
  hip_detail::check(visfd_hip_apply_log(hip_detail::context(), hip_detail::flat(src), hip_detail::flat(dest),
                                        hip_detail::flat(mask), image_size[0], image_size[1], image_size[2], sigma,
                                        delta_sigma_over_sigma, truncate_ratio, pA, pB));
}
inline void ApplyLog(const int image_size[3], float const* const* const* src, float*** dest,
                     float const* const* const* mask, float sigma, float delta_sigma_over_sigma = 0.02,
                     float truncate_ratio = 2.5, float* pA = nullptr, float* pB = nullptr,
                     std::ostream* pReportProgress = nullptr) {
  const float s[3] = {sigma, sigma, sigma};
  ApplyLog(image_size, src, dest, mask, s, delta_sigma_over_sigma, truncate_ratio, pA, pB, pReportProgress);
}

// ---- grayscale morphology: lib/visfd/morphology.hpp:134-597 ------------------------------------------------------
// Dilate / Erode with an arbitrary structuring element: a list of (ix, iy, iz, b), walked in the given order.
namespace hip_detail {
inline void morph_table(int op, const std::vector<std::tuple<int, int, int, float> >& structure_factor,
                        const int image_size[3], float const* const* const* src, float*** dest,
                        float const* const* const* mask) {
  require_contiguous(src, image_size);
  require_contiguous(dest, image_size);
  require_contiguous(mask, image_size);
  std::vector<int> dxyz;
  std::vector<float> b;
  dxyz.reserve(3 * structure_factor.size());
  b.reserve(structure_factor.size());
  for (size_t k = 0; k < structure_factor.size(); k++) {
    dxyz.push_back(std::get<0>(structure_factor[k]));
    dxyz.push_back(std::get<1>(structure_factor[k]));
    dxyz.push_back(std::get<2>(structure_factor[k]));
    b.push_back(std::get<3>(structure_factor[k]));
  }
  check(visfd_hip_morph_table(context(), flat(src), flat(dest), flat(mask), image_size[0], image_size[1], image_size[2],
                              op, dxyz.empty() ? nullptr : &dxyz[0], b.empty() ? nullptr : &b[0],
                              (int64_t)b.size()));
}
// the *Sphere functions: dest keeps its values where mask == 0; the top-hats read it (dest -= open(src), dest = close(src) - dest)
inline void morph_sphere(int op, float radius, const int image_size[3], float const* const* const* src, float*** dest,
                         float const* const* const* mask, float radius_max, float bmax) {
  require_contiguous(src, image_size);
  require_contiguous(dest, image_size);
  require_contiguous(mask, image_size);
  check(visfd_hip_morph_sphere(context(), flat(src), flat(dest), flat(mask), image_size[0], image_size[1], image_size[2],
                               op, radius, radius_max, bmax));
}
}  // namespace hip_detail

inline void Dilate(std::vector<std::tuple<int, int, int, float> > structure_factor, const int image_size[3],
                   float const* const* const* aaafSource, float*** aaafDest,
                   float const* const* const* aaafMask = nullptr, std::ostream* = nullptr) {
  hip_detail::morph_table(VISFD_HIP_MORPH_DILATE, structure_factor, image_size, aaafSource, aaafDest, aaafMask);
}
inline void Erode(std::vector<std::tuple<int, int, int, float> > structure_factor, const int image_size[3],
                  float const* const* const* aaafSource, float*** aaafDest,
                  float const* const* const* aaafMask = nullptr, std::ostream* = nullptr) {
  hip_detail::morph_table(VISFD_HIP_MORPH_ERODE, structure_factor, image_size, aaafSource, aaafDest, aaafMask);
}
inline void DilateSphere(float radius, int const image_size[3], float const* const* const* aaafSource, float*** aaafDest,
                         float const* const* const* aaafMask = nullptr, float radius_max = 0.0, float bmax = 0.0,
                         std::ostream* = nullptr) {
  hip_detail::morph_sphere(VISFD_HIP_MORPH_DILATE, radius, image_size, aaafSource, aaafDest, aaafMask, radius_max, bmax);
}
inline void ErodeSphere(float radius, int const image_size[3], float const* const* const* aaafSource, float*** aaafDest,
                        float const* const* const* aaafMask = nullptr, float radius_max = 0.0, float bmax = 0.0,
                        std::ostream* = nullptr) {
  hip_detail::morph_sphere(VISFD_HIP_MORPH_ERODE, radius, image_size, aaafSource, aaafDest, aaafMask, radius_max, bmax);
}
inline void OpenSphere(float radius, const int image_size[3], float const* const* const* aaafSource, float*** aaafDest,
                       float const* const* const* aaafMask = nullptr, float radius_max = 0.0, float bmax = 0.0,
                       std::ostream* = nullptr) {
  hip_detail::morph_sphere(VISFD_HIP_MORPH_OPEN, radius, image_size, aaafSource, aaafDest, aaafMask, radius_max, bmax);
}
inline void CloseSphere(float radius, const int image_size[3], float const* const* const* aaafSource, float*** aaafDest,
                        float const* const* const* aaafMask = nullptr, float radius_max = 0.0, float bmax = 0.0,
                        std::ostream* = nullptr) {
  hip_detail::morph_sphere(VISFD_HIP_MORPH_CLOSE, radius, image_size, aaafSource, aaafDest, aaafMask, radius_max, bmax);
}
inline void WhiteTopHatSphere(float radius, const int image_size[3], float const* const* const* aaafSource,
                              float*** aaafDest, float const* const* const* aaafMask = nullptr, float radius_max = 0.0,
                              float bmax = 0.0, std::ostream* = nullptr) {
  hip_detail::morph_sphere(VISFD_HIP_MORPH_TOP_HAT_WHITE, radius, image_size, aaafSource, aaafDest, aaafMask, radius_max,
                           bmax);
}
inline void BlackTopHatSphere(float radius, const int image_size[3], float const* const* const* aaafSource,
                              float*** aaafDest, float const* const* const* aaafMask = nullptr, float radius_max = 0.0,
                              float bmax = 0.0, std::ostream* = nullptr) {
  hip_detail::morph_sphere(VISFD_HIP_MORPH_TOP_HAT_BLACK, radius, image_size, aaafSource, aaafDest, aaafMask, radius_max,
                           bmax);
}

// ---- the median filter: lib/visfd/filter3d.hpp:1577-1674 ----------------------------------------------------------
// The reference's signatures.  Its footprint loop does not end once a neighbour is skipped; the semantics here are the
// ones include/visfd_hip.h states (rank n / 2 of the neighbours inside the image with mask != 0; dest keeps its values
// where mask == 0).
inline void Median(std::vector<std::tuple<int, int, int> > footprint, const int image_size[3],
                   float const* const* const* aaafSource, float*** aaafDest,
                   float const* const* const* aaafMask = nullptr, std::ostream* = nullptr) {
  hip_detail::require_contiguous(aaafSource, image_size);
  hip_detail::require_contiguous(aaafDest, image_size);
  hip_detail::require_contiguous(aaafMask, image_size);
  std::vector<int> dxyz;
  dxyz.reserve(3 * footprint.size());
  for (size_t k = 0; k < footprint.size(); k++) {
    dxyz.push_back(std::get<0>(footprint[k]));
    dxyz.push_back(std::get<1>(footprint[k]));
    dxyz.push_back(std::get<2>(footprint[k]));
  }
  hip_detail::check(visfd_hip_median_table(hip_detail::context(), hip_detail::flat(aaafSource), hip_detail::flat(aaafDest),
                                           hip_detail::flat(aaafMask), image_size[0], image_size[1], image_size[2],
                                           dxyz.empty() ? nullptr : &dxyz[0], (int64_t)footprint.size()));
}
inline void MedianSphere(float radius, int const image_size[3], float const* const* const* aaafSource, float*** aaafDest,
                         float const* const* const* aaafMask = nullptr, std::ostream* = nullptr) {
  hip_detail::require_contiguous(aaafSource, image_size);
  hip_detail::require_contiguous(aaafDest, image_size);
  hip_detail::require_contiguous(aaafMask, image_size);
  hip_detail::check(visfd_hip_median_sphere(hip_detail::context(), hip_detail::flat(aaafSource), hip_detail::flat(aaafDest),
                                            hip_detail::flat(aaafMask), image_size[0], image_size[1], image_size[2], radius));
}

// ---- intensity maps: lib/threshold/threshold.hpp (Number = float), and the image-level calls of include/visfd_hip.h m1c --
// The reference's names, arguments and defaults; the arithmetic is csrc/intensity.hpp's, the one the kernels run.
inline float Threshold2(float intensity, float threshold_01_a, float threshold_01_b, float outA = 0, float outB = 1) {
  return vh_intensity::threshold2(intensity, threshold_01_a, threshold_01_b, outA, outB);
}
inline float Threshold4(float intensity, float threshold_01_a, float threshold_01_b, float threshold_10_a,
                        float threshold_10_b, float outA = 0, float outB = 1) {
  return vh_intensity::threshold4(intensity, threshold_01_a, threshold_01_b, threshold_10_a, threshold_10_b, outA, outB);
}
// (the reference takes outA and outB and returns 1 or 0 whatever they are)
inline float SelectIntensityRange(float intensity, float range_a, float range_b, float = 0, float = 1) {
  return vh_intensity::select_range(intensity, range_a, range_b);
}
inline float SelectIntensityRangeGauss(float intensity, float x0, float sigma, float outA = 0, float outB = 1) {
  return vh_intensity::gauss(intensity, x0, sigma, outA, outB);
}
// count, extremes and the exact sum of the voxels with mask != 0 (visfd_hip_image_stats)
inline visfd_hip_stats ImageStats(const int image_size[3], float const* const* const* aaafI,
                                  float const* const* const* aaafMask = nullptr) {
  hip_detail::require_contiguous(aaafI, image_size);
  hip_detail::require_contiguous(aaafMask, image_size);
  visfd_hip_stats st;
  hip_detail::check(visfd_hip_image_stats(hip_detail::context(), hip_detail::flat(aaafI), hip_detail::flat(aaafMask),
                                          (int64_t)image_size[0] * image_size[1] * image_size[2], &st));
  return st;
}
// one pass of the stages of `p` over aaafOut, in place (visfd_hip_intensity_map); aaafIn: the threshold maps' input, which
// may be aaafOut itself
inline void IntensityMap(const int image_size[3], float const* const* const* aaafIn, float*** aaafOut,
                         float const* const* const* aaafMask, const visfd_hip_intensity& p, visfd_hip_stats* stats = nullptr) {
  hip_detail::require_contiguous(aaafIn, image_size);
  hip_detail::require_contiguous(aaafOut, image_size);
  hip_detail::require_contiguous(aaafMask, image_size);
  hip_detail::check(visfd_hip_intensity_map(hip_detail::context(), hip_detail::flat(aaafIn), hip_detail::flat(aaafOut),
                                            hip_detail::flat(aaafMask), image_size[0], image_size[1], image_size[2], &p, stats));
}

// ---- local minima and maxima with plateaus: lib/visfd/morphology.hpp:56-118, morphology_implementation.hpp:57-796 --
// The reference's signatures and defaults with Scalar = float.  Lists come back in the reference's order; aaaiDest (any
// arithmetic Label) receives the label image where mask != 0, converted from the 32-bit labels of the C ABI exactly as
// the reference converts its ptrdiff_t (images have fewer than 2^31 - 2 voxels, so every label fits).  Connectivity
// above 3 is refused (visfd_hip.h).
namespace hip_detail {
struct ExtremaLists {
  std::vector<int64_t> index[2], nvoxels[2];   // [0] minima, [1] maxima
  std::vector<float> score[2];
};
template <typename Label>
inline size_t find_extrema(const int image_size[3], float const* const* const* src, float const* const* const* mask,
                           bool find_minima, bool find_maxima, float minima_threshold, float maxima_threshold,
                           int connectivity, bool allow_borders, Label*** dest, ExtremaLists* out) {
  require_contiguous(src, image_size);
  require_contiguous(mask, image_size);
  const size_t nvox = (size_t)image_size[0] * image_size[1] * image_size[2];
  std::vector<int32_t> labels(dest ? nvox : 0);
  int64_t n[2] = {0, 0};
  // a first try with room for one voxel in 32 per list (blurred tomograms list about one in 150); a call that finds more
  // returns the counts, and the second call -- which repeats the device work -- is sized by them
  const int64_t cap0 = (int64_t)(nvox / 32) > 65536 ? (int64_t)(nvox / 32) : 65536;
  int64_t cap[2] = {find_minima ? cap0 : 1, find_maxima ? cap0 : 1};
  for (;;) {
    for (int k = 0; k < 2; k++) {
      out->index[k].resize((size_t)cap[k]);
      out->score[k].resize((size_t)cap[k]);
      out->nvoxels[k].resize((size_t)cap[k]);
    }
    const int rc = visfd_hip_find_extrema(
        context(), flat(src), flat(mask), image_size[0], image_size[1], image_size[2], find_minima ? 1 : 0,
        find_maxima ? 1 : 0, minima_threshold, maxima_threshold, connectivity, allow_borders ? 1 : 0,
        out->index[0].data(), out->score[0].data(), out->nvoxels[0].data(), cap[0], &n[0], out->index[1].data(),
        out->score[1].data(), out->nvoxels[1].data(), cap[1], &n[1], dest ? labels.data() : nullptr);
    if (rc != VISFD_HIP_ECAPACITY) {
      check(rc);
      break;
    }
    cap[0] = n[0] > cap[0] ? n[0] : cap[0];
    cap[1] = n[1] > cap[1] ? n[1] : cap[1];
  }
  for (int k = 0; k < 2; k++) {
    out->index[k].resize((size_t)n[k]);
    out->score[k].resize((size_t)n[k]);
    out->nvoxels[k].resize((size_t)n[k]);
  }
  if (dest) {
    size_t i = 0;
    for (int iz = 0; iz < image_size[2]; iz++)
      for (int iy = 0; iy < image_size[1]; iy++)
        for (int ix = 0; ix < image_size[0]; ix++, i++)
          if (!mask || mask[iz][iy][ix] != 0.0f) dest[iz][iy][ix] = (Label)labels[i];
  }
  return (size_t)(n[0] + n[1]);
}
template <typename T, typename S>
inline void assign(std::vector<T>* dst, const std::vector<S>& src) {
  if (!dst) return;
  dst->resize(src.size());
  for (size_t k = 0; k < src.size(); k++) (*dst)[k] = (T)src[k];
}
template <typename Coordinate>
inline void assign_crds(std::vector<std::array<Coordinate, 3> >* dst, const std::vector<int64_t>& index,
                        const int image_size[3]) {
  if (!dst) return;
  dst->resize(index.size());
  for (size_t k = 0; k < index.size(); k++) {
    size_t i = (size_t)index[k];
    (*dst)[k][0] = (Coordinate)(i % image_size[0]);
    i /= image_size[0];
    (*dst)[k][1] = (Coordinate)(i % image_size[1]);
    (*dst)[k][2] = (Coordinate)(i / image_size[1]);
  }
}
}  // namespace hip_detail

// both lists, locations as linear indices ix + nx * (iy + ny * iz); a null index list means that kind is not sought
template <typename IntegerIndex, typename Label>
size_t _FindExtrema(int const image_size[3], float const* const* const* aaafSource, float const* const* const* aaafMask,
                    std::vector<IntegerIndex>* pv_minima_indices, std::vector<IntegerIndex>* pv_maxima_indices,
                    std::vector<float>* pv_minima_scores, std::vector<float>* pv_maxima_scores,
                    std::vector<IntegerIndex>* pv_minima_nvoxels, std::vector<IntegerIndex>* pv_maxima_nvoxels,
                    float minima_threshold = std::numeric_limits<float>::infinity(),
                    float maxima_threshold = -std::numeric_limits<float>::infinity(), int connectivity = 3,
                    bool allow_borders = true, Label*** aaaiDest = nullptr, std::ostream* = nullptr) {
  hip_detail::ExtremaLists l;
  const bool find_minima = pv_minima_indices != nullptr, find_maxima = pv_maxima_indices != nullptr;
  const size_t n = hip_detail::find_extrema(image_size, aaafSource, aaafMask, find_minima, find_maxima, minima_threshold,
                                            maxima_threshold, connectivity, allow_borders, aaaiDest, &l);
  if (find_minima) {
    hip_detail::assign(pv_minima_indices, l.index[0]);
    hip_detail::assign(pv_minima_scores, l.score[0]);
    hip_detail::assign(pv_minima_nvoxels, l.nvoxels[0]);
  }
  if (find_maxima) {
    hip_detail::assign(pv_maxima_indices, l.index[1]);
    hip_detail::assign(pv_maxima_scores, l.score[1]);
    hip_detail::assign(pv_maxima_nvoxels, l.nvoxels[1]);
  }
  return n;
}
// both lists, locations as (ix, iy, iz)
template <typename Coordinate, typename IntegerIndex, typename Label>
size_t _FindExtrema(int const image_size[3], float const* const* const* aaafI, float const* const* const* aaafMask,
                    std::vector<std::array<Coordinate, 3> >* pva_minima_crds,
                    std::vector<std::array<Coordinate, 3> >* pva_maxima_crds, std::vector<float>* pv_minima_scores,
                    std::vector<float>* pv_maxima_scores, std::vector<IntegerIndex>* pv_minima_nvoxels,
                    std::vector<IntegerIndex>* pv_maxima_nvoxels,
                    float minima_threshold = std::numeric_limits<float>::infinity(),
                    float maxima_threshold = -std::numeric_limits<float>::infinity(), int connectivity = 3,
                    bool allow_borders = true, Label*** aaaiDest = nullptr, std::ostream* = nullptr) {
  hip_detail::ExtremaLists l;
  const bool find_minima = pva_minima_crds != nullptr, find_maxima = pva_maxima_crds != nullptr;
  const size_t n = hip_detail::find_extrema(image_size, aaafI, aaafMask, find_minima, find_maxima, minima_threshold,
                                            maxima_threshold, connectivity, allow_borders, aaaiDest, &l);
  if (find_minima) {
    hip_detail::assign_crds(pva_minima_crds, l.index[0], image_size);
    hip_detail::assign(pv_minima_scores, l.score[0]);
    hip_detail::assign(pv_minima_nvoxels, l.nvoxels[0]);
  }
  if (find_maxima) {
    hip_detail::assign_crds(pva_maxima_crds, l.index[1], image_size);
    hip_detail::assign(pv_maxima_scores, l.score[1]);
    hip_detail::assign(pv_maxima_nvoxels, l.nvoxels[1]);
  }
  return n;
}
// one kind, locations as (ix, iy, iz).  Seeking maxima, a threshold of +inf means none (morphology_implementation.hpp:775-776).
template <typename Coordinate, typename IntegerIndex, typename Label>
size_t _FindExtrema(int const image_size[3], float const* const* const* aaafI, float const* const* const* aaafMask,
                    std::vector<std::array<Coordinate, 3> >& extrema_crds, std::vector<float>& extrema_scores,
                    std::vector<IntegerIndex>& extrema_nvoxels, bool seek_minima = true,
                    float threshold = std::numeric_limits<float>::infinity(), int connectivity = 3,
                    bool allow_borders = true, Label*** aaaiDest = nullptr, std::ostream* = nullptr) {
  const float inf = std::numeric_limits<float>::infinity();
  std::vector<std::array<Coordinate, 3> >* none_crds = nullptr;
  std::vector<float>* none_scores = nullptr;
  std::vector<IntegerIndex>* none_nvoxels = nullptr;
  if (seek_minima)
    return _FindExtrema(image_size, aaafI, aaafMask, &extrema_crds, none_crds, &extrema_scores, none_scores,
                        &extrema_nvoxels, none_nvoxels, threshold, -inf, connectivity, allow_borders, aaaiDest);
  if (threshold == inf) threshold = -inf;
  return _FindExtrema(image_size, aaafI, aaafMask, none_crds, &extrema_crds, none_scores, &extrema_scores, none_nvoxels,
                      &extrema_nvoxels, inf, threshold, connectivity, allow_borders, aaaiDest);
}
template <typename Coordinate, typename IntegerIndex, typename Label>
size_t FindMinima(int const image_size[3], float const* const* const* aaafI, float const* const* const* aaafMask,
                  std::vector<std::array<Coordinate, 3> >& minima_crds, std::vector<float>& minima_scores,
                  std::vector<IntegerIndex>& minima_nvoxels, float threshold = std::numeric_limits<float>::infinity(),
                  int connectivity = 3, bool allow_borders = true, Label*** aaaiDest = nullptr,
                  std::ostream* pReportProgress = nullptr) {
  return _FindExtrema(image_size, aaafI, aaafMask, minima_crds, minima_scores, minima_nvoxels, true, threshold,
                      connectivity, allow_borders, aaaiDest, pReportProgress);
}
template <typename Coordinate, typename IntegerIndex, typename Label>
size_t FindMaxima(int const image_size[3], float const* const* const* aaafI, float const* const* const* aaafMask,
                  std::vector<std::array<Coordinate, 3> >& maxima_crds, std::vector<float>& maxima_scores,
                  std::vector<IntegerIndex>& maxima_nvoxels, float threshold = std::numeric_limits<float>::infinity(),
                  int connectivity = 3, bool allow_borders = true, Label*** aaaiDest = nullptr,
                  std::ostream* pReportProgress = nullptr) {
  return _FindExtrema(image_size, aaafI, aaafMask, maxima_crds, maxima_scores, maxima_nvoxels, false, threshold,
                      connectivity, allow_borders, aaaiDest, pReportProgress);
}

// ---- watershed segmentation: lib/visfd/segmentation.hpp:65-559 -------------------------------------------------------------
// The reference's signature and defaults with Scalar = float and any integer Label.  aaaiDest is written everywhere: basin
// k of the seed list as k + 1 (or its marker's label), label_boundary, label_undefined, and -1 where the mask is 0.  Labels
// travel through the C ABI as int32: marker labels, label_boundary and label_undefined outside its range are refused.
// Without markers the labels are computed on the GPU; with markers the sequential flood runs on the host (visfd_hip.h).
// The progress stream is ignored.
template <typename Label, typename Coordinate>
size_t Watershed(int const image_size[3], float const* const* const* aaafSource, Label*** aaaiDest,
                 float const* const* const* aaafMask, Label const* const* const* aaaiMarkers = nullptr,
                 float halt_threshold = std::numeric_limits<float>::infinity(), bool start_from_minima = true,
                 int connectivity = 1, bool show_boundaries = true, Label label_boundary = 0, Label label_undefined = -1,
                 std::vector<std::array<Coordinate, 3> >* pv_basin_locations = nullptr,
                 std::vector<float>* pv_basin_scores = nullptr, std::ostream* = nullptr) {
  hip_detail::require_contiguous(aaafSource, image_size);
  hip_detail::require_contiguous(aaafMask, image_size);
  const float inf = std::numeric_limits<float>::infinity();
  if (!start_from_minima && halt_threshold == inf) halt_threshold = -inf;   // segmentation.hpp:125-134
  const size_t nvox = (size_t)image_size[0] * image_size[1] * image_size[2];
  const long long lo = std::numeric_limits<int32_t>::min(), hi = std::numeric_limits<int32_t>::max();
  if ((long long)label_boundary < lo || (long long)label_boundary > hi || (long long)label_undefined < lo ||
      (long long)label_undefined > hi)
    throw VisfdErr("visfd_hip: Watershed: label_boundary and label_undefined must fit 32 bits");
  std::vector<int32_t> labels(nvox), markers(aaaiMarkers ? nvox : 0);
  if (aaaiMarkers) {
    size_t i = 0;
    for (int iz = 0; iz < image_size[2]; iz++)
      for (int iy = 0; iy < image_size[1]; iy++)
        for (int ix = 0; ix < image_size[0]; ix++, i++) {
          const long long m = (long long)aaaiMarkers[iz][iy][ix];
          if (m > hi) throw VisfdErr("visfd_hip: Watershed: marker labels must fit 32 bits");
          markers[i] = m < 0 ? -1 : (int32_t)m;   // entries <= 0 are ignored alike
        }
  }
  const int64_t cap0 = (int64_t)(nvox / 32) > 65536 ? (int64_t)(nvox / 32) : 65536;
  std::vector<int64_t> index((size_t)cap0);
  std::vector<float> score((size_t)cap0);
  int64_t n = 0;
  for (;;) {
    const int rc = visfd_hip_watershed(hip_detail::context(), hip_detail::flat(aaafSource), hip_detail::flat(aaafMask),
                                       aaaiMarkers ? markers.data() : nullptr, image_size[0], image_size[1], image_size[2],
                                       halt_threshold, start_from_minima ? 1 : 0, connectivity, show_boundaries ? 1 : 0,
                                       (int32_t)label_boundary, (int32_t)label_undefined, labels.data(), index.data(),
                                       score.data(), (int64_t)index.size(), &n);
    if (rc != VISFD_HIP_ECAPACITY) {
      hip_detail::check(rc);
      break;
    }
    index.resize((size_t)n);
    score.resize((size_t)n);
  }
  index.resize((size_t)n);
  score.resize((size_t)n);
  hip_detail::assign_crds(pv_basin_locations, index, image_size);
  hip_detail::assign(pv_basin_scores, score);
  size_t i = 0;
  for (int iz = 0; iz < image_size[2]; iz++)
    for (int iy = 0; iy < image_size[1]; iy++)
      for (int ix = 0; ix < image_size[0]; ix++, i++) aaaiDest[iz][iy][ix] = (Label)labels[i];
  return (size_t)n;
}

// ---- Filter3D: lib/visfd/filter3d.hpp:37-530 ---------------------------------------------------------------------------
// The reference's public face: aaafH indexable [jz][jy][jx] from -halfwidth to +halfwidth, halfwidth, array_size, both
// Apply overloads (on the GPU: visfd_hip_filter3d), the table arithmetic, copy, move and assignment.  What Apply computes,
// what it defines where the reference has nothing to say (voxels with mask == 0 get 0, with or without a denominator)
// and its one divergence (a NaN or Inf under a zero weight or outside the mask does not spread) are in visfd_hip.h.
template <typename Scalar, typename Integer>
class Filter3D {
 public:
  Scalar*** aaafH;
  Integer halfwidth[3];
  Integer array_size[3];

  // filter3d.hpp:81-109: g = sum h * f * mask, divided by the sum of the weights considered when `normalize`
  void Apply(Integer const size_source[3], Scalar const* const* const* aaafSource, Scalar*** aaafDest,
             Scalar const* const* const* aaafMask = nullptr, bool normalize = false,
             std::ostream* pReportProgress = nullptr) const {
    run(size_source, aaafSource, aaafDest, aaafMask, normalize, nullptr, pReportProgress);
  }
  // filter3d.hpp:150-198: never normalises; hands back the denominator where aaafDenominator is given
  void Apply(Integer const size_source[3], Scalar const* const* const* aaafSource, Scalar*** aaafDest,
             Scalar const* const* const* aaafMask = nullptr, Scalar*** aaafDenominator = nullptr,
             std::ostream* pReportProgress = nullptr) const {
    run(size_source, aaafSource, aaafDest, aaafMask, false, aaafDenominator, pReportProgress);
  }

  void Normalize() {   // filter3d.hpp:202-214
    Scalar total = 0.0;
    for (size_t k = 0; k < data_.size(); k++) total += data_[k];
    for (size_t k = 0; k < data_.size(); k++) data_[k] /= total;
  }
  // filter3d.hpp:274-384; aaafW: optional weights, indexed like aaafH
  Scalar Average(Scalar const* const* const* aaafW = nullptr) const { return wsum(aaafW, 1) / wsum(aaafW, 0); }
  Scalar AverageSqr(Scalar const* const* const* aaafW = nullptr) const { return wsum(aaafW, 2) / wsum(aaafW, 0); }
  Scalar StdDev(Scalar const* const* const* aaafW = nullptr) const {
    return static_cast<Scalar>(std::sqrt(wsum(aaafW, 2, Average(aaafW)) / wsum(aaafW, 0)));
  }
  Scalar Sum(Scalar const* const* const* aaafW = nullptr) const { return wsum(aaafW, 1); }
  Scalar SumSqr(Scalar const* const* const* aaafW = nullptr) const { return wsum(aaafW, 2); }
  void AddScalar(Scalar offset) { for (size_t k = 0; k < data_.size(); k++) data_[k] += offset; }
  void MultiplyScalar(Scalar scale) { for (size_t k = 0; k < data_.size(); k++) data_[k] *= scale; }

  Filter3D() { Init(); }
  Filter3D(Integer const set_halfwidth[3]) { Init(); Resize(set_halfwidth); }
  virtual ~Filter3D() {}
  Filter3D(const Filter3D<Scalar, Integer>& source) {
    Init();
    if (source.aaafH) {
      Resize(source.halfwidth);
      data_ = source.data_;
    }
  }
  void swap(Filter3D<Scalar, Integer>& other) {
    data_.swap(other.data_);   // the buffers change owners where they lie: the pointers into them stay good
    rows_.swap(other.rows_);
    planes_.swap(other.planes_);
    std::swap(aaafH, other.aaafH);
    for (int d = 0; d < 3; d++) {
      std::swap(halfwidth[d], other.halfwidth[d]);
      std::swap(array_size[d], other.array_size[d]);
    }
  }
  Filter3D(Filter3D<Scalar, Integer>&& other) { Init(); this->swap(other); }
  Filter3D<Scalar, Integer>& operator=(Filter3D<Scalar, Integer> source) { this->swap(source); return *this; }

  // the table as the C ABI takes it: (2 hx + 1)(2 hy + 1)(2 hz + 1) numbers, x fastest
  Scalar* flat_table() { return data_.empty() ? nullptr : &data_[0]; }
  const Scalar* flat_table() const { return data_.empty() ? nullptr : &data_[0]; }

 private:
  std::vector<Scalar> data_;
  std::vector<Scalar*> rows_;
  std::vector<Scalar**> planes_;

  void Init() {
    aaafH = nullptr;
    for (int d = 0; d < 3; d++) halfwidth[d] = array_size[d] = -1;
  }
  void Resize(Integer const set_halfwidth[3]) {
    for (int d = 0; d < 3; d++) {
      if (set_halfwidth[d] < 0) throw VisfdErr("visfd_hip: filter half-widths must not be negative");
      halfwidth[d] = set_halfwidth[d];
      array_size[d] = 1 + 2 * halfwidth[d];
    }
    const size_t sx = array_size[0], sy = array_size[1], sz = array_size[2];
    data_.assign(sx * sy * sz, (Scalar)-1.0e38);   // as the reference fills a new table
    rows_.resize(sy * sz);
    planes_.resize(sz);
    for (size_t k = 0; k < sy * sz; k++) rows_[k] = &data_[0] + k * sx + halfwidth[0];
    for (size_t k = 0; k < sz; k++) planes_[k] = &rows_[0] + k * sy + halfwidth[1];
    aaafH = &planes_[0] + halfwidth[2];
  }
  // what = 0: sum of w; 1: sum of w * h; 2: sum of w * (h - shift)^2
  Scalar wsum(Scalar const* const* const* aaafW, int what, Scalar shift = 0.0) const {
    Scalar sum = 0.0;
    for (Integer iz = -halfwidth[2]; iz <= halfwidth[2]; iz++)
      for (Integer iy = -halfwidth[1]; iy <= halfwidth[1]; iy++)
        for (Integer ix = -halfwidth[0]; ix <= halfwidth[0]; ix++) {
          const Scalar w = aaafW ? aaafW[iz][iy][ix] : (Scalar)1.0;
          const Scalar h = aaafH[iz][iy][ix] - shift;
          sum += what == 0 ? w : what == 1 ? w * h : w * (h * h);
        }
    return sum;
  }
  void run(Integer const size_source[3], float const* const* const* src, float*** dest, float const* const* const* mask,
           bool normalize, float*** den, std::ostream* pReportProgress) const {
    const int size[3] = {(int)size_source[0], (int)size_source[1], (int)size_source[2]};
    const int hw[3] = {(int)halfwidth[0], (int)halfwidth[1], (int)halfwidth[2]};
    hip_detail::require_contiguous(src, size);
    hip_detail::require_contiguous(dest, size);
    hip_detail::require_contiguous(mask, size);
    hip_detail::require_contiguous(den, size);
    if (pReportProgress) *pReportProgress << "  progress: applying the 3-D filter on the GPU" << std::endl;
    hip_detail::check(visfd_hip_filter3d(hip_detail::context(), hip_detail::flat(src), hip_detail::flat(dest),
                                         hip_detail::flat(mask), size[0], size[1], size[2], flat_table(), hw,
                                         normalize ? 1 : 0, hip_detail::flat(den)));
  }
};

// lib/visfd/filter3d.hpp:546-601: h(x,y,z) = A*exp(-r^m), r = sqrt((x/s_x)^2 + (y/s_y)^2 + (z/s_z)^2), entries below
// the smallest face value zeroed, the sum 1
inline Filter3D<float, int> GenFilterGenGauss3D(const float width[3], float m_exp, const int truncate_halfwidth[3],
                                                float* pA = nullptr) {
  Filter3D<float, int> filter(truncate_halfwidth);
  int64_t n = 0;
  hip_detail::check(visfd_hip_gengauss3d_table(width, m_exp, truncate_halfwidth, filter.flat_table(),
                                               (int64_t)filter.array_size[0] * filter.array_size[1] * filter.array_size[2],
                                               &n, pA));
  return filter;
}
// :618-638: the window is floor(width * filter_cutoff_ratio)
inline Filter3D<float, int> GenFilterGenGauss3D(const float width[3], float m_exp, const float filter_cutoff_ratio = 2.5,
                                                float* pA = nullptr) {
  if (filter_cutoff_ratio < 0) throw VisfdErr("visfd_hip: the filter cutoff ratio must not be negative");
  int hw[3];
  hip_detail::check(visfd_hip_gengauss3d_halfwidths(width, m_exp, filter_cutoff_ratio, 0.0f, hw));
  return GenFilterGenGauss3D(width, m_exp, hw, pA);
}

// ---- LocalFluctuations: lib/visfd/filter3d.hpp:1698-1711 (any exponent; 2 takes the separable Gaussians) -------
inline void LocalFluctuations(const int image_size[3], float const* const* const* src, float*** dest,
                              float const* const* const* mask, const float sigma[3],
                              float template_background_exponent = 2, float filter_truncate_ratio = 2.5,
                              bool normalize = true, std::ostream* = nullptr) {
  hip_detail::require_contiguous(src, image_size);
  hip_detail::require_contiguous(dest, image_size);
  hip_detail::require_contiguous(mask, image_size);
  hip_detail::check(visfd_hip_local_fluctuations_gen(hip_detail::context(), hip_detail::flat(src), hip_detail::flat(dest),
                                                     hip_detail::flat(mask), image_size[0], image_size[1], image_size[2],
                                                     sigma, template_background_exponent, filter_truncate_ratio,
                                                     normalize ? 1 : 0));
}
// ---- LocalFluctuationsByRadius: lib/visfd/filter3d.hpp:1897-1926 and the variant with a decay threshold,
//      bin/filter_mrc/filter3d_variants.hpp:651-681 (a negative ratio selects the threshold) --------------
inline void LocalFluctuationsByRadius(const int image_size[3], float const* const* const* src, float*** dest,
                                      float const* const* const* mask, const float radius[3],
                                      float template_background_exponent, float filter_truncate_ratio,
                                      float filter_truncate_threshold, bool normalize = true,
                                      std::ostream* pReportProgress = nullptr) {
  float sigma[3], ratio;
  hip_detail::check(visfd_hip_fluctuation_sigmas(radius, template_background_exponent, filter_truncate_ratio,
                                                 filter_truncate_threshold, sigma, &ratio));
  LocalFluctuations(image_size, src, dest, mask, sigma, template_background_exponent, ratio, normalize,
                    pReportProgress);
}
inline void LocalFluctuationsByRadius(const int image_size[3], float const* const* const* src, float*** dest,
                                      float const* const* const* mask, const float radius[3],
                                      float template_background_exponent = 2, float filter_truncate_ratio = 2.5,
                                      bool normalize = true, std::ostream* pReportProgress = nullptr) {
  // a non-negative ratio is taken as is (the threshold argument is then unused)
  LocalFluctuationsByRadius(image_size, src, dest, mask, radius, template_background_exponent,
                            filter_truncate_ratio < 0 ? 0.0f : filter_truncate_ratio, 0.02f, normalize, pReportProgress);
}

// ---- BlobDog: lib/visfd/feature.hpp:53-77 --------------------------------------------------------------
// The optional preallocated-images argument of the reference (aaaafI) is accepted and ignored: the
// rolling LoG volumes live in HBM.
inline void BlobDog(int const image_size[3], float const* const* const* aaafSource,
                    float const* const* const* aaafMask, const std::vector<float>& blob_sigma,
                    std::vector<std::array<float, 3> >* pva_minima_crds = nullptr,
                    std::vector<std::array<float, 3> >* pva_maxima_crds = nullptr,
                    std::vector<float>* pv_minima_sigma = nullptr, std::vector<float>* pv_maxima_sigma = nullptr,
                    std::vector<float>* pv_minima_scores = nullptr, std::vector<float>* pv_maxima_scores = nullptr,
                    const float aspect_ratio[3] = nullptr, float delta_sigma_over_sigma = 0.02,
                    float truncate_ratio = 2.5,
                    float minima_threshold = std::numeric_limits<float>::infinity(),
                    float maxima_threshold = -std::numeric_limits<float>::infinity(),
                    bool use_threshold_ratios = true, std::ostream* pReportProgress = nullptr,
                    float**** /*aaaafI*/ = nullptr) {
  hip_detail::require_contiguous(aaafSource, image_size);
  hip_detail::require_contiguous(aaafMask, image_size);
  if (pReportProgress)
    *pReportProgress << "\n----- Blob detection initiated using " << blob_sigma.size()
                     << " trial Gaussians -----\n\n";
  int64_t cap = 1 << 16, nmin = 0, nmax = 0;
  std::vector<visfd_hip_blob> mins, maxs;
  for (int attempt = 0; attempt < 2; attempt++) {
    mins.resize((size_t)cap);
    maxs.resize((size_t)cap);
    int rc = visfd_hip_blob_dog(hip_detail::context(), hip_detail::flat(aaafSource), hip_detail::flat(aaafMask),
                                image_size[0], image_size[1], image_size[2], blob_sigma.data(),
                                (int)blob_sigma.size(), aspect_ratio, delta_sigma_over_sigma, truncate_ratio,
                                minima_threshold, maxima_threshold, use_threshold_ratios ? 1 : 0, mins.data(), cap,
                                &nmin, maxs.data(), cap, &nmax);
    if (rc == VISFD_HIP_ECAPACITY) { cap = (nmin > nmax ? nmin : nmax); continue; }
    hip_detail::check(rc);
    break;
  }
  for (int side = 0; side < 2; side++) {
    const std::vector<visfd_hip_blob>& L = side ? maxs : mins;
    const int64_t n = side ? nmax : nmin;
    std::vector<std::array<float, 3> >* crds = side ? pva_maxima_crds : pva_minima_crds;
    std::vector<float>* sig = side ? pv_maxima_sigma : pv_minima_sigma;
    std::vector<float>* sc = side ? pv_maxima_scores : pv_minima_scores;
    for (int64_t i = 0; i < n; i++) {
      if (crds) {
        std::array<float, 3> c;
        c[0] = (float)L[i].ix; c[1] = (float)L[i].iy; c[2] = (float)L[i].iz;
        crds->push_back(c);
      }
      if (sig) sig->push_back(L[i].sigma);
      if (sc) sc->push_back(L[i].score);
    }
  }
  if (pReportProgress)
    *pReportProgress << "--- (Found " << nmin << " and " << nmax
                     << " local minima and maxima, respectively) ---\n" << std::endl;
}

// ---- BlobDogD: lib/visfd/feature.hpp:446-470 ------------------------------------------------------------
inline void BlobDogD(int const image_size[3], float const* const* const* aaafSource,
                     float const* const* const* aaafMask, const std::vector<float>& blob_diameters,
                     std::vector<std::array<float, 3> >* pva_minima_crds = nullptr,
                     std::vector<std::array<float, 3> >* pva_maxima_crds = nullptr,
                     std::vector<float>* pv_minima_diameters = nullptr,
                     std::vector<float>* pv_maxima_diameters = nullptr,
                     std::vector<float>* pv_minima_scores = nullptr, std::vector<float>* pv_maxima_scores = nullptr,
                     const float aspect_ratio[3] = nullptr, float delta_sigma_over_sigma = 0.02,
                     float truncate_ratio = 2.5,
                     float minima_threshold = std::numeric_limits<float>::infinity(),
                     float maxima_threshold = -std::numeric_limits<float>::infinity(),
                     bool use_threshold_ratios = false, std::ostream* pReportProgress = nullptr,
                     float**** aaaafI = nullptr) {
  std::vector<float> blob_sigma(blob_diameters.size()), min_sig, max_sig;
  hip_detail::check(visfd_hip_blob_diameters_to_sigmas(blob_diameters.data(), (int)blob_diameters.size(),
                                                       blob_sigma.data()));
  BlobDog(image_size, aaafSource, aaafMask, blob_sigma, pva_minima_crds, pva_maxima_crds, &min_sig, &max_sig,
          pv_minima_scores, pv_maxima_scores, aspect_ratio, delta_sigma_over_sigma, truncate_ratio,
          minima_threshold, maxima_threshold, use_threshold_ratios, pReportProgress, aaaafI);
  if (pv_minima_diameters) {
    pv_minima_diameters->resize(min_sig.size());
    hip_detail::check(visfd_hip_blob_sigmas_to_diameters(min_sig.data(), (int)min_sig.size(),
                                                         pv_minima_diameters->data()));
  }
  if (pv_maxima_diameters) {
    pv_maxima_diameters->resize(max_sig.size());
    hip_detail::check(visfd_hip_blob_sigmas_to_diameters(max_sig.data(), (int)max_sig.size(),
                                                         pv_maxima_diameters->data()));
  }
}

// ---- BinArray3D / UnbinArray3D: lib/visfd/resample.hpp:53-58, :120-124 ---------------------------------
inline void BinArray3D(int const size_source[3], int const size_dest[3], float const* const* const* aaafSource,
                       float*** aaafDest, int const* offset = nullptr) {
  hip_detail::require_contiguous(aaafSource, size_source);
  hip_detail::require_contiguous(aaafDest, size_dest);
  const int64_t ss[3] = {size_source[0], size_source[1], size_source[2]}, ds[3] = {size_dest[0], size_dest[1], size_dest[2]};
  hip_detail::check(visfd_hip_bin_array3d(hip_detail::context(), hip_detail::flat(aaafSource), ss,
                                          hip_detail::flat(aaafDest), ds, offset));
}
inline void UnbinArray3D(int const size_source[3], int const size_dest[3], float const* const* const* aaafSource,
                         float*** aaafDest, int const* offset = nullptr) {
  hip_detail::require_contiguous(aaafSource, size_source);
  hip_detail::require_contiguous(aaafDest, size_dest);
  const int64_t ss[3] = {size_source[0], size_source[1], size_source[2]}, ds[3] = {size_dest[0], size_dest[1], size_dest[2]};
  hip_detail::check(visfd_hip_unbin_array3d(hip_detail::context(), hip_detail::flat(aaafSource), ss,
                                            hip_detail::flat(aaafDest), ds, offset));
}

// ---- drawing: lib/visfd/draw.hpp:46-81, :90-224, :238-457 --------------------------------------------------------
// A rectangle or a sphere with a brightness; `value` < 0 means "take these voxels away" under negative_means_subtract.
template <typename Scalar>
struct SimpleRegion {
  struct Rect { Scalar xmin, xmax, ymin, ymax, zmin, zmax; };
  struct Sphere { Scalar x0, y0, z0, r; };
  enum RegionType { RECT, SPHERE };
  RegionType type;
  union { Rect rect; Sphere sphere; } data;
  Scalar value;
  SimpleRegion() : type(RECT), value(1) {   // an empty rectangle
    data.rect.xmin = 0; data.rect.xmax = -1;
    data.rect.ymin = 0; data.rect.ymax = -1;
    data.rect.zmin = 0; data.rect.zmax = -1;
  }
};

template <typename Scalar>
void DrawRegions(int const image_size[3], Scalar*** aaafDest, Scalar const* const* const* aaafMask,
                 std::vector<SimpleRegion<Scalar> > vRegions, bool negative_means_subtract = false) {
  static_assert(std::is_same<Scalar, float>::value, "visfd_hip draws float images");
  hip_detail::require_contiguous(aaafDest, image_size);
  hip_detail::require_contiguous(aaafMask, image_size);
  std::vector<visfd_hip_region> r(vRegions.size());
  for (size_t i = 0; i < r.size(); i++) {
    const SimpleRegion<Scalar>& g = vRegions[i];
    r[i].value = g.value;
    for (int k = 0; k < 6; k++) r[i].c[k] = 0.0f;
    if (g.type == SimpleRegion<Scalar>::SPHERE) {
      r[i].type = VISFD_HIP_REGION_SPHERE;
      r[i].c[0] = g.data.sphere.x0; r[i].c[1] = g.data.sphere.y0; r[i].c[2] = g.data.sphere.z0; r[i].c[3] = g.data.sphere.r;
    } else {
      r[i].type = VISFD_HIP_REGION_RECT;
      r[i].c[0] = g.data.rect.xmin; r[i].c[1] = g.data.rect.xmax; r[i].c[2] = g.data.rect.ymin;
      r[i].c[3] = g.data.rect.ymax; r[i].c[4] = g.data.rect.zmin; r[i].c[5] = g.data.rect.zmax;
    }
  }
  hip_detail::check(visfd_hip_draw_regions(hip_detail::context(), hip_detail::flat(aaafDest), hip_detail::flat(aaafMask),
                                           image_size[0], image_size[1], image_size[2], r.empty() ? nullptr : r.data(),
                                           (int64_t)r.size(), negative_means_subtract ? 1 : 0));
}

// aaafDest may be aaafBackground.  A null background is an error here (the reference dereferences it).
template <typename Scalar>
void DrawSpheres(int const image_size[3], Scalar*** aaafDest, Scalar const* const* const* aaafMask,
                 const std::vector<std::array<Scalar, 3> >& centers, const std::vector<Scalar>* pDiameters = nullptr,
                 const std::vector<Scalar>* pShellThicknesses = nullptr,
                 const std::vector<Scalar>* pVoxelIntensitiesForeground = nullptr,
                 Scalar const* const* const* aaafBackground = nullptr, Scalar voxel_intensity_background_offset = 0.0,
                 Scalar voxel_intensity_background_rescale = 1.0, bool voxel_intensity_background_normalize = false,
                 bool voxel_intensity_foreground_normalize = false, std::ostream* pReportProgress = nullptr) {
  static_assert(std::is_same<Scalar, float>::value, "visfd_hip draws float images");
  hip_detail::require_contiguous(aaafDest, image_size);
  hip_detail::require_contiguous(aaafMask, image_size);
  hip_detail::require_contiguous(aaafBackground, image_size);
  const size_t n = centers.size();
  if ((pDiameters && pDiameters->size() != n) || (pShellThicknesses && pShellThicknesses->size() != n) ||
      (pVoxelIntensitiesForeground && pVoxelIntensitiesForeground->size() != n))
    throw VisfdErr("Error: DrawSpheres: the sphere lists differ in length.\n");
  std::vector<float> c(3 * n);
  for (size_t i = 0; i < n; i++) { c[3 * i] = centers[i][0]; c[3 * i + 1] = centers[i][1]; c[3 * i + 2] = centers[i][2]; }
  if (pReportProgress)   // draw.hpp:360-386
    for (size_t i = 0; i < n; i++) {
      const float d = pDiameters ? (*pDiameters)[i] : 0.0f;
      *pReportProgress << "processing coordinates " << i + 1 << " / " << n << ": x,y,z(in_voxels)=" << centers[i][0] << ","
                       << centers[i][1] << "," << centers[i][2] << ", diameter=" << d
                       << ", th=" << (pShellThicknesses ? (*pShellThicknesses)[i] : d / 2) << "\n";
    }
  int outside = 0;
  hip_detail::check(visfd_hip_draw_spheres(
      hip_detail::context(), hip_detail::flat(aaafDest), hip_detail::flat(aaafMask), hip_detail::flat(aaafBackground),
      image_size[0], image_size[1], image_size[2], n ? c.data() : nullptr, pDiameters && n ? pDiameters->data() : nullptr,
      pShellThicknesses && n ? pShellThicknesses->data() : nullptr,
      pVoxelIntensitiesForeground && n ? pVoxelIntensitiesForeground->data() : nullptr, (int64_t)n,
      voxel_intensity_background_offset, voxel_intensity_background_rescale, voxel_intensity_background_normalize ? 1 : 0,
      voxel_intensity_foreground_normalize ? 1 : 0, &outside));
  if (pReportProgress && outside)   // draw.hpp:447-455
    *pReportProgress << "------------------------------------------------------------------------------\n"
                        "WARNING:\n"
                        "    Some coordinates in the text file lie outside the boundaries of the image.\n"
                        "    Did you remember to set the voxel width correctly?\n"
                        "    (Did you use the \"-w\" argument?)\n"
                        "--------------------------------------------------------------------------=---\n"
                     << std::endl;
}

// ---- voxelising a closed mesh: what bin/voxelize_mesh/voxelize_mesh.py asks vtk, by the exact rule of visfd_hip.h --------
// aaafDest[iz][iy][ix] becomes 1 where sample (ix, iy, iz) lies inside the mesh and 0 elsewhere.  vertices are in physical
// units (divided by voxel_width), origin is the position of voxel 0 in voxels (null: 0, 0, 0); check_closed refuses a
// surface with boundary or non-manifold edges, as the script's check_surface=True does.  A null ctx is the shim's own.
inline void VoxelizeMesh(visfd_hip_ctx* ctx, int const image_size[3], const std::vector<std::array<float, 3> >& vertices,
                         const std::vector<std::array<int, 3> >& triangles, float*** aaafDest, double voxel_width = 1.0,
                         const double* origin = nullptr, bool check_closed = true) {
  hip_detail::require_contiguous(aaafDest, image_size);
  std::vector<float> v(3 * vertices.size());
  std::vector<int32_t> t(3 * triangles.size());
  for (size_t i = 0; i < vertices.size(); i++)
    for (int d = 0; d < 3; d++) v[3 * i + d] = vertices[i][d];
  for (size_t i = 0; i < triangles.size(); i++)
    for (int d = 0; d < 3; d++) t[3 * i + d] = triangles[i][d];
  const double zero[3] = {0.0, 0.0, 0.0};
  hip_detail::check(visfd_hip_voxelize_mesh(ctx ? ctx : hip_detail::context(), v.empty() ? nullptr : v.data(),
                                            (int64_t)vertices.size(), t.empty() ? nullptr : t.data(), (int64_t)triangles.size(),
                                            voxel_width, origin ? origin : zero, image_size[0], image_size[1], image_size[2],
                                            check_closed ? 1 : 0, hip_detail::flat(aaafDest)));
}

// ---- closing an oriented point cloud into a mask (visfd_hip.h states the definition) ---------------------
// aaafDest[iz][iy][ix] becomes 1 inside the solid the cloud bounds and 0 elsewhere.  points are in voxel coordinates (the
// cloud of -normals-file divided by the voxel width), orientation is VISFD_HIP_CLOSE_OUTWARD, _INWARD or _AUTO, pad the
// number of nodes the solve's box extends beyond the image on every face.  aaafChi (nullable) receives the field that was
// cut.  A null ctx is the shim's own.
inline void CloseSurface(visfd_hip_ctx* ctx, int const image_size[3], const std::vector<std::array<float, 3> >& points,
                         const std::vector<std::array<float, 3> >& normals, float*** aaafDest, int pad = 0,
                         int orientation = VISFD_HIP_CLOSE_OUTWARD, float*** aaafChi = nullptr) {
  hip_detail::require_contiguous(aaafDest, image_size);
  if (aaafChi) hip_detail::require_contiguous(aaafChi, image_size);
  if (points.size() != normals.size()) throw VisfdErr("Error: CloseSurface needs as many normals as points.\n");
  std::vector<float> p(3 * points.size()), m(3 * points.size());
  for (size_t i = 0; i < points.size(); i++)
    for (int d = 0; d < 3; d++) {
      p[3 * i + d] = points[i][d];
      m[3 * i + d] = normals[i][d];
    }
  hip_detail::check(visfd_hip_close_surface(ctx ? ctx : hip_detail::context(), p.empty() ? nullptr : p.data(),
                                            m.empty() ? nullptr : m.data(), (int64_t)points.size(), image_size[0], image_size[1],
                                            image_size[2], pad, orientation, hip_detail::flat(aaafDest),
                                            aaafChi ? hip_detail::flat(aaafChi) : nullptr));
}

// ---- the closed triangle mesh of a level set (visfd_hip.h states the definition) -------------------------
// The surface of {aaafSource < iso} (side VISFD_HIP_ISO_BELOW) or {aaafSource > iso} (_ABOVE) as vertices (x, y, z in voxel
// coordinates) and triangles with outward normals; closed also where the image border cuts the solid.  A null ctx is the
// shim's own.  Returns the number of triangles.
inline size_t IsoSurface(visfd_hip_ctx* ctx, int const image_size[3], float const* const* const* aaafSource, double iso, int side,
                         std::vector<std::array<float, 3> >& vertices, std::vector<std::array<int, 3> >& triangles) {
  hip_detail::require_contiguous(aaafSource, image_size);
  visfd_hip_ctx* c = ctx ? ctx : hip_detail::context();
  const float* src = hip_detail::flat(aaafSource);
  int64_t nv = 0, nt = 0;
  hip_detail::check(visfd_hip_isosurface(c, src, image_size[0], image_size[1], image_size[2], iso, side, nullptr, 0, nullptr, 0,
                                         &nv, &nt));
  std::vector<float> v(3 * (size_t)nv + 3);
  std::vector<int32_t> t(3 * (size_t)nt + 3);
  hip_detail::check(visfd_hip_isosurface(c, src, image_size[0], image_size[1], image_size[2], iso, side, v.data(), nv, t.data(),
                                         nt, &nv, &nt));
  vertices.resize((size_t)nv);
  triangles.resize((size_t)nt);
  for (size_t i = 0; i < (size_t)nv; i++)
    for (int d = 0; d < 3; d++) vertices[i][d] = v[3 * i + d];
  for (size_t i = 0; i < (size_t)nt; i++)
    for (int d = 0; d < 3; d++) triangles[i][d] = (int)t[3 * i + d];
  return (size_t)nt;
}

// ---- blob list post-processing: lib/visfd/visfd_utils.hpp:49-55,95-118; feature.hpp:519-616,720-969 ------
typedef enum eSortCriteria {
  DO_NOT_SORT = VISFD_HIP_DO_NOT_SORT,
  SORT_DECREASING = VISFD_HIP_SORT_DECREASING,
  SORT_INCREASING = VISFD_HIP_SORT_INCREASING,
  SORT_DECREASING_MAGNITUDE = VISFD_HIP_SORT_DECREASING_MAGNITUDE,
  SORT_INCREASING_MAGNITUDE = VISFD_HIP_SORT_INCREASING_MAGNITUDE
} SortCriteria;

inline float CalcSphereOverlap(float rij, float Ri, float Rj) { return visfd_hip_sphere_overlap(rij, Ri, Rj); }

namespace hip_detail {
struct FlatBlobs {   // the three parallel vectors as the flat arrays of the C ABI, and back
  std::vector<float> c, d, s;
  FlatBlobs(const std::vector<std::array<float, 3> >& crds, const std::vector<float>& diam,
            const std::vector<float>& score) : c(3 * crds.size()), d(diam), s(score) {
    if (diam.size() != crds.size() || score.size() != crds.size())
      throw VisfdErr("Error: blob coordinate, diameter and score lists differ in length.\n");
    for (size_t i = 0; i < crds.size(); i++) { c[3 * i] = crds[i][0]; c[3 * i + 1] = crds[i][1]; c[3 * i + 2] = crds[i][2]; }
  }
  void store(size_t n, std::vector<std::array<float, 3> >& crds, std::vector<float>& diam, std::vector<float>& score) {
    crds.resize(n); diam.assign(d.begin(), d.begin() + n); score.assign(s.begin(), s.begin() + n);
    for (size_t i = 0; i < n; i++) { crds[i][0] = c[3 * i]; crds[i][1] = c[3 * i + 1]; crds[i][2] = c[3 * i + 2]; }
  }
};
}  // namespace hip_detail

inline void SortBlobs(std::vector<std::array<float, 3> >& blob_crds, std::vector<float>& blob_diameters,
                      std::vector<float>& blob_scores, SortCriteria sort_blob_criteria, bool ascending_order = true,
                      std::vector<size_t>* pPermutation = nullptr, std::ostream* pReportProgress = nullptr) {
  hip_detail::FlatBlobs f(blob_crds, blob_diameters, blob_scores);
  std::vector<uint64_t> perm(blob_crds.size());
  if (pReportProgress && !blob_crds.empty() && sort_blob_criteria != DO_NOT_SORT)
    *pReportProgress << "-- Sorting blobs according to their scores... ";
  hip_detail::check(visfd_hip_sort_blobs(f.c.data(), f.d.data(), f.s.data(), (int64_t)blob_crds.size(),
                                         (int)sort_blob_criteria, ascending_order ? 1 : 0, perm.data()));
  f.store(blob_crds.size(), blob_crds, blob_diameters, blob_scores);
  if (pPermutation && !blob_crds.empty() && sort_blob_criteria != DO_NOT_SORT) pPermutation->assign(perm.begin(), perm.end());
  if (pReportProgress && !blob_crds.empty() && sort_blob_criteria != DO_NOT_SORT) *pReportProgress << "done --" << std::endl;
}

// the (ascending_order, ignore_score_sign) form, feature.hpp:519-560
inline void SortBlobs(std::vector<std::array<float, 3> >& blob_crds, std::vector<float>& blob_diameters,
                      std::vector<float>& blob_scores, bool ascending_order = true, bool ignore_score_sign = true,
                      std::vector<size_t>* pPermutation = nullptr, std::ostream* pReportProgress = nullptr) {
  SortBlobs(blob_crds, blob_diameters, blob_scores, ignore_score_sign ? SORT_DECREASING_MAGNITUDE : SORT_DECREASING,
            ascending_order, pPermutation, pReportProgress);
}

// image_size is needed here (the reference indexes the mask unchecked): pass the mask's dimensions
inline void DiscardMaskedBlobs(std::vector<std::array<float, 3> >& blob_crds, std::vector<float>& blob_diameters,
                               std::vector<float>& blob_scores, float const* const* const* aaafMask,
                               int const image_size[3], std::ostream* pReportProgress = nullptr) {
  if (!aaafMask) return;
  hip_detail::FlatBlobs f(blob_crds, blob_diameters, blob_scores);
  int64_t n = (int64_t)blob_crds.size();
  hip_detail::check(visfd_hip_discard_masked_blobs(f.c.data(), f.d.data(), f.s.data(), &n, &aaafMask[0][0][0],
                                                   image_size[0], image_size[1], image_size[2]));
  if (pReportProgress)
    *pReportProgress << "  discarded " << (blob_crds.size() - (size_t)n) << "  blobs lying outside the mask." << std::endl;
  f.store((size_t)n, blob_crds, blob_diameters, blob_scores);
}

inline void DiscardOverlappingBlobs(std::vector<std::array<float, 3> >& blob_crds, std::vector<float>& blob_diameters,
                                    std::vector<float>& blob_scores, float min_radial_separation_ratio,
                                    float max_volume_overlap_large = std::numeric_limits<float>::infinity(),
                                    float max_volume_overlap_small = std::numeric_limits<float>::infinity(),
                                    SortCriteria sort_blob_criteria = SORT_DECREASING_MAGNITUDE,
                                    std::ostream* pReportProgress = nullptr, int scale = 6) {
  hip_detail::FlatBlobs f(blob_crds, blob_diameters, blob_scores);
  int64_t n = (int64_t)blob_crds.size();
  if (pReportProgress) *pReportProgress << "  detecting collisions between " << n << " blobs... ";
  hip_detail::check(visfd_hip_discard_overlapping_blobs(f.c.data(), f.d.data(), f.s.data(), &n,
                                                        min_radial_separation_ratio, max_volume_overlap_large,
                                                        max_volume_overlap_small, (int)sort_blob_criteria, scale));
  f.store((size_t)n, blob_crds, blob_diameters, blob_scores);
  if (pReportProgress) *pReportProgress << "done.\n";
}

// The same on a context's device (visfd_hip_discard_overlapping_blobs_ctx): the same lists bit for bit, the same progress
// text.  A null context is the host form above.
inline void DiscardOverlappingBlobs(visfd_hip_ctx* ctx, std::vector<std::array<float, 3> >& blob_crds,
                                    std::vector<float>& blob_diameters, std::vector<float>& blob_scores,
                                    float min_radial_separation_ratio,
                                    float max_volume_overlap_large = std::numeric_limits<float>::infinity(),
                                    float max_volume_overlap_small = std::numeric_limits<float>::infinity(),
                                    SortCriteria sort_blob_criteria = SORT_DECREASING_MAGNITUDE,
                                    std::ostream* pReportProgress = nullptr, int scale = 6) {
  if (!ctx) {
    DiscardOverlappingBlobs(blob_crds, blob_diameters, blob_scores, min_radial_separation_ratio, max_volume_overlap_large,
                            max_volume_overlap_small, sort_blob_criteria, pReportProgress, scale);
    return;
  }
  hip_detail::FlatBlobs f(blob_crds, blob_diameters, blob_scores);
  int64_t n = (int64_t)blob_crds.size();
  if (pReportProgress) *pReportProgress << "  detecting collisions between " << n << " blobs... ";
  hip_detail::check(visfd_hip_discard_overlapping_blobs_ctx(ctx, f.c.data(), f.d.data(), f.s.data(), &n,
                                                            min_radial_separation_ratio, max_volume_overlap_large,
                                                            max_volume_overlap_small, (int)sort_blob_criteria, scale));
  f.store((size_t)n, blob_crds, blob_diameters, blob_scores);
  if (pReportProgress) *pReportProgress << "done.\n";
}

// ---- FindSpheres and the supervised score thresholds: lib/visfd/visfd_utils.hpp:271-516, feature.hpp:643-697, :988-1180 ----
// The search over (training point, blob) pairs runs on the device (visfd_hip_find_spheres); the progress lines are the
// reference's, text for text -- its table is not allocated here, but its stderr says so and programs compare it.
namespace hip_detail {
inline std::vector<float> flat_crds(const std::vector<std::array<float, 3> >& crds) {
  std::vector<float> c(3 * crds.size());
  for (size_t i = 0; i < crds.size(); i++) { c[3 * i] = crds[i][0]; c[3 * i + 1] = crds[i][1]; c[3 * i + 2] = crds[i][2]; }
  return c;
}
// Which search the supervised wrappers use: the process-wide context, or -- with a null result -- the host walk
// (filter_mrc sets it for small lists, which then need no GPU)
inline bool& supervised_on_host() { static bool on_host = false; return on_host; }
inline visfd_hip_ctx* supervised_context() { return supervised_on_host() ? nullptr : context(); }
inline void report_find_spheres(std::ostream* p) {
  if (p) *p << " -- Attempting to allocate space for one more image.       --\n"
            << " -- (If this crashes your computer, find a computer with   --\n"
            << " --  more RAM and use \"ulimit\", OR use a smaller image.)   --\n";
}
inline void report_sort(std::ostream* p, size_t n_blobs, SortCriteria criteria) {
  if (p && n_blobs > 0 && criteria != DO_NOT_SORT) *p << "-- Sorting blobs according to their scores... done --" << std::endl;
}
// the C ABI's EINVAL for an empty training set carries the reference's exception text: thrown as it is
inline void check_supervised(int rc) {
  if (rc == VISFD_HIP_EINVAL && std::string(visfd_hip_last_error()).compare(0, 20, "Error: Empty list of") == 0)
    throw VisfdErr(visfd_hip_last_error());
  check(rc);
}
// _ChooseThresholdInterval's report, feature_implementation.hpp:240-273
inline void report_thresholds(std::ostream* p, float lower, float upper, const int64_t report[4]) {
  if (!p) return;
  *p << "  threshold lower bound: " << lower << "\n"
     << "  threshold upper bound: " << upper << "\n";
  *p << "  number of false positives: " << report[0] << " (out of " << report[1] << " negatives)\n"
     << "  number of false negatives: " << report[2] << " (out of " << report[3] << " positives)\n"
     << std::endl;
}
}  // namespace hip_detail

// Not in the reference: the wrappers below search on the process-wide context's device; FindSpheresOnHost(true) makes them
// walk the pairs on the host instead (visfd_hip_find_spheres_host: no context is created, no GPU is needed).
inline void FindSpheresOnHost(bool on_host) { hip_detail::supervised_on_host() = on_host; }

template <typename Integer>
inline void FindSpheres(const std::vector<std::array<float, 3> >& crds, std::vector<Integer>& sphere_ids,
                        const std::vector<std::array<float, 3> >& sphere_center_crds,
                        const std::vector<float>& sphere_diameters, std::ostream* pReportProgress = nullptr) {
  if (sphere_diameters.size() != sphere_center_crds.size())
    throw VisfdErr("Error: sphere coordinate and diameter lists differ in length.\n");
  hip_detail::report_find_spheres(pReportProgress);
  const std::vector<float> q = hip_detail::flat_crds(crds), c = hip_detail::flat_crds(sphere_center_crds);
  std::vector<int64_t> ids(crds.size());
  visfd_hip_ctx* ctx = hip_detail::supervised_context();
  hip_detail::check(ctx ? visfd_hip_find_spheres(ctx, q.data(), (int64_t)crds.size(), c.data(), sphere_diameters.data(),
                                                 (int64_t)sphere_diameters.size(), ids.data())
                        : visfd_hip_find_spheres_host(q.data(), (int64_t)crds.size(), c.data(), sphere_diameters.data(),
                                                      (int64_t)sphere_diameters.size(), ids.data()));
  sphere_ids.clear();
  for (size_t i = 0; i < ids.size(); i++) sphere_ids.push_back((Integer)ids[i]);
}

inline float ChooseThreshold1D(const std::vector<float>& training_scores, const std::vector<bool>& training_accepted,
                               bool threshold_is_lower_bound = true) {
  std::vector<unsigned char> acc(training_accepted.begin(), training_accepted.end());
  float thr = 0.0f;
  hip_detail::check(visfd_hip_choose_threshold_1d(training_scores.data(), acc.data(), (int64_t)training_scores.size(),
                                                  threshold_is_lower_bound ? 1 : 0, &thr));
  return thr;
}

// the survivors are APPENDED to the three out_ vectors, as in the reference
inline void FindBlobScores(const std::vector<std::array<float, 3> >& in_training_crds,
                           const std::vector<bool>& in_training_accepted,
                           std::vector<std::array<float, 3> >& out_training_crds, std::vector<bool>& out_training_accepted,
                           std::vector<float>& out_training_scores, const std::vector<std::array<float, 3> >& blob_crds,
                           const std::vector<float>& blob_diameters, const std::vector<float>& blob_scores,
                           SortCriteria sort_blob_criteria = SORT_DECREASING_MAGNITUDE,
                           std::ostream* pReportProgress = nullptr) {
  hip_detail::FlatBlobs f(blob_crds, blob_diameters, blob_scores);
  const std::vector<float> t = hip_detail::flat_crds(in_training_crds);
  std::vector<float> scores(in_training_crds.size());
  std::vector<int64_t> which(in_training_crds.size());
  hip_detail::report_sort(pReportProgress, blob_crds.size(), sort_blob_criteria);
  hip_detail::report_find_spheres(pReportProgress);
  hip_detail::check(visfd_hip_find_blob_scores(hip_detail::supervised_context(), t.data(), (int64_t)in_training_crds.size(),
                                               f.c.data(), f.d.data(), f.s.data(), (int64_t)blob_crds.size(),
                                               (int)sort_blob_criteria, scores.data(), which.data()));
  for (size_t i = 0; i < which.size(); i++)
    if (which[i] != 0) {
      out_training_crds.push_back(in_training_crds[i]);
      out_training_scores.push_back(scores[i]);
      out_training_accepted.push_back(in_training_accepted[i]);
    }
}

inline void ChooseBlobScoreThresholds(const std::vector<std::array<float, 3> >& blob_crds,
                                      const std::vector<float>& blob_diameters, const std::vector<float>& blob_scores,
                                      const std::vector<std::array<float, 3> >& training_set_pos,
                                      const std::vector<std::array<float, 3> >& training_set_neg,
                                      float* pthreshold_lower_bound = nullptr, float* pthreshold_upper_bound = nullptr,
                                      SortCriteria sort_blob_criteria = SORT_DECREASING_MAGNITUDE,
                                      std::ostream* pReportProgress = nullptr) {
  hip_detail::FlatBlobs f(blob_crds, blob_diameters, blob_scores);
  const std::vector<float> p = hip_detail::flat_crds(training_set_pos), n = hip_detail::flat_crds(training_set_neg);
  float lower = 0.0f, upper = 0.0f;
  int64_t report[4] = {0, 0, 0, 0};
  hip_detail::report_sort(pReportProgress, blob_crds.size(), sort_blob_criteria);
  hip_detail::report_find_spheres(pReportProgress);
  hip_detail::check_supervised(visfd_hip_choose_blob_score_thresholds(
      hip_detail::supervised_context(), f.c.data(), f.d.data(), f.s.data(), (int64_t)blob_crds.size(), p.data(),
      (int64_t)training_set_pos.size(), n.data(), (int64_t)training_set_neg.size(), (int)sort_blob_criteria, &lower, &upper,
      report));
  if (pReportProgress) *pReportProgress << "  examining training data to determine optimal thresholds\n";
  if (pthreshold_lower_bound) *pthreshold_lower_bound = lower;
  if (pthreshold_upper_bound) *pthreshold_upper_bound = upper;
  hip_detail::report_thresholds(pReportProgress, lower, upper, report);
}

inline void ChooseBlobScoreThresholdsMulti(const std::vector<std::vector<std::array<float, 3> > >& blob_crds,
                                           const std::vector<std::vector<float> >& blob_diameters,
                                           const std::vector<std::vector<float> >& blob_scores,
                                           const std::vector<std::vector<std::array<float, 3> > >& training_set_pos,
                                           const std::vector<std::vector<std::array<float, 3> > >& training_set_neg,
                                           float* pthreshold_lower_bound = nullptr, float* pthreshold_upper_bound = nullptr,
                                           SortCriteria sort_blob_criteria = SORT_DECREASING_MAGNITUDE,
                                           std::ostream* pReportProgress = nullptr) {
  const size_t n_sets = training_set_pos.size();
  if (training_set_neg.size() != n_sets || blob_crds.size() != n_sets || blob_diameters.size() != n_sets ||
      blob_scores.size() != n_sets)
    throw VisfdErr("Error: the lists of training sets and blob lists differ in length.\n");
  std::vector<float> bc, bd, bs, pc, nc;
  std::vector<int64_t> nb(n_sets), np(n_sets), nn(n_sets);
  for (size_t I = 0; I < n_sets; I++) {
    hip_detail::FlatBlobs f(blob_crds[I], blob_diameters[I], blob_scores[I]);
    const std::vector<float> p = hip_detail::flat_crds(training_set_pos[I]), n = hip_detail::flat_crds(training_set_neg[I]);
    bc.insert(bc.end(), f.c.begin(), f.c.end()); bd.insert(bd.end(), f.d.begin(), f.d.end());
    bs.insert(bs.end(), f.s.begin(), f.s.end());
    pc.insert(pc.end(), p.begin(), p.end()); nc.insert(nc.end(), n.begin(), n.end());
    nb[I] = (int64_t)blob_crds[I].size(); np[I] = (int64_t)training_set_pos[I].size(); nn[I] = (int64_t)training_set_neg[I].size();
    hip_detail::report_sort(pReportProgress, blob_crds[I].size(), sort_blob_criteria);
    hip_detail::report_find_spheres(pReportProgress);
  }
  float lower = 0.0f, upper = 0.0f;
  int64_t report[4] = {0, 0, 0, 0};
  hip_detail::check_supervised(visfd_hip_choose_blob_score_thresholds_multi(
      hip_detail::supervised_context(), (int64_t)n_sets, bc.data(), bd.data(), bs.data(), nb.data(), pc.data(), np.data(),
      nc.data(), nn.data(), (int)sort_blob_criteria, &lower, &upper, report));
  if (pReportProgress) *pReportProgress << "  examining training data to determine optimal thresholds\n";
  if (pthreshold_lower_bound) *pthreshold_lower_bound = lower;
  if (pthreshold_upper_bound) *pthreshold_upper_bound = upper;
  hip_detail::report_thresholds(pReportProgress, lower, upper, report);
}

inline void DiscardBlobsByScoreSupervised(std::vector<std::array<float, 3> >& blob_crds, std::vector<float>& blob_diameters,
                                          std::vector<float>& blob_scores,
                                          const std::vector<std::array<float, 3> >& training_set_pos,
                                          const std::vector<std::array<float, 3> >& training_set_neg,
                                          SortCriteria sort_blob_criteria = SORT_DECREASING_MAGNITUDE,
                                          float* pthreshold_lower_bound = nullptr, float* pthreshold_upper_bound = nullptr,
                                          std::ostream* pReportProgress = nullptr) {
  float lower = 0.0f, upper = 0.0f;
  ChooseBlobScoreThresholds(blob_crds, blob_diameters, blob_scores, training_set_pos, training_set_neg, &lower, &upper,
                            sort_blob_criteria, pReportProgress);
  if (pthreshold_lower_bound) *pthreshold_lower_bound = lower;
  if (pthreshold_upper_bound) *pthreshold_upper_bound = upper;
  if (pReportProgress) *pReportProgress << "  allocating another blob list copy." << std::endl;
  size_t kept = 0;
  for (size_t i = 0; i < blob_crds.size(); i++)
    if (blob_scores[i] >= lower && blob_scores[i] <= upper) {
      blob_crds[kept] = blob_crds[i]; blob_diameters[kept] = blob_diameters[i]; blob_scores[kept] = blob_scores[i];
      kept++;
    }
  blob_crds.resize(kept); blob_diameters.resize(kept); blob_scores.resize(kept);
}

// ---- BlobDogNM / _BlobDogNM: bin/filter_mrc/feature_variants.hpp:393-580 --------------------------------------
// BlobDogD followed by non-max suppression of overlapping blobs (minima best-first by increasing score, maxima by
// decreasing score); the `_` form takes the filter window either as a ratio or as a decay threshold.
inline void BlobDogNM(int const image_size[3], float const* const* const* aaafSource,
                      float const* const* const* aaafMask, const std::vector<float>& blob_diameters,
                      std::vector<std::array<float, 3> >* pva_minima_crds = nullptr,
                      std::vector<std::array<float, 3> >* pva_maxima_crds = nullptr,
                      std::vector<float>* pv_minima_diameters = nullptr,
                      std::vector<float>* pv_maxima_diameters = nullptr,
                      std::vector<float>* pv_minima_scores = nullptr, std::vector<float>* pv_maxima_scores = nullptr,
                      const float aspect_ratio[3] = nullptr, float delta_sigma_over_sigma = 0.02,
                      float truncate_ratio = 2.5, float minima_threshold = 0.5, float maxima_threshold = 0.5,
                      bool use_threshold_ratios = true, float sep_ratio_thresh = 1.0,
                      float nonmax_max_overlap_large = 1.0, float nonmax_max_overlap_small = 1.0,
                      std::ostream* pReportProgress = nullptr, float**** aaaafI = nullptr) {
  std::vector<std::array<float, 3> > minima_crds, maxima_crds;
  std::vector<float> minima_diameters, maxima_diameters, minima_scores, maxima_scores;
  if (!pva_minima_crds) pva_minima_crds = &minima_crds;
  if (!pva_maxima_crds) pva_maxima_crds = &maxima_crds;
  if (!pv_minima_diameters) pv_minima_diameters = &minima_diameters;
  if (!pv_maxima_diameters) pv_maxima_diameters = &maxima_diameters;
  if (!pv_minima_scores) pv_minima_scores = &minima_scores;
  if (!pv_maxima_scores) pv_maxima_scores = &maxima_scores;
  const float default_aspect_ratio[3] = {1.0f, 1.0f, 1.0f};
  BlobDogD(image_size, aaafSource, aaafMask, blob_diameters, pva_minima_crds, pva_maxima_crds, pv_minima_diameters,
           pv_maxima_diameters, pv_minima_scores, pv_maxima_scores, aspect_ratio ? aspect_ratio : default_aspect_ratio,
           delta_sigma_over_sigma, truncate_ratio, minima_threshold, maxima_threshold, use_threshold_ratios,
           pReportProgress, aaaafI);
  const bool discard_overlapping_blobs =
      (sep_ratio_thresh > 0.0f) || (nonmax_max_overlap_small < 1.0f) || (nonmax_max_overlap_large < 1.0f);
  if (!discard_overlapping_blobs) return;
  if (pReportProgress)
    *pReportProgress << "----------- Removing overlapping blobs -----------\n" << std::endl
                     << "--- Discarding overlapping minima blobs ---\n";
  DiscardOverlappingBlobs(*pva_minima_crds, *pv_minima_diameters, *pv_minima_scores, sep_ratio_thresh,
                          nonmax_max_overlap_large, nonmax_max_overlap_small, SORT_INCREASING, pReportProgress);
  if (pReportProgress) *pReportProgress << "done --\n" << "--- Discarding overlapping maxima blobs ---\n";
  DiscardOverlappingBlobs(*pva_maxima_crds, *pv_maxima_diameters, *pv_maxima_scores, sep_ratio_thresh,
                          nonmax_max_overlap_large, nonmax_max_overlap_small, SORT_DECREASING, pReportProgress);
}

inline void _BlobDogNM(int const image_size[3], float const* const* const* aaafSource,
                       float const* const* const* aaafMask, const std::vector<float>& blob_diameters,
                       std::vector<std::array<float, 3> >* pva_minima_crds = nullptr,
                       std::vector<std::array<float, 3> >* pva_maxima_crds = nullptr,
                       std::vector<float>* pv_minima_diameters = nullptr,
                       std::vector<float>* pv_maxima_diameters = nullptr,
                       std::vector<float>* pv_minima_scores = nullptr, std::vector<float>* pv_maxima_scores = nullptr,
                       const float aspect_ratio[3] = nullptr, float delta_sigma_over_sigma = 0.02,
                       float filter_truncate_ratio = 2.5, float filter_truncate_threshold = 0.02,
                       float minima_threshold = 0.0, float maxima_threshold = 0.0, bool use_threshold_ratios = true,
                       float sep_ratio_thresh = 1.0, float nonmax_max_overlap_large = 1.0,
                       float nonmax_max_overlap_small = 1.0, std::ostream* pReportProgress = nullptr,
                       float**** aaaafI = nullptr) {
  if (filter_truncate_ratio <= 0)   // exp(-ratio^2 / 2) = threshold, evaluated in double as the reference does (:543)
    filter_truncate_ratio = (float)std::sqrt(-2 * std::log((double)filter_truncate_threshold));
  BlobDogNM(image_size, aaafSource, aaafMask, blob_diameters, pva_minima_crds, pva_maxima_crds, pv_minima_diameters,
            pv_maxima_diameters, pv_minima_scores, pv_maxima_scores, aspect_ratio, delta_sigma_over_sigma,
            filter_truncate_ratio, minima_threshold, maxima_threshold, use_threshold_ratios, sep_ratio_thresh,
            nonmax_max_overlap_large, nonmax_max_overlap_small, pReportProgress, aaaafI);
}

// ---- LabelConnected: lib/visfd/connect.hpp:47-65, :168-197 ------------------------------------------------
// The form bin/filter_mrc/handlers.cpp:1985-2013 calls: Scalar = float, Label = ptrdiff_t, Coordinate = float,
// directions as array<float,3>*** (contiguous, Alloc3D), tensors as one float* per voxel (nullptr = no storage,
// e.g. CompactMultiChannelImage3D::aaaafI).
typedef enum eRegionSortCriteria { SORT_BY_VALUE, SORT_BY_SIZE } RegionSortCriteria;
typedef enum eDirectionPairType { SAME_DIRECTION, OPPOSITE_DIRECTION, AUTO } DirectionPairType;

namespace hip_detail {
// What the three functions below share: the reference's arguments as the flat arrays of the C ABI, and the call.
inline size_t label_connected_entry(
    bool graph, visfd_hip_ctx* ctx, const int image_size[3], float const* const* const* aaafSaliency, ptrdiff_t*** aaaiDest,
    float const* const* const* aaafMask,
    float threshold_saliency,
    std::array<float, 3> const* const* const* aaaafVector,
    float threshold_vector_saliency,
    float threshold_vector_neighbor, bool consider_dot_product_sign,
    float* const* const* const* aaaafSymmetricTensor,
    float threshold_tensor_saliency,
    float threshold_tensor_neighbor,
    bool tensor_is_positive_definite_near_target, int connectivity, ptrdiff_t label_undefined,
    std::vector<std::array<float, 3> >* pv_cluster_maxima, std::vector<float>* pv_cluster_sizes,
    std::vector<float>* pv_cluster_saliencies, RegionSortCriteria sort_criteria,
    float const* const* const* aaafVoxelWeights, std::array<float, 3>*** aaaafVectorStandardized,
    const std::vector<std::vector<std::array<float, 3> > >* pMustLinkConstraints,
    const std::vector<std::vector<DirectionPairType> >* pMustLinkDirections,
    bool start_from_saliency_maxima, std::ostream* pReportProgress) {
  static_assert(sizeof(ptrdiff_t) == sizeof(int64_t), "labels travel as 64-bit integers");
  hip_detail::require_contiguous(aaafSaliency, image_size);
  hip_detail::require_contiguous(aaafVoxelWeights, image_size);
  // must-link constraints as the flat arrays of the C ABI (connect.hpp:829-1045)
  std::vector<float> ml_crds;
  std::vector<int64_t> ml_sizes;
  std::vector<int> ml_dirs;
  if (pMustLinkConstraints) {
    for (size_t g = 0; g < pMustLinkConstraints->size(); g++) {
      ml_sizes.push_back((int64_t)(*pMustLinkConstraints)[g].size());
      for (size_t k = 0; k < (*pMustLinkConstraints)[g].size(); k++) {
        for (int d = 0; d < 3; d++) ml_crds.push_back((*pMustLinkConstraints)[g][k][d]);
        if (pMustLinkDirections) {
          const DirectionPairType how = (*pMustLinkDirections)[g][k];
          ml_dirs.push_back(how == SAME_DIRECTION ? 0 : (how == OPPOSITE_DIRECTION ? 1 : 2));
        }
      }
    }
  }
  const size_t n = (size_t)image_size[0] * image_size[1] * image_size[2];
  // directions: the standardized output array if one is given (it starts as a copy of the input), else a copy
  std::vector<float> dir_copy;
  float* dir = nullptr;
  if (aaaafVector) {
    const float* in = reinterpret_cast<const float*>(&aaaafVector[0][0][0]);
    if (aaaafVectorStandardized) {
      dir = reinterpret_cast<float*>(&aaaafVectorStandardized[0][0][0]);
      if (dir != in) for (size_t i = 0; i < 3 * n; i++) dir[i] = in[i];
    } else {
      dir_copy.assign(in, in + 3 * n);
      dir = dir_copy.data();
    }
  }
  std::vector<float> ten;
  if (aaaafSymmetricTensor) {
    ten.assign(6 * n, 0.0f);
    size_t v = 0;
    for (int iz = 0; iz < image_size[2]; iz++)
      for (int iy = 0; iy < image_size[1]; iy++)
        for (int ix = 0; ix < image_size[0]; ix++, v++)
          if (aaaafSymmetricTensor[iz][iy][ix])
            for (int c = 0; c < 6; c++) ten[6 * v + c] = aaaafSymmetricTensor[iz][iy][ix][c];
  }
  std::vector<float> cm(pv_cluster_maxima ? 3 * n : 0), cs(pv_cluster_sizes ? n : 0), csal(pv_cluster_saliencies ? n : 0);
  int64_t n_clusters = 0;
  int64_t* const dest = reinterpret_cast<int64_t*>(&aaaiDest[0][0][0]);
  const float* const w = hip_detail::flat(aaafVoxelWeights);
  const float* const mlc = ml_crds.empty() ? nullptr : ml_crds.data();
  const int64_t* const mls = ml_sizes.empty() ? nullptr : ml_sizes.data();
  const int* const mld = ml_dirs.empty() ? nullptr : ml_dirs.data();
  // one argument list, four entries: the flood (seeds on the host or on ctx's device) or the graph form (on ctx's device,
  // or its serial host walk)
#define VISFD_HIP_LC_ARGS                                                                                                   \
  hip_detail::flat(aaafSaliency), dest, hip_detail::flat(aaafMask), image_size[0], image_size[1], image_size[2],            \
      threshold_saliency, dir, threshold_vector_saliency, threshold_vector_neighbor, consider_dot_product_sign ? 1 : 0,     \
      aaaafSymmetricTensor ? ten.data() : nullptr, threshold_tensor_saliency, threshold_tensor_neighbor,                    \
      tensor_is_positive_definite_near_target ? 1 : 0, connectivity, (int64_t)label_undefined,                              \
      sort_criteria == SORT_BY_SIZE ? 1 : 0, aaaafVectorStandardized ? 1 : 0, start_from_saliency_maxima ? 1 : 0,           \
      &n_clusters, cm.empty() ? nullptr : cm.data(), cs.empty() ? nullptr : cs.data(),                                      \
      csal.empty() ? nullptr : csal.data(), (int64_t)n, w, mlc, mls, (int64_t)ml_sizes.size(), mld
  const int rc = graph ? (ctx ? visfd_hip_label_connected_graph(ctx, VISFD_HIP_LC_ARGS)
                              : visfd_hip_label_connected_graph_host(VISFD_HIP_LC_ARGS))
                       : (ctx ? visfd_hip_label_connected_device_seeds(ctx, VISFD_HIP_LC_ARGS)
                              : visfd_hip_label_connected_ex(VISFD_HIP_LC_ARGS));
#undef VISFD_HIP_LC_ARGS
  hip_detail::check(rc);
  if (pReportProgress) *pReportProgress << "Number of clusters found: " << n_clusters << "\n";
  if (pv_cluster_maxima) {
    pv_cluster_maxima->resize((size_t)n_clusters);
    for (int64_t k = 0; k < n_clusters; k++) (*pv_cluster_maxima)[(size_t)k] = {{cm[3 * k], cm[3 * k + 1], cm[3 * k + 2]}};
  }
  if (pv_cluster_sizes) pv_cluster_sizes->assign(cs.begin(), cs.begin() + n_clusters);
  if (pv_cluster_saliencies) pv_cluster_saliencies->assign(csal.begin(), csal.begin() + n_clusters);
  return (size_t)n_clusters;
}
}  // namespace hip_detail

// Not in the reference: LabelConnected with its seed search on a context's device (visfd_hip_label_connected_device_seeds;
// the flood stays on the host, the results are the same bits); a null context is the drop-in below.
inline size_t LabelConnectedDeviceSeeds(
    visfd_hip_ctx* ctx, const int image_size[3], float const* const* const* aaafSaliency, ptrdiff_t*** aaaiDest,
    float const* const* const* aaafMask,
    float threshold_saliency = -std::numeric_limits<float>::infinity(),
    std::array<float, 3> const* const* const* aaaafVector = nullptr,
    float threshold_vector_saliency = -std::numeric_limits<float>::infinity(),
    float threshold_vector_neighbor = -std::numeric_limits<float>::infinity(), bool consider_dot_product_sign = true,
    float* const* const* const* aaaafSymmetricTensor = nullptr,
    float threshold_tensor_saliency = -std::numeric_limits<float>::infinity(),
    float threshold_tensor_neighbor = -std::numeric_limits<float>::infinity(),
    bool tensor_is_positive_definite_near_target = true, int connectivity = 1, ptrdiff_t label_undefined = -1,
    std::vector<std::array<float, 3> >* pv_cluster_maxima = nullptr, std::vector<float>* pv_cluster_sizes = nullptr,
    std::vector<float>* pv_cluster_saliencies = nullptr, RegionSortCriteria sort_criteria = SORT_BY_SIZE,
    float const* const* const* aaafVoxelWeights = nullptr, std::array<float, 3>*** aaaafVectorStandardized = nullptr,
    const std::vector<std::vector<std::array<float, 3> > >* pMustLinkConstraints = nullptr,
    const std::vector<std::vector<DirectionPairType> >* pMustLinkDirections = nullptr,
    bool start_from_saliency_maxima = true, std::ostream* pReportProgress = nullptr) {
  return hip_detail::label_connected_entry(false, ctx, image_size, aaafSaliency, aaaiDest, aaafMask, threshold_saliency, aaaafVector,
                             threshold_vector_saliency, threshold_vector_neighbor, consider_dot_product_sign,
                             aaaafSymmetricTensor, threshold_tensor_saliency, threshold_tensor_neighbor,
                             tensor_is_positive_definite_near_target, connectivity, label_undefined, pv_cluster_maxima,
                             pv_cluster_sizes, pv_cluster_saliencies, sort_criteria, aaafVoxelWeights,
                             aaaafVectorStandardized, pMustLinkConstraints, pMustLinkDirections, start_from_saliency_maxima,
                             pReportProgress);
}

// Not in the reference: LabelConnected as a graph problem (visfd_hip_label_connected_graph), on a context's
// device or, with a null context, by the serial host walk.  Labels, lists and the directions of labelled voxels are the
// drop-in's bits; aaaafVectorStandardized keeps the input's directions at every unlabelled or masked voxel (the drop-in
// turns a halo of them).  visfd_hip_label_connected_graph_last says which path the call took.
inline size_t LabelConnectedGraph(
    visfd_hip_ctx* ctx, const int image_size[3], float const* const* const* aaafSaliency, ptrdiff_t*** aaaiDest,
    float const* const* const* aaafMask,
    float threshold_saliency = -std::numeric_limits<float>::infinity(),
    std::array<float, 3> const* const* const* aaaafVector = nullptr,
    float threshold_vector_saliency = -std::numeric_limits<float>::infinity(),
    float threshold_vector_neighbor = -std::numeric_limits<float>::infinity(), bool consider_dot_product_sign = true,
    float* const* const* const* aaaafSymmetricTensor = nullptr,
    float threshold_tensor_saliency = -std::numeric_limits<float>::infinity(),
    float threshold_tensor_neighbor = -std::numeric_limits<float>::infinity(),
    bool tensor_is_positive_definite_near_target = true, int connectivity = 1, ptrdiff_t label_undefined = -1,
    std::vector<std::array<float, 3> >* pv_cluster_maxima = nullptr, std::vector<float>* pv_cluster_sizes = nullptr,
    std::vector<float>* pv_cluster_saliencies = nullptr, RegionSortCriteria sort_criteria = SORT_BY_SIZE,
    float const* const* const* aaafVoxelWeights = nullptr, std::array<float, 3>*** aaaafVectorStandardized = nullptr,
    const std::vector<std::vector<std::array<float, 3> > >* pMustLinkConstraints = nullptr,
    const std::vector<std::vector<DirectionPairType> >* pMustLinkDirections = nullptr,
    bool start_from_saliency_maxima = true, std::ostream* pReportProgress = nullptr) {
  return hip_detail::label_connected_entry(true, ctx, image_size, aaafSaliency, aaaiDest, aaafMask, threshold_saliency, aaaafVector,
                             threshold_vector_saliency, threshold_vector_neighbor, consider_dot_product_sign,
                             aaaafSymmetricTensor, threshold_tensor_saliency, threshold_tensor_neighbor,
                             tensor_is_positive_definite_near_target, connectivity, label_undefined, pv_cluster_maxima,
                             pv_cluster_sizes, pv_cluster_saliencies, sort_criteria, aaafVoxelWeights,
                             aaaafVectorStandardized, pMustLinkConstraints, pMustLinkDirections, start_from_saliency_maxima,
                             pReportProgress);
}

// the reference's signature: everything on the host, no GPU needed
inline size_t LabelConnected(
    const int image_size[3], float const* const* const* aaafSaliency, ptrdiff_t*** aaaiDest,
    float const* const* const* aaafMask,
    float threshold_saliency = -std::numeric_limits<float>::infinity(),
    std::array<float, 3> const* const* const* aaaafVector = nullptr,
    float threshold_vector_saliency = -std::numeric_limits<float>::infinity(),
    float threshold_vector_neighbor = -std::numeric_limits<float>::infinity(), bool consider_dot_product_sign = true,
    float* const* const* const* aaaafSymmetricTensor = nullptr,
    float threshold_tensor_saliency = -std::numeric_limits<float>::infinity(),
    float threshold_tensor_neighbor = -std::numeric_limits<float>::infinity(),
    bool tensor_is_positive_definite_near_target = true, int connectivity = 1, ptrdiff_t label_undefined = -1,
    std::vector<std::array<float, 3> >* pv_cluster_maxima = nullptr, std::vector<float>* pv_cluster_sizes = nullptr,
    std::vector<float>* pv_cluster_saliencies = nullptr, RegionSortCriteria sort_criteria = SORT_BY_SIZE,
    float const* const* const* aaafVoxelWeights = nullptr, std::array<float, 3>*** aaaafVectorStandardized = nullptr,
    const std::vector<std::vector<std::array<float, 3> > >* pMustLinkConstraints = nullptr,
    const std::vector<std::vector<DirectionPairType> >* pMustLinkDirections = nullptr,
    bool start_from_saliency_maxima = true, std::ostream* pReportProgress = nullptr) {
  return LabelConnectedDeviceSeeds(nullptr, image_size, aaafSaliency, aaaiDest, aaafMask, threshold_saliency, aaaafVector,
                        threshold_vector_saliency, threshold_vector_neighbor, consider_dot_product_sign, aaaafSymmetricTensor,
                        threshold_tensor_saliency, threshold_tensor_neighbor, tensor_is_positive_definite_near_target,
                        connectivity, label_undefined, pv_cluster_maxima, pv_cluster_sizes, pv_cluster_saliencies,
                        sort_criteria, aaafVoxelWeights, aaaafVectorStandardized, pMustLinkConstraints, pMustLinkDirections,
                        start_from_saliency_maxima, pReportProgress);
}

// ---- eigenvalue order: lib/visfd/eigen3_simple.hpp:36-43 ------------------------------------------------
namespace selfadjoint_eigen3 {
typedef enum eEigenOrderType {
  INCREASING_EIVALS = VISFD_HIP_INCREASING_EIVALS,
  DECREASING_EIVALS = VISFD_HIP_DECREASING_EIVALS
} EigenOrderType;

// ---- DiagonalizeFlatSym3: lib/visfd/eigen3_simple.hpp:271-275 (one flat matrix, on the host) -------------
// source = {xx,yy,zz,xy,yz,xz}; dest = {lambda0,lambda1,lambda2, shoemake0..2}.  For whole volumes use the batch
// entry points of the C ABI (visfd_hip_diagonalize_flat_sym3 / visfd_hip_ridge_saliency) instead of a voxel loop.
inline void DiagonalizeFlatSym3(const float* source, float* dest, EigenOrderType eival_order = INCREASING_EIVALS) {
  hip_detail::check(visfd_hip_diagonalize_flat_sym3_host(source, dest, 1, (int)eival_order));
}

// ---- ConvertFlatSym2Evects3: lib/visfd/eigen3_simple.hpp:392-405 -----------------------------------------
inline void ConvertFlatSym2Evects3(const float m[6], float eivals[3], float eivects[3][3],
                                   EigenOrderType eival_order = INCREASING_EIVALS) {
  hip_detail::check(visfd_hip_convert_flat_sym2_evects3_host(m, (int)eival_order, eivals, &eivects[0][0]));
}
}  // namespace selfadjoint_eigen3

// ---- a11 scores of a diagonalised matrix: lib/visfd/feature.hpp:1526-1561, :1570-1581, :1591-1598, :1608-1612
template <typename TensorContainer, typename VectorContainer = const float*>
inline double ScoreHessianPlanar(TensorContainer diagonalizedHessian, VectorContainer = nullptr) {
  const double lambda1 = diagonalizedHessian[0], lambda2 = diagonalizedHessian[1];
  double N = lambda1 * lambda1 - lambda2 * lambda2;
  N *= N;
  return N;
}
template <typename TensorContainer, typename VectorContainer = const float*>
inline double ScoreHessianLinear(TensorContainer diagonalizedHessian, VectorContainer = nullptr) {
  const double lambda1 = diagonalizedHessian[0], lambda2 = diagonalizedHessian[1], lambda3 = diagonalizedHessian[2];
  return lambda1 * lambda2 - lambda3 * lambda3;
}
template <typename TensorContainer>
inline double ScoreTensorPlanar(const TensorContainer diagonalizedMatrix3) {
  const double lambda1 = diagonalizedMatrix3[0], lambda2 = diagonalizedMatrix3[1];
  return lambda1 - lambda2;
}
template <typename TensorContainer>
inline double ScoreTensorLinear(const TensorContainer diagonalizedMatrix3) {
  return ScoreHessianLinear(diagonalizedMatrix3, (const float*)nullptr);   // feature.hpp:1608-1612
}

// ---- CalcHessian: lib/visfd/feature.hpp:1203-1219 --------------------------------------------------------
// Containers as HandleTV instantiates them (bin/filter_mrc/handlers.cpp:1547-1565): gradient as
// array<float,3>***, Hessian as float**** with one pointer per voxel (nullptr where mask == 0).
inline void CalcHessian(int const image_size[3], float const* const* const* aaafSource,
                        std::array<float, 3>*** aaaafGradient, float**** aaaafHessian,
                        float const* const* const* aaafMask, float sigma, float truncate_ratio = 2.5,
                        std::ostream* pReportProgress = nullptr) {
  hip_detail::require_contiguous(aaafSource, image_size);
  hip_detail::require_contiguous(aaafMask, image_size);
  const size_t n = (size_t)image_size[0] * image_size[1] * image_size[2];
  std::vector<float> hess(aaaafHessian ? 6 * n : 0);
  float* grad = aaaafGradient ? &aaaafGradient[0][0][0][0] : nullptr;
  if (pReportProgress) *pReportProgress << "Calculating the Hessian associated with each voxel\n";
  hip_detail::check(visfd_hip_calc_hessian(hip_detail::context(), hip_detail::flat(aaafSource), grad,
                                           aaaafHessian ? hess.data() : nullptr, hip_detail::flat(aaafMask),
                                           image_size[0], image_size[1], image_size[2], sigma, truncate_ratio));
  if (aaaafHessian) {
    size_t v = 0;
    for (int iz = 0; iz < image_size[2]; iz++)
      for (int iy = 0; iy < image_size[1]; iy++)
        for (int ix = 0; ix < image_size[0]; ix++, v++)
          if (float* h = aaaafHessian[iz][iy][ix])
            for (int c = 0; c < 6; c++) h[c] = hess[6 * v + c];
  }
}

// ---- TV3D: lib/visfd/feature.hpp:1631-1724 (dense stick voting only) --------------------------------------
template <typename Scalar, typename Integer, typename VectorContainer, typename TensorContainer>
class TV3D {
  float sigma;
  Integer exponent;
  float cutoff;
 public:
  TV3D() : sigma(0), exponent(4), cutoff(2.5f) {}
  TV3D(Scalar set_sigma, Integer set_exponent, Scalar filter_cutoff_ratio = 2.5)
      : sigma(set_sigma), exponent(set_exponent), cutoff(filter_cutoff_ratio) {}
  void SetExponent(Scalar e) { exponent = (Integer)e; }
  void SetSigma(Scalar s, Scalar filter_cutoff_ratio = 2.5) { sigma = s; cutoff = filter_cutoff_ratio; }

  // aaaafV: array<float,3>*** ; aaaafDest: float**** (pointer per voxel, nullptr = no storage, e.g.
  // CompactMultiChannelImage3D::aaaafI).  The optional steps run on the host after the votes, AS THE REFERENCE
  // EXECUTES THEM (feature.hpp:1784-1901), oddities included:
  //   normalize (the reference's default; filter_mrc passes false, handlers.cpp:1832):
  //     nothing happens without a destination mask (the loops skip every voxel when aaafMaskDest is null, :1793, :1848);
  //     with a source mask every tensor entry is divided by the sum of the vote weights w * mask_src the voxel
  //     received, where that sum is positive; without one the divisor is (Dx*Dy)*Dz, D = GenFilterGauss1D(sigma, h)
  //     summed over the in-image taps (a different kernel than the votes), and because the loop runs over all nine
  //     (di, dj) the off-diagonal entries are divided TWICE (:1854-1858);
  //   diagonalize_dest: DiagonalizeHessianImage with DECREASING_EIVALS -- interior voxels 1..n-2 only (:1380-1386).
  // A null saliency array is refused: the reference then reads saliencies it never initialised (:1748-1756).
  void TVDenseStick(Integer const image_size[3], Scalar const* const* const* aaafSaliency,
                    VectorContainer const* const* const* aaaafV, TensorContainer*** aaaafDest,
                    Scalar const* const* const* aaafMaskSource = nullptr,
                    Scalar const* const* const* aaafMaskDest = nullptr, bool detect_curves_not_surfaces = false,
                    bool normalize = true, bool diagonalize_dest = false, std::ostream* pReportProgress = nullptr) {
    if (!aaafSaliency) throw VisfdErr("visfd_hip: TVDenseStick needs an explicit saliency array");
    int size[3] = {(int)image_size[0], (int)image_size[1], (int)image_size[2]};
    hip_detail::require_contiguous(aaafSaliency, size);
    hip_detail::require_contiguous(aaafMaskSource, size);
    hip_detail::require_contiguous(aaafMaskDest, size);
    const size_t n = (size_t)size[0] * size[1] * size[2];
    std::vector<float> ten(6 * n, 0.0f);
    const float* dir = reinterpret_cast<const float*>(&aaaafV[0][0][0]);
    if (pReportProgress) *pReportProgress << "---- Begin Tensor Voting (dense, stick) on the GPU ----" << std::endl;
    hip_detail::check(visfd_hip_tv_dense_stick(hip_detail::context(), hip_detail::flat(aaafSaliency), dir,
                                               ten.data(), hip_detail::flat(aaafMaskSource),
                                               hip_detail::flat(aaafMaskDest), size[0], size[1], size[2], sigma,
                                               (int)exponent, cutoff, detect_curves_not_surfaces ? 1 : 0));
    const float* mdst = hip_detail::flat(aaafMaskDest);
    if (normalize && mdst) {
      if (pReportProgress) *pReportProgress << "  Normalizing the result of tensor voting...";
      if (aaafMaskSource) {
        std::vector<float> den(n, 0.0f);
        hip_detail::check(visfd_hip_tv_weight_sum(hip_detail::context(), hip_detail::flat(aaafSaliency), den.data(),
                                                  hip_detail::flat(aaafMaskSource), mdst, size[0], size[1], size[2],
                                                  sigma, cutoff));
        for (size_t v = 0; v < n; v++)
          if (mdst[v] != 0.0f && den[v] > 0.0f)
            for (int c = 0; c < 6; c++) ten[6 * v + c] /= den[v];
      } else {
        int h = 0;
        hip_detail::check(visfd_hip_tv_tables(sigma, cutoff, &h, nullptr, nullptr));
        std::vector<float> taps(2 * (size_t)h + 1), D[3];
        hip_detail::check(visfd_hip_gauss_taps(sigma, h, taps.data()));
        for (int d = 0; d < 3; d++) {          // Filter1D::Apply on a line of ones (filter1d.hpp:47-104)
          D[d].resize((size_t)size[d]);
          for (int i = 0; i < size[d]; i++) {
            float a = 0.0f;
            for (int j = -h; j <= h; j++)
              if (i - j >= 0 && i - j < size[d]) a += taps[(size_t)(j + h)] * 1.0f;
            D[d][(size_t)i] = a;
          }
        }
        size_t v = 0;
        for (int iz = 0; iz < size[2]; iz++)
          for (int iy = 0; iy < size[1]; iy++)
            for (int ix = 0; ix < size[0]; ix++, v++) {
              if (mdst[v] == 0.0f) continue;
              const float denominator = (D[0][(size_t)ix] * D[1][(size_t)iy]) * D[2][(size_t)iz];
              float* T = &ten[6 * v];
              for (int c = 0; c < 3; c++) T[c] /= denominator;                            // (0,0), (1,1), (2,2)
              for (int c = 3; c < 6; c++) { T[c] /= denominator; T[c] /= denominator; }   // (di,dj) and (dj,di)
            }
      }
      if (pReportProgress) *pReportProgress << "done." << std::endl;
    }
    if (diagonalize_dest) {
      if (pReportProgress) *pReportProgress << "---- Diagonalizing Tensor Voting results ----" << std::endl;
      for (int iz = 1; iz < size[2] - 1; iz++)
        for (int iy = 1; iy < size[1] - 1; iy++)
          for (int ix = 1; ix < size[0] - 1; ix++) {
            const size_t v = ((size_t)iz * size[1] + iy) * size[0] + ix;
            if (mdst && mdst[v] == 0.0f) continue;
            float d6[6];
            hip_detail::check(visfd_hip_diagonalize_flat_sym3_host(&ten[6 * v], d6, 1, VISFD_HIP_DECREASING_EIVALS));
            for (int c = 0; c < 6; c++) ten[6 * v + c] = d6[c];
          }
    }
    size_t v = 0;
    for (int iz = 0; iz < size[2]; iz++)
      for (int iy = 0; iy < size[1]; iy++)
        for (int ix = 0; ix < size[0]; ix++, v++)
          if (aaaafDest[iz][iy][ix] && !(mdst && mdst[v] == 0.0f))
            for (int c = 0; c < 6; c++) aaaafDest[iz][iy][ix][c] = ten[6 * v + c];
  }
};

}  // namespace visfd

#endif  // VISFD_HIP_HPP
