// host_math.cpp -- the small host-side arithmetic of the hot path: filter taps and the
// tensor-voting lookup tables.  These are O(filter width) computations the reference also does
// on the CPU; their float/long-double evaluation order is part of the
// parity contract, so this file must be built without FMA contraction or fast-math.
#include <algorithm>
#include <cmath>
#include <limits>
#include <vector>

#include "common.hpp"

namespace vh {

// Discrete-Gaussian taps: reference lib/visfd/filter1d.hpp:409-460.
//   sigma<=10 and |i|<=20 : exp(-s^2) * I_|i|(s^2)  (modified Bessel function, long double)
//   otherwise             : exp(-i^2/(2 s^2)) / sqrt(2 pi s^2)
//   sigma==0              : Kronecker delta
// Each tap is rounded to float before the long-double normalising sum is formed.
void host_gauss_taps(float sigma, int h, float* t) {
  long double norm = 0.0L;
  for (int i = -h; i <= h; i++) {
    float v;
    if (sigma == 0.0f) {
      v = (i == 0) ? 1.0f : 0.0f;
    } else {
      const long double s = sigma;
      const long double x = i;
      const long double ax = std::abs(x);
      if (s <= 10.0 && ax <= 20.0)
        v = (float)(std::exp(-s * s) * std::cyl_bessel_i(ax, s * s));
      else
        v = (float)(std::exp(-(x * x) / (2.0 * s * s)) / std::sqrt(2 * s * s * M_PI));
    }
    t[i + h] = v;
    norm += v;
  }
  for (int k = 0; k < 2 * h + 1; k++) t[k] = (float)(t[k] / norm);
}

// The separable filter's boundary normaliser: the axis filter applied to a line of n ones with
// zero extension (reference lib/visfd/filter3d.hpp:1004-1012 via filter1d.hpp:47-104).
void host_conv_ones(i64 n, const float* t, int h, float* out) {
  for (i64 i = 0; i < n; i++) {
    float acc = 0.0f;
    for (int j = -h; j <= h; j++) {
      i64 k = i - j;
      if (k < 0 || k >= n) continue;
      acc += t[j + h] * 1.0f;
    }
    out[i] = acc;
  }
}

// Half-width of the isotropic Gaussian of the ridge and background stages: reference lib/visfd/feature.hpp:1223, the floor
// of the float product with no lower bound of 1.
int host_iso_halfwidth(float sigma, float ratio) { return (int)std::floor(sigma * ratio); }

// Tensor-voting window: reference lib/visfd/feature.hpp:1669-1675.
int host_tv_halfwidth(float sigma, float cutoff) { return (int)std::floor(sigma * cutoff); }

// The entry loop of GenFilterGenGauss3D(width, m, truncate_halfwidth) (reference lib/visfd/filter3d.hpp:546-583) in float,
// with the reference's types: the cut is the smallest face value exp(-pow(h_d / width_d, m)) over the axes with
// width_d > 0 (starting from 1); entries exp(-pow(r, m)), r = sqrt(x^2 + y^2 + z^2), x = ix / width_x (not divided when
// width == 0 and ix == 0), the centre entry 1; entries below the cut zeroed.  Writes the entries before their division
// (z outermost, then y, then x) where `out` is given and returns their float sum accumulated in that order.
// SQUARE: the exponent is the literal 2 of TV3D::Resize (feature.hpp:2419-2428), which compilers evaluate as a product;
// a run-time exponent of 2 goes through powf instead, and the two differ in the last bit for some r.  The vote table is
// pinned to the first (tests/test_gpu_parity.py), the central value LocalFluctuations uses to the second
// (tests/golden/fluctuations.npz).
template <bool SQUARE>
static float gengauss3d_entries(const float width[3], float m_exp, const int hw[3], float* out) {
  auto power = [m_exp](float v) { return SQUARE ? std::pow(v, 2.0f) : std::pow(v, m_exp); };
  float cut = 1.0f;
  for (int d = 0; d < 3; d++) {
    const float e = (width[d] > 0) ? std::exp(-power(hw[d] / width[d])) : 1.0f;
    if (e < cut) cut = e;
  }
  float total = 0;
  size_t k = 0;
  for (int iz = -hw[2]; iz <= hw[2]; iz++)
    for (int iy = -hw[1]; iy <= hw[1]; iy++)
      for (int ix = -hw[0]; ix <= hw[0]; ix++, k++) {
        const float x = (width[0] == 0.0f && ix == 0) ? 0.0f : ix / width[0];
        const float y = (width[1] == 0.0f && iy == 0) ? 0.0f : iy / width[1];
        const float z = (width[2] == 0.0f && iz == 0) ? 0.0f : iz / width[2];
        const float r = std::sqrt(x * x + y * y + z * z);
        float v = (r > 0) ? std::exp(-power(r)) : 1.0f;
        if (std::fabs(v) < cut) v = 0.0f;
        if (out) out[k] = v;
        total += v;
      }
  return total;
}

// GenFilterGenGauss3D(width, m, truncate_halfwidth) (filter3d.hpp:546-601): the entries above divided by their sum;
// A = the centre entry.  table_out has (2 hx + 1)(2 hy + 1)(2 hz + 1) entries, x fastest.
template <bool SQUARE>
static void gengauss3d_table(const float width[3], float m_exp, const int hw[3], float* table_out, float* A_out) {
  const float total = gengauss3d_entries<SQUARE>(width, m_exp, hw, table_out);
  const size_t sx = 2 * (size_t)hw[0] + 1, sy = 2 * (size_t)hw[1] + 1, sz = 2 * (size_t)hw[2] + 1;
  for (size_t k = 0; k < sx * sy * sz; k++) table_out[k] /= total;
  if (A_out) *A_out = table_out[((size_t)hw[2] * sy + hw[1]) * sx + hw[0]];
}
void host_gengauss3d_table(const float width[3], float m_exp, const int hw[3], float* table_out, float* A_out) {
  gengauss3d_table<false>(width, m_exp, hw, table_out, A_out);
}

// Window of the generalised Gaussians: floor(width_d * ratio); a negative ratio is first replaced by
// pow(-log(threshold), 1.0 / m): float log, double pow, stored to float (bin/filter_mrc/filter3d_variants.hpp:99-103,
// lib/visfd/filter3d.hpp:631-633).
void host_gengauss3d_halfwidths(const float width[3], float m_exp, float ratio, float threshold, int hw[3]) {
  if (ratio < 0.0f) ratio = (float)std::pow((double)(-std::log(threshold)), 1.0 / (double)m_exp);
  for (int d = 0; d < 3; d++) hw[d] = (int)std::floor(width[d] * ratio);
}

// GenFilterDogg3D(width_a, width_b, m, n, ratio, threshold) (filter3d_variants.hpp:284-345, :441-482): each generalised
// Gaussian with its own half-widths (its own ratio when that comes from the threshold), the window the per-axis maximum,
// every entry 0 + A_entry - B_entry with either term left out outside that filter's own window.  hw receives the window;
// the first min(n, cap) entries are written and n is returned.  A, B: the two centre values.
i64 host_dogg3d_table(const float width_a[3], const float width_b[3], float m_exp, float n_exp, float ratio,
                      float threshold, int hw[3], float* table_out, i64 cap, float* A_out, float* B_out) {
  int ha[3], hb[3];
  host_gengauss3d_halfwidths(width_a, m_exp, ratio, threshold, ha);
  host_gengauss3d_halfwidths(width_b, n_exp, ratio, threshold, hb);
  for (int d = 0; d < 3; d++) {
    if (ha[d] < 0 || hb[d] < 0) {   // no such window: the caller refuses it
      hw[0] = hw[1] = hw[2] = -1;
      return 0;
    }
    hw[d] = std::max(ha[d], hb[d]);
  }
  const i64 sx = 2 * (i64)hw[0] + 1, sy = 2 * (i64)hw[1] + 1, sz = 2 * (i64)hw[2] + 1;
  const i64 n = sx * sy * sz;
  if (cap <= 0 && !A_out && !B_out) return n;
  auto size_of = [](const int h[3]) { return (size_t)(2 * h[0] + 1) * (2 * h[1] + 1) * (2 * h[2] + 1); };
  std::vector<float> fa(size_of(ha)), fb(size_of(hb));
  float A = 0, B = 0;
  host_gengauss3d_table(width_a, m_exp, ha, fa.data(), &A);
  host_gengauss3d_table(width_b, n_exp, hb, fb.data(), &B);
  if (A_out) *A_out = A;
  if (B_out) *B_out = B;
  auto at = [](const std::vector<float>& f, const int h[3], int ix, int iy, int iz, float* v) {
    if (ix < -h[0] || ix > h[0] || iy < -h[1] || iy > h[1] || iz < -h[2] || iz > h[2]) return false;
    *v = f[((size_t)(iz + h[2]) * (2 * h[1] + 1) + (iy + h[1])) * (2 * h[0] + 1) + (ix + h[0])];
    return true;
  };
  i64 k = 0;
  for (int iz = -hw[2]; iz <= hw[2]; iz++)
    for (int iy = -hw[1]; iy <= hw[1]; iy++)
      for (int ix = -hw[0]; ix <= hw[0]; ix++, k++) {
        if (k >= cap) continue;
        float v = 0.0f, t;
        if (at(fa, ha, ix, iy, iz, &t)) v += t;
        if (at(fb, hb, ix, iy, iz, &t)) v -= t;
        table_out[k] = v;
      }
  return n;
}

// Radial weight exp(-(r/sigma)^2) with spherical support, normalised to unit sum: GenFilterGenGauss3D with m_exp = 2 as
// TV3D::Resize calls it (feature.hpp:2419-2428), and the unit displacement vectors (feature.hpp:2468-2482).
void host_tv_tables(float sigma, int h, float* w, float* rhat) {
  const float width[3] = {sigma, sigma, sigma};
  const int hw[3] = {h, h, h};
  gengauss3d_table<true>(width, 2.0f, hw, w, nullptr);
  if (!rhat) return;
  size_t k = 0;
  for (int iz = -h; iz <= h; iz++)
    for (int iy = -h; iy <= h; iy++)
      for (int ix = -h; ix <= h; ix++, k++) {
        float len = (float)std::sqrt((double)(ix * ix + iy * iy + iz * iz));
        if (len == 0) len = 1.0f;
        rhat[3 * k + 0] = ix / len;
        rhat[3 * k + 1] = iy / len;
        rhat[3 * k + 2] = iz / len;
      }
}

// Central value A of GenFilterGenGauss3D(width, m, ratio) (filter3d.hpp:609-638): window half-widths floor(width*ratio);
// the centre entry is 1 before the division by the sum.  LocalFluctuations multiplies its variance by this number
// (filter3d.hpp:1725,1836).
float host_gengauss3d_peak(const float width[3], float m_exp, float ratio) {
  int hw[3];
  for (int d = 0; d < 3; d++) hw[d] = (int)std::floor(width[d] * ratio);
  return 1.0f / gengauss3d_entries<false>(width, m_exp, hw, nullptr);
}

// Structuring element of DilateSphere / ErodeSphere (reference lib/visfd/morphology.hpp:241-420): entries
// (dx, dy, dz, b) with dz outermost, then dy, then dx, each over [-Ri, Ri], Ri = ceil(max(radius, radius_max)) in float.
// Three rules, tested in this order, with the reference's types (integer squares, double sqrt stored to float, float b):
//   bmax == 0                flat ball: r <= radius, b = +0
//   radius_max > radius      linear rim: b = -(r - radius) / (radius_max - radius) * bmax for radius < r <= radius_max
//   otherwise                corner rule on the 8 corners (d +- 0.5): in when r_max < radius (b = +0), out when
//                            r_min > radius, else b = -(r_max - radius) / (r_max - r_min) * bmax (may be -0.0f)
// Writes the first min(n, cap) entries (dxyz: 3 ints per entry) and returns the count n.
i64 host_sphere_structure(float radius, float radius_max, float bmax, int* dxyz, float* b, i64 cap) {
  const int Ri = (int)std::ceil(std::max(radius, radius_max));
  i64 n = 0;
  for (int iz = -Ri; iz <= Ri; iz++)
    for (int iy = -Ri; iy <= Ri; iy++)
      for (int ix = -Ri; ix <= Ri; ix++) {
        bool add = false;
        float bb = 0.0f;
        if (bmax == 0.0f) {
          const float r = (float)std::sqrt((double)(ix * ix + iy * iy + iz * iz));
          add = r <= radius;
        } else if (radius_max > radius) {
          const float r = (float)std::sqrt((double)(ix * ix + iy * iy + iz * iz));
          if (r <= radius) {
            add = true;
          } else if (r <= radius_max) {
            add = true;
            bb = -(r - radius) / (radius_max - radius);
            bb *= bmax;
          }
        } else {
          float r_max = -std::numeric_limits<float>::infinity();
          float r_min = std::numeric_limits<float>::infinity();
          for (int jz = 0; jz <= 1; jz++)
            for (int jy = 0; jy <= 1; jy++)
              for (int jx = 0; jx <= 1; jx++) {
                const double cx = ix + jx - 0.5, cy = iy + jy - 0.5, cz = iz + jz - 0.5;
                const float r = (float)std::sqrt(cx * cx + cy * cy + cz * cz);
                if (r < r_min) r_min = r;
                if (r > r_max) r_max = r;
              }
          if (r_max < radius) {
            add = true;
          } else if (r_min > radius) {
            add = false;
          } else {
            add = true;
            bb = -(r_max - radius) / (r_max - r_min);
            bb *= bmax;
          }
        }
        if (!add) continue;
        if (n < cap) {
          dxyz[3 * n + 0] = ix;
          dxyz[3 * n + 1] = iy;
          dxyz[3 * n + 2] = iz;
          b[n] = bb;
        }
        n++;
      }
  return n;
}

}  // namespace vh
