// intensity.hpp -- the scalar intensity maps of filter_mrc's tail, for the host and the device: the functions of
// lib/threshold/threshold.hpp with Number = float, the step, rescale and invert maps of HandleThresholds
// (handlers.cpp:1003-1081) and MrcSimple::Invert / Rescale01 (mrc_simple.cpp:427-481), and `apply`, one voxel through the
// stages of a visfd_hip_intensity in the reference's order (include/visfd_hip.h states them).
//
// Every operation is one IEEE float operation, written as its own statement where the reference's expression has more
// than one: built with -ffp-contract=off (visfd_amd/build.py) the bits are the reference's on either side.  The one
// exception is gauss(): its double exp comes from the platform's library.
#pragma once

#include <cmath>
#include <cstdint>

#include "../../include/visfd_hip.h"

#if defined(__HIPCC__)
#define VH_HD __host__ __device__
#else
#define VH_HD
#endif

namespace vh_intensity {

// IsBetween, threshold.hpp:9-12: [a, b) for a < b, (b, a] for b < a
VH_HD inline bool is_between(float x, float a, float b) { return ((a <= x) && (x < b)) || ((b < x) && (x <= a)); }

// the ramp of Threshold2 before it is stretched to [out_a, out_b]
VH_HD inline float ramp(float I, float a, float b) {
  if (is_between(I, a, b)) {
    const float num = I - a, den = b - a;
    return num / den;
  }
  const float u = I - a, w = b - a;
  const float prod = u * w;
  return prod > 0.0f ? 1.0f : 0.0f;
}

VH_HD inline float stretch(float g, float out_a, float out_b) {
  const float span = out_b - out_a;
  const float scaled = g * span;
  return out_a + scaled;
}

VH_HD inline float step(float I, float t, float out_a, float out_b) { return I > t ? out_b : out_a; }

VH_HD inline float threshold2(float I, float a, float b, float out_a = 0.0f, float out_b = 1.0f) {
  return stretch(ramp(I, a, b), out_a, out_b);
}

// Threshold4, threshold.hpp:117-169.  Every inner Threshold2 has the default outputs 0 and 1, so its result is
// 0 + g * 1; with b == c == d that unstretched g is returned as it is.
VH_HD inline float threshold4(float I, float a, float b, float c, float d, float out_a = 0.0f, float out_b = 1.0f) {
  float g = threshold2(I, a, b);
  if (b == c && b == d) return g;
  if (is_between(I, a, b)) g = threshold2(I, a, b);
  else if (is_between(I, c, d)) g = threshold2(I, c, d);
  else if (b <= c) g = is_between(I, b, c) ? 1.0f : 0.0f;
  else if (d <= a) g = is_between(I, d, a) ? 0.0f : 1.0f;
  // (else: thresholds in no order; the reference asserts, g stays the first ramp's)
  return stretch(g, out_a, out_b);
}

// SelectIntensityRange, threshold.hpp:206-229: 1 inside [a, b) (a < b) or outside (b, a] (otherwise); the reference takes
// two output values and returns g itself
VH_HD inline float select_range(float I, float a, float b) {
  if (a < b) return is_between(I, a, b) ? 1.0f : 0.0f;
  return is_between(I, b, a) ? 0.0f : 1.0f;
}

// SelectIntensityRangeGauss, threshold.hpp:248-258: the quotient in float, the exponent and the blend in double
VH_HD inline float gauss(float I, float x0, float sigma, float out_a = 0.0f, float out_b = 1.0f) {
  const float dx = I - x0;
  const float xr = dx / sigma;
  const double h = -0.5 * (double)xr;
  const double arg = h * (double)xr;
  const float span = out_b - out_a;
  const double bump = (double)span * exp(arg);
  return (float)((double)out_a + bump);
}

VH_HD inline float rescale(float v, float factor, float offset) {   // handlers.cpp:1041-1042
  const float m = v * factor;
  return m + offset;
}

VH_HD inline float invert(float v, double ave) {   // mrc_simple.cpp:470
  const double twice = 2.0 * ave;
  return (float)(twice - (double)v);
}

VH_HD inline float rescale01(float v, float out_a, float out_b, float dmin, float dmax) {   // mrc_simple.cpp:438-439
  const float span = out_b - out_a, off = v - dmin;
  const float num = span * off;
  const float den = dmax - dmin;
  const float q = num / den;
  return out_a + q;
}

VH_HD inline bool reads_input(int map) { return map >= VISFD_HIP_MAP_STEP && map <= VISFD_HIP_MAP_GAUSS; }
// whether the stages need what `out` holds before the call
VH_HD inline bool reads_output(const visfd_hip_intensity& p) { return !reads_input(p.map); }

// one voxel: vin = in[i] (looked at by the threshold family only), vout = out[i] (looked at by the rest), in_mask:
// there is no mask or mask[i] != 0
VH_HD inline float apply(const visfd_hip_intensity& p, float vin, float vout, bool in_mask) {
  float v = vout;
  if (p.invert && in_mask) v = invert(v, p.ave);
  switch (p.map) {
    case VISFD_HIP_MAP_STEP: v = step(vin, p.t[0], p.out_a, p.out_b); break;
    case VISFD_HIP_MAP_THRESH2: v = threshold2(vin, p.t[0], p.t[1], p.out_a, p.out_b); break;
    case VISFD_HIP_MAP_THRESH4: v = threshold4(vin, p.t[0], p.t[1], p.t[2], p.t[3], p.out_a, p.out_b); break;
    case VISFD_HIP_MAP_RANGE: v = select_range(vin, p.t[0], p.t[1]); break;
    case VISFD_HIP_MAP_GAUSS: v = gauss(vin, p.t[0], p.t[1], p.out_a, p.out_b); break;
    case VISFD_HIP_MAP_RESCALE: v = rescale(v, p.t[0], p.t[1]); break;
    default: break;
  }
  if (p.mask_fill && !in_mask) v = p.masked_value;
  if (p.rescale01) v = rescale01(v, p.rescale_a, p.rescale_b, p.dmin, p.dmax);
  return v;
}

}  // namespace vh_intensity
