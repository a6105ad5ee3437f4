// exact_div.hpp -- the correctly rounded float quotient a / d from a KNOWN reciprocal of d, for kernels that divide many
// numerators by a divisor that is constant per lane (the normaliser (Dx*Dy)*Dz of a Gaussian away from the faces:
// csrc/gauss_fused.hip, csrc/gauss_pair.hip).  Plain C++ as well as HIP: tests/test_exact_div.py compiles it with g++.
//
// With y = RN(1 / d), the correctly rounded reciprocal (one IEEE division, done once), two Newton corrections with exact FMA
// residuals give the quotient (Markstein): q0 = RN(a y); q1 = RN(q0 + (a - d q0) y) is a faithful quotient; q2 = RN(q1 +
// (a - d q1) y) is the correctly rounded one, RN(a / d) bit for bit.  Five instructions against the dozen of the full-range
// division.  The residuals are exact only while nothing under- or overflows, hence the range guard on |a|; the divisor is
// meant to be near 1 (the callers use it for sums of normalised taps; exact_div_divisor_ok is the host-side check).  Whatever
// the guard turns away -- zeros, denormals, infinities, NaN, extreme magnitudes -- takes the ordinary division.
#pragma once

#if defined(__HIPCC__)
#define VH_EXACT_DIV_FN __host__ __device__ __forceinline__
#else
#define VH_EXACT_DIV_FN inline
#endif

namespace vh {

constexpr float EXACT_DIV_HI = 0x1p100f;    // |a| below this and
constexpr float EXACT_DIV_LO = 0x1p-100f;   // not below this

// true when EVERY one of the N numerators may take exact_div.  (The extrema go through fmaxf / fminf, which drop a NaN next to
// a number: a NaN among in-range numerators passes, and both paths then give a NaN for it.  A NaN on its own does not pass.)
template <int N>
VH_EXACT_DIV_FN bool exact_div_in_range(const float (&a)[N]) {
  float hi = __builtin_fabsf(a[0]), lo = hi;
#pragma unroll
  for (int k = 1; k < N; k++) {
    hi = __builtin_fmaxf(hi, __builtin_fabsf(a[k]));
    lo = __builtin_fminf(lo, __builtin_fabsf(a[k]));
  }
  return (hi < EXACT_DIV_HI) && (lo >= EXACT_DIV_LO);
}

// RN(a / d) for a inside the guard, y = RN(1 / d)
VH_EXACT_DIV_FN float exact_div(float a, float d, float y) {
  const float q0 = a * y;
  const float r0 = __builtin_fmaf(-d, q0, a);
  const float q1 = __builtin_fmaf(r0, y, q0);
  const float r1 = __builtin_fmaf(-d, q1, a);
  return __builtin_fmaf(r1, y, q1);
}

// the divisors a caller may prepare a reciprocal for: normal numbers within a factor of two of 1
inline bool exact_div_divisor_ok(float d) { return d >= 0.5f && d <= 2.0f; }

}  // namespace vh
