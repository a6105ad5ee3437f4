// csrc/exact_div.hpp on the host, for tests/test_exact_div.py: exact_div(a, d, RN(1 / d)) must have the bits of a / d wherever
// the guard lets a numerator through, and the guard must turn away what the sequence cannot take.  Compiled with
// -ffp-contract=off, like every kernel that includes the header.  Prints "checked N quotients" and exits 0, or prints the
// first mismatches and exits 1.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <initializer_list>
#include <limits>

#include "exact_div.hpp"

static uint32_t bits(float x) { uint32_t u; std::memcpy(&u, &x, 4); return u; }
static float from_bits(uint32_t u) { float x; std::memcpy(&x, &u, 4); return x; }

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint32_t rnd() {   // xorshift64*
  rng_state ^= rng_state >> 12; rng_state ^= rng_state << 25; rng_state ^= rng_state >> 27;
  return (uint32_t)((rng_state * 0x2545F4914F6CDD1Dull) >> 32);
}
// a float of either sign, its exponent uniform over the guard's range [2^-100, 2^100), its fraction random
static float random_numerator() {
  const uint32_t r = rnd();
  const uint32_t e = 127 - 100 + rnd() % 200;
  return from_bits((r & 0x80000000u) | (e << 23) | (r & 0x007fffffu));
}

static long checked = 0, bad = 0;
static volatile float sink_d;   // the quotient and the reciprocal are formed at run time, by the division instruction

// one numerator against one divisor; `pass` is what the guard must say
static void check(float a, float d, bool pass) {
  const float one[1] = {a};
  const bool ok = vh::exact_div_in_range<1>(one);
  if (ok != pass) {
    if (bad++ < 10) std::printf("guard: a=%a (%08x) passes=%d, expected %d\n", a, bits(a), (int)ok, (int)pass);
    return;
  }
  if (!ok) return;
  sink_d = d;
  const float dd = sink_d;
  const float y = 1.0f / dd;
  const float want = a / dd;
  const float got = vh::exact_div(a, dd, y);
  checked++;
  if (bits(got) != bits(want) && bad++ < 10)
    std::printf("a=%a d=%a: exact_div %a (%08x), a / d %a (%08x)\n", a, dd, got, bits(got), want, bits(want));
}

static void edges(float d) {
  const float lo = vh::EXACT_DIV_LO, hi = vh::EXACT_DIV_HI;
  for (float sgn : {1.0f, -1.0f}) {
    check(sgn * lo, d, true);                                   // the lower bound is inside
    check(sgn * std::nextafterf(lo, 1.0f), d, true);
    check(sgn * std::nextafterf(lo, 0.0f), d, false);           // just below it
    check(sgn * std::nextafterf(hi, 0.0f), d, true);            // just below the upper bound
    check(sgn * hi, d, false);                                  // the upper bound is outside
    check(sgn * std::nextafterf(hi, INFINITY), d, false);
    check(sgn * 0.0f, d, false);
    check(sgn * std::numeric_limits<float>::denorm_min(), d, false);
    check(sgn * from_bits(0x007fffffu), d, false);              // the largest denormal
    check(sgn * std::numeric_limits<float>::min(), d, false);   // the smallest normal: a number, but below the guard
    check(sgn * std::numeric_limits<float>::max(), d, false);
    check(sgn * INFINITY, d, false);
    check(sgn * std::numeric_limits<float>::quiet_NaN(), d, false);
  }
}

int main() {
  if (!vh::exact_div_divisor_ok(1.0f) || !vh::exact_div_divisor_ok(0.5f) || !vh::exact_div_divisor_ok(2.0f) ||
      vh::exact_div_divisor_ok(0.0f) || vh::exact_div_divisor_ok(-1.0f) || vh::exact_div_divisor_ok(2.5f) ||
      vh::exact_div_divisor_ok(0.49f) || vh::exact_div_divisor_ok(std::numeric_limits<float>::quiet_NaN()) ||
      vh::exact_div_divisor_ok(INFINITY)) {
    std::printf("exact_div_divisor_ok\n");
    return 1;
  }
  // every divisor within 300 ulps of 1.0 on either side (the sums of normalised taps lie within a few ulps of 1)
  const uint32_t one = bits(1.0f);
  for (int k = -300; k <= 300; k++) {
    const float d = from_bits(one + k);   // (below 1.0 an ulp is half as wide: the bit pattern steps all the same)
    edges(d);
    for (int i = 0; i < 5000; i++) check(random_numerator(), d, true);
  }
  // divisors far from 1, the ends of what exact_div_divisor_ok admits among them
  const float far[] = {0.5f, from_bits(bits(0.5f) + 1), 0.75f, 0.9f, 1.1f, 4.0f / 3.0f, 1.5f, from_bits(bits(2.0f) - 1), 2.0f};
  for (float d : far) {
    edges(d);
    for (int i = 0; i < 200000; i++) check(random_numerator(), d, true);
  }
  // random divisors over [0.5, 2)
  for (int i = 0; i < 1500000; i++) check(random_numerator(), from_bits(bits(0.5f) + rnd() % (2u << 23)), true);
  // several numerators at once: one of them outside the range turns all of them away, a NaN on its own as well; beside
  // in-range numbers a NaN is not seen (fmaxf / fminf), and both routes then give a NaN for it
  const float nan = std::numeric_limits<float>::quiet_NaN();
  const float in4[4] = {1.0f, -3.5f, 0x1p-100f, 0x1.fffffep99f}, zero4[4] = {1.0f, 0.0f, 2.0f, 3.0f},
              big4[4] = {1.0f, 2.0f, 3.0f, -0x1p100f}, inf4[4] = {INFINITY, 2.0f, 3.0f, 4.0f}, nan4[4] = {nan, nan, nan, nan},
              mixed4[4] = {1.0f, nan, 2.0f, 3.0f};
  if (!vh::exact_div_in_range<4>(in4) || vh::exact_div_in_range<4>(zero4) || vh::exact_div_in_range<4>(big4) ||
      vh::exact_div_in_range<4>(inf4) || vh::exact_div_in_range<4>(nan4)) {
    std::printf("exact_div_in_range<4>\n");
    return 1;
  }
  if (vh::exact_div_in_range<4>(mixed4)) {
    sink_d = from_bits(one + 3);
    const float d = sink_d, q = vh::exact_div(nan, d, 1.0f / d);
    if (q == q) { std::printf("a NaN numerator gave %a\n", q); return 1; }
  }
  std::printf("checked %ld quotients\n", checked);
  if (bad) std::printf("%ld mismatches\n", bad);
  return bad ? 1 : 0;
}
