// precision_check.cpp -- the host-checkable part of the float32 boundary (climt_amd/csrc/rrtmg_precision.h: the element
// functions, the head / body / tail split and the loop over one table entry) on the CPU, no device: a stand-alone program for
// the host sanitizers.
//
//   c++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/precision_check.cpp -o precision_check && ./precision_check
//
// widen_span / narrow_span are what a thread of widen_kernel / narrow_kernel runs; here every "thread" runs in turn.  For
// every float-side offset of 0..3 elements from a 16-byte boundary and every count of 0, 1, 3, 4, 5, 63, 64, 65 and 1027: each
// result equals the C cast (with the unit factor: the cast, one product, one quotient), every element is written exactly once,
// and the guard elements in front of and behind every destination are intact.  The values cover +-0, the smallest and the
// largest f32 subnormal, FLT_MIN, and the two doubles either side of a float rounding tie.
// Exit status 0 and "ok" when everything holds.
#include <cfloat>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../climt_amd/csrc/rrtmg_precision.h"
#include "check_common.h"

using namespace rrtmg;

static const size_t kCounts[] = {0, 1, 3, 4, 5, 63, 64, 65, 1027};
static const size_t kThreads[] = {7, 256, 4096};   // (at least 6: the first threads take the head and the tail)

int main() {
  // ---- the element functions ------------------------------------------------------------------------------------------------
  const float sub_min = nextafterf(0.0f, 1.0f), sub_max = nextafterf(FLT_MIN, 0.0f);
  const float fvals[] = {0.0f, -0.0f, sub_min, -sub_min, sub_max, -sub_max, FLT_MIN, -FLT_MIN, 1.0f, 1e-41f, 3.25f, FLT_MAX};
  for (float f : fvals) {
    CHECK(same_bits(widen_element(f, 0.0, 0.0), (double)f));
    CHECK(same_bits(narrow_element(widen_element(f, 0.0, 0.0)), f));      // exact both ways
    volatile double p = (double)f * 0.01;
    CHECK(same_bits(widen_element(f, 0.01, 0.0), (double)p));
    volatile double q = (double)f * 28.964; q = q / 18.02;
    CHECK(same_bits(widen_element(f, 28.964, 18.02), (double)q));
  }
  CHECK(std::signbit(widen_element(-0.0f, 0.0, 0.0)) && !std::signbit(widen_element(0.0f, 0.0, 0.0)));
  // a rounding tie of float: exactly half-way between 1 and 1 + 2^-23; the doubles either side of it, and the tie itself (even)
  const double tie = 1.0 + std::ldexp(1.0, -24), below = std::nextafter(tie, 0.0), above = std::nextafter(tie, 2.0);
  CHECK(same_bits(narrow_element(below), 1.0f) && same_bits(narrow_element(above), nextafterf(1.0f, 2.0f)) && same_bits(narrow_element(tie), 1.0f));
  // ... and of the subnormal range: half the smallest subnormal rounds to +0 (even), the double above it to the subnormal
  const double half_min = std::ldexp(1.0, -150);
  CHECK(same_bits(narrow_element(half_min), 0.0f) && same_bits(narrow_element(std::nextafter(half_min, 1.0)), sub_min));
  CHECK(same_bits(narrow_element(-half_min), -0.0f) && same_bits(narrow_element((double)sub_max), sub_max) && same_bits(narrow_element(1e-41), 1e-41f));
  const double dvals[] = {0.0, -0.0, tie, below, above, half_min, -half_min, std::nextafter(half_min, 1.0), (double)sub_min, (double)sub_max,
                          (double)FLT_MIN, 1e-41, -1e-41, 3e-39, 1361.0 / 3.0, -240.123456789, 1e-300, std::ldexp(1.0, -127) + std::ldexp(1.0, -151)};
  const size_t nd = sizeof dvals / sizeof dvals[0], nf = sizeof fvals / sizeof fvals[0];
  for (double d : dvals) CHECK(same_bits(narrow_element(d), (float)d));

  // ---- the split ---------------------------------------------------------------------------------------------------------------
  for (uintptr_t a = 0; a < 64; a += 4)
    for (size_t n : kCounts) {
      const PrecisionSplit s = precision_split(a, n);
      CHECK(s.head <= 3 && s.head <= n && s.head + 4 * s.quads <= n && n - s.head - 4 * s.quads <= 3);
      if (s.quads) CHECK((a + 4 * s.head) % 16 == 0);
    }

  // ---- the spans: every offset x count x thread count, guards on both sides ------------------------------------------------------
  long cases = 0;
  for (size_t off = 0; off < 4; ++off)
    for (size_t n : kCounts)
      for (size_t nt : kThreads)
        for (int scaled = 0; scaled < 2; ++scaled) {
          const double mul = scaled ? 28.964 : 0.0, div = scaled ? 18.02 : 0.0;
          // widen: the float side is the source, `off` elements behind a 16-byte boundary
          {
            std::vector<float> raw(n + 8);
            float *src = raw.data();
            while ((uintptr_t)src % 16) ++src;
            src += off;
            for (size_t i = 0; i < n; ++i) src[i] = fvals[i % nf] * (i % 5 == 4 ? 0.5f : 1.0f);
            const std::vector<float> before(src, src + n);
            std::vector<double> dst(n + 2 * kGuard, -777.25);
            for (size_t t = 0; t < nt; ++t) widen_span(src, dst.data() + kGuard, n, mul, div, t, nt);
            for (size_t i = 0; i < n; ++i) {
              volatile double w = (double)src[i];
              if (scaled) { w = w * mul; w = w / div; }
              CHECK(same_bits(dst[kGuard + i], (double)w));
            }
            for (size_t g = 0; g < kGuard; ++g) CHECK(dst[g] == -777.25 && dst[kGuard + n + g] == -777.25);
            CHECK(n == 0 || memcmp(before.data(), src, n * sizeof(float)) == 0);
          }
          // narrow: the float side is the destination
          if (!scaled) {
            std::vector<double> src(n);
            for (size_t i = 0; i < n; ++i) src[i] = dvals[i % nd];
            std::vector<float> raw(n + 2 * kGuard + 8, -777.25f);
            float *dst = raw.data() + kGuard;
            while ((uintptr_t)dst % 16) ++dst;
            dst += off;
            // (count the writes: a second pass on a zeroed copy must produce the same, and a poisoned one shows a missed element)
            for (size_t t = 0; t < nt; ++t) narrow_span(src.data(), dst, n, t, nt);
            for (size_t i = 0; i < n; ++i) CHECK(same_bits(dst[i], (float)src[i]));
            for (float *g = raw.data(); g < dst; ++g) CHECK(*g == -777.25f);
            for (float *g = dst + n; g < raw.data() + raw.size(); ++g) CHECK(*g == -777.25f);
          }
          ++cases;
        }
  printf("ok (%ld span cases)\n", cases);
  return 0;
}
