// rrtmg_precision.h -- the float32 BOUNDARY (rrtmg_hip_{sw,lw,radiation}_fluxes_f32): the caller's grid arrays are 4-byte reals,
// the call itself is the unchanged fp64 one on an internal copy.  One WIDEN launch in front (float -> double, exact; a unit
// factor folds in: double(x) * mul, then / div, one rounding per operation), one NARROW launch behind (double -> float, one
// rounding to nearest-even, subnormal results included: what numpy.astype(float32) does).  No kernel that does physics knows.
//
// Both launches take a by-value table with one entry per blockIdx.z (the pattern of permute_gather_kernel).  A thread moves four
// elements per trip -- one 16-byte access on the float side, two on the double side -- between a scalar head and a scalar tail.
// The head is computed from the address of the FLOAT side, the caller's, which is only 4-byte aligned; the double side is an
// internal buffer whose 16-byte phase then follows the head's parity, so its accesses are declared 8-byte aligned.
//
// The first part is plain C++ -- the element functions, the split and the loop over one entry: tools/precision_check.cpp runs
// it on the CPU -- the kernels and the host struct follow under __HIPCC__.
#pragma once
#include <cstddef>
#include <cstdint>

#ifdef __HIPCC__
#define RRTMG_PRECISION_HD __host__ __device__ inline
#else
#define RRTMG_PRECISION_HD inline
#endif

namespace rrtmg {

// ---- the element functions: ONE rule for the device and the CPU check -------------------------------------------------------
// float -> double is exact (subnormals included); mul == 0: as given; div == 0: no division
RRTMG_PRECISION_HD double widen_element(float x, double mul, double div) {
#pragma clang fp contract(off)
  double v = (double)x;
  if (mul != 0.0) {
    v = v * mul;
    if (div != 0.0) v = v / div;
  }
  return v;
}
// double -> float: one rounding, to nearest-even, into the subnormal range where the result lies there
RRTMG_PRECISION_HD float narrow_element(double x) { return (float)x; }

// ---- the split of an array of n elements whose float side starts at address `addr` (4-byte aligned) ----------------------------
// [0, head) scalar, then `quads` groups of four whose float side is 16-byte aligned, then the scalar tail up to n
struct PrecisionSplit { size_t head, quads; };
RRTMG_PRECISION_HD PrecisionSplit precision_split(uintptr_t addr, size_t n) {
  size_t head = ((16 - (addr & 15)) & 15) >> 2;
  if (head > n) head = n;
  return {head, (n - head) >> 2};
}

// One table entry: widen src = const float *, dst = double *; narrow src = const double *, dst = float *
struct PrecisionEntry { const void *src; void *dst; size_t n; double mul, div; };
// one widen table for a call's inputs, one narrow table for its outputs: rrtmg_call.h asserts that the lists of
// rrtmg_call_arrays.h fit (HostInputs' batch of a host-pointer call may flush a full table and go on)
constexpr int kPrecisionMaxEntries = 32;
struct PrecisionTable { PrecisionEntry e[kPrecisionMaxEntries]; };
static_assert(sizeof(PrecisionTable) + 40 <= 4096, "kernel arguments: 4 KB at the most");

// four elements at once; the device compiles these to vector accesses, the host walks the same indices one by one
#if defined(__HIP_DEVICE_COMPILE__)
typedef float precision_f4 __attribute__((ext_vector_type(4)));                  // 16-byte aligned: the split sees to it
typedef double precision_d2 __attribute__((ext_vector_type(2), aligned(8)));     // an 8-byte aligned pair
#endif
RRTMG_PRECISION_HD void widen_quad(const float *src, double *dst, double mul, double div) {
#if defined(__HIP_DEVICE_COMPILE__)
  const precision_f4 x = *(const precision_f4 *)src;
  precision_d2 lo, hi;
  lo.x = widen_element(x.x, mul, div); lo.y = widen_element(x.y, mul, div);
  hi.x = widen_element(x.z, mul, div); hi.y = widen_element(x.w, mul, div);
  *(precision_d2 *)dst = lo; *(precision_d2 *)(dst + 2) = hi;
#else
  for (int k = 0; k < 4; ++k) dst[k] = widen_element(src[k], mul, div);
#endif
}
RRTMG_PRECISION_HD void narrow_quad(const double *src, float *dst) {
#if defined(__HIP_DEVICE_COMPILE__)
  const precision_d2 lo = *(const precision_d2 *)src, hi = *(const precision_d2 *)(src + 2);
  precision_f4 y;
  y.x = narrow_element(lo.x); y.y = narrow_element(lo.y); y.z = narrow_element(hi.x); y.w = narrow_element(hi.y);
  *(precision_f4 *)dst = y;
#else
  for (int k = 0; k < 4; ++k) dst[k] = narrow_element(src[k]);
#endif
}
// The work of thread `tid` of `nthreads` on one entry: quads tid, tid + nthreads, ...; the first threads take one head or tail
// element each (at most 3 + 3).  Every element of [0, n) is written by exactly one thread, and nothing else is.
RRTMG_PRECISION_HD void widen_span(const float *src, double *dst, size_t n, double mul, double div, size_t tid, size_t nthreads) {
  const PrecisionSplit sp = precision_split((uintptr_t)src, n);
  for (size_t q = tid; q < sp.quads; q += nthreads) widen_quad(src + sp.head + 4 * q, dst + sp.head + 4 * q, mul, div);
  const size_t tail0 = sp.head + 4 * sp.quads;
  if (tid < sp.head) dst[tid] = widen_element(src[tid], mul, div);
  else if (tid - sp.head < n - tail0) { const size_t i = tail0 + (tid - sp.head); dst[i] = widen_element(src[i], mul, div); }
}
RRTMG_PRECISION_HD void narrow_span(const double *src, float *dst, size_t n, size_t tid, size_t nthreads) {
  const PrecisionSplit sp = precision_split((uintptr_t)dst, n);
  for (size_t q = tid; q < sp.quads; q += nthreads) narrow_quad(src + sp.head + 4 * q, dst + sp.head + 4 * q);
  const size_t tail0 = sp.head + 4 * sp.quads;
  if (tid < sp.head) dst[tid] = narrow_element(src[tid]);
  else if (tid - sp.head < n - tail0) { const size_t i = tail0 + (tid - sp.head); dst[i] = narrow_element(src[i]); }
}

}  // namespace rrtmg

#ifdef __HIPCC__
#include <hip/hip_runtime.h>


namespace rrtmg {

// launches (rrtmg_precision.hip): n entries of t, grid.x sized from the largest of them
void launch_widen(hipStream_t s, const PrecisionTable &t, int n);
void launch_narrow(hipStream_t s, const PrecisionTable &t, int n);

// The host side of one launch: entries collected, one launch at flush() (a full table is flushed and goes on).
struct PrecisionBatch {
  hipStream_t s;
  bool widen;
  PrecisionTable tab{};
  int ntab = 0;
  PrecisionBatch(hipStream_t st, bool w) : s(st), widen(w) {}
  void add(const void *src, void *dst, size_t n, double mul = 0.0, double div = 0.0) {
    if (!n) return;
    if (ntab == kPrecisionMaxEntries) flush();
    tab.e[ntab++] = {src, dst, n, mul, div};
  }
  void flush() {
    if (ntab) { if (widen) launch_widen(s, tab, ntab); else launch_narrow(s, tab, ntab); }
    ntab = 0;
  }
};

}  // namespace rrtmg
#endif  // __HIPCC__
