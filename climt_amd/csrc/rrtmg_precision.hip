// rrtmg_precision.hip -- the two kernels of the float32 boundary (rrtmg_precision.h) and their launches.
#include "rrtmg_precision.h"

namespace rrtmg {

// Streaming, HBM-bound: entry blockIdx.z of the table, the blocks of grid.x striding over its groups of four elements
// (widen_span / narrow_span: float4 in and two double2 out, and the reverse; scalar head and tail).  Plain loads and stores.
__global__ void __launch_bounds__(256) widen_kernel(PrecisionTable t) {
  const PrecisionEntry e = t.e[blockIdx.z];
  widen_span((const float *)e.src, (double *)e.dst, e.n, e.mul, e.div, (size_t)blockIdx.x * 256 + threadIdx.x, (size_t)gridDim.x * 256);
}
__global__ void __launch_bounds__(256) narrow_kernel(PrecisionTable t) {
  const PrecisionEntry e = t.e[blockIdx.z];
  narrow_span((const double *)e.src, (float *)e.dst, e.n, (size_t)blockIdx.x * 256 + threadIdx.x, (size_t)gridDim.x * 256);
}

// grid.x: one trip per thread for the largest entry, up to 2048 blocks (8 per CU); at least one block, whose first threads
// take the head and the tail of an entry too short for a group of four
static dim3 precision_grid(const PrecisionTable &t, int n) {
  size_t most = 0;
  for (int i = 0; i < n; ++i) most = t.e[i].n > most ? t.e[i].n : most;
  size_t bx = (most / 4 + 255) / 256;
  bx = bx < 1 ? 1 : (bx > 2048 ? 2048 : bx);
  return dim3((unsigned)bx, 1, (unsigned)n);
}
void launch_widen(hipStream_t s, const PrecisionTable &t, int n) { hipLaunchKernelGGL(widen_kernel, precision_grid(t, n), dim3(256), 0, s, t); }
void launch_narrow(hipStream_t s, const PrecisionTable &t, int n) { hipLaunchKernelGGL(narrow_kernel, precision_grid(t, n), dim3(256), 0, s, t); }

}  // namespace rrtmg
