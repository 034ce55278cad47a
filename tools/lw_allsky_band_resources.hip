// Development tool (no GPU needed): where lw_solve_all_allsky_kernel<true, MR> spills.  Every (band, G) instantiation of
// lw_solve_thread in the one-stream mode as a kernel of its own, with the solve kernel's launch bounds, waves-per-SIMD attribute
// and LDS slice, so that the compiler's resource report states VGPRs, scratch and spilled VGPRs per band:
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 --cuda-device-only -Rpass-analysis=kernel-resource-usage [-DRRTMG_BAND_MR=true] \
//         -c tools/lw_allsky_band_resources.hip -o /dev/null
// (the product kernel holds all of them behind one switch: its figures are at least the largest of these)
#include "../climt_amd/csrc/rrtmg_lw_device.h"

#ifndef RRTMG_BAND_MR
#define RRTMG_BAND_MR false
#endif

namespace rrtmg {

template <int BAND, int G>
__global__ void __launch_bounds__(64 * 4) __attribute__((amdgpu_waves_per_eu(2))) band_kernel(LwDev d, LwTab T, int slot, int ig0) {
  __shared__ __attribute__((aligned(16))) double sh_k[kLwSlabMaxRows * 4];
  for (int i = threadIdx.x; i < kLwSlabMaxRows * 4; i += 256) sh_k[i] = T.t[i];
  __syncthreads();
  const int col = blockIdx.x * 64 + (threadIdx.x & 63);
  if (col >= d.ncol) return;
  double *scr = d.scratch + (long)blockIdx.x * LF_N * d.nlay * 64 * G + (threadIdx.x & 63) * 2;
  LwPartSinkAllsky sink = lw_part_sink_allsky(d, slot, col);
  lw_solve_thread<BAND, G, true, RRTMG_BAND_MR, true, true>(d, T, col, ig0, scr, 64, sink, sh_k);
}

template <int BAND>
void instantiate(LwDev d, LwTab T) {
  constexpr int ng = kLwNg[BAND - 1];
  if constexpr (ng >= 4) hipLaunchKernelGGL((band_kernel<BAND, 4>), dim3(1), dim3(256), 0, 0, d, T, 0, 0);
  if constexpr (ng % 4 != 0) hipLaunchKernelGGL((band_kernel<BAND, 2>), dim3(1), dim3(256), 0, 0, d, T, 0, 0);
}
void all(LwDev d, LwTab T) {
  instantiate<1>(d, T); instantiate<2>(d, T); instantiate<3>(d, T); instantiate<4>(d, T); instantiate<5>(d, T); instantiate<6>(d, T);
  instantiate<7>(d, T); instantiate<8>(d, T); instantiate<9>(d, T); instantiate<10>(d, T); instantiate<11>(d, T); instantiate<12>(d, T);
  instantiate<13>(d, T); instantiate<14>(d, T); instantiate<15>(d, T); instantiate<16>(d, T);
}

}  // namespace rrtmg
