// rrtmg_lw_adjust.h -- the longwave BETWEEN two radiation calls (rrtmg_hip_lw_adjust_surface): a model that calls the radiation
// every few steps corrects the kept upward fluxes at every step for the surface temperature of that step, with the derivative
// the call formed under idrv = 1 (the comment on idrv in rrtmg_lw_rad; Hogan & Bozzo 2015), and forms the heating rates again
// from the corrected net fluxes.  OPT-IN, beside the radiation path: no kernel that does physics knows.  First order in dT: there
// is no clamp, and the downward fluxes are the call's.
//
//   one column, dT = tsfc_now - tsfc_call
//   one level     uflx'[l] = uflx[l] + duflx_dt[l] * dT                      the product rounded, then the sum: dT = 0 returns
//                                                                            the bits of uflx
//   one layer     hr'[k] = heatfac * ((uflx'[k] - dflx[k]) - (uflx'[k+1] - dflx[k+1])) / dp[k]     the expression and the order of
//                 dp[k]  = plev[k] - plev[k+1], or plev[k] * scale - plev[k+1] * scale            lw_heat_layer (rrtmg_lw_device.h):
//                                                                            dT = 0 returns the bits of the call's hr
//   (the same for the clear-sky stream: uflxc, dflxc, duflxc_dt -> uflxc', hrc')
//
// Plain C++: tools/lw_adjust_check.cpp runs every "thread" of a launch on the CPU; the kernel is in rrtmg_lw_adjust.hip.
#pragma once
#include <cstddef>
#include <cstdint>

#ifdef __HIPCC__
#define RRTMG_LW_ADJUST_HD __host__ __device__ inline
#else
#define RRTMG_LW_ADJUST_HD inline
#endif

namespace rrtmg {

// ---- the rule: ONE statement for the device and the CPU check --------------------------------------------------------------------
RRTMG_LW_ADJUST_HD double lw_adjust_flux(double uflx, double duflx_dt, double dT) {
#pragma clang fp contract(off)   // the product rounded on its own, then the sum: as the numpy statement is
  const double change = duflx_dt * dT;
  return uflx + change;
}
// pressure_scale of rrtmg_lw_args: 0 = mbar already; else the flux call scaled every element first and then took the difference
RRTMG_LW_ADJUST_HD double lw_adjust_pressure(double plev, double scale) {
#pragma clang fp contract(off)
  return scale != 0.0 ? plev * scale : plev;
}
RRTMG_LW_ADJUST_HD double lw_adjust_heat(double heatfac, double fnet0, double fnet1, double p0, double p1) {
#pragma clang fp contract(off)
  const double dp = p0 - p1;
  return heatfac * (fnet0 - fnet1) / dp;
}

// ---- the launch: who owns what ----------------------------------------------------------------------------------------------------
// One stream of the call: uflx, dflx, duflx_dt [nlay+1][ncol] -> uflx_out [nlay+1][ncol] (may be uflx), hr_out [nlay][ncol]
struct LwAdjustStream { const double *uflx, *dflx, *duflx_dt; double *uflx_out, *hr_out; };
struct LwAdjustCall {
  int32_t ncol, nlay;
  const double *tsfc_call, *tsfc_now, *plev;
  double pressure_scale, heatfac;
  LwAdjustStream all, clr;   // clr.uflx == nullptr: no clear-sky stream
};
constexpr int kLwAdjustChunk = 8;       // layers a thread keeps in flight per trip, and the depth of one thread's block of layers
constexpr int kLwAdjustMaxGridY = 64;   // blocks of layers side by side at the most: a deeper column gives every thread more trips
// Blocks of layers along gridDim.y.  IN PLACE (uflx_out == uflx, for either stream) the launch is ONE block deep: see lw_adjust_thread.
inline int lw_adjust_grid_y(int nlay, bool in_place) {
  if (in_place) return 1;
  const int g = (nlay + kLwAdjustChunk - 1) / kLwAdjustChunk;
  return g < 1 ? 1 : (g > kLwAdjustMaxGridY ? kLwAdjustMaxGridY : g);
}
// layers per thread of a launch `ny` blocks deep: a multiple of the chunk
RRTMG_LW_ADJUST_HD int lw_adjust_layers_per_thread(int nlay, int ny) {
  const int chunks = (nlay + kLwAdjustChunk - 1) / kLwAdjustChunk;
  return (chunks + ny - 1) / ny * kLwAdjustChunk;
}

RRTMG_LW_ADJUST_HD double lw_adjust_load(const double *p) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __builtin_nontemporal_load(p);
#else
  return *p;
#endif
}
RRTMG_LW_ADJUST_HD void lw_adjust_store(double v, double *p) {
#if defined(__HIP_DEVICE_COMPILE__)
  __builtin_nontemporal_store(v, p);
#else
  *p = v;
#endif
}

// One stream over the layers [k, k + n), n <= chunk, of column `col`: `net` comes in as the net flux of level k and goes out as
// that of level k + n; pr[0..n] are the (scaled) pressures of the levels k .. k + n.  write_top: level k + n is this thread's to write.
RRTMG_LW_ADJUST_HD void lw_adjust_trip(const LwAdjustStream &s, double heatfac, long ncol, long col, int k, int n, bool write_top, double dT,
                                       const double *pr, double &net) {
  double u[kLwAdjustChunk], d[kLwAdjustChunk], g[kLwAdjustChunk];
#pragma unroll
  for (int j = 0; j < kLwAdjustChunk; ++j)
    if (j < n) {
      const long o = (long)(k + 1 + j) * ncol + col;
      u[j] = lw_adjust_load(s.uflx + o); d[j] = lw_adjust_load(s.dflx + o); g[j] = lw_adjust_load(s.duflx_dt + o);
    }
#pragma unroll
  for (int j = 0; j < kLwAdjustChunk; ++j)
    if (j < n) {
      const double up = lw_adjust_flux(u[j], g[j], dT);
      if (j + 1 < n || write_top) lw_adjust_store(up, s.uflx_out + (long)(k + 1 + j) * ncol + col);
      const double above = up - d[j];
      lw_adjust_store(lw_adjust_heat(heatfac, net, above, pr[j], pr[j + 1]), s.hr_out + (long)(k + j) * ncol + col);
      net = above;
    }
}

// The work of thread (col, y) of a launch `ny` blocks deep: the layers [k0, k1), k0 = y * per, per = lw_adjust_layers_per_thread.
// It OWNS -- writes uflx' of -- the levels k0 .. k1 - 1, and level nlay where k1 == nlay; level k1 < nlay is its halo: read
// (uflx, dflx, duflx_dt, plev), its uflx' formed in registers for the layer k1 - 1, not written -- the thread y + 1 owns it and
// forms the same value from the same three inputs.  Every level is loaded ONCE per thread and its uflx' and net flux carried in
// registers to the next layer and the next trip, so a thread never reads what it wrote itself.
// IN PLACE nothing orders the read of a halo in thread y before the write of its owner y + 1, and a halo read after it would be
// corrected twice: so an in-place launch is one block deep (lw_adjust_grid_y), k1 == nlay for its only y, NO level is a halo, and
// each element of uflx is read once and written once by the one thread of its column.  Out of place uflx is only read.
RRTMG_LW_ADJUST_HD void lw_adjust_thread(const LwAdjustCall &a, long col, int y, int ny) {
  const int per = lw_adjust_layers_per_thread(a.nlay, ny);
  const long k0 = (long)y * per;
  if (k0 >= a.nlay) return;
  const int k1 = k0 + per < a.nlay ? (int)(k0 + per) : a.nlay;
  const long N = a.ncol;
  const bool clr = a.clr.uflx != nullptr;
  const double dT = lw_adjust_load(a.tsfc_now + col) - lw_adjust_load(a.tsfc_call + col);
  // level k0: owned
  const long o = k0 * N + col;
  double pr[kLwAdjustChunk + 1] = {};
  pr[0] = lw_adjust_pressure(lw_adjust_load(a.plev + o), a.pressure_scale);
  double up = lw_adjust_flux(lw_adjust_load(a.all.uflx + o), lw_adjust_load(a.all.duflx_dt + o), dT);
  double net = up - lw_adjust_load(a.all.dflx + o), netc = 0.0;
  lw_adjust_store(up, a.all.uflx_out + o);
  if (clr) {
    up = lw_adjust_flux(lw_adjust_load(a.clr.uflx + o), lw_adjust_load(a.clr.duflx_dt + o), dT);
    netc = up - lw_adjust_load(a.clr.dflx + o);
    lw_adjust_store(up, a.clr.uflx_out + o);
  }
  for (int k = (int)k0; k < k1; k += kLwAdjustChunk) {
    const int n = k1 - k < kLwAdjustChunk ? k1 - k : kLwAdjustChunk;
    const bool write_top = k + n < k1 || k1 == a.nlay;
#pragma unroll
    for (int j = 0; j < kLwAdjustChunk; ++j)
      if (j < n) pr[j + 1] = lw_adjust_pressure(lw_adjust_load(a.plev + (long)(k + 1 + j) * N + col), a.pressure_scale);
    lw_adjust_trip(a.all, a.heatfac, N, col, k, n, write_top, dT, pr, net);
    if (clr) lw_adjust_trip(a.clr, a.heatfac, N, col, k, n, write_top, dT, pr, netc);
    pr[0] = pr[kLwAdjustChunk];   // (read by a further trip only, and only a full trip has one)
  }
}

}  // namespace rrtmg
