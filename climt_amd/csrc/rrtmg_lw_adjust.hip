// rrtmg_lw_adjust.hip -- the kernel of the longwave between radiation calls (rrtmg_lw_adjust.h) and its C entry:
//   rrtmg_hip_lw_adjust_surface   uflx' = uflx + duflx_dt * (tsfc_now - tsfc_call) at every level and the heating rates of the
//                                 corrected net fluxes, all-sky and clear-sky stream in ONE launch: streaming (7 or 13 arrays read,
//                                 2 or 4 written, once each), a handful of flops per element
#include "rrtmg_column_call.h"   // the aliasing check of the column components
#include "rrtmg_ctx.h"
#include "rrtmg_lw_adjust.h"
#include "rrtmg_lw_device.h"   // LwTab: the heatfac of rrtmg_hip_lw_init

namespace rrtmg {

// grid (column tiles of 64, blocks of layers): a thread owns one column of one block of layers (lw_adjust_thread: which levels it
// writes, its one halo level, and why an in-place launch is one block deep).  One thread per column alone would leave 8192
// columns at 128 waves on 256 CUs; 8 layers per thread give 60 layers 8 times as many.  Columns fastest: every access of a wave is
// one coalesced run of 64 x 8 bytes; non-temporal (every element is read once or -- a halo -- twice, and the next reader is
// another kernel).  dT is formed once per thread; the net flux and the pressure of the level below stay in registers.
__global__ void __launch_bounds__(64) lw_adjust_surface_kernel(LwAdjustCall a) {
  const int col = blockIdx.x * 64 + threadIdx.x;
  if (col >= a.ncol) return;
  lw_adjust_thread(a, col, blockIdx.y, gridDim.y);
}

}  // namespace rrtmg

using namespace rrtmg;

extern "C" int rrtmg_hip_lw_adjust_surface(rrtmg_ctx *ctx, const rrtmg_lw_adjust *a) {
  if (!ctx) return RRTMG_ERR_ARG;
  if (!a) return ctx->fail(RRTMG_ERR_ARG, "lw_adjust_surface: NULL argument struct");
  if (a->struct_size != sizeof(rrtmg_lw_adjust))
    return ctx->fail(RRTMG_ERR_ARG, "lw_adjust_surface: struct_size %u, this library's rrtmg_lw_adjust has %zu bytes", a->struct_size, sizeof(rrtmg_lw_adjust));
  if (a->ncol <= 0 || a->nlay <= 0) return ctx->fail(RRTMG_ERR_ARG, "lw_adjust_surface: ncol/nlay must be positive");
  if (!a->tsfc_call || !a->tsfc_now || !a->plev || !a->uflx || !a->dflx || !a->duflx_dt || !a->uflx_out || !a->hr_out)
    return ctx->fail(RRTMG_ERR_ARG, "lw_adjust_surface: tsfc_call, tsfc_now, plev, uflx, dflx, duflx_dt, uflx_out and hr_out must be given");
  const int nclr = (a->uflxc != nullptr) + (a->dflxc != nullptr) + (a->duflxc_dt != nullptr), nclr_out = (a->uflxc_out != nullptr) + (a->hrc_out != nullptr);
  if ((nclr != 0 && nclr != 3) || nclr_out != (nclr ? 2 : 0))
    return ctx->fail(RRTMG_ERR_ARG, "lw_adjust_surface: the clear-sky stream is uflxc, dflxc, duflxc_dt, uflxc_out and hrc_out: all five, or none");
  // (sizes in bytes)
  const size_t b1 = (size_t)a->ncol * sizeof(double), bl = (size_t)a->nlay * b1, bl1 = bl + b1;
  const ColumnSpan spans[] = {{"tsfc_call", a->tsfc_call, b1}, {"tsfc_now", a->tsfc_now, b1}, {"plev", a->plev, bl1}, {"uflx", a->uflx, bl1}, {"dflx", a->dflx, bl1},
      {"duflx_dt", a->duflx_dt, bl1}, {"uflxc", a->uflxc, bl1}, {"dflxc", a->dflxc, bl1}, {"duflxc_dt", a->duflxc_dt, bl1},
      {"uflx_out", a->uflx_out, bl1, true, a->uflx}, {"hr_out", a->hr_out, bl, true}, {"uflxc_out", a->uflxc_out, bl1, true, a->uflxc}, {"hrc_out", a->hrc_out, bl, true}};
  char msg[160];
  if (aliasing_refusal(spans, sizeof spans / sizeof spans[0], " (in place: exactly the upward flux of its stream)", msg, sizeof msg))
    return ctx->fail(RRTMG_ERR_ARG, "lw_adjust_surface: %s", msg);
  // heatfac is that of rrtmg_hip_lw_init: the status and the message of the flux call (call_begin)
  if (!ctx->lw_ready || !ctx->lw_desc) return ctx->fail(RRTMG_ERR_NOT_INITIALISED, "%s", "rrtmg_hip_lw_init has not been called");
  int rc = ctx_prepare_device(ctx);
  if (rc) return rc;
  LwAdjustCall c{};
  c.ncol = a->ncol; c.nlay = a->nlay;
  c.tsfc_call = a->tsfc_call; c.tsfc_now = a->tsfc_now; c.plev = a->plev;
  c.pressure_scale = a->pressure_scale; c.heatfac = ((const LwTab *)ctx->lw_desc)->heatfac;
  c.all = {a->uflx, a->dflx, a->duflx_dt, a->uflx_out, a->hr_out};
  if (nclr) c.clr = {a->uflxc, a->dflxc, a->duflxc_dt, a->uflxc_out, a->hrc_out};
  const bool in_place = a->uflx_out == a->uflx || (nclr && a->uflxc_out == a->uflxc);
  // the longwave's stream (the rule of call_stream, rrtmg_call.h, for device pointers): behind the flux call that wrote the kept arrays
  hipStream_t s = ctx->deferred ? ctx->stream_lw : ctx->stream;
  hipLaunchKernelGGL(lw_adjust_surface_kernel, dim3((a->ncol + 63) / 64, lw_adjust_grid_y(a->nlay, in_place)), dim3(64), 0, s, c);
  RRTMG_HIP_CHECK(ctx, hipGetLastError());
  if (!ctx->deferred) RRTMG_HIP_CHECK(ctx, hipStreamSynchronize(s));
  return RRTMG_OK;
}
