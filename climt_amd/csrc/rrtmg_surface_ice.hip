// rrtmg_surface_ice.hip -- the kernel of the implicit snow/ice column (rrtmg_surface_ice.h) and its C entry:
//   rrtmg_hip_surface_ice    climt SeaIce (kind 0) and LandIce (kind 1): one Crank-Nicolson heat-diffusion step of the snow/ice
//                            column, surface melt, basal growth, the surface temperature, albedo and the flux the slab reads
#include "rrtmg_column_call.h"
#include "rrtmg_surface_ice.h"

namespace rrtmg {

// the arrays of the public struct (rrtmg_column_call.h); tools/surface_ice_check.cpp includes this file for the table alone.
// Every two-dimensional array is [nlay][ncol]: nlay counts the ice interface levels
#define ROW(m) RRTMG_COLUMN_ROW(rrtmg_surface_ice, SurfaceIceCall, m)
constexpr ColumnRow kSurfaceIceRows[] = {
    {ROW(t), ColumnExt::Lay, true}, {ROW(height), ColumnExt::Lay, true},
    {ROW(thick), ColumnExt::Col, true}, {ROW(snow), ColumnExt::Col, true}, {ROW(base), ColumnExt::Col, true},
    {ROW(sw_down), ColumnExt::Col, true}, {ROW(lw_down), ColumnExt::Col, true}, {ROW(sw_up), ColumnExt::Col, true}, {ROW(lw_up), ColumnExt::Col, true},
    {ROW(lh), ColumnExt::Col, true}, {ROW(sh), ColumnExt::Col, true}, {ROW(area_type), ColumnExt::Col, true},
    {ROW(t_out), ColumnExt::Lay, true, "t"}, {ROW(height_out), ColumnExt::Lay, true, "height"},
    {ROW(thick_out), ColumnExt::Col, true, "thick"}, {ROW(snow_out), ColumnExt::Col, true, "snow"}, {ROW(tsfc_out), ColumnExt::Col, true},
    {ROW(base_flux_out), ColumnExt::Col, true, "base"},      // in place for kind 0 only: the entry refuses it for kind 1
    {ROW(cond_flux), ColumnExt::Col, false}, {ROW(albedo), ColumnExt::Col, false}, {ROW(flags), ColumnExt::Col, false}};
#undef ROW
constexpr ColumnTable kSurfaceIce = column_table("surface_ice", "rrtmg_surface_ice", 3, "ncol must be positive",
                                                 "nlay must be at least 3 (the ice interface levels: the rule reads the two uppermost layers)",
                                                 " (in place: exactly its own input)", kSurfaceIceRows);

}  // namespace rrtmg

#ifdef __HIPCC__
namespace rrtmg {

// One thread per column, tiles of 64 columns: the Thomas sweep is sequential in the vertical (rrtmg_surface_ice.h), so the
// parallelism is the columns'.  Every array is [node][ncol]: the 64 lanes of a wave read and write one run of 512 bytes per
// access, and every element is touched by one lane only.  A column reads t once (twice where a melt is reverted), writes c' and d'
// and reads them back once; at 8192 columns (128 waves on 256 CUs) what bounds the kernel is the latency of one column's chain --
// three dependent double divisions per node on the way up -- not bandwidth.  The lanes of a wave diverge only where columns
// differ in kind (inactive, reverted melt); every loop is bounded by nlay and a thread keeps no array of its own.
__global__ void __launch_bounds__(64) surface_ice_kernel(SurfaceIceCall a) {
  const long col = (long)blockIdx.x * 64 + threadIdx.x;
  if (col >= a.ncol) return;
  surface_ice_column(a, col);
}

}  // namespace rrtmg

using namespace rrtmg;

extern "C" int rrtmg_hip_surface_ice(rrtmg_ctx *ctx, const rrtmg_surface_ice *a) {
  int rc = column_head(ctx, kSurfaceIce, a);
  if (rc) return rc;
  if (a->kind != 0 && a->kind != 1) return ctx->fail(RRTMG_ERR_ARG, "surface_ice: kind must be 0 (sea ice) or 1 (land ice)");
  if (a->reserved != 0) return ctx->fail(RRTMG_ERR_ARG, "surface_ice: reserved must be 0");
  if (!(a->dt > 0.0)) return ctx->fail(RRTMG_ERR_ARG, "surface_ice: dt must be positive");
  rc = column_required(ctx, kSurfaceIce, a);
  if (rc) return rc;
  if (a->kind == 1 && (const void *)a->base_flux_out == (const void *)a->base)
    return ctx->fail(RRTMG_ERR_ARG, "surface_ice: base_flux_out aliases an input (kind 1: base is the soil temperature, which the call does not step)");
  const size_t nl = (size_t)a->nlay * (size_t)a->ncol;
  SurfaceIceCall c{};
  c.ncol = a->ncol; c.nlay = a->nlay; c.kind = a->kind;
  c.dt = a->dt; c.rho_ice = a->rho_ice; c.rho_snow = a->rho_snow; c.c_ice = a->c_ice; c.c_snow = a->c_snow; c.k_ice = a->k_ice; c.k_snow = a->k_snow;
  c.lf = a->lf; c.t_melt = a->t_melt; c.eps = a->eps; c.max_height = a->max_height;
  c.albedo_snow = a->albedo_snow; c.albedo_ice = a->albedo_ice; c.albedo_melt = a->albedo_melt;
  // host pointers: the inputs go up; temperature, heights, thickness, snow and the base flux are stepped in place in their device copies
  return column_call(ctx, kSurfaceIce, a, c, 0u, "ice.io", [&]() -> int {
    double *work = (double *)ctx->buf("ice.work", 2 * nl * sizeof(double));
    if (!work) return ctx->status;
    c.work_c = work; c.work_d = work + nl;
    return RRTMG_OK;
  }, [&] { return column_launch(ctx, surface_ice_kernel, (size_t)a->ncol, c); });
}
#endif
