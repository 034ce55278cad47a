// rrtmg_land_surface.hip -- the kernels of the two land-surface components (rrtmg_land_surface.h) and their C entries:
//   rrtmg_hip_bucket_hydrology   climt BucketHydrology: bulk surface fluxes, beta-limited evaporation, one or two soil-moisture
//                                layers with exchange, drainage and runoff, the slab (and deep-store) temperature
//   rrtmg_hip_second_best        climt SecondBEST with its default processes: surface-layer drag, albedo, beta-limited evaporation,
//                                the implicit soil heat column with freeze/melt, the screen-level diagnostics
#include "rrtmg_column_call.h"
#include "rrtmg_land_surface.h"

namespace rrtmg {

// the arrays of the public structs (rrtmg_column_call.h); tools/land_surface_check.cpp includes this file for the tables alone.
// BucketHydrology has no profile: every row is [ncol] and nlay is 1.  SecondBEST: nlay counts the soil interface levels
#define ROW(m) RRTMG_COLUMN_ROW(rrtmg_bucket_hydrology, BucketHydrologyCall, m)
constexpr ColumnRow kBucketHydrologyRows[] = {
    {ROW(t_air), ColumnExt::Col, true}, {ROW(q_air), ColumnExt::Col, true}, {ROW(u), ColumnExt::Col, true}, {ROW(v), ColumnExt::Col, true}, {ROW(p_air), ColumnExt::Col, true},
    {ROW(ts), ColumnExt::Col, true}, {ROW(q_sfc), ColumnExt::Col, true},
    {ROW(sw_down), ColumnExt::Col, true}, {ROW(lw_down), ColumnExt::Col, true}, {ROW(sw_up), ColumnExt::Col, true}, {ROW(lw_up), ColumnExt::Col, true},
    {ROW(soil_moisture), ColumnExt::Col, true}, {ROW(precip_conv), ColumnExt::Col, true}, {ROW(precip_strat), ColumnExt::Col, true},
    {ROW(density), ColumnExt::Col, true}, {ROW(thickness), ColumnExt::Col, true}, {ROW(heat_capacity), ColumnExt::Col, true},
    {ROW(deep_moisture), ColumnExt::Col, false}, {ROW(deep_temperature), ColumnExt::Col, false},      // required with layers 2, unread otherwise
    {ROW(ts_out), ColumnExt::Col, true, "ts"}, {ROW(soil_moisture_out), ColumnExt::Col, true, "soil_moisture"},
    {ROW(deep_moisture_out), ColumnExt::Col, false, "deep_moisture"}, {ROW(deep_temperature_out), ColumnExt::Col, false, "deep_temperature"},
    {ROW(precip), ColumnExt::Col, false}, {ROW(lh), ColumnExt::Col, false}, {ROW(sh), ColumnExt::Col, false}, {ROW(evaporation), ColumnExt::Col, false},
    {ROW(runoff), ColumnExt::Col, false}, {ROW(deep_fraction), ColumnExt::Col, false}};
#undef ROW
constexpr ColumnTable kBucketHydrology = column_table("bucket_hydrology", "rrtmg_bucket_hydrology", 1, "ncol must be positive",
                                                      "nlay must be 1 (every array is [ncol]: the lowest model level and the surface)",
                                                      " (in place: exactly its own input)", kBucketHydrologyRows);

#define ROW(m) RRTMG_COLUMN_ROW(rrtmg_second_best, SecondBestCall, m)
constexpr ColumnRow kSecondBestRows[] = {
    {ROW(t_soil), ColumnExt::Lay, true}, {ROW(x_w), ColumnExt::Lay, true}, {ROW(x_i), ColumnExt::Lay, true}, {ROW(height), ColumnExt::Lay, true},
    {ROW(t_air), ColumnExt::Col, true}, {ROW(q_air), ColumnExt::Col, true}, {ROW(u), ColumnExt::Col, true}, {ROW(v), ColumnExt::Col, true}, {ROW(p_air), ColumnExt::Col, true},
    {ROW(ps), ColumnExt::Col, true}, {ROW(ts), ColumnExt::Col, true}, {ROW(snow), ColumnExt::Col, true},
    {ROW(sw_down), ColumnExt::Col, true}, {ROW(lw_down), ColumnExt::Col, true}, {ROW(sw_up), ColumnExt::Col, true}, {ROW(lw_up), ColumnExt::Col, true},
    {ROW(area_type), ColumnExt::Col, true},
    {ROW(t_soil_out), ColumnExt::Lay, true, "t_soil"}, {ROW(x_w_out), ColumnExt::Lay, true, "x_w"}, {ROW(x_i_out), ColumnExt::Lay, true, "x_i"},
    {ROW(ts_out), ColumnExt::Col, true, "ts"}, {ROW(snow_out), ColumnExt::Col, true, "snow"},
    {ROW(sh), ColumnExt::Col, false}, {ROW(lh), ColumnExt::Col, false}, {ROW(evaporation), ColumnExt::Col, false},
    {ROW(albedo_direct), ColumnExt::Col, false}, {ROW(albedo_diffuse), ColumnExt::Col, false}, {ROW(cd_heat), ColumnExt::Col, false}, {ROW(cd_momentum), ColumnExt::Col, false},
    {ROW(t2m), ColumnExt::Col, false}, {ROW(q2m), ColumnExt::Col, false}, {ROW(u10), ColumnExt::Col, false}, {ROW(v10), ColumnExt::Col, false}, {ROW(flags), ColumnExt::Col, false}};
#undef ROW
constexpr ColumnTable kSecondBest = column_table("second_best", "rrtmg_second_best", 2, "ncol must be positive",
                                                 "nlay must be at least 2 (the soil interface levels: the rule reads the spacing of the two lowest)",
                                                 " (in place: exactly its own input)", kSecondBestRows);

}  // namespace rrtmg

#ifdef __HIPCC__
namespace rrtmg {

// One thread per column, tiles of 64 columns; every array is [ncol] or [node][ncol], so the 64 lanes of a wave read and write one
// run of 512 bytes per access and every element is touched by one lane only.
//
// The bucket is elementwise: 19 doubles in and at most 10 out per column, one sqrt and a dozen divisions on a chain of about 25
// dependent fp64 operations.  At 8192 columns that is 1.9 MB of traffic and 128 waves on 256 CUs: the launch and the latency of one
// column's chain bound it, neither bandwidth nor flops.  The lanes of a wave diverge at the three comparisons of the rule only.
__global__ void __launch_bounds__(64) bucket_hydrology_kernel(BucketHydrologyCall a) {
  const long col = (long)blockIdx.x * 64 + threadIdx.x;
  if (col >= a.ncol) return;
  bucket_hydrology_column(a, col);
}

// SecondBEST: the surface part is one chain through five log, two exp, two pow and four sqrt (the drag needs the height, the
// fluxes the drag, the soil column the net flux), then the Thomas sweep, sequential in the vertical: two dependent divisions per
// node on the way down to the surface row, and on the way back one multiply-subtract and the freeze/melt source, whose three
// divisions per node do not depend on the next node.  A column reads its four soil arrays once, writes c' and d' and reads them
// back once.  With 128 waves on 256 CUs at 8192 columns the latency of that chain bounds the kernel, not bandwidth.  The lanes of a
// wave diverge where columns differ in area type (inactive columns only copy) and in the stability branch; every loop is bounded
// by nlay and a thread keeps no array of its own.
__global__ void __launch_bounds__(64) second_best_kernel(SecondBestCall a) {
  const long col = (long)blockIdx.x * 64 + threadIdx.x;
  if (col >= a.ncol) return;
  second_best_column(a, col);
}

}  // namespace rrtmg

using namespace rrtmg;

extern "C" int rrtmg_hip_bucket_hydrology(rrtmg_ctx *ctx, const rrtmg_bucket_hydrology *a) {
  int rc = column_head(ctx, kBucketHydrology, a);
  if (rc) return rc;
  if (a->nlay != 1) return ctx->fail(RRTMG_ERR_ARG, "bucket_hydrology: %s", kBucketHydrology.nlay_msg);
  rc = column_required(ctx, kBucketHydrology, a);
  if (rc) return rc;
  constexpr ColumnMask deep = column_bits(kBucketHydrology, {"deep_moisture", "deep_temperature", "deep_moisture_out", "deep_temperature_out", "runoff", "deep_fraction"});
  const ColumnMask unread = a->layers == 2 ? ColumnMask(0) : deep;
  rc = column_aliasing(ctx, kBucketHydrology, a, unread);
  if (rc) return rc;
  if (!(a->dt > 0.0)) return ctx->fail(RRTMG_ERR_ARG, "bucket_hydrology: dt must be positive");
  if (a->layers != 1 && a->layers != 2) return ctx->fail(RRTMG_ERR_ARG, "bucket_hydrology: layers must be 1 or 2");
  if (a->reserved != 0 || a->reserved2 != 0) return ctx->fail(RRTMG_ERR_ARG, "bucket_hydrology: reserved must be 0");
  if (a->layers == 2) {
    if (!(a->tau_m > 0.0)) return ctx->fail(RRTMG_ERR_ARG, "bucket_hydrology: tau_m must be positive with layers 2");
    if (!a->deep_moisture || !a->deep_temperature || !a->deep_moisture_out || !a->deep_temperature_out)
      return ctx->fail(RRTMG_ERR_ARG, "bucket_hydrology: deep_moisture, deep_temperature, deep_moisture_out and deep_temperature_out must be given with layers 2");
  }
  BucketHydrologyCall c{};
  c.ncol = a->ncol; c.layers = a->layers; c.has_drain = a->has_drain != 0;
  c.dt = a->dt; c.rd = a->rd; c.cp = a->cp; c.rho_water = a->rho_water; c.lv = a->lv; c.bulk_coefficient = a->bulk_coefficient;
  c.beta_parameter = a->beta_parameter; c.soil_moisture_max = a->soil_moisture_max; c.deep_soil_moisture_max = a->deep_soil_moisture_max;
  c.tau_m = a->tau_m; c.deep_ratio = a->deep_ratio; c.tau_drain = a->tau_drain; c.pressure_scale = a->pressure_scale;
  // host pointers: the inputs go up; the temperatures and the moistures are stepped in place in their device copies
  return column_call(ctx, kBucketHydrology, a, c, unread, "bucket.io", [] { return RRTMG_OK; },
                     [&] { return column_launch(ctx, bucket_hydrology_kernel, (size_t)a->ncol, c); }, true);
}

extern "C" int rrtmg_hip_second_best(rrtmg_ctx *ctx, const rrtmg_second_best *a) {
  int rc = column_head(ctx, kSecondBest, a);
  if (rc) return rc;
  rc = column_required(ctx, kSecondBest, a);
  if (rc) return rc;
  rc = column_aliasing(ctx, kSecondBest, a, ColumnMask(0));
  if (rc) return rc;
  if (!(a->dt > 0.0)) return ctx->fail(RRTMG_ERR_ARG, "second_best: dt must be positive");
  if (a->reserved != 0 || a->reserved2 != 0) return ctx->fail(RRTMG_ERR_ARG, "second_best: reserved must be 0");
  const size_t nl = (size_t)a->nlay * (size_t)a->ncol;
  SecondBestCall c{};
  c.ncol = a->ncol; c.nlay = a->nlay;
  c.dt = a->dt; c.rd = a->rd; c.g = a->g; c.cp = a->cp; c.lv = a->lv; c.lf = a->lf; c.rho_water = a->rho_water; c.karman = a->karman;
  c.t_freeze = a->t_freeze; c.min_wind = a->min_wind; c.kappa_soil = a->kappa_soil; c.cv_soil = a->cv_soil;
  c.colour = a->colour; c.texture = a->texture; c.B = a->B; c.K_H0 = a->K_H0; c.psi_0 = a->psi_0;
  c.pressure_scale = a->pressure_scale; c.ps_scale = a->ps_scale;
  // host pointers: the inputs go up; the soil column, the surface temperature and the snow are stepped in place in their device copies
  return column_call(ctx, kSecondBest, a, c, ColumnMask(0), "best.io", [&]() -> int {
    double *work = (double *)ctx->buf("best.work", 2 * nl * sizeof(double));
    if (!work) return ctx->status;
    c.work_c = work; c.work_d = work + nl;
    return RRTMG_OK;
  }, [&] { return column_launch(ctx, second_best_kernel, (size_t)a->ncol, c); }, true);
}
#endif
