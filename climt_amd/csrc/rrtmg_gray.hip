// rrtmg_gray.hip -- the kernels of the gray radiation path and its moisture sink (rrtmg_gray.h) and their C entries:
//   rrtmg_hip_frierson_optical_depth    climt Frierson06LongwaveOpticalDepth: the longwave optical depth of every interface
//   rrtmg_hip_gray_longwave             climt GrayLongwaveRadiation: the two-stream gray sweep and its heating; with `frierson` the
//                                       optical depth is formed inside the sweep and never touches HBM
//   rrtmg_hip_grid_scale_condensation   climt GridScaleCondensation: grid-scale supersaturation removed, layer by layer
#include "rrtmg_column_call.h"
#include "rrtmg_gray.h"

namespace rrtmg {

// the arrays of the three public structs (rrtmg_column_call.h); tools/gray_check.cpp includes this file for the tables alone
#define ROW(m) RRTMG_COLUMN_ROW(rrtmg_frierson_optical_depth, FriersonCall, m)
constexpr ColumnRow kFriersonRows[] = {{ROW(pint), ColumnExt::Lev, true}, {ROW(ps), ColumnExt::Col, true}, {ROW(lat), ColumnExt::Col, true}, {ROW(tau), ColumnExt::Lev, true}};
#undef ROW
constexpr ColumnTable kFrierson = column_table("frierson_optical_depth", "rrtmg_frierson_optical_depth", 1, "ncol must be positive", "nlay must be at least 1", "", kFriersonRows);

#define ROW(m) RRTMG_COLUMN_ROW(rrtmg_gray_longwave, GrayLongwaveCall, m)
constexpr ColumnRow kGrayLongwaveRows[] = {
    {ROW(t), ColumnExt::Lay, true}, {ROW(tsfc), ColumnExt::Col, true}, {ROW(pint), ColumnExt::Lev, true},
    {ROW(tau), ColumnExt::Lev, false}, {ROW(ps), ColumnExt::Col, false}, {ROW(lat), ColumnExt::Col, false},   // read where `frierson` says so
    {ROW(up), ColumnExt::Lev, true}, {ROW(dn), ColumnExt::Lev, true}, {ROW(tend), ColumnExt::Lay, true},
    {ROW(hr), ColumnExt::Lay, false}, {ROW(tau_out), ColumnExt::Lev, false}};
#undef ROW
constexpr ColumnTable kGrayLongwave = column_table("gray_longwave", "rrtmg_gray_longwave", 1, "ncol must be positive", "nlay must be at least 1", "", kGrayLongwaveRows);

#define ROW(m) RRTMG_COLUMN_ROW(rrtmg_grid_scale_condensation, GridScaleCondensationCall, m)
constexpr ColumnRow kGridScaleCondensationRows[] = {
    {ROW(t), ColumnExt::Lay, true}, {ROW(q), ColumnExt::Lay, true}, {ROW(pmid), ColumnExt::Lay, true}, {ROW(pint), ColumnExt::Lev, true},
    {ROW(t_out), ColumnExt::Lay, true, "t"}, {ROW(q_out), ColumnExt::Lay, true, "q"}, {ROW(precip), ColumnExt::Col, false}};
#undef ROW
constexpr ColumnTable kGridScaleCondensation = column_table("grid_scale_condensation", "rrtmg_grid_scale_condensation", 1, "ncol must be positive",
                                                            "nlay must be at least 1", " (in place: exactly its own input)", kGridScaleCondensationRows);

}  // namespace rrtmg

#ifdef __HIPCC__
namespace rrtmg {

// One thread per column, tiles of 64 columns: the two sweeps and the precipitation sum are sequential in the vertical
// (rrtmg_gray.h), so the parallelism is the columns'.  Every array is [k][ncol]: the 64 lanes of a wave read and write one run of
// 512 bytes per access, and every element is touched by one lane only.  The kernels stream their arrays -- the depth once, the
// condensation once, the sweep its inputs once and three of its outputs twice (rrtmg_gray.h: what the upward pass leaves for
// the downward one); what bounds them at 8192 columns (128 waves on 256 CUs) is the latency of one column's chain, an exp and a
// pow per layer, not bandwidth.  Every loop is bounded by nlay and a thread keeps no array of its own.
__global__ void __launch_bounds__(64) frierson_kernel(FriersonCall a) {
  const long col = (long)blockIdx.x * 64 + threadIdx.x;
  if (col >= a.ncol) return;
  frierson_column(a, col);
}

__global__ void __launch_bounds__(64) gray_longwave_kernel(GrayLongwaveCall a) {
  const long col = (long)blockIdx.x * 64 + threadIdx.x;
  if (col >= a.ncol) return;
  gray_longwave_column(a, col);
}

__global__ void __launch_bounds__(64) grid_scale_condensation_kernel(GridScaleCondensationCall a) {
  const long col = (long)blockIdx.x * 64 + threadIdx.x;
  if (col >= a.ncol) return;
  grid_scale_condensation_column(a, col);
}

}  // namespace rrtmg

using namespace rrtmg;

extern "C" int rrtmg_hip_frierson_optical_depth(rrtmg_ctx *ctx, const rrtmg_frierson_optical_depth *a) {
  int rc = column_head(ctx, kFrierson, a);
  if (rc) return rc;
  rc = column_required(ctx, kFrierson, a);
  if (rc) return rc;
  FriersonCall c{};
  c.ncol = a->ncol; c.nlay = a->nlay;
  c.tau0e = a->tau0e; c.tau0p = a->tau0p; c.fl = a->fl; c.pressure_scale = a->pressure_scale; c.ps_scale = a->ps_scale;
  return column_call(ctx, kFrierson, a, c, 0u, "fr.io", [] { return RRTMG_OK; }, [&] { return column_launch(ctx, frierson_kernel, (size_t)a->ncol, c); });
}

extern "C" int rrtmg_hip_gray_longwave(rrtmg_ctx *ctx, const rrtmg_gray_longwave *a) {
  int rc = column_head(ctx, kGrayLongwave, a);
  if (rc) return rc;
  if (a->frierson != 0 && a->frierson != 1) return ctx->fail(RRTMG_ERR_ARG, "gray_longwave: frierson must be 0 (tau is read) or 1 (the optical depth is formed in the sweep)");
  rc = column_required(ctx, kGrayLongwave, a);
  if (rc) return rc;
  const bool fused = a->frierson == 1;
  if (fused && !(a->ps && a->lat)) return ctx->fail(RRTMG_ERR_ARG, "gray_longwave: ps and lat must be given with frierson 1 (the optical depth is formed from pint, ps and lat)");
  if (!fused && !a->tau) return ctx->fail(RRTMG_ERR_ARG, "gray_longwave: tau must be given with frierson 0");
  constexpr unsigned tau = column_bits(kGrayLongwave, {"tau"}), surface = column_bits(kGrayLongwave, {"ps", "lat"});
  GrayLongwaveCall c{};
  c.ncol = a->ncol; c.nlay = a->nlay; c.frierson = a->frierson;
  c.tau0e = a->tau0e; c.tau0p = a->tau0p; c.fl = a->fl; c.sigma_sb = a->sigma_sb; c.g = a->g; c.cpd = a->cpd;
  c.pressure_scale = a->pressure_scale; c.ps_scale = a->ps_scale;
  return column_call(ctx, kGrayLongwave, a, c, fused ? tau : surface, "gray.io", [] { return RRTMG_OK; },
                     [&] { return column_launch(ctx, gray_longwave_kernel, (size_t)a->ncol, c); });
}

extern "C" int rrtmg_hip_grid_scale_condensation(rrtmg_ctx *ctx, const rrtmg_grid_scale_condensation *a) {
  int rc = column_head(ctx, kGridScaleCondensation, a);
  if (rc) return rc;
  rc = column_required(ctx, kGridScaleCondensation, a);
  if (rc) return rc;
  GridScaleCondensationCall c{};
  c.ncol = a->ncol; c.nlay = a->nlay;
  c.cpd = a->cpd; c.lv = a->lv; c.rd = a->rd; c.rh2o = a->rh2o; c.g = a->g; c.rhow = a->rhow; c.pressure_scale = a->pressure_scale;
  // host pointers: the inputs go up; the two profiles are written in place in their device copies
  return column_call(ctx, kGridScaleCondensation, a, c, 0u, "gsc.io", [] { return RRTMG_OK; },
                     [&] { return column_launch(ctx, grid_scale_condensation_kernel, (size_t)a->ncol, c); });
}
#endif
