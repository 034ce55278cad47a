// rrtmg_simple_physics.hip -- the kernel of the simple physics package (rrtmg_simple_physics.h) and its C entry:
//   rrtmg_hip_simple_physics   climt SimplePhysics (simple_physics/component.py around simple_physics_custom.f90): large-scale
//                              condensation, surface fluxes on the lowest layer and the implicit boundary-layer mixing of
//                              temperature, humidity and the two winds of every column
#include "rrtmg_column_call.h"
#include "rrtmg_simple_physics.h"

namespace rrtmg {

// the arrays of rrtmg_simple_physics (rrtmg_column_call.h); tools/column_call_check.cpp includes this file for the table alone
#define ROW(m) RRTMG_COLUMN_ROW(rrtmg_simple_physics, SimplePhysicsCall, m)
constexpr ColumnRow kSimplePhysicsRows[] = {
    {ROW(t), ColumnExt::Lay, true}, {ROW(q), ColumnExt::Lay, true}, {ROW(u), ColumnExt::Lay, true}, {ROW(v), ColumnExt::Lay, true},
    {ROW(pmid), ColumnExt::Lay, true}, {ROW(pint), ColumnExt::Lev, true}, {ROW(ps), ColumnExt::Col, true},
    {ROW(ts), ColumnExt::Col, false}, {ROW(qsurf), ColumnExt::Col, false}, {ROW(lat), ColumnExt::Col, false},   // read where the switches say so
    {ROW(t_out), ColumnExt::Lay, true, "t"}, {ROW(q_out), ColumnExt::Lay, true, "q"}, {ROW(u_out), ColumnExt::Lay, true, "u"}, {ROW(v_out), ColumnExt::Lay, true, "v"},
    {ROW(precl), ColumnExt::Col, false}, {ROW(sh_out), ColumnExt::Col, false}, {ROW(lh_out), ColumnExt::Col, false}};
#undef ROW
constexpr ColumnTable kSimplePhysics = column_table("simple_physics", "rrtmg_simple_physics", 1, "ncol must be positive", "nlay must be at least 1",
                                                    " (in place: exactly its own input)", kSimplePhysicsRows);

}  // namespace rrtmg

#ifdef __HIPCC__
namespace rrtmg {

// One thread per column, tiles of 64 columns: the precipitation sum, the elimination and the back-substitution are sequential in
// the vertical (rrtmg_simple_physics.h), so the parallelism is the columns'.  8192 columns are 128 waves on 256 CUs: the kernel
// streams its arrays once per pass and is bound by the latency of one column's dependent chain in fp64 -- per layer an exp and
// two divisions in pass 1 (independent between layers but for the precipitation sum), the div -> mul -> sub -> div recurrence of
// CE with a pow and an exp beside it in pass 2, two pow on the chain of t in pass 3 -- not by bandwidth or flops.  The four
// profiles ride one sweep, which gives each step of the chain independent divisions to overlap.  Every loop is bounded by nlay
// and a thread keeps no array of its own; the two work slabs are [nlay][ncol], so the 64 lanes of a wave read and write one run.
__global__ void __launch_bounds__(64) simple_physics_kernel(SimplePhysicsCall a) {
  const long col = (long)blockIdx.x * 64 + threadIdx.x;
  if (col >= a.ncol) return;
  simple_physics_column(a, col);
}

}  // namespace rrtmg

using namespace rrtmg;

extern "C" int rrtmg_hip_simple_physics(rrtmg_ctx *ctx, const rrtmg_simple_physics *a) {
  int rc = column_head(ctx, kSimplePhysics, a);
  if (rc) return rc;
  if (a->do_pbl == 1 && a->do_surf_flux != 1)
    return ctx->fail(RRTMG_ERR_ARG, "simple_physics: do_pbl needs do_surf_flux (the mixing reads the surface diffusivities and the drag coefficient that only the "
                                    "surface step sets: the reference reads them unset, there is nothing to reproduce)");
  rc = column_required(ctx, kSimplePhysics, a);
  if (rc) return rc;
  const bool surf = a->do_surf_flux == 1;
  const bool need_ts = surf && a->use_ts_ext == 1, need_qsurf = surf && a->use_qsurf_ext == 1, need_lat = surf && a->use_ts_ext != 1 && a->test == 1;
  if (need_ts && !a->ts) return ctx->fail(RRTMG_ERR_ARG, "simple_physics: ts must be given with do_surf_flux and use_ts_ext");
  if (need_qsurf && !a->qsurf) return ctx->fail(RRTMG_ERR_ARG, "simple_physics: qsurf must be given with do_surf_flux and use_qsurf_ext");
  if (need_lat && !a->lat) return ctx->fail(RRTMG_ERR_ARG, "simple_physics: lat must be given with do_surf_flux, test 1 and no use_ts_ext (the internal surface temperature)");
  constexpr unsigned ts = column_bits(kSimplePhysics, {"ts"}), qsurf = column_bits(kSimplePhysics, {"qsurf"}), lat = column_bits(kSimplePhysics, {"lat"});
  const unsigned unread = (need_ts ? 0 : ts) | (need_qsurf ? 0 : qsurf) | (need_lat ? 0 : lat);
  const size_t n1 = (size_t)a->ncol, nl = (size_t)a->nlay * n1;
  SimplePhysicsCall c{};
  c.ncol = a->ncol; c.nlay = a->nlay;
  c.do_lsc = a->do_lsc; c.do_pbl = a->do_pbl; c.do_surf_flux = a->do_surf_flux; c.use_ts_ext = a->use_ts_ext; c.use_qsurf_ext = a->use_qsurf_ext;
  c.test = a->test; c.clamp_latent_heat_flux = a->clamp_latent_heat_flux;
  c.dt = a->dt; c.g = a->g; c.cpair = a->cpair; c.rair = a->rair; c.latvap = a->latvap; c.rh2o = a->rh2o; c.radius = a->radius; c.omega = a->omega;
  c.rhow = a->rhow; c.pbltop = a->pbltop; c.pblconst = a->pblconst; c.c_heat = a->c_heat; c.cd0 = a->cd0; c.cd1 = a->cd1; c.cm = a->cm;
  c.pressure_scale = a->pressure_scale; c.ps_scale = a->ps_scale;
  // host pointers: the inputs go up; the four profiles are written in place in their device copies
  return column_call(ctx, kSimplePhysics, a, c, unread, "sp.io", [&]() -> int {
    double *work = (double *)ctx->buf("sp.work", 2 * nl * sizeof(double));
    if (!work) return ctx->status;
    c.work_ce = work; c.work_cem = work + nl;
    return RRTMG_OK;
  }, [&] { return column_launch(ctx, simple_physics_kernel, n1, c); });
}
#endif
