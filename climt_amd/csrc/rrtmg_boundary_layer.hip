// rrtmg_boundary_layer.hip -- the kernel of the simple boundary layer (rrtmg_boundary_layer.h) and its C entry:
//   rrtmg_hip_boundary_layer   climt SimpleBoundaryLayer (simple_boundary_layer/component.py): bulk surface exchange and the implicit
//                              diffusion of temperature, humidity and the two winds through the boundary layer of every column
#include "rrtmg_column_call.h"
#include "rrtmg_boundary_layer.h"

namespace rrtmg {

// the arrays of rrtmg_boundary_layer (rrtmg_column_call.h); tools/column_call_check.cpp includes this file for the table alone
#define ROW(m) RRTMG_COLUMN_ROW(rrtmg_boundary_layer, BoundaryLayerCall, m)
constexpr ColumnRow kBoundaryLayerRows[] = {
    {ROW(t), ColumnExt::Lay, true}, {ROW(q), ColumnExt::Lay, true}, {ROW(u), ColumnExt::Lay, true}, {ROW(v), ColumnExt::Lay, true},
    {ROW(pmid), ColumnExt::Lay, true}, {ROW(pint), ColumnExt::Lev, true}, {ROW(ps), ColumnExt::Col, true}, {ROW(ts), ColumnExt::Col, true},
    {ROW(qs), ColumnExt::Col, true}, {ROW(sh_in), ColumnExt::Col, false}, {ROW(lh_in), ColumnExt::Col, false},   // read in mode 2 only
    {ROW(t_out), ColumnExt::Lay, true, "t"}, {ROW(q_out), ColumnExt::Lay, true, "q"}, {ROW(u_out), ColumnExt::Lay, true, "u"}, {ROW(v_out), ColumnExt::Lay, true, "v"},
    {ROW(stress_north), ColumnExt::Col, false}, {ROW(stress_east), ColumnExt::Col, false}, {ROW(height), ColumnExt::Col, false},
    {ROW(sh_out), ColumnExt::Col, false}, {ROW(lh_out), ColumnExt::Col, false}};
#undef ROW
constexpr ColumnTable kBoundaryLayer = column_table("boundary_layer", "rrtmg_boundary_layer", 2, "ncol must be positive",
    "nlay must be at least 2 (with one layer there is no interior interface: the reference indexes an empty array)",
    " (in place: exactly its own input)", kBoundaryLayerRows);

}  // namespace rrtmg

#ifdef __HIPCC__
namespace rrtmg {

// One thread per column, tiles of 64 columns: the hypsometric sum, the search for the top and the two sweeps of the Thomas solve
// are sequential in the vertical (rrtmg_boundary_layer.h), so the parallelism is the columns'.  8192 columns are 128 waves on 256
// CUs: the kernel is bound by the latency of one column's dependent chain -- per level a log and a pow in pass 1 and the
// div -> mul -> sub -> div recurrence of m and c' in pass 2, in fp64 -- not by bandwidth or flops.  The four right-hand sides ride
// one elimination, which gives each step of the chain four independent divisions to overlap.  Every loop is bounded by nlay and
// a thread keeps no array of its own; the two work slabs are [nlay-1][ncol], so the 64 lanes of a wave read and write one run.
__global__ void __launch_bounds__(64) boundary_layer_kernel(BoundaryLayerCall a) {
  const long col = (long)blockIdx.x * 64 + threadIdx.x;
  if (col >= a.ncol) return;
  boundary_layer_column(a, col);
}

}  // namespace rrtmg

using namespace rrtmg;

extern "C" int rrtmg_hip_boundary_layer(rrtmg_ctx *ctx, const rrtmg_boundary_layer *a) {
  int rc = column_head(ctx, kBoundaryLayer, a);
  if (rc) return rc;
  if (a->flux_mode < 0 || a->flux_mode > 2) return ctx->fail(RRTMG_ERR_ARG, "boundary_layer: flux_mode must be 0 (none), 1 (bulk) or 2 (external)");
  rc = column_required(ctx, kBoundaryLayer, a);
  if (rc) return rc;
  const bool external = a->flux_mode == 2;
  if (external && (!a->sh_in || !a->lh_in)) return ctx->fail(RRTMG_ERR_ARG, "boundary_layer: sh_in and lh_in must be given with flux_mode 2 (external)");
  const double positive[] = {a->dt, a->rd, a->cp, a->g, a->lv, a->karman, a->z0, a->fb, a->p0, a->ric, a->pressure_scale, a->ps_scale};
  for (double x : positive)
    if (!(x > 0.0)) return ctx->fail(RRTMG_ERR_ARG, "boundary_layer: dt, rd, cp, g, lv, karman, z0, fb, p0, ric, pressure_scale and ps_scale must be positive");
  if (!(a->fb < 1.0)) return ctx->fail(RRTMG_ERR_ARG, "boundary_layer: fb must lie inside (0, 1)");
  const size_t n1 = (size_t)a->ncol, nl = (size_t)a->nlay * n1;
  BoundaryLayerCall c{};
  c.ncol = a->ncol; c.nlay = a->nlay; c.flux_mode = a->flux_mode;
  c.dt = a->dt; c.rd = a->rd; c.cp = a->cp; c.g = a->g; c.lv = a->lv; c.karman = a->karman; c.z0 = a->z0; c.fb = a->fb; c.p0 = a->p0; c.ric = a->ric;
  c.pressure_scale = a->pressure_scale; c.ps_scale = a->ps_scale;
  // host pointers: the inputs go up; the four profiles are solved in place in their device copies
  constexpr unsigned fluxes_in = column_bits(kBoundaryLayer, {"sh_in", "lh_in"});
  return column_call(ctx, kBoundaryLayer, a, c, external ? 0 : fluxes_in, "bl.io", [&]() -> int {
    double *work = (double *)ctx->buf("bl.work", 2 * (nl - n1) * sizeof(double));
    if (!work) return ctx->status;
    c.work_z = work; c.work_rho = work + (nl - n1);
    return RRTMG_OK;
  }, [&] { return column_launch(ctx, boundary_layer_kernel, n1, c); });
}
#endif
