// rrtmg_dry_adjust.hip -- the kernel of the dry convective adjustment (rrtmg_dry_adjust.h) and its C entry:
//   rrtmg_hip_dry_adjustment   climt DryConvectiveAdjustment (dry_convection/component.py): air temperature and specific humidity
//                              of every column after one downward sweep that mixes super-adiabatic runs of layers
#include "rrtmg_column_call.h"
#include "rrtmg_dry_adjust.h"

namespace rrtmg {

// the arrays of rrtmg_dry_adjust (rrtmg_column_call.h); tools/column_call_check.cpp includes this file for the table alone
#define ROW(m) RRTMG_COLUMN_ROW(rrtmg_dry_adjust, DryAdjustCall, m)
constexpr ColumnRow kDryAdjustRows[] = {
    {ROW(t), ColumnExt::Lay, true}, {ROW(q), ColumnExt::Lay, true}, {ROW(pmid), ColumnExt::Lay, true}, {ROW(pint), ColumnExt::Lev, true},
    {ROW(t_out), ColumnExt::Lay, true, "t"}, {ROW(q_out), ColumnExt::Lay, true, "q"}, {ROW(mixed_top), ColumnExt::Col, false}};
#undef ROW
constexpr ColumnTable kDryAdjust = column_table("dry_adjustment", "rrtmg_dry_adjust", 1, "ncol/nlay must be positive", "ncol/nlay must be positive",
                                                " (in place: exactly its own input)", kDryAdjustRows);

}  // namespace rrtmg

#ifdef __HIPCC__
namespace rrtmg {

// One thread per column, tiles of 64 columns: the sweep of a column is sequential (rrtmg_dry_adjust.h: the order of its sums
// decides which layers mix), so the parallelism is the columns'.  8192 columns are 128 waves on 256 CUs: the kernel is bound by
// the latency of one column's chain of loads, divisions and pow, not by bandwidth or by flops.  Every loop is bounded by nlay
// and a thread keeps no array of its own; the work slabs are [nlay][ncol], so the 64 lanes of a wave read and write one run.
__global__ void __launch_bounds__(64) dry_adjust_kernel(DryAdjustCall a) {
  const long col = (long)blockIdx.x * 64 + threadIdx.x;
  if (col >= a.ncol) return;
  dry_adjust_column(a, col);
}

}  // namespace rrtmg

using namespace rrtmg;

extern "C" int rrtmg_hip_dry_adjustment(rrtmg_ctx *ctx, const rrtmg_dry_adjust *a) {
  int rc = column_head(ctx, kDryAdjust, a);
  if (!rc) rc = column_required(ctx, kDryAdjust, a);
  if (rc) return rc;
  if (!(a->cpd > 0.0) || !(a->rd > 0.0) || !(a->pref > 0.0) || !(a->cvap >= 0.0) || !(a->rv >= 0.0))
    return ctx->fail(RRTMG_ERR_ARG, "dry_adjustment: cpd, rd and pref must be positive, cvap and rv not negative");
  const size_t n1 = (size_t)a->ncol, nl = (size_t)a->nlay * n1;
  DryAdjustCall c{};
  c.ncol = a->ncol; c.nlay = a->nlay;
  c.cpd = a->cpd; c.cvap = a->cvap; c.rd = a->rd; c.rv = a->rv; c.pref = a->pref;
  // host pointers: four arrays up; T and q are adjusted in place in their device copies
  return column_call(ctx, kDryAdjust, a, c, 0, "dry.io", [&]() -> int {
    double *work = (double *)ctx->buf("dry.work", 2 * nl * sizeof(double));
    if (!work) return ctx->status;
    c.theta = work; c.dp = work + nl;
    return RRTMG_OK;
  }, [&] { return column_launch(ctx, dry_adjust_kernel, n1, c); });
}
#endif
