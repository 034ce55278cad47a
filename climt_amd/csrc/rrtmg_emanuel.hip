// rrtmg_emanuel.hip -- the kernel of the Emanuel convection scheme (rrtmg_emanuel.h) and its C entry:
//   rrtmg_hip_emanuel_convection   climt EmanuelConvection (emanuel/component.py; the rule as emanuel/pure_python.py states it): the
//                                  convective tendencies of temperature, humidity and the two winds, and the precipitation, of every column
#include "rrtmg_column_call.h"
#include "rrtmg_emanuel.h"

namespace rrtmg {

// the arrays of rrtmg_emanuel (rrtmg_column_call.h); tools/column_call_check.cpp includes this file for the table alone
#define ROW(m) RRTMG_COLUMN_ROW(rrtmg_emanuel, EmanuelCall, m)
constexpr ColumnRow kEmanuelRows[] = {
    {ROW(t), ColumnExt::Lay, true}, {ROW(q), ColumnExt::Lay, true}, {ROW(u), ColumnExt::Lay, true}, {ROW(v), ColumnExt::Lay, true},
    {ROW(pmid), ColumnExt::Lay, true}, {ROW(pint), ColumnExt::Lev, true}, {ROW(cbmf), ColumnExt::Col, true},
    {ROW(qs), ColumnExt::Lay, false},   // read where given: else the kernel forms it
    {ROW(ft), ColumnExt::Lay, true}, {ROW(fq), ColumnExt::Lay, true}, {ROW(fu), ColumnExt::Lay, true}, {ROW(fv), ColumnExt::Lay, true},
    {ROW(precip), ColumnExt::Col, false}, {ROW(wd), ColumnExt::Col, false}, {ROW(tprime), ColumnExt::Col, false}, {ROW(qprime), ColumnExt::Col, false},
    {ROW(cape), ColumnExt::Col, false}, {ROW(iflag), ColumnExt::Col, false}, {ROW(ft_per_day), ColumnExt::Lay, false}, {ROW(cbmf_out), ColumnExt::Col, true, "cbmf"}};
#undef ROW
constexpr ColumnTable kEmanuel = column_table("emanuel_convection", "rrtmg_emanuel", 4, "ncol must be positive",
    "nlay must be at least 4 (NL = nlay - 3 >= 1: with fewer layers the reference's cap NL - 1 of the level of minimum moist static energy is not a level)",
    " (in place: exactly cbmf)", kEmanuelRows);

}  // namespace rrtmg

#ifdef __HIPCC__
namespace rrtmg {

// One thread per column, tiles of 64 columns: lifting, the mixing spectrum, the downdraft and the tendencies are chains of decisions
// in the vertical (rrtmg_emanuel.h), so the parallelism is the columns'.  A convecting column walks the (INB - ICB)^2 block of its six
// 2-D slabs about four times (first mixing loop, normalisation, the downdraft's WDTRAIN, the tendencies' AMP1 / AD / entrainment sums);
// a column that leaves by an early exit costs one pass over its levels.  A wave takes as long as its deepest column; the slabs are
// [..][ccol] with the column fastest, so the lanes of a wave that are at the same (i, j) touch one run of 512 bytes.  Every loop
// is bounded by nlay and a thread keeps no array of its own.
__global__ void __launch_bounds__(64) emanuel_kernel(EmanuelCall a) {
  const long col = a.col0 + (long)blockIdx.x * 64 + threadIdx.x;
  if (col >= a.col0 + a.ccol || col >= a.ncol) return;
  emanuel_column(a, col);
}

}  // namespace rrtmg

using namespace rrtmg;

extern "C" int rrtmg_hip_emanuel_convection(rrtmg_ctx *ctx, const rrtmg_emanuel *a) {
  int rc = column_head(ctx, kEmanuel, a);
  if (!rc) rc = column_required(ctx, kEmanuel, a);
  if (rc) return rc;
  const double positive[] = {a->dt, a->pressure_scale, a->cpd, a->rd, a->rv, a->g};
  for (double x : positive)
    if (!(x > 0.0)) return ctx->fail(RRTMG_ERR_ARG, "emanuel_convection: dt, pressure_scale, cpd, rd, rv and g must be positive");
  if (a->minorig < 1) return ctx->fail(RRTMG_ERR_ARG, "emanuel_convection: minorig must be at least 1 (the first model level)");
  if (!(a->cu >= 0.0 && a->cu <= 1.0)) return ctx->fail(RRTMG_ERR_ARG, "emanuel_convection: cu (momentum transfer coefficient) must be between 0 and 1");
  if (!(a->sigd >= 0.0 && a->sigd <= 1.0)) return ctx->fail(RRTMG_ERR_ARG, "emanuel_convection: sigd (downdraft fraction) must be between 0 and 1");
  if (!(a->sigs >= 0.0 && a->sigs <= 1.0)) return ctx->fail(RRTMG_ERR_ARG, "emanuel_convection: sigs (outside cloud precipitation fraction) must be between 0 and 1");
  EmanuelCall c{};
  c.ncol = a->ncol; c.nlay = a->nlay; c.minorig = a->minorig; c.dt = a->dt; c.pressure_scale = a->pressure_scale;
  c.elcrit = a->elcrit; c.tlcrit = a->tlcrit; c.entp = a->entp; c.sigd = a->sigd; c.sigs = a->sigs; c.omtrain = a->omtrain; c.omtsnow = a->omtsnow;
  c.coeffr = a->coeffr; c.coeffs = a->coeffs; c.cu = a->cu; c.beta = a->beta; c.dtmax = a->dtmax; c.alpha = a->alpha; c.damp = a->damp; c.delt0 = a->delt0;
  c.cpd = a->cpd; c.cpv = a->cpv; c.cl = a->cl; c.rv = a->rv; c.rd = a->rd; c.lv0 = a->lv0; c.g = a->g; c.rowl = a->rowl;
  // host pointers: t, q, u, v, pmid, pint, cbmf and (where given) qs go up; ft, fq, fu, fv, the scalars asked for and cbmf_out come back
  const size_t n1 = (size_t)a->ncol;
  size_t ccol = 0;
  return column_call(ctx, kEmanuel, a, c, 0, "emanuel.io", [&]() -> int {
    // work space: per column 8 (kEmanuelSlabs1 (nlay + 1) + 6 (nlay - 4) (nlay - 3)) bytes, sized per chunk of whole 64-column tiles
    // against the context's scratch budget (RRTMG_HIP_MAX_SCRATCH_BYTES, default an eighth of the device's memory; a given
    // RRTMG_HIP_CHUNK_TILES caps the chunk as well): one launch per chunk, all on the main stream, the slabs re-used
    const size_t per_col = (emanuel_work1(a->nlay) + emanuel_work2(a->nlay)) * sizeof(double), per_tile = 64 * per_col;
    const size_t ntile = (n1 + 63) / 64;
    const size_t budget = ctx->max_scratch_bytes ? ctx->max_scratch_bytes : ctx->device_mem / 8;
    size_t ctile = budget / per_tile;
    if (!ctx->chunk_auto && ctile > (size_t)ctx->chunk_tiles) ctile = (size_t)ctx->chunk_tiles;
    if (ctile < 1) ctile = 1;
    if (ctile > ntile) ctile = ntile;
    ccol = ctile * 64 < n1 ? ctile * 64 : n1;
    double *work = (double *)ctx->buf("emanuel.work", ccol * per_col);
    if (!work) return ctx->status;
    c.w1 = work; c.w2 = work + emanuel_work1(a->nlay) * ccol;
    return RRTMG_OK;
  }, [&]() -> int {
    for (size_t c0 = 0; c0 < n1; c0 += ccol) {
      c.col0 = (int64_t)c0; c.ccol = (int32_t)ccol;
      const int err = column_launch(ctx, emanuel_kernel, n1 - c0 < ccol ? n1 - c0 : ccol, c);
      if (err) return err;
    }
    return RRTMG_OK;
  });
}
#endif
