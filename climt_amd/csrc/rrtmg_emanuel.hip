// rrtmg_emanuel.hip -- the kernel of the Emanuel convection scheme (rrtmg_emanuel.h) and its C entry:
//   rrtmg_hip_emanuel_convection   climt EmanuelConvection (emanuel/component.py; the rule as emanuel/pure_python.py states it): the
//                                  convective tendencies of temperature, humidity and the two winds, and the precipitation, of every column
#include "rrtmg_ctx.h"
#include "rrtmg_emanuel.h"

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

static bool em_overlap(const void *p, size_t n, const void *q, size_t m) {
  return p && q && (uintptr_t)p < (uintptr_t)q + m && (uintptr_t)q < (uintptr_t)p + n;
}

}  // namespace rrtmg

using namespace rrtmg;

extern "C" int rrtmg_hip_emanuel_convection(rrtmg_ctx *ctx, const rrtmg_emanuel *a) {
  if (!ctx) return RRTMG_ERR_ARG;
  if (!a) return ctx->fail(RRTMG_ERR_ARG, "emanuel_convection: NULL argument struct");
  if (a->struct_size != sizeof(rrtmg_emanuel))
    return ctx->fail(RRTMG_ERR_ARG, "emanuel_convection: struct_size %u, this library's rrtmg_emanuel has %zu bytes", a->struct_size, sizeof(rrtmg_emanuel));
  if (a->ncol <= 0) return ctx->fail(RRTMG_ERR_ARG, "emanuel_convection: ncol must be positive");
  if (a->nlay < 4)
    return ctx->fail(RRTMG_ERR_ARG, "emanuel_convection: nlay must be at least 4 (NL = nlay - 3 >= 1: with fewer layers the reference's cap NL - 1 of the level of minimum moist static energy is not a level)");
  if (a->memspace != 0 && a->memspace != 1) return ctx->fail(RRTMG_ERR_ARG, "emanuel_convection: memspace must be 0 (host) or 1 (device)");
  if (!a->t || !a->q || !a->u || !a->v || !a->pmid || !a->pint || !a->cbmf || !a->ft || !a->fq || !a->fu || !a->fv || !a->cbmf_out)
    return ctx->fail(RRTMG_ERR_ARG, "emanuel_convection: t, q, u, v, pmid, pint, cbmf, ft, fq, fu, fv and cbmf_out must be given");
  const double positive[] = {a->dt, a->pressure_scale, a->cpd, a->rd, a->rv, a->g};
  for (double x : positive)
    if (!(x > 0.0)) return ctx->fail(RRTMG_ERR_ARG, "emanuel_convection: dt, pressure_scale, cpd, rd, rv and g must be positive");
  if (a->minorig < 1) return ctx->fail(RRTMG_ERR_ARG, "emanuel_convection: minorig must be at least 1 (the first model level)");
  if (!(a->cu >= 0.0 && a->cu <= 1.0)) return ctx->fail(RRTMG_ERR_ARG, "emanuel_convection: cu (momentum transfer coefficient) must be between 0 and 1");
  if (!(a->sigd >= 0.0 && a->sigd <= 1.0)) return ctx->fail(RRTMG_ERR_ARG, "emanuel_convection: sigd (downdraft fraction) must be between 0 and 1");
  if (!(a->sigs >= 0.0 && a->sigs <= 1.0)) return ctx->fail(RRTMG_ERR_ARG, "emanuel_convection: sigs (outside cloud precipitation fraction) must be between 0 and 1");
  // (sizes in bytes)
  const size_t n1 = (size_t)a->ncol, nl = (size_t)a->nlay * n1, b1 = n1 * sizeof(double), bl = nl * sizeof(double), bl1 = bl + b1, bi = n1 * sizeof(int32_t);
  const struct { const void *p; size_t n; } in[] = {{a->t, bl}, {a->q, bl}, {a->u, bl}, {a->v, bl}, {a->pmid, bl}, {a->pint, bl1}, {a->cbmf, b1}, {a->qs, bl}};
  const struct { const void *p; size_t n; const void *may_be; const char *name; } out[] = {
      {a->ft, bl, nullptr, "ft"}, {a->fq, bl, nullptr, "fq"}, {a->fu, bl, nullptr, "fu"}, {a->fv, bl, nullptr, "fv"},
      {a->precip, b1, nullptr, "precip"}, {a->wd, b1, nullptr, "wd"}, {a->tprime, b1, nullptr, "tprime"}, {a->qprime, b1, nullptr, "qprime"},
      {a->cape, b1, nullptr, "cape"}, {a->iflag, bi, nullptr, "iflag"}, {a->ft_per_day, bl, nullptr, "ft_per_day"}, {a->cbmf_out, b1, a->cbmf, "cbmf_out"}};
  for (size_t i = 0; i < sizeof out / sizeof out[0]; ++i) {
    for (const auto &e : in)
      if (em_overlap(out[i].p, out[i].n, e.p, e.n) && !(out[i].may_be && out[i].p == out[i].may_be && e.p == out[i].may_be))
        return ctx->fail(RRTMG_ERR_ARG, "emanuel_convection: %s aliases an input%s", out[i].name, out[i].may_be ? " (in place: exactly cbmf)" : "");
    for (size_t j = 0; j < i; ++j)
      if (em_overlap(out[i].p, out[i].n, out[j].p, out[j].n)) return ctx->fail(RRTMG_ERR_ARG, "emanuel_convection: %s overlaps %s", out[i].name, out[j].name);
  }
  int rc = ctx_prepare_device(ctx);
  if (rc) return rc;
  hipStream_t s = ctx->stream;
  EmanuelCall c{};
  c.ncol = a->ncol; c.nlay = a->nlay; c.minorig = a->minorig; c.dt = a->dt; c.pressure_scale = a->pressure_scale;
  c.elcrit = a->elcrit; c.tlcrit = a->tlcrit; c.entp = a->entp; c.sigd = a->sigd; c.sigs = a->sigs; c.omtrain = a->omtrain; c.omtsnow = a->omtsnow;
  c.coeffr = a->coeffr; c.coeffs = a->coeffs; c.cu = a->cu; c.beta = a->beta; c.dtmax = a->dtmax; c.alpha = a->alpha; c.damp = a->damp; c.delt0 = a->delt0;
  c.cpd = a->cpd; c.cpv = a->cpv; c.cl = a->cl; c.rv = a->rv; c.rd = a->rd; c.lv0 = a->lv0; c.g = a->g; c.rowl = a->rowl;
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
  const size_t ccol = ctile * 64 < n1 ? ctile * 64 : n1;
  double *work = (double *)ctx->buf("emanuel.work", ccol * per_col);
  if (!work) return ctx->status;
  c.w1 = work; c.w2 = work + emanuel_work1(a->nlay) * ccol;
  double *const host_col[5] = {a->precip, a->wd, a->tprime, a->qprime, a->cape};
  double *dev_col[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
  if (a->memspace == 0) {
    // t, q, u, v, pmid, pint, cbmf and (where given) qs go up; ft, fq, fu, fv, the scalars asked for and cbmf_out come back
    const size_t words = 12 * nl + n1 + 7 * n1 + (n1 + 1) / 2;
    double *io = (double *)ctx->buf("emanuel.io", words * sizeof(double));
    if (!io) return ctx->status;
    double *col1 = io + 12 * nl + n1;      // cbmf, cbmf_out, the five scalars, iflag
    const struct { double *d; const double *h; size_t n; } up[] = {{io, a->t, bl}, {io + nl, a->q, bl}, {io + 2 * nl, a->u, bl}, {io + 3 * nl, a->v, bl},
        {io + 4 * nl, a->pmid, bl}, {io + 5 * nl, a->pint, bl1}, {io + 6 * nl + n1, a->qs, bl}, {col1, a->cbmf, b1}};
    for (const auto &e : up)
      if (e.h) RRTMG_HIP_CHECK(ctx, hipMemcpyAsync(e.d, e.h, e.n, hipMemcpyHostToDevice, s));
    c.t = io; c.q = io + nl; c.u = io + 2 * nl; c.v = io + 3 * nl; c.pmid = io + 4 * nl; c.pint = io + 5 * nl;
    c.qs = a->qs ? io + 6 * nl + n1 : nullptr;
    double *o = io + 7 * nl + n1;
    c.ft = o; c.fq = o + nl; c.fu = o + 2 * nl; c.fv = o + 3 * nl;
    c.ft_per_day = a->ft_per_day ? o + 4 * nl : nullptr;
    c.cbmf = col1; c.cbmf_out = col1 + n1;
    for (int i = 0; i < 5; ++i) dev_col[i] = host_col[i] ? col1 + (2 + i) * n1 : nullptr;
    c.iflag = a->iflag ? (int32_t *)(col1 + 7 * n1) : nullptr;
  } else {
    c.t = a->t; c.q = a->q; c.u = a->u; c.v = a->v; c.pmid = a->pmid; c.pint = a->pint; c.cbmf = a->cbmf; c.qs = a->qs;
    c.ft = a->ft; c.fq = a->fq; c.fu = a->fu; c.fv = a->fv; c.ft_per_day = a->ft_per_day; c.cbmf_out = a->cbmf_out; c.iflag = a->iflag;
    for (int i = 0; i < 5; ++i) dev_col[i] = host_col[i];
  }
  c.precip = dev_col[0]; c.wd = dev_col[1]; c.tprime = dev_col[2]; c.qprime = dev_col[3]; c.cape = dev_col[4];
  for (size_t c0 = 0; c0 < n1; c0 += ccol) {
    const size_t cols = n1 - c0 < ccol ? n1 - c0 : ccol;
    c.col0 = (int64_t)c0; c.ccol = (int32_t)ccol;
    hipLaunchKernelGGL(emanuel_kernel, dim3((unsigned)((cols + 63) / 64)), dim3(64), 0, s, c);
    RRTMG_HIP_CHECK(ctx, hipGetLastError());
  }
  if (a->memspace == 0) {
    RRTMG_HIP_CHECK(ctx, hipMemcpyAsync(a->ft, c.ft, bl, hipMemcpyDeviceToHost, s));
    RRTMG_HIP_CHECK(ctx, hipMemcpyAsync(a->fq, c.fq, bl, hipMemcpyDeviceToHost, s));
    RRTMG_HIP_CHECK(ctx, hipMemcpyAsync(a->fu, c.fu, bl, hipMemcpyDeviceToHost, s));
    RRTMG_HIP_CHECK(ctx, hipMemcpyAsync(a->fv, c.fv, bl, hipMemcpyDeviceToHost, s));
    if (a->ft_per_day) RRTMG_HIP_CHECK(ctx, hipMemcpyAsync(a->ft_per_day, c.ft_per_day, bl, hipMemcpyDeviceToHost, s));
    RRTMG_HIP_CHECK(ctx, hipMemcpyAsync(a->cbmf_out, c.cbmf_out, b1, hipMemcpyDeviceToHost, s));
    for (int i = 0; i < 5; ++i)
      if (host_col[i]) RRTMG_HIP_CHECK(ctx, hipMemcpyAsync(host_col[i], dev_col[i], b1, hipMemcpyDeviceToHost, s));
    if (a->iflag) RRTMG_HIP_CHECK(ctx, hipMemcpyAsync(a->iflag, c.iflag, bi, hipMemcpyDeviceToHost, s));
  }
  if (ctx->deferred && a->memspace == 1) return RRTMG_OK;
  RRTMG_HIP_CHECK(ctx, hipStreamSynchronize(s));
  return RRTMG_OK;
}
