// rrtmg_dry_adjust.hip -- the kernel of the dry convective adjustment (rrtmg_dry_adjust.h) and its C entry:
//   rrtmg_hip_dry_adjustment   climt DryConvectiveAdjustment (dry_convection/component.py): air temperature and specific humidity
//                              of every column after one downward sweep that mixes super-adiabatic runs of layers
#include "rrtmg_ctx.h"
#include "rrtmg_dry_adjust.h"

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

static bool dry_overlap(const void *p, size_t n, const void *q, size_t m) {
  return p && q && (uintptr_t)p < (uintptr_t)q + m && (uintptr_t)q < (uintptr_t)p + n;
}

}  // namespace rrtmg

using namespace rrtmg;

extern "C" int rrtmg_hip_dry_adjustment(rrtmg_ctx *ctx, const rrtmg_dry_adjust *a) {
  if (!ctx) return RRTMG_ERR_ARG;
  if (!a) return ctx->fail(RRTMG_ERR_ARG, "dry_adjustment: NULL argument struct");
  if (a->struct_size != sizeof(rrtmg_dry_adjust))
    return ctx->fail(RRTMG_ERR_ARG, "dry_adjustment: struct_size %u, this library's rrtmg_dry_adjust has %zu bytes", a->struct_size, sizeof(rrtmg_dry_adjust));
  if (a->ncol <= 0 || a->nlay <= 0) return ctx->fail(RRTMG_ERR_ARG, "dry_adjustment: ncol/nlay must be positive");
  if (a->memspace != 0 && a->memspace != 1) return ctx->fail(RRTMG_ERR_ARG, "dry_adjustment: memspace must be 0 (host) or 1 (device)");
  if (!a->t || !a->q || !a->pmid || !a->pint || !a->t_out || !a->q_out)
    return ctx->fail(RRTMG_ERR_ARG, "dry_adjustment: t, q, pmid, pint, t_out and q_out must be given");
  if (!(a->cpd > 0.0) || !(a->rd > 0.0) || !(a->pref > 0.0) || !(a->cvap >= 0.0) || !(a->rv >= 0.0))
    return ctx->fail(RRTMG_ERR_ARG, "dry_adjustment: cpd, rd and pref must be positive, cvap and rv not negative");
  // (sizes in bytes)
  const size_t n1 = (size_t)a->ncol, nl = (size_t)a->nlay * n1, bl = nl * sizeof(double), bl1 = (nl + n1) * sizeof(double);
  const struct { const void *p; size_t n; } in[] = {{a->t, bl}, {a->q, bl}, {a->pmid, bl}, {a->pint, bl1}};
  const struct { const void *p; size_t n; const void *may_be; const char *name; } out[] = {
      {a->t_out, bl, a->t, "t_out"}, {a->q_out, bl, a->q, "q_out"}, {a->mixed_top, n1 * sizeof(int32_t), nullptr, "mixed_top"}};
  for (size_t i = 0; i < sizeof out / sizeof out[0]; ++i) {
    for (const auto &e : in)
      if (dry_overlap(out[i].p, out[i].n, e.p, e.n) && !(out[i].may_be && out[i].p == out[i].may_be && e.p == out[i].may_be))
        return ctx->fail(RRTMG_ERR_ARG, "dry_adjustment: %s aliases an input%s", out[i].name, out[i].may_be ? " (in place: exactly its own input)" : "");
    for (size_t j = 0; j < i; ++j)
      if (dry_overlap(out[i].p, out[i].n, out[j].p, out[j].n)) return ctx->fail(RRTMG_ERR_ARG, "dry_adjustment: %s overlaps %s", out[i].name, out[j].name);
  }
  int rc = ctx_prepare_device(ctx);
  if (rc) return rc;
  hipStream_t s = ctx->stream;
  DryAdjustCall c{};
  c.ncol = a->ncol; c.nlay = a->nlay;
  c.cpd = a->cpd; c.cvap = a->cvap; c.rd = a->rd; c.rv = a->rv; c.pref = a->pref;
  double *work = (double *)ctx->buf("dry.work", 2 * bl);
  if (!work) return ctx->status;
  c.theta = work; c.dp = work + nl;
  if (a->memspace == 0) {
    // four arrays up; T and q are adjusted in place in their device copies
    double *io = (double *)ctx->buf("dry.io", 3 * bl + bl1);
    int32_t *top = (int32_t *)ctx->buf("dry.top", n1 * sizeof(int32_t));
    if (!io || !top) return ctx->status;
    RRTMG_HIP_CHECK(ctx, hipMemcpyAsync(io, a->t, bl, hipMemcpyHostToDevice, s));
    RRTMG_HIP_CHECK(ctx, hipMemcpyAsync(io + nl, a->q, bl, hipMemcpyHostToDevice, s));
    RRTMG_HIP_CHECK(ctx, hipMemcpyAsync(io + 2 * nl, a->pmid, bl, hipMemcpyHostToDevice, s));
    RRTMG_HIP_CHECK(ctx, hipMemcpyAsync(io + 3 * nl, a->pint, bl1, hipMemcpyHostToDevice, s));
    c.t = c.t_out = io; c.q = c.q_out = io + nl; c.pmid = io + 2 * nl; c.pint = io + 3 * nl;
    c.mixed_top = a->mixed_top ? top : nullptr;
  } else {
    c.t = a->t; c.q = a->q; c.pmid = a->pmid; c.pint = a->pint;
    c.t_out = a->t_out; c.q_out = a->q_out; c.mixed_top = a->mixed_top;
  }
  hipLaunchKernelGGL(dry_adjust_kernel, dim3((unsigned)((n1 + 63) / 64)), dim3(64), 0, s, c);
  RRTMG_HIP_CHECK(ctx, hipGetLastError());
  if (a->memspace == 0) {
    RRTMG_HIP_CHECK(ctx, hipMemcpyAsync(a->t_out, c.t_out, bl, hipMemcpyDeviceToHost, s));
    RRTMG_HIP_CHECK(ctx, hipMemcpyAsync(a->q_out, c.q_out, bl, hipMemcpyDeviceToHost, s));
    if (a->mixed_top) RRTMG_HIP_CHECK(ctx, hipMemcpyAsync(a->mixed_top, c.mixed_top, n1 * sizeof(int32_t), hipMemcpyDeviceToHost, s));
  }
  if (ctx->deferred && a->memspace == 1) return RRTMG_OK;
  RRTMG_HIP_CHECK(ctx, hipStreamSynchronize(s));
  return RRTMG_OK;
}
