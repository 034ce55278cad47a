// rrtmg_boundary_layer.hip -- the kernel of the simple boundary layer (rrtmg_boundary_layer.h) and its C entry:
//   rrtmg_hip_boundary_layer   climt SimpleBoundaryLayer (simple_boundary_layer/component.py): bulk surface exchange and the implicit
//                              diffusion of temperature, humidity and the two winds through the boundary layer of every column
#include "rrtmg_ctx.h"
#include "rrtmg_boundary_layer.h"

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

static bool bl_overlap(const void *p, size_t n, const void *q, size_t m) {
  return p && q && (uintptr_t)p < (uintptr_t)q + m && (uintptr_t)q < (uintptr_t)p + n;
}

}  // namespace rrtmg

using namespace rrtmg;

extern "C" int rrtmg_hip_boundary_layer(rrtmg_ctx *ctx, const rrtmg_boundary_layer *a) {
  if (!ctx) return RRTMG_ERR_ARG;
  if (!a) return ctx->fail(RRTMG_ERR_ARG, "boundary_layer: NULL argument struct");
  if (a->struct_size != sizeof(rrtmg_boundary_layer))
    return ctx->fail(RRTMG_ERR_ARG, "boundary_layer: struct_size %u, this library's rrtmg_boundary_layer has %zu bytes", a->struct_size, sizeof(rrtmg_boundary_layer));
  if (a->ncol <= 0) return ctx->fail(RRTMG_ERR_ARG, "boundary_layer: ncol must be positive");
  if (a->nlay < 2)
    return ctx->fail(RRTMG_ERR_ARG, "boundary_layer: nlay must be at least 2 (with one layer there is no interior interface: the reference indexes an empty array)");
  if (a->memspace != 0 && a->memspace != 1) return ctx->fail(RRTMG_ERR_ARG, "boundary_layer: memspace must be 0 (host) or 1 (device)");
  if (a->flux_mode < 0 || a->flux_mode > 2) return ctx->fail(RRTMG_ERR_ARG, "boundary_layer: flux_mode must be 0 (none), 1 (bulk) or 2 (external)");
  if (!a->t || !a->q || !a->u || !a->v || !a->pmid || !a->pint || !a->ps || !a->ts || !a->qs || !a->t_out || !a->q_out || !a->u_out || !a->v_out)
    return ctx->fail(RRTMG_ERR_ARG, "boundary_layer: t, q, u, v, pmid, pint, ps, ts, qs, t_out, q_out, u_out and v_out must be given");
  const bool external = a->flux_mode == 2;
  if (external && (!a->sh_in || !a->lh_in)) return ctx->fail(RRTMG_ERR_ARG, "boundary_layer: sh_in and lh_in must be given with flux_mode 2 (external)");
  const double positive[] = {a->dt, a->rd, a->cp, a->g, a->lv, a->karman, a->z0, a->fb, a->p0, a->ric, a->pressure_scale, a->ps_scale};
  for (double x : positive)
    if (!(x > 0.0)) return ctx->fail(RRTMG_ERR_ARG, "boundary_layer: dt, rd, cp, g, lv, karman, z0, fb, p0, ric, pressure_scale and ps_scale must be positive");
  if (!(a->fb < 1.0)) return ctx->fail(RRTMG_ERR_ARG, "boundary_layer: fb must lie inside (0, 1)");
  // (sizes in bytes)
  const size_t n1 = (size_t)a->ncol, nl = (size_t)a->nlay * n1, b1 = n1 * sizeof(double), bl = nl * sizeof(double), bl1 = bl + b1;
  const struct { const void *p; size_t n; } in[] = {{a->t, bl}, {a->q, bl}, {a->u, bl}, {a->v, bl}, {a->pmid, bl}, {a->pint, bl1}, {a->ps, b1}, {a->ts, b1}, {a->qs, b1},
                                                    {external ? a->sh_in : nullptr, b1}, {external ? a->lh_in : nullptr, b1}};
  const struct { const void *p; size_t n; const void *may_be; const char *name; } out[] = {
      {a->t_out, bl, a->t, "t_out"}, {a->q_out, bl, a->q, "q_out"}, {a->u_out, bl, a->u, "u_out"}, {a->v_out, bl, a->v, "v_out"},
      {a->stress_north, b1, nullptr, "stress_north"}, {a->stress_east, b1, nullptr, "stress_east"}, {a->height, b1, nullptr, "height"},
      {a->sh_out, b1, nullptr, "sh_out"}, {a->lh_out, b1, nullptr, "lh_out"}};
  for (size_t i = 0; i < sizeof out / sizeof out[0]; ++i) {
    for (const auto &e : in)
      if (bl_overlap(out[i].p, out[i].n, e.p, e.n) && !(out[i].may_be && out[i].p == out[i].may_be && e.p == out[i].may_be))
        return ctx->fail(RRTMG_ERR_ARG, "boundary_layer: %s aliases an input%s", out[i].name, out[i].may_be ? " (in place: exactly its own input)" : "");
    for (size_t j = 0; j < i; ++j)
      if (bl_overlap(out[i].p, out[i].n, out[j].p, out[j].n)) return ctx->fail(RRTMG_ERR_ARG, "boundary_layer: %s overlaps %s", out[i].name, out[j].name);
  }
  int rc = ctx_prepare_device(ctx);
  if (rc) return rc;
  hipStream_t s = ctx->stream;
  BoundaryLayerCall c{};
  c.ncol = a->ncol; c.nlay = a->nlay; c.flux_mode = a->flux_mode;
  c.dt = a->dt; c.rd = a->rd; c.cp = a->cp; c.g = a->g; c.lv = a->lv; c.karman = a->karman; c.z0 = a->z0; c.fb = a->fb; c.p0 = a->p0; c.ric = a->ric;
  c.pressure_scale = a->pressure_scale; c.ps_scale = a->ps_scale;
  double *work = (double *)ctx->buf("bl.work", 2 * (bl - b1));
  if (!work) return ctx->status;
  c.work_z = work; c.work_rho = work + (nl - n1);
  double *const host_diag[5] = {a->stress_north, a->stress_east, a->height, a->sh_out, a->lh_out};
  double *dev_diag[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
  if (a->memspace == 0) {
    // the inputs go up; the four profiles are solved in place in their device copies
    double *io = (double *)ctx->buf("bl.io", 5 * bl + bl1 + 10 * b1);
    if (!io) return ctx->status;
    double *col1 = io + 6 * nl + n1;      // ps, ts, qs, sh_in, lh_in, then the five diagnostics
    const struct { double *d; const double *h; size_t n; } up[] = {{io, a->t, bl}, {io + nl, a->q, bl}, {io + 2 * nl, a->u, bl}, {io + 3 * nl, a->v, bl},
        {io + 4 * nl, a->pmid, bl}, {io + 5 * nl, a->pint, bl1}, {col1, a->ps, b1}, {col1 + n1, a->ts, b1}, {col1 + 2 * n1, a->qs, b1},
        {col1 + 3 * n1, external ? a->sh_in : nullptr, b1}, {col1 + 4 * n1, external ? a->lh_in : nullptr, b1}};
    for (const auto &e : up)
      if (e.h) RRTMG_HIP_CHECK(ctx, hipMemcpyAsync(e.d, e.h, e.n, hipMemcpyHostToDevice, s));
    c.t = c.t_out = io; c.q = c.q_out = io + nl; c.u = c.u_out = io + 2 * nl; c.v = c.v_out = io + 3 * nl;
    c.pmid = io + 4 * nl; c.pint = io + 5 * nl; c.ps = col1; c.ts = col1 + n1; c.qs = col1 + 2 * n1;
    c.sh_in = external ? col1 + 3 * n1 : nullptr; c.lh_in = external ? col1 + 4 * n1 : nullptr;
    for (int i = 0; i < 5; ++i) dev_diag[i] = host_diag[i] ? col1 + (5 + i) * n1 : nullptr;
  } else {
    c.t = a->t; c.q = a->q; c.u = a->u; c.v = a->v; c.pmid = a->pmid; c.pint = a->pint; c.ps = a->ps; c.ts = a->ts; c.qs = a->qs;
    c.sh_in = external ? a->sh_in : nullptr; c.lh_in = external ? a->lh_in : nullptr;
    c.t_out = a->t_out; c.q_out = a->q_out; c.u_out = a->u_out; c.v_out = a->v_out;
    for (int i = 0; i < 5; ++i) dev_diag[i] = host_diag[i];
  }
  c.stress_north = dev_diag[0]; c.stress_east = dev_diag[1]; c.height = dev_diag[2]; c.sh_out = dev_diag[3]; c.lh_out = dev_diag[4];
  hipLaunchKernelGGL(boundary_layer_kernel, dim3((unsigned)((n1 + 63) / 64)), dim3(64), 0, s, c);
  RRTMG_HIP_CHECK(ctx, hipGetLastError());
  if (a->memspace == 0) {
    RRTMG_HIP_CHECK(ctx, hipMemcpyAsync(a->t_out, c.t_out, bl, hipMemcpyDeviceToHost, s));
    RRTMG_HIP_CHECK(ctx, hipMemcpyAsync(a->q_out, c.q_out, bl, hipMemcpyDeviceToHost, s));
    RRTMG_HIP_CHECK(ctx, hipMemcpyAsync(a->u_out, c.u_out, bl, hipMemcpyDeviceToHost, s));
    RRTMG_HIP_CHECK(ctx, hipMemcpyAsync(a->v_out, c.v_out, bl, hipMemcpyDeviceToHost, s));
    for (int i = 0; i < 5; ++i)
      if (host_diag[i]) RRTMG_HIP_CHECK(ctx, hipMemcpyAsync(host_diag[i], dev_diag[i], b1, hipMemcpyDeviceToHost, s));
  }
  if (ctx->deferred && a->memspace == 1) return RRTMG_OK;
  RRTMG_HIP_CHECK(ctx, hipStreamSynchronize(s));
  return RRTMG_OK;
}
