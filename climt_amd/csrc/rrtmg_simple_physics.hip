// rrtmg_simple_physics.hip -- the kernel of the simple physics package (rrtmg_simple_physics.h) and its C entry:
//   rrtmg_hip_simple_physics   climt SimplePhysics (simple_physics/component.py around simple_physics_custom.f90): large-scale
//                              condensation, surface fluxes on the lowest layer and the implicit boundary-layer mixing of
//                              temperature, humidity and the two winds of every column
#include "rrtmg_ctx.h"
#include "rrtmg_simple_physics.h"

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

static bool sp_overlap(const void *p, size_t n, const void *q, size_t m) {
  return p && q && (uintptr_t)p < (uintptr_t)q + m && (uintptr_t)q < (uintptr_t)p + n;
}

}  // namespace rrtmg

using namespace rrtmg;

extern "C" int rrtmg_hip_simple_physics(rrtmg_ctx *ctx, const rrtmg_simple_physics *a) {
  if (!ctx) return RRTMG_ERR_ARG;
  if (!a) return ctx->fail(RRTMG_ERR_ARG, "simple_physics: NULL argument struct");
  if (a->struct_size != sizeof(rrtmg_simple_physics))
    return ctx->fail(RRTMG_ERR_ARG, "simple_physics: struct_size %u, this library's rrtmg_simple_physics has %zu bytes", a->struct_size, sizeof(rrtmg_simple_physics));
  if (a->ncol <= 0) return ctx->fail(RRTMG_ERR_ARG, "simple_physics: ncol must be positive");
  if (a->nlay < 1) return ctx->fail(RRTMG_ERR_ARG, "simple_physics: nlay must be at least 1");
  if (a->memspace != 0 && a->memspace != 1) return ctx->fail(RRTMG_ERR_ARG, "simple_physics: memspace must be 0 (host) or 1 (device)");
  if (a->do_pbl == 1 && a->do_surf_flux != 1)
    return ctx->fail(RRTMG_ERR_ARG, "simple_physics: do_pbl needs do_surf_flux (the mixing reads the surface diffusivities and the drag coefficient that only the "
                                    "surface step sets: the reference reads them unset, there is nothing to reproduce)");
  if (!a->t || !a->q || !a->u || !a->v || !a->pmid || !a->pint || !a->ps || !a->t_out || !a->q_out || !a->u_out || !a->v_out)
    return ctx->fail(RRTMG_ERR_ARG, "simple_physics: t, q, u, v, pmid, pint, ps, t_out, q_out, u_out and v_out must be given");
  const bool surf = a->do_surf_flux == 1;
  const bool need_ts = surf && a->use_ts_ext == 1, need_qsurf = surf && a->use_qsurf_ext == 1, need_lat = surf && a->use_ts_ext != 1 && a->test == 1;
  if (need_ts && !a->ts) return ctx->fail(RRTMG_ERR_ARG, "simple_physics: ts must be given with do_surf_flux and use_ts_ext");
  if (need_qsurf && !a->qsurf) return ctx->fail(RRTMG_ERR_ARG, "simple_physics: qsurf must be given with do_surf_flux and use_qsurf_ext");
  if (need_lat && !a->lat) return ctx->fail(RRTMG_ERR_ARG, "simple_physics: lat must be given with do_surf_flux, test 1 and no use_ts_ext (the internal surface temperature)");
  // (sizes in bytes)
  const size_t n1 = (size_t)a->ncol, nl = (size_t)a->nlay * n1, b1 = n1 * sizeof(double), bl = nl * sizeof(double), bl1 = bl + b1;
  const double *const ts = need_ts ? a->ts : nullptr, *const qsurf = need_qsurf ? a->qsurf : nullptr, *const lat = need_lat ? a->lat : nullptr;
  const struct { const void *p; size_t n; } in[] = {{a->t, bl}, {a->q, bl}, {a->u, bl}, {a->v, bl}, {a->pmid, bl}, {a->pint, bl1}, {a->ps, b1}, {ts, b1}, {qsurf, b1}, {lat, b1}};
  const struct { const void *p; size_t n; const void *may_be; const char *name; } out[] = {
      {a->t_out, bl, a->t, "t_out"}, {a->q_out, bl, a->q, "q_out"}, {a->u_out, bl, a->u, "u_out"}, {a->v_out, bl, a->v, "v_out"},
      {a->precl, b1, nullptr, "precl"}, {a->sh_out, b1, nullptr, "sh_out"}, {a->lh_out, b1, nullptr, "lh_out"}};
  for (size_t i = 0; i < sizeof out / sizeof out[0]; ++i) {
    for (const auto &e : in)
      if (sp_overlap(out[i].p, out[i].n, e.p, e.n) && !(out[i].may_be && out[i].p == out[i].may_be && e.p == out[i].may_be))
        return ctx->fail(RRTMG_ERR_ARG, "simple_physics: %s aliases an input%s", out[i].name, out[i].may_be ? " (in place: exactly its own input)" : "");
    for (size_t j = 0; j < i; ++j)
      if (sp_overlap(out[i].p, out[i].n, out[j].p, out[j].n)) return ctx->fail(RRTMG_ERR_ARG, "simple_physics: %s overlaps %s", out[i].name, out[j].name);
  }
  int rc = ctx_prepare_device(ctx);
  if (rc) return rc;
  hipStream_t s = ctx->stream;
  SimplePhysicsCall c{};
  c.ncol = a->ncol; c.nlay = a->nlay;
  c.do_lsc = a->do_lsc; c.do_pbl = a->do_pbl; c.do_surf_flux = a->do_surf_flux; c.use_ts_ext = a->use_ts_ext; c.use_qsurf_ext = a->use_qsurf_ext;
  c.test = a->test; c.clamp_latent_heat_flux = a->clamp_latent_heat_flux;
  c.dt = a->dt; c.g = a->g; c.cpair = a->cpair; c.rair = a->rair; c.latvap = a->latvap; c.rh2o = a->rh2o; c.radius = a->radius; c.omega = a->omega;
  c.rhow = a->rhow; c.pbltop = a->pbltop; c.pblconst = a->pblconst; c.c_heat = a->c_heat; c.cd0 = a->cd0; c.cd1 = a->cd1; c.cm = a->cm;
  c.pressure_scale = a->pressure_scale; c.ps_scale = a->ps_scale;
  double *work = (double *)ctx->buf("sp.work", 2 * bl);
  if (!work) return ctx->status;
  c.work_ce = work; c.work_cem = work + nl;
  double *const host_diag[3] = {a->precl, a->sh_out, a->lh_out};
  double *dev_diag[3] = {nullptr, nullptr, nullptr};
  if (a->memspace == 0) {
    // the inputs go up; the four profiles are written in place in their device copies
    double *io = (double *)ctx->buf("sp.io", 5 * bl + bl1 + 7 * b1);
    if (!io) return ctx->status;
    double *col1 = io + 6 * nl + n1;      // ps, ts, qsurf, lat, then the three diagnostics
    const struct { double *d; const double *h; size_t n; } up[] = {{io, a->t, bl}, {io + nl, a->q, bl}, {io + 2 * nl, a->u, bl}, {io + 3 * nl, a->v, bl},
        {io + 4 * nl, a->pmid, bl}, {io + 5 * nl, a->pint, bl1}, {col1, a->ps, b1}, {col1 + n1, ts, b1}, {col1 + 2 * n1, qsurf, b1}, {col1 + 3 * n1, lat, b1}};
    for (const auto &e : up)
      if (e.h) RRTMG_HIP_CHECK(ctx, hipMemcpyAsync(e.d, e.h, e.n, hipMemcpyHostToDevice, s));
    c.t = c.t_out = io; c.q = c.q_out = io + nl; c.u = c.u_out = io + 2 * nl; c.v = c.v_out = io + 3 * nl;
    c.pmid = io + 4 * nl; c.pint = io + 5 * nl; c.ps = col1;
    c.ts = ts ? col1 + n1 : nullptr; c.qsurf = qsurf ? col1 + 2 * n1 : nullptr; c.lat = lat ? col1 + 3 * n1 : nullptr;
    for (int i = 0; i < 3; ++i) dev_diag[i] = host_diag[i] ? col1 + (4 + i) * n1 : nullptr;
  } else {
    c.t = a->t; c.q = a->q; c.u = a->u; c.v = a->v; c.pmid = a->pmid; c.pint = a->pint; c.ps = a->ps; c.ts = ts; c.qsurf = qsurf; c.lat = lat;
    c.t_out = a->t_out; c.q_out = a->q_out; c.u_out = a->u_out; c.v_out = a->v_out;
    for (int i = 0; i < 3; ++i) dev_diag[i] = host_diag[i];
  }
  c.precl = dev_diag[0]; c.sh_out = dev_diag[1]; c.lh_out = dev_diag[2];
  hipLaunchKernelGGL(simple_physics_kernel, dim3((unsigned)((n1 + 63) / 64)), dim3(64), 0, s, c);
  RRTMG_HIP_CHECK(ctx, hipGetLastError());
  if (a->memspace == 0) {
    RRTMG_HIP_CHECK(ctx, hipMemcpyAsync(a->t_out, c.t_out, bl, hipMemcpyDeviceToHost, s));
    RRTMG_HIP_CHECK(ctx, hipMemcpyAsync(a->q_out, c.q_out, bl, hipMemcpyDeviceToHost, s));
    RRTMG_HIP_CHECK(ctx, hipMemcpyAsync(a->u_out, c.u_out, bl, hipMemcpyDeviceToHost, s));
    RRTMG_HIP_CHECK(ctx, hipMemcpyAsync(a->v_out, c.v_out, bl, hipMemcpyDeviceToHost, s));
    for (int i = 0; i < 3; ++i)
      if (host_diag[i]) RRTMG_HIP_CHECK(ctx, hipMemcpyAsync(host_diag[i], dev_diag[i], b1, hipMemcpyDeviceToHost, s));
  }
  if (ctx->deferred && a->memspace == 1) return RRTMG_OK;
  RRTMG_HIP_CHECK(ctx, hipStreamSynchronize(s));
  return RRTMG_OK;
}
