// rrtmg_cork.hip -- the table-driven correlated-k longwave (rrtmg_cork.h), its table on the device and their C entries:
//   rrtmg_hip_cork_table_create / _destroy   a correlated-k table checked, re-laid out and uploaded once; the handle belongs to the context
//                                            (cork_table_upload and cork_find serve the shortwave tables of rrtmg_cork_sw.hip too)
//   rrtmg_hip_cork_longwave                  climt CorkLongwaveRadiation (optics "correlated_k", additive overlap): interpolation, Planck
//                                            source and both sweeps in one pass per (column, band); the band reduction in a second
#include <string>
#include <vector>

#include "rrtmg_column_call.h"
#include "rrtmg_cork.h"
#include "rrtmg_cork_table.h"

namespace rrtmg {

// the arrays of the public struct (rrtmg_column_call.h); tools/cork_check.cpp includes this file for the table and the checks alone.
// taucld is [nlay][ncol][nband]: the bytes of a band-multiplied layer array.
#define ROW(m) RRTMG_COLUMN_ROW(rrtmg_cork_longwave, CorkLongwaveCall, m)
constexpr ColumnRow kCorkLongwaveRows[] = {
    {ROW(t), ColumnExt::Lay, true}, {ROW(pmid), ColumnExt::Lay, true}, {ROW(pint), ColumnExt::Lev, true}, {ROW(tsfc), ColumnExt::Col, true},
    {ROW(emis), ColumnExt::BandCol, true}, {ROW(taucld), ColumnExt::BandLay, false},
    {ROW(gas0), ColumnExt::Lay, false}, {ROW(gas1), ColumnExt::Lay, false}, {ROW(gas2), ColumnExt::Lay, false}, {ROW(gas3), ColumnExt::Lay, false},   // read where the
    {ROW(gas4), ColumnExt::Lay, false}, {ROW(gas5), ColumnExt::Lay, false}, {ROW(gas6), ColumnExt::Lay, false}, {ROW(gas7), ColumnExt::Lay, false},   // table and the rule say so
    {ROW(up), ColumnExt::Lev, true}, {ROW(dn), ColumnExt::Lev, true}, {ROW(tend), ColumnExt::Lay, true}, {ROW(hr), ColumnExt::Lay, false},
    {ROW(up_band), ColumnExt::BandLev, false}, {ROW(dn_band), ColumnExt::BandLev, false},
    {ROW(tau_band), ColumnExt::BandLay, false}, {ROW(trans_band), ColumnExt::BandLay, false}, {ROW(hr_band), ColumnExt::BandLay, false}};
#undef ROW
constexpr ColumnTable kCorkLongwave = column_table("cork_longwave", "rrtmg_cork_longwave", 1, "ncol must be positive", "nlay must be at least 1", "", kCorkLongwaveRows);

// the rows a call does not read (the checks of a table's description and of a call's gases: rrtmg_cork_table.h)
inline ColumnMask cork_unread(int gas_rule, int ngas, int nX, int nC) { return cork_unread(kCorkLongwave, gas_rule, ngas, nX, nC); }

}  // namespace rrtmg

#ifdef __HIPCC__
namespace rrtmg {

void free_cork_tables(rrtmg_ctx *ctx) {
  for (CorkTable *t : ctx->cork_tables) delete t;
  ctx->cork_tables.clear();
}

// One thread per (column, band): waves of 64 consecutive columns of one band, grid (ceil(ncol / 64), nband).  Layers in the outer
// loop and g-points in the inner one; the running fluxes, the optical depths and the sources of the NG g-points are registers.
// Neighbouring columns bracket alike, so the 4, 8 or 16 corners of a layer fall on few lines for the whole wave, and the g-points
// of a corner are one run of ngpt elements.  Profiles are [k][ncol]: a wave touches one run of 512 bytes per access; the cloud
// depth [k][ncol][band] is read with a stride of nband doubles, the bands' waves of the same columns sharing its lines in L2.
template <int NG, class K>
__global__ void __launch_bounds__(64) cork_band_kernel(CorkLongwaveCall a) {
  const long col = (long)blockIdx.x * 64 + threadIdx.x;
  if (col >= a.ncol) return;
  cork_band_column<NG, K>(a, col, (int)blockIdx.y);
}

// the band reduction: one thread per (column, level), bands in ascending order
__global__ void __launch_bounds__(64) cork_broadband_kernel(CorkLongwaveCall a) {
  const long col = (long)blockIdx.x * 64 + threadIdx.x;
  if (col >= a.ncol) return;
  cork_broadband(a, col, (int)blockIdx.y);
}

// (the shortwave's entry launches it too: rrtmg_cork_table.h)
void cork_launch_broadband(hipStream_t s, const CorkLongwaveCall &c) {
  hipLaunchKernelGGL(cork_broadband_kernel, dim3((unsigned)((c.ncol + 63) / 64), (unsigned)(c.nlay + 1)), dim3(64), 0, s, c);
}

template <class K>
static void cork_launch_band(hipStream_t s, dim3 grid, const CorkLongwaveCall &c) {
  const int n = c.tab.ngpt;
  if (n <= 1) hipLaunchKernelGGL((cork_band_kernel<1, K>), grid, dim3(64), 0, s, c);
  else if (n <= 2) hipLaunchKernelGGL((cork_band_kernel<2, K>), grid, dim3(64), 0, s, c);
  else if (n <= 4) hipLaunchKernelGGL((cork_band_kernel<4, K>), grid, dim3(64), 0, s, c);
  else if (n <= 8) hipLaunchKernelGGL((cork_band_kernel<8, K>), grid, dim3(64), 0, s, c);
  else hipLaunchKernelGGL((cork_band_kernel<16, K>), grid, dim3(64), 0, s, c);
}

}  // namespace rrtmg

using namespace rrtmg;

// the one upload of both kinds of table (rrtmg_cork_table.h)
int rrtmg::cork_table_upload(rrtmg_ctx *ctx, const char *entry, const rrtmg_cork_table_desc &desc, const CorkSolar *solar, rrtmg_cork_table **out) {
  const rrtmg_cork_table_desc *d = &desc;
  int rc = ctx_prepare_device(ctx);
  if (rc) return rc;

  // one buffer: the doubles (weights, planck re-laid out or the solar source and the Rayleigh coefficient, the grids, the continuum),
  // then k in the device layout
  const size_t nw = (size_t)d->nband * d->ngpt, npl = solar ? nw + (solar->rayleigh ? d->nband : 0) : nw * d->nT;
  const size_t ncont = d->log_cont ? (size_t)d->nband * d->nT * d->nP * d->nX : 0;
  const size_t ndouble = nw + npl + d->nT + d->nP + d->nX + d->nC + ncont, nk = cork_k_count(*d), kbytes = nk * (d->k_is_f32 ? sizeof(float) : sizeof(double));
  std::vector<char> host(ndouble * sizeof(double) + kbytes);
  double *p = (double *)host.data();
  size_t at = 0;
  const size_t o_w = at; memcpy(p + at, d->weights, nw * sizeof(double)); at += nw;
  const size_t o_pl = at;
  if (solar) {
    for (size_t i = 0; i < nw; ++i) p[at + i] = solar->is_f32 ? (double)((const float *)solar->source)[i] : ((const double *)solar->source)[i];
    if (solar->rayleigh) memcpy(p + at + nw, solar->rayleigh, d->nband * sizeof(double));
  } else {
    for (int b = 0; b < d->nband; ++b)
      for (int g = 0; g < d->ngpt; ++g)
        for (int i = 0; i < d->nT; ++i) p[at + ((size_t)b * d->nT + i) * d->ngpt + g] = d->planck[((size_t)b * d->ngpt + g) * d->nT + i];
  }
  at += npl;
  const size_t o_t = at; memcpy(p + at, d->t_grid, d->nT * sizeof(double)); at += d->nT;
  const size_t o_p = at; memcpy(p + at, d->p_grid_log, d->nP * sizeof(double)); at += d->nP;
  const size_t o_x = at; if (d->nX > 0) memcpy(p + at, d->x_grid_log, d->nX * sizeof(double)); at += d->nX;
  const size_t o_c = at; if (d->nC > 0) memcpy(p + at, d->c_grid_log, d->nC * sizeof(double)); at += d->nC;
  const size_t o_cont = at; if (ncont) memcpy(p + at, d->log_cont, ncont * sizeof(double)); at += ncont;
  if (d->k_is_f32) cork_relayout(*d, (const float *)d->k, (float *)(p + at));
  else cork_relayout(*d, (const double *)d->k, p + at);

  CorkTable *t = new CorkTable();
  t->owner = ctx;
  t->buffer = "cork.table." + std::to_string(ctx->cork_serial++);
  char *dev = (char *)ctx->buf(t->buffer, host.size());
  if (!dev) { ctx->bufs.erase(t->buffer); delete t; return ctx->status; }
  hipError_t e = hipMemcpyAsync(dev, host.data(), host.size(), hipMemcpyHostToDevice, ctx->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
  if (e != hipSuccess) {
    (void)hipFree(dev); ctx->bufs.erase(t->buffer); delete t;
    return ctx->fail(RRTMG_ERR_HIP, "%s: the upload failed: %s", entry, hipGetErrorString(e));
  }
  const double *dd = (const double *)dev;
  CorkTableView &v = t->view;
  v.ngas = d->ngas; v.nband = d->nband; v.ngpt = d->ngpt; v.nT = d->nT; v.nP = d->nP; v.nX = d->nX; v.nC = d->nC;
  v.k_f32 = d->k_is_f32; v.has_cont = ncont ? 1 : 0;
  v.weights = dd + o_w; v.planck = solar ? nullptr : dd + o_pl; v.t_grid = dd + o_t; v.p_grid = dd + o_p; v.x_grid = dd + o_x; v.c_grid = dd + o_c; v.log_cont = dd + o_cont;
  v.k = dd + ndouble;
  v.x_lo = d->x_clip[0]; v.x_hi = d->x_clip[1]; v.c_lo = d->c_clip[0]; v.c_hi = d->c_clip[1];
  t->kind = solar ? kCorkShortwaveTable : kCorkLongwaveTable;
  t->solar_f32 = solar ? solar->is_f32 : 0;
  t->solar = solar ? dd + o_pl : nullptr;
  t->rayleigh = solar && solar->rayleigh ? dd + o_pl + nw : nullptr;
  ctx->cork_tables.push_back(t);
  *out = (rrtmg_cork_table *)t;
  return RRTMG_OK;
}

extern "C" int rrtmg_hip_cork_table_create(rrtmg_ctx *ctx, const rrtmg_cork_table_desc *d, rrtmg_cork_table **out) {
  if (!ctx) return RRTMG_ERR_ARG;
  if (!d || !out) return ctx->fail(RRTMG_ERR_ARG, "cork_table_create: NULL argument");
  if (d->struct_size != sizeof(rrtmg_cork_table_desc))
    return ctx->fail(RRTMG_ERR_ARG, "cork_table_create: struct_size %u, this library's rrtmg_cork_table_desc has %zu bytes", d->struct_size, sizeof(rrtmg_cork_table_desc));
  if (const char *why = cork_table_refusal(*d)) return ctx->fail(RRTMG_ERR_ARG, "cork_table_create: %s", why);
  return cork_table_upload(ctx, "cork_table_create", *d, nullptr, out);
}

CorkTable *rrtmg::cork_find(rrtmg_ctx *ctx, const rrtmg_cork_table *table) {
  for (CorkTable *t : ctx->cork_tables)
    if ((const void *)t == (const void *)table) return t;
  return nullptr;
}

extern "C" int rrtmg_hip_cork_table_destroy(rrtmg_ctx *ctx, rrtmg_cork_table *table) {
  if (!ctx) return RRTMG_ERR_ARG;
  CorkTable *t = cork_find(ctx, table);
  if (!t) return ctx->fail(RRTMG_ERR_ARG, "cork_table_destroy: not a table of this context");
  (void)hipSetDevice(ctx->device);
  if (ctx->stream) (void)hipStreamSynchronize(ctx->stream);      // a call that reads it may be in flight
  auto it = ctx->bufs.find(t->buffer);
  if (it != ctx->bufs.end()) {
    if (it->second.p) (void)hipFree(it->second.p);
    ctx->bufs.erase(it);
  }
  for (size_t i = 0; i < ctx->cork_tables.size(); ++i)
    if (ctx->cork_tables[i] == t) { ctx->cork_tables.erase(ctx->cork_tables.begin() + i); break; }
  delete t;
  return RRTMG_OK;
}

extern "C" int rrtmg_hip_cork_longwave(rrtmg_ctx *ctx, const rrtmg_cork_longwave *a) {
  int rc = column_head(ctx, kCorkLongwave, a);
  if (rc) return rc;
  if (a->reserved != 0) return ctx->fail(RRTMG_ERR_ARG, "cork_longwave: reserved must be 0");
  if (!a->table) return ctx->fail(RRTMG_ERR_ARG, "cork_longwave: table must be given");
  const CorkTable *t = cork_find(ctx, a->table);      // (the list is searched: a handle of another context is never dereferenced)
  if (!t) return ctx->fail(RRTMG_ERR_ARG, "cork_longwave: the table is not one of this context");
  if (t->kind != kCorkLongwaveTable) return ctx->fail(RRTMG_ERR_ARG, "cork_longwave: the table is a shortwave table (rrtmg_hip_cork_sw_table_create)");
  const CorkTableView &v = t->view;
  rc = column_required(ctx, kCorkLongwave, a);
  if (rc) return rc;
  if (const char *why = cork_gas_refusal(*a, v.ngas, v.nX, v.nC)) return ctx->fail(RRTMG_ERR_ARG, "cork_longwave: %s", why);
  const ColumnMask unread = cork_unread(a->gas_rule, v.ngas, v.nX, v.nC);
  const size_t ncol = (size_t)a->ncol, nlev = (size_t)a->nlay + 1, nband = (size_t)v.nband;

  CorkLongwaveCall c{};
  c.ncol = a->ncol; c.nlay = a->nlay; c.gas_rule = a->gas_rule;
  c.tab = v;
  if (a->gas_rule != 1) c.tab.has_cont = 0;      // the continuum goes with the H2O mole fraction, which rule 1 alone has
  for (int i = 0; i < kCorkMaxGas; ++i) c.gas_scale[i] = a->gas_scale[i];
  c.m_h2o = a->m_h2o; c.sigma_sb = a->sigma_sb; c.g = a->g; c.cpd = a->cpd; c.diffusivity = a->diffusivity; c.pressure_scale = a->pressure_scale;
  // the per-band fluxes the caller does not ask for still feed the band reduction: work space of the outputs' own size
  double *work_up = nullptr, *work_dn = nullptr;
  return column_call(
      ctx, kCorkLongwave, a, c, unread, "cork.io",
      [&] {
        if (!a->up_band && !(work_up = (double *)ctx->buf("cork.up_band", nband * nlev * ncol * sizeof(double)))) return ctx->status;
        if (!a->dn_band && !(work_dn = (double *)ctx->buf("cork.dn_band", nband * nlev * ncol * sizeof(double)))) return ctx->status;
        return (int)RRTMG_OK;
      },
      [&] {
        if (!c.up_band) c.up_band = work_up;
        if (!c.dn_band) c.dn_band = work_dn;
        const dim3 grid((unsigned)((ncol + 63) / 64), (unsigned)nband);
        if (v.k_f32) cork_launch_band<float>(ctx->stream, grid, c);
        else cork_launch_band<double>(ctx->stream, grid, c);
        RRTMG_HIP_CHECK(ctx, hipGetLastError());
        cork_launch_broadband(ctx->stream, c);
        RRTMG_HIP_CHECK(ctx, hipGetLastError());
        return (int)RRTMG_OK;
      },
      false, nband);
}
#endif
