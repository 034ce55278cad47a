// rrtmg_cork.hip -- the table-driven correlated-k longwave (rrtmg_cork.h), its table on the device and their C entries:
//   rrtmg_hip_cork_table_create / _destroy   a correlated-k table checked, re-laid out and uploaded once; the handle belongs to the context
//   rrtmg_hip_cork_longwave                  climt CorkLongwaveRadiation (optics "correlated_k", additive overlap): interpolation, Planck
//                                            source and both sweeps in one pass per (column, band); the band reduction in a second
#include <string>
#include <vector>

#include "rrtmg_column_call.h"
#include "rrtmg_cork.h"

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

// ---- the table's description, checked on the host: -> nullptr, or why it is refused ---------------------------------------------------
inline bool cork_increasing(const double *g, int n) {
  for (int i = 1; i < n; ++i)
    if (!(g[i] > g[i - 1])) return false;
  return true;
}
inline const char *cork_table_refusal(const rrtmg_cork_table_desc &d) {
  if (d.reserved != 0) return "reserved must be 0";
  if (d.k_is_f32 != 0 && d.k_is_f32 != 1) return "k_is_f32 must be 0 (double) or 1 (float)";
  if (d.ngas < 1 || d.ngas > kCorkMaxGas) return "ngas must be 1 .. 8";
  if (d.nband < 1 || d.nband > kCorkMaxBand) return "nband must be 1 .. 32";
  if (d.ngpt < 1 || d.ngpt > kCorkMaxGpt) return "ngpt must be 1 .. 16";
  if (d.nT < 2 || d.nP < 2) return "the temperature and the pressure axis need at least 2 nodes each";
  if (d.nX != 0 && d.nX < 2) return "the H2O axis needs at least 2 nodes (or 0: no such axis)";
  if (d.nC != 0 && d.nC < 2) return "the CO2 axis needs at least 2 nodes (or 0: no such axis)";
  if (d.nC > 0 && d.nX == 0) return "a CO2 axis needs an H2O axis";
  if (!d.k || !d.weights || !d.planck || !d.t_grid || !d.p_grid_log) return "k, weights, planck, t_grid and p_grid_log must be given";
  if (d.nX > 0 && !d.x_grid_log) return "x_grid_log must be given with an H2O axis";
  if (d.nC > 0 && !d.c_grid_log) return "c_grid_log must be given with a CO2 axis";
  if (d.log_cont && d.nX == 0) return "a continuum needs an H2O axis";
  if (!cork_increasing(d.t_grid, d.nT)) return "t_grid must strictly increase";
  if (!cork_increasing(d.p_grid_log, d.nP)) return "p_grid_log must strictly increase";
  if (d.nX > 0 && !cork_increasing(d.x_grid_log, d.nX)) return "x_grid_log must strictly increase";
  if (d.nC > 0 && !cork_increasing(d.c_grid_log, d.nC)) return "c_grid_log must strictly increase";
  if (d.nX > 0 && !(d.x_clip[1] > d.x_clip[0])) return "x_clip must be an interval";
  if (d.nC > 0 && !(d.c_clip[1] > d.c_clip[0])) return "c_clip must be an interval";
  return nullptr;
}

// the number of k elements, and the place of the reference's element [ig][b][g][iT][iP][iX][iC] in the device layout
inline size_t cork_k_count(const rrtmg_cork_table_desc &d) {
  return (size_t)d.ngas * d.nband * d.ngpt * d.nT * d.nP * (d.nX > 0 ? d.nX : 1) * (d.nC > 0 ? d.nC : 1);
}
template <class K>
void cork_relayout(const rrtmg_cork_table_desc &d, const K *src, K *dst) {
  const size_t nX = d.nX > 0 ? d.nX : 1, nC = d.nC > 0 ? d.nC : 1, inner = (size_t)d.nT * d.nP * nX * nC;
  for (size_t gb = 0; gb < (size_t)d.ngas * d.nband; ++gb)
    for (size_t g = 0; g < (size_t)d.ngpt; ++g)
      for (size_t i = 0; i < inner; ++i) dst[(gb * inner + i) * d.ngpt + g] = src[(gb * d.ngpt + g) * inner + i];
}

// what the entry refuses of a call's gases: -> nullptr, or why
inline const char *cork_gas_refusal(const rrtmg_cork_longwave &a, int ngas, int nX, int nC) {
  const double *const gas[kCorkMaxGas] = {a.gas0, a.gas1, a.gas2, a.gas3, a.gas4, a.gas5, a.gas6, a.gas7};
  if (a.gas_rule < 0 || a.gas_rule > 2) return "gas_rule must be 0 (fully premixed), 1 (premixed background) or 2 (per gas)";
  if (a.gas_rule != 1 && nX > 0) return "a table with an H2O axis needs gas_rule 1 (the specific humidity in gas0)";
  if (a.gas_rule == 1 && nX > 0 && !gas[0]) return "gas0 (the specific humidity) must be given: the table has an H2O axis";
  if (a.gas_rule == 1 && nC > 0 && !gas[1]) return "gas1 (the CO2 mole fraction) must be given: the table has a CO2 axis";
  for (int i = 0; a.gas_rule == 2 && i < ngas; ++i)
    if (!gas[i]) return "a gas array is missing: gas_rule 2 reads gas<i> for every gas of the table";
  return nullptr;
}
// the rows a call does not read: the gas arrays beyond what the table and the rule ask for
inline ColumnMask cork_unread(int gas_rule, int ngas, int nX, int nC) {
  ColumnMask unread = 0;
  const int first = column_index(kCorkLongwave, "gas0");
  for (int i = 0; i < kCorkMaxGas; ++i) {
    const bool read = gas_rule == 2 ? i < ngas : gas_rule == 1 ? (i == 0 && nX > 0) || (i == 1 && nC > 0) : false;
    if (!read) unread |= ColumnMask(1) << (first + i);
  }
  return unread;
}

}  // namespace rrtmg

#ifdef __HIPCC__
namespace rrtmg {

struct CorkTable {
  rrtmg_ctx *owner;
  CorkTableView view;
  std::string buffer;
};

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

extern "C" int rrtmg_hip_cork_table_create(rrtmg_ctx *ctx, const rrtmg_cork_table_desc *d, rrtmg_cork_table **out) {
  if (!ctx) return RRTMG_ERR_ARG;
  if (!d || !out) return ctx->fail(RRTMG_ERR_ARG, "cork_table_create: NULL argument");
  if (d->struct_size != sizeof(rrtmg_cork_table_desc))
    return ctx->fail(RRTMG_ERR_ARG, "cork_table_create: struct_size %u, this library's rrtmg_cork_table_desc has %zu bytes", d->struct_size, sizeof(rrtmg_cork_table_desc));
  if (const char *why = cork_table_refusal(*d)) return ctx->fail(RRTMG_ERR_ARG, "cork_table_create: %s", why);
  int rc = ctx_prepare_device(ctx);
  if (rc) return rc;

  // one buffer: the doubles (weights, planck re-laid out, the grids, the continuum), then k in the device layout
  const size_t nw = (size_t)d->nband * d->ngpt, npl = nw * d->nT, ncont = d->log_cont ? (size_t)d->nband * d->nT * d->nP * d->nX : 0;
  const size_t ndouble = nw + npl + d->nT + d->nP + d->nX + d->nC + ncont, nk = cork_k_count(*d), kbytes = nk * (d->k_is_f32 ? sizeof(float) : sizeof(double));
  std::vector<char> host(ndouble * sizeof(double) + kbytes);
  double *p = (double *)host.data();
  size_t at = 0;
  const size_t o_w = at; memcpy(p + at, d->weights, nw * sizeof(double)); at += nw;
  const size_t o_pl = at;
  for (int b = 0; b < d->nband; ++b)
    for (int g = 0; g < d->ngpt; ++g)
      for (int i = 0; i < d->nT; ++i) p[at + ((size_t)b * d->nT + i) * d->ngpt + g] = d->planck[((size_t)b * d->ngpt + g) * d->nT + i];
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
    return ctx->fail(RRTMG_ERR_HIP, "cork_table_create: the upload failed: %s", hipGetErrorString(e));
  }
  const double *dd = (const double *)dev;
  CorkTableView &v = t->view;
  v.ngas = d->ngas; v.nband = d->nband; v.ngpt = d->ngpt; v.nT = d->nT; v.nP = d->nP; v.nX = d->nX; v.nC = d->nC;
  v.k_f32 = d->k_is_f32; v.has_cont = ncont ? 1 : 0;
  v.weights = dd + o_w; v.planck = dd + o_pl; v.t_grid = dd + o_t; v.p_grid = dd + o_p; v.x_grid = dd + o_x; v.c_grid = dd + o_c; v.log_cont = dd + o_cont;
  v.k = dd + ndouble;
  v.x_lo = d->x_clip[0]; v.x_hi = d->x_clip[1]; v.c_lo = d->c_clip[0]; v.c_hi = d->c_clip[1];
  ctx->cork_tables.push_back(t);
  *out = (rrtmg_cork_table *)t;
  return RRTMG_OK;
}

static CorkTable *cork_find(rrtmg_ctx *ctx, const rrtmg_cork_table *table) {
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
        hipLaunchKernelGGL(cork_broadband_kernel, dim3((unsigned)((ncol + 63) / 64), (unsigned)nlev), dim3(64), 0, ctx->stream, c);
        RRTMG_HIP_CHECK(ctx, hipGetLastError());
        return (int)RRTMG_OK;
      },
      false, nband);
}
#endif
