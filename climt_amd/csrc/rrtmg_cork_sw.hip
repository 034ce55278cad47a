// rrtmg_cork_sw.hip -- the table-driven correlated-k two-stream shortwave (rrtmg_cork_sw.h), its table and their C entries:
//   rrtmg_hip_cork_sw_table_create   a shortwave table checked and uploaded by the longwave's upload (rrtmg_cork_table.h); the same handle
//                                    type, tagged by kind, freed by rrtmg_hip_cork_table_destroy
//   rrtmg_hip_cork_shortwave         climt CorkShortwaveRadiation (optics "correlated_k", additive overlap): per chunk of columns one
//                                    launch of three passes per (column, band), then the longwave's band reduction kernel
#include "rrtmg_column_call.h"
#include "rrtmg_cork_sw.h"
#include "rrtmg_cork_table.h"

namespace rrtmg {

// the arrays of the public struct (rrtmg_column_call.h); tools/cork_sw_check.cpp includes this file for the table and the checks alone.
// The three cloud arrays are [nlay][ncol][nband]: the bytes of a band-multiplied layer array.
#define ROW(m) RRTMG_COLUMN_ROW(rrtmg_cork_shortwave, CorkShortwaveCall, m)
constexpr ColumnRow kCorkShortwaveRows[] = {
    {ROW(t), ColumnExt::Lay, true}, {ROW(pmid), ColumnExt::Lay, true}, {ROW(pint), ColumnExt::Lev, true},
    {ROW(zenith), ColumnExt::Col, true}, {ROW(albedo), ColumnExt::Col, true}, {ROW(earth_sun), ColumnExt::Col, true},
    {ROW(taucld), ColumnExt::BandLay, false}, {ROW(ssacld), ColumnExt::BandLay, false}, {ROW(asycld), ColumnExt::BandLay, false},
    {ROW(gas0), ColumnExt::Lay, false}, {ROW(gas1), ColumnExt::Lay, false}, {ROW(gas2), ColumnExt::Lay, false}, {ROW(gas3), ColumnExt::Lay, false},   // read where the
    {ROW(gas4), ColumnExt::Lay, false}, {ROW(gas5), ColumnExt::Lay, false}, {ROW(gas6), ColumnExt::Lay, false}, {ROW(gas7), ColumnExt::Lay, false},   // table and the rule say so
    {ROW(up), ColumnExt::Lev, true}, {ROW(dn), ColumnExt::Lev, true}, {ROW(tend), ColumnExt::Lay, true}, {ROW(hr), ColumnExt::Lay, false},
    {ROW(up_band), ColumnExt::BandLev, false}, {ROW(dn_band), ColumnExt::BandLev, false},
    {ROW(tau_band), ColumnExt::BandLay, false}, {ROW(hr_band), ColumnExt::BandLay, false}};
#undef ROW
constexpr ColumnTable kCorkShortwave = column_table("cork_shortwave", "rrtmg_cork_shortwave", 1, "ncol must be positive", "nlay must be at least 1", "", kCorkShortwaveRows);

// ---- a shortwave table's description as the description both kinds are checked and uploaded by (planck stays NULL) ----------------------
inline rrtmg_cork_table_desc cork_sw_common_desc(const rrtmg_cork_sw_table_desc &d) {
  rrtmg_cork_table_desc c{};
  c.struct_size = sizeof c;
  c.ngas = d.ngas; c.nband = d.nband; c.ngpt = d.ngpt; c.nT = d.nT; c.nP = d.nP; c.nX = d.nX; c.nC = d.nC; c.k_is_f32 = d.k_is_f32;
  c.k = d.k; c.weights = d.weights; c.t_grid = d.t_grid; c.p_grid_log = d.p_grid_log; c.x_grid_log = d.x_grid_log;
  c.x_clip[0] = d.x_clip[0]; c.x_clip[1] = d.x_clip[1]; c.log_cont = d.log_cont;
  return c;
}
inline const char *cork_sw_table_refusal(const rrtmg_cork_sw_table_desc &d) {
  if (d.nC != 0) return "nC must be 0: the shortwave reads no CO2 axis (tables of rank 5 and 6)";
  if (d.solar_is_f32 != 0 && d.solar_is_f32 != 1) return "solar_is_f32 must be 0 (double) or 1 (float)";
  if (const char *why = cork_table_refusal(cork_sw_common_desc(d), false)) return why;
  if (!d.solar_source) return "solar_source must be given";
  return nullptr;
}

// what the call refuses beyond its gases, its table and its rows: -> nullptr, or why
inline const char *cork_sw_call_refusal(const rrtmg_cork_shortwave &a) {
  if (a.max_chunk_cols < 0) return "max_chunk_cols must be 0 (the library's choice) or positive";
  const int given = (a.taucld != nullptr) + (a.ssacld != nullptr) + (a.asycld != nullptr);
  if (given != 0 && given != 3) return "taucld, ssacld and asycld must be given together or not at all";
  return nullptr;
}

}  // namespace rrtmg

#ifdef __HIPCC__
namespace rrtmg {

// One thread per (column, band): waves of 64 consecutive columns of one band, grid (ceil(cols / 64), nband) over the chunk's columns.
// Layers in the outer loop and g-points in the inner one; the gas depths and the two running values per g-point are registers.  The
// work space is [band][g][row][level][column]: a wave writes and reads one run of 512 bytes per (g, row, level), and reads back only
// what it wrote itself.  The cloud arrays [k][ncol][band] are read with a stride of nband doubles, as the longwave's cloud depth is.
template <int NG, class K>
__global__ void __launch_bounds__(64) cork_sw_band_kernel(CorkShortwaveCall a) {
  const long col = a.col0 + (long)blockIdx.x * 64 + threadIdx.x;
  if (col >= a.col0 + a.cols) return;
  cork_sw_band_column<NG, K>(a, col, (int)blockIdx.y);
}

template <class K>
static void cork_sw_launch_band(hipStream_t s, dim3 grid, const CorkShortwaveCall &c) {
  const int n = c.tab.ngpt;
  if (n <= 1) hipLaunchKernelGGL((cork_sw_band_kernel<1, K>), grid, dim3(64), 0, s, c);
  else if (n <= 2) hipLaunchKernelGGL((cork_sw_band_kernel<2, K>), grid, dim3(64), 0, s, c);
  else if (n <= 4) hipLaunchKernelGGL((cork_sw_band_kernel<4, K>), grid, dim3(64), 0, s, c);
  else if (n <= 8) hipLaunchKernelGGL((cork_sw_band_kernel<8, K>), grid, dim3(64), 0, s, c);
  else hipLaunchKernelGGL((cork_sw_band_kernel<16, K>), grid, dim3(64), 0, s, c);
}

}  // namespace rrtmg

using namespace rrtmg;

extern "C" int rrtmg_hip_cork_sw_table_create(rrtmg_ctx *ctx, const rrtmg_cork_sw_table_desc *d, rrtmg_cork_table **out) {
  if (!ctx) return RRTMG_ERR_ARG;
  if (!d || !out) return ctx->fail(RRTMG_ERR_ARG, "cork_sw_table_create: NULL argument");
  if (d->struct_size != sizeof(rrtmg_cork_sw_table_desc))
    return ctx->fail(RRTMG_ERR_ARG, "cork_sw_table_create: struct_size %u, this library's rrtmg_cork_sw_table_desc has %zu bytes", d->struct_size, sizeof(rrtmg_cork_sw_table_desc));
  if (const char *why = cork_sw_table_refusal(*d)) return ctx->fail(RRTMG_ERR_ARG, "cork_sw_table_create: %s", why);
  const CorkSolar solar{d->solar_source, d->solar_is_f32, d->rayleigh};
  return cork_table_upload(ctx, "cork_sw_table_create", cork_sw_common_desc(*d), &solar, out);
}

extern "C" int rrtmg_hip_cork_shortwave(rrtmg_ctx *ctx, const rrtmg_cork_shortwave *a) {
  int rc = column_head(ctx, kCorkShortwave, a);
  if (rc) return rc;
  if (!a->table) return ctx->fail(RRTMG_ERR_ARG, "cork_shortwave: table must be given");
  const CorkTable *t = cork_find(ctx, a->table);
  if (!t) return ctx->fail(RRTMG_ERR_ARG, "cork_shortwave: the table is not one of this context");
  if (t->kind != kCorkShortwaveTable) return ctx->fail(RRTMG_ERR_ARG, "cork_shortwave: the table is a longwave table (rrtmg_hip_cork_table_create)");
  const CorkTableView &v = t->view;
  if (v.nC > 0) return ctx->fail(RRTMG_ERR_ARG, "cork_shortwave: the table has a CO2 axis");
  rc = column_required(ctx, kCorkShortwave, a);
  if (rc) return rc;
  if (const char *why = cork_gas_refusal(*a, v.ngas, v.nX, v.nC)) return ctx->fail(RRTMG_ERR_ARG, "cork_shortwave: %s", why);
  if (const char *why = cork_sw_call_refusal(*a)) return ctx->fail(RRTMG_ERR_ARG, "cork_shortwave: %s", why);
  const ColumnMask unread = cork_unread(kCorkShortwave, a->gas_rule, v.ngas, v.nX, v.nC);
  const size_t ncol = (size_t)a->ncol, nlev = (size_t)a->nlay + 1, nband = (size_t)v.nband;
  const size_t chunk = cork_sw_chunk_cols(nband, (size_t)v.ngpt, (size_t)a->nlay, ncol, (size_t)a->max_chunk_cols);

  CorkShortwaveCall c{};
  c.ncol = a->ncol; c.nlay = a->nlay; c.gas_rule = a->gas_rule; c.solar_f32 = t->solar_f32;
  c.tab = v;
  if (a->gas_rule != 1) c.tab.has_cont = 0;      // the continuum goes with the H2O mole fraction, which rule 1 alone has
  c.solar = t->solar; c.rayleigh = t->rayleigh;
  for (int i = 0; i < kCorkMaxGas; ++i) c.gas_scale[i] = a->gas_scale[i];
  c.m_h2o = a->m_h2o; c.g = a->g; c.cpd = a->cpd; c.pressure_scale = a->pressure_scale;
  c.work_cols = (int64_t)chunk;
  double *work_up = nullptr, *work_dn = nullptr, *work = nullptr;
  return column_call(
      ctx, kCorkShortwave, a, c, unread, "cork_sw.io",
      [&] {
        if (!a->up_band && !(work_up = (double *)ctx->buf("cork_sw.up_band", nband * nlev * ncol * sizeof(double)))) return ctx->status;
        if (!a->dn_band && !(work_dn = (double *)ctx->buf("cork_sw.dn_band", nband * nlev * ncol * sizeof(double)))) return ctx->status;
        if (!(work = (double *)ctx->buf("cork_sw.work", cork_sw_work_per_column(nband, (size_t)v.ngpt, (size_t)a->nlay) * chunk))) return ctx->status;
        return (int)RRTMG_OK;
      },
      [&] {
        if (!c.up_band) c.up_band = work_up;
        if (!c.dn_band) c.dn_band = work_dn;
        c.work = work;
        for (size_t col0 = 0; col0 < ncol; col0 += chunk) {      // the chunks follow each other on the stream: one work space
          c.col0 = (int64_t)col0;
          c.cols = (int64_t)(ncol - col0 < chunk ? ncol - col0 : chunk);
          const dim3 grid((unsigned)((c.cols + 63) / 64), (unsigned)nband);
          if (v.k_f32) cork_sw_launch_band<float>(ctx->stream, grid, c);
          else cork_sw_launch_band<double>(ctx->stream, grid, c);
          RRTMG_HIP_CHECK(ctx, hipGetLastError());
        }
        CorkLongwaveCall bb{};      // what cork_broadband reads
        bb.ncol = c.ncol; bb.nlay = c.nlay; bb.tab.nband = v.nband;
        bb.pint = c.pint; bb.g = c.g; bb.cpd = c.cpd; bb.pressure_scale = c.pressure_scale;
        bb.up = c.up; bb.dn = c.dn; bb.tend = c.tend; bb.hr = c.hr; bb.up_band = c.up_band; bb.dn_band = c.dn_band;
        cork_launch_broadband(ctx->stream, bb);      // the longwave's kernel (rrtmg_cork.hip)
        RRTMG_HIP_CHECK(ctx, hipGetLastError());
        return (int)RRTMG_OK;
      },
      false, nband);
}
#endif
