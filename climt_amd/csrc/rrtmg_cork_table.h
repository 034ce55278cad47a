// rrtmg_cork_table.h -- a correlated-k table of the cork scheme, of either kind (longwave: with the Planck fraction; shortwave: with the
// solar source and the Rayleigh coefficient): what rrtmg_cork.hip and rrtmg_cork_sw.hip share.  The checks of a description and of a
// call's gases are plain C++ (the two check programs under tools/ run them); the resident table is behind __HIPCC__.
#pragma once
#include <string>

#include "rrtmg_column_call.h"
#include "rrtmg_cork.h"

namespace rrtmg {

// ---- the table's description, checked on the host: -> nullptr, or why it is refused ---------------------------------------------------
inline bool cork_increasing(const double *g, int n) {
  for (int i = 1; i < n; ++i)
    if (!(g[i] > g[i - 1])) return false;
  return true;
}
// (a shortwave table is checked as this description with planck left NULL: need_planck false)
inline const char *cork_table_refusal(const rrtmg_cork_table_desc &d, bool need_planck = true) {
  if (d.reserved != 0) return "reserved must be 0";
  if (d.k_is_f32 != 0 && d.k_is_f32 != 1) return "k_is_f32 must be 0 (double) or 1 (float)";
  if (d.ngas < 1 || d.ngas > kCorkMaxGas) return "ngas must be 1 .. 8";
  if (d.nband < 1 || d.nband > kCorkMaxBand) return "nband must be 1 .. 32";
  if (d.ngpt < 1 || d.ngpt > kCorkMaxGpt) return "ngpt must be 1 .. 16";
  if (d.nT < 2 || d.nP < 2) return "the temperature and the pressure axis need at least 2 nodes each";
  if (d.nX != 0 && d.nX < 2) return "the H2O axis needs at least 2 nodes (or 0: no such axis)";
  if (d.nC != 0 && d.nC < 2) return "the CO2 axis needs at least 2 nodes (or 0: no such axis)";
  if (d.nC > 0 && d.nX == 0) return "a CO2 axis needs an H2O axis";
  if (need_planck && (!d.k || !d.weights || !d.planck || !d.t_grid || !d.p_grid_log)) return "k, weights, planck, t_grid and p_grid_log must be given";
  if (!need_planck && (!d.k || !d.weights || !d.t_grid || !d.p_grid_log)) return "k, weights, t_grid and p_grid_log must be given";
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

// what an entry refuses of a call's gases (A: rrtmg_cork_longwave or rrtmg_cork_shortwave): -> nullptr, or why
template <class A>
inline const char *cork_gas_refusal(const A &a, int ngas, int nX, int nC) {
  const double *const gas[kCorkMaxGas] = {a.gas0, a.gas1, a.gas2, a.gas3, a.gas4, a.gas5, a.gas6, a.gas7};
  if (a.gas_rule < 0 || a.gas_rule > 2) return "gas_rule must be 0 (fully premixed), 1 (premixed background) or 2 (per gas)";
  if (a.gas_rule != 1 && nX > 0) return "a table with an H2O axis needs gas_rule 1 (the specific humidity in gas0)";
  if (a.gas_rule == 1 && nX > 0 && !gas[0]) return "gas0 (the specific humidity) must be given: the table has an H2O axis";
  if (a.gas_rule == 1 && nC > 0 && !gas[1]) return "gas1 (the CO2 mole fraction) must be given: the table has a CO2 axis";
  for (int i = 0; a.gas_rule == 2 && i < ngas; ++i)
    if (!gas[i]) return "a gas array is missing: gas_rule 2 reads gas<i> for every gas of the table";
  return nullptr;
}
// the rows of the entry's table `t` a call does not read: the gas arrays beyond what the table and the rule ask for
inline ColumnMask cork_unread(const ColumnTable &t, int gas_rule, int ngas, int nX, int nC) {
  ColumnMask unread = 0;
  const int first = column_index(t, "gas0");
  for (int i = 0; i < kCorkMaxGas; ++i) {
    const bool read = gas_rule == 2 ? i < ngas : gas_rule == 1 ? (i == 0 && nX > 0) || (i == 1 && nC > 0) : false;
    if (!read) unread |= ColumnMask(1) << (first + i);
  }
  return unread;
}

}  // namespace rrtmg

#ifdef __HIPCC__
#include "rrtmg_ctx.h"

namespace rrtmg {

enum CorkKind { kCorkLongwaveTable = 0, kCorkShortwaveTable = 1 };

struct CorkTable {
  rrtmg_ctx *owner;
  CorkTableView view;
  std::string buffer;
  int kind;
  int solar_f32;                       // a shortwave table: whether solar_source came as float
  const double *solar, *rayleigh;      // a shortwave table: [nband][ngpt] widened to double; [nband] or nullptr
};

// what a shortwave table has in place of the Planck fraction
struct CorkSolar { const void *source; int is_f32; const double *rayleigh; };

// The one upload of both kinds (rrtmg_cork.hip): `d` checked already (a shortwave table: planck NULL, `solar` given); one device buffer,
// the handle added to the context's list.  `entry`: the prefix of the messages.
int cork_table_upload(rrtmg_ctx *ctx, const char *entry, const rrtmg_cork_table_desc &d, const CorkSolar *solar, rrtmg_cork_table **out);
// the table of this context behind a handle, or nullptr (the list is searched: a handle of another context is never dereferenced)
CorkTable *cork_find(rrtmg_ctx *ctx, const rrtmg_cork_table *table);
// cork_broadband_kernel (rrtmg_cork.hip) over every (column, level) of `c`: the band reduction of both spectra
void cork_launch_broadband(hipStream_t s, const CorkLongwaveCall &c);

}  // namespace rrtmg
#endif
