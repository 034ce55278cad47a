// cork_check.cpp -- the table-driven correlated-k longwave (climt_amd/csrc/rrtmg_cork.h: the rules of one (column, band) and of one
// (column, level), as one thread of cork_band_kernel and cork_broadband_kernel runs them) and the host side of rrtmg_cork.hip (the row
// table, the table's checks and re-layout, the gas refusals) on the CPU, no device: a stand-alone program for tests/test_cork_lw.py
// and the host sanitizers.
//
//   c++ -std=c++17 -ffp-contract=off -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/cork_check.cpp -o cork_check
//
//   cork_check tables
//       Line: <entry> <in|out> <struct> <member> <extent> <f64|i32> <required or -> <the input it may be, or ->, then the checks of
//       tools/column_table_check.h: the staging plan at nband 1, 4 with every combination of the optional outputs, gas0 and taucld
//       (the sizes of the band-multiplied extents among them), the aliasing refusals and the "must be given" text; then the refusals
//       of a table's description and of a call's gases.  Last line "ok".
//   cork_check run <in.bin> <out.bin>
//       in : 40 doubles {ncol, nlay, gas_rule, ngas, nband, ngpt, nT, nP, nX, nC, k_is_f32, has_cont, has_cloud, gas_scale[8], m_h2o,
//            sigma_sb, g, cpd, diffusivity, pressure_scale, x_clip[2], c_clip[2], 0...}, then k (the reference's layout, as doubles),
//            weights, planck [nband][ngpt][nT], t_grid, p_grid_log, x_grid_log, c_grid_log, log_cont, then t, pmid [nlay][ncol], pint
//            [nlay+1][ncol], tsfc [ncol], emis [nband][ncol], taucld [nlay][ncol][nband] (with has_cloud), the gas arrays the rule reads
//       out: up, dn [nlay+1][ncol], tend, hr [nlay][ncol], up_band, dn_band [nband][nlay+1][ncol], tau_band, trans_band, hr_band
//       The run without the optional outputs must agree bit for bit.  Every "thread" of the two launches runs in turn, the last
//       column first.  The program checks that every output element was written, that the guard elements around every array are
//       intact and that the inputs are untouched.
// Exit status 0 and a last line that starts with "ok" when everything holds.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../climt_amd/csrc/rrtmg_cork.hip"
#include "column_table_check.h"

using namespace rrtmg;

static int tables() {
  const ColumnTable &t = kCorkLongwave;
  print_table(t);
  ColumnMask optional_out = 0;
  for (int i = 0; i < t.n; ++i) {
    CHECK(!t.rows[i].in_place_of && !t.rows[i].i32);
    if (t.rows[i].out && !t.rows[i].required) optional_out |= ColumnMask(1) << i;
  }
  check_plan(t, {1, 4}, optional_out | column_bits(t, {"gas0", "taucld"}));      // (every subset of the fifteen optional rows is too many)
  check_aliasing<rrtmg_cork_longwave>(t, "", "t, pmid, pint, tsfc, emis, up, dn and tend must be given", 4);
  rrtmg_cork_longwave a{};

  // the description of a table
  const double grid[3] = {1.0, 2.0, 3.0}, flat[3] = {1.0, 2.0, 2.0}, k[64] = {0.0};
  rrtmg_cork_table_desc d{};
  d.ngas = 1; d.nband = 2; d.ngpt = 2; d.nT = 3; d.nP = 3; d.k = k; d.weights = k; d.planck = k; d.t_grid = grid; d.p_grid_log = grid;
  CHECK(!cork_table_refusal(d) && cork_k_count(d) == 36);
  auto refused = [&](auto change) { rrtmg_cork_table_desc e = d; change(e); return cork_table_refusal(e) != nullptr; };
  CHECK(refused([](auto &e) { e.ngas = 9; }) && refused([](auto &e) { e.nband = 33; }) && refused([](auto &e) { e.ngpt = 17; }) && refused([](auto &e) { e.ngas = 0; }));
  CHECK(refused([](auto &e) { e.nT = 1; }) && refused([](auto &e) { e.nX = 1; }) && refused([](auto &e) { e.nC = 3; }) && refused([](auto &e) { e.k = nullptr; }));
  CHECK(refused([&](auto &e) { e.t_grid = flat; }) && refused([&](auto &e) { e.p_grid_log = flat; }) && refused([&](auto &e) { e.log_cont = k; }));
  CHECK(refused([](auto &e) { e.nX = 3; }) && refused([&](auto &e) { e.nX = 3; e.x_grid_log = flat; e.x_clip[1] = 1.0; }));
  CHECK(refused([&](auto &e) { e.nX = 3; e.x_grid_log = grid; }) && !refused([&](auto &e) { e.nX = 3; e.x_grid_log = grid; e.x_clip[1] = 1.0; }));
  CHECK(refused([](auto &e) { e.reserved = 1; }) && refused([](auto &e) { e.k_is_f32 = 2; }));

  // the gases of a call
  const double *some = grid;
  CHECK(!cork_gas_refusal(a, 1, 0, 0));                                       // rule 0 reads none
  a.gas_rule = 3; CHECK(cork_gas_refusal(a, 1, 0, 0));
  a.gas_rule = 0; CHECK(cork_gas_refusal(a, 1, 3, 0));                        // an H2O axis needs rule 1
  a.gas_rule = 1; CHECK(cork_gas_refusal(a, 1, 3, 0)); a.gas0 = some; CHECK(!cork_gas_refusal(a, 1, 3, 0) && cork_gas_refusal(a, 1, 3, 4));
  a.gas1 = some; CHECK(!cork_gas_refusal(a, 1, 3, 4));
  a.gas_rule = 2; CHECK(!cork_gas_refusal(a, 2, 0, 0) && cork_gas_refusal(a, 3, 0, 0));
  const int g0 = column_index(t, "gas0");
  CHECK(cork_unread(0, 1, 0, 0) == ColumnMask(0xff) << g0 && cork_unread(2, 2, 0, 0) == ColumnMask(0xfc) << g0);
  CHECK(cork_unread(1, 1, 3, 0) == ColumnMask(0xfe) << g0 && cork_unread(1, 1, 3, 4) == ColumnMask(0xfc) << g0 && cork_unread(1, 1, 0, 0) == ColumnMask(0xff) << g0);
  printf("ok\n");
  return 0;
}

// ---- the rules -------------------------------------------------------------------------------------------------------------------

template <class K>
static void run_bands(const CorkLongwaveCall &c) {
  for (int b = c.tab.nband - 1; b >= 0; --b)
    for (int col = c.ncol - 1; col >= 0; --col) {
      const int n = c.tab.ngpt;
      if (n <= 1) cork_band_column<1, K>(c, col, b);
      else if (n <= 2) cork_band_column<2, K>(c, col, b);
      else if (n <= 4) cork_band_column<4, K>(c, col, b);
      else if (n <= 8) cork_band_column<8, K>(c, col, b);
      else cork_band_column<16, K>(c, col, b);
    }
}

static int run(const char *in, const char *out) {
  const std::vector<double> file = read_all(in);
  CHECK(file.size() > 40);
  const double *h = file.data();
  rrtmg_cork_table_desc d{};
  const int ncol = (int)h[0], nlay = (int)h[1], rule = (int)h[2];
  d.ngas = (int)h[3]; d.nband = (int)h[4]; d.ngpt = (int)h[5]; d.nT = (int)h[6]; d.nP = (int)h[7]; d.nX = (int)h[8]; d.nC = (int)h[9]; d.k_is_f32 = (int)h[10];
  const bool has_cont = h[11] != 0.0, has_cloud = h[12] != 0.0;
  CHECK(ncol > 0 && nlay >= 1);
  const size_t nk = cork_k_count(d), nw = (size_t)d.nband * d.ngpt, ncont = has_cont ? (size_t)d.nband * d.nT * d.nP * d.nX : 0;
  const double *p = h + 40;
  const double *k = p; p += nk;
  d.k = k; d.weights = p; p += nw; d.planck = p; p += nw * d.nT; d.t_grid = p; p += d.nT; d.p_grid_log = p; p += d.nP;
  d.x_grid_log = d.nX ? p : nullptr; p += d.nX; d.c_grid_log = d.nC ? p : nullptr; p += d.nC; d.log_cont = ncont ? p : nullptr; p += ncont;
  d.x_clip[0] = h[27]; d.x_clip[1] = h[28]; d.c_clip[0] = h[29]; d.c_clip[1] = h[30];
  CHECK(cork_table_refusal(d) == nullptr);

  // the device layout, as rrtmg_hip_cork_table_create makes it
  std::vector<double> kd(nk), planck(nw * d.nT);
  std::vector<float> kf(nk), kf_src(nk);
  if (d.k_is_f32) {
    for (size_t i = 0; i < nk; ++i) { kf_src[i] = (float)k[i]; CHECK((double)kf_src[i] == k[i]); }
    cork_relayout(d, kf_src.data(), kf.data());
  } else cork_relayout(d, k, kd.data());
  for (int b = 0; b < d.nband; ++b)
    for (int g = 0; g < d.ngpt; ++g)
      for (int i = 0; i < d.nT; ++i) planck[((size_t)b * d.nT + i) * d.ngpt + g] = d.planck[((size_t)b * d.ngpt + g) * d.nT + i];

  const size_t n1 = ncol, nl = (size_t)nlay * n1, nl1 = nl + n1, nb = d.nband;
  const double *t = p, *pmid = t + nl, *pint = pmid + nl, *tsfc = pint + nl1, *emis = tsfc + n1, *cloud = emis + nb * n1, *gases = cloud + (has_cloud ? nl * nb : 0);
  rrtmg_cork_longwave pub{};
  pub.gas_rule = rule;
  const double *gp[kCorkMaxGas] = {};
  const ColumnMask unread = cork_unread(rule, d.ngas, d.nX, d.nC);
  size_t ngiven = 0;
  for (int i = 0; i < kCorkMaxGas; ++i)
    if (!(unread >> (column_index(kCorkLongwave, "gas0") + i) & 1)) gp[i] = gases + nl * ngiven++;
  CHECK((size_t)(gases + nl * ngiven - h) == file.size());
  pub.gas0 = gp[0]; pub.gas1 = gp[1]; pub.gas2 = gp[2]; pub.gas3 = gp[3]; pub.gas4 = gp[4]; pub.gas5 = gp[5]; pub.gas6 = gp[6]; pub.gas7 = gp[7];
  CHECK(cork_gas_refusal(pub, d.ngas, d.nX, d.nC) == nullptr);

  std::vector<double> result;
  for (int pass = 0; pass < 2; ++pass) {      // with every optional output, then with none
    Guarded gt, gpm, gpi, gts, ge, gc, gg[kCorkMaxGas], up, dn, tend, hr, ub, db, tb, trb, hb;
    gt.set(t, nl); gpm.set(pmid, nl); gpi.set(pint, nl1); gts.set(tsfc, n1); ge.set(emis, nb * n1); gc.set(has_cloud ? cloud : nullptr, has_cloud ? nl * nb : 0);
    for (int i = 0; i < kCorkMaxGas; ++i) gg[i].set(gp[i], gp[i] ? nl : 0);
    up.set(nullptr, nl1); dn.set(nullptr, nl1); tend.set(nullptr, nl); hr.set(nullptr, nl);
    ub.set(nullptr, nb * nl1); db.set(nullptr, nb * nl1); tb.set(nullptr, nb * nl); trb.set(nullptr, nb * nl); hb.set(nullptr, nb * nl);
    CorkLongwaveCall c{};
    c.ncol = ncol; c.nlay = nlay; c.gas_rule = rule;
    CorkTableView &v = c.tab;
    v.ngas = d.ngas; v.nband = d.nband; v.ngpt = d.ngpt; v.nT = d.nT; v.nP = d.nP; v.nX = d.nX; v.nC = d.nC; v.k_f32 = d.k_is_f32; v.has_cont = ncont && rule == 1 ? 1 : 0;
    v.k = d.k_is_f32 ? (const void *)kf.data() : (const void *)kd.data();
    v.weights = d.weights; v.planck = planck.data(); v.t_grid = d.t_grid; v.p_grid = d.p_grid_log; v.x_grid = d.x_grid_log; v.c_grid = d.c_grid_log; v.log_cont = d.log_cont;
    v.x_lo = d.x_clip[0]; v.x_hi = d.x_clip[1]; v.c_lo = d.c_clip[0]; v.c_hi = d.c_clip[1];
    c.t = gt.p(); c.pmid = gpm.p(); c.pint = gpi.p(); c.tsfc = gts.p(); c.emis = ge.p(); c.taucld = has_cloud ? gc.p() : nullptr;
    const double *bound[kCorkMaxGas];
    for (int i = 0; i < kCorkMaxGas; ++i) bound[i] = gp[i] ? gg[i].p() : nullptr;
    c.gas0 = bound[0]; c.gas1 = bound[1]; c.gas2 = bound[2]; c.gas3 = bound[3]; c.gas4 = bound[4]; c.gas5 = bound[5]; c.gas6 = bound[6]; c.gas7 = bound[7];
    for (int i = 0; i < kCorkMaxGas; ++i) c.gas_scale[i] = h[13 + i];
    c.m_h2o = h[21]; c.sigma_sb = h[22]; c.g = h[23]; c.cpd = h[24]; c.diffusivity = h[25]; c.pressure_scale = h[26];
    c.up = up.p(); c.dn = dn.p(); c.tend = tend.p(); c.up_band = ub.p(); c.dn_band = db.p();      // (the band fluxes: the caller's or the entry's work space)
    if (pass == 0) { c.hr = hr.p(); c.tau_band = tb.p(); c.trans_band = trb.p(); c.hr_band = hb.p(); }
    if (d.k_is_f32) run_bands<float>(c); else run_bands<double>(c);
    for (int lev = nlay; lev >= 0; --lev)
      for (int col = ncol - 1; col >= 0; --col) cork_broadband(c, col, lev);
    for (Guarded *g : {&gt, &gpm, &gpi, &gts, &ge, &gc, &up, &dn, &tend, &hr, &ub, &db, &tb, &trb, &hb}) g->check_guards();
    for (int i = 0; i < kCorkMaxGas; ++i) { gg[i].check_guards(); CHECK(!gp[i] || gg[i].holds(gp[i])); }
    CHECK(gt.holds(t) && gpm.holds(pmid) && gpi.holds(pint) && gts.holds(tsfc) && ge.holds(emis) && (!has_cloud || gc.holds(cloud)));      // only read
    CHECK(up.written() && dn.written() && tend.written() && ub.written() && db.written());
    std::vector<double> o;
    for (Guarded *g : {&up, &dn, &tend}) o.insert(o.end(), g->p(), g->p() + g->n);
    if (pass == 0) {
      CHECK(hr.written() && tb.written() && trb.written() && hb.written());
      for (size_t i = 0; i < nl; ++i) CHECK(hr.p()[i] == tend.p()[i] * 86400.0);
      for (size_t b = 0; b < nb; ++b)
        for (size_t i = 0; i < n1; ++i) CHECK(db.p()[(b * (nlay + 1) + nlay) * n1 + i] == 0.0 && !std::signbit(db.p()[(b * (nlay + 1) + nlay) * n1 + i]));
      result = o;
      for (Guarded *g : {&hr, &ub, &db, &tb, &trb, &hb}) result.insert(result.end(), g->p(), g->p() + g->n);
    } else {
      CHECK(hr.untouched() && tb.untouched() && trb.untouched() && hb.untouched());
      CHECK(memcmp(o.data(), result.data(), o.size() * sizeof(double)) == 0);      // the optional outputs change no bit of the others
    }
  }
  FILE *f = fopen(out, "wb");
  CHECK(f != nullptr && fwrite(result.data(), sizeof(double), result.size(), f) == result.size());
  fclose(f);
  printf("ok (cork, %d columns, %d layers, %d bands, %d g-points, rank %d, rule %d)\n", ncol, nlay, d.nband, d.ngpt, 5 + (d.nX > 0) + (d.nC > 0), rule);
  return 0;
}

int main(int argc, char **argv) {
  if (argc == 2 && !strcmp(argv[1], "tables")) return tables();
  if (argc == 4 && !strcmp(argv[1], "run")) return run(argv[2], argv[3]);
  fprintf(stderr, "usage: %s tables | %s run <in.bin> <out.bin>\n", argv[0], argv[0]);
  return 2;
}
