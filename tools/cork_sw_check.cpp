// cork_sw_check.cpp -- the table-driven correlated-k two-stream shortwave (climt_amd/csrc/rrtmg_cork_sw.h: the rules of one (column, band)
// as one thread of cork_sw_band_kernel runs them, and the longwave's cork_broadband behind them) and the host side of rrtmg_cork_sw.hip
// (the row table, the checks of a table's description and of a call) on the CPU, no device: a stand-alone program for
// tests/test_cork_sw.py and the host sanitizers.
//
//   c++ -std=c++17 -ffp-contract=off -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/cork_sw_check.cpp -o cork_sw_check
//
//   cork_sw_check tables
//       The rows of the entry's table as tools/column_table_check.h prints them, its checks of the staging plan and the aliasing
//       refusals, then the refusals of a shortwave table's description and of a call, and the chunk rule.  Last line "ok".
//   cork_sw_check layer <in.bin> <out.bin>
//       in : rows of 4 doubles {tau, ssa, g, mu0}.  out: rows of 9 doubles {tau_s, ssa_s, g_s, Rdif, Tdif, Rdir, Tdir, Tnoscat, guard},
//       guard 1.0 where |1 - (k mu0)^2| < 1e-30 was taken: cork_sw_delta_scale and cork_sw_layer driven directly.
//   cork_sw_check run <in.bin> <out.bin>
//       in : 40 doubles {ncol, nlay, gas_rule, ngas, nband, ngpt, nT, nP, nX, k_is_f32, has_cont, has_cloud, has_rayleigh, solar_is_f32,
//            max_chunk_cols, gas_scale[8], m_h2o, g, cpd, pressure_scale, 0, 0, 0, 0, x_clip[2], null_outputs, 0...}, then k (the reference's layout, as doubles),
//            weights, solar [nband][ngpt], rayleigh [nband] (with has_rayleigh), t_grid, p_grid_log, x_grid_log, log_cont, then t, pmid
//            [nlay][ncol], pint [nlay+1][ncol], zenith, albedo, earth_sun [ncol], taucld, ssacld, asycld [nlay][ncol][nband] (with
//            has_cloud), the gas arrays the rule reads
//       out: up, dn [nlay+1][ncol], tend, hr [nlay][ncol], up_band, dn_band [nband][nlay+1][ncol], tau_band, hr_band [nband][nlay][ncol]
//       The columns run in the chunks the entry would make (cork_sw_chunk_cols), one work space of exactly the entry's size on the
//       heap, every "thread" of a launch in turn, the last column first; then the band reduction.  The run without the optional
//       outputs must agree bit for bit.  With null_outputs (slot 33) not 0 that run is the only one: the kernel function gets NULL
//       for hr, tau_band and hr_band and, for up_band and dn_band, buffers of the program's own as the entry hands it its own, and
//       out holds up, dn and tend alone -- an absent output is written as nothing.  The program checks that every output element was written, that the guard elements around
//       every array are intact and that the inputs are untouched.
// Exit status 0 and a last line that starts with "ok" when everything holds.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../climt_amd/csrc/rrtmg_cork_sw.hip"
#include "column_table_check.h"

using namespace rrtmg;

static int tables() {
  const ColumnTable &t = kCorkShortwave;
  print_table(t);
  ColumnMask optional_out = 0;
  for (int i = 0; i < t.n; ++i) {
    CHECK(!t.rows[i].in_place_of && !t.rows[i].i32);
    if (t.rows[i].out && !t.rows[i].required) optional_out |= ColumnMask(1) << i;
  }
  check_plan(t, {1, 3}, optional_out | column_bits(t, {"gas0", "taucld"}));
  check_aliasing<rrtmg_cork_shortwave>(t, "", "t, pmid, pint, zenith, albedo, earth_sun, up, dn and tend must be given", 3);

  // the description of a shortwave table
  const double grid[3] = {1.0, 2.0, 3.0}, flat[3] = {1.0, 2.0, 2.0}, k[64] = {0.0};
  rrtmg_cork_sw_table_desc d{};
  d.ngas = 1; d.nband = 2; d.ngpt = 2; d.nT = 3; d.nP = 3; d.k = k; d.weights = k; d.t_grid = grid; d.p_grid_log = grid; d.solar_source = k;
  CHECK(!cork_sw_table_refusal(d));
  auto refused = [&](auto change) { rrtmg_cork_sw_table_desc e = d; change(e); return cork_sw_table_refusal(e) != nullptr; };
  CHECK(refused([](auto &e) { e.nC = 2; }) && refused([](auto &e) { e.solar_source = nullptr; }) && refused([](auto &e) { e.solar_is_f32 = 2; }));
  CHECK(refused([](auto &e) { e.ngpt = 17; }) && refused([](auto &e) { e.k = nullptr; }) && refused([&](auto &e) { e.t_grid = flat; }) && refused([&](auto &e) { e.log_cont = k; }));
  CHECK(refused([](auto &e) { e.nX = 3; }) && !refused([&](auto &e) { e.nX = 3; e.x_grid_log = grid; e.x_clip[1] = 1.0; }) && !refused([&](auto &e) { e.rayleigh = k; }));

  // a call
  rrtmg_cork_shortwave a{};
  CHECK(!cork_sw_call_refusal(a) && !cork_gas_refusal(a, 1, 0, 0));
  a.max_chunk_cols = -1; CHECK(cork_sw_call_refusal(a)); a.max_chunk_cols = 0;
  a.taucld = grid; CHECK(cork_sw_call_refusal(a)); a.ssacld = grid; CHECK(cork_sw_call_refusal(a)); a.asycld = grid; CHECK(!cork_sw_call_refusal(a));
  a.gas_rule = 2; CHECK(cork_gas_refusal(a, 1, 0, 0)); a.gas0 = grid; CHECK(!cork_gas_refusal(a, 1, 0, 0) && cork_gas_refusal(a, 1, 3, 0));
  const int g0 = column_index(t, "gas0");
  CHECK(cork_unread(t, 0, 1, 0, 0) == ColumnMask(0xff) << g0 && cork_unread(t, 2, 2, 0, 0) == ColumnMask(0xfc) << g0 && cork_unread(t, 1, 1, 3, 0) == ColumnMask(0xfe) << g0);

  // the chunks: whole waves under the cap, at least one wave, the caller's bound below that, never more than the call has
  CHECK(cork_sw_chunk_cols(3, 2, 30, 130, 0) == 130 && cork_sw_chunk_cols(3, 2, 30, 130, 64) == 64 && cork_sw_chunk_cols(3, 2, 30, 130, 1) == 1);
  const size_t big = cork_sw_chunk_cols(32, 16, 200, (size_t)1 << 30, 0);
  CHECK(big % 64 == 0 && big >= 64 && big * cork_sw_work_per_column(32, 16, 200) <= kCorkSwWorkCap && (big + 64) * cork_sw_work_per_column(32, 16, 200) > kCorkSwWorkCap);
  CHECK(cork_sw_chunk_cols(32, 16, 1 << 20, 1000, 0) == 64);
  printf("ok\n");
  return 0;
}

static int layer(const char *in, const char *out) {
  const std::vector<double> file = read_all(in);
  CHECK(file.size() % 4 == 0 && !file.empty());
  std::vector<double> result;
  for (size_t i = 0; i < file.size(); i += 4) {
    double ts, ws, gs;
    cork_sw_delta_scale(file[i], file[i + 1], file[i + 2], ts, ws, gs);
    const CorkSwLayer L = cork_sw_layer(ts, ws, gs, file[i + 3]);
    CHECK(L.Tnoscat == cork_sw_tnoscat(ts, file[i + 3]));      // the beam pass forms the same bits
    // whether the guard is taken, from the same operations (contraction is off for the whole program)
    const double g1 = (8.0 - ws * (5.0 + 3.0 * gs)) * 0.25, g2 = 3.0 * (ws * (1.0 - gs)) * 0.25, k2 = (g1 - g2) * (g1 + g2);
    const double k = sqrt(kCorkSwMinK > k2 ? kCorkSwMinK : k2), mu = kCorkSwMinMu0 > file[i + 3] ? kCorkSwMinMu0 : file[i + 3], kmu = k * mu;
    for (double v : {ts, ws, gs, L.Rdif, L.Tdif, L.Rdir, L.Tdir, L.Tnoscat, fabs(1.0 - kmu * kmu) < 1e-30 ? 1.0 : 0.0}) result.push_back(v);
  }
  FILE *f = fopen(out, "wb");
  CHECK(f != nullptr && fwrite(result.data(), sizeof(double), result.size(), f) == result.size());
  fclose(f);
  printf("ok (cork_sw layer, %zu rows)\n", file.size() / 4);
  return 0;
}

template <class K>
static void run_bands(const CorkShortwaveCall &c) {
  for (int b = c.tab.nband - 1; b >= 0; --b)
    for (long col = c.col0 + c.cols - 1; col >= c.col0; --col) {
      const int n = c.tab.ngpt;
      if (n <= 1) cork_sw_band_column<1, K>(c, col, b);
      else if (n <= 2) cork_sw_band_column<2, K>(c, col, b);
      else if (n <= 4) cork_sw_band_column<4, K>(c, col, b);
      else if (n <= 8) cork_sw_band_column<8, K>(c, col, b);
      else cork_sw_band_column<16, K>(c, col, b);
    }
}

static int run(const char *in, const char *out) {
  const std::vector<double> file = read_all(in);
  CHECK(file.size() > 40);
  const double *h = file.data();
  rrtmg_cork_sw_table_desc sd{};
  const int ncol = (int)h[0], nlay = (int)h[1], rule = (int)h[2];
  sd.ngas = (int)h[3]; sd.nband = (int)h[4]; sd.ngpt = (int)h[5]; sd.nT = (int)h[6]; sd.nP = (int)h[7]; sd.nX = (int)h[8]; sd.k_is_f32 = (int)h[9];
  const bool has_cont = h[10] != 0.0, has_cloud = h[11] != 0.0, has_ray = h[12] != 0.0;
  sd.solar_is_f32 = (int)h[13];
  const size_t max_chunk = (size_t)h[14];
  const bool null_outputs = h[33] != 0.0;
  CHECK(ncol > 0 && nlay >= 1);
  rrtmg_cork_table_desc d = cork_sw_common_desc(sd);
  const size_t nk = cork_k_count(d), nw = (size_t)d.nband * d.ngpt, ncont = has_cont ? (size_t)d.nband * d.nT * d.nP * d.nX : 0;
  const double *p = h + 40;
  const double *k = p; p += nk;
  const double *weights = p; p += nw;
  const double *solar = p; p += nw;
  const double *rayleigh = has_ray ? p : nullptr; p += has_ray ? d.nband : 0;
  const double *t_grid = p; p += d.nT;
  const double *p_grid = p; p += d.nP;
  const double *x_grid = d.nX ? p : nullptr; p += d.nX;
  const double *log_cont = ncont ? p : nullptr; p += ncont;
  std::vector<float> solar_f(nw);
  for (size_t i = 0; i < nw; ++i) { solar_f[i] = (float)solar[i]; if (sd.solar_is_f32) CHECK((double)solar_f[i] == solar[i]); }
  sd.k = k; sd.weights = weights; sd.t_grid = t_grid; sd.p_grid_log = p_grid; sd.x_grid_log = x_grid; sd.log_cont = log_cont;
  sd.x_clip[0] = h[31]; sd.x_clip[1] = h[32];
  sd.solar_source = sd.solar_is_f32 ? (const void *)solar_f.data() : (const void *)solar; sd.rayleigh = rayleigh;
  CHECK(cork_sw_table_refusal(sd) == nullptr);
  d = cork_sw_common_desc(sd);

  std::vector<double> kd(nk);
  std::vector<float> kf(nk), kf_src(nk);
  if (d.k_is_f32) {
    for (size_t i = 0; i < nk; ++i) { kf_src[i] = (float)k[i]; CHECK((double)kf_src[i] == k[i]); }
    cork_relayout(d, kf_src.data(), kf.data());
  } else cork_relayout(d, k, kd.data());

  const size_t n1 = ncol, nl = (size_t)nlay * n1, nl1 = nl + n1, nb = d.nband;
  const double *t = p, *pmid = t + nl, *pint = pmid + nl, *zen = pint + nl1, *alb = zen + n1, *esf = alb + n1, *cloud = esf + n1, *gases = cloud + (has_cloud ? 3 * nl * nb : 0);
  rrtmg_cork_shortwave pub{};
  pub.gas_rule = rule;
  const double *gp[kCorkMaxGas] = {};
  const ColumnMask unread = cork_unread(kCorkShortwave, rule, d.ngas, d.nX, 0);
  size_t ngiven = 0;
  for (int i = 0; i < kCorkMaxGas; ++i)
    if (!(unread >> (column_index(kCorkShortwave, "gas0") + i) & 1)) gp[i] = gases + nl * ngiven++;
  CHECK((size_t)(gases + nl * ngiven - h) == file.size());
  pub.gas0 = gp[0]; pub.gas1 = gp[1]; pub.gas2 = gp[2]; pub.gas3 = gp[3]; pub.gas4 = gp[4]; pub.gas5 = gp[5]; pub.gas6 = gp[6]; pub.gas7 = gp[7];
  CHECK(cork_gas_refusal(pub, d.ngas, d.nX, 0) == nullptr);

  const size_t chunk = cork_sw_chunk_cols(nb, (size_t)d.ngpt, (size_t)nlay, n1, max_chunk);
  size_t launches = 0;
  std::vector<double> result;
  for (int pass = null_outputs ? 1 : 0; pass < 2; ++pass) {      // with every optional output, then with none
    Guarded gt, gpm, gpi, gz, ga, ge, gc[3], gg[kCorkMaxGas], up, dn, tend, hr, ub, db, tb, hb;
    gt.set(t, nl); gpm.set(pmid, nl); gpi.set(pint, nl1); gz.set(zen, n1); ga.set(alb, n1); ge.set(esf, n1);
    for (int i = 0; i < 3; ++i) gc[i].set(has_cloud ? cloud + i * nl * nb : nullptr, has_cloud ? nl * nb : 0);
    for (int i = 0; i < kCorkMaxGas; ++i) gg[i].set(gp[i], gp[i] ? nl : 0);
    up.set(nullptr, nl1); dn.set(nullptr, nl1); tend.set(nullptr, nl); hr.set(nullptr, nl);
    ub.set(nullptr, nb * nl1); db.set(nullptr, nb * nl1); tb.set(nullptr, nb * nl); hb.set(nullptr, nb * nl);
    // the work space: exactly the entry's size, on the heap, so that an index past it is the sanitizer's finding
    std::vector<double> work(cork_sw_work_per_column(nb, (size_t)d.ngpt, (size_t)nlay) / sizeof(double) * chunk, kPoison);
    CorkShortwaveCall c{};
    c.ncol = ncol; c.nlay = nlay; c.gas_rule = rule; c.solar_f32 = sd.solar_is_f32;
    CorkTableView &v = c.tab;
    v.ngas = d.ngas; v.nband = d.nband; v.ngpt = d.ngpt; v.nT = d.nT; v.nP = d.nP; v.nX = d.nX; v.nC = 0; v.k_f32 = d.k_is_f32; v.has_cont = ncont && rule == 1 ? 1 : 0;
    v.k = d.k_is_f32 ? (const void *)kf.data() : (const void *)kd.data();
    v.weights = weights; v.planck = nullptr; v.t_grid = t_grid; v.p_grid = p_grid; v.x_grid = x_grid; v.c_grid = nullptr; v.log_cont = log_cont;
    v.x_lo = sd.x_clip[0]; v.x_hi = sd.x_clip[1];
    c.solar = solar; c.rayleigh = rayleigh;
    c.t = gt.p(); c.pmid = gpm.p(); c.pint = gpi.p(); c.zenith = gz.p(); c.albedo = ga.p(); c.earth_sun = ge.p();
    if (has_cloud) { c.taucld = gc[0].p(); c.ssacld = gc[1].p(); c.asycld = gc[2].p(); }
    const double *bound[kCorkMaxGas];
    for (int i = 0; i < kCorkMaxGas; ++i) bound[i] = gp[i] ? gg[i].p() : nullptr;
    c.gas0 = bound[0]; c.gas1 = bound[1]; c.gas2 = bound[2]; c.gas3 = bound[3]; c.gas4 = bound[4]; c.gas5 = bound[5]; c.gas6 = bound[6]; c.gas7 = bound[7];
    for (int i = 0; i < kCorkMaxGas; ++i) c.gas_scale[i] = h[15 + i];
    c.m_h2o = h[23]; c.g = h[24]; c.cpd = h[25]; c.pressure_scale = h[26];
    c.up = up.p(); c.dn = dn.p(); c.tend = tend.p(); c.up_band = ub.p(); c.dn_band = db.p();
    if (pass == 0) { c.hr = hr.p(); c.tau_band = tb.p(); c.hr_band = hb.p(); }
    c.work = work.data(); c.work_cols = (int64_t)chunk;
    launches = 0;
    for (size_t col0 = 0; col0 < n1; col0 += chunk, ++launches) {      // the chunks, as the entry makes them
      c.col0 = (int64_t)col0; c.cols = (int64_t)(n1 - col0 < chunk ? n1 - col0 : chunk);
      if (d.k_is_f32) run_bands<float>(c); else run_bands<double>(c);
    }
    CorkLongwaveCall bb{};
    bb.ncol = c.ncol; bb.nlay = c.nlay; bb.tab.nband = d.nband; bb.pint = c.pint; bb.g = c.g; bb.cpd = c.cpd; bb.pressure_scale = c.pressure_scale;
    bb.up = c.up; bb.dn = c.dn; bb.tend = c.tend; bb.hr = c.hr; bb.up_band = c.up_band; bb.dn_band = c.dn_band;
    for (int lev = nlay; lev >= 0; --lev)
      for (int col = ncol - 1; col >= 0; --col) cork_broadband(bb, col, lev);
    for (Guarded *g : {&gt, &gpm, &gpi, &gz, &ga, &ge, &gc[0], &gc[1], &gc[2], &up, &dn, &tend, &hr, &ub, &db, &tb, &hb}) g->check_guards();
    for (int i = 0; i < kCorkMaxGas; ++i) { gg[i].check_guards(); CHECK(!gp[i] || gg[i].holds(gp[i])); }
    CHECK(gt.holds(t) && gpm.holds(pmid) && gpi.holds(pint) && gz.holds(zen) && ga.holds(alb) && ge.holds(esf));      // only read
    for (int i = 0; i < 3; ++i) CHECK(!has_cloud || gc[i].holds(cloud + i * nl * nb));
    CHECK(up.written() && dn.written() && tend.written() && ub.written() && db.written());
    std::vector<double> o;
    for (Guarded *g : {&up, &dn, &tend}) o.insert(o.end(), g->p(), g->p() + g->n);
    for (size_t i = 0; i < n1; ++i)      // a dark column: +0.0 in every flux
      if (cos(zen[i]) <= kCorkSwNight)
        for (size_t lev = 0; lev <= (size_t)nlay; ++lev) CHECK(up.p()[lev * n1 + i] == 0.0 && !std::signbit(up.p()[lev * n1 + i]) && dn.p()[lev * n1 + i] == 0.0 && !std::signbit(dn.p()[lev * n1 + i]));
    if (pass == 0) {
      CHECK(hr.written() && tb.written() && hb.written());
      for (size_t i = 0; i < nl; ++i) CHECK(hr.p()[i] == tend.p()[i] * 86400.0);
      result = o;
      for (Guarded *g : {&hr, &ub, &db, &tb, &hb}) result.insert(result.end(), g->p(), g->p() + g->n);
    } else {
      CHECK(hr.untouched() && tb.untouched() && hb.untouched());
      if (null_outputs) result = o;
      else CHECK(memcmp(o.data(), result.data(), o.size() * sizeof(double)) == 0);      // the optional outputs change no bit of the others
    }
  }
  FILE *f = fopen(out, "wb");
  CHECK(f != nullptr && fwrite(result.data(), sizeof(double), result.size(), f) == result.size());
  fclose(f);
  printf("ok (cork_sw, %d columns in %zu chunks, %d layers, %d bands, %d g-points, rank %d, rule %d%s)\n", ncol, launches, nlay, d.nband, d.ngpt, 5 + (d.nX > 0), rule,
         null_outputs ? ", no optional outputs" : "");
  return 0;
}

int main(int argc, char **argv) {
  if (argc == 2 && !strcmp(argv[1], "tables")) return tables();
  if (argc == 4 && !strcmp(argv[1], "layer")) return layer(argv[2], argv[3]);
  if (argc == 4 && !strcmp(argv[1], "run")) return run(argv[2], argv[3]);
  fprintf(stderr, "usage: %s tables | %s layer <in.bin> <out.bin> | %s run <in.bin> <out.bin>\n", argv[0], argv[0], argv[0]);
  return 2;
}
