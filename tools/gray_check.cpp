// gray_check.cpp -- the gray radiation path (climt_amd/csrc/rrtmg_gray.h: the rules of one column, as one thread of frierson_kernel,
// gray_longwave_kernel and grid_scale_condensation_kernel runs them) and the three tables at the head of rrtmg_gray.hip on the CPU,
// no device: a stand-alone program for tests/test_gray.py and the host sanitizers.
//
//   c++ -std=c++17 -ffp-contract=off -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/gray_check.cpp -o gray_check
//
//   gray_check tables
//       Line: <entry> <in|out> <struct> <member> <extent> <f64|i32> <required or -> <the input it may be, or ->   (the format of
//       tools/column_call_check.cpp), then for every table the checks of tools/column_table_check.h: the staging plan at ncol 1, 63,
//       64, 65 x nlay 1, 2, 61 x every combination of optional rows, the aliasing refusals with made-up addresses and the "must be
//       given" text.  Last line "ok".
//   gray_check frierson <ncol> <nlay> <in.bin> <out.bin>
//       in : 5 doubles {tau0e, tau0p, fl, pressure_scale, ps_scale}, pint [nlay+1][ncol], ps, lat [ncol];  out: tau [nlay+1][ncol]
//   gray_check gray <ncol> <nlay> <in.bin> <out.bin>
//       in : 9 doubles {frierson (0 / 1), tau0e, tau0p, fl, sigma_sb, g, cpd, pressure_scale, ps_scale}, t [nlay][ncol], tsfc [ncol],
//            pint, tau [nlay+1][ncol], ps, lat [ncol];  out: up, dn [nlay+1][ncol], tend, hr [nlay][ncol], tau_out [nlay+1][ncol]
//       The arrays the switch leaves unread are not handed over at all (null pointers).  The run without hr and tau_out must agree
//       bit for bit, and with frierson 1 so must the optical depth followed by the sweep on its output, tau_out being that depth.
//   gray_check gsc <ncol> <nlay> <in.bin> <out.bin>
//       in : 8 doubles {in_place (0 / 1), cpd, lv, rd, rh2o, g, rhow, pressure_scale}, t, q, pmid [nlay][ncol], pint [nlay+1][ncol]
//       out: t', q' [nlay][ncol], precip [ncol].  In place, out of place and without precip must agree bit for bit.
//   Every "thread" (column) of the launch the entry would make runs in turn, the last column first.  The program checks that every
//   output element was written, that the guard elements around every array are intact and that the inputs are untouched.
// Exit status 0 and a last line that starts with "ok" when everything holds.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../climt_amd/csrc/rrtmg_gray.hip"
#include "column_table_check.h"

using namespace rrtmg;

// ---- the tables ------------------------------------------------------------------------------------------------------------------
static int tables() {
  print_table(kFrierson); print_table(kGrayLongwave); print_table(kGridScaleCondensation);
  check_plan(kFrierson); check_plan(kGrayLongwave); check_plan(kGridScaleCondensation);
  check_aliasing<rrtmg_frierson_optical_depth>(kFrierson, "", "pint, ps, lat and tau must be given");
  check_aliasing<rrtmg_gray_longwave>(kGrayLongwave, "", "t, tsfc, pint, up, dn and tend must be given");
  check_aliasing<rrtmg_grid_scale_condensation>(kGridScaleCondensation, " (in place: exactly its own input)", "t, q, pmid, pint, t_out and q_out must be given");
  static_assert(column_bits(kGrayLongwave, {"tau"}) == ColumnMask(1) << 3 && column_bits(kGrayLongwave, {"ps", "lat"}) == (ColumnMask(1) << 4 | ColumnMask(1) << 5), "the bits of the named rows");
  printf("ok\n");
  return 0;
}

// ---- the rules -------------------------------------------------------------------------------------------------------------------

static std::vector<double> run_frierson(int ncol, int nlay, const double *k, const double *pint, const double *ps, const double *lat) {
  const size_t n1 = ncol, nl1 = (size_t)(nlay + 1) * n1;
  Guarded gp, gs, gl, tau;
  gp.set(pint, nl1); gs.set(ps, n1); gl.set(lat, n1); tau.set(nullptr, nl1);
  FriersonCall a{};
  a.ncol = ncol; a.nlay = nlay; a.pint = gp.p(); a.ps = gs.p(); a.lat = gl.p();
  a.tau0e = k[0]; a.tau0p = k[1]; a.fl = k[2]; a.pressure_scale = k[3]; a.ps_scale = k[4];
  a.tau = tau.p();
  for (int c = ncol - 1; c >= 0; --c) frierson_column(a, c);
  gp.check_guards(); gs.check_guards(); gl.check_guards(); tau.check_guards();
  CHECK(gp.holds(pint) && gs.holds(ps) && gl.holds(lat) && tau.written());
  return tau.get();
}

static int frierson(int ncol, int nlay, const char *in, const char *out) {
  const std::vector<double> file = read_all(in);
  const size_t n1 = ncol, nl1 = (size_t)(nlay + 1) * n1;
  CHECK(file.size() == 5 + nl1 + 2 * n1);
  const double *k = file.data(), *pint = k + 5;
  write_all(out, run_frierson(ncol, nlay, k, pint, pint + nl1, pint + nl1 + n1));
  printf("ok (frierson, %d columns, %d layers)\n", ncol, nlay);
  return 0;
}

struct GrayResult { std::vector<double> up, dn, tend, hr, tau_out; };

// one launch on the CPU; tau: the depth the sweep reads without `fused`
static GrayResult run_gray(int ncol, int nlay, bool fused, bool want_diag, const double *k, const double *t, const double *tsfc, const double *pint,
                           const double *tau, const double *ps, const double *lat) {
  const size_t n1 = ncol, nl = (size_t)nlay * n1, nl1 = nl + n1;
  Guarded gt, gts, gp, gtau, gps, glat, up, dn, tend, hr, tau_out;
  gt.set(t, nl); gts.set(tsfc, n1); gp.set(pint, nl1); gtau.set(tau, nl1); gps.set(ps, n1); glat.set(lat, n1);
  up.set(nullptr, nl1); dn.set(nullptr, nl1); tend.set(nullptr, nl); hr.set(nullptr, nl); tau_out.set(nullptr, nl1);
  GrayLongwaveCall a{};
  a.ncol = ncol; a.nlay = nlay; a.frierson = fused ? 1 : 0;
  a.t = gt.p(); a.tsfc = gts.p(); a.pint = gp.p();
  a.tau = fused ? nullptr : gtau.p();
  a.ps = fused ? gps.p() : nullptr; a.lat = fused ? glat.p() : nullptr;
  a.tau0e = k[1]; a.tau0p = k[2]; a.fl = k[3]; a.sigma_sb = k[4]; a.g = k[5]; a.cpd = k[6]; a.pressure_scale = k[7]; a.ps_scale = k[8];
  a.up = up.p(); a.dn = dn.p(); a.tend = tend.p();
  if (want_diag) { a.hr = hr.p(); a.tau_out = tau_out.p(); }
  for (int c = ncol - 1; c >= 0; --c) gray_longwave_column(a, c);
  for (Guarded *g : {&gt, &gts, &gp, &gtau, &gps, &glat, &up, &dn, &tend, &hr, &tau_out}) g->check_guards();
  CHECK(gt.holds(t) && gts.holds(tsfc) && gp.holds(pint) && gtau.holds(tau) && gps.holds(ps) && glat.holds(lat));      // only read
  CHECK(up.written() && dn.written() && tend.written());
  GrayResult r{up.get(), dn.get(), tend.get(), {}, {}};
  if (want_diag) { CHECK(hr.written() && tau_out.written()); r.hr = hr.get(); r.tau_out = tau_out.get(); }
  else CHECK(hr.untouched() && tau_out.untouched());
  return r;
}

static int gray(int ncol, int nlay, const char *in, const char *out) {
  const std::vector<double> file = read_all(in);
  const size_t n1 = ncol, nl = (size_t)nlay * n1, nl1 = nl + n1;
  CHECK(file.size() == 9 + nl + n1 + 2 * nl1 + 2 * n1);
  const double *k = file.data(), *t = k + 9, *tsfc = t + nl, *pint = tsfc + n1, *tau = pint + nl1, *ps = tau + nl1, *lat = ps + n1;
  CHECK(k[0] == 0.0 || k[0] == 1.0);
  const bool fused = k[0] == 1.0;
  const GrayResult got = run_gray(ncol, nlay, fused, true, k, t, tsfc, pint, tau, ps, lat), bare = run_gray(ncol, nlay, fused, false, k, t, tsfc, pint, tau, ps, lat);
  CHECK(equal(bare.up, got.up) && equal(bare.dn, got.dn) && equal(bare.tend, got.tend));
  for (size_t i = 0; i < nl; ++i) CHECK(got.hr[i] == got.tend[i] * 86400.0 || (got.hr[i] != got.hr[i] && got.tend[i] != got.tend[i]));
  if (fused) {      // the depth, then the sweep on it: every output the same bits
    const double kf[5] = {k[1], k[2], k[3], k[7], k[8]};
    const std::vector<double> depth = run_frierson(ncol, nlay, kf, pint, ps, lat);
    const GrayResult two = run_gray(ncol, nlay, false, true, k, t, tsfc, pint, depth.data(), ps, lat);
    CHECK(equal(depth, got.tau_out) && equal(two.tau_out, depth));
    CHECK(equal(two.up, got.up) && equal(two.dn, got.dn) && equal(two.tend, got.tend) && equal(two.hr, got.hr));
  } else {
    CHECK(memcmp(got.tau_out.data(), tau, nl1 * sizeof(double)) == 0);
  }
  std::vector<double> o;
  for (const std::vector<double> *v : {&got.up, &got.dn, &got.tend, &got.hr, &got.tau_out}) o.insert(o.end(), v->begin(), v->end());
  write_all(out, o);
  printf("ok (gray, %d columns, %d layers%s)\n", ncol, nlay, fused ? ", fused" : "");
  return 0;
}

struct GscResult { std::vector<double> t, q, precip; };

static GscResult run_gsc(int ncol, int nlay, bool in_place, bool want_precip, const double *k, const double *in) {
  const size_t n1 = ncol, nl = (size_t)nlay * n1, nl1 = nl + n1;
  Guarded t, q, pm, pi, t_out, q_out, precip;
  t.set(in, nl); q.set(in + nl, nl); pm.set(in + 2 * nl, nl); pi.set(in + 3 * nl, nl1);
  t_out.set(nullptr, nl); q_out.set(nullptr, nl); precip.set(nullptr, n1);
  GridScaleCondensationCall a{};
  a.ncol = ncol; a.nlay = nlay; a.t = t.p(); a.q = q.p(); a.pmid = pm.p(); a.pint = pi.p();
  a.cpd = k[1]; a.lv = k[2]; a.rd = k[3]; a.rh2o = k[4]; a.g = k[5]; a.rhow = k[6]; a.pressure_scale = k[7];
  a.t_out = in_place ? t.p() : t_out.p(); a.q_out = in_place ? q.p() : q_out.p();
  if (want_precip) a.precip = precip.p();
  for (int c = ncol - 1; c >= 0; --c) grid_scale_condensation_column(a, c);
  for (Guarded *g : {&t, &q, &pm, &pi, &t_out, &q_out, &precip}) g->check_guards();
  CHECK(pm.holds(in + 2 * nl) && pi.holds(in + 3 * nl));
  if (in_place) CHECK(t_out.untouched() && q_out.untouched());
  else CHECK(t.holds(in) && q.holds(in + nl) && t_out.written() && q_out.written());
  GscResult r{(in_place ? t : t_out).get(), (in_place ? q : q_out).get(), {}};
  if (want_precip) { CHECK(precip.written()); r.precip = precip.get(); }
  else CHECK(precip.untouched());
  return r;
}

static int gsc(int ncol, int nlay, const char *in, const char *out) {
  const std::vector<double> file = read_all(in);
  const size_t n1 = ncol, nl = (size_t)nlay * n1;
  CHECK(file.size() == 8 + 4 * nl + n1);
  const double *k = file.data();
  CHECK(k[0] == 0.0 || k[0] == 1.0);
  const bool in_place = k[0] == 1.0;
  const GscResult got = run_gsc(ncol, nlay, in_place, true, k, k + 8), other = run_gsc(ncol, nlay, !in_place, true, k, k + 8), bare = run_gsc(ncol, nlay, in_place, false, k, k + 8);
  CHECK(equal(other.t, got.t) && equal(other.q, got.q) && equal(other.precip, got.precip) && equal(bare.t, got.t) && equal(bare.q, got.q));
  std::vector<double> o;
  for (const std::vector<double> *v : {&got.t, &got.q, &got.precip}) o.insert(o.end(), v->begin(), v->end());
  write_all(out, o);
  printf("ok (gsc, %d columns, %d layers%s)\n", ncol, nlay, in_place ? ", in place" : "");
  return 0;
}

int main(int argc, char **argv) {
  if (argc == 2 && !strcmp(argv[1], "tables")) return tables();
  if (argc != 6) { fprintf(stderr, "usage: %s tables | %s frierson|gray|gsc <ncol> <nlay> <in.bin> <out.bin>\n", argv[0], argv[0]); return 2; }
  const int ncol = atoi(argv[2]), nlay = atoi(argv[3]);
  CHECK(ncol > 0 && nlay >= 1);
  if (!strcmp(argv[1], "frierson")) return frierson(ncol, nlay, argv[4], argv[5]);
  if (!strcmp(argv[1], "gray")) return gray(ncol, nlay, argv[4], argv[5]);
  if (!strcmp(argv[1], "gsc")) return gsc(ncol, nlay, argv[4], argv[5]);
  fprintf(stderr, "%s: no mode %s\n", argv[0], argv[1]);
  return 2;
}
