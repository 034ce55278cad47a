// simple_physics_check.cpp -- the simple physics package (climt_amd/csrc/rrtmg_simple_physics.h: the rule of one column, as one
// thread of simple_physics_kernel runs it) on the CPU, no device: a stand-alone program for the host sanitizers.
//
//   c++ -std=c++17 -ffp-contract=off -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/simple_physics_check.cpp -o simple_physics_check
//
//   simple_physics_check <ncol> <nlay> <in.bin> <out.bin>
//       in : 25 doubles {in_place (0 / 1), do_lsc, do_pbl, do_surf_flux, use_ts_ext, use_qsurf_ext, test, clamp_latent_heat_flux, dt,
//            g, cpair, rair, latvap, rh2o, radius, omega, rhow, pbltop, pblconst, c_heat, cd0, cd1, cm, pressure_scale, ps_scale},
//            t, q, u, v, pmid [nlay][ncol], pint [nlay+1][ncol], ps, ts, qsurf, lat [ncol]
//       out: t', q', u', v' [nlay][ncol], precl, sh, lh [ncol]
//   Every "thread" (column) of the launch the entry would make runs in turn, the last column first.  The program checks that every
//   output element was written, that the guard elements around every array (the work slabs included) are intact, that the inputs
//   of an out-of-place run are untouched, and that the run in place, the run out of place and a run without diagnostics agree
//   bit for bit.  ts, qsurf and lat are not handed over at all (null pointers) where the switches leave them unread, and the work
//   slabs must stay untouched without do_pbl.
// Exit status 0 and a line that starts with "ok" when everything holds.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../climt_amd/csrc/rrtmg_simple_physics.h"
#include "check_common.h"

using namespace rrtmg;

constexpr int kHead = 25;

struct Result { std::vector<double> prof[4], diag[3]; };

// one launch on the CPU
static Result run_launch(int ncol, int nlay, bool in_place, bool want_diag, const double *k, const double *in) {
  const size_t n1 = ncol, nl = (size_t)nlay * n1, nl1 = nl + n1;
  Guarded prof[4], pm, pi, col[4], out[4], diag[3], wce, wcem;
  for (int j = 0; j < 4; ++j) { prof[j].set(in + j * nl, nl); out[j].set(nullptr, nl); }
  pm.set(in + 4 * nl, nl); pi.set(in + 5 * nl, nl1);
  const double *cols = in + 5 * nl + nl1;
  for (int j = 0; j < 4; ++j) col[j].set(cols + j * n1, n1);
  for (int j = 0; j < 3; ++j) diag[j].set(nullptr, n1);
  wce.set(nullptr, nl); wcem.set(nullptr, nl);
  SimplePhysicsCall a{};
  a.ncol = ncol; a.nlay = nlay;
  a.do_lsc = (int)k[1]; a.do_pbl = (int)k[2]; a.do_surf_flux = (int)k[3]; a.use_ts_ext = (int)k[4]; a.use_qsurf_ext = (int)k[5]; a.test = (int)k[6];
  a.clamp_latent_heat_flux = (int)k[7];
  a.t = prof[0].p(); a.q = prof[1].p(); a.u = prof[2].p(); a.v = prof[3].p(); a.pmid = pm.p(); a.pint = pi.p();
  a.ps = col[0].p();
  const bool surf = a.do_surf_flux == 1;
  a.ts = surf && a.use_ts_ext == 1 ? col[1].p() : nullptr;
  a.qsurf = surf && a.use_qsurf_ext == 1 ? col[2].p() : nullptr;
  a.lat = surf && a.use_ts_ext != 1 && a.test == 1 ? col[3].p() : nullptr;
  a.dt = k[8]; a.g = k[9]; a.cpair = k[10]; a.rair = k[11]; a.latvap = k[12]; a.rh2o = k[13]; a.radius = k[14]; a.omega = k[15]; a.rhow = k[16];
  a.pbltop = k[17]; a.pblconst = k[18]; a.c_heat = k[19]; a.cd0 = k[20]; a.cd1 = k[21]; a.cm = k[22];
  a.pressure_scale = k[23]; a.ps_scale = k[24];
  a.t_out = (in_place ? prof : out)[0].p(); a.q_out = (in_place ? prof : out)[1].p();
  a.u_out = (in_place ? prof : out)[2].p(); a.v_out = (in_place ? prof : out)[3].p();
  if (want_diag) { a.precl = diag[0].p(); a.sh_out = diag[1].p(); a.lh_out = diag[2].p(); }
  a.work_ce = wce.p(); a.work_cem = wcem.p();
  for (int c = ncol - 1; c >= 0; --c) simple_physics_column(a, c);
  for (int j = 0; j < 4; ++j) { prof[j].check_guards(); out[j].check_guards(); col[j].check_guards(); CHECK(col[j].holds(cols + j * n1)); }
  for (int j = 0; j < 3; ++j) diag[j].check_guards();
  pm.check_guards(); pi.check_guards(); wce.check_guards(); wcem.check_guards();
  CHECK(pm.holds(in + 4 * nl) && pi.holds(in + 5 * nl));                                   // only read
  if (a.do_pbl == 1) CHECK(wce.written() && wcem.written());
  else CHECK(wce.untouched() && wcem.untouched());
  Result r;
  for (int j = 0; j < 4; ++j) {
    if (in_place) CHECK(out[j].untouched());                                                // the other arrays are not touched
    else CHECK(prof[j].holds(in + j * nl));
    Guarded &g = in_place ? prof[j] : out[j];
    CHECK(g.written());
    r.prof[j].assign(g.p(), g.p() + nl);
    for (double x : r.prof[j]) CHECK(std::isfinite(x));
  }
  for (int j = 0; j < 3; ++j) {
    if (want_diag) { CHECK(diag[j].written()); r.diag[j].assign(diag[j].p(), diag[j].p() + n1); }
    else CHECK(diag[j].untouched());
  }
  return r;
}

int main(int argc, char **argv) {
  if (argc != 5) { fprintf(stderr, "usage: %s <ncol> <nlay> <in.bin> <out.bin>\n", argv[0]); return 2; }
  const int ncol = atoi(argv[1]), nlay = atoi(argv[2]);
  CHECK(ncol > 0 && nlay >= 1);
  const std::vector<double> file = read_all(argv[3]);
  const size_t n1 = ncol, nl = (size_t)nlay * n1;
  CHECK(file.size() == kHead + 6 * nl + n1 + 4 * n1);
  const bool in_place = file[0] != 0.0;
  const double *k = file.data(), *in = file.data() + kHead;
  for (int j = 1; j <= 7; ++j) CHECK(k[j] == 0.0 || k[j] == 1.0);
  CHECK(!(k[2] == 1.0 && k[3] != 1.0));      // do_pbl needs do_surf_flux: the entry refuses it
  const Result got = run_launch(ncol, nlay, in_place, true, k, in);
  const Result other = run_launch(ncol, nlay, !in_place, true, k, in), bare = run_launch(ncol, nlay, in_place, false, k, in);
  for (int j = 0; j < 4; ++j) CHECK(equal(other.prof[j], got.prof[j]) && equal(bare.prof[j], got.prof[j]));
  for (int j = 0; j < 3; ++j) CHECK(equal(other.diag[j], got.diag[j]));
  std::vector<double> out;
  for (int j = 0; j < 4; ++j) out.insert(out.end(), got.prof[j].begin(), got.prof[j].end());
  for (int j = 0; j < 3; ++j) out.insert(out.end(), got.diag[j].begin(), got.diag[j].end());
  write_all(argv[4], out);
  printf("ok (%d columns, %d layers, lsc %d, pbl %d, surface %d%s)\n", ncol, nlay, (int)k[1], (int)k[2], (int)k[3], in_place ? ", in place" : "");
  return 0;
}
