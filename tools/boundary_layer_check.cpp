// boundary_layer_check.cpp -- the simple boundary layer (climt_amd/csrc/rrtmg_boundary_layer.h: the rule of one column, as one
// thread of boundary_layer_kernel runs it) on the CPU, no device: a stand-alone program for the host sanitizers.
//
//   c++ -std=c++17 -ffp-contract=off -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/boundary_layer_check.cpp -o boundary_layer_check
//
//   boundary_layer_check <ncol> <nlay> <in.bin> <out.bin>
//       in : 14 doubles {in_place (0 / 1), flux_mode, dt, rd, cp, g, lv, karman, z0, fb, p0, ric, pressure_scale, ps_scale},
//            t, q, u, v, pmid [nlay][ncol], pint [nlay+1][ncol], ps, ts, qs, sh_in, lh_in [ncol]
//       out: t', q', u', v' [nlay][ncol], stress_north, stress_east, height, sh, lh [ncol]
//   Every "thread" (column) of the launch the entry would make runs in turn, the last column first.  The program checks that every
//   output element was written, that the guard elements around every array (the work slabs included) are intact, that the inputs
//   of an out-of-place run are untouched, and that the run in place, the run out of place and a run without diagnostics agree
//   bit for bit.  In modes 0 and 1 sh_in and lh_in are not handed over at all (null pointers).
// Exit status 0 and a line that starts with "ok" when everything holds.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../climt_amd/csrc/rrtmg_boundary_layer.h"
#include "check_common.h"

using namespace rrtmg;

constexpr int kHead = 14;

struct Result { std::vector<double> prof[4], diag[5]; };

// one launch on the CPU
static Result run_launch(int ncol, int nlay, bool in_place, bool want_diag, const double *k, const double *in) {
  const size_t n1 = ncol, nl = (size_t)nlay * n1, nl1 = nl + n1, nw = nl - n1;
  const int mode = (int)k[1];
  Guarded prof[4], pm, pi, col[5], out[4], diag[5], wz, wr;
  for (int j = 0; j < 4; ++j) { prof[j].set(in + j * nl, nl); out[j].set(nullptr, nl); }
  pm.set(in + 4 * nl, nl); pi.set(in + 5 * nl, nl1);
  const double *cols = in + 5 * nl + nl1;
  for (int j = 0; j < 5; ++j) { col[j].set(cols + j * n1, n1); diag[j].set(nullptr, n1); }
  wz.set(nullptr, nw); wr.set(nullptr, nw);
  BoundaryLayerCall a{};
  a.ncol = ncol; a.nlay = nlay; a.flux_mode = mode;
  a.t = prof[0].p(); a.q = prof[1].p(); a.u = prof[2].p(); a.v = prof[3].p(); a.pmid = pm.p(); a.pint = pi.p();
  a.ps = col[0].p(); a.ts = col[1].p(); a.qs = col[2].p();
  a.sh_in = mode == 2 ? col[3].p() : nullptr; a.lh_in = mode == 2 ? col[4].p() : nullptr;
  a.dt = k[2]; a.rd = k[3]; a.cp = k[4]; a.g = k[5]; a.lv = k[6]; a.karman = k[7]; a.z0 = k[8]; a.fb = k[9]; a.p0 = k[10]; a.ric = k[11];
  a.pressure_scale = k[12]; a.ps_scale = k[13];
  a.t_out = (in_place ? prof : out)[0].p(); a.q_out = (in_place ? prof : out)[1].p();
  a.u_out = (in_place ? prof : out)[2].p(); a.v_out = (in_place ? prof : out)[3].p();
  if (want_diag) { a.stress_north = diag[0].p(); a.stress_east = diag[1].p(); a.height = diag[2].p(); a.sh_out = diag[3].p(); a.lh_out = diag[4].p(); }
  a.work_z = wz.p(); a.work_rho = wr.p();
  for (int c = ncol - 1; c >= 0; --c) boundary_layer_column(a, c);
  for (int j = 0; j < 4; ++j) { prof[j].check_guards(); out[j].check_guards(); }
  for (int j = 0; j < 5; ++j) { col[j].check_guards(); diag[j].check_guards(); CHECK(col[j].holds(cols + j * n1)); }
  pm.check_guards(); pi.check_guards(); wz.check_guards(); wr.check_guards();
  CHECK(pm.holds(in + 4 * nl) && pi.holds(in + 5 * nl));                                   // only read
  CHECK(wz.written());                                                                      // (work_rho is rewritten in mode 2 only, but filled in pass 1)
  CHECK(wr.written());
  Result r;
  for (int j = 0; j < 4; ++j) {
    if (in_place) CHECK(out[j].untouched());                                                // the other arrays are not touched
    else CHECK(prof[j].holds(in + j * nl));
    Guarded &g = in_place ? prof[j] : out[j];
    CHECK(g.written());
    r.prof[j].assign(g.p(), g.p() + nl);
    for (double x : r.prof[j]) CHECK(std::isfinite(x));
  }
  for (int j = 0; j < 5; ++j) {
    if (want_diag) { CHECK(diag[j].written()); r.diag[j].assign(diag[j].p(), diag[j].p() + n1); }
    else CHECK(diag[j].untouched());
  }
  return r;
}

int main(int argc, char **argv) {
  if (argc != 5) { fprintf(stderr, "usage: %s <ncol> <nlay> <in.bin> <out.bin>\n", argv[0]); return 2; }
  const int ncol = atoi(argv[1]), nlay = atoi(argv[2]);
  CHECK(ncol > 0 && nlay >= 2);
  const std::vector<double> file = read_all(argv[3]);
  const size_t n1 = ncol, nl = (size_t)nlay * n1;
  CHECK(file.size() == kHead + 6 * nl + n1 + 5 * n1);
  const bool in_place = file[0] != 0.0;
  const double *k = file.data(), *in = file.data() + kHead;
  CHECK(k[1] == 0.0 || k[1] == 1.0 || k[1] == 2.0);
  const Result got = run_launch(ncol, nlay, in_place, true, k, in);
  const Result other = run_launch(ncol, nlay, !in_place, true, k, in), bare = run_launch(ncol, nlay, in_place, false, k, in);
  for (int j = 0; j < 4; ++j) CHECK(equal(other.prof[j], got.prof[j]) && equal(bare.prof[j], got.prof[j]));
  for (int j = 0; j < 5; ++j) CHECK(equal(other.diag[j], got.diag[j]));
  std::vector<double> out;
  for (int j = 0; j < 4; ++j) out.insert(out.end(), got.prof[j].begin(), got.prof[j].end());
  for (int j = 0; j < 5; ++j) out.insert(out.end(), got.diag[j].begin(), got.diag[j].end());
  write_all(argv[4], out);
  printf("ok (%d columns, %d layers, flux mode %d%s)\n", ncol, nlay, (int)k[1], in_place ? ", in place" : "");
  return 0;
}
