// emanuel_check.cpp -- the Emanuel convection scheme (climt_amd/csrc/rrtmg_emanuel.h: the rule of one column, as one thread of
// emanuel_kernel runs it) on the CPU, no device: a stand-alone program for the host sanitizers.
//
//   c++ -std=c++17 -ffp-contract=off -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/emanuel_check.cpp -o emanuel_check
//
//   emanuel_check <ncol> <nlay> <in.bin> <out.bin>
//       in : 28 doubles {use_qs (0 / 1), cbmf in place (0 / 1), dt, pressure_scale, minorig, elcrit, tlcrit, entp, sigd, sigs, omtrain,
//            omtsnow, coeffr, coeffs, cu, beta, dtmax, alpha, damp, delt0, cpd, cpv, cl, rv, rd, lv0, g, rowl},
//            t, q, u, v, pmid [nlay][ncol], pint [nlay+1][ncol], cbmf [ncol], qs [nlay][ncol] (handed over only with use_qs)
//       out: ft, fq, fu, fv [nlay][ncol], precip, wd, tprime, qprime, cbmf_out, cape, iflag [ncol], ft_per_day [nlay][ncol]
//   Every "thread" (column) of the launches the entry would make runs in turn, the last column first, the work slabs filled with
//   NaN beforehand (a value the rule read without having written it would reach an output).  The program checks that every output
//   element was written and is finite, that the guard elements around every array (the work slabs included) are intact, that the
//   inputs are untouched, and that the run in one chunk, the run in chunks of 64 columns, the run with cbmf_out == cbmf (or, where
//   that was asked for, without) and a run without diagnostics agree bit for bit.
// Exit status 0 and a line that starts with "ok" when everything holds.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <vector>

#include "../climt_amd/csrc/rrtmg_emanuel.h"
#include "check_common.h"

using namespace rrtmg;

constexpr int kHead = 28;

struct FiniteGuarded : Guarded {      // written means: every element finite, too
  bool written() { for (size_t i = 0; i < n; ++i) if (!std::isfinite(p()[i])) return false; return Guarded::written(); }
};

struct Result { std::vector<double> prof[5], col[7]; };      // ft fq fu fv ft_per_day; precip wd tprime qprime cbmf_out cape iflag

// the launches of one call on the CPU: chunks of `chunk` columns
static Result run_call(int ncol, int nlay, long chunk, bool in_place, bool want_diag, const double *k, const double *in) {
  const size_t n1 = ncol, nl = (size_t)nlay * n1, nl1 = nl + n1;
  const bool use_qs = k[0] != 0.0;
  FiniteGuarded prof[5], pi, cb, qs, out[5], diag[6], w1, w2;
  std::vector<int32_t> flag(n1 + 2 * kGuard, -99);
  for (int j = 0; j < 5; ++j) { prof[j].set(in + j * nl, nl); out[j].set(nullptr, nl); }
  pi.set(in + 5 * nl, nl1); cb.set(in + 5 * nl + nl1, n1); qs.set(in + 5 * nl + nl1 + n1, nl);
  for (int j = 0; j < 6; ++j) diag[j].set(nullptr, n1);
  const size_t cc = (size_t)(chunk < ncol ? chunk : ncol);
  const double nan = std::numeric_limits<double>::quiet_NaN();
  EmanuelCall a{};
  a.ncol = ncol; a.nlay = nlay; a.ccol = (int32_t)cc;
  a.t = prof[0].p(); a.q = prof[1].p(); a.u = prof[2].p(); a.v = prof[3].p(); a.pmid = prof[4].p(); a.pint = pi.p(); a.cbmf = cb.p();
  a.qs = use_qs ? qs.p() : nullptr;
  a.dt = k[2]; a.pressure_scale = k[3]; a.minorig = (int32_t)k[4];
  a.elcrit = k[5]; a.tlcrit = k[6]; a.entp = k[7]; a.sigd = k[8]; a.sigs = k[9]; a.omtrain = k[10]; a.omtsnow = k[11]; a.coeffr = k[12]; a.coeffs = k[13];
  a.cu = k[14]; a.beta = k[15]; a.dtmax = k[16]; a.alpha = k[17]; a.damp = k[18]; a.delt0 = k[19];
  a.cpd = k[20]; a.cpv = k[21]; a.cl = k[22]; a.rv = k[23]; a.rd = k[24]; a.lv0 = k[25]; a.g = k[26]; a.rowl = k[27];
  a.ft = out[0].p(); a.fq = out[1].p(); a.fu = out[2].p(); a.fv = out[3].p();
  a.cbmf_out = in_place ? cb.p() : diag[4].p();
  if (want_diag) {
    a.precip = diag[0].p(); a.wd = diag[1].p(); a.tprime = diag[2].p(); a.qprime = diag[3].p(); a.cape = diag[5].p();
    a.iflag = flag.data() + kGuard; a.ft_per_day = out[4].p();
  }
  for (long c0 = 0; c0 < ncol; c0 += (long)cc) {
    w1.set(nullptr, emanuel_work1(nlay) * cc, nan); w2.set(nullptr, emanuel_work2(nlay) * cc, nan);
    a.col0 = c0; a.w1 = w1.p(); a.w2 = w2.p();
    const long c1 = c0 + (long)cc < ncol ? c0 + (long)cc : ncol;
    for (long c = c1 - 1; c >= c0; --c) emanuel_column(a, c);
    w1.check_guards(); w2.check_guards();
  }
  for (int j = 0; j < 5; ++j) { prof[j].check_guards(); out[j].check_guards(); CHECK(prof[j].holds(in + j * nl)); }
  pi.check_guards(); cb.check_guards(); qs.check_guards();
  CHECK(pi.holds(in + 5 * nl) && qs.holds(in + 5 * nl + nl1 + n1));
  for (int j = 0; j < 6; ++j) diag[j].check_guards();
  for (size_t g = 0; g < kGuard; ++g) CHECK(flag[g] == -99 && flag[kGuard + n1 + g] == -99);
  Result r;
  for (int j = 0; j < 4; ++j) { CHECK(out[j].written()); r.prof[j].assign(out[j].p(), out[j].p() + nl); }
  if (in_place) { CHECK(diag[4].untouched()); CHECK(cb.written()); r.col[4].assign(cb.p(), cb.p() + n1); }
  else { CHECK(cb.holds(in + 5 * nl + nl1)); CHECK(diag[4].written()); r.col[4].assign(diag[4].p(), diag[4].p() + n1); }
  if (want_diag) {
    CHECK(out[4].written());
    r.prof[4].assign(out[4].p(), out[4].p() + nl);
    const int at[5] = {0, 1, 2, 3, 5};
    for (int j = 0; j < 5; ++j) { CHECK(diag[at[j]].written()); r.col[at[j]].assign(diag[at[j]].p(), diag[at[j]].p() + n1); }
    for (size_t c = 0; c < n1; ++c) { const int f = flag[kGuard + c]; CHECK(f >= 0 && f <= 4); r.col[6].push_back((double)f); }
  } else {
    CHECK(out[4].untouched());
    const int at[5] = {0, 1, 2, 3, 5};
    for (int j = 0; j < 5; ++j) CHECK(diag[at[j]].untouched());
    for (size_t c = 0; c < n1; ++c) CHECK(flag[kGuard + c] == -99);
  }
  return r;
}

int main(int argc, char **argv) {
  if (argc != 5) { fprintf(stderr, "usage: %s <ncol> <nlay> <in.bin> <out.bin>\n", argv[0]); return 2; }
  const int ncol = atoi(argv[1]), nlay = atoi(argv[2]);
  CHECK(ncol > 0 && nlay >= 4);
  const std::vector<double> file = read_all(argv[3]);
  const size_t n1 = ncol, nl = (size_t)nlay * n1;
  CHECK(file.size() == kHead + 7 * nl + 2 * n1);
  const bool in_place = file[1] != 0.0;
  const double *k = file.data(), *in = file.data() + kHead;
  CHECK(k[4] >= 1.0);
  const Result got = run_call(ncol, nlay, ncol, in_place, true, k, in);
  const Result chunked = run_call(ncol, nlay, 64, in_place, true, k, in), other = run_call(ncol, nlay, ncol, !in_place, true, k, in),
               bare = run_call(ncol, nlay, 64, in_place, false, k, in);
  for (int j = 0; j < 5; ++j) CHECK(equal(chunked.prof[j], got.prof[j]) && equal(other.prof[j], got.prof[j]));
  for (int j = 0; j < 4; ++j) CHECK(equal(bare.prof[j], got.prof[j]));
  for (int j = 0; j < 7; ++j) CHECK(equal(chunked.col[j], got.col[j]) && equal(other.col[j], got.col[j]));
  CHECK(equal(bare.col[4], got.col[4]));
  std::vector<double> out;
  for (int j = 0; j < 4; ++j) out.insert(out.end(), got.prof[j].begin(), got.prof[j].end());
  for (int j = 0; j < 7; ++j) out.insert(out.end(), got.col[j].begin(), got.col[j].end());
  out.insert(out.end(), got.prof[4].begin(), got.prof[4].end());
  write_all(argv[4], out);
  printf("ok (%d columns, %d layers%s%s)\n", ncol, nlay, k[0] != 0.0 ? ", qs given" : ", qs formed", in_place ? ", cbmf in place" : "");
  return 0;
}
