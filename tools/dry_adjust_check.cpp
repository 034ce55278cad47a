// dry_adjust_check.cpp -- the dry convective adjustment (climt_amd/csrc/rrtmg_dry_adjust.h: the sweep of one column, as one thread
// of dry_adjust_kernel runs it) on the CPU, no device: a stand-alone program for the host sanitizers.
//
//   c++ -std=c++17 -ffp-contract=off -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/dry_adjust_check.cpp -o dry_adjust_check
//
//   dry_adjust_check <ncol> <nlay> <in.bin> <out.bin>
//       in : 6 doubles {in_place (0 / 1), cpd, cvap, rd, rv, pref}, t, q, pmid [nlay][ncol], pint [nlay+1][ncol]
//       out: t' [nlay][ncol], q' [nlay][ncol], mixed_top [ncol] (as doubles)
//   Every "thread" (column) of the launch the entry would make runs in turn, the last column first.  The program checks that every
//   output element was written, that the guard elements around every array (the work slabs included) are intact, that the inputs
//   of an out-of-place run are untouched, and that the run in place, the run out of place and a run without mixed_top agree bit
//   for bit.
// Exit status 0 and a line that starts with "ok" when everything holds.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../climt_amd/csrc/rrtmg_dry_adjust.h"
#include "check_common.h"

using namespace rrtmg;

struct Result { std::vector<double> t, q; std::vector<int32_t> top; };

// one launch on the CPU
static Result run_launch(int ncol, int nlay, bool in_place, bool want_top, const double *k, const double *in) {
  const size_t n1 = ncol, nl = (size_t)nlay * n1, nl1 = nl + n1;
  Guarded t, q, pm, pi, to, qo, theta, dp;
  t.set(in, nl); q.set(in + nl, nl); pm.set(in + 2 * nl, nl); pi.set(in + 3 * nl, nl1);
  to.set(nullptr, nl); qo.set(nullptr, nl); theta.set(nullptr, nl); dp.set(nullptr, nl);
  const int32_t kTopPoison = -12345;
  std::vector<int32_t> top(n1 + 2, kTopPoison);
  DryAdjustCall a{};
  a.ncol = ncol; a.nlay = nlay; a.t = t.p(); a.q = q.p(); a.pmid = pm.p(); a.pint = pi.p();
  a.cpd = k[0]; a.cvap = k[1]; a.rd = k[2]; a.rv = k[3]; a.pref = k[4];
  a.t_out = in_place ? t.p() : to.p(); a.q_out = in_place ? q.p() : qo.p();
  a.theta = theta.p(); a.dp = dp.p(); a.mixed_top = want_top ? top.data() + 1 : nullptr;
  for (int col = ncol - 1; col >= 0; --col) dry_adjust_column(a, col);
  for (Guarded *g : {&t, &q, &pm, &pi, &to, &qo, &theta, &dp}) g->check_guards();
  CHECK(top.front() == kTopPoison && top.back() == kTopPoison);
  CHECK(pm.holds(in + 2 * nl) && pi.holds(in + 3 * nl));                                  // only read
  if (in_place) for (size_t i = 0; i < nl; ++i) CHECK(to.p()[i] == kPoison && qo.p()[i] == kPoison);   // the other arrays are not touched
  else CHECK(t.holds(in) && q.holds(in + nl));
  Result r;
  r.t.assign(a.t_out, a.t_out + nl); r.q.assign(a.q_out, a.q_out + nl);
  for (size_t i = 0; i < nl; ++i) CHECK(r.t[i] != kPoison && r.q[i] != kPoison && theta.p()[i] != kPoison && dp.p()[i] != kPoison);
  if (want_top) {
    r.top.assign(top.begin() + 1, top.end() - 1);
    for (int32_t v : r.top) CHECK(v >= -1 && v < nlay);
  } else {
    for (int32_t v : top) CHECK(v == kTopPoison);
  }
  return r;
}

int main(int argc, char **argv) {
  if (argc != 5) { fprintf(stderr, "usage: %s <ncol> <nlay> <in.bin> <out.bin>\n", argv[0]); return 2; }
  const int ncol = atoi(argv[1]), nlay = atoi(argv[2]);
  CHECK(ncol > 0 && nlay > 0);
  const std::vector<double> file = read_all(argv[3]);
  const size_t n1 = ncol, nl = (size_t)nlay * n1;
  CHECK(file.size() == 6 + 4 * nl + n1);
  const bool in_place = file[0] != 0.0;
  const double *k = file.data() + 1, *in = file.data() + 6;
  const Result got = run_launch(ncol, nlay, in_place, true, k, in);
  const Result other = run_launch(ncol, nlay, !in_place, true, k, in), bare = run_launch(ncol, nlay, in_place, false, k, in);
  CHECK(equal(other.t, got.t) && equal(other.q, got.q) && other.top == got.top && equal(bare.t, got.t) && equal(bare.q, got.q));
  // a column that no mixing wrote has the bits of its input
  int untouched = 0;
  for (int col = 0; col < ncol; ++col)
    if (got.top[col] == -1) {
      ++untouched;
      for (int m = 0; m < nlay; ++m) {
        const size_t o = (size_t)m * n1 + col;
        CHECK(memcmp(&got.t[o], &in[o], sizeof(double)) == 0 && memcmp(&got.q[o], &in[nl + o], sizeof(double)) == 0);
      }
    }
  std::vector<double> out(got.t);
  out.insert(out.end(), got.q.begin(), got.q.end());
  for (int32_t v : got.top) out.push_back((double)v);
  write_all(argv[4], out);
  printf("ok (%d columns, %d layers, %d left alone%s)\n", ncol, nlay, untouched, in_place ? ", in place" : "");
  return 0;
}
