// lw_adjust_check.cpp -- the longwave between radiation calls (climt_amd/csrc/rrtmg_lw_adjust.h: the rule of one level and one
// layer, the launch geometry and the levels one thread of lw_adjust_surface_kernel owns) on the CPU, no device: a stand-alone
// program for the host sanitizers.
//
//   c++ -std=c++17 -ffp-contract=off -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/lw_adjust_check.cpp -o lw_adjust_check
//
//   lw_adjust_check <ncol> <nlay> <in.bin> <out.bin>
//       in : 4 doubles {clear (0 / 1), in_place (0 / 1), pressure_scale, heatfac}, tsfc_call[ncol], tsfc_now[ncol],
//            plev, uflx, dflx, duflx_dt [nlay+1][ncol] and, with clear = 1, uflxc, dflxc, duflxc_dt [nlay+1][ncol]
//       out: uflx' [nlay+1][ncol], hr' [nlay][ncol] and, with clear = 1, uflxc', hrc'
//   Every "thread" (column, block of layers) of the launch the entry would make runs in turn, the blocks of layers from the TOP
//   down -- the owner of a halo level before its reader, the order that corrects a halo twice if an in-place launch had more than
//   one block.  The program checks that every output element was written, that the guard elements around every array are intact,
//   that the inputs of an out-of-place run are untouched, and that launches 1, 2, 3 and 64 blocks deep (out of place) agree with it
//   bit for bit.
// Exit status 0 and a line that starts with "ok" when everything holds.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../climt_amd/csrc/rrtmg_lw_adjust.h"
#include "check_common.h"

using namespace rrtmg;

struct Streams { std::vector<double> up, hr, upc, hrc; };

// one launch on the CPU, `ny` blocks of layers deep
static Streams run_launch(int ncol, int nlay, bool clear, bool in_place, double scale, double heatfac, const double *in, int ny) {
  const size_t n1 = ncol, nl = (size_t)nlay * n1, nl1 = nl + n1;
  Guarded tc, tn, pl, src[6], up[2], hr[2];
  tc.set(in, n1); tn.set(in + n1, n1); pl.set(in + 2 * n1, nl1);
  const int nsrc = clear ? 6 : 3;
  for (int k = 0; k < nsrc; ++k) src[k].set(in + 2 * n1 + (size_t)(k + 1) * nl1, nl1);
  for (int s = 0; s < (clear ? 2 : 1); ++s) { up[s].set(nullptr, nl1); hr[s].set(nullptr, nl); }
  LwAdjustCall a{};
  a.ncol = ncol; a.nlay = nlay; a.tsfc_call = tc.p(); a.tsfc_now = tn.p(); a.plev = pl.p(); a.pressure_scale = scale; a.heatfac = heatfac;
  a.all = {src[0].p(), src[1].p(), src[2].p(), in_place ? src[0].p() : up[0].p(), hr[0].p()};
  if (clear) a.clr = {src[3].p(), src[4].p(), src[5].p(), in_place ? src[3].p() : up[1].p(), hr[1].p()};
  for (int y = ny - 1; y >= 0; --y)
    for (int col = ncol - 1; col >= 0; --col) lw_adjust_thread(a, col, y, ny);
  tc.check_guards(); tn.check_guards(); pl.check_guards();
  CHECK(memcmp(pl.p(), in + 2 * n1, nl1 * sizeof(double)) == 0 && memcmp(tn.p(), in + n1, n1 * sizeof(double)) == 0 && memcmp(tc.p(), in, n1 * sizeof(double)) == 0);
  for (int k = 0; k < nsrc; ++k) {
    src[k].check_guards();
    if (!(in_place && k % 3 == 0)) CHECK(memcmp(src[k].p(), in + 2 * n1 + (size_t)(k + 1) * nl1, nl1 * sizeof(double)) == 0);      // only read
  }
  Streams out;
  for (int s = 0; s < (clear ? 2 : 1); ++s) {
    up[s].check_guards(); hr[s].check_guards();
    const double *u = in_place ? src[3 * s].p() : up[s].p();
    if (in_place) for (size_t i = 0; i < nl1; ++i) CHECK(up[s].p()[i] == kPoison);      // the other array is not touched
    else for (size_t i = 0; i < nl1; ++i) CHECK(u[i] != kPoison);
    for (size_t i = 0; i < nl; ++i) CHECK(hr[s].p()[i] != kPoison);
    (s ? out.upc : out.up).assign(u, u + nl1);
    (s ? out.hrc : out.hr).assign(hr[s].p(), hr[s].p() + nl);
  }
  return out;
}

int main(int argc, char **argv) {
  // the rule and the geometry
  CHECK(same_bits(lw_adjust_flux(3.5, 2.0, 0.0), 3.5) && same_bits(lw_adjust_flux(-0.0, 5.0, 0.0), 0.0) && same_bits(lw_adjust_flux(1.0, 0.5, -2.0), 0.0));
  CHECK(same_bits(lw_adjust_pressure(7.0, 0.0), 7.0) && same_bits(lw_adjust_pressure(700.0, 0.01), 700.0 * 0.01));
  CHECK(same_bits(lw_adjust_heat(2.0, 5.0, 2.0, 10.0, 4.0), 1.0));
  CHECK(lw_adjust_grid_y(1, false) == 1 && lw_adjust_grid_y(kLwAdjustChunk, false) == 1 && lw_adjust_grid_y(kLwAdjustChunk + 1, false) == 2 && lw_adjust_grid_y(60, false) == 8);
  CHECK(lw_adjust_grid_y(100000, false) == kLwAdjustMaxGridY && lw_adjust_grid_y(60, true) == 1 && lw_adjust_grid_y(100000, true) == 1);
  CHECK(lw_adjust_layers_per_thread(60, 8) == 8 && lw_adjust_layers_per_thread(60, 1) == 64 && lw_adjust_layers_per_thread(60, 3) == 24 && lw_adjust_layers_per_thread(1, 1) == 8);
  CHECK(lw_adjust_layers_per_thread(1000, kLwAdjustMaxGridY) == 16);
  if (argc != 5) { fprintf(stderr, "usage: %s <ncol> <nlay> <in.bin> <out.bin>\n", argv[0]); return 2; }
  const int ncol = atoi(argv[1]), nlay = atoi(argv[2]);
  CHECK(ncol > 0 && nlay > 0);
  const std::vector<double> file = read_all(argv[3]);
  CHECK(file.size() >= 4);
  const bool clear = file[0] != 0.0, in_place = file[1] != 0.0;
  const size_t n1 = ncol, nl1 = ((size_t)nlay + 1) * n1;
  CHECK(file.size() == 4 + 2 * n1 + (clear ? 7 : 4) * nl1);
  const double *in = file.data() + 4;
  const int ny = lw_adjust_grid_y(nlay, in_place);
  const Streams got = run_launch(ncol, nlay, clear, in_place, file[2], file[3], in, ny);
  for (int other : {1, 2, 3, kLwAdjustMaxGridY}) {
    const Streams o = run_launch(ncol, nlay, clear, false, file[2], file[3], in, other);
    CHECK(equal(o.up, got.up) && equal(o.hr, got.hr) && equal(o.upc, got.upc) && equal(o.hrc, got.hrc));
  }
  std::vector<double> out;
  for (const std::vector<double> *v : {&got.up, &got.hr, &got.upc, &got.hrc}) out.insert(out.end(), v->begin(), v->end());
  write_all(argv[4], out);
  printf("ok (%d columns, %d layers, %d block(s) of layers%s%s)\n", ncol, nlay, ny, clear ? ", clear-sky stream" : "", in_place ? ", in place" : "");
  return 0;
}
