// surface_ice_check.cpp -- the snow/ice column (climt_amd/csrc/rrtmg_surface_ice.h: the rule of one column, as one thread of
// surface_ice_kernel runs it) and the table at the head of rrtmg_surface_ice.hip on the CPU, no device: a stand-alone program for
// tests/test_surface_ice.py and the host sanitizers.
//
//   c++ -std=c++17 -ffp-contract=off -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/surface_ice_check.cpp -o surface_ice_check
//
//   surface_ice_check tables
//       Line: <entry> <in|out> <struct> <member> <extent> <f64|i32> <required or -> <the input it may be, or ->   (the format of
//       tools/gray_check.cpp), then the checks of tools/column_table_check.h: the staging plan at ncol 1, 63, 64, 65 x nlay 3, 4, 61
//       x every combination of optional rows, the aliasing refusals with made-up addresses and the "must be given" text.  Last line "ok".
//   surface_ice_check run <ncol> <nlay> <in.bin> <out.bin>
//       in : 15 doubles {kind (0 / 1), dt, rho_ice, rho_snow, c_ice, c_snow, k_ice, k_snow, lf, t_melt, eps, max_height, albedo_snow,
//            albedo_ice, albedo_melt}, t, height [nlay][ncol], thick, snow, base, sw_down, lw_down, sw_up, lw_up, lh, sh [ncol], the
//            area-type codes as doubles [ncol]
//       out: t_out, height_out [nlay][ncol], thick_out, snow_out, tsfc_out, base_flux_out, cond_flux, albedo, flags (as doubles) [ncol]
//       Out of place, fully in place (t, height, thick, snow and, for kind 0, base) and without the optional outputs must agree bit
//       for bit.  Every "thread" (column) of the launch the entry would make runs in turn, the last column first.  The program
//       checks that every output element was written, that the guard elements around every array are intact and that the inputs
//       of the out-of-place run are untouched.
// Exit status 0 and a last line that starts with "ok" when everything holds.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../climt_amd/csrc/rrtmg_surface_ice.hip"
#include "column_table_check.h"

using namespace rrtmg;

// ---- the table -------------------------------------------------------------------------------------------------------------------
static int tables() {
  print_table(kSurfaceIce);
  check_plan(kSurfaceIce);
  check_aliasing<rrtmg_surface_ice>(kSurfaceIce, " (in place: exactly its own input)",
                 "t, height, thick, snow, base, sw_down, lw_down, sw_up, lw_up, lh, sh, area_type, t_out, height_out, thick_out, snow_out, tsfc_out and base_flux_out must be given");
  printf("ok\n");
  return 0;
}

// ---- the rule --------------------------------------------------------------------------------------------------------------------

struct IceResult { std::vector<double> t, height, thick, snow, tsfc, base_flux, cond, albedo, flags; };

// one launch on the CPU.  in: t, height [nl], then thick, snow, base, the six fluxes [n1]; area: the codes
static IceResult run(int ncol, int nlay, const double *k, const double *in, const std::vector<int32_t> &area, bool in_place, bool want_optional) {
  const size_t n1 = ncol, nl = (size_t)nlay * n1;
  const int kind = (int)k[0];
  Guarded t, h, col[9], t_out, h_out, thick_out, snow_out, tsfc, base_out, cond, albedo, wc, wd;
  t.set(in, nl); h.set(in + nl, nl);
  for (int i = 0; i < 9; ++i) col[i].set(in + 2 * nl + (size_t)i * n1, n1);
  for (Guarded *g : {&t_out, &h_out, &wc, &wd}) g->set(nullptr, nl);
  for (Guarded *g : {&thick_out, &snow_out, &tsfc, &base_out, &cond, &albedo}) g->set(nullptr, n1);
  std::vector<int32_t> at(n1 + 2 * kGuard, -77), flags(n1 + 2 * kGuard, -77);
  memcpy(at.data() + kGuard, area.data(), n1 * sizeof(int32_t));
  SurfaceIceCall a{};
  a.ncol = ncol; a.nlay = nlay; a.kind = kind;
  a.t = t.p(); a.height = h.p(); a.thick = col[0].p(); a.snow = col[1].p(); a.base = col[2].p();
  a.sw_down = col[3].p(); a.lw_down = col[4].p(); a.sw_up = col[5].p(); a.lw_up = col[6].p(); a.lh = col[7].p(); a.sh = col[8].p();
  a.area_type = at.data() + kGuard;
  a.dt = k[1]; a.rho_ice = k[2]; a.rho_snow = k[3]; a.c_ice = k[4]; a.c_snow = k[5]; a.k_ice = k[6]; a.k_snow = k[7]; a.lf = k[8]; a.t_melt = k[9];
  a.eps = k[10]; a.max_height = k[11]; a.albedo_snow = k[12]; a.albedo_ice = k[13]; a.albedo_melt = k[14];
  const bool base_in_place = in_place && kind == 0;
  a.t_out = in_place ? t.p() : t_out.p(); a.height_out = in_place ? h.p() : h_out.p();
  a.thick_out = in_place ? col[0].p() : thick_out.p(); a.snow_out = in_place ? col[1].p() : snow_out.p();
  a.tsfc_out = tsfc.p(); a.base_flux_out = base_in_place ? col[2].p() : base_out.p();
  if (want_optional) { a.cond_flux = cond.p(); a.albedo = albedo.p(); a.flags = flags.data() + kGuard; }
  a.work_c = wc.p(); a.work_d = wd.p();
  for (int c = ncol - 1; c >= 0; --c) surface_ice_column(a, c);
  for (Guarded *g : {&t, &h, &t_out, &h_out, &thick_out, &snow_out, &tsfc, &base_out, &cond, &albedo, &wc, &wd}) g->check_guards();
  for (int i = 0; i < 9; ++i) { col[i].check_guards(); if (i >= 3) CHECK(col[i].holds(in + 2 * nl + (size_t)i * n1)); }
  for (size_t g = 0; g < kGuard; ++g) CHECK(at[g] == -77 && at[kGuard + n1 + g] == -77 && flags[g] == -77 && flags[kGuard + n1 + g] == -77);
  CHECK(memcmp(at.data() + kGuard, area.data(), n1 * sizeof(int32_t)) == 0);
  if (in_place) CHECK(t_out.untouched() && h_out.untouched() && thick_out.untouched() && snow_out.untouched());
  else CHECK(t.holds(in) && h.holds(in + nl) && col[0].holds(in + 2 * nl) && col[1].holds(in + 2 * nl + n1) && t_out.written() && h_out.written() && thick_out.written() && snow_out.written());
  if (base_in_place) CHECK(base_out.untouched());
  else CHECK(col[2].holds(in + 2 * nl + 2 * n1) && base_out.written());
  CHECK(tsfc.written());
  IceResult r{(in_place ? t : t_out).get(), (in_place ? h : h_out).get(), (in_place ? col[0] : thick_out).get(), (in_place ? col[1] : snow_out).get(),
              tsfc.get(), (base_in_place ? col[2] : base_out).get(), {}, {}, {}};
  if (want_optional) {
    CHECK(cond.written() && albedo.written());
    r.cond = cond.get(); r.albedo = albedo.get();
    for (size_t i = 0; i < n1; ++i) { CHECK(flags[kGuard + i] >= 0 && flags[kGuard + i] < 8); r.flags.push_back((double)flags[kGuard + i]); }
  } else {
    CHECK(cond.untouched() && albedo.untouched());
    for (size_t i = 0; i < n1; ++i) CHECK(flags[kGuard + i] == -77);
  }
  return r;
}

static bool same(const IceResult &a, const IceResult &b) {
  return equal(a.t, b.t) && equal(a.height, b.height) && equal(a.thick, b.thick) && equal(a.snow, b.snow) && equal(a.tsfc, b.tsfc) && equal(a.base_flux, b.base_flux);
}

static int run_file(int ncol, int nlay, const char *in, const char *out) {
  const std::vector<double> file = read_all(in);
  const size_t n1 = ncol, nl = (size_t)nlay * n1;
  CHECK(file.size() == 15 + 2 * nl + 10 * n1);
  const double *k = file.data(), *arrays = k + 15, *codes = arrays + 2 * nl + 9 * n1;
  CHECK(k[0] == 0.0 || k[0] == 1.0);
  std::vector<int32_t> area(n1);
  for (size_t i = 0; i < n1; ++i) area[i] = (int32_t)codes[i];
  const IceResult got = run(ncol, nlay, k, arrays, area, false, true), in_place = run(ncol, nlay, k, arrays, area, true, true), bare = run(ncol, nlay, k, arrays, area, false, false);
  CHECK(same(got, in_place) && equal(got.cond, in_place.cond) && equal(got.albedo, in_place.albedo) && equal(got.flags, in_place.flags) && same(got, bare));
  std::vector<double> o;
  for (const std::vector<double> *v : {&got.t, &got.height, &got.thick, &got.snow, &got.tsfc, &got.base_flux, &got.cond, &got.albedo, &got.flags}) o.insert(o.end(), v->begin(), v->end());
  write_all(out, o);
  printf("ok (surface_ice kind %d, %d columns, %d nodes)\n", (int)k[0], ncol, nlay);
  return 0;
}

int main(int argc, char **argv) {
  if (argc == 2 && !strcmp(argv[1], "tables")) return tables();
  if (argc != 6 || strcmp(argv[1], "run")) { fprintf(stderr, "usage: %s tables | %s run <ncol> <nlay> <in.bin> <out.bin>\n", argv[0], argv[0]); return 2; }
  const int ncol = atoi(argv[2]), nlay = atoi(argv[3]);
  CHECK(ncol > 0 && nlay >= 3);
  return run_file(ncol, nlay, argv[4], argv[5]);
}
