// land_surface_check.cpp -- the two land-surface rules (climt_amd/csrc/rrtmg_land_surface.h: the rule of one column, as one thread
// of bucket_hydrology_kernel / second_best_kernel runs it) and the two tables at the head of rrtmg_land_surface.hip on the CPU, no
// device: a stand-alone program for tests/test_land_surface.py and the host sanitizers.
//
//   c++ -std=c++17 -ffp-contract=off -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/land_surface_check.cpp -o land_surface_check
//
//   land_surface_check tables
//       Line: <entry> <in|out> <struct> <member> <extent> <f64|i32> <required or -> <the input it may be, or ->   (the format of
//       tools/surface_ice_check.cpp), both tables; then the checks of tools/column_table_check.h: the staging plan at ncol 1, 63, 64,
//       65 x three nlay x every combination of optional rows, the aliasing refusals with made-up addresses and the "must be given"
//       text.  Last line "ok".
//   land_surface_check bucket <ncol> <in.bin> <out.bin>
//       in : 15 doubles {layers, has_drain, dt, rd, cp, rho_water, lv, bulk_coefficient, beta_parameter, soil_moisture_max,
//            deep_soil_moisture_max, tau_m, deep_ratio, tau_drain, pressure_scale}, then the 19 input rows [ncol] in the table's order
//            (the two deep ones are in the file with layers 1 too, and are not handed to the rule)
//       out: ts_out, soil_moisture_out, deep_moisture_out, deep_temperature_out, precip, lh, sh, evaporation, runoff, deep_fraction
//            [ncol]; what layers 1 does not write is 0
//   land_surface_check best <ncol> <nlay> <in.bin> <out.bin>
//       in : 19 doubles {dt, rd, g, cp, lv, lf, rho_water, karman, t_freeze, min_wind, kappa_soil, cv_soil, colour, texture, B, K_H0,
//            psi_0, pressure_scale, ps_scale}, t_soil, x_w, x_i, height [nlay][ncol], then t_air, q_air, u, v, p_air, ps, ts, snow,
//            sw_down, lw_down, sw_up, lw_up and the area-type codes as doubles [ncol]
//       out: t_soil_out, x_w_out, x_i_out [nlay][ncol], ts_out, snow_out, the eleven diagnostics and flags (as doubles) [ncol]
//   Out of place, fully in place and without the optional outputs must agree bit for bit.  Every "thread" (column) of the launch
//   the entry would make runs in turn, the last column first.  The program checks that every output element was written, that the
//   guard elements around every array are intact and that the inputs of the out-of-place run are untouched.
// Exit status 0 and a last line that starts with "ok" when everything holds.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../climt_amd/csrc/rrtmg_land_surface.hip"
#include "column_table_check.h"

using namespace rrtmg;

// ---- the tables ------------------------------------------------------------------------------------------------------------------
static int tables() {
  print_table(kBucketHydrology);
  print_table(kSecondBest);
  check_plan(kBucketHydrology);
  check_plan(kSecondBest);
  const char *note = " (in place: exactly its own input)";
  check_aliasing<rrtmg_bucket_hydrology>(kBucketHydrology, note,
      "t_air, q_air, u, v, p_air, ts, q_sfc, sw_down, lw_down, sw_up, lw_up, soil_moisture, precip_conv, precip_strat, density, thickness, heat_capacity, ts_out and soil_moisture_out must be given");
  check_aliasing<rrtmg_second_best>(kSecondBest, note,
      "t_soil, x_w, x_i, height, t_air, q_air, u, v, p_air, ps, ts, snow, sw_down, lw_down, sw_up, lw_up, area_type, t_soil_out, x_w_out, x_i_out, ts_out and snow_out must be given");
  printf("ok\n");
  return 0;
}

// ---- the rules -------------------------------------------------------------------------------------------------------------------

// ---- BucketHydrology: one launch on the CPU -> the ten output rows (a row that is not written: zeros) ----------------------------------
constexpr int kBucketIn = 19, kBucketOut = 10;
static std::vector<double> run_bucket(int ncol, const double *k, const double *in, bool in_place, bool want_optional) {
  const size_t n1 = ncol;
  const int layers = (int)k[0];
  Guarded x[kBucketIn], y[kBucketOut];
  for (int i = 0; i < kBucketIn; ++i) x[i].set(in + (size_t)i * n1, n1);
  for (int i = 0; i < kBucketOut; ++i) y[i].set(nullptr, n1);
  BucketHydrologyCall a{};
  a.ncol = ncol; a.layers = layers; a.has_drain = (int)k[1];
  a.dt = k[2]; a.rd = k[3]; a.cp = k[4]; a.rho_water = k[5]; a.lv = k[6]; a.bulk_coefficient = k[7]; a.beta_parameter = k[8]; a.soil_moisture_max = k[9];
  a.deep_soil_moisture_max = k[10]; a.tau_m = k[11]; a.deep_ratio = k[12]; a.tau_drain = k[13]; a.pressure_scale = k[14];
  const double **inputs[kBucketIn] = {&a.t_air, &a.q_air, &a.u, &a.v, &a.p_air, &a.ts, &a.q_sfc, &a.sw_down, &a.lw_down, &a.sw_up, &a.lw_up, &a.soil_moisture,
                                      &a.precip_conv, &a.precip_strat, &a.density, &a.thickness, &a.heat_capacity, &a.deep_moisture, &a.deep_temperature};
  double **outputs[kBucketOut] = {&a.ts_out, &a.soil_moisture_out, &a.deep_moisture_out, &a.deep_temperature_out, &a.precip, &a.lh, &a.sh, &a.evaporation,
                                  &a.runoff, &a.deep_fraction};
  const int partner[4] = {5, 11, 17, 18};      // ts, soil_moisture, deep_moisture, deep_temperature
  const bool deep_row[kBucketOut] = {false, false, true, true, false, false, false, false, true, true};
  for (int i = 0; i < kBucketIn; ++i)
    if (i < 17 || layers == 2) *inputs[i] = x[i].p();      // what layers 1 does not read is not handed over: a read would fault
  bool bound[kBucketOut];
  for (int i = 0; i < kBucketOut; ++i) {
    bound[i] = (i < 4 || want_optional) && (!deep_row[i] || layers == 2);
    if (bound[i]) *outputs[i] = i < 4 && in_place ? x[partner[i]].p() : y[i].p();
  }
  for (int c = ncol - 1; c >= 0; --c) bucket_hydrology_column(a, c);
  std::vector<double> r;
  for (int i = 0; i < kBucketIn; ++i) {
    x[i].check_guards();
    bool stepped = false;
    for (int j = 0; j < 4; ++j) stepped |= in_place && bound[j] && partner[j] == i;
    if (!stepped) CHECK(x[i].holds(in + (size_t)i * n1));
  }
  for (int i = 0; i < kBucketOut; ++i) {
    y[i].check_guards();
    Guarded &from = i < 4 && in_place && bound[i] ? x[partner[i]] : y[i];
    if (bound[i]) CHECK(from.written());
    if (!bound[i] || (i < 4 && in_place)) CHECK(y[i].untouched());
    for (size_t c = 0; c < n1; ++c) r.push_back(bound[i] ? from.p()[c] : 0.0);
  }
  return r;
}

static int bucket_file(int ncol, const char *in, const char *out) {
  const std::vector<double> file = read_all(in);
  const size_t n1 = ncol;
  CHECK(file.size() == 15 + kBucketIn * n1);
  const double *k = file.data(), *arrays = k + 15;
  CHECK((k[0] == 1.0 || k[0] == 2.0) && (k[1] == 0.0 || k[1] == 1.0));
  const std::vector<double> got = run_bucket(ncol, k, arrays, false, true), in_place = run_bucket(ncol, k, arrays, true, true), bare = run_bucket(ncol, k, arrays, false, false);
  CHECK(equal(got, in_place));
  CHECK(memcmp(got.data(), bare.data(), 4 * n1 * sizeof(double)) == 0);
  write_all(out, got);
  printf("ok (bucket_hydrology layers %d, %d columns)\n", (int)k[0], ncol);
  return 0;
}

// ---- SecondBEST: one launch on the CPU -> t_soil_out, x_w_out, x_i_out [nl], ts_out, snow_out, the diagnostics, flags [n1] -----------------
constexpr int kBestCol = 12, kBestDiag = 11;
static std::vector<double> run_best(int ncol, int nlay, const double *k, const double *in, const std::vector<int32_t> &area, bool in_place, bool want_optional) {
  const size_t n1 = ncol, nl = (size_t)nlay * n1;
  Guarded soil[4], col[kBestCol], soil_out[3], col_out[2], diag[kBestDiag], wc, wd;
  for (int i = 0; i < 4; ++i) soil[i].set(in + (size_t)i * nl, nl);
  for (int i = 0; i < kBestCol; ++i) col[i].set(in + 4 * nl + (size_t)i * n1, n1);
  for (Guarded *g : {&soil_out[0], &soil_out[1], &soil_out[2], &wc, &wd}) g->set(nullptr, nl);
  for (Guarded &g : col_out) g.set(nullptr, n1);
  for (Guarded &g : diag) g.set(nullptr, n1);
  std::vector<int32_t> at(n1 + 2 * kGuard, -77), flags(n1 + 2 * kGuard, -77);
  memcpy(at.data() + kGuard, area.data(), n1 * sizeof(int32_t));
  SecondBestCall a{};
  a.ncol = ncol; a.nlay = nlay;
  a.dt = k[0]; a.rd = k[1]; a.g = k[2]; a.cp = k[3]; a.lv = k[4]; a.lf = k[5]; a.rho_water = k[6]; a.karman = k[7]; a.t_freeze = k[8]; a.min_wind = k[9];
  a.kappa_soil = k[10]; a.cv_soil = k[11]; a.colour = k[12]; a.texture = k[13]; a.B = k[14]; a.K_H0 = k[15]; a.psi_0 = k[16]; a.pressure_scale = k[17]; a.ps_scale = k[18];
  a.t_soil = soil[0].p(); a.x_w = soil[1].p(); a.x_i = soil[2].p(); a.height = soil[3].p();
  a.t_air = col[0].p(); a.q_air = col[1].p(); a.u = col[2].p(); a.v = col[3].p(); a.p_air = col[4].p(); a.ps = col[5].p(); a.ts = col[6].p(); a.snow = col[7].p();
  a.sw_down = col[8].p(); a.lw_down = col[9].p(); a.sw_up = col[10].p(); a.lw_up = col[11].p();
  a.area_type = at.data() + kGuard;
  a.t_soil_out = in_place ? soil[0].p() : soil_out[0].p(); a.x_w_out = in_place ? soil[1].p() : soil_out[1].p(); a.x_i_out = in_place ? soil[2].p() : soil_out[2].p();
  a.ts_out = in_place ? col[6].p() : col_out[0].p(); a.snow_out = in_place ? col[7].p() : col_out[1].p();
  if (want_optional) {
    a.sh = diag[0].p(); a.lh = diag[1].p(); a.evaporation = diag[2].p(); a.albedo_direct = diag[3].p(); a.albedo_diffuse = diag[4].p(); a.cd_heat = diag[5].p();
    a.cd_momentum = diag[6].p(); a.t2m = diag[7].p(); a.q2m = diag[8].p(); a.u10 = diag[9].p(); a.v10 = diag[10].p(); a.flags = flags.data() + kGuard;
  }
  a.work_c = wc.p(); a.work_d = wd.p();
  for (int c = ncol - 1; c >= 0; --c) second_best_column(a, c);
  for (Guarded *g : {&soil[0], &soil[1], &soil[2], &soil[3], &soil_out[0], &soil_out[1], &soil_out[2], &col_out[0], &col_out[1], &wc, &wd}) g->check_guards();
  for (Guarded &g : col) g.check_guards();
  for (Guarded &g : diag) g.check_guards();
  for (size_t g = 0; g < kGuard; ++g) CHECK(at[g] == -77 && at[kGuard + n1 + g] == -77 && flags[g] == -77 && flags[kGuard + n1 + g] == -77);
  CHECK(memcmp(at.data() + kGuard, area.data(), n1 * sizeof(int32_t)) == 0 && soil[3].holds(in + 3 * nl));
  for (int i = 0; i < kBestCol; ++i)
    if (!(in_place && (i == 6 || i == 7))) CHECK(col[i].holds(in + 4 * nl + (size_t)i * n1));
  if (in_place) {
    for (Guarded &g : soil_out) CHECK(g.untouched());
    for (Guarded &g : col_out) CHECK(g.untouched());
  } else {
    for (int i = 0; i < 3; ++i) CHECK(soil[i].holds(in + (size_t)i * nl) && soil_out[i].written());
    CHECK(col_out[0].written() && col_out[1].written());
  }
  std::vector<double> r;
  for (int i = 0; i < 3; ++i) { Guarded &g = in_place ? soil[i] : soil_out[i]; r.insert(r.end(), g.p(), g.p() + nl); }
  for (int i = 0; i < 2; ++i) { Guarded &g = in_place ? col[6 + i] : col_out[i]; r.insert(r.end(), g.p(), g.p() + n1); }
  if (want_optional) {
    for (Guarded &g : diag) { CHECK(g.written()); r.insert(r.end(), g.p(), g.p() + n1); }
    for (size_t i = 0; i < n1; ++i) { CHECK(flags[kGuard + i] >= 0 && flags[kGuard + i] < 8); r.push_back((double)flags[kGuard + i]); }
  } else {
    for (Guarded &g : diag) CHECK(g.untouched());
    for (size_t i = 0; i < n1; ++i) CHECK(flags[kGuard + i] == -77);
  }
  return r;
}

static int best_file(int ncol, int nlay, const char *in, const char *out) {
  const std::vector<double> file = read_all(in);
  const size_t n1 = ncol, nl = (size_t)nlay * n1;
  CHECK(file.size() == 19 + 4 * nl + (kBestCol + 1) * n1);
  const double *k = file.data(), *arrays = k + 19, *codes = arrays + 4 * nl + kBestCol * n1;
  std::vector<int32_t> area(n1);
  for (size_t i = 0; i < n1; ++i) area[i] = (int32_t)codes[i];
  const std::vector<double> got = run_best(ncol, nlay, k, arrays, area, false, true), in_place = run_best(ncol, nlay, k, arrays, area, true, true),
                            bare = run_best(ncol, nlay, k, arrays, area, false, false);
  CHECK(equal(got, in_place));
  CHECK(bare.size() == 3 * nl + 2 * n1 && memcmp(got.data(), bare.data(), bare.size() * sizeof(double)) == 0);
  write_all(out, got);
  printf("ok (second_best, %d columns, %d nodes)\n", ncol, nlay);
  return 0;
}

int main(int argc, char **argv) {
  if (argc == 2 && !strcmp(argv[1], "tables")) return tables();
  if (argc == 5 && !strcmp(argv[1], "bucket")) { const int ncol = atoi(argv[2]); CHECK(ncol > 0); return bucket_file(ncol, argv[3], argv[4]); }
  if (argc == 6 && !strcmp(argv[1], "best")) { const int ncol = atoi(argv[2]), nlay = atoi(argv[3]); CHECK(ncol > 0 && nlay >= 2); return best_file(ncol, nlay, argv[4], argv[5]); }
  fprintf(stderr, "usage: %s tables | %s bucket <ncol> <in.bin> <out.bin> | %s best <ncol> <nlay> <in.bin> <out.bin>\n", argv[0], argv[0], argv[0]);
  return 2;
}
