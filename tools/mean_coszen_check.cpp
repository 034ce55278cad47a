// mean_coszen_check.cpp -- the host-checkable part of the shortwave between radiation calls (climt_amd/csrc/rrtmg_intermittent.h:
// the sun over an interval, the per-column interval mean of the cosine of the zenith angle, the element rule of the rescale and
// the rows one of its threads owns) on the CPU, no device: a stand-alone program for the host sanitizers.
//
//   c++ -std=c++17 -ffp-contract=off -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/mean_coszen_check.cpp -o mean_coszen_check
//
//   mean_coszen_check mean <ncol> <in.bin> <out.bin>
//       in : 7 doubles {mode, t0, t1, sin_dec, cos_dec, g0, D}, lat_deg[ncol], lon_deg[ncol]
//            mode 0: the interval [t0, t1] in Julian centuries, as rrtmg_hip_mean_coszen; an interval that call refuses ends the
//            program with status 4 (RRTMG_ERR_ARG).  mode 1: the sun as given, as rrtmg_hip_mean_coszen_sun.
//       out: 4 doubles {sin_dec, cos_dec, g0, D} as used, then mean, fraction, zenith, insolation [ncol] each -- what
//            mean_coszen_kernel writes, column by column
//   mean_coszen_check scale <ncol> <in.bin> <out.bin>
//       in : 1 double n (entries, 16 at the most), n doubles rows, n doubles in_place (0 / 1), num[ncol], den[ncol], then each
//            entry's src [rows][ncol]
//       out: each entry's dst [rows][ncol].  Every "thread" (column, row group, entry) of scale_columns_kernel runs in turn, for
//            the launch's own depth and for depths 1 and 3; the program checks that every element was written exactly once (a second
//            write in place would scale twice), that the guard elements around every array are intact and that no +0.0 rule is
//            broken, and that the three depths agree bit for bit.
// Exit status 0 and a line that starts with "ok" when everything holds.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../climt_amd/csrc/rrtmg_intermittent.h"
#include "check_common.h"

using namespace rrtmg;

static void element_rules() {
  const double nan = std::nan(""), inf = INFINITY;
  CHECK(same_bits(scale_factor(1.0, 0.0), 0.0) && same_bits(scale_factor(1.0, -1.0), 0.0) && same_bits(scale_factor(nan, 0.0), 0.0));
  CHECK(same_bits(scale_factor(1.0, nan), 0.0));                      // a NaN denominator is not > 0
  CHECK(same_bits(scale_factor(3.0, 4.0), 0.75) && same_bits(scale_factor(0.0, 4.0), 0.0));
  for (double x : {1.5, -1.5, 0.0, -0.0, nan, inf, -inf})
    for (double z : {0.0, -0.0}) CHECK(same_bits(scale_element(x, z), 0.0));      // +0.0: never -0.0, never NaN * 0
  CHECK(same_bits(scale_element(-0.0, 0.5), -0.0) && same_bits(scale_element(3.0, 0.25), 0.75) && same_bits(scale_element(-2.0, 1.0), -2.0));
  CHECK(interval_ok(0.2, 0.2 + 0.5 / 36525.0) && interval_ok(0.2, 0.2 + 60.0 / 86400.0 / 36525.0));
  CHECK(!interval_ok(0.2, 0.2) && !interval_ok(0.2, 0.1) && !interval_ok(0.2, 0.2 + 0.51 / 36525.0) && !interval_ok(0.2, std::nan("")));
  CHECK(same_bits(mean_zenith(0.0), 1.5707963267948966) && same_bits(mean_zenith(1.0), 0.0));
}

static int run_mean(int ncol, const char *in_path, const char *out_path) {
  const std::vector<double> in = read_all(in_path);
  CHECK(in.size() == 7 + 2 * (size_t)ncol);
  IntervalSun sun;
  if (in[0] == 0.0) {
    if (!interval_ok(in[1], in[2])) { fprintf(stderr, "interval refused: t0 < t1 of 12 hours at the most\n"); return 4; }
    sun = interval_sun(in[1], in[2]);
  } else {
    sun = {in[3], in[4], in[5], in[6]};
  }
  if (!interval_sun_ok(sun)) { fprintf(stderr, "the advance of the hour angle must lie in (0, 2 pi)\n"); return 4; }
  const double *lat = in.data() + 7, *lon = lat + ncol;
  std::vector<double> out(4 + 4 * (size_t)ncol);
  out[0] = sun.sin_dec; out[1] = sun.cos_dec; out[2] = sun.g0; out[3] = sun.D;
  for (int i = 0; i < ncol; ++i) {
    const MeanCoszen r = mean_coszen_column(lat[i], lon[i], sun);
    CHECK(r.mean >= 0.0 && r.mean <= 1.0 && r.fraction >= 0.0 && r.fraction <= 1.0 + 1e-12);
    out[4 + i] = r.mean; out[4 + ncol + i] = r.fraction;
    out[4 + 2 * (size_t)ncol + i] = mean_zenith(r.mean); out[4 + 3 * (size_t)ncol + i] = mean_insolation(r);
  }
  write_all(out_path, out);
  printf("ok (%d columns, D = %.17g)\n", ncol, sun.D);
  return 0;
}

// one launch on the CPU: every thread of grid (columns, ny, n) in turn -> the dst arrays, guards checked
static std::vector<std::vector<double>> run_launch(int ncol, int n, const std::vector<int> &rows, const std::vector<int> &in_place, const double *num,
                                                   const double *den, const std::vector<std::vector<double>> &src, int ny) {
  // (guards on both sides of every array; an in-place entry works on a copy of its source)
  std::vector<std::vector<double>> work(n), dst(n);
  ScaleTable t{};
  for (int k = 0; k < n; ++k) {
    const size_t len = (size_t)rows[k] * ncol;
    work[k].assign(len + 2 * kGuard, kPoison);
    memcpy(work[k].data() + kGuard, src[k].data(), len * sizeof(double));
    dst[k].assign(len + 2 * kGuard, kPoison);
    t.e[k] = {work[k].data() + kGuard, (in_place[k] ? work[k].data() : dst[k].data()) + kGuard, rows[k], 0};
  }
  // the count of writes: a shadow launch on arrays of ones with s = 2 -- an element written twice in place would read 4
  for (int pass = 0; pass < 2; ++pass) {
    std::vector<std::vector<double>> ones(n);
    ScaleTable u = t;
    if (pass == 0)
      for (int k = 0; k < n; ++k) { ones[k].assign((size_t)rows[k] * ncol, 1.0); u.e[k] = {ones[k].data(), ones[k].data(), rows[k], 0}; }
    for (int z = 0; z < n; ++z)
      for (int y = 0; y < ny; ++y)
        for (int col = 0; col < ncol; ++col) {
          if (y * kScaleRows >= u.e[z].rows) continue;      // (the kernel's early return)
          scale_thread(u.e[z], ncol, col, y, ny, pass == 0 ? 2.0 : scale_factor(num[col], den[col]));
        }
    if (pass == 0)
      for (int k = 0; k < n; ++k) for (double v : ones[k]) CHECK(v == 2.0);
  }
  std::vector<std::vector<double>> out(n);
  for (int k = 0; k < n; ++k) {
    const size_t len = (size_t)rows[k] * ncol;
    const std::vector<double> &d = in_place[k] ? work[k] : dst[k];
    for (size_t g = 0; g < kGuard; ++g) CHECK(work[k][g] == kPoison && work[k][kGuard + len + g] == kPoison && dst[k][g] == kPoison && dst[k][kGuard + len + g] == kPoison);
    if (!in_place[k]) CHECK(memcmp(work[k].data() + kGuard, src[k].data(), len * sizeof(double)) == 0);      // the source is only read
    out[k].assign(d.begin() + kGuard, d.begin() + kGuard + len);
    for (size_t i = 0; i < len; ++i) {
      const double s = scale_factor(num[i % ncol], den[i % ncol]);
      if (s == 0.0) CHECK(same_bits(out[k][i], 0.0));
      else { volatile double p = src[k][i] * s; CHECK(same_bits(out[k][i], (double)p) || (std::isnan(out[k][i]) && std::isnan((double)p))); }
    }
  }
  return out;
}

static int run_scale(int ncol, const char *in_path, const char *out_path) {
  const std::vector<double> in = read_all(in_path);
  CHECK(!in.empty());
  const int n = (int)in[0];
  CHECK(n >= 1 && n <= kScaleMaxEntries && in.size() >= 1 + 2 * (size_t)n + 2 * (size_t)ncol);
  std::vector<int> rows(n), in_place(n);
  int most = 0;
  size_t total = 0;
  for (int k = 0; k < n; ++k) { rows[k] = (int)in[1 + k]; in_place[k] = (int)in[1 + n + k]; CHECK(rows[k] > 0); most = rows[k] > most ? rows[k] : most; total += (size_t)rows[k] * ncol; }
  const double *num = in.data() + 1 + 2 * n, *den = num + ncol, *p = den + ncol;
  CHECK(in.size() == 1 + 2 * (size_t)n + 2 * (size_t)ncol + total);
  std::vector<std::vector<double>> src(n);
  for (int k = 0; k < n; ++k) { src[k].assign(p, p + (size_t)rows[k] * ncol); p += (size_t)rows[k] * ncol; }
  const std::vector<std::vector<double>> got = run_launch(ncol, n, rows, in_place, num, den, src, scale_grid_y(most));
  for (int ny : {1, 3}) {
    const std::vector<std::vector<double>> other = run_launch(ncol, n, rows, in_place, num, den, src, ny);
    for (int k = 0; k < n; ++k) CHECK(memcmp(other[k].data(), got[k].data(), got[k].size() * sizeof(double)) == 0);
  }
  std::vector<double> out;
  for (int k = 0; k < n; ++k) out.insert(out.end(), got[k].begin(), got[k].end());
  write_all(out_path, out);
  printf("ok (%d entries, %zu elements, %d row groups)\n", n, total, scale_grid_y(most));
  return 0;
}

int main(int argc, char **argv) {
  element_rules();
  CHECK(scale_grid_y(1) == 1 && scale_grid_y(8) == 1 && scale_grid_y(9) == 2 && scale_grid_y(61) == 8 && scale_grid_y(14 * 61) == kScaleMaxGridY);
  if (argc == 5 && !strcmp(argv[1], "mean")) return run_mean(atoi(argv[2]), argv[3], argv[4]);
  if (argc == 5 && !strcmp(argv[1], "scale")) return run_scale(atoi(argv[2]), argv[3], argv[4]);
  fprintf(stderr, "usage: %s mean|scale <ncol> <in.bin> <out.bin>\n", argv[0]);
  return 2;
}
