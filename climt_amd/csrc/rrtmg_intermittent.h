// rrtmg_intermittent.h -- the shortwave BETWEEN two radiation calls (rrtmg_hip_mean_coszen, rrtmg_hip_scale_columns): a model
// that calls the radiation every few steps hands it the cosine of the zenith angle averaged over the sunlit part of the
// interval the call stands for, and rescales the call's fluxes and heating rates at every step by that step's own insolation
// (Hogan & Hirahara 2016; Manners et al. 2009).  Both are OPT-IN and stand beside the radiation path: no kernel that does
// physics knows.
//
//   the sun over an interval   interval_sun: sun_position at t0, t1 and the midpoint -> declination of the midpoint, the hour
//                              angle of Greenwich at t0 (g0) and its advance to t1 (D, in (0, 2 pi): intervals of 12 h at most)
//   one column                 mean_coszen_column: A = sin(lat) sin(dec), B = cos(lat) cos(dec); h0 = g0 + lon in [-pi, pi),
//                              h1 = h0 + D; H = acos(clamp(-A / B)) the sunset hour angle (pi or 0 by the sign of A where B = 0:
//                              the poles); the sunlit set [h0, h1] n U_k [-H + 2 pi k, H + 2 pi k], k = -1, 0, 1, has up to TWO
//                              pieces (an interval that spans a short polar-summer night); S = their length,
//                              I = sum of A (b - a) + B (sin b - sin a); fraction = S / D, mean = I / S (0 where S = 0) in [0, 1]
//   one element of the rescale dst = src * s, s = den > 0 ? num / den : +0.0; s = 0 writes +0.0 whatever src holds
//
// The first part is plain C++ -- the sun's position (moved here from rrtmg_neighbours.hip, which includes this file: one
// statement for the zenith angle of an instant and of an interval), the interval, the column function, the element rule and
// the rows one thread of the rescale owns: tools/mean_coszen_check.cpp runs it on the CPU -- the table type is shared with
// the kernels in rrtmg_intermittent.hip.
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>

#ifdef __HIPCC__
#define RRTMG_INTERMITTENT_HD __host__ __device__ inline
#else
#define RRTMG_INTERMITTENT_HD inline
#endif

namespace rrtmg {

// ---- the sun at one instant (host): climt Instellation's helpers (instellation/component.py:90-99, 138-191), same arithmetic ----
struct SunPos { double sin_dec, cos_dec, ra, gmst; };

inline double deg2rad(double x) { return x * (M_PI / 180.0); }

inline SunPos sun_position(double t) {
  const double eps = deg2rad(23.0 + 26.0 / 60 + 21.406 / 3600.0 -
                             (46.836769 * t - 0.0001831 * (t * t) + 0.00200340 * (t * t * t) - 0.576e-6 * (t * t * t * t) -
                              4.34e-8 * (t * t * t * t * t)) / 3600.0);
  const double mean_anomaly = deg2rad(357.52910 + 35999.05030 * t - 0.0001559 * t * t - 0.00000048 * t * t * t);
  const double mean_longitude = deg2rad(280.46645 + 36000.76983 * t + 0.0003032 * (t * t));
  const double d_l = deg2rad((1.914600 - 0.004817 * t - 0.000014 * (t * t)) * sin(mean_anomaly) +
                             (0.019993 - 0.000101 * t) * sin(2 * mean_anomaly) + 0.000290 * sin(3 * mean_anomaly));
  const double eclon = mean_longitude + d_l;
  const double x = cos(eclon), y = cos(eps) * sin(eclon), z = sin(eps) * sin(eclon);
  const double r = sqrt(1.0 - z * z);
  const double declination = atan2(z, r);
  SunPos s;
  s.sin_dec = sin(declination); s.cos_dec = cos(declination);
  s.ra = 2.0 * atan2(y, (x + r));
  // "6.2 * 10e-6" is the reference's literal (component.py:186)
  const double theta = 67310.54841 + t * (876600.0 * 3600 + 8640184.812866 + t * (0.093104 - t * 6.2 * 10e-6));
  double g = fmod(deg2rad(theta / 240.0), 2.0 * M_PI);
  if (g < 0) g += 2.0 * M_PI;   // numpy's % is non-negative for a positive modulus
  s.gmst = g;
  return s;
}

// ---- the sun over an interval [t0, t1] (Julian centuries) --------------------------------------------------------------------
// 12 hours at the most (the advance of the hour angle is then unambiguous); the slack is for a t1 formed as t0 + 12 h in doubles
constexpr double kMeanCoszenMaxCenturies = 0.5 / 36525.0 * (1.0 + 1.0e-9);
inline bool interval_ok(double t0, double t1) { return t1 > t0 && t1 - t0 <= kMeanCoszenMaxCenturies; }

struct IntervalSun { double sin_dec, cos_dec, g0, D; };
inline bool interval_sun_ok(const IntervalSun &s) { return s.D > 0.0 && s.D < 2.0 * M_PI; }

inline IntervalSun interval_sun(double t0, double t1) {
  const SunPos a = sun_position(t0), b = sun_position(t1), m = sun_position(0.5 * (t0 + t1));
  IntervalSun s;
  s.sin_dec = m.sin_dec; s.cos_dec = m.cos_dec;
  s.g0 = a.gmst - a.ra;
  double d = fmod((b.gmst - b.ra) - s.g0, 2.0 * M_PI);
  if (d <= 0) d += 2.0 * M_PI;
  s.D = d;
  return s;
}

// ---- one column --------------------------------------------------------------------------------------------------------------
struct MeanCoszen { double mean, fraction; };

RRTMG_INTERMITTENT_HD MeanCoszen mean_coszen_column(double lat_deg, double lon_deg, const IntervalSun &s) {
#pragma clang fp contract(off)   // every product and sum rounded on its own, as the numpy statement of the definition is
  const double pi = 3.14159265358979323846, two_pi = 2.0 * pi;
  const double lat = lat_deg * (pi / 180.0);
  // (the cosine of the double nearest pi/2 is 6e-17: a pole is a pole by its latitude in degrees)
  const double cos_lat = fabs(lat_deg) == 90.0 ? 0.0 : cos(lat);
  const double A = sin(lat) * s.sin_dec, B = cos_lat * s.cos_dec;
  double h0 = s.g0 + lon_deg * (pi / 180.0);
  h0 = h0 - two_pi * floor((h0 + pi) / two_pi);
  if (h0 >= pi) h0 -= two_pi; else if (h0 < -pi) h0 += two_pi;
  const double h1 = h0 + s.D;
  double H;
  if (B > 0.0) {
    double x = -A / B;
    if (x > 1.0) x = 1.0; else if (x < -1.0) x = -1.0;
    H = acos(x);
  } else {
    H = A > 0.0 ? pi : 0.0;
  }
  double S = 0.0, I = 0.0;
  for (int k = -1; k <= 1; ++k) {
    const double c = two_pi * k;
    const double a = fmax(h0, c - H), b = fmin(h1, c + H);
    if (b > a) {
      S = S + (b - a);
      I = I + (A * (b - a) + B * (sin(b) - sin(a)));
    }
  }
  MeanCoszen r;
  r.fraction = S / s.D;
  double m = S > 0.0 ? I / S : 0.0;
  if (m > 1.0) m = 1.0; else if (!(m > 0.0)) m = 0.0;
  r.mean = m;
  return r;
}
// what the call may write beside the two: the zenith angle a shortwave call takes for the interval -- pi/2 (the double the
// night-column skip tests against) where the mean is 0 -- and the interval-mean insolation factor mean * fraction
RRTMG_INTERMITTENT_HD double mean_zenith(double mean) { return mean > 0.0 ? acos(mean) : 1.5707963267948966; }
RRTMG_INTERMITTENT_HD double mean_insolation(const MeanCoszen &r) {
#pragma clang fp contract(off)
  return r.mean * r.fraction;
}

// ---- the rescale: ONE rule for the device and the CPU check -------------------------------------------------------------------
RRTMG_INTERMITTENT_HD double scale_factor(double num, double den) { return den > 0.0 ? num / den : 0.0; }
// s = 0 (-0.0 too): +0.0, never -0.0 and never NaN * 0
RRTMG_INTERMITTENT_HD double scale_element(double x, double s) { return s == 0.0 ? 0.0 : x * s; }

// One table entry: src, dst [rows][ncol] (dst == src: in place).  The table goes to the kernel by value, one entry per blockIdx.z
// (the pattern of permute_gather_kernel and narrow_kernel); the public rrtmg_scale_entry (include/rrtmg_hip.h) has this layout.
struct ScaleEntry { const double *src; double *dst; int32_t rows, reserved; };
constexpr int kScaleMaxEntries = 16;
struct ScaleTable { ScaleEntry e[kScaleMaxEntries]; };
static_assert(sizeof(ScaleTable) + 40 <= 4096, "kernel arguments: 4 KB at the most");
constexpr int kScaleRows = 8;        // rows a thread keeps in flight per trip
constexpr int kScaleMaxGridY = 64;   // row groups side by side at the most: a deeper array is walked in trips
inline int scale_grid_y(int max_rows) {
  const int g = (max_rows + kScaleRows - 1) / kScaleRows;
  return g < 1 ? 1 : (g > kScaleMaxGridY ? kScaleMaxGridY : g);
}
// The work of thread (col, y) of a launch `ny` row groups deep on one entry: rows [8 y, 8 y + 8), then ny * 8 further on, ...
// Every element of the entry's column `col` is read once and written once by exactly one y: in place is safe.
RRTMG_INTERMITTENT_HD void scale_thread(const ScaleEntry &e, long ncol, long col, int y, int ny, double s) {
  for (int r0 = y * kScaleRows; r0 < e.rows; r0 += ny * kScaleRows) {
    double v[kScaleRows];
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
    for (int k = 0; k < kScaleRows; ++k) if (r0 + k < e.rows) v[k] = __builtin_nontemporal_load(e.src + (long)(r0 + k) * ncol + col);
#pragma unroll
    for (int k = 0; k < kScaleRows; ++k) if (r0 + k < e.rows) __builtin_nontemporal_store(scale_element(v[k], s), e.dst + (long)(r0 + k) * ncol + col);
#else
    for (int k = 0; k < kScaleRows; ++k) if (r0 + k < e.rows) v[k] = e.src[(long)(r0 + k) * ncol + col];
    for (int k = 0; k < kScaleRows; ++k) if (r0 + k < e.rows) e.dst[(long)(r0 + k) * ncol + col] = scale_element(v[k], s);
#endif
  }
}

}  // namespace rrtmg
