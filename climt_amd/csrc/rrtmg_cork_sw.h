// rrtmg_cork_sw.h -- the reference's table-driven correlated-k two-stream shortwave for ONE column and ONE band: CorkShortwaveRadiation
// with optics "correlated_k" and additive overlap (climt/_components/cork/sw/component.py: array_call; cork/sw/kernels.py: _delta_scale,
// _sw_dif_and_source, _adding, _sw_two_stream_core; cork/optics/correlated_k.py and cork/common.py as in rrtmg_cork.h).  Level 0 is the
// surface; interface i lies below layer i; profiles are [k][ncol], columns fastest; per-band arrays [band][k][ncol]; the three cloud
// arrays [k][ncol][band].
//
//   gas depth      tau_abs: cork_gas_depth of rrtmg_cork.h -- the brackets, the three gas-amount rules, k summed over the gases from 0.0,
//                  the band-grey continuum behind it.  Tables of rank 5 and 6 (the reference's shortwave passes no CO2 mole fraction)
//   Rayleigh       with rayleigh_coefficient: tau_ray = (rayleigh[b] dp) / g, dp = |pint[k+1] - pint[k]|;  tau = tau_abs + tau_ray;
//                  ssa = tau > 0 ? tau_ray / tau : 0.  Without: tau = tau_abs, ssa = 0
//   cloud mixing   tau_total = tau + tau_c;  scat_gas = tau ssa;  scat_cloud = tau_c ssa_c;  scat_total = scat_gas + scat_cloud;
//                  ssa_total = tau_total > 0 ? scat_total / tau_total : 0;
//                  g_total = scat_total > 0 ? (scat_gas 0.0 + scat_cloud g_c) / scat_total : 0.  Without cloud arrays the same with
//                  tau_c = ssa_c = g_c = 0.0: (tau ssa) / tau is not ssa in every bit, and the reference always mixes
//   delta scaling  f = g g;  tau_s = tau (1 - ssa f);  ssa_s = (1 - ssa f) > 1e-30 ? (ssa (1 - f)) / (1 - ssa f) : 0;
//                  g_s = (1 - f) > 1e-30 ? (g - f) / (1 - f) : 0
//   layer          gamma1 = (8 - w0 (5 + 3 g)) 0.25;  gamma2 = (3 (w0 (1 - g))) 0.25;  k = sqrt(max((gamma1 - gamma2) (gamma1 + gamma2), 1e-12));
//                  e1 = exp((-tau) k), e2 = e1 e1;  RT = 1 / (k (1 + e2) + gamma1 (1 - e2));  Rdif = (RT gamma2) (1 - e2);
//                  Tdif = ((RT 2) k) e1;  mu = max(mu0, 1e-8);  Tnoscat = exp((-tau) / mu);  kmu = k mu;  den = 1 - kmu kmu, 1e-30 where
//                  |den| < 1e-30;  RTd = (w0 RT) / den;  gamma3 = (2 - (3 mu) g) 0.25, gamma4 = 1 - gamma3;  alpha1 = gamma1 gamma4 + gamma2 gamma3,
//                  alpha2 = gamma1 gamma3 + gamma2 gamma4;  Rdir and Tdir as Meador & Weaver's Eqs. 14 and 15 in the reference's grouping
//                  (cork_sw_layer below), then Rdir = max(0, min(Rdir, 1 - Tnoscat)), Tdir = max(0, min(Tdir, 1 - Tnoscat - Rdir))
//                  with Python's max and min (the first argument unless the second is strictly beyond it)
//   direct beam    dir[nlay] = 1.0;  dir[k] = Tnoscat[k] dir[k+1];  src_up[k] = Rdir[k] dir[k+1], src_dn[k] = Tdir[k] dir[k+1]
//   adding         alb[0] = albedo, src[0] = dir[0] albedo;  upward: denom = 1 / (1 - Rdif alb[k]);  alb[k+1] = Rdif + ((Tdif Tdif) alb[k]) denom;
//                  src[k+1] = src_up + (Tdif denom) (src[k] + alb[k] src_dn);  downward from dn[nlay] = 0.0: up[nlay] = dn[nlay] alb[nlay] + src[nlay];
//                  dn[k] = (Tdif dn[k+1] + Rdif src[k] + src_dn) denom;  up[k] = dn[k] alb[k] + src[k]
//   accumulation   scale = (solar_flux[b][g] mu0) w[b][g];  up_band = 0.0 + up_0 scale_0 + up_1 scale_1 + ... in ascending g;  dn_band likewise of
//                  (dir + dn);  tau_band = 0.0 + w0 tau0 + ... of the UNSCALED total depth;  the broadband sums, tend, hr and hr_band as
//                  in rrtmg_cork.h (cork_broadband is called as it is)
//   sun            mu0 = cos(zenith);  a column with mu0 <= 1e-4 contributes nothing: +0.0 in every flux, its heating what the formula
//                  makes of zeros (pressures fall upward: -0.0); tau_band is formed all the same.  solar_flux = solar_source factor, where
//                  factor is earth_sun of the FIRST column for every column, and in a float32 table factor is rounded to float and the
//                  product is a float product (the reference multiplies in the table's element type)
// Every operation is rounded on its own (contraction off), in the reference's order; exp is cork_exp.
//
// One thread owns one (column, band): layers in the outer loop, g-points in the inner one under the compile-time bound NG, the
// running beam, albedo, source and downward flux of the g-points in registers.  The adding method reads, top-down, what the upward
// recursion made bottom-up (alb, src) and, bottom-up, what the beam made top-down (dir): those three rows per (g-point, level,
// column) go to a work space in global memory, [band][g][row][level][column] with `work_cols` columns, columns fastest.  Everything
// else -- the optical depth, the layer operator, denom -- is formed again by the same function, hence to the same bits: three
// passes (beam down, adding up, fluxes down).  The entry (rrtmg_cork_sw.hip) runs the columns in chunks so that the work space stays
// below kCorkSwWorkCap.
//
// Plain C++: tools/cork_sw_check.cpp runs every "thread" of a launch on the CPU; the kernels are in rrtmg_cork_sw.hip.
#pragma once
#include "rrtmg_cork.h"

namespace rrtmg {

constexpr size_t kCorkSwWorkCap = (size_t)512 << 20;      // bytes of work space at most (one chunk of at least 64 columns is always run)
constexpr double kCorkSwMinK = 1.0e-12, kCorkSwMinMu0 = 1.0e-8, kCorkSwNight = 1.0e-4;

struct CorkShortwaveCall {
  int32_t ncol, nlay, gas_rule, solar_f32;
  int64_t col0, cols, work_cols;   // this launch: columns col0 .. col0 + cols - 1; the column extent of the work space
  CorkTableView tab;               // (planck is not read)
  const double *solar;             // [nband][ngpt]: solar_source_per_gpoint, a float table's widened
  const double *rayleigh;          // [nband] or nullptr
  const double *t, *pmid;          // [nlay][ncol]
  const double *pint;              // [nlay+1][ncol]
  const double *zenith, *albedo, *earth_sun;   // [ncol]
  const double *taucld, *ssacld, *asycld;      // [nlay][ncol][nband], all three or none
  const double *gas0, *gas1, *gas2, *gas3, *gas4, *gas5, *gas6, *gas7;   // [nlay][ncol]
  double gas_scale[kCorkMaxGas];
  double m_h2o, g, cpd, pressure_scale;
  double *up, *dn;                 // [nlay+1][ncol]
  double *tend;                    // [nlay][ncol]
  double *hr;                      // [nlay][ncol] or nullptr
  double *up_band, *dn_band;       // [nband][nlay+1][ncol]: the caller's, or the entry's work space
  double *tau_band, *hr_band;      // [nband][nlay][ncol] or nullptr
  double *work;                    // [nband][ngpt][3][nlay+1][work_cols]
};

// the bytes of work space one column takes
inline size_t cork_sw_work_per_column(size_t nband, size_t ngpt, size_t nlay) { return nband * ngpt * 3 * (nlay + 1) * sizeof(double); }
// the columns of a chunk: what the cap holds, in whole waves, at least one wave; a caller's max_chunk_cols (> 0) below that
inline size_t cork_sw_chunk_cols(size_t nband, size_t ngpt, size_t nlay, size_t ncol, size_t max_chunk_cols) {
  size_t cols = kCorkSwWorkCap / cork_sw_work_per_column(nband, ngpt, nlay) / 64 * 64;
  if (cols < 64) cols = 64;
  if (max_chunk_cols > 0 && max_chunk_cols < cols) cols = max_chunk_cols;
  return cols < ncol ? cols : ncol;
}

// ---- _delta_scale -----------------------------------------------------------------------------------------------------------------------
RRTMG_CORK_HD void cork_sw_delta_scale(double tau, double ssa, double g, double &tau_s, double &ssa_s, double &g_s) {
#pragma clang fp contract(off)
  const double f = g * g;
  tau_s = tau * (1.0 - ssa * f);
  ssa_s = (1.0 - ssa * f) > 1e-30 ? ssa * (1.0 - f) / (1.0 - ssa * f) : 0.0;
  g_s = (1.0 - f) > 1e-30 ? (g - f) / (1.0 - f) : 0.0;
}

// ---- the direct transmittance of _sw_dif_and_source alone (the beam pass needs no more) ------------------------------------------------
RRTMG_CORK_HD double cork_sw_tnoscat(double tau, double mu0) {
#pragma clang fp contract(off)
  const double mu0_s = kCorkSwMinMu0 > mu0 ? kCorkSwMinMu0 : mu0;
  return cork_exp(-tau / mu0_s);
}

// ---- _sw_dif_and_source: the layer operator of delta-scaled (tau, w0, g) under the sun at mu0 --------------------------------------------
struct CorkSwLayer { double Rdif, Tdif, Rdir, Tdir, Tnoscat; };
RRTMG_CORK_HD CorkSwLayer cork_sw_layer(double tau, double w0, double g, double mu0) {
#pragma clang fp contract(off)
  CorkSwLayer o;
  const double gamma1 = (8.0 - w0 * (5.0 + 3.0 * g)) * 0.25;
  const double gamma2 = 3.0 * (w0 * (1.0 - g)) * 0.25;
  const double kk2 = (gamma1 - gamma2) * (gamma1 + gamma2);
  const double k = sqrt(kCorkSwMinK > kk2 ? kCorkSwMinK : kk2);
  const double e1 = cork_exp(-tau * k);
  const double e2 = e1 * e1;
  const double RT = 1.0 / (k * (1.0 + e2) + gamma1 * (1.0 - e2));
  o.Rdif = RT * gamma2 * (1.0 - e2);
  o.Tdif = RT * 2.0 * k * e1;
  const double mu0_s = kCorkSwMinMu0 > mu0 ? kCorkSwMinMu0 : mu0;
  o.Tnoscat = cork_exp(-tau / mu0_s);
  const double k_mu = k * mu0_s;
  double denom_dir = 1.0 - k_mu * k_mu;
  if (fabs(denom_dir) < 1e-30) denom_dir = 1e-30;
  const double RTd = w0 * RT / denom_dir;
  const double gamma3 = (2.0 - 3.0 * mu0_s * g) * 0.25;
  const double gamma4 = 1.0 - gamma3;
  const double alpha1 = gamma1 * gamma4 + gamma2 * gamma3;
  const double alpha2 = gamma1 * gamma3 + gamma2 * gamma4;
  const double k_gamma3 = k * gamma3, k_gamma4 = k * gamma4;
  double Rdir = RTd * ((1.0 - k_mu) * (alpha2 + k_gamma3) - (1.0 + k_mu) * (alpha2 - k_gamma3) * e2 - 2.0 * (k_gamma3 - alpha2 * k_mu) * e1 * o.Tnoscat);
  double Tdir = -RTd * ((1.0 + k_mu) * (alpha1 + k_gamma4) * o.Tnoscat - (1.0 - k_mu) * (alpha1 - k_gamma4) * e2 * o.Tnoscat - 2.0 * (k_gamma4 + alpha1 * k_mu) * e1);
  // the two energy clamps: Python's min(x, lim) is lim only where lim < x, max(0.0, x) is x only where x > 0.0
  const double lim_r = 1.0 - o.Tnoscat;
  Rdir = lim_r < Rdir ? lim_r : Rdir;
  Rdir = Rdir > 0.0 ? Rdir : 0.0;
  const double lim_t = 1.0 - o.Tnoscat - Rdir;
  Tdir = lim_t < Tdir ? lim_t : Tdir;
  Tdir = Tdir > 0.0 ? Tdir : 0.0;
  o.Rdir = Rdir; o.Tdir = Tdir;
  return o;
}

// ---- what a layer adds to the gas depth, the same for every g-point of the band ----------------------------------------------------------
struct CorkSwMix { double tau_ray, tau_c, ssa_c, g_c; };
RRTMG_CORK_HD CorkSwMix cork_sw_mix_of(const CorkShortwaveCall &a, long col, int b, int k) {
#pragma clang fp contract(off)
  const long N = a.ncol, o = (long)k * N + col;
  CorkSwMix m;
  m.tau_ray = 0.0;
  if (a.rayleigh) {
    const double dp = fabs(a.pint[o + N] * a.pressure_scale - a.pint[o] * a.pressure_scale);
    m.tau_ray = a.rayleigh[b] * dp / a.g;
  }
  const long oc = o * a.tab.nband + b;
  m.tau_c = a.taucld ? a.taucld[oc] : 0.0;
  m.ssa_c = a.taucld ? a.ssacld[oc] : 0.0;
  m.g_c = a.taucld ? a.asycld[oc] : 0.0;
  return m;
}
// the total optical properties of one g-point: Rayleigh, then the cloud
RRTMG_CORK_HD void cork_sw_mix(double tau_abs, const CorkSwMix &m, bool has_rayleigh, double &tau, double &ssa, double &asy) {
#pragma clang fp contract(off)
  double tg = tau_abs, sg = 0.0;
  if (has_rayleigh) {
    tg = tau_abs + m.tau_ray;
    sg = tg > 0.0 ? m.tau_ray / tg : 0.0;
  }
  const double tau_total = tg + m.tau_c;
  const double scat_gas = tg * sg, scat_cloud = m.tau_c * m.ssa_c;
  const double scat_total = scat_gas + scat_cloud;
  tau = tau_total;
  ssa = tau_total > 0.0 ? scat_total / tau_total : 0.0;
  asy = scat_total > 0.0 ? (scat_gas * 0.0 + scat_cloud * m.g_c) / scat_total : 0.0;
}

// scale = (solar_flux mu0) w, solar_flux formed in the table's element type from the first column's factor
RRTMG_CORK_HD double cork_sw_scale(const CorkShortwaveCall &a, int b, int g, double mu0) {
#pragma clang fp contract(off)
  const int i = b * a.tab.ngpt + g;
  const double factor = a.earth_sun[0];
  const double flux = a.solar_f32 ? (double)((float)a.solar[i] * (float)factor) : a.solar[i] * factor;
  return flux * mu0 * a.tab.weights[i];
}

// ---- one (column, band): the three passes, the per-band outputs ---------------------------------------------------------------------------
template <int NG, class K>
RRTMG_CORK_HD void cork_sw_band_column(const CorkShortwaveCall &a, long col, int b) {
#pragma clang fp contract(off)
  const CorkTableView &tb = a.tab;
  const long N = a.ncol, W = a.work_cols;
  const int nlay = a.nlay, ngpt = tb.ngpt;
  const long nlev = nlay + 1;
  double *const ub = a.up_band + (long)b * nlev * N + col, *const db = a.dn_band + (long)b * nlev * N + col;
  const long ob = (long)b * nlay * N + col;
  // row r of g-point g at level 0 of this column; a level is W doubles on
  double *const work = a.work + (long)b * ngpt * 3 * nlev * W + (col - a.col0);
  const long sRow = nlev * W, sG = 3 * sRow;
  const bool has_ray = a.rayleigh != nullptr;
  const double mu0 = cos(a.zenith[col]);
  const bool night = mu0 <= kCorkSwNight;
  double acc[NG], run0[NG], run1[NG];
  int iT;
  double fT;

  // the beam, downwards: run0 is dir
#pragma unroll
  for (int g = 0; g < NG; ++g) {
    if (g >= ngpt) continue;
    run0[g] = 1.0;
    if (!night) work[g * sG + (long)nlay * W] = 1.0;
  }
  for (int k = nlay - 1; k >= 0; --k) {
    if (night && !a.tau_band) break;      // a dark column's beam pass has one consumer, the band's optical depth
    cork_gas_depth<NG, K>(a, col, b, k, acc, iT, fT);
    const CorkSwMix m = cork_sw_mix_of(a, col, b, k);
    double depth = 0.0;
#pragma unroll
    for (int g = 0; g < NG; ++g) {
      if (g >= ngpt) continue;
      double tau, ssa, asy;
      cork_sw_mix(acc[g], m, has_ray, tau, ssa, asy);
      depth += tb.weights[b * ngpt + g] * tau;
      if (night) continue;
      double tau_s, ssa_s, g_s;
      cork_sw_delta_scale(tau, ssa, asy, tau_s, ssa_s, g_s);
      run0[g] = cork_sw_tnoscat(tau_s, mu0) * run0[g];
      work[g * sG + (long)k * W] = run0[g];
    }
    if (a.tau_band) a.tau_band[ob + (long)k * N] = depth;
  }
  if (night) {      // nothing is accumulated: the zeros the reference's arrays were made with, and the heating of zeros
    double p_hi = a.pint[(long)nlay * N + col] * a.pressure_scale;
    ub[(long)nlay * N] = 0.0; db[(long)nlay * N] = 0.0;
    for (int k = nlay - 1; k >= 0; --k) {
      ub[(long)k * N] = 0.0; db[(long)k * N] = 0.0;
      if (a.hr_band) {
        const double p_lo = a.pint[(long)k * N + col] * a.pressure_scale;
        a.hr_band[ob + (long)k * N] = a.g / a.cpd * ((0.0 - 0.0) - (0.0 - 0.0)) / (p_hi - p_lo) * 86400.0;
        p_hi = p_lo;
      }
    }
    return;
  }

  // adding, upwards: run0 is alb, run1 is src
  {
    const double albedo = a.albedo[col];
#pragma unroll
    for (int g = 0; g < NG; ++g) {
      if (g >= ngpt) continue;
      const double src_sfc = run0[g] * albedo;      // run0: the beam at the surface
      run0[g] = albedo; run1[g] = src_sfc;
      work[g * sG + sRow] = albedo;
      work[g * sG + 2 * sRow] = src_sfc;
    }
  }
  for (int k = 0; k < nlay; ++k) {
    cork_gas_depth<NG, K>(a, col, b, k, acc, iT, fT);
    const CorkSwMix m = cork_sw_mix_of(a, col, b, k);
#pragma unroll
    for (int g = 0; g < NG; ++g) {
      if (g >= ngpt) continue;
      double tau, ssa, asy, tau_s, ssa_s, g_s;
      cork_sw_mix(acc[g], m, has_ray, tau, ssa, asy);
      cork_sw_delta_scale(tau, ssa, asy, tau_s, ssa_s, g_s);
      const CorkSwLayer L = cork_sw_layer(tau_s, ssa_s, g_s, mu0);
      const double dir_top = work[g * sG + (long)(k + 1) * W];
      const double src_up = L.Rdir * dir_top, src_dn = L.Tdir * dir_top;
      const double denom = 1.0 / (1.0 - L.Rdif * run0[g]);
      const double alb = L.Rdif + L.Tdif * L.Tdif * run0[g] * denom;
      const double src = src_up + L.Tdif * denom * (run1[g] + run0[g] * src_dn);
      run0[g] = alb; run1[g] = src;
      work[g * sG + sRow + (long)(k + 1) * W] = alb;
      work[g * sG + 2 * sRow + (long)(k + 1) * W] = src;
    }
  }

  // the fluxes, downwards: run0 becomes the downward diffuse flux
  double net_hi, p_hi = a.pint[(long)nlay * N + col] * a.pressure_scale;
  {
    double up_sum = 0.0, dn_sum = 0.0;
#pragma unroll
    for (int g = 0; g < NG; ++g) {
      if (g >= ngpt) continue;
      const double scale = cork_sw_scale(a, b, g, mu0);
      const double dn = 0.0, up = dn * run0[g] + run1[g];
      up_sum += up * scale;
      dn_sum += (1.0 + dn) * scale;
      run0[g] = dn;
    }
    ub[(long)nlay * N] = up_sum; db[(long)nlay * N] = dn_sum;
    net_hi = up_sum - dn_sum;
  }
  for (int k = nlay - 1; k >= 0; --k) {
    cork_gas_depth<NG, K>(a, col, b, k, acc, iT, fT);
    const CorkSwMix m = cork_sw_mix_of(a, col, b, k);
    double up_sum = 0.0, dn_sum = 0.0;
#pragma unroll
    for (int g = 0; g < NG; ++g) {
      if (g >= ngpt) continue;
      double tau, ssa, asy, tau_s, ssa_s, g_s;
      cork_sw_mix(acc[g], m, has_ray, tau, ssa, asy);
      cork_sw_delta_scale(tau, ssa, asy, tau_s, ssa_s, g_s);
      const CorkSwLayer L = cork_sw_layer(tau_s, ssa_s, g_s, mu0);
      const double dir_top = work[g * sG + (long)(k + 1) * W], dir_k = work[g * sG + (long)k * W];
      const double alb_k = work[g * sG + sRow + (long)k * W], src_k = work[g * sG + 2 * sRow + (long)k * W];
      const double src_dn = L.Tdir * dir_top;
      const double denom = 1.0 / (1.0 - L.Rdif * alb_k);
      const double dn = (L.Tdif * run0[g] + L.Rdif * src_k + src_dn) * denom;
      const double up = dn * alb_k + src_k;
      const double scale = cork_sw_scale(a, b, g, mu0);
      up_sum += up * scale;
      dn_sum += (dir_k + dn) * scale;
      run0[g] = dn;
    }
    ub[(long)k * N] = up_sum; db[(long)k * N] = dn_sum;
    if (a.hr_band) {
      const double net_lo = up_sum - dn_sum, p_lo = a.pint[(long)k * N + col] * a.pressure_scale;
      a.hr_band[ob + (long)k * N] = a.g / a.cpd * (net_hi - net_lo) / (p_hi - p_lo) * 86400.0;
      net_hi = net_lo; p_hi = p_lo;
    }
  }
}

}  // namespace rrtmg
