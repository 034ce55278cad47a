// rrtmg_cork.h -- the reference's table-driven correlated-k longwave for ONE column and ONE band: CorkLongwaveRadiation with optics
// "correlated_k" and additive overlap (climt/_components/cork/lw/component.py: array_call; cork/optics/correlated_k.py: _ck_bracket,
// _ck_txx7, _txx, _tp, interpolate_continuum, _ck_tau_additive_co2_kernel; cork/lw/kernels.py: planck_sources_kernel,
// _lw_transport_kernel; cork/common.py: compute_column_amount, compute_heating_rate).  Level 0 is the surface; interface i lies
// below layer i; profiles are [k][ncol], columns fastest; per-band arrays [band][k][ncol]; the cloud depth [k][ncol][band].
//
//   bracket        i = (number of nodes < v) - 1, clamped to 0 .. n-2;  f = (v - grid[i]) / (grid[i+1] - grid[i]), clamped to 0 .. 1
//   layer          T;  log(max(p, 1));  with an H2O axis x = q / max(q + (1 - q) m_h2o, 1e-30), clipped to the axis' first and last
//                  node, log(max(x, 1e-30));  with a CO2 axis the same of the CO2 mole fraction;  dp = |pint[k+1] - pint[k]|
//   amounts        rule 0 and 1: gas 0 has dp / g, any other gas 0.0;  rule 2: ((q_gas scale_gas) dp) / g
//   k              rank 5: ((v00 (1-fT)) (1-fP) + (v10 fT) (1-fP) + (v01 (1-fT)) fP + (v11 fT) fP), summed left to right;  rank 6: x0
//                  of the four corners at iX, x1 of those at iX+1, x0 (1-fX) + x1 fX;  rank 7: that at iC and at iC+1,
//                  exp(log(max(c0, 1e-40)) (1-fC) + log(max(c1, 1e-40)) fC)
//   tau            acc = 0.0; acc += k amount by gas in ascending order;  with a continuum acc += exp(trilinear log_cont) amount[0];
//                  then + the band's cloud depth of the layer
//   source         (pf[iT] (1-fT) + pf[iT+1] fT) (sigma pow(T, 4)) with the bracket of T;  the surface likewise with tsfc, times emis
//   sweeps         trans = exp(-D tau);  up = up_prev trans + src (1 - trans) from the surface;  dn likewise from +0.0 at the top;
//                  the band's flux at a level is 0.0 + w0 f0 + w1 f1 + ... in ascending g
//   band outputs   tau_band = 0.0 + w0 tau0 + ...;  trans_band = exp(-D tau_band);
//                  hr_band = (((g / cpd) (net[k+1] - net[k])) / (pint[k+1] - pint[k])) 86400.0 of the band's own net = up - dn
//   broadband      up = 0.0 + up_band[0] + up_band[1] + ...;  dn likewise;  tend of net = up - dn as above, in K/s;  hr = tend 86400.0
// Every operation is rounded on its own (contraction off), in the reference's order.  numpy's `x ** 4` is pow(x, 4.0): cork_pow4;
// exp is cork_exp (below: why neither is the device library's).
//
// One thread owns one (column, band): layers in the outer loop, g-points in the inner one, the running fluxes of the g-points in
// registers (NG is the compile-time bound of the g-point loops, so no array is indexed dynamically).  The downward sweep forms the
// layer's optical depths and sources AGAIN with the same function: same operations, same bits, nothing with a g-point axis stored.
// The table is read in the layout rrtmg_cork.hip gives it on the device: the g-points of one corner lie side by side,
//   k [ngas][nband][nT][nP][nX'][nC'][ngpt] (nX' = max(nX, 1), nC' likewise), planck [nband][nT][ngpt].
//
// The gas optical depth (brackets, amounts, k, continuum: cork_gas_depth) is what the shortwave of the same scheme runs too
// (rrtmg_cork_sw.h): one function, templated on the call struct.
// Plain C++: tools/cork_check.cpp runs every "thread" of a launch on the CPU; the kernels are in rrtmg_cork.hip.
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>

#ifdef __HIPCC__
#define RRTMG_CORK_HD __host__ __device__ inline
#else
#define RRTMG_CORK_HD inline
#endif

namespace rrtmg {

constexpr int kCorkMaxGas = 8, kCorkMaxBand = 32, kCorkMaxGpt = 16;

struct CorkTableView {
  int32_t ngas, nband, ngpt, nT, nP, nX, nC;   // nX, nC: 0 where the table has no such axis
  int32_t k_f32, has_cont;
  const void *k;                               // float or double (k_f32), the device layout above
  const double *weights, *planck, *t_grid, *p_grid, *x_grid, *c_grid;   // the two mole-fraction grids in log
  const double *log_cont;                      // [nband][nT][nP][nX]
  double x_lo, x_hi, c_lo, c_hi;
};

struct CorkLongwaveCall {
  int32_t ncol, nlay, gas_rule;
  CorkTableView tab;
  const double *t, *pmid;       // [nlay][ncol]
  const double *pint;           // [nlay+1][ncol]
  const double *tsfc;           // [ncol]
  const double *emis;           // [nband][ncol]
  const double *taucld;         // [nlay][ncol][nband] or nullptr
  const double *gas0, *gas1, *gas2, *gas3, *gas4, *gas5, *gas6, *gas7;   // [nlay][ncol]
  double gas_scale[kCorkMaxGas];
  double m_h2o, sigma_sb, g, cpd, diffusivity, pressure_scale;
  double *up, *dn;              // [nlay+1][ncol]
  double *tend;                 // [nlay][ncol]
  double *hr;                   // [nlay][ncol] or nullptr
  double *up_band, *dn_band;    // [nband][nlay+1][ncol]: the caller's, or the entry's work space
  double *tau_band, *trans_band, *hr_band;   // [nband][nlay][ncol] or nullptr
};

// (Call: CorkLongwaveCall, or the shortwave's call struct of rrtmg_cork_sw.h, which names the same members)
template <class Call>
RRTMG_CORK_HD const double *cork_gas(const Call &a, int ig) {
  return ig == 0 ? a.gas0 : ig == 1 ? a.gas1 : ig == 2 ? a.gas2 : ig == 3 ? a.gas3 : ig == 4 ? a.gas4 : ig == 5 ? a.gas5 : ig == 6 ? a.gas6 : a.gas7;
}
// (chains of selects, not indexed loads: a kernel's by-value argument that is indexed dynamically is copied to scratch)
template <class Call>
RRTMG_CORK_HD double cork_gas_scale(const Call &a, int ig) {
  return ig == 0 ? a.gas_scale[0] : ig == 1 ? a.gas_scale[1] : ig == 2 ? a.gas_scale[2] : ig == 3 ? a.gas_scale[3] : ig == 4 ? a.gas_scale[4]
       : ig == 5 ? a.gas_scale[5] : ig == 6 ? a.gas_scale[6] : a.gas_scale[7];
}

// ---- exp and x^4 rounded to within 0.53 ulp (exp: where the result is normal) ----------------------------------------------------------------------------------------------
// The sweeps take 1 - exp(-D tau) of layers that are nearly transparent and differences of fluxes that nearly cancel: there the last
// bit of exp is the leading error of the heating rate.  numpy's (and libm's) exp and pow are good to about half an ulp; a device
// library function that is good to one ulp differs from them often enough to show.  So both are formed here, the same way on the
// device and on the host: exp(x) = 2^k exp(r), r = x - k ln2 carried as rh + rl, exp(r) = 1 + rh + rh^2 / 2 in double-double plus
// the terms from r^3 / 6 on in double (|r| <= 0.347: at most 0.0073, so their rounding is below 2e-18);  x^4 as the square of
// x^2 = h + l in double-double.  A subnormal result of exp is rounded a second time by ldexp (0.75 ulp seen near x = -709; such a
// transmittance is below 1e-307).  fma() is called by name: contraction stays off.
RRTMG_CORK_HD void cork_two_sum(double a, double b, double &s, double &e) {
#pragma clang fp contract(off)
  s = a + b;
  const double bb = s - a;
  e = (a - (s - bb)) + (b - bb);
}
RRTMG_CORK_HD double cork_exp(double x) {
#pragma clang fp contract(off)
  if (!(x == x)) return x;
  if (x > 709.79) return HUGE_VAL;
  if (x < -745.2) return 0.0;
  const double k = rint(x * 1.4426950408889634);
  const double rh = fma(-k, 6.93147180369123816490e-01, x), rl = -k * 1.90821492927058770002e-10;      // ln2 = hi (32 bits) + lo: k hi is exact
  const double r = rh + rl;
  double q = 1.0 / 20922789888000.0;                                                                      // 1 / 16!
  q = fma(q, r, 1.0 / 1307674368000.0); q = fma(q, r, 1.0 / 87178291200.0); q = fma(q, r, 1.0 / 6227020800.0); q = fma(q, r, 1.0 / 479001600.0);
  q = fma(q, r, 1.0 / 39916800.0); q = fma(q, r, 1.0 / 3628800.0); q = fma(q, r, 1.0 / 362880.0); q = fma(q, r, 1.0 / 40320.0);
  q = fma(q, r, 1.0 / 5040.0); q = fma(q, r, 1.0 / 720.0); q = fma(q, r, 1.0 / 120.0); q = fma(q, r, 1.0 / 24.0); q = fma(q, r, 1.0 / 6.0);
  const double tail = r * r * r * q;
  const double sh = rh * rh, sl = fma(rh, rh, -sh) + (2.0 * rh * rl + rl * rl);                                     // (rh + rl)^2 = sh + sl
  double t1, e1, t2, e2;
  cork_two_sum(1.0, rh, t1, e1);
  cork_two_sum(t1, 0.5 * sh, t2, e2);
  const double w = ((e1 + e2) + (rl + 0.5 * sl)) + tail;
  return ldexp(t2 + w, (int)k);
}
RRTMG_CORK_HD double cork_pow4(double x) {
#pragma clang fp contract(off)
  const double h = x * x, l = fma(x, x, -h);      // x^2 = h + l
  const double a = h * h;
  if (!(fabs(a) < HUGE_VAL)) return a;            // overflow, infinity, NaN
  const double b = fma(h, h, -a);                 // h^2 = a + b
  return a + (b + 2.0 * h * l);
}

// ---- _ck_bracket: searchsorted-left minus one, the index clamp, the fraction clamp ---------------------------------------------------
RRTMG_CORK_HD void cork_bracket(const double *grid, int n, double v, int &i, double &f) {
#pragma clang fp contract(off)
  int below = 0;
  for (int j = 0; j < n; ++j) below += grid[j] < v ? 1 : 0;      // the grid increases: the count is searchsorted's insertion point
  i = below - 1;
  if (i < 0) i = 0;
  else if (i > n - 2) i = n - 2;
  f = (v - grid[i]) / (grid[i + 1] - grid[i]);
  if (f < 0.0) f = 0.0;
  else if (f > 1.0) f = 1.0;
}

// ---- _tp: the four corners of (T, P) at p[0], p[sT], p[sP], p[sT + sP] -------------------------------------------------------------------
template <class K>
RRTMG_CORK_HD double cork_tp(const K *p, long sT, long sP, double fT, double fP) {
#pragma clang fp contract(off)
  const double v00 = (double)p[0], v10 = (double)p[sT], v01 = (double)p[sP], v11 = (double)p[sT + sP];
  return v00 * (1.0 - fT) * (1.0 - fP) + v10 * fT * (1.0 - fP) + v01 * (1.0 - fT) * fP + v11 * fT * fP;
}
// ---- _txx / _ck_txx7 / _ck_txx_cont: the eight corners of (T, P, X) -----------------------------------------------------------------------
template <class K>
RRTMG_CORK_HD double cork_txx(const K *p, long sT, long sP, long sX, double fT, double fP, double fX) {
#pragma clang fp contract(off)
  const double x0 = cork_tp(p, sT, sP, fT, fP);
  const double x1 = cork_tp(p + sX, sT, sP, fT, fP);
  return x0 * (1.0 - fX) + x1 * fX;
}

// ---- one layer of one band: the gas optical depth of every g-point (k summed over the gases from 0.0, the continuum behind it), and
// the bracket of T.  Both spectra call it: the longwave's cork_layer below, the shortwave's passes in rrtmg_cork_sw.h -------------------
template <int NG, class K, class Call>
RRTMG_CORK_HD void cork_gas_depth(const Call &a, long col, int b, int k, double (&acc)[NG], int &iT, double &fT) {
#pragma clang fp contract(off)
  const CorkTableView &tb = a.tab;
  const K *ktab = (const K *)tb.k;
  const long N = a.ncol, o = (long)k * N + col;
  const int ngpt = tb.ngpt;
  const double T = a.t[o];
  const double p = a.pmid[o] * a.pressure_scale;
  int iP, iX = 0, iC = 0;
  double fP, fX = 0.0, fC = 0.0;
  cork_bracket(tb.t_grid, tb.nT, T, iT, fT);
  cork_bracket(tb.p_grid, tb.nP, log(p > 1.0 ? p : 1.0), iP, fP);
  if (tb.nX > 0) {
    const double q = a.gas0[o];
    const double den = q + (1.0 - q) * a.m_h2o;
    double x = q / (den > 1e-30 ? den : 1e-30);
    x = x > tb.x_lo ? x : tb.x_lo;
    x = x < tb.x_hi ? x : tb.x_hi;
    cork_bracket(tb.x_grid, tb.nX, log(x > 1e-30 ? x : 1e-30), iX, fX);
  }
  if (tb.nC > 0) {
    double c = a.gas1[o];
    c = c > tb.c_lo ? c : tb.c_lo;
    c = c < tb.c_hi ? c : tb.c_hi;
    cork_bracket(tb.c_grid, tb.nC, log(c > 1e-30 ? c : 1e-30), iC, fC);
  }
  const double dp = fabs(a.pint[o + N] * a.pressure_scale - a.pint[o] * a.pressure_scale);
  const long nX1 = tb.nX > 0 ? tb.nX : 1, nC1 = tb.nC > 0 ? tb.nC : 1;
  const long sC = ngpt, sX = sC * nC1, sP = sX * nX1, sT = sP * tb.nP, sB = sT * tb.nT, sG = sB * tb.nband;

#pragma unroll
  for (int g = 0; g < NG; ++g) acc[g] = 0.0;
  double amount0 = 0.0;
  for (int ig = 0; ig < tb.ngas; ++ig) {
    double amount;
    if (a.gas_rule == 2) {
      const double scale = cork_gas_scale(a, ig), q = cork_gas(a, ig)[o];
      amount = (scale == 1.0 ? q : q * scale) * dp / a.g;
    }
    else amount = ig == 0 ? 1.0 * dp / a.g : 0.0;
    if (ig == 0) amount0 = amount;
    const K *corner = ktab + ig * sG + b * sB + iT * sT + iP * sP + iX * sX + iC * sC;
#pragma unroll
    for (int g = 0; g < NG; ++g) {
      if (g >= ngpt) continue;
      double kv;
      if (tb.nC > 0) {
        const double c0 = cork_txx(corner + g, sT, sP, sX, fT, fP, fX);
        const double c1 = cork_txx(corner + sC + g, sT, sP, sX, fT, fP, fX);
        const double l0 = log(c0 > 1e-40 ? c0 : 1e-40), l1 = log(c1 > 1e-40 ? c1 : 1e-40);
        kv = cork_exp(l0 * (1.0 - fC) + l1 * fC);
      } else if (tb.nX > 0) {
        kv = cork_txx(corner + g, sT, sP, sX, fT, fP, fX);
      } else {
        kv = cork_tp(corner + g, sT, sP, fT, fP);
      }
      acc[g] += kv * amount;
    }
  }
  if (tb.has_cont) {
    const long cX = 1, cP = tb.nX, cT = cP * tb.nP, cB = cT * tb.nT;
    const double cont = cork_exp(cork_txx(tb.log_cont + b * cB + iT * cT + iP * cP + iX * cX, cT, cP, cX, fT, fP, fX)) * amount0;
#pragma unroll
    for (int g = 0; g < NG; ++g) {
      if (g >= ngpt) continue;
      acc[g] += cont;
    }
  }
}

// ---- one layer of one band: the optical depth and the Planck source of every g-point ---------------------------------------------------
template <int NG, class K>
RRTMG_CORK_HD void cork_layer(const CorkLongwaveCall &a, long col, int b, int k, double (&tau)[NG], double (&src)[NG]) {
#pragma clang fp contract(off)
  const CorkTableView &tb = a.tab;
  const long N = a.ncol, o = (long)k * N + col;
  const int ngpt = tb.ngpt;
  const double T = a.t[o];
  int iT;
  double fT;
  double acc[NG];
  cork_gas_depth<NG, K>(a, col, b, k, acc, iT, fT);
  const double cloud = a.taucld ? a.taucld[o * tb.nband + b] : 0.0;
  const double planck = a.sigma_sb * cork_pow4(T);
  const double *pf = tb.planck + ((long)b * tb.nT + iT) * ngpt;
#pragma unroll
  for (int g = 0; g < NG; ++g) {
    if (g >= ngpt) continue;
    double t = acc[g];
    if (a.taucld) t = t + cloud;
    tau[g] = t;
    src[g] = (pf[g] * (1.0 - fT) + pf[ngpt + g] * fT) * planck;
  }
}

// ---- one (column, band): both sweeps, the per-band outputs -----------------------------------------------------------------------------
template <int NG, class K>
RRTMG_CORK_HD void cork_band_column(const CorkLongwaveCall &a, long col, int b) {
#pragma clang fp contract(off)
  const CorkTableView &tb = a.tab;
  const long N = a.ncol;
  const int nlay = a.nlay, ngpt = tb.ngpt;
  const double D = a.diffusivity;
  double *const ub = a.up_band + (long)b * (nlay + 1) * N + col, *const db = a.dn_band + (long)b * (nlay + 1) * N + col;
  const long ob = (long)b * nlay * N + col;
  double w[NG], up_prev[NG], tau[NG], src[NG];
#pragma unroll
  for (int g = 0; g < NG; ++g) w[g] = g < ngpt ? tb.weights[b * ngpt + g] : 0.0;

  // the surface
  {
    const double Ts = a.tsfc[col];
    int iT;
    double fT;
    cork_bracket(tb.t_grid, tb.nT, Ts, iT, fT);
    const double planck = a.sigma_sb * cork_pow4(Ts), e = a.emis[(long)b * N + col];
    const double *pf = tb.planck + ((long)b * tb.nT + iT) * ngpt;
    double sum = 0.0;
#pragma unroll
    for (int g = 0; g < NG; ++g) {
      if (g >= ngpt) continue;
      up_prev[g] = e * ((pf[g] * (1.0 - fT) + pf[ngpt + g] * fT) * planck);
      sum += w[g] * up_prev[g];
    }
    ub[0] = sum;
  }
  // upwards
  for (int k = 0; k < nlay; ++k) {
    cork_layer<NG, K>(a, col, b, k, tau, src);
    double sum = 0.0, depth = 0.0;
#pragma unroll
    for (int g = 0; g < NG; ++g) {
      if (g >= ngpt) continue;
      const double trans = cork_exp(-D * tau[g]);
      const double up = up_prev[g] * trans + src[g] * (1.0 - trans);
      sum += w[g] * up;
      depth += w[g] * tau[g];
      up_prev[g] = up;
    }
    ub[(long)(k + 1) * N] = sum;
    if (a.tau_band) a.tau_band[ob + (long)k * N] = depth;
    if (a.trans_band) a.trans_band[ob + (long)k * N] = cork_exp(-D * depth);
  }
  // downwards: up_prev now carries the downward fluxes
#pragma unroll
  for (int g = 0; g < NG; ++g) up_prev[g] = 0.0;
  db[(long)nlay * N] = 0.0;
  double net_hi = ub[(long)nlay * N] - 0.0, p_hi = a.pint[(long)nlay * N + col] * a.pressure_scale;
  for (int k = nlay - 1; k >= 0; --k) {
    cork_layer<NG, K>(a, col, b, k, tau, src);
    double sum = 0.0;
#pragma unroll
    for (int g = 0; g < NG; ++g) {
      if (g >= ngpt) continue;
      const double trans = cork_exp(-D * tau[g]);
      const double dn = up_prev[g] * trans + src[g] * (1.0 - trans);
      sum += w[g] * dn;
      up_prev[g] = dn;
    }
    db[(long)k * N] = sum;
    if (a.hr_band) {
      const double net_lo = ub[(long)k * N] - sum, p_lo = a.pint[(long)k * N + col] * a.pressure_scale;
      a.hr_band[ob + (long)k * N] = a.g / a.cpd * (net_hi - net_lo) / (p_hi - p_lo) * 86400.0;
      net_hi = net_lo; p_hi = p_lo;
    }
  }
}

// ---- the band reduction of one (column, level): the broadband fluxes, and the heating of the layer above the level ---------------------
RRTMG_CORK_HD void cork_broadband(const CorkLongwaveCall &a, long col, int k) {
#pragma clang fp contract(off)
  const long N = a.ncol, plane = (long)(a.nlay + 1) * N, o = (long)k * N + col;
  double up = 0.0, dn = 0.0;
  for (int b = 0; b < a.tab.nband; ++b) { up += a.up_band[b * plane + o]; dn += a.dn_band[b * plane + o]; }
  a.up[o] = up; a.dn[o] = dn;
  if (k == a.nlay) return;
  double up_hi = 0.0, dn_hi = 0.0;
  for (int b = 0; b < a.tab.nband; ++b) { up_hi += a.up_band[b * plane + o + N]; dn_hi += a.dn_band[b * plane + o + N]; }
  const double tend = a.g / a.cpd * ((up_hi - dn_hi) - (up - dn)) / (a.pint[o + N] * a.pressure_scale - a.pint[o] * a.pressure_scale);
  a.tend[o] = tend;
  if (a.hr) a.hr[o] = tend * 86400.0;
}

}  // namespace rrtmg
