// rrtmg_gray.h -- the reference's gray radiation path and its moisture sink for ONE column: Frierson06LongwaveOpticalDepth and
// GrayLongwaveRadiation (climt/_components/radiation.py: _frierson_tau_kernel_np, _gray_lw_kernel_np and the heating lines of
// array_call) and GridScaleCondensation (climt/_components/grid_scale_condensation.py: _gsc_kernel_np).  Level 0 is the surface;
// interface i lies below layer i at pint[i]; arrays are [k][ncol], columns fastest.
//
//   optical depth  lat_rad = lat (pi / 180);  tau_0 = tau0e + (tau0p - tau0e) pow(sin(lat_rad), 2);  sigma = pint / ps;
//                  tau = tau_0 (1 - (fl sigma + (1 - fl) pow(sigma, 4))): 0 at the surface and tau_0 at the top, as the reference
//                  has it (the depth is measured from the surface upwards; only its differences enter the sweep)
//   gray sweep     up[0] = sigma_sb pow(Ts, 4);  upwards dtau = tau[k] - tau[k-1], trans = exp(-dtau),
//                  up[k] = up[k-1] trans + (sigma_sb pow(T[k-1], 4)) (1 - trans);  dn[nlay] = +0.0;  downwards with the same dtau and
//                  trans of the layer, dn[k] = dn[k+1] trans + (sigma_sb pow(T[k], 4)) (1 - trans).  dtau is not clamped: a depth that
//                  decreases upwards gives trans > 1, as in the reference
//   heating        net = up - dn;  tend[k] = ((g / cpd) (net[k+1] - net[k])) / (pint[k+1] - pint[k])  [K/s];  hr = tend 86400.0
//   condensation   by layer from the surface up: es = 611.2 exp(17.67 (T - 273.15) / (T - 29.65)), eps = rd / rh2o,
//                  q_sat = eps es / (p - (1 - eps) es);  where q > q_sat: dqsat_dT = lv q_sat / (rh2o (T T)),
//                  condensed = (q - q_sat) / (1 + lv / cpd dqsat_dT), q' = q - condensed, T' = T + lv / cpd condensed,
//                  precip += condensed ((pint[k+1] - pint[k]) / (g rhow)) -- with level 0 at the surface that difference is negative
//                  and so is the reference's precipitation_amount: reproduced.  A layer that is not supersaturated keeps its
//                  input bits.  The time step does not enter, as in the reference
// Every operation is rounded on its own (contraction off), in the reference's order.  The rules are reproduced, not improved.
// numpy's `x ** 4` is pow(x, 4.0) and stays one here; `x ** 2` is written x * x (what every compiler makes of pow(x, 2.0)).
//
// The gray sweep is two passes over the column, none of them spread over lanes, and the transmittance is NOT recomputed: the
// upward pass leaves trans of layer k in dn[k] and sigma_sb T^4 of layer k in tend[k] -- outputs that the downward pass of the same
// thread reads just before it overwrites them with dn[k] and the heating of layer k.  With `frierson` the optical depth of each
// interface is formed during the upward pass (one division and one pow per interface) and never stored unless tau_out is given;
// the downward pass needs no depth at all.
// Storage: nlay has no upper bound, so a thread keeps NO array of its own; every loop is bounded by nlay; the 64 lanes of a wave
// touch one run of 512 bytes per access.
//
// Pressures: pint and pmid are read as p * pressure_scale, ps as ps * ps_scale (Pa per resident unit; 1.0 is exact): the heating
// and the saturation formula need Pa.
//
// Plain C++: tools/gray_check.cpp runs every "thread" of a launch on the CPU; the kernels are in rrtmg_gray.hip.
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>

#ifdef __HIPCC__
#define RRTMG_GRAY_HD __host__ __device__ inline
#else
#define RRTMG_GRAY_HD inline
#endif

namespace rrtmg {

struct FriersonCall {
  int32_t ncol, nlay;
  const double *pint;        // [nlay+1][ncol]
  const double *ps, *lat;    // [ncol]
  double tau0e, tau0p, fl, pressure_scale, ps_scale;
  double *tau;               // [nlay+1][ncol]
};

struct GrayLongwaveCall {
  int32_t ncol, nlay, frierson;
  const double *t;           // [nlay][ncol]
  const double *tsfc;        // [ncol]
  const double *pint, *tau;  // [nlay+1][ncol]; tau is read without `frierson` only
  const double *ps, *lat;    // [ncol]; read with `frierson` only
  double tau0e, tau0p, fl, sigma_sb, g, cpd, pressure_scale, ps_scale;
  double *up, *dn;           // [nlay+1][ncol]
  double *tend;              // [nlay][ncol]
  double *hr;                // [nlay][ncol] or nullptr
  double *tau_out;           // [nlay+1][ncol] or nullptr
};

struct GridScaleCondensationCall {
  int32_t ncol, nlay;
  const double *t, *q, *pmid;   // [nlay][ncol]
  const double *pint;           // [nlay+1][ncol]
  double cpd, lv, rd, rh2o, g, rhow, pressure_scale;
  double *t_out, *q_out;        // [nlay][ncol]; each may be its own input
  double *precip;               // [ncol] or nullptr
};

// ---- the optical depth of the column's latitude at the top of the atmosphere -----------------------------------------------------
RRTMG_GRAY_HD double frierson_tau_0(double lat, double tau0e, double tau0p) {
#pragma clang fp contract(off)
  const double lat_rad = lat * (3.141592653589793 / 180.0);
  const double s = sin(lat_rad);
  return tau0e + (tau0p - tau0e) * (s * s);
}

// ---- the optical depth of one interface: pint_k and ps in Pa ---------------------------------------------------------------------
RRTMG_GRAY_HD double frierson_tau(double tau_0, double pint_k, double ps, double fl) {
#pragma clang fp contract(off)
  const double sigma = pint_k / ps;
  return tau_0 * (1.0 - (fl * sigma + (1.0 - fl) * pow(sigma, 4.0)));
}

// ---- Frierson06LongwaveOpticalDepth, one column ----------------------------------------------------------------------------------
RRTMG_GRAY_HD void frierson_column(const FriersonCall &a, long col) {
#pragma clang fp contract(off)
  const long N = a.ncol;
  const double tau_0 = frierson_tau_0(a.lat[col], a.tau0e, a.tau0p);
  const double ps = a.ps[col] * a.ps_scale;
  for (int k = 0; k <= a.nlay; ++k) {
    const long o = (long)k * N + col;
    a.tau[o] = frierson_tau(tau_0, a.pint[o] * a.pressure_scale, ps, a.fl);
  }
}

// ---- GrayLongwaveRadiation, one column -------------------------------------------------------------------------------------------
RRTMG_GRAY_HD void gray_longwave_column(const GrayLongwaveCall &a, long col) {
#pragma clang fp contract(off)
  const long N = a.ncol;
  const int nlay = a.nlay;
  const bool fused = a.frierson == 1;
  const double tau_0 = fused ? frierson_tau_0(a.lat[col], a.tau0e, a.tau0p) : 0.0;
  const double ps = fused ? a.ps[col] * a.ps_scale : 0.0;

  // pass 1: upwards -- the depth of the interface, the upward flux; trans of layer k-1 into dn[k-1], its emission into tend[k-1]
  double tau_lo = fused ? frierson_tau(tau_0, a.pint[col] * a.pressure_scale, ps, a.fl) : a.tau[col];
  if (a.tau_out) a.tau_out[col] = tau_lo;
  double up = a.sigma_sb * pow(a.tsfc[col], 4.0);
  a.up[col] = up;
  for (int k = 1; k <= nlay; ++k) {
    const long o = (long)k * N + col;
    const double tau_hi = fused ? frierson_tau(tau_0, a.pint[o] * a.pressure_scale, ps, a.fl) : a.tau[o];
    if (a.tau_out) a.tau_out[o] = tau_hi;
    const double dtau = tau_hi - tau_lo;
    const double trans = exp(-dtau);
    const double t4 = a.sigma_sb * pow(a.t[o - N], 4.0);
    up = up * trans + t4 * (1.0 - trans);
    a.up[o] = up;
    a.dn[o - N] = trans;
    a.tend[o - N] = t4;
    tau_lo = tau_hi;
  }

  // pass 2: downwards -- the downward flux and the heating of layer k, over what pass 1 left in dn[k] and tend[k]
  double dn = 0.0, p_hi = a.pint[(long)nlay * N + col] * a.pressure_scale;
  a.dn[(long)nlay * N + col] = dn;
  double net_hi = up - dn;
  for (int k = nlay - 1; k >= 0; --k) {
    const long o = (long)k * N + col;
    const double trans = a.dn[o], t4 = a.tend[o];
    dn = dn * trans + t4 * (1.0 - trans);
    a.dn[o] = dn;
    const double net_lo = a.up[o] - dn, p_lo = a.pint[o] * a.pressure_scale;
    const double tend = a.g / a.cpd * (net_hi - net_lo) / (p_hi - p_lo);
    a.tend[o] = tend;
    if (a.hr) a.hr[o] = tend * 86400.0;
    net_hi = net_lo; p_hi = p_lo;
  }
}

// ---- GridScaleCondensation, one column -------------------------------------------------------------------------------------------
RRTMG_GRAY_HD void grid_scale_condensation_column(const GridScaleCondensationCall &a, long col) {
#pragma clang fp contract(off)
  const long N = a.ncol;
  const double sc = a.pressure_scale;
  double precip = 0.0, p_lo = a.pint[col] * sc;
  for (int k = 0; k < a.nlay; ++k) {
    const long o = (long)k * N + col;
    const double t = a.t[o], q = a.q[o], p = a.pmid[o] * sc, p_hi = a.pint[o + N] * sc;
    const double es = 611.2 * exp(17.67 * (t - 273.15) / (t - 29.65));
    const double eps = a.rd / a.rh2o;
    const double q_sat = eps * es / (p - (1.0 - eps) * es);
    double t_new = t, q_new = q;
    if (q > q_sat) {
      const double dqsat_dt = a.lv * q_sat / (a.rh2o * (t * t));
      const double condensed = (q - q_sat) / (1.0 + a.lv / a.cpd * dqsat_dt);
      q_new = q - condensed;
      t_new = t + a.lv / a.cpd * condensed;
      const double mass = (p_hi - p_lo) / (a.g * a.rhow);
      precip += condensed * mass;
    }
    a.t_out[o] = t_new; a.q_out[o] = q_new;
    p_lo = p_hi;
  }
  if (a.precip) a.precip[col] = precip;
}

}  // namespace rrtmg
