// rrtmg_dry_adjust.h -- climt's DryConvectiveAdjustment (dry_convection/component.py) for ONE column: the step behind the
// radiation and the slab in a radiative-convective column model (rrtmg_hip_dry_adjustment).  Level 0 is the surface.
//
//   one layer     rd_cp[m]   = (rd (1 - q) + rv q) / (cpd (1 - q) + cvap q)
//                 theta_q[m] = T[m] * pow(pref / p[m], rd_cp[m]) * (1 + q[m] (rv / rd) - q[m])
//   k = nlay-1 .. 0, ONE sweep from the top layer down:
//     scan  m = k .. nlay-1:  sum += theta_q[m];  theta_avg = sum / (m - k + 1)  (a division);  the HIGHEST m > k with
//           theta_avg > theta_q[m] (strictly) is the top of the unstable run
//     mix   k .. top, where there is one:
//           mean_q     = sum(q dp) / (pint[k] - pint[top + 1]),            dp[m] = pint[m] - pint[m + 1]
//           cp_mixed   = cpd (1 - mean_q) + cvap mean_q,   rdcp_mixed = (rd (1 - mean_q) + rv mean_q) / cp_mixed
//           mean_theta = sum(cp_m T dp) / sum(cp_mixed pow(p / pref, rdcp_mixed) dp),      cp_m = cpd (1 - q) + cvap q
//           every layer of the run: q = mean_q, T = mean_theta * pow(p / pref, rdcp_mixed)
// The sums run upwards from k, every operation is rounded on its own (contraction off) and pow has the reference's operands:
// which layers mix is a DISCRETE decision, so another order of summation is another answer, not a rounding difference.  One
// sweep leaves unadjusted what the reference's one sweep leaves: the rule is reproduced, not improved.
//
// theta_q: the reference forms theta_q of ALL layers again for every k.  Here it is formed once for every layer and again only
// for the layers a mixing has just rewritten: the same expression on the same operands, hence the same bits, and O(nlay) pow
// per column instead of O(nlay^2).  (The scan itself stays O(nlay^2) additions.)
//
// Storage: nlay is a run-time value without an upper bound, so a thread keeps NO array of its own.  T and q of the column are
// adjusted in place in t_out / q_out (which may be t / q); theta_q and dp live in a [nlay][ncol] work slab each, columns fastest:
// the lanes of a wave walk their columns in step and every access of the wave is one run of 64 x 8 bytes.  Every loop is
// bounded by nlay; one column is one thread's, start to end -- the scan is not spread over lanes.
//
// Plain C++: tools/dry_adjust_check.cpp runs every "thread" of a launch on the CPU; the kernel is in rrtmg_dry_adjust.hip.
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>

#ifdef __HIPCC__
#define RRTMG_DRY_ADJUST_HD __host__ __device__ inline
#else
#define RRTMG_DRY_ADJUST_HD inline
#endif

namespace rrtmg {

struct DryAdjustCall {
  int32_t ncol, nlay;
  const double *t, *q, *pmid;   // [nlay][ncol]
  const double *pint;           // [nlay+1][ncol]
  double cpd, cvap, rd, rv, pref;
  double *t_out, *q_out;        // [nlay][ncol]; t_out may be t, q_out may be q
  double *theta, *dp;           // work, [nlay][ncol] each
  int32_t *mixed_top;           // [ncol] or nullptr: the highest layer any mixing wrote, -1 where the column was left alone
};

// ---- the rule of one layer: ONE statement for the device and the CPU check -----------------------------------------------------------
RRTMG_DRY_ADJUST_HD double dry_adjust_cp(double cpd, double cvap, double q) {
#pragma clang fp contract(off)
  return cpd * (1.0 - q) + cvap * q;
}
RRTMG_DRY_ADJUST_HD double dry_adjust_rd(double rd, double rv, double q) {
#pragma clang fp contract(off)
  return rd * (1.0 - q) + rv * q;
}
RRTMG_DRY_ADJUST_HD double dry_adjust_theta_q(const DryAdjustCall &a, double eps, double T, double q, double p) {
#pragma clang fp contract(off)
  const double rd_cp = dry_adjust_rd(a.rd, a.rv, q) / dry_adjust_cp(a.cpd, a.cvap, q);
  return T * pow(a.pref / p, rd_cp) * (1.0 + q * eps - q);
}

// ---- one column ------------------------------------------------------------------------------------------------------------------
RRTMG_DRY_ADJUST_HD void dry_adjust_column(const DryAdjustCall &a, long col) {
#pragma clang fp contract(off)
  const long N = a.ncol;
  const int nlay = a.nlay;
  const double eps = a.rv / a.rd;
  for (int m = 0; m < nlay; ++m) {
    const long o = (long)m * N + col;
    const double T = a.t[o], q = a.q[o];
    a.t_out[o] = T;
    a.q_out[o] = q;
    a.dp[o] = a.pint[o] - a.pint[o + N];
    a.theta[o] = dry_adjust_theta_q(a, eps, T, q, a.pmid[o]);
  }
  int mixed_top = -1;
  for (int k = nlay - 1; k >= 0; --k) {
    double sum = 0.0;
    int top = -1;
    for (int m = k; m < nlay; ++m) {
      const double th = a.theta[(long)m * N + col];
      sum += th;
      const double theta_avg = sum / (double)(m - k + 1);
      if (m > k && theta_avg > th) top = m;
    }
    if (top < 0) continue;
    double sum_enthalpy = 0.0, sum_q_dp = 0.0;
    for (int m = k; m <= top; ++m) {
      const long o = (long)m * N + col;
      const double q = a.q_out[o], dp = a.dp[o];
      sum_enthalpy += dry_adjust_cp(a.cpd, a.cvap, q) * a.t_out[o] * dp;
      sum_q_dp += q * dp;
    }
    const double mean_q = sum_q_dp / (a.pint[(long)k * N + col] - a.pint[(long)(top + 1) * N + col]);
    const double cp_mixed = dry_adjust_cp(a.cpd, a.cvap, mean_q);
    const double rdcp_mixed = dry_adjust_rd(a.rd, a.rv, mean_q) / cp_mixed;
    // theta_coeff of the run's layers: kept in the theta slab (these layers' theta_q is formed again below) -- one pow per layer
    double sum_theta_den = 0.0;
    for (int m = k; m <= top; ++m) {
      const long o = (long)m * N + col;
      const double theta_coeff = pow(a.pmid[o] / a.pref, rdcp_mixed);
      a.theta[o] = theta_coeff;
      sum_theta_den += cp_mixed * theta_coeff * a.dp[o];
    }
    const double mean_theta = sum_enthalpy / sum_theta_den;
    for (int m = k; m <= top; ++m) {
      const long o = (long)m * N + col;
      const double T = mean_theta * a.theta[o];
      a.q_out[o] = mean_q;
      a.t_out[o] = T;
      a.theta[o] = dry_adjust_theta_q(a, eps, T, mean_q, a.pmid[o]);
    }
    if (top > mixed_top) mixed_top = top;
  }
  if (a.mixed_top) a.mixed_top[col] = mixed_top;
}

}  // namespace rrtmg
