// rrtmg_simple_physics.h -- climt's SimplePhysics (simple_physics/component.py around simple_physics_custom.f90: simple_physics_func,
// the Reed-Jablonowski package) for ONE column: large-scale condensation, surface fluxes on the lowest layer and the implicit
// boundary-layer mixing of T, q, u and v, time-split in that order (rrtmg_hip_simple_physics).  Level 0 is the surface (the
// reference runs top-down and its binder flips the levels); interface i lies below layer i at pint[i]; pdel[i] = pint[i] - pint[i+1]
// and rpdel[i] = 1 / pdel[i] as the binder forms them.
//
//   constants     epsilo = rair / rh2o, zvir = rh2o / rair - 1, kappa = rair / cpair;  T0 = 273.16, e0 = 610.78, p0 = 1e5, v20 = 20
//   height        za = rair / g * t[0] * (1 + zvir q[0]) * 0.5 * (log(ps) - log(pint[1])), of the state BEFORE any update; ps, not pint[0]
//   surface T     use_ts_ext: ts.  Else test == 1: the moist baroclinic wave's SST of the latitude, else 302.15 K.  The reference hands
//                 `simulate_cyclone` through as `test`, so the cyclone switch selects the WAVE's formula, and the latitude arrives in
//                 degrees and is taken as radians: both reproduced.  pi = 4.*atan(1.) and q0 = 0.021 are SINGLE-precision literals there
//   condensation  (do_lsc) per layer: qsat = epsilo e0 / pmid * exp(-latvap / rh2o * (1 / t - 1 / T0));  where q > qsat:
//                 tmp = 1 / dt * (q - qsat) / (1 + (latvap / cpair) * (epsilo latvap qsat / (rair t t))), else 0;
//                 t += (latvap / cpair * tmp) dt,  q += (-tmp) dt,  precl += tmp pdel / (g rhow), summed from the model TOP downwards
//   surface       (do_surf_flux) layer 0: wind = sqrt(u u + v v);  Cd = cd0 + cd1 wind  [wind < v20],  else cm;
//                 Ke_s = c wind za,  Km_s = Cd wind za (cm wind za at and above v20);  u, v /= 1 + Cd wind dt / za;
//                 rho = pmid / (rair t);  F = c wind (Tsurf - t);  sh = rho cpair F;  t += (F (rho g) / (pint[0] - pint[1])) dt;
//                 qsats = qsurf  [use_qsurf_ext],  else epsilo es / (ps - 0.378 es) with es = (1.0007 + 3.46e-8 ps) 611.21
//                 exp(17.966 (Tsurf - 273) / (247.15 + (Tsurf - 273)))  [Tsurf > 271: water],  (1.0003 + 4.18e-8 ps) 611.15
//                 exp(22.452 (Tsurf - 273) / (272.5 + (Tsurf - 273)))  [else: ice] -- every constant of the two fits the double of its
//                 FLOAT value, as the reference's default-real literals are;  rho again from the UPDATED t;  F = c wind (qsats - q);
//                 lh = latvap rho F;  q += (F (rho g) / (pint[0] - pint[1])) dt.  lh is written as it is (negative over dew) unless
//                 clamp_latent_heat_flux: then lh < 0 ? 0 : lh, which keeps a NaN.  Without do_surf_flux: sh = lh = +0.0
//   mixing        (do_pbl; needs do_surf_flux: Km_s, Ke_s) interface i = 1 .. nlay-1 of the state after the two steps above:
//                 K = K_s  [pint[i] >= pbltop],  else K_s exp(-(d d) / (pblconst pblconst)), d = pbltop - pint[i];
//                 rho = pint[i] / (rair (t[i-1] + t[i]) / 2);  x(r) = r dt g g K rho rho / (pmid[i-1] - pmid[i]), left to right;
//                 CA[i] = x(rpdel[i]) and CC[i-1] = x(rpdel[i-1]) with Ke, CAm, CCm with Km;  CA[0] = CC[nlay-1] = 0
//   elimination   upwards: den = 1 + CA + CC - CA CE[i-1];  CE[i] = CC / den;  CFq[i] = (q[i] + CA CFq[i-1]) / den;
//                 CFt[i] = (pow(p0 / pmid[i], kappa) t[i] + CA CFt[i-1]) / den;  CEm, CFu, CFv the same with CAm, CCm
//   back          downwards: the top layer takes CF (t: CFt pow(pmid / p0, kappa));  x[i] = CE[i] x[i+1] + CF[i];
//                 t[i] = (CE[i] t[i+1] pow(p0 / pmid[i+1], kappa) + CFt[i]) pow(pmid[i] / p0, kappa) -- theta is NOT carried across:
//                 three pow per layer as in the reference, which has other bits than carrying it
// Every operation is rounded on its own (contraction off), in the reference's order.  The rule is reproduced, not improved.
//
// Three passes over the column, none of them spread over lanes:
//   1  layers downwards: condensation, t, q to the outputs (u, v copied), precl summed; then the surface step on layer 0
//   2  layers upwards: the coefficients of the interface above, the elimination; CE and CEm to the two work slabs, the four CF to
//      the OUTPUT arrays.  Layer i needs t[i-1] of the state, which CFt[i-1] has overwritten: rho, K, the pressure difference of the
//      interface below and the four CF[i-1] are carried in registers
//   3  layers downwards: the back-substitution in place
// Storage: nlay has no upper bound, so a thread keeps NO array of its own.  TWO work slabs [nlay][ncol], columns fastest (CE, CEm),
// and the four outputs: the 64 lanes of a wave touch one run of 512 bytes per access.  Every loop is bounded by nlay.  The inputs
// t, q, u, v are read at layer i of pass 1 just before the outputs of layer i are written: an output may be exactly its own input.
//
// Pressures: pmid and pint are read as p * pressure_scale, ps as ps * ps_scale (Pa per resident unit; 1.0 is exact): the saturation
// formulas, the densities and pbltop need Pa, so the rule is not unit-free.
//
// Plain C++: tools/simple_physics_check.cpp runs every "thread" of a launch on the CPU; the kernel is in rrtmg_simple_physics.hip.
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>

#ifdef __HIPCC__
#define RRTMG_SIMPLE_PHYSICS_HD __host__ __device__ inline
#else
#define RRTMG_SIMPLE_PHYSICS_HD inline
#endif

namespace rrtmg {

struct SimplePhysicsCall {
  int32_t ncol, nlay;
  int32_t do_lsc, do_pbl, do_surf_flux, use_ts_ext, use_qsurf_ext, test, clamp_latent_heat_flux;
  const double *t, *q, *u, *v, *pmid;   // [nlay][ncol]
  const double *pint;                   // [nlay+1][ncol]
  const double *ps;                     // [ncol]
  const double *ts, *qsurf, *lat;       // [ncol]; read with use_ts_ext, with use_qsurf_ext, without use_ts_ext and test == 1
  double dt, g, cpair, rair, latvap, rh2o, radius, omega, rhow, pbltop, pblconst, c_heat, cd0, cd1, cm, pressure_scale, ps_scale;
  double *t_out, *q_out, *u_out, *v_out;   // [nlay][ncol]; each may be its own input
  double *precl, *sh_out, *lh_out;         // [ncol] or nullptr
  double *work_ce, *work_cem;              // work, [nlay][ncol] each (read and written with do_pbl only)
};

// ---- the surface temperature the reference makes up where none is handed in ------------------------------------------------------
RRTMG_SIMPLE_PHYSICS_HD double simple_physics_internal_sst(const SimplePhysicsCall &a, long col, double zvir) {
#pragma clang fp contract(off)
  if (a.test != 1) return 302.15;
  const double lat = a.lat[col];
  const double pi = (double)3.14159274f;      // 4.*atan(1.) in single precision
  const double q0 = (double)0.021f;
  const double T00 = 288.0, u0 = 35.0, eta0 = 0.252;
  const double latw = 2.0 * pi / 9.0;
  const double etav = (1.0 - eta0) * 0.5 * pi;
  const double s = sin(lat), c = cos(lat);
  const double s2 = s * s, s4 = s2 * s2, s6 = s2 * s4, c2 = c * c, c3 = c * c2;
  const double y = lat / latw, y2 = y * y, y4 = y2 * y2;
  const double lead = pi * u0 / a.rair * 1.5 * sin(etav) * pow(cos(etav), 0.5);
  const double x = -(2.0 * s6 * (c2 + 1.0 / 3.0)) + 10.0 / 63.0;
  const double w = 8.0 / 5.0 * c3 * (s2 + 2.0 / 3.0) - pi / 4.0;
  return (T00 + lead * (x * u0 * pow(cos(etav), 1.5) + w * a.radius * a.omega * 0.5)) / (1.0 + zvir * q0 * exp(-y4));
}

// ---- saturation specific humidity of the surface: the two fits, their constants the doubles of single-precision literals ---------
RRTMG_SIMPLE_PHYSICS_HD double simple_physics_qsats(double tsurf, double ps, double epsilo) {
#pragma clang fp contract(off)
  const double c273 = (double)273.f, c378 = (double)0.378f;
  double esats;
  if (tsurf > 271.0)
    esats = ((double)1.0007f + (double)3.46e-8f * ps) * (double)611.21f * exp((double)17.966f * (tsurf - c273) / ((double)247.15f + (tsurf - c273)));
  else
    esats = ((double)1.0003f + (double)4.18e-8f * ps) * (double)611.15f * exp((double)22.452f * (tsurf - c273) / ((double)272.5f + (tsurf - c273)));
  return epsilo * esats / (ps - c378 * esats);
}

// ---- one column ------------------------------------------------------------------------------------------------------------------
RRTMG_SIMPLE_PHYSICS_HD void simple_physics_column(const SimplePhysicsCall &a, long col) {
#pragma clang fp contract(off)
  const long N = a.ncol;
  const int nlay = a.nlay;
  const double g = a.g, dt = a.dt, sc = a.pressure_scale, rair = a.rair, cpair = a.cpair, latvap = a.latvap;
  const double epsilo = rair / a.rh2o, zvir = (a.rh2o / rair) - 1.0, kappa = rair / cpair;
  const double T0 = 273.16, e0 = 610.78, p0 = 100000.0, v20 = 20.0;
  const double ps = a.ps[col] * a.ps_scale;
  const double pint0 = a.pint[col] * sc, pint1 = a.pint[N + col] * sc;
  const double za = rair / g * a.t[col] * (1.0 + zvir * a.q[col]) * 0.5 * (log(ps) - log(pint1));

  // pass 1: the layers, downwards -- condensation; the precipitation is summed from the top
  double precl = 0.0;
  double t0 = 0.0, q0 = 0.0, u0 = 0.0, v0 = 0.0, pm0 = 0.0;      // layer 0 as the loop leaves it
  double p_hi = a.pint[(long)nlay * N + col] * sc;
  for (int i = nlay - 1; i >= 0; --i) {
    const long o = (long)i * N + col;
    const double p_lo = i == 0 ? pint0 : a.pint[o] * sc;
    const double pm = a.pmid[o] * sc;
    double t = a.t[o], q = a.q[o];
    if (a.do_lsc == 1) {
      double dtdt = 0.0, dqdt = 0.0;
      const double qsat = epsilo * e0 / pm * exp(-(latvap / a.rh2o * ((1.0 / t) - 1.0 / T0)));
      if (q > qsat) {
        const double tmp = 1.0 / dt * (q - qsat) / (1.0 + (latvap / cpair) * (epsilo * latvap * qsat / (rair * (t * t))));
        dtdt = dtdt + latvap / cpair * tmp;
        dqdt = dqdt - tmp;
        precl = precl + tmp * (p_lo - p_hi) / (g * a.rhow);
      }
      t = t + dtdt * dt;
      q = q + dqdt * dt;
    }
    u0 = a.u[o]; v0 = a.v[o]; t0 = t; q0 = q; pm0 = pm;
    a.t_out[o] = t; a.q_out[o] = q; a.u_out[o] = u0; a.v_out[o] = v0;
    p_hi = p_lo;
  }

  // the surface step on layer 0
  double sh = 0.0, lh = 0.0, km_s = 0.0, ke_s = 0.0;
  if (a.do_surf_flux == 1) {
    const double tsurf = a.use_ts_ext == 1 ? a.ts[col] : simple_physics_internal_sst(a, col, zvir);
    const double wind = sqrt(u0 * u0 + v0 * v0);
    double cd;
    ke_s = a.c_heat * wind * za;
    if (wind < v20) { cd = a.cd0 + a.cd1 * wind; km_s = cd * wind * za; }
    else { cd = a.cm; km_s = a.cm * wind * za; }
    u0 = u0 / (1.0 + cd * wind * dt / za);
    v0 = v0 / (1.0 + cd * wind * dt / za);
    double rho = pm0 / (rair * t0);
    double flux = a.c_heat * wind * (tsurf - t0);
    sh = rho * cpair * flux;
    t0 = t0 + flux * (rho * g) / (pint0 - pint1) * dt;
    const double qsats = a.use_qsurf_ext == 1 ? a.qsurf[col] : simple_physics_qsats(tsurf, ps, epsilo);
    rho = pm0 / (rair * t0);
    flux = a.c_heat * wind * (qsats - q0);
    lh = latvap * rho * flux;
    q0 = q0 + flux * (rho * g) / (pint0 - pint1) * dt;
    a.t_out[col] = t0; a.q_out[col] = q0; a.u_out[col] = u0; a.v_out[col] = v0;
    if (a.clamp_latent_heat_flux) lh = lh < 0.0 ? 0.0 : lh;
  }
  if (a.precl) a.precl[col] = precl;
  if (a.sh_out) a.sh_out[col] = sh;
  if (a.lh_out) a.lh_out[col] = lh;
  if (a.do_pbl != 1) return;

  // pass 2: the layers, upwards -- the interface above layer i, the elimination, the four CF into the outputs
  double t_here = t0, pm_here = pm0, p_lo = pint0;
  double x_rho = 0.0, x_km = 0.0, x_ke = 0.0, x_dpm = 1.0;     // the interface below layer i (none below layer 0)
  double ce = 0.0, cem = 0.0, cfu = 0.0, cfv = 0.0, cft = 0.0, cfq = 0.0;
  for (int i = 0; i < nlay; ++i) {
    const long o = (long)i * N + col;
    const double p_up = i == 0 ? pint1 : a.pint[o + N] * sc;
    const double rpdel = 1. / (p_lo - p_up);
    double ca = 0.0, cam = 0.0, cc = 0.0, ccm = 0.0;
    if (i > 0) {
      cam = rpdel * dt * g * g * x_km * x_rho * x_rho / x_dpm;
      ca = rpdel * dt * g * g * x_ke * x_rho * x_rho / x_dpm;
    }
    double t_up = 0.0, pm_up = 0.0;
    if (i < nlay - 1) {
      t_up = a.t_out[o + N];
      pm_up = a.pmid[o + N] * sc;
      if (p_up >= a.pbltop) { x_km = km_s; x_ke = ke_s; }
      else {
        const double taper = exp(-((a.pbltop - p_up) * (a.pbltop - p_up) / (a.pblconst * a.pblconst)));
        x_km = km_s * taper; x_ke = ke_s * taper;
      }
      x_rho = p_up / (rair * (t_here + t_up) / 2.0);
      x_dpm = pm_here - pm_up;
      ccm = rpdel * dt * g * g * x_km * x_rho * x_rho / x_dpm;
      cc = rpdel * dt * g * g * x_ke * x_rho * x_rho / x_dpm;
    }
    const double den = 1.0 + ca + cc - ca * ce, denm = 1.0 + cam + ccm - cam * cem;
    ce = cc / den;
    cem = ccm / denm;
    cfu = (a.u_out[o] + cam * cfu) / denm;
    cfv = (a.v_out[o] + cam * cfv) / denm;
    cft = (pow(p0 / pm_here, kappa) * t_here + ca * cft) / den;
    cfq = (a.q_out[o] + ca * cfq) / den;
    a.work_ce[o] = ce; a.work_cem[o] = cem;
    a.u_out[o] = cfu; a.v_out[o] = cfv; a.t_out[o] = cft; a.q_out[o] = cfq;
    t_here = t_up; p_lo = p_up;
    if (i < nlay - 1) pm_here = pm_up;
  }

  // pass 3: the back-substitution, downwards and in place; pm_here is pmid of the top layer
  double xu = cfu, xv = cfv, xq = cfq, pm_above = pm_here;
  double xt = cft * pow(pm_here / p0, kappa);
  a.t_out[(long)(nlay - 1) * N + col] = xt;
  for (int i = nlay - 2; i >= 0; --i) {
    const long o = (long)i * N + col;
    const double c_s = a.work_ce[o], c_m = a.work_cem[o], pm = a.pmid[o] * sc;
    xu = c_m * xu + a.u_out[o]; a.u_out[o] = xu;
    xv = c_m * xv + a.v_out[o]; a.v_out[o] = xv;
    xt = (c_s * xt * pow(p0 / pm_above, kappa) + a.t_out[o]) * pow(pm / p0, kappa); a.t_out[o] = xt;
    xq = c_s * xq + a.q_out[o]; a.q_out[o] = xq;
    pm_above = pm;
  }
}

}  // namespace rrtmg
