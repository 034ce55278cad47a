// rrtmg_land_surface.h -- the reference's two land-surface components for ONE column: BucketHydrology
// (climt/_components/bucket_hydrology/component.py: array_call) and SecondBEST (climt/_components/second_best/component.py: the body
// of the column loop of array_call) with its five default processes (processes/soil_properties.py, albedo.py, surface_layer.py,
// fluxes.py, subsurface.py: _best_subsurface_step) and the Thomas sweep (climt/_core/tridiagonal.py: solve_tridiagonal) inlined.
// Both read the lowest model level of the atmosphere and the surface level of the radiative fluxes only, so every atmospheric and
// flux array is [ncol]; the soil arrays of SecondBEST are [node][ncol], columns fastest, node 0 the bottom and node n-1 the surface.
//
// Every operation is rounded on its own (contraction off) and stands in the reference's order, so + - * / sqrt give numpy's bits;
// exp, log and pow are the library's of whoever compiles this file.  The comparisons are the reference's: Python's max(a, b) is
// `b > a ? b : a`, numpy's clip is `min(max(x, lo), hi)` with x kept where it is equal; none of them meets a NaN or depends on the
// sign of a zero (the header of include/rrtmg_hip.h has the rule in formulas).  The reference's literals stand here as literals:
// Bolton's 611.2 / 17.67 / 29.65 / 0.622 / 0.378, 56.768 and 41.801, k_soil 2.0, z0 0.01 / 0.001, the z_mid floor 2.0 and the
// land-ice overrides of the soil table; every constant and parameter that Python can set is a scalar of the call.
//
// Storage: nlay has no upper bound, so a thread keeps NO array of its own; every loop is a `for` bounded by nlay.  The forward
// sweep leaves c' and d' in two [nlay][ncol] work slabs and reads t_soil for the last time; the back substitution then reads x_w
// and x_i of a node before it writes the node's three outputs, so each output may be its own input and the call in place gives
// the bits of the call out of place.
//
// Plain C++: tools/land_surface_check.cpp runs every "thread" of a launch on the CPU; the kernels are in rrtmg_land_surface.hip.
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>

#ifdef __HIPCC__
#define RRTMG_LAND_HD __host__ __device__ inline
#else
#define RRTMG_LAND_HD inline
#endif

namespace rrtmg {

constexpr int32_t kLandActive = 1, kLandUnstable = 2, kLandCapped = 4;   // the bits of SecondBEST's `flags`

RRTMG_LAND_HD double land_max(double x, double lo) { return x > lo ? x : lo; }      // numpy's and Python's for finite operands
RRTMG_LAND_HD double land_min(double x, double hi) { return x < hi ? x : hi; }
RRTMG_LAND_HD double land_clip(double x, double lo, double hi) { return land_min(land_max(x, lo), hi); }

// ---- BucketHydrology, one column -------------------------------------------------------------------------------------------------
struct BucketHydrologyCall {
  int32_t ncol, layers, has_drain;
  const double *t_air, *q_air, *u, *v, *p_air, *ts, *q_sfc, *sw_down, *lw_down, *sw_up, *lw_up;
  const double *soil_moisture, *precip_conv, *precip_strat, *density, *thickness, *heat_capacity, *deep_moisture, *deep_temperature;
  double dt, rd, cp, rho_water, lv, bulk_coefficient, beta_parameter, soil_moisture_max, deep_soil_moisture_max, tau_m, deep_ratio, tau_drain, pressure_scale;
  double *ts_out, *soil_moisture_out, *deep_moisture_out, *deep_temperature_out;   // each may be its own input
  double *precip, *lh, *sh, *evaporation, *runoff, *deep_fraction;                // or nullptr
};

RRTMG_LAND_HD void bucket_hydrology_column(const BucketHydrologyCall &a, long col) {
#pragma clang fp contract(off)
  const double north = a.v[col], east = a.u[col], t_air = a.t_air[col], ts = a.ts[col], w = a.soil_moisture[col];
  const double wind = sqrt(north * north + east * east);
  const double rho = a.p_air[col] * a.pressure_scale / (a.rd * t_air);
  const double potential = rho * a.bulk_coefficient * wind * (a.q_sfc[col] - a.q_air[col]);
  const double precip = a.precip_conv[col] + a.precip_strat[col];
  const double threshold = a.beta_parameter * a.soil_moisture_max;
  const double beta = w <= threshold ? w / threshold : 1.0;
  const double mass_flux = beta * potential;
  const double evaporation = mass_flux / a.rho_water;
  const double lh = a.lv * mass_flux;
  const double sh = rho * a.cp * a.bulk_coefficient * wind * (ts - t_air);
  const double net = a.sw_down[col] + a.lw_down[col] - a.sw_up[col] - a.lw_up[col] - sh - lh;
  const double density = a.density[col], dz_s = a.thickness[col], hc = a.heat_capacity[col];
  if (a.layers == 1) {
    const double tendency = (w < a.soil_moisture_max || precip <= evaporation) ? precip - evaporation : 0.0;
    const double capacity = density * dz_s * hc;
    a.ts_out[col] = ts + net / capacity * a.dt;
    a.soil_moisture_out[col] = land_min(w + tendency * a.dt, a.soil_moisture_max);
  } else {
    const double w_d = a.deep_moisture[col], t_d = a.deep_temperature[col];
    const double s_s = a.soil_moisture_max, s_d = a.deep_soil_moisture_max;
    const double exchange = (w / s_s - w_d / s_d) * (0.5 * (s_s + s_d)) / a.tau_m;
    const double drainage = a.has_drain ? w_d / a.tau_drain : 0.0;
    double w_s_new = w + (precip - evaporation - exchange) * a.dt;
    double w_d_new = w_d + (exchange - drainage) * a.dt;
    const double over_s = land_max(w_s_new - s_s, 0.0), over_d = land_max(w_d_new - s_d, 0.0);
    const double runoff = (over_s + over_d) / a.dt;
    w_s_new = land_clip(w_s_new - over_s, 0.0, s_s);
    w_d_new = land_clip(w_d_new - over_d, 0.0, s_d);
    const double dz_d = a.deep_ratio * dz_s;
    const double c_s = density * dz_s * hc, c_d = density * dz_d * hc;
    const double conducted = 2.0 * (ts - t_d) / (0.5 * (dz_s + dz_d));      // k_soil = 2.0
    a.ts_out[col] = ts + (net - conducted) / c_s * a.dt;
    a.deep_temperature_out[col] = t_d + conducted / c_d * a.dt;
    a.soil_moisture_out[col] = w_s_new;
    a.deep_moisture_out[col] = w_d_new;
    if (a.runoff) a.runoff[col] = runoff;
    if (a.deep_fraction) a.deep_fraction[col] = w_d_new / s_d;
  }
  if (a.precip) a.precip[col] = precip;
  if (a.lh) a.lh[col] = lh;
  if (a.sh) a.sh[col] = sh;
  if (a.evaporation) a.evaporation[col] = evaporation;
}

// ---- SecondBEST, one column ------------------------------------------------------------------------------------------------------
struct SecondBestCall {
  int32_t ncol, nlay;
  const double *t_soil, *x_w, *x_i, *height;                                    // [nlay][ncol]
  const double *t_air, *q_air, *u, *v, *p_air, *ps, *ts, *snow, *sw_down, *lw_down, *sw_up, *lw_up;   // [ncol]
  const int32_t *area_type;                                                     // [ncol]
  double dt, rd, g, cp, lv, lf, rho_water, karman, t_freeze, min_wind, kappa_soil, cv_soil, colour, texture, B, K_H0, psi_0, pressure_scale, ps_scale;
  double *t_soil_out, *x_w_out, *x_i_out;                                       // [nlay][ncol]; each may be its own input
  double *ts_out, *snow_out;                                                    // [ncol]; each may be its own input
  double *sh, *lh, *evaporation, *albedo_direct, *albedo_diffuse, *cd_heat, *cd_momentum, *t2m, *q2m, *u10, *v10;   // [ncol] or nullptr
  int32_t *flags;                                                               // [ncol] or nullptr
  double *work_c, *work_d;                                                      // [nlay][ncol] each: c' and d' of the Thomas sweep
};

// the weight of SurfaceLayer.interpolate_to_height: psi is psi_m (wind) or psi_h (scalar)
RRTMG_LAND_HD double land_height_weight(double ln_mid, double ln_tgt, double frac, double psi) {
#pragma clang fp contract(off)
  const double denom = ln_mid - psi;
  return land_min(land_max((ln_tgt - psi * frac) / denom, 0.0), 1.0);
}

RRTMG_LAND_HD void second_best_column(const SecondBestCall &a, long col) {
#pragma clang fp contract(off)
  const long N = a.ncol;
  const int n = a.nlay;
  const int32_t area = a.area_type[col];
  if (area != 0 && area != 1) {      // not land, not land ice: every output is its input, every diagnostic +0.0
    for (int j = 0; j < n; ++j) {
      const long o = (long)j * N + col;
      if (a.t_soil_out != a.t_soil) a.t_soil_out[o] = a.t_soil[o];
      if (a.x_w_out != a.x_w) a.x_w_out[o] = a.x_w[o];
      if (a.x_i_out != a.x_i) a.x_i_out[o] = a.x_i[o];
    }
    if (a.ts_out != a.ts) a.ts_out[col] = a.ts[col];
    if (a.snow_out != a.snow) a.snow_out[col] = a.snow[col];
    if (a.sh) a.sh[col] = 0.0;
    if (a.lh) a.lh[col] = 0.0;
    if (a.evaporation) a.evaporation[col] = 0.0;
    if (a.albedo_direct) a.albedo_direct[col] = 0.0;
    if (a.albedo_diffuse) a.albedo_diffuse[col] = 0.0;
    if (a.cd_heat) a.cd_heat[col] = 0.0;
    if (a.cd_momentum) a.cd_momentum[col] = 0.0;
    if (a.t2m) a.t2m[col] = 0.0;
    if (a.q2m) a.q2m[col] = 0.0;
    if (a.u10) a.u10[col] = 0.0;
    if (a.v10) a.v10[col] = 0.0;
    if (a.flags) a.flags[col] = 0;
    return;
  }
  const bool ice = area == 1;
  int32_t flags = kLandActive;

  // 1, 2: the air and the height of the lowest model level
  const double u = a.u[col], v = a.v[col], t_air = a.t_air[col], q_air = a.q_air[col], ts = a.ts[col];
  const double speed = sqrt(u * u + v * v);
  const double wind = a.min_wind > speed ? a.min_wind : speed;
  const double p = a.p_air[col] * a.pressure_scale, p_surf = a.ps[col] * a.ps_scale;
  const double rho = p / (a.rd * t_air);
  double z_mid = a.rd * t_air / a.g * log(p_surf / p);
  z_mid = 2.0 > z_mid ? 2.0 : z_mid;
  const double z0 = ice ? 0.001 : 0.01;

  // 3: BestSurfaceLayer
  const double U = land_max(wind, 1e-3);
  const double cdn_root = a.karman / (log(z_mid) - log(z0));
  const double c_dn = cdn_root * cdn_root;
  const double zeta = exp(-a.karman / sqrt(c_dn));
  const double ri = -(a.g * z_mid / (ts * U * U)) * (ts - t_air);
  double c_dm, c_dh;
  if (ri < 0.0) {
    flags |= kLandUnstable;
    const double root = sqrt(fabs(ri) / zeta);
    c_dm = c_dn * (1.0 - 8.0 * ri / (1.0 + 56.768 * c_dn * root));
    c_dh = c_dn * (1.0 - 12.0 * ri / (1.0 + 41.801 * c_dn * root));
  } else {
    const double eps = 0.01;
    const double top = 1.0 - 4.0 * eps * ri;
    c_dm = c_dn * (top * top) / (1.0 + 8.0 * (1.0 - eps) * ri);
    const double part = top / (1.0 + (6.0 - 4.0 * eps) * ri);
    c_dh = c_dn * (part * part);
  }

  // the soil table (BestSoilProperties) and 4: the albedo
  const double texture = ice ? 0.07 : a.texture;
  const double porosity = 0.6 - 0.03 * texture;
  const long top_node = (long)(n - 1) * N + col;
  const double w_lu = a.x_w[top_node] / porosity, w_fu = a.x_i[top_node] / porosity;
  const double albedo = ice ? 0.60 + 0.06 * (1.0 - w_lu) : 0.10 + 0.1 * a.colour + 0.06 * (1.0 - w_lu);

  // 5: Bolton
  const double es = 611.2 * exp(17.67 * (ts - 273.15) / (ts - 29.65));
  const double q_sat = 0.622 * es / (p - 0.378 * es);

  // 6: BestSurfaceFluxes
  const double li = a.lv + a.lf;
  const double sh = rho * a.cp * wind * c_dh * (ts - t_air);
  const double c_u = c_dh * wind;
  const double e_p = rho * c_u * (q_sat - q_air);
  const double free_pores = 1.0 - w_fu;
  const double theta = land_clip((w_lu - 0.01) / (1e-6 > free_pores ? 1e-6 : free_pores), 1e-3, 1.0);
  const double k_hd = -4.0 * a.K_H0 * a.B * a.psi_0 * a.rho_water * porosity * (1.0 - w_fu) / (M_PI * a.dt);
  const double e_max = k_hd * pow(theta, 0.5 * a.B + 2.0) - a.K_H0 * pow(theta, 2.0 * a.B + 3.0);
  const double frozen = li > 0.0 ? w_fu * a.lv / li : 0.0;
  const double ratio = fabs(e_p) > 1e-12 ? land_clip(e_max / e_p, 0.0, 1.0) : 0.0;
  const double beta = land_clip(frozen + ratio, 0.0, 1.0);
  const double evaporation = beta * e_p / rho;
  const double lh = a.lv * rho * evaporation;

  // 7: the net surface flux
  const double net = a.sw_down[col] + a.lw_down[col] - a.sw_up[col] - a.lw_up[col] - sh - lh;
  const bool capped = net <= 0.0;
  if (capped) flags |= kLandCapped;

  // 8: _best_subsurface_step.  Forward sweep: lower = upper = -r, diagonal 1 + 2 r, 1 + r in the first and the last row
  const double dz = fabs(a.height[N + col] - a.height[col]);
  const double r = a.kappa_soil * a.dt / (a.cv_soil * dz * dz);
  const double lower = -r, edge = 1.0 + r, inner = 1.0 + 2.0 * r;
  double *const cp = a.work_c + col, *const dp = a.work_d + col;
  double c_prev = lower / edge, d_prev = a.t_soil[col] / edge;
  cp[0] = c_prev; dp[0] = d_prev;
  for (int i = 1; i <= n - 2; ++i) {
    const double m = inner - lower * c_prev;
    c_prev = lower / m;
    d_prev = (a.t_soil[(long)i * N + col] - lower * d_prev) / m;
    cp[(long)i * N] = c_prev; dp[(long)i * N] = d_prev;
  }
  const double rhs_top = a.t_soil[top_node] + net * a.dt / (a.cv_soil * dz);
  double x = (rhs_top - lower * d_prev) / (edge - lower * c_prev);
  // back substitution with the freeze/melt source node by node: t_soil is not read any more
  double t_top = 0.0;
  for (int i = n - 1; i >= 0; --i) {
    const long o = (long)i * N + col;
    if (i < n - 1) x = dp[(long)i * N] - cp[(long)i * N] * x;
    const double x_w = a.x_w[o], x_i = a.x_i[o];
    double gamma = a.cv_soil / a.lf * (a.t_freeze - x) / a.dt;
    const double max_freeze = a.rho_water * x_w / a.dt, max_melt = a.rho_water * x_i / a.dt;
    gamma = land_min(land_max(gamma, -max_melt), max_freeze);
    const double moved = gamma * a.dt / a.rho_water;
    double t_new = x + a.lf * gamma * a.dt / a.cv_soil;
    if (capped) t_new = land_min(t_new, a.t_freeze);
    a.t_soil_out[o] = t_new;
    a.x_w_out[o] = land_max(x_w - moved, 0.0);
    a.x_i_out[o] = land_max(x_i + moved, 0.0);
    if (i == n - 1) t_top = t_new;
  }
  a.ts_out[col] = t_top;
  const double snow = a.snow[col];
  a.snow_out[col] = snow;

  if (a.sh) a.sh[col] = sh;
  if (a.lh) a.lh[col] = lh;
  if (a.evaporation) a.evaporation[col] = evaporation;
  if (a.albedo_direct) a.albedo_direct[col] = albedo;
  if (a.albedo_diffuse) a.albedo_diffuse[col] = albedo;
  if (a.cd_heat) a.cd_heat[col] = c_dh;
  if (a.cd_momentum) a.cd_momentum[col] = c_dm;
  if (a.flags) a.flags[col] = flags;

  // 9: the screen-level diagnostics (SurfaceLayer.interpolate_to_height)
  if (a.t2m || a.q2m || a.u10 || a.v10) {
    const double ln_mid = log(z_mid / z0);
    const double root = sqrt(c_dm);
    if (a.t2m || a.q2m) {
      const double w2 = land_height_weight(ln_mid, log(2.0 / z0), 2.0 / z_mid, ln_mid - a.karman * root / c_dh);
      const double q_eff = beta * q_sat + (1.0 - beta) * q_air;
      if (a.t2m) a.t2m[col] = ts + (t_air - ts) * w2;
      if (a.q2m) a.q2m[col] = q_eff + (q_air - q_eff) * w2;
    }
    if (a.u10 || a.v10) {
      const double speed10 = wind * land_height_weight(ln_mid, log(10.0 / z0), 10.0 / z_mid, ln_mid - a.karman / root);
      const bool moving = speed > 0.0;
      if (a.u10) a.u10[col] = moving ? speed10 * u / speed : 0.0;
      if (a.v10) a.v10[col] = moving ? speed10 * v / speed : 0.0;
    }
  }
}

}  // namespace rrtmg
