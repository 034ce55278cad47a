// rrtmg_surface_ice.h -- the reference's snow/ice column for ONE column: SeaIce and LandIce (climt/_components/sea_ice/component.py:
// _sea_ice_columns, land_ice/component.py: _land_ice_columns) with their shared solver (climt/_core/snow_ice_column.py:
// _solve_column_kernel, a Crank-Nicolson heat-diffusion step with the two boundary rows folded into the diagonals) and the Thomas
// sweep (climt/_core/tridiagonal.py: solve_tridiagonal) inlined.  Node 0 is the base and node n-1 the surface; arrays are
// [node][ncol], columns fastest; `nlay` is the number of ice interface levels n >= 3 (the reference indexes kappa[-2]).
//
//   active         kind 0 (sea ice): area_type == 3 && thick > 0 && thick + snow >= eps;  kind 1 (land ice): area_type 0 or 1 and
//                  thick + snow >= eps.  A column that is not active is written with what the reference's shell pre-fills: thickness,
//                  snow, temperature and heights their input bits, tsfc = t[n-1], kind 0 base_flux_out = base, every other
//                  diagnostic +0.0.  A column that would be active and is taller than max_height is left as inactive and flagged
//                  (the reference raises there; the caller decides what to do with the flag)
//   net flux       swd + lwd - swu - lwu - sh - lh, in this order
//   layers         total = thick + snow, dz = total / n, snow_level = int((1 - snow / total) n) - 1; layer i (between nodes i and
//                  i+1) is snow where i > snow_level: rho, c and kappa are two-valued functions of i
//   system         hc = rho c;  mu_j = dt / (((0.5 (hc_j + hc_j+1)) 2) dz dz);  r_j+1 = (0.5 (kappa_j + kappa_j+1)) mu_j;
//                  row i = j+1: sub -(mu_j kappa_j), diagonal 1 + 2 r_i, super -(mu_j kappa_j+1); the right-hand side is
//                  ((1 - 2 r_i) T_i + (mu_j kappa_j) T_i-1) + (mu_j kappa_j+1) T_i+1, formed on the fly from three rolling temperatures
//   boundaries     Dirichlet: diagonal 1, off-diagonal 0, rhs the value;  flux: diagonal -1, off-diagonal 1, rhs ((-flux) dz) / kappa of
//                  the boundary layer.  Base: kind 0 flux -q_ocean, kind 1 Dirichlet at the soil temperature.  Top: Dirichlet at
//                  t_melt where T[n-1] >= t_melt - eps (melting), else the net flux
//   melting        conducted = (((T'[n-1] - T'[n-2]) (kappa[n-2] + kappa[n-3])) 0.5) / dz;  where T[n-1] > t_melt - eps and conducted > net
//                  the column is solved again with a flux top and T[n-1] - 10 eps, and does not melt.  Otherwise energy =
//                  round6((net - conducted) dt), clamped at 0 (flagged); melt = energy / (rho[n-2] lf) eats the snow first, then the ice
//   base           kind 0: q = round6((((T'[1] - T'[0]) (kappa[0] + kappa[1])) 0.5) / dz), thick' = thick + -(q dt / (rho[0] lf)), and a
//                  thick' < 0 is clamped to 0.0 with (((-thick') rho[n-2]) lf) / dt added to q;  kind 1: ground flux
//                  ((T'[0] - T'[1]) kappa[0]) / dz, thick' and snow' clamped at 0.0
//   heights        height'[j] = ((thick' + snow') j) / (n - 1);  albedo: snow where snow' > 0, else ice; melt where melt > 0
//   round6(x)      rint(x 1e6) / 1e6: round-half-even, what np.round does
// Every operation is rounded on its own (contraction off), in the reference's order.  The rule is reproduced, not improved: on a
// thin 3-node column the surface temperature may rise above melting, as in the reference.
//
// Storage: nlay has no upper bound, so a thread keeps NO array of its own; every loop is a `for` bounded by nlay.  The forward
// sweep leaves c' and d' in two [nlay][ncol] work slabs; the two uppermost unknowns follow from d'[n-1], d'[n-2] and c'[n-2] alone,
// so whether the column is solved again is known BEFORE any back substitution: only the sweep that stands is substituted back, and
// it writes t_out directly -- after the last read of t, which allows t_out == t although a reverted melt reads t twice.  The second
// solve repeats the whole forward sweep: the bits of the full re-solve by construction.
//
// Plain C++: tools/surface_ice_check.cpp runs every "thread" of a launch on the CPU; the kernel is in rrtmg_surface_ice.hip.
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>

#ifdef __HIPCC__
#define RRTMG_ICE_HD __host__ __device__ inline
#else
#define RRTMG_ICE_HD inline
#endif

namespace rrtmg {

constexpr int32_t kIceActive = 1, kIceNegativeEnergy = 2, kIceTooTall = 4;   // the bits of `flags`

struct SurfaceIceCall {
  int32_t ncol, nlay, kind;
  const double *t, *height;                    // [nlay][ncol]
  const double *thick, *snow, *base;           // [ncol]; base: kind 0 the ocean flux, kind 1 the soil temperature
  const double *sw_down, *lw_down, *sw_up, *lw_up, *lh, *sh;   // [ncol]
  const int32_t *area_type;                    // [ncol]
  double dt, rho_ice, rho_snow, c_ice, c_snow, k_ice, k_snow, lf, t_melt, eps, max_height, albedo_snow, albedo_ice, albedo_melt;
  double *t_out, *height_out;                  // [nlay][ncol]; each may be its own input
  double *thick_out, *snow_out, *tsfc_out;     // [ncol]; thick_out and snow_out may be their own inputs
  double *base_flux_out;                       // [ncol]; kind 0: may be base
  double *cond_flux, *albedo;                  // [ncol] or nullptr
  int32_t *flags;                              // [ncol] or nullptr
  double *work_c, *work_d;                     // [nlay][ncol] each: c' and d' of the Thomas sweep
};

RRTMG_ICE_HD double ice_round6(double x) {
#pragma clang fp contract(off)
  return rint(x * 1e6) / 1e6;
}

// the two-valued layer properties: layer i is snow where i > snow_level (kept as a double: the truncated value, whatever its size)
struct IceLayers {
  double snow_level, rho_ice, rho_snow, c_ice, c_snow, k_ice, k_snow;
  RRTMG_ICE_HD bool is_snow(int i) const { return (double)i > snow_level; }
  RRTMG_ICE_HD double rho(int i) const { return is_snow(i) ? rho_snow : rho_ice; }
  RRTMG_ICE_HD double kappa(int i) const { return is_snow(i) ? k_snow : k_ice; }
  RRTMG_ICE_HD double hc(int i) const {
#pragma clang fp contract(off)
    return is_snow(i) ? rho_snow * c_snow : rho_ice * c_ice;
  }
};

// ---- the forward sweep of one solve: c' and d' into the work slabs; -> T'[n-1] and T'[n-2] ---------------------------------------
// t_top: what the solve reads as T[n-1];  top_flux / bot_flux: a flux boundary (else Dirichlet) with the value top_val / bot_val
RRTMG_ICE_HD void ice_forward(const SurfaceIceCall &a, long col, const IceLayers &L, double dz, double t_top, bool top_flux, double top_val,
                              bool bot_flux, double bot_val, double &x_top, double &x_below) {
#pragma clang fp contract(off)
  const long N = a.ncol;
  const int n = a.nlay;
  double *const cp = a.work_c + col, *const dp = a.work_d + col;
  // row 0
  const double diag0 = bot_flux ? -1.0 : 1.0, upper0 = bot_flux ? 1.0 : 0.0;
  const double rhs0 = bot_flux ? -bot_val * dz / L.kappa(0) : bot_val;
  double c_prev = upper0 / diag0, d_prev = rhs0 / diag0;
  cp[0] = c_prev; dp[0] = d_prev;
  // rows 1 .. n-2, three rolling temperatures
  double t_lo = a.t[col], t_mid = a.t[N + col];
  for (int i = 1; i <= n - 2; ++i) {
    const double t_hi = i + 1 == n - 1 ? t_top : a.t[(long)(i + 1) * N + col];
    const int j = i - 1;
    const double k_int = 0.5 * (L.kappa(j) + L.kappa(j + 1));
    const double hc_int = 0.5 * (L.hc(j) + L.hc(j + 1));
    const double mu = a.dt / (hc_int * 2.0 * dz * dz);
    const double r = k_int * mu;
    const double lower = -mu * L.kappa(j), upper = -mu * L.kappa(j + 1);
    const double rhs = ((1.0 - 2.0 * r) * t_mid + -lower * t_lo) + -upper * t_hi;
    const double m = (1.0 + 2.0 * r) - lower * c_prev;
    c_prev = upper / m;
    d_prev = (rhs - lower * d_prev) / m;
    cp[(long)i * N] = c_prev; dp[(long)i * N] = d_prev;
    t_lo = t_mid; t_mid = t_hi;
  }
  // row n-1
  const double diag1 = top_flux ? -1.0 : 1.0, lower1 = top_flux ? 1.0 : 0.0;
  const double rhs1 = top_flux ? -top_val * dz / L.kappa(n - 2) : top_val;
  const double m = diag1 - lower1 * c_prev;
  x_top = (rhs1 - lower1 * d_prev) / m;
  dp[(long)(n - 1) * N] = x_top;
  x_below = d_prev - c_prev * x_top;
}

// ---- SeaIce (kind 0) / LandIce (kind 1), one column ------------------------------------------------------------------------------
RRTMG_ICE_HD void surface_ice_column(const SurfaceIceCall &a, long col) {
#pragma clang fp contract(off)
  const long N = a.ncol;
  const int n = a.nlay;
  const bool sea = a.kind == 0;
  const double thick = a.thick[col], snow = a.snow[col], base = a.base[col];
  const int32_t area = a.area_type[col];
  const double total = thick + snow;
  bool active = sea ? (area == 3 && thick > 0.0 && total >= a.eps) : ((area == 0 || area == 1) && total >= a.eps);
  int32_t flags = 0;
  if (active && total > a.max_height) { active = false; flags = kIceTooTall; }

  if (!active) {
    double top = 0.0;
    for (int j = 0; j < n; ++j) {
      const long o = (long)j * N + col;
      top = a.t[o];
      const double h = a.height[o];
      a.t_out[o] = top; a.height_out[o] = h;
    }
    a.thick_out[col] = thick; a.snow_out[col] = snow; a.tsfc_out[col] = top;
    a.base_flux_out[col] = sea ? base : 0.0;
    if (a.cond_flux) a.cond_flux[col] = 0.0;
    if (a.albedo) a.albedo[col] = 0.0;
    if (a.flags) a.flags[col] = flags;
    return;
  }
  flags = kIceActive;

  const double net = a.sw_down[col] + a.lw_down[col] - a.sw_up[col] - a.lw_up[col] - a.sh[col] - a.lh[col];
  const double frac = snow / total;
  const double dz = total / n;
  const IceLayers L{trunc((1.0 - frac) * n) - 1.0, a.rho_ice, a.rho_snow, a.c_ice, a.c_snow, a.k_ice, a.k_snow};
  const double t_top = a.t[(long)(n - 1) * N + col];
  bool melting = t_top >= a.t_melt - a.eps;
  const bool bot_flux = sea;
  const double bot_val = sea ? -base : base;
  const double k_top = L.kappa(n - 2) + L.kappa(n - 3);

  double x_top, x_below;
  ice_forward(a, col, L, dz, t_top, !melting, melting ? a.t_melt : net, bot_flux, bot_val, x_top, x_below);
  double cond = (x_top - x_below) * k_top * 0.5 / dz;
  if (t_top > a.t_melt - a.eps && cond > net) {
    ice_forward(a, col, L, dz, t_top - 10.0 * a.eps, true, net, bot_flux, bot_val, x_top, x_below);
    melting = false;
    cond = (x_top - x_below) * k_top * 0.5 / dz;
  }

  // back substitution of the sweep that stands: t is not read any more
  a.t_out[(long)(n - 1) * N + col] = x_top;
  double x1 = x_top, x0 = x_top;      // after the loop: T'[1], T'[0]
  for (int i = n - 2; i >= 0; --i) {
    const long o = (long)i * N + col;
    const double x = a.work_d[o] - a.work_c[o] * x0;
    a.t_out[o] = x;
    x1 = x0; x0 = x;
  }
  a.tsfc_out[col] = x_top;

  double thick_out = thick, snow_out = snow, base_out;
  if (sea) {
    base_out = ice_round6((x1 - x0) * (L.kappa(0) + L.kappa(1)) * 0.5 / dz);
    const double growth = -(base_out * a.dt / (L.rho(0) * a.lf));
    thick_out = thick + growth;
  } else {
    base_out = (x0 - x1) * L.kappa(0) / dz;
  }

  double melt = 0.0;
  if (melting) {
    double energy = ice_round6((net - cond) * a.dt);
    if (energy < 0.0) { flags |= kIceNegativeEnergy; energy = 0.0; }
    melt = energy / (L.rho(n - 2) * a.lf);
    if (melt > snow) {
      thick_out -= melt - snow;
      snow_out = 0.0;
    } else {
      snow_out = snow - melt;
    }
  }

  if (sea) {
    if (thick_out < 0.0) {
      const double leftover = -thick_out * L.rho(n - 2) * a.lf / a.dt;
      thick_out = 0.0;
      base_out += leftover;
    }
  } else {
    if (thick_out < 0.0) thick_out = 0.0;
    if (snow_out < 0.0) snow_out = 0.0;
  }

  const double total_out = thick_out + snow_out;
  for (int j = 0; j < n; ++j) a.height_out[(long)j * N + col] = total_out * j / (n - 1);
  a.thick_out[col] = thick_out; a.snow_out[col] = snow_out; a.base_flux_out[col] = base_out;
  if (a.cond_flux) a.cond_flux[col] = sea ? cond : 0.0;
  if (a.albedo) a.albedo[col] = melt > 0.0 ? a.albedo_melt : snow_out > 0.0 ? a.albedo_snow : a.albedo_ice;
  if (a.flags) a.flags[col] = flags;
}

}  // namespace rrtmg
