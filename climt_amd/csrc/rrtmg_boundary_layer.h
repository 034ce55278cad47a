// rrtmg_boundary_layer.h -- climt's SimpleBoundaryLayer (simple_boundary_layer/component.py: _boundary_layer_kernel, with
// _core/tridiagonal.py) for ONE column: bulk surface exchange, the Richardson-number search for the boundary-layer top, the
// K-profile and the implicit diffusion of T, q, u and v (rrtmg_hip_boundary_layer).  Level 0 is the surface; n = nlay - 1
// interior interfaces, interface i between the layers i and i + 1 at pint[i + 1].
//
//   interface i   x_int = 0.5 * (x[i+1] + x[i]) for T, q, u, v;   rho[i] = pint[i+1] / (Rd (1 + 0.608 q_int) T_int)
//                 theta_v[i] = T_int * pow(P0 / pint[i+1], Rd / Cp) * (1 + 0.608 q_int);   the surface: the same of ts, ps, qs
//                 z[i] = z[i-1] + (Rd (1 + 0.608 q[i]) T[i] / g) * log(pint[i] / pint[i+1]),  the FIRST term with ps for pint[0]
//                 wind[i] = max(sqrt(v_int^2 + u_int^2), 1)
//   surface layer Ri_a = g z[0] (theta_v[0] - theta_v_s) / (theta_v_s wind[0]^2)
//                 C = k^2 pow(log(z[0] / z0), -2)  [Ri_a < 0],  that times pow(1 - Ri_a / Ric, 2)  [Ri_a < Ric],  else 0
//   top           the first i with Rich[i] = g z[i] (theta_v[i] - theta_v[0]) / (theta_v[0] wind[i]^2) > Ric: count = i + 1, h = z[i].
//                 None: count = 0 and h = z[n - 1] (the reference reads z[count - 1] = z[-1]): no layer diffuses, the surface
//                 exchange still acts.  The rule is reproduced, not improved.
//   diffusivity   i < count:  K_b(z[i])  [z[i] < fb h],  else K_b(fb h) * z[i] / (h fb) * pow(1 - (z[i] - fb h) / ((1 - fb) h), 2);
//                 K_b(z) = k wind[0] sqrt(C) z  [Ri_a <= 0],  else that / (1 + Ri_a / Ric * log(z / z0) / (1 - Ri_a / Ric)) -- where C == 0
//                 this is 0 / (1 + inf) = 0 in IEEE arithmetic, which is relied on.  i >= count: 0.
//   matrix        dp[i] = g g rho[i]^2 diff[i] dt / (p[i] - p[i+1]) / (pint[i] - pint[i+1])  (0 at the top layer),
//                 dm[i] = g g rho[i-1]^2 diff[i-1] dt / (p[i-1] - p[i]) / (pint[i] - pint[i+1])  (0 at layer 0),
//                 diag[i] = 1 + dm[i] + dp[i], lower = -dm, upper = -dp;  bulk = rho[0] C wind[0], beta = g bulk dt / (pint[0] - pint[1])
//   flux_mode 0   nothing on diag[0] or rhs[0];   1 ('bulk'): beta on diag[0], beta X_s on rhs[0] (X_s: ts, qs, 0, 0);
//             2   ('external'): g dt F / (Cp | Lv) / dp0 on rhs[0] of T | q, nothing on their diag[0]; the winds keep beta
//   solve         Thomas: c'[0] = upper[0] / diag[0], d'[0] = rhs[0] / diag[0];  m = diag[i] - lower[i-1] c'[i-1], c'[i] = upper[i] / m,
//                 d'[i] = (rhs[i] - lower[i-1] d'[i-1]) / m;  x[i] = d'[i] - c'[i] x[i+1]  -- divisions, never a reciprocal
//   diagnostics   height = h;  stresses bulk * v_new[0], bulk * u_new[0] (in every mode; advisory in mode 0);
//                 sh = Cp bulk (ts - T_new[0]),  lh = Lv bulk (qs - q_new[0])
// Every operation is rounded on its own (contraction off), in the reference's order.
//
// One matrix, one elimination: T and q share a matrix, u and v share one, and the two differ in diag[0] alone (mode 2; in modes 0
// and 1 they are one matrix).  m and c' are formed ONCE per distinct matrix, in the one forward sweep that carries all four
// right-hand sides: same operands in the same order as the reference's four solves, hence the same bits.  d' is kept in the
// output arrays and the back-substitution runs in place.
//
// Three passes over the column, none of them spread over lanes:
//   1  interfaces upwards: z and rho to their slabs; theta_v, wind and Rich are used as they are formed (Rich of the interfaces
//      beyond the first hit is formed and ignored, where the reference stops), so they need no storage
//   2  layers upwards: diff[i] from z[i], the off-diagonals from rho[i], m, c' and the four d'.  c' of the scalar matrix replaces
//      z[i], c' of the wind matrix (mode 2) replaces rho[i]: both are dead once diff[i] and dp[i] are formed
//   3  layers downwards: the back-substitution, then the diagnostics from x[0]
// Storage: nlay has no upper bound, so a thread keeps NO array of its own.  TWO work slabs [nlay-1][ncol], columns fastest (z then
// c' of T/q; rho then c' of u/v), and the four outputs: the 64 lanes of a wave touch one run of 512 bytes per access.  Every loop
// is bounded by nlay.  The inputs T, q, u, v are read in pass 1 and, as right-hand sides, at layer i of pass 2 just before d'[i]
// is written: an output may be exactly its own input.
//
// Pressures: pmid and pint are read as p * pressure_scale, ps as ps * ps_scale (Pa per resident unit; 1.0 is exact): rho and
// g^2 rho^2 dt / dp^2 need Pa, so the rule is not unit-free.
//
// Plain C++: tools/boundary_layer_check.cpp runs every "thread" of a launch on the CPU; the kernel is in rrtmg_boundary_layer.hip.
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>

#ifdef __HIPCC__
#define RRTMG_BOUNDARY_LAYER_HD __host__ __device__ inline
#else
#define RRTMG_BOUNDARY_LAYER_HD inline
#endif

namespace rrtmg {

struct BoundaryLayerCall {
  int32_t ncol, nlay, flux_mode;
  const double *t, *q, *u, *v, *pmid;   // [nlay][ncol]
  const double *pint;                   // [nlay+1][ncol]
  const double *ps, *ts, *qs;           // [ncol]
  const double *sh_in, *lh_in;          // [ncol], read in mode 2 only
  double dt, rd, cp, g, lv, karman, z0, fb, p0, ric, pressure_scale, ps_scale;
  double *t_out, *q_out, *u_out, *v_out;                          // [nlay][ncol]; each may be its own input
  double *stress_north, *stress_east, *height, *sh_out, *lh_out;  // [ncol] or nullptr
  double *work_z, *work_rho;                                      // work, [nlay-1][ncol] each
};

// ---- K_b of the surface layer: ONE statement for the device and the CPU check -------------------------------------------------------
RRTMG_BOUNDARY_LAYER_HD double boundary_layer_kb(const BoundaryLayerCall &a, double ri_a, double u_fric, double C, double z) {
#pragma clang fp contract(off)
  const double base = a.karman * u_fric * sqrt(C) * z;
  if (ri_a <= 0.0) return base;
  return base / (1.0 + ri_a / a.ric * log(z / a.z0) / (1.0 - ri_a / a.ric));
}

RRTMG_BOUNDARY_LAYER_HD double boundary_layer_diff(const BoundaryLayerCall &a, double ri_a, double u_fric, double C, double z, double h) {
#pragma clang fp contract(off)
  if (z < a.fb * h) return boundary_layer_kb(a, ri_a, u_fric, C, z);
  return boundary_layer_kb(a, ri_a, u_fric, C, a.fb * h) * z / (h * a.fb) * pow(1.0 - (z - a.fb * h) / ((1.0 - a.fb) * h), 2.0);
}

// ---- one column ------------------------------------------------------------------------------------------------------------------
RRTMG_BOUNDARY_LAYER_HD void boundary_layer_column(const BoundaryLayerCall &a, long col) {
#pragma clang fp contract(off)
  const long N = a.ncol;
  const int nlay = a.nlay, n = a.nlay - 1;
  const double g = a.g, dt = a.dt, sc = a.pressure_scale;
  const double kappa = a.rd / a.cp;
  const double ps = a.ps[col] * a.ps_scale, ts = a.ts[col], qs = a.qs[col];
  const double thv_s = ts * pow(a.p0 / ps, kappa) * (1.0 + 0.608 * qs);

  // pass 1: the interfaces, upwards
  double T0 = a.t[col], q0 = a.q[col], u0 = a.u[col], v0 = a.v[col];   // layer i; layer i + 1 is read in the loop
  double p_below = ps;                                                  // the first term of z takes ps, not pint[0]
  double z = 0.0, h = 0.0, thv0 = 0.0, wind0 = 0.0, rho0 = 0.0, z_first = 0.0;
  int count = 0;
  for (int i = 0; i < n; ++i) {
    const long o = (long)(i + 1) * N + col;
    const double T1 = a.t[o], q1 = a.q[o], u1 = a.u[o], v1 = a.v[o];
    const double p_here = a.pint[o] * sc;
    const double v_int = 0.5 * (v1 + v0), u_int = 0.5 * (u1 + u0), T_int = 0.5 * (T1 + T0), q_int = 0.5 * (q1 + q0);
    const double rho = p_here / (a.rd * (1.0 + 0.608 * q_int) * T_int);
    const double thv = T_int * pow(a.p0 / p_here, kappa) * (1.0 + 0.608 * q_int);
    const double dz = (a.rd * (1.0 + 0.608 * q0) * T0 / g) * log(p_below / p_here);
    z = i == 0 ? dz : z + dz;
    double wind = sqrt(v_int * v_int + u_int * u_int);
    if (wind < 1.0) wind = 1.0;
    if (i == 0) { thv0 = thv; wind0 = wind; rho0 = rho; z_first = z; }
    const double rich = g * z * (thv - thv0) / (thv0 * wind * wind);
    if (count == 0 && rich > a.ric) { count = i + 1; h = z; }
    a.work_z[o - N] = z;
    a.work_rho[o - N] = rho;
    T0 = T1; q0 = q1; u0 = u1; v0 = v1; p_below = p_here;
  }
  if (count == 0) h = z;      // z[n - 1]: the reference's z[count - 1] with count == 0

  const double ri_a = g * z_first * (thv0 - thv_s) / (thv_s * wind0 * wind0);
  double C;
  if (ri_a < 0.0) C = a.karman * a.karman * pow(log(z_first / a.z0), -2.0);
  else if (ri_a < a.ric) C = a.karman * a.karman * pow(log(z_first / a.z0), -2.0) * pow(1.0 - ri_a / a.ric, 2.0);
  else C = 0.0;

  const double pint0 = a.pint[col] * sc, pint1 = a.pint[N + col] * sc;
  const double dp0 = pint0 - pint1;
  const double bulk = rho0 * C * wind0;
  const double beta = g * bulk * dt / dp0;
  double ex_s = 0.0, src_t = 0.0, src_q = 0.0;
  if (a.flux_mode == 1) {
    ex_s = beta; src_t = beta * ts; src_q = beta * qs;
  } else if (a.flux_mode == 2) {
    src_t = g * dt * a.sh_in[col] / (a.cp * dp0);
    src_q = g * dt * a.lh_in[col] / (a.lv * dp0);
  }
  const double ex_w = a.flux_mode == 0 ? 0.0 : beta;
  const bool two = a.flux_mode == 2;      // the wind matrix differs from the scalar one (in diag[0])

  // pass 2: the layers, upwards -- coefficients, elimination and the four d'
  double e_below = 0.0;                          // g g rho^2 diff dt / (p[i-1] - p[i]) of the interface below layer i
  double c_s = 0.0, c_w = 0.0;                   // c'[i-1] of the two matrices
  double dT = 0.0, dq = 0.0, du = 0.0, dv = 0.0; // d'[i-1]
  double p_lo = pint0, pm = a.pmid[col] * sc;
  for (int i = 0; i < nlay; ++i) {
    const long o = (long)i * N + col;
    const double p_hi = i == 0 ? pint1 : a.pint[o + N] * sc;
    const double dpi = p_lo - p_hi;
    const double dm = i == 0 ? 0.0 : e_below / dpi;
    double dp = 0.0, pm_up = 0.0;
    if (i < n) {
      const double zi = a.work_z[o], rho = a.work_rho[o];
      const double diff = i < count ? boundary_layer_diff(a, ri_a, wind0, C, zi, h) : 0.0;
      pm_up = a.pmid[o + N] * sc;
      e_below = g * g * rho * rho * diff * dt / (pm - pm_up);
      dp = e_below / dpi;
    }
    const double diag = 1.0 + dm + dp;
    const double lower = -dm, upper = -dp;
    double m_s, m_w;
    if (i == 0) {
      m_s = diag + ex_s;
      m_w = two ? diag + ex_w : m_s;
      dT = (a.t[o] + src_t) / m_s;
      dq = (a.q[o] + src_q) / m_s;
      dv = (a.v[o] + 0.0) / m_w;
      du = (a.u[o] + 0.0) / m_w;
    } else {
      m_s = diag - lower * c_s;
      m_w = two ? diag - lower * c_w : m_s;
      dT = (a.t[o] - lower * dT) / m_s;
      dq = (a.q[o] - lower * dq) / m_s;
      dv = (a.v[o] - lower * dv) / m_w;
      du = (a.u[o] - lower * du) / m_w;
    }
    a.t_out[o] = dT; a.q_out[o] = dq; a.v_out[o] = dv; a.u_out[o] = du;
    if (i < n) {
      c_s = upper / m_s;
      a.work_z[o] = c_s;
      if (two) { c_w = upper / m_w; a.work_rho[o] = c_w; }
    }
    p_lo = p_hi; pm = pm_up;
  }

  // pass 3: the back-substitution, in place (x[nlay-1] = d'[nlay-1] is there already)
  double xT = dT, xq = dq, xu = du, xv = dv;
  for (int i = n - 1; i >= 0; --i) {
    const long o = (long)i * N + col;
    const double cs = a.work_z[o], cw = two ? a.work_rho[o] : cs;
    xT = a.t_out[o] - cs * xT; a.t_out[o] = xT;
    xq = a.q_out[o] - cs * xq; a.q_out[o] = xq;
    xv = a.v_out[o] - cw * xv; a.v_out[o] = xv;
    xu = a.u_out[o] - cw * xu; a.u_out[o] = xu;
  }

  if (a.height) a.height[col] = h;
  if (a.stress_north) a.stress_north[col] = bulk * xv;
  if (a.stress_east) a.stress_east[col] = bulk * xu;
  if (a.sh_out) a.sh_out[col] = a.cp * bulk * (ts - xT);
  if (a.lh_out) a.lh_out[col] = a.lv * bulk * (qs - xq);
}

}  // namespace rrtmg
