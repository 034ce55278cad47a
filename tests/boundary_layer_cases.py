"""The simple boundary layer (rrtmg_hip_boundary_layer, climt_amd.SimpleBoundaryLayer): the numpy statement of the rule and the
cases the tests run.

`statement` is the rule as include/rrtmg_hip.h states it, a plain loop per column on Python floats (`**` is libm's pow,
math.log libm's log), in the SHAPE of the reference: per-column lists for z, rho, theta_v, wind, Rich and diff, the three
diagonals assembled for each of the four profiles and one Thomas solve per profile (tests/golden/
make_boundary_layer_golden.py runs the reference's own kernel; tests/test_boundary_layer.py compares).  The library instead
eliminates once per distinct matrix and keeps none of those lists; that the two agree is what the tests show.  Besides the four
profiles and the five diagnostics it returns, by column, `count`, the branch taken for C (0: Ri_a < 0, 1: Ri_a < Ric, 2: C = 0)
and, for the whole call, the smallest relative margin over every discrete comparison it made: Ri_a against 0 and against Ric,
the unclamped wind against 1, every Rich[i] the search formed against Ric, every z[i < count] against fb h.

Every case has a margin >= MIN_MARGIN = 1e-9 (`case` asserts it): a pow or log that differs from libm's in its last bits moves
these quantities by ~1e-15 relative and cannot flip a decision, so the values agree to rounding.

TOL, from the operation count.  eps = 2^-53 = 1.1e-16; log and pow are good to about 1 ulp = 2 eps on either side.
  * theta_v, rho, wind of an interface: a handful of roundings and one pow whose exponent Rd/Cp = 0.29 does not amplify the
    rounding of its base: <= 10 eps.  z[i]: i + 1 terms of ~6 roundings each with a log of a ratio >= 1.01, whose own relative
    conditioning 1 / log(ratio) <= 100 applies to the ONE rounding of the ratio; all terms positive, so the sum grows no error:
    <= (6 + 100 + nlay) eps per term, ~2e-14 at 61 levels.
  * Ri_a and Rich hold theta_v differences, which cancel.  Rich only decides (the margins).  Where Ri_a <= 0, C is a function of
    z[0] alone.  Where 0 < Ri_a < Ric, C = ... (1 - Ri_a / Ric)^2 depends on theta_v with the factor
    cond = 2 Ri_a / (Ric - Ri_a) * theta_v_s / |theta_v[0] - theta_v_s| (the statement returns it).  The two sides do the same
    IEEE operations on the same operands and differ in pow and log alone, so their theta_v differ by <= 2 ulp = 4 eps each side of
    the difference: C, and with it bulk, beta and K_b, by <= 8 eps cond.  `case` asserts cond <= 500: 4.4e-13, half of TOL, and
    that only on what the surface exchange and the damped K_b contribute.  C and K_b otherwise: <= 20 eps beyond z's own.  diff,
    the off-diagonals: three more divisions.  So every matrix entry is good to ~(nlay + 150) eps <= 3e-14 (+ 8 eps cond).
  * The matrix is a strictly diagonally dominant M-matrix (diag = 1 + the sum of the off-diagonals' magnitudes, plus beta >= 0):
    the Thomas sweep has no pivot growth (all m >= 1, all |c'| < 1), the inverse is non-negative with row sums <= 1, so a
    relative perturbation delta of the entries moves the solution by <= 2 delta max|x| and each of the 2 nlay sweep steps adds
    <= 3 eps max|x|: <= (2 (nlay + 150) + 6 nlay) eps max|x| ~ 9e-14 max|x| at 61 levels, two sides: 2e-13.
  So the figure is stated relative to the column's LARGEST magnitude of the field (the winds cross zero), and 1e-12 holds with a
  factor 5 to spare at 61 levels: TOL = 1e-12, the project's.  sh and lh are differences that cancel: their tolerance is
  absolute, TOL * Cp * bulk * ts and TOL * Lv * bulk * max(qs, q[0]) -- the operands set the scale.  height and the stresses:
  TOL relative to the column's value, resp. to bulk * max|wind profile|."""
import functools
import math

import numpy as np

# sympl's default constants, as SimpleBoundaryLayer asks for them, and the constructor's defaults
CONSTANTS = dict(rd=287.0, cp=1004.64, g=9.80665, lv=2.5e6, karman=0.4, z0=0.0000321, fb=0.1, p0=100000.0, ric=1.0)
CONSTANT_NAMES = ("rd", "cp", "g", "lv", "karman", "z0", "fb", "p0", "ric")
DT = 600.0
MIN_MARGIN = 1.0e-9
TOL = 1.0e-12
CASES = ("heated", "stable_surface", "decoupled", "calm", "no_top", "varied")
MODES = (0, 1, 2)
NLAYS = (2, 3, 30, 61)
NCOLS = (1, 63, 64, 65, 130)
PROFILES = ("t_new", "q_new", "u_new", "v_new")
DIAGNOSTICS = ("stress_north", "stress_east", "height", "sh", "lh")


def _div(a, b):
    """IEEE division: x / 0 is an infinity and 0 / 0 a NaN, not an exception."""
    with np.errstate(divide="ignore", invalid="ignore"):
        return float(np.float64(a) / np.float64(b))


def solve_tridiagonal(lower, diag, upper, rhs):
    n = len(rhs)
    x = [0.0] * n
    c_prime, d_prime = [0.0] * (n - 1), [0.0] * n
    c_prime[0] = upper[0] / diag[0]
    d_prime[0] = rhs[0] / diag[0]
    for i in range(1, n - 1):
        m = diag[i] - lower[i - 1] * c_prime[i - 1]
        c_prime[i] = upper[i] / m
        d_prime[i] = (rhs[i] - lower[i - 1] * d_prime[i - 1]) / m
    m = diag[n - 1] - lower[n - 2] * c_prime[n - 2]
    d_prime[n - 1] = (rhs[n - 1] - lower[n - 2] * d_prime[n - 2]) / m
    x[n - 1] = d_prime[n - 1]
    for i in range(n - 2, -1, -1):
        x[i] = d_prime[i] - c_prime[i] * x[i + 1]
    return x


def statement(t, q, u, v, p, p_int, ps, ts, qs, mode, sh_in=None, lh_in=None, dt=DT, k=CONSTANTS, pressure_scale=1.0, ps_scale=1.0):
    """-> dict: t_new, q_new, u_new, v_new [nlay][ncol]; stress_north, stress_east, height, sh, lh, bulk, ri_a [ncol]; count,
    branch (int [ncol]); hit (bool [ncol][2]: a diffusing interface below fb h, one above); clamped (int [ncol]: interfaces
    whose wind was raised to 1); margin (float).  Level 0 at the surface; p_int [nlay+1][ncol]."""
    Rd, Cp, g, Lv, kk, z0, fb, P0, Ric = (float(k[name]) for name in CONSTANT_NAMES)
    nlay, ncol = t.shape
    n = nlay - 1
    out = {name: np.zeros((nlay, ncol)) for name in PROFILES}
    out.update({name: np.zeros(ncol) for name in DIAGNOSTICS + ("bulk", "ri_a", "beta")})
    out.update(count=np.zeros(ncol, dtype=np.int32), branch=np.zeros(ncol, dtype=np.int32), clamped=np.zeros(ncol, dtype=np.int32),
               hit=np.zeros((ncol, 2), dtype=bool), diff_max=np.zeros(ncol), cond=np.zeros(ncol))
    margin = [np.inf]

    def decide(a, b, scale=None):
        margin[0] = min(margin[0], abs(a - b) / abs(scale if scale is not None else b))

    for col in range(ncol):
        T, Q = [float(x) for x in t[:, col]], [float(x) for x in q[:, col]]
        U, V = [float(x) for x in u[:, col]], [float(x) for x in v[:, col]]
        P = [float(x) * pressure_scale for x in p[:, col]]
        PI = [float(x) * pressure_scale for x in p_int[:, col]]
        Ps, Ts, Qs = float(ps[col]) * ps_scale, float(ts[col]), float(qs[col])
        pi_in = PI[1:-1]
        v_int = [0.5 * (V[i + 1] + V[i]) for i in range(n)]
        u_int = [0.5 * (U[i + 1] + U[i]) for i in range(n)]
        T_int = [0.5 * (T[i + 1] + T[i]) for i in range(n)]
        q_int = [0.5 * (Q[i + 1] + Q[i]) for i in range(n)]
        rho = [pi_in[i] / (Rd * (1.0 + 0.608 * q_int[i]) * T_int[i]) for i in range(n)]
        thv = [T_int[i] * (P0 / pi_in[i]) ** (Rd / Cp) * (1.0 + 0.608 * q_int[i]) for i in range(n)]
        thv_s = Ts * (P0 / Ps) ** (Rd / Cp) * (1.0 + 0.608 * Qs)
        z = [0.0] * n
        z[0] = (Rd * (1.0 + 0.608 * Q[0]) * T[0] / g) * math.log(Ps / pi_in[0])
        for i in range(1, n):
            z[i] = z[i - 1] + (Rd * (1.0 + 0.608 * Q[i]) * T[i] / g) * math.log(pi_in[i - 1] / pi_in[i])
        wind = [math.sqrt(v_int[i] * v_int[i] + u_int[i] * u_int[i]) for i in range(n)]
        for i in range(n):
            decide(wind[i], 1.0)
            if wind[i] < 1.0:
                wind[i] = 1.0
                out["clamped"][col] += 1
        Ri_a = g * z[0] * (thv[0] - thv_s) / (thv_s * wind[0] * wind[0])
        # the comparisons of Ri_a: against 0 on the scale of the two theta_v whose difference it is, against Ric as it stands
        decide(thv[0], thv_s)
        decide(Ri_a, Ric)
        if Ri_a < 0:
            C, branch = kk * kk * math.log(z[0] / z0) ** -2, 0
        elif Ri_a < Ric:
            C, branch = kk * kk * math.log(z[0] / z0) ** -2 * (1.0 - Ri_a / Ric) ** 2, 1
            out["cond"][col] = 2.0 * Ri_a / (Ric - Ri_a) * thv_s / abs(thv[0] - thv_s)      # d ln C / d ln theta_v
        else:
            C, branch = 0.0, 2
        count = 0
        for i in range(n):
            rich = g * z[i] * (thv[i] - thv[0]) / (thv[0] * wind[i] * wind[i])
            decide(rich, Ric)
            if rich > Ric:
                count = i + 1
                break
        h = z[count - 1]
        u_fric = wind[0]
        dp0 = PI[0] - PI[1]
        bulk = rho[0] * C * wind[0]
        beta = g * bulk * dt / dp0
        if mode == 1:
            scalar_exchange, source_T, source_q = beta, beta * Ts, beta * Qs
        elif mode == 2:
            scalar_exchange = 0.0
            source_T = g * dt * float(sh_in[col]) / (Cp * dp0)
            source_q = g * dt * float(lh_in[col]) / (Lv * dp0)
        else:
            scalar_exchange, source_T, source_q = 0.0, 0.0, 0.0
        wind_exchange = 0.0 if mode == 0 else beta

        def k_b(zz):
            base = kk * u_fric * math.sqrt(C) * zz
            if Ri_a <= 0:
                return base
            return _div(base, 1.0 + _div(Ri_a / Ric * math.log(zz / z0), 1.0 - Ri_a / Ric))

        diff = [0.0] * n
        for i in range(count):
            decide(z[i], fb * h)
            if z[i] < fb * h:
                diff[i] = k_b(z[i])
                out["hit"][col, 0] = True
            else:
                diff[i] = k_b(fb * h) * z[i] / (h * fb) * (1.0 - (z[i] - fb * h) / ((1.0 - fb) * h)) ** 2
                out["hit"][col, 1] = True

        def diffuse(profile, surface_exchange, surface_source):
            diag_m, diag_p, diag = [0.0] * nlay, [0.0] * nlay, [0.0] * nlay
            for i in range(nlay):
                if i != 0:
                    diag_m[i] = g * g * rho[i - 1] * rho[i - 1] * diff[i - 1] * dt / (P[i - 1] - P[i]) / (PI[i] - PI[i + 1])
                if i != nlay - 1:
                    diag_p[i] = g * g * rho[i] * rho[i] * diff[i] * dt / (P[i] - P[i + 1]) / (PI[i] - PI[i + 1])
                diag[i] = 1.0 + diag_m[i] + diag_p[i]
            diag[0] = diag[0] + surface_exchange
            rhs = list(profile)
            rhs[0] = rhs[0] + surface_source
            return solve_tridiagonal([-x for x in diag_m[1:]], diag, [-x for x in diag_p[:-1]], rhs)

        T_new, q_new = diffuse(T, scalar_exchange, source_T), diffuse(Q, scalar_exchange, source_q)
        v_new, u_new = diffuse(V, wind_exchange, 0.0), diffuse(U, wind_exchange, 0.0)
        out["t_new"][:, col], out["q_new"][:, col], out["u_new"][:, col], out["v_new"][:, col] = T_new, q_new, u_new, v_new
        out["height"][col] = h
        out["sh"][col] = Cp * bulk * (Ts - T_new[0])
        out["lh"][col] = Lv * bulk * (Qs - q_new[0])
        out["stress_north"][col] = bulk * v_new[0]
        out["stress_east"][col] = bulk * u_new[0]
        out["bulk"][col], out["ri_a"][col], out["beta"][col] = bulk, Ri_a, beta
        out["count"][col], out["branch"][col], out["diff_max"][col] = count, branch, max(abs(d) for d in diff)
    out["margin"] = float(margin[0])
    return out


def pressures(nlay, ncol):
    """-> (p [nlay][ncol], p_int [nlay+1][ncol], ps [ncol]) in Pa.  From 30 levels the sigma^1.5 grid of the dry adjustment's cases
    (lowest interface ~420 m up at 30 levels).  With fewer levels that grid puts the lowest interface kilometres up, where
    nothing couples to the surface (C == 0 throughout): there the domain is shallow instead, layers of 30 hPa from the surface
    up, the lowest interface ~260 m up."""
    ps = 1.0e5 + 37.0 * np.arange(ncol)
    if nlay >= 30:
        sigma = (1.0 - np.arange(nlay + 1) / float(nlay)) ** 1.5
        p_int = 2000.0 + sigma[:, None] * (ps[None, :] - 2000.0)
    else:
        p_int = ps[None, :] - 3000.0 * np.arange(nlay + 1)[:, None]
    return 0.5 * (p_int[:-1] + p_int[1:]), p_int, ps.copy()


def _inputs(name, nlay, ncol):
    p, p_int, ps = pressures(nlay, ncol)
    kappa = CONSTANTS["rd"] / CONSTANTS["cp"]
    colv = np.arange(ncol)[None, :]
    amp = 1.0 + 0.01 * colv                                          # every column its own numbers
    lev = np.arange(nlay)[:, None] * np.ones((1, ncol))
    s = 1.0 - p / p_int[0]                                           # 0 at the surface, ~1 at the top
    theta = 300.0 + 60.0 * s + 0.02 * amp                            # stable throughout: ~ +1 K per 17 hPa
    q = 0.010 * (p / p_int[0]) ** 3 * amp
    u = 5.0 + 12.0 * s * amp
    v = -2.0 + 3.0 * np.sin(0.37 * lev) * amp                        # crosses zero
    t_offset = np.full(ncol, 3.0)                                    # ts - T[0]
    q_offset = np.full(ncol, 4.0e-3)                                 # qs - q[0]
    if name == "heated":
        # a mixed layer of ~500 hPa, faintly unstable, under the stable air: Rich stays below Ric through it, so the top is
        # many interfaces up and more than ten times as high as the lowest interface: K-profile interfaces below and above fb h
        theta = np.where(p > p_int[0] - 50000.0, 300.0 + 0.02 * amp - 0.2 * s, theta + 1.0)
        u = 12.0 + 12.0 * s * amp
    elif name == "stable_surface":
        t_offset[:] = -0.7                                           # a surface a little colder than the air: 0 < Ri_a < Ric
        q_offset[:] = -1.0e-3
        u = 16.0 + 12.0 * s * amp                                    # (strong enough for fluxes of whole W m^-2: the budgets resolve them)
    elif name == "decoupled":
        t_offset[:] = -12.0                                          # much colder, light wind: Ri_a >= Ric
        q_offset[:] = -2.0e-3
        u = 1.5 + 2.0 * s * amp
        v = 0.5 * np.cos(0.37 * lev) * amp
    elif name == "calm":
        # below 1 m/s near the surface and aloft on alternate stretches, above it between
        slow = 1.0 + 0.0005 * colv
        u = (0.2 + 2.5 * np.abs(np.sin(0.45 * (lev + 0.5))) if nlay >= 30 else 0.3 + 0.2 * lev + 2.0 * (lev >= 2)) * slow
        v = 0.1 * np.cos(0.3 * lev) * slow
    elif name == "no_top":
        # neutral to slightly unstable all the way up and a strong wind: no Rich exceeds Ric
        theta = 300.0 - 0.5 * s + 0.02 * amp
        u = 25.0 + 10.0 * s * amp
    elif name == "varied":
        # neighbouring columns take different branches: surface warmer / colder / much colder by column mod 3, the
        # mixed layer's depth and the wind by column
        kind = np.arange(ncol) % 3
        t_offset = np.where(kind == 0, 2.0 + 0.05 * (np.arange(ncol) % 7), np.where(kind == 1, -2.0 - 0.01 * (np.arange(ncol) % 5), -14.0))
        q_offset = np.where(kind == 0, 3.0e-3, -1.5e-3)
        depth = 12000.0 + 5000.0 * (colv % 5)
        theta = np.where(p > p_int[0] - depth, 300.0 + 0.02 * amp + 0.3 * s, theta + 1.0)
        u = np.where(kind[None, :] == 2, 1.2 + 1.0 * s, (15.0 + 1.0 * (colv % 4)) + 12.0 * s * amp)
        v = np.where(kind[None, :] == 2, 0.4 * np.cos(0.37 * lev), v)
    elif name not in CASES:
        raise KeyError(name)
    t = theta * (p / CONSTANTS["p0"]) ** kappa
    ts = t[0] + t_offset
    qs = q[0] + q_offset
    c = dict(t=t, q=q, u=u * np.ones((nlay, ncol)), v=v * np.ones((nlay, ncol)), p=p, p_int=p_int, ps=ps, ts=ts, qs=qs)
    # the prescribed fluxes of mode 2: their own numbers by column, upward and (every fourth, resp. fifth column) downward, at
    # least 15 and 30 W m^-2 strong
    c["sh_in"] = (40.0 + 25.0 * np.cos(0.7 * np.arange(ncol))) * np.where(np.arange(ncol) % 4 == 3, -1.0, 1.0)
    c["lh_in"] = (80.0 + 50.0 * np.sin(0.3 * np.arange(ncol))) * np.where(np.arange(ncol) % 5 == 4, -1.0, 1.0)
    return {k: np.ascontiguousarray(x, dtype=np.float64) for k, x in c.items()}


INPUTS = ("t", "q", "u", "v", "p", "p_int", "ps", "ts", "qs", "sh_in", "lh_in")
# from how many levels a case is required to do what its name says: all of them from 2, but "calm" from 3 -- with one interface
# the clamp cannot be taken at some and not at others -- and, inside `case`, what needs a deep column from 30 ("heated": a top
# above the first interface with K-profile interfaces on both sides of fb h; "varied": tops that differ by column)
ACTS_FROM = dict(heated=2, stable_surface=2, decoupled=2, calm=3, no_top=2, varied=2)


@functools.lru_cache(maxsize=None)
def case(name, nlay, ncol, mode):
    """-> dict(the INPUTS; the statement's outputs).  Shared and read-only."""
    c = _inputs(name, nlay, ncol)
    c.update(statement(*(c[k] for k in INPUTS[:9]), mode, c["sh_in"], c["lh_in"]))
    assert c["margin"] >= MIN_MARGIN, (name, nlay, ncol, c["margin"])
    assert np.abs(c["ts"] - c["t"][0]).min() >= 0.5 and np.abs(c["qs"] - c["q"][0]).min() >= 1e-4
    assert c["cond"].max() <= 500.0, (name, nlay, ncol, c["cond"].max())      # (module docstring: what TOL rests on)
    for k in PROFILES + DIAGNOSTICS:
        assert np.isfinite(c[k]).all(), (name, k)
    if nlay >= ACTS_FROM[name]:
        if name == "heated":
            assert (c["ri_a"] < 0).all() and (c["branch"] == 0).all() and (c["bulk"] > 0).all()
            if nlay >= 30:
                assert (c["count"] >= 2).all() and c["hit"].all(), "both K-profile branches"
        elif name == "stable_surface":
            assert ((c["ri_a"] > 0) & (c["ri_a"] < CONSTANTS["ric"])).all() and (c["branch"] == 1).all() and (c["bulk"] > 0).all()
        elif name == "decoupled":
            assert (c["ri_a"] >= CONSTANTS["ric"]).all() and (c["branch"] == 2).all() and (c["bulk"] == 0).all()
            if mode == 0:
                assert all(same_bits(c[k + "_new"], c[k]) for k in "tquv")
        elif name == "calm":
            assert ((c["clamped"] > 0) & (c["clamped"] < nlay - 1)).all()
        elif name == "no_top":
            assert (c["count"] == 0).all() and same_bits(c["height"], _top_interface_height(c)) and (c["diff_max"] == 0).all() and (c["beta"] > 0).all()
        elif name == "varied" and ncol >= 3:
            assert set(c["branch"][:3]) == {0, 1, 2}
            if nlay >= 30 and ncol >= 63:
                assert len(set(c["count"][:63])) >= 3
    for x in c.values():
        if isinstance(x, np.ndarray):
            x.setflags(write=False)
    return c


def _top_interface_height(c):
    """z[n - 1] of every column by the statement's own hypsometric sum (no_top: h must be exactly this)."""
    Rd, g = CONSTANTS["rd"], CONSTANTS["g"]
    nlay, ncol = c["t"].shape
    h = np.zeros(ncol)
    for col in range(ncol):
        pi_in = [float(x) for x in c["p_int"][1:-1, col]]
        z = (Rd * (1.0 + 0.608 * float(c["q"][0, col])) * float(c["t"][0, col]) / g) * math.log(float(c["ps"][col]) / pi_in[0])
        for i in range(1, nlay - 1):
            z = z + (Rd * (1.0 + 0.608 * float(c["q"][i, col])) * float(c["t"][i, col]) / g) * math.log(pi_in[i - 1] / pi_in[i])
        h[col] = z
    return h


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def deviations(got, c):
    """got: dict with the PROFILES and DIAGNOSTICS (a diagnostic may be absent) -> {name: deviation / tolerance scale}, each to be
    held against TOL: profiles relative to the column's largest magnitude of the field, sh and lh absolute on the scale of
    their operands (module docstring)."""
    k = CONSTANTS
    dev = {}
    for name in PROFILES:
        scale = np.maximum(np.abs(c[name]).max(axis=0), 1e-300)
        dev[name] = float((np.abs(np.asarray(got[name]) - c[name]).max(axis=0) / scale).max())
    tiny = 1e-300
    wind_scale = np.maximum(np.abs(c["u_new"]).max(axis=0), np.abs(c["v_new"]).max(axis=0))
    scales = dict(height=np.abs(c["height"]), stress_north=c["bulk"] * wind_scale, stress_east=c["bulk"] * wind_scale,
                  sh=k["cp"] * c["bulk"] * c["ts"], lh=k["lv"] * c["bulk"] * np.maximum(c["qs"], c["q"][0]))
    for name in DIAGNOSTICS:
        if got.get(name) is not None:
            dev[name] = float((np.abs(np.asarray(got[name]) - c[name]) / np.maximum(scales[name], tiny)).max())
    return dev


def column_integrals(x, p_int):
    """sum(x dp) by column."""
    return (x * (p_int[:-1] - p_int[1:])).sum(axis=0)
