"""The snow/ice column (rrtmg_hip_surface_ice and the two components on it, SeaIce and LandIce): the numpy statement of both kinds
and the cases the tests run.

The statement is the rule of the reference's climt/_components/sea_ice/component.py (_sea_ice_columns), land_ice/component.py
(_land_ice_columns), climt/_core/snow_ice_column.py (_solve_column_kernel) and climt/_core/tridiagonal.py in numpy's own
operations: a loop per column, the assembly of the tridiagonal system on whole numpy arrays as the reference forms it, the Thomas
sweep on numpy float64 scalars.  tests/golden/make_surface_ice_golden.py runs the reference's own array_call and
tests/test_surface_ice.py compares the statement with what it returned.  Node 0 is the base; arrays are [node][column].

Besides the outputs the statement returns what it DECIDED, per column -- `active`, `too_tall`, `melting` (the Dirichlet top of
the first solve), `reverted`, `negative`, `snow_level`, the two rounded integers `i_base` and `i_energy` (rint(x 1e6)), `eats_ice`
(melt > snow), `clamped` (thickness < 0) -- and `margin` [ncol]: the smallest distance of the column from any decision of the rule,

  * a comparison a < b:  |a - b| / scale, scale the largest magnitude among the operands a and b were formed from BEFORE any
    cancellation (a conducted flux is a difference of two temperatures of 273 K times kappa / dz: its scale is 273 kappa / dz),
  * a rounding rint(y), y = x 1e6:  the distance of y from the nearest half-integer, over the same kind of scale of y,
  * the truncation int(z), z = (1 - frac) n:  the distance of z from the nearest integer, over n,
  * an exact 0.0 operand (no ice at all) decides exactly and takes no part, and so does a surface temperature that has the very
    bits of t_melt - eps (the only way to a negative melt energy: above it the column is solved again); an area-type code
    decides exactly.

Every case keeps margin >= MIN_MARGIN = 1e-13 in every column (`ice_case` asserts it).  Why 1e-13: with contraction off and
correctly rounded + - * / the device computes the statement's bits, so the margin is there for the maker's +-1 ulp runs and for a
libm-free rule it has to cover only the growth of rounding errors: about 10 roundings per node and at most 30 nodes, which in a
diagonally dominant sweep add up at worst linearly -- 300 ulps of the operands' scale, 7e-14.  The melting cases use a short time
step and the melts_away cases a very large net flux because of this: the melt energy in units of 1e-6 J m^-2 is otherwise so large
a number that no double lies a robust distance from a half-integer.

Tolerances are not chosen here.  tests/golden/sea_ice_<case>.npz and land_ice_<case>.npz carry `tol_<field>`, measured by the
maker from the reference itself (its docstring has the rule); `tolerances` reads them and `deviations` states a result on their
scale: relative to the column's largest magnitude of the field, absolute where that is zero."""
import functools
import os

import numpy as np

from gray_cases import deviations, same_bits, within  # noqa: F401  (the project's one scale of deviations)

# the constants as climt_amd/_sympl_compat.py has them (the order of _lib.SURFACE_ICE_CONSTANTS up to t_melt)
CONSTANTS = dict(rho_ice=916.7, rho_snow=100.0, c_ice=2108.0, c_snow=2108.0, k_ice=2.22, k_snow=0.2, lf=333550.0, t_melt=273.0)
EPS, MAX_HEIGHT = 1e-5, 10.0
ALBEDO = {0: dict(albedo_snow=0.8, albedo_ice=0.5, albedo_melt=0.2), 1: dict(albedo_snow=0.8, albedo_ice=0.6, albedo_melt=0.2)}
MIN_MARGIN = 1.0e-13
NLAYS = (3, 10, 30)
NCOLS = (1, 64, 65, 130)
KINDS = {"sea_ice": 0, "land_ice": 1}
COMMON_CASES = ("cold", "melting", "melt_reverts", "melt_through_snow", "melts_away", "snow_free", "deep_snow", "negative_energy", "mixed_types")
CASES = {0: COMMON_CASES + ("basal_growth", "basal_melt"), 1: COMMON_CASES + ("warm_soil", "cold_soil")}
FLUXES = ("sw_down", "lw_down", "sw_up", "lw_up", "lh", "sh")
INPUTS = ("t", "height", "thick", "snow", "base") + FLUXES + ("area_type",)
FIELDS = ("t_out", "height_out", "thick_out", "snow_out", "tsfc_out", "base_flux_out", "cond_flux", "albedo")
DECISIONS = ("active", "too_tall", "melting", "reverted", "negative", "snow_level", "i_base", "i_energy", "eats_ice", "clamped")
FLAG_ACTIVE, FLAG_NEGATIVE_ENERGY, FLAG_TOO_TALL = 1, 2, 4
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def constants(kind, **over):
    """The scalars of a call as Context.surface_ice takes them."""
    return dict(CONSTANTS, eps=EPS, max_height=MAX_HEIGHT, **dict(ALBEDO[kind], **over))


# ---- the rule -------------------------------------------------------------------------------------------------------------------------
def _round6(x):
    return np.round(x * 1e6) / 1e6


def _thomas(lower, diag, upper, rhs):
    n = rhs.shape[0]
    x, c_prime, d_prime = np.zeros(n), np.zeros(n - 1), np.zeros(n)
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


def _solve(rho, c, kappa, temperature, dt, dz, top_flux, top_val, bot_flux, bot_val):
    n = temperature.shape[0]
    k_interface = 0.5 * (kappa[:-1] + kappa[1:])
    heat_capacity = rho * c
    heat_capacity_int = 0.5 * (heat_capacity[:-1] + heat_capacity[1:])
    mu_inv_int = dt / (heat_capacity_int * 2.0 * dz * dz)
    r, a_sub, a_sup = np.zeros(n), np.zeros(n), np.zeros(n)
    r[1:-1] = k_interface * mu_inv_int
    dp, dm = 1.0 + 2.0 * r, 1.0 - 2.0 * r
    a_sub[:-2] = -mu_inv_int * kappa[:-1]
    a_sup[2:] = -mu_inv_int * kappa[1:]
    rhs = dm * temperature
    rhs[1:] = rhs[1:] + (-a_sub[:-1]) * temperature[:-1]
    rhs[:-1] = rhs[:-1] + (-a_sup[1:]) * temperature[1:]
    if top_flux:
        dp[-1], a_sub[-2], rhs[-1] = -1.0, 1.0, -top_val * dz / kappa[-1]
    else:
        dp[-1], a_sub[-2], rhs[-1] = 1.0, 0.0, top_val
    if bot_flux:
        dp[0], a_sup[1], rhs[0] = -1.0, 1.0, -bot_val * dz / kappa[0]
    else:
        dp[0], a_sup[1], rhs[0] = 1.0, 0.0, bot_val
    return _thomas(a_sub[:-1], dp, a_sup[1:], rhs)


def _half_distance(y):
    return abs(abs(y - np.floor(y)) - 0.5)


def ice_statement(kind, t, height, thick, snow, base, sw_down, lw_down, sw_up, lw_up, lh, sh, area_type, dt, k=None):
    """-> dict: the FIELDS (cond_flux is +0.0 for kind 1), flags, the DECISIONS and margin [ncol]."""
    k = constants(kind) if k is None else k
    rho_ice, rho_snow, c_ice, c_snow, k_ice, k_snow, lf, t_melt = (float(k[n]) for n in ("rho_ice", "rho_snow", "c_ice", "c_snow", "k_ice", "k_snow", "lf", "t_melt"))
    eps, max_height = float(k["eps"]), float(k["max_height"])
    n, ncol = t.shape
    sea = kind == 0
    out = dict(t_out=t.copy(), height_out=height.copy(), thick_out=thick.copy(), snow_out=snow.copy(), tsfc_out=t[-1].copy(),
               base_flux_out=base.copy() if sea else np.zeros(ncol), cond_flux=np.zeros(ncol), albedo=np.zeros(ncol), flags=np.zeros(ncol, dtype=np.int32))
    dec = {d: np.zeros(ncol, dtype=np.int64) for d in DECISIONS}
    dec["snow_level"][:] = -9
    margin = np.full(ncol, np.inf)
    net_flux = sw_down + lw_down - sw_up - lw_up - sh - lh

    def decide(col, a, b, scale):
        margin[col] = min(margin[col], abs(a - b) / scale)

    for col in range(ncol):
        total = thick[col] + snow[col]
        mine = area_type[col] == 3 if sea else area_type[col] in (0, 1)
        if not mine:
            continue
        if sea and thick[col] != 0.0:
            decide(col, thick[col], 0.0, max(abs(thick[col]), abs(snow[col])))
        if sea and not thick[col] > 0.0:
            continue
        if total != 0.0 or thick[col] != 0.0:
            decide(col, total, eps, max(abs(thick[col]), abs(snow[col]), eps))
        if not total >= eps:
            continue
        decide(col, total, max_height, max_height)
        if total > max_height:
            dec["too_tall"][col] = 1
            out["flags"][col] = FLAG_TOO_TALL
            continue
        dec["active"][col] = 1
        flags = FLAG_ACTIVE
        net = net_flux[col]
        net_scale = max(abs(x[col]) for x in (sw_down, lw_down, sw_up, lw_up, lh, sh))
        frac = snow[col] / total
        temp = t[:, col].copy()
        dz = total / n
        z = (1.0 - frac) * n
        snow_level = int(z) - 1
        if snow[col] != 0.0 and thick[col] != 0.0:      # (frac is exactly 0 or 1 otherwise)
            margin[col] = min(margin[col], abs(z - np.round(z)) / n)
        dec["snow_level"][col] = snow_level
        layer = np.arange(n - 1) > snow_level
        rho, c, kappa = np.where(layer, rho_snow, rho_ice), np.where(layer, c_snow, c_ice), np.where(layer, k_snow, k_ice)
        check_melting = temp[-1] >= t_melt - eps
        if temp[-1] != t_melt - eps:      # (the same bits decide exactly: the only way to a negative melt energy)
            decide(col, temp[-1], t_melt - eps, t_melt)
        dec["melting"][col] = int(check_melting)
        bot_flux, bot_val = (True, -base[col]) if sea else (False, base[col])
        new = _solve(rho, c, kappa, temp, dt, dz, not check_melting, net if not check_melting else t_melt, bot_flux, bot_val)
        k_top = (kappa[-1] + kappa[-2]) * 0.5 / dz
        cond = (new[-1] - new[-2]) * (kappa[-1] + kappa[-2]) * 0.5 / dz
        if temp[-1] > t_melt - eps:
            decide(col, cond, net, max(k_top * max(abs(new[-1]), abs(new[-2])), net_scale))
            if cond > net:
                temp[-1] = temp[-1] - 10.0 * eps
                new = _solve(rho, c, kappa, temp, dt, dz, True, net, bot_flux, bot_val)
                check_melting = False
                dec["reverted"][col] = 1
        if sea:
            raw = (new[1] - new[0]) * (kappa[0] + kappa[1]) * 0.5 / dz
            y = raw * 1e6
            margin[col] = min(margin[col], _half_distance(y) / max((kappa[0] + kappa[1]) * 0.5 / dz * max(abs(new[0]), abs(new[1])) * 1e6, 1.0))
            dec["i_base"][col] = int(np.round(y))
            base_out = _round6(raw)
            thick_out = thick[col] + -(base_out * dt / (rho[0] * lf))
        else:
            base_out = (new[0] - new[1]) * kappa[0] / dz
            thick_out = thick[col]
        cond = (new[-1] - new[-2]) * (kappa[-1] + kappa[-2]) * 0.5 / dz
        snow_out, melt = snow[col], 0.0
        if check_melting:
            y = (net - cond) * dt * 1e6
            margin[col] = min(margin[col], _half_distance(y) / max(max(k_top * max(abs(new[-1]), abs(new[-2])), net_scale) * dt * 1e6, 1.0))
            dec["i_energy"][col] = int(np.round(y))
            energy = _round6((net - cond) * dt)
            if energy < 0.0:
                flags |= FLAG_NEGATIVE_ENERGY
                dec["negative"][col] = 1
                energy = 0.0
            melt = energy / (rho[-1] * lf)
            decide(col, melt, snow[col], max(abs(melt), abs(snow[col]), 1e-300))
            if melt > snow[col]:
                dec["eats_ice"][col] = 1
                thick_out -= melt - snow[col]
                snow_out = 0.0
            else:
                snow_out = snow[col] - melt
        if thick_out != 0.0 or thick[col] != 0.0:      # (no ice and none melted: an exact 0.0)
            decide(col, thick_out, 0.0, max(abs(thick[col]), abs(melt), abs(snow[col])))
        if thick_out < 0.0:
            dec["clamped"][col] = 1
            if sea:
                base_out += -thick_out * rho[-1] * lf / dt
            thick_out = 0.0
        if not sea and snow_out < 0.0:
            snow_out = 0.0
        total_out = thick_out + snow_out
        out["t_out"][:, col] = new
        out["tsfc_out"][col] = new[-1]
        for j in range(n):
            out["height_out"][j, col] = total_out * j / (n - 1)
        out["thick_out"][col], out["snow_out"][col], out["base_flux_out"][col] = thick_out, snow_out, base_out
        out["cond_flux"][col] = cond if sea else 0.0
        out["albedo"][col] = k["albedo_melt"] if melt > 0 else k["albedo_snow"] if snow_out > 0 else k["albedo_ice"]
        out["flags"][col] = flags
    out.update(dec)
    out["margin"] = margin
    return out


def decisions_key(s):
    """The decisions of a statement's result as bytes: what a +-1 ulp run of the maker has to share."""
    return b"".join(np.ascontiguousarray(s[d]).tobytes() for d in DECISIONS)


# ---- the cases ------------------------------------------------------------------------------------------------------------------------
def _column(kind, name, n, rng):
    """One column's inputs -> dict(t [n], height [n], thick, snow, base, the six fluxes, area_type, dt) and `aim`: None, or
    (what, delta) -- the net flux is to be set to the conducted flux of the Dirichlet solve plus delta."""
    u = rng.uniform
    sea = kind == 0
    area = 3 if sea else int(rng.randint(0, 2))
    thick, snow = u(0.5, 3.0), u(0.05, 0.4)
    t_base, t_top = (u(268.0, 271.0) if sea else u(255.0, 268.0)), u(240.0, 265.0)
    base = u(-5.0, 5.0) if sea else t_base + u(-2.0, 2.0)
    dt, aim = 1800.0, None
    net = u(-60.0, 60.0)
    if name == "melting":
        t_top, dt, aim = 273.0, 60.0, u(5.0, 50.0)
    elif name == "melt_reverts":
        t_top, dt, aim = 273.0 + (0.0 if rng.randint(0, 2) else u(0.0, 0.5)), 60.0, -u(5.0, 50.0)
    elif name == "melt_through_snow":      # so little snow that every layer is ice: 0.6 to 1.6 um melt in 6 s
        t_top, dt, aim, snow = 273.0, 6.0, u(30.0, 80.0), u(1.0e-7, 5.0e-7)
    elif name == "melts_away":             # 4 to 6 mm, every layer snow: 3 to 4e5 J m^-2 in one second melt up to 12 mm
        t_top, dt, aim = 273.0, 1.0, u(3.0e5, 4.0e5)
        thick, snow = u(5.0e-5, 1.0e-4), u(4.0e-3, 6.0e-3)
    elif name == "snow_free":
        snow = 0.0
        if rng.randint(0, 2):
            t_top, dt, aim = 273.0, 6.0, u(5.0, 50.0)
    elif name == "deep_snow":
        thick, snow = u(0.01, 0.03), u(1.5, 3.0)
        if rng.randint(0, 2):
            t_top, dt, aim = 273.0, 60.0, u(5.0, 50.0)
    elif name == "negative_energy":      # the top at the threshold itself: melting, the conducted flux is not compared, the energy is negative
        t_top, dt, aim = CONSTANTS["t_melt"] - EPS, 60.0, -u(5.0, 50.0)
    elif name == "basal_growth":
        base = -u(5.0, 30.0)
    elif name == "basal_melt":
        base = u(5.0, 30.0)
    elif name == "warm_soil":
        base = u(270.0, 272.9)
    elif name == "cold_soil":
        base = u(230.0, 245.0)
    t = t_base + (t_top - t_base) * np.arange(n) / (n - 1) + np.where((np.arange(n) > 0) & (np.arange(n) < n - 1), u(-0.3, 0.3, n), 0.0)
    t[-1] = t_top
    total = thick + snow
    parts = dict(lw_down=u(150.0, 350.0), sw_up=u(0.0, 80.0), lw_up=u(200.0, 320.0), lh=u(-10.0, 30.0), sh=u(-20.0, 40.0))
    c = dict(t=t, height=total * np.arange(n) / (n - 1) * u(0.9, 1.1), thick=thick, snow=snow, base=base, area_type=area, dt=dt, aim=aim, net=net, **parts)
    return c


def _one(kind, c, net):
    """The statement on one column with the net flux `net` (sw_down closes the sum)."""
    sw_down = net - c["lw_down"] + c["sw_up"] + c["lw_up"] + c["sh"] + c["lh"]
    one = lambda x: np.array([x], dtype=np.float64)
    s = ice_statement(kind, c["t"][:, None].copy(), c["height"][:, None].copy(), one(c["thick"]), one(c["snow"]), one(c["base"]), one(sw_down), one(c["lw_down"]),
                      one(c["sw_up"]), one(c["lw_up"]), one(c["lh"]), one(c["sh"]), np.array([c["area_type"]], dtype=np.int32), c["dt"])
    return sw_down, s


def _settle(kind, c):
    """-> (sw_down, base) of the column such that it keeps the margin: the aimed net flux and, for sea ice, the ocean flux, nudged
    by parts in 1e4 until it does."""
    base = c["base"]
    for attempt in range(400):
        c = dict(c, base=base * (1.0 + 1.0e-4 * attempt) + 1.2345678e-3 * attempt if kind == 0 else base)
        target = c["net"]
        if c["aim"] is not None:      # the Dirichlet solve does not depend on the net flux
            target = float(_one(kind, c, 1.0e9)[1]["cond_flux"][0] if kind == 0 else _land_cond(c)) + c["aim"]
        sw_down, s = _one(kind, c, target * (1.0 + 1.0e-4 * attempt) + 1.3572468e-3 * attempt)
        if s["margin"][0] >= 4.0 * MIN_MARGIN:
            return sw_down, c["base"]
    raise AssertionError("no net flux keeps the margin")


def _land_cond(c):
    """The conducted flux of a land column's Dirichlet solve (kind 1 does not report it)."""
    k = constants(1)
    n = c["t"].shape[0]
    total = c["thick"] + c["snow"]
    if total < EPS:
        return 0.0
    dz = total / n
    layer = np.arange(n - 1) > int((1.0 - c["snow"] / total) * n) - 1
    rho, cc, kappa = np.where(layer, k["rho_snow"], k["rho_ice"]), np.where(layer, k["c_snow"], k["c_ice"]), np.where(layer, k["k_snow"], k["k_ice"])
    new = _solve(rho, cc, kappa, c["t"].copy(), c["dt"], dz, False, k["t_melt"], False, c["base"])
    return (new[-1] - new[-2]) * (kappa[-1] + kappa[-2]) * 0.5 / dz


def _inputs(kind, name, nlay, ncol):
    rng = np.random.RandomState(1000 * sum(map(ord, name)) + 100 * nlay + 7 * ncol + kind)
    cols = []
    for col in range(ncol):
        if name == "mixed_types":
            sub = ("cold", "melting", "melt_reverts")[(col // 4 + col) % 3]
            c = _column(kind, sub, nlay, rng)
            c["area_type"] = col % 4 if ncol > 1 else (3 if kind == 0 else 1)
            if col % 7 == 4:
                c["thick"], c["snow"] = 0.0, (0.0 if col % 2 else 0.2)      # no ice at all
            if col % 7 == 5:
                c["thick"], c["snow"] = 0.3 * EPS, 0.2 * EPS                 # thinner than eps
            if col == (8 if kind == 1 else 7) and ncol > 8:
                c["thick"], c["snow"] = 9.5, 0.9                             # taller than the maximum: area type 0 (land) or 3 (sea ice)
        else:
            c = _column(kind, name, nlay, rng)
        c["dt"] = {"mixed_types": 60.0}.get(name, c["dt"])
        cols.append(c)
    dts = {c["dt"] for c in cols}
    if len(dts) > 1:      # one time step per call: the shortest any column asked for
        for c in cols:
            c["dt"] = min(dts)
    for c in cols:
        c["sw_down"], c["base"] = _settle(kind, c)
    two = lambda key: np.ascontiguousarray(np.stack([c[key] for c in cols], axis=1), dtype=np.float64)
    one = lambda key: np.array([c[key] for c in cols], dtype=np.float64)
    out = dict(t=two("t"), height=two("height"), area_type=np.array([c["area_type"] for c in cols], dtype=np.int32), dt=float(cols[0]["dt"]))
    out.update({key: one(key) for key in ("thick", "snow", "base") + FLUXES})
    return out


def check_ice_case(kind, name, c):
    nlay, ncol = c["t"].shape
    assert (c["margin"] >= MIN_MARGIN).all(), (kind, name, nlay, ncol, c["margin"].min())
    a, on = c["active"] == 1, lambda key: c[key][c["active"] == 1]
    for key in FIELDS:
        assert np.isfinite(c[key]).all(), (name, key)
    assert same_bits(c["tsfc_out"], c["t_out"][-1])
    for key in ("t", "height", "thick", "snow"):      # a column that is not active keeps its bits and gets +0.0 diagnostics
        assert same_bits(c[key + "_out"][..., ~a], c[key][..., ~a])
    zeros = np.zeros(int((~a).sum()))
    assert same_bits(c["albedo"][~a], zeros) and same_bits(c["cond_flux"][~a], zeros) and same_bits(c["base_flux_out"][~a], c["base"][~a] if kind == 0 else zeros)
    if name != "mixed_types":
        assert a.all()
    if name in ("cold", "basal_growth", "basal_melt", "warm_soil", "cold_soil"):
        assert not c["melting"].any() and not c["reverted"].any()
    if name in ("melting", "melt_through_snow", "melts_away"):
        assert c["melting"].all() and not c["reverted"].any() and not c["negative"].any() and (c["i_energy"] > 0).all()
        assert same_bits(c["albedo"], np.full(ncol, ALBEDO[kind]["albedo_melt"]))
    if name == "melting":
        assert not c["eats_ice"].any() and (c["snow_out"] > 0).all() and (c["snow_out"] < c["snow"]).all()
    if name == "melt_reverts":
        assert c["melting"].all() and c["reverted"].all()
    if name == "melt_through_snow":
        assert c["eats_ice"].all() and not c["clamped"].any() and same_bits(c["snow_out"], np.zeros(ncol)) and (c["thick_out"] < c["thick"]).all()
    if name == "melts_away":
        assert c["clamped"].all() and same_bits(c["thick_out"], np.zeros(ncol)) and same_bits(c["snow_out"], np.zeros(ncol))
        assert same_bits(c["height_out"], np.zeros((nlay, ncol)))
    if name == "snow_free":
        assert (c["snow_level"] == nlay - 1).all()
    if name == "deep_snow":
        assert (c["snow_level"] == -1).all()
    if name == "negative_energy":
        assert c["melting"].all() and not c["reverted"].any() and c["negative"].all() and ((c["flags"] & FLAG_NEGATIVE_ENERGY) != 0).all()
    if name == "basal_growth":
        assert (c["thick_out"] > c["thick"]).all()
    if name == "basal_melt":
        assert (c["thick_out"] < c["thick"]).all()
    if name == "warm_soil":
        assert (c["base_flux_out"] > 0).all()
    if name == "cold_soil":
        assert (c["base_flux_out"] < 0).all()
    if name == "mixed_types" and ncol >= 64:
        assert set(c["area_type"]) == {0, 1, 2, 3} and c["too_tall"].sum() == 1 and a.any() and (~a).any()
        assert ((c["thick"] == 0.0) & (c["area_type"] == (3 if kind == 0 else 1))).any() and ((c["thick"] + c["snow"] < EPS) & (c["thick"] > 0)).any()


@functools.lru_cache(maxsize=None)
def ice_case(kind, name, nlay, ncol):
    """-> dict(the INPUTS, dt; the statement's outputs, flags, decisions, margin).  Deterministic in (kind, name, nlay, ncol); every
    column differs.  Shared and read-only."""
    c = _inputs(kind, name, nlay, ncol)
    c.update(ice_statement(kind, *(c[k] for k in INPUTS), c["dt"]))
    check_ice_case(kind, name, c)
    for x in c.values():
        if isinstance(x, np.ndarray):
            x.setflags(write=False)
    return c


def fluxes_of(c):
    return {k: c[k] for k in FLUXES}


# ---- what holds in ANY result: exact properties and the energy budget ----------------------------------------------------------------------
def check_exact_properties(kind, name, c, got):
    """What holds to the bit in a result `got` (the FIELDS and flags: the host program's, the kernel's) on the inputs and decisions
    of the case `c`, whatever its deviation from the statement: flags, the surface temperature, the heights, what a column that is
    not active keeps, the albedo (one of three constants), and every exact +0.0 (the sign included)."""
    n, ncol = c["t"].shape
    a = c["active"] == 1
    flags = np.asarray(got["flags"])
    assert ((flags & FLAG_ACTIVE) != 0).tolist() == a.tolist() and (((flags & FLAG_TOO_TALL) != 0) == (c["too_tall"] == 1)).all()
    assert (((flags & FLAG_NEGATIVE_ENERGY) != 0) == (c["negative"] == 1)).all() and (flags & ~7 == 0).all()
    assert same_bits(got["tsfc_out"], got["t_out"][-1])
    total = got["thick_out"] + got["snow_out"]
    for j in range(n):
        assert same_bits(got["height_out"][j][a], (total * j / (n - 1))[a]), j
    for key in ("t", "height", "thick", "snow"):
        assert same_bits(got[key + "_out"][..., ~a], c[key][..., ~a]), key
    zeros = np.zeros(int((~a).sum()))
    assert same_bits(got["albedo"][~a], zeros) and same_bits(got["cond_flux"][~a], zeros)
    assert same_bits(got["base_flux_out"][~a], c["base"][~a] if kind == 0 else zeros)
    assert same_bits(got["albedo"], c["albedo"])
    if kind == 1:
        assert same_bits(got["cond_flux"], np.zeros(ncol))
    gone = a & (c["melting"] == 1) & (c["reverted"] == 0) & (c["eats_ice"] == 1)      # the snow went: an exact +0.0
    assert same_bits(got["snow_out"][gone], np.zeros(int(gone.sum())))
    clamped = c["clamped"] == 1
    assert same_bits(got["thick_out"][clamped], np.zeros(int(clamped.sum())))
    kept = a & ~((c["melting"] == 1) & (c["reverted"] == 0))                           # no melt: the snow keeps its bits
    assert same_bits(got["snow_out"][kept], np.maximum(c["snow"][kept], 0.0) if kind == 1 else c["snow"][kept])
    if name == "melts_away":
        assert a.all() and clamped.all() and same_bits(got["thick_out"], np.zeros(ncol)) and same_bits(got["snow_out"], np.zeros(ncol))
        assert same_bits(got["height_out"], np.zeros((n, ncol)))
        if kind == 0:
            assert (got["base_flux_out"] > c["base_flux_out"] * 0.0).all() and (got["base_flux_out"] > 0).all()      # the leftover goes to the ocean


BUDGET_FACTOR = 16.0      # roundings that can add up in one interior row's residual and its two face fluxes (see energy_budget)


def energy_budget(kind, c, got, k=None):
    """The energy budget that the rule keeps, checked on a result `got` (asserts) -> dict of what was measured.

    What closes.  The interior rows of the Crank-Nicolson step are conservative: with hc_i = 0.5 (hc[i-1] + hc[i]) the heat capacity
    of node i and S = T' + T,
        sum over the interior nodes 1 .. n-2 of hc_i dz (T'_i - T_i)  =  dt (F_top - F_base),
        F_top = kappa[n-2] (S[n-1] - S[n-2]) / (2 dz),   F_base = kappa[0] (S[1] - S[0]) / (2 dz)
    -- the two face fluxes are the means of the old and the new gradient.  This is an identity of the solved system, so only
    rounding is left: each interior row is met to a few ulps of (1 + 4 r_i) |T| (its diagonal and off-diagonals times the
    temperatures), which weighs hc_i dz in the sum; the bound is BUDGET_FACTOR 2^-52 sum hc_i dz (1 + 4 r_i) max|T|, from the
    number format and the row's operation count, not from what the code gives.  `ratio` is the residual over that sum in units
    of 2^-52.  (A reverted melt is solved from T[n-1] - 10 eps: the identity is then about that profile.)
    Sea ice, thickness not clamped and no ice melted: lf rho[0] (thick' - thick) + base_flux_out dt = 0 to 4 ulps of lf rho[0]
    thick (the growth is formed from the rounded flux, so this is the statement of the rule), and base_flux_out is the new
    gradient's flux (kappa[0] + kappa[1]) 0.5 (T'[1] - T'[0]) / dz rounded to 1e-6: within 0.5e-6 and an ulp.

    What does NOT close, and is only measured.  The folded boundary rows hold the boundary node to the NEW gradient alone (flux
    top: kappa[n-2] (T'[n-1] - T'[n-2]) / dz = net), so F_top, a mean of old and new, is not the net flux, and the whole column's
    sum(rho c T dz) + lf rho growth does not close against the boundary fluxes times dt -- the reference's own
    tests/test_conservation.py says so and closes only the zero-forcing step (atol 1.0 J m^-2).  `face_gap` is the largest
    |F_top - net| over flux-top columns, `base_gap` the largest |F_base - base_flux_out| over sea-ice columns, in W m^-2."""
    k = constants(kind) if k is None else k
    n, ncol = c["t"].shape
    dt, eps = float(c["dt"]), float(k["eps"])
    net = c["sw_down"] + c["lw_down"] - c["sw_up"] - c["lw_up"] - c["sh"] - c["lh"]
    out = dict(ratio=0.0, residual=0.0, face_gap=0.0, base_gap=0.0, growth=0.0, columns=0)
    for col in np.nonzero(c["active"] == 1)[0]:
        total = c["thick"][col] + c["snow"][col]
        dz = total / n
        layer = np.arange(n - 1) > c["snow_level"][col]
        rho, cc, kappa = np.where(layer, k["rho_snow"], k["rho_ice"]), np.where(layer, k["c_snow"], k["c_ice"]), np.where(layer, k["k_snow"], k["k_ice"])
        hc = rho * cc
        hc_int = 0.5 * (hc[:-1] + hc[1:])
        r = 0.5 * (kappa[:-1] + kappa[1:]) * dt / (hc_int * 2.0 * dz * dz)
        old, new = c["t"][:, col].copy(), np.asarray(got["t_out"])[:, col]
        if c["reverted"][col]:
            old[-1] = old[-1] - 10.0 * eps
        s = new + old
        f_top, f_base = kappa[-1] * (s[-1] - s[-2]) / (2.0 * dz), kappa[0] * (s[1] - s[0]) / (2.0 * dz)
        residual = float(np.sum(hc_int * dz * (new[1:-1] - old[1:-1])) - dt * (f_top - f_base))
        scale = float(np.sum(hc_int * dz * (1.0 + 4.0 * r)) * np.abs(s).max() * 0.5) * 2.0 ** -52
        assert abs(residual) <= BUDGET_FACTOR * scale, (col, residual, scale)
        out["ratio"], out["residual"], out["columns"] = max(out["ratio"], abs(residual) / scale), max(out["residual"], abs(residual)), out["columns"] + 1
        if not (c["melting"][col] and not c["reverted"][col]):
            out["face_gap"] = max(out["face_gap"], abs(f_top - net[col]))
        if kind == 0:
            q = got["base_flux_out"][col]
            if not c["clamped"][col]:
                raw = (new[1] - new[0]) * (kappa[0] + kappa[1]) * 0.5 / dz
                assert abs(q - raw) <= 0.5e-6 + 4.0 * 2.0 ** -52 * abs(raw), (col, q, raw)
                out["base_gap"] = max(out["base_gap"], abs(f_base - q))
            if not c["clamped"][col] and not c["eats_ice"][col]:
                closing = k["lf"] * rho[0] * (got["thick_out"][col] - c["thick"][col]) + q * dt
                assert abs(closing) <= 4.0 * 2.0 ** -52 * k["lf"] * rho[0] * abs(c["thick"][col]), (col, closing)
                out["growth"] = max(out["growth"], abs(got["thick_out"][col] - c["thick"][col]))
    return out


# ---- host states for the components ---------------------------------------------------------------------------------------------------
AREA_NAMES = np.array(["land", "land_ice", "sea", "sea_ice"])


def host_state(kind, c, ny, nx):
    """A (lat, lon) grid; the radiative fluxes [lat][lon][interface_levels] of two levels (level 0 is the surface), the ice arrays
    with their levels LAST."""
    import datetime
    from climt_amd._sympl_compat import DataArray      # (here: the maker imports this module without the package)
    n = c["t"].shape[0]
    q2 = lambda a, units: DataArray(np.array(a).reshape(ny, nx), dims=("lat", "lon"), attrs={"units": units})
    ice = lambda a, units: DataArray(np.ascontiguousarray(np.transpose(a.reshape(n, ny, nx), (1, 2, 0))), dims=("lat", "lon", "ice_interface_levels"), attrs={"units": units})
    flux = lambda a: DataArray(np.stack([a.reshape(ny, nx), np.full((ny, nx), -5.0)], axis=-1), dims=("lat", "lon", "interface_levels"), attrs={"units": "W m^-2"})
    state = {"time": datetime.datetime(2000, 1, 1), "area_type": q2(AREA_NAMES[c["area_type"]], "dimensionless"),
             "snow_and_ice_temperature": ice(c["t"], "degK"), "height_on_ice_interface_levels": ice(c["height"], "m"),
             "surface_snow_thickness": q2(c["snow"], "m"), "surface_upward_latent_heat_flux": q2(c["lh"], "W m^-2"),
             "surface_upward_sensible_heat_flux": q2(c["sh"], "W m^-2"), "sea_surface_temperature": q2(np.full(ny * nx, 271.0), "degK")}
    for short, long in (("sw_down", "downwelling_shortwave_flux_in_air"), ("lw_down", "downwelling_longwave_flux_in_air"),
                        ("sw_up", "upwelling_shortwave_flux_in_air"), ("lw_up", "upwelling_longwave_flux_in_air")):
        state[long] = flux(c[short])
    if kind == 0:
        state.update({"sea_ice_thickness": q2(c["thick"], "m"), "heat_flux_into_sea_water_due_to_sea_ice": q2(c["base"], "W m^-2")})
    else:
        state.update({"land_ice_thickness": q2(c["thick"], "m"), "soil_surface_temperature": q2(c["base"], "degK")})
    return state


def without_the_tall_column(c):
    """The case with its one column that is too tall turned into open sea (neither component steps it) -> (case, which column)."""
    c = {k: np.array(v) if isinstance(v, np.ndarray) else v for k, v in c.items()}
    tall = c["too_tall"] == 1
    c["area_type"][tall] = 2      # open sea: neither component steps it
    return c, tall


@functools.lru_cache(maxsize=None)
def fixture(kind_name, name):
    return np.load(os.path.join(GOLDEN, "%s_%s.npz" % (kind_name, name)))


@functools.lru_cache(maxsize=None)
def tolerances(kind_name, name):
    """{field: tol} of tests/golden/<kind_name>_<name>.npz: measured by the maker on the reference (16 x the largest deviation under
    +-1 ulp of every input among runs with the same decisions, at least 1e-13), on the scale of `deviations`."""
    z = fixture(kind_name, name)
    return {f[4:]: float(z[f]) for f in z.files if f.startswith("tol_")}
