"""The gray radiation path (rrtmg_hip_frierson_optical_depth, rrtmg_hip_gray_longwave, rrtmg_hip_grid_scale_condensation and the three
components on them): the numpy statement of the three rules and the cases the tests run.

The statements are the rules of the reference's climt/_components/radiation.py and grid_scale_condensation.py in numpy's own
operations: a loop per column on numpy float64 scalars (`**` on them is numpy's scalar pow, np.exp / np.sin numpy's scalar
functions), the layer emission sigma T**4 and the heating lines on whole arrays, as the reference forms them.
tests/golden/make_gray_golden.py runs the reference's own functions and tests/test_gray.py compares the statements with what
they returned.  Level 0 is the surface; arrays are [levels][columns].

The condensation statement returns, besides the two profiles and the precipitation, `saturated` [nlay][ncol] -- what it decided --
and `margin`, the smallest |q - q_sat| / q_sat of the call.  Every condensation case keeps it >= MIN_MARGIN = 1e-9 (`gsc_case`
asserts it), so an exp that differs from libm's in its last bits cannot flip a decision.  The gray rules decide nothing.

Tolerances are not chosen here.  tests/golden/gray_<case>.npz and gsc_<case>.npz carry `tol_<field>`, measured by the maker from
the reference itself (its docstring has the rule); `tolerances` reads them and `deviations` states a result on their scale:
relative to the column's largest magnitude of the field, absolute where that is zero."""
import functools
import os

import numpy as np

SIGMA_SB, G, CPD = 5.670367e-8, 9.80665, 1004.64      # sympl's defaults, as GrayLongwaveRadiation asks for them
GRAY_CONSTANTS = dict(sigma_sb=SIGMA_SB, g=G, cpd=CPD)
FRIERSON = dict(tau0e=6.0, tau0p=1.5, fl=0.1)           # the reference's keyword defaults
GSC_CONSTANT_NAMES = ("cpd", "lv", "rd", "rh2o", "g", "rhow")
GSC_CONSTANTS = dict(cpd=1004.64, lv=2.5e6, rd=287.0, rh2o=461.5, g=9.80665, rhow=1000.0)
MIN_MARGIN = 1.0e-9
NLAYS = (1, 2, 30, 61)
NCOLS = (1, 64, 65, 130)
GRAY_CASES = ("varied", "isothermal", "transparent", "opaque", "decreasing", "zero_dtau")
FUSED_CASES = ("varied", "isothermal")      # their depth IS the Frierson depth of their pressures and latitudes: what the fused call computes
GSC_CASES = ("dry", "supersaturated", "alternate", "top_only", "bottom_only", "cold_stratosphere")
GRAY_INPUTS = ("t", "tsfc", "p_int", "tau", "ps", "lat")
GRAY_FIELDS = ("up", "dn", "tend", "hr")
GSC_INPUTS = ("t", "q", "p", "p_int")
GSC_FIELDS = ("t_new", "q_new", "precip")
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


# ---- the three rules ----------------------------------------------------------------------------------------------------------------
def frierson_statement(lat, p_int, ps, tau0e=FRIERSON["tau0e"], tau0p=FRIERSON["tau0p"], fl=FRIERSON["fl"], pressure_scale=1.0, ps_scale=1.0):
    """-> tau [nlay+1][ncol]: 0 at the surface, the latitude's tau_0 at the top."""
    nlev, ncol = p_int.shape
    tau = np.zeros((nlev, ncol))
    deg_to_rad = np.pi / 180.0
    for i in range(ncol):
        lat_rad = lat[i] * deg_to_rad
        tau_0 = tau0e + (tau0p - tau0e) * np.sin(lat_rad) ** 2
        ps_val = ps[i] * ps_scale
        for k in range(nlev):
            sigma = (p_int[k, i] * pressure_scale) / ps_val
            tau[k, i] = tau_0 * (1.0 - (fl * sigma + (1.0 - fl) * sigma ** 4))
    return tau


def gray_statement(t, tsfc, p_int, tau, k=GRAY_CONSTANTS, pressure_scale=1.0):
    """-> dict: up, dn [nlay+1][ncol], tend [K/s], hr [K/day] [nlay][ncol]."""
    sigma, g, cpd = (float(k[n]) for n in ("sigma_sb", "g", "cpd"))
    nlay, ncol = t.shape
    up, dn = np.zeros((nlay + 1, ncol)), np.zeros((nlay + 1, ncol))
    t4 = sigma * t ** 4
    for i in range(ncol):
        up[0, i] = sigma * tsfc[i] ** 4
        for j in range(1, nlay + 1):
            dtau = tau[j, i] - tau[j - 1, i]
            trans = np.exp(-dtau)
            up[j, i] = up[j - 1, i] * trans + t4[j - 1, i] * (1.0 - trans)
        dn[nlay, i] = 0.0
        for j in range(nlay - 1, -1, -1):
            dtau = tau[j + 1, i] - tau[j, i]
            trans = np.exp(-dtau)
            dn[j, i] = dn[j + 1, i] * trans + t4[j, i] * (1.0 - trans)
    net = up - dn
    p = p_int * pressure_scale
    tend = g / cpd * (net[1:, :] - net[:-1, :]) / (p[1:, :] - p[:-1, :])
    return dict(up=up, dn=dn, tend=tend, hr=tend * 86400.0)


def gsc_statement(t, q, p, p_int, k=GSC_CONSTANTS, pressure_scale=1.0):
    """-> dict: t_new, q_new [nlay][ncol], precip [ncol] (negative where it rains: level 0 is the surface and the reference takes
    p_int[k+1] - p_int[k]); saturated [nlay][ncol]; margin."""
    cpd, lv, rd, rh2o, g, rhow = (float(k[n]) for n in GSC_CONSTANT_NAMES)
    nlay, ncol = t.shape
    t_new, q_new, precip = t.copy(), q.copy(), np.zeros(ncol)
    saturated, margin = np.zeros((nlay, ncol), dtype=bool), np.inf
    for i in range(ncol):
        total = 0.0
        for j in range(nlay):
            tj, qj, pj = t[j, i], q[j, i], p[j, i] * pressure_scale
            es = 611.2 * np.exp(17.67 * (tj - 273.15) / (tj - 29.65))
            eps = rd / rh2o
            q_sat = eps * es / (pj - (1.0 - eps) * es)
            margin = min(margin, abs(qj - q_sat) / q_sat)
            if qj > q_sat:
                dqsat_dt = lv * q_sat / (rh2o * tj ** 2)
                condensed = (qj - q_sat) / (1.0 + lv / cpd * dqsat_dt)
                q_new[j, i] = qj - condensed
                t_new[j, i] = tj + lv / cpd * condensed
                dp = p_int[j + 1, i] * pressure_scale - p_int[j, i] * pressure_scale
                total += condensed * (dp / (g * rhow))
                saturated[j, i] = True
        precip[i] = total
    return dict(t_new=t_new, q_new=q_new, precip=precip, saturated=saturated, margin=float(margin))


def bolton_q_sat(t, p, k=GSC_CONSTANTS):
    es = 611.2 * np.exp(17.67 * (t - 273.15) / (t - 29.65))
    eps = k["rd"] / k["rh2o"]
    return eps * es / (p - (1.0 - eps) * es)


# ---- the grids ----------------------------------------------------------------------------------------------------------------------
def pressures(nlay, ncol):
    """-> (p [nlay][ncol], p_int [nlay+1][ncol], ps [ncol]) in Pa.  From 30 levels a sigma^1.5 grid up to 20 hPa; with fewer levels
    layers of 60 hPa from the surface up.  The surface pressure is NOT the lowest interface's (20 Pa more), so sigma < 1 there."""
    base = 1.0e5 + 37.0 * np.arange(ncol)
    if nlay >= 30:
        sigma = (1.0 - np.arange(nlay + 1) / float(nlay)) ** 1.5
        p_int = 2000.0 + sigma[:, None] * (base[None, :] - 2000.0)
    else:
        p_int = base[None, :] - 6000.0 * np.arange(nlay + 1)[:, None]
    return 0.5 * (p_int[:-1] + p_int[1:]), p_int, base + 20.0


def latitudes(ncol):
    """Degrees north, pole to pole, the equator itself in the middle column."""
    if ncol == 1:
        return np.array([35.0])
    lat = np.linspace(-90.0, 90.0, ncol)
    if ncol >= 3:
        lat[ncol // 2] = 0.0
    return lat


def _profile(nlay, ncol, seed):
    p, p_int, ps = pressures(nlay, ncol)
    rng = np.random.RandomState(seed + 131 * nlay + ncol)
    t = 212.0 + 80.0 * (p / p_int[0]) ** 1.3 + 0.013 * np.arange(ncol)[None, :] + rng.uniform(-1.5, 1.5, (nlay, ncol))
    return t, p, p_int, ps, rng


# ---- the gray cases -----------------------------------------------------------------------------------------------------------------
def _gray_inputs(name, nlay, ncol):
    if name not in GRAY_CASES:
        raise KeyError(name)
    t, p, p_int, ps, rng = _profile(nlay, ncol, 6006)
    lat = latitudes(ncol)
    tsfc = t[0] + 2.0 + 0.01 * (np.arange(ncol) % 9)
    lev = np.arange(nlay + 1)[:, None] * np.ones((1, ncol))
    tau = frierson_statement(lat, p_int, ps)
    if name == "isothermal":
        t, tsfc = np.full((nlay, ncol), 260.0), np.full(ncol, 260.0)
    elif name == "transparent":
        tau = np.ones((nlay + 1, 1)) * (0.3 + 0.01 * np.arange(ncol))[None, :]
    elif name == "opaque":
        tau = (760.0 + np.arange(ncol)[None, :]) * lev
        tsfc = np.array(t[0])
    elif name == "decreasing":
        tau = (3.0 + 0.002 * np.arange(ncol))[None, :] * (1.0 - lev / nlay)
    elif name == "zero_dtau":      # single layers of no depth: the layers k with (k + column) % 3 == 0, the lowest of column 0 among them
        dtau = np.where((lev[:-1] + np.arange(ncol)[None, :]) % 3 == 0, 0.0, tau[1:] - tau[:-1])
        tau = np.cumsum(np.concatenate([tau[:1], dtau]), axis=0)
    c = dict(t=t, tsfc=tsfc * np.ones(ncol), p_int=p_int, tau=tau * np.ones((nlay + 1, ncol)), ps=ps, lat=lat)
    return {k: np.ascontiguousarray(x, dtype=np.float64) for k, x in c.items()}


def check_gray_case(name, c):
    """Asserts that a case does what its name says (c: inputs and the statement's outputs)."""
    nlay, ncol = c["t"].shape
    for k in GRAY_FIELDS:
        assert np.isfinite(c[k]).all(), (name, k)
    dtau = c["tau"][1:] - c["tau"][:-1]
    if name in FUSED_CASES:
        assert same_bits(c["tau"], frierson_statement(c["lat"], c["p_int"], c["ps"])) and (dtau > 0).all() and (c["tau"][0] > 0).all()
    if name == "varied":
        if ncol >= 3:
            assert c["lat"][0] == -90.0 and c["lat"][-1] == 90.0 and (c["lat"] == 0.0).sum() == 1
        if ncol >= 3 and nlay >= 30:
            assert abs(c["tau"][-1, ncol // 2] / 6.0 - 1.0) < 0.01 and abs(c["tau"][-1, 0] / 1.5 - 1.0) < 0.01      # tau_0 at the top
    if name == "isothermal":      # up[k] = up t + up (1 - t): constant to a rounding per layer
        assert float(np.abs(c["up"] / c["up"][0] - 1.0).max()) <= 4 * nlay * np.finfo(float).eps
    if name == "transparent":
        assert not dtau.any()
        assert same_bits(c["dn"], np.zeros((nlay + 1, ncol))) and same_bits(c["up"], np.ones((nlay + 1, 1)) * c["up"][0][None, :])
        assert same_bits(c["tend"], -np.zeros((nlay, ncol)))      # a zero divergence over a negative pressure difference: -0.0
    if name == "opaque":
        assert (dtau >= 750.0).all() and not np.exp(-dtau).any()
        emission = SIGMA_SB * c["t"] ** 4
        assert same_bits(c["up"][1:], emission) and same_bits(c["dn"][:-1], emission)
    if name == "decreasing":
        assert (dtau < 0).all()
    if name == "zero_dtau":
        flat = dtau == 0.0
        assert flat.any(axis=0).all() or nlay < 3
        assert flat[0, 0] and (nlay < 2 or not flat[1, 0]) and (flat.sum(axis=0) >= nlay // 3).all()
        assert same_bits(c["up"][1:][flat], c["up"][:-1][flat]) and same_bits(c["dn"][1:][flat], c["dn"][:-1][flat])


@functools.lru_cache(maxsize=None)
def gray_case(name, nlay, ncol):
    """-> dict(the GRAY_INPUTS; the statement's outputs for the case's own tau).  Shared and read-only."""
    c = _gray_inputs(name, nlay, ncol)
    c.update(gray_statement(c["t"], c["tsfc"], c["p_int"], c["tau"]))
    check_gray_case(name, c)
    for x in c.values():
        x.setflags(write=False)
    return c


# ---- the condensation cases ---------------------------------------------------------------------------------------------------------
def _gsc_inputs(name, nlay, ncol):
    if name not in GSC_CASES:
        raise KeyError(name)
    t, p, p_int, ps, rng = _profile(nlay, ncol, 7007)
    colv = np.arange(ncol)[None, :]
    lev = np.arange(nlay)[:, None] * np.ones((1, ncol))
    dry = 0.45 + 0.2 * np.sin(0.31 * lev + 0.1 * colv)            # 0.25 .. 0.65
    wet = 1.06 + 0.002 * (colv % 11) + 0.05 * (1.0 + np.cos(lev))  # 1.06 .. 1.18
    q_fixed = None
    if name == "dry":
        rh = dry
    elif name == "supersaturated":
        rh = wet
    elif name == "alternate":
        rh = np.where((lev + colv) % 2 == 0, wet, dry)
    elif name == "top_only":
        rh = np.where(lev == nlay - 1, wet, dry)
    elif name == "bottom_only":
        rh = np.where(lev == 0, wet, dry)
    elif name == "cold_stratosphere":      # above 200 hPa: 185 .. 200 K and 3 ppm of water; below, each third column rains from two layers
        aloft = p < 20000.0
        t = np.where(aloft, 185.0 + 15.0 * rng.uniform(0.0, 1.0, (nlay, ncol)), t)
        rh = np.where((colv % 3 == 1) & (lev < 2), wet, dry)
        q_fixed = np.where(aloft, np.minimum(3.0e-6 * (1.0 + 0.1 * np.sin(lev + colv)), 0.3 * bolton_q_sat(t, p)), np.nan)
    q = rh * bolton_q_sat(t, p)
    if q_fixed is not None:
        q = np.where(np.isnan(q_fixed), q, q_fixed)
    return {k: np.ascontiguousarray(x, dtype=np.float64) for k, x in dict(t=t, q=q, p=p, p_int=p_int).items()}


def check_gsc_case(name, c):
    nlay, ncol = c["t"].shape
    assert c["margin"] >= MIN_MARGIN, (name, nlay, ncol, c["margin"])
    s, cols, lev = c["saturated"], np.arange(ncol)[None, :], np.arange(nlay)[:, None]
    for k in GSC_FIELDS:
        assert np.isfinite(c[k]).all(), (name, k)
    assert same_bits(c["t_new"][~s], c["t"][~s]) and same_bits(c["q_new"][~s], c["q"][~s])      # a layer that keeps its humidity keeps its bits
    assert (c["q_new"][s] < c["q"][s]).all() and (c["t_new"][s] > c["t"][s]).all()
    raining = s.any(axis=0)
    assert same_bits(c["precip"][~raining], np.zeros(int((~raining).sum()))) and (c["precip"][raining] < 0).all()      # the reference's sign
    if name == "dry":
        assert not s.any()
    if name == "supersaturated":
        assert s.all()
    if name == "alternate":
        assert (s == ((lev + cols) % 2 == 0)).all()
    if name == "top_only":
        assert (s == (lev == nlay - 1) * np.ones((1, ncol), dtype=bool)).all()
    if name == "bottom_only":
        assert (s == (lev == 0) * np.ones((1, ncol), dtype=bool)).all()
    if name == "cold_stratosphere":
        assert (s == ((cols % 3 == 1) & (lev < 2))).all()
        if nlay >= 30:
            aloft = c["p"] < 20000.0
            assert aloft.any(axis=0).all() and (c["t"][aloft] <= 200.0).all() and (c["q"][aloft] < 4e-6).all()


@functools.lru_cache(maxsize=None)
def gsc_case(name, nlay, ncol):
    """-> dict(the GSC_INPUTS; the statement's outputs, saturated, margin).  Shared and read-only."""
    c = _gsc_inputs(name, nlay, ncol)
    c.update(gsc_statement(c["t"], c["q"], c["p"], c["p_int"]))
    check_gsc_case(name, c)
    for x in c.values():
        if isinstance(x, np.ndarray):
            x.setflags(write=False)
    return c


# ---- comparing ----------------------------------------------------------------------------------------------------------------------
def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def deviations(got, c, fields):
    """got: dict with `fields` (one may be absent or None) -> {name: largest deviation over the columns}, each relative to the
    column's largest magnitude of the field in `c`, absolute where that is zero: the scale of the fixtures' tol_<field>."""
    dev = {}
    for name in fields:
        if got.get(name) is None:
            continue
        want = np.asarray(c[name])
        scale = np.abs(want).max(axis=0) if want.ndim == 2 else np.abs(want)
        diff = np.abs(np.asarray(got[name]) - want)
        diff = diff.max(axis=0) if want.ndim == 2 else diff
        with np.errstate(invalid="ignore"):
            dev[name] = float(np.max(diff / np.where(scale > 0, scale, 1.0)))
    return dev


@functools.lru_cache(maxsize=None)
def tolerances(kind, name):
    """{field: tol} of tests/golden/<kind>_<name>.npz (kind: "gray" or "gsc"): measured by the maker on the reference (16 x the
    largest deviation under +-1 ulp of every input, at least 1e-13), on the scale of `deviations`.  A gray file carries tol_tau
    too: the Frierson depth of the case's pressures and latitudes."""
    z = np.load(os.path.join(GOLDEN, "%s_%s.npz" % (kind, name)))
    return {f[4:]: float(z[f]) for f in z.files if f.startswith("tol_")}


def within(dev, tol):
    return all(v <= tol[k] for k, v in dev.items())
