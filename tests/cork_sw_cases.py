"""The table-driven correlated-k two-stream shortwave (rrtmg_hip_cork_shortwave and CorkShortwaveRadiation on it): the numpy
statement of the rules and the cases the tests run.

The statement is the rules of the reference's climt/_components/cork (sw/component.py, sw/kernels.py, optics/correlated_k.py,
common.py) in numpy's own operations on whole [layers][columns] arrays: every product, sum and quotient is the reference's, in
its order; Python's max(a, b) and min(a, b) are the first argument unless the second is strictly beyond it (pymax, pymin); only
the loops over columns and, in the layer operator, over layers are numpy's.  The brackets and the corner sums are cork_cases'.
tests/golden/make_cork_sw_golden.py runs the reference's own array_call and tests/test_cork_sw.py compares the statement with what
it returned.  Level 0 is the surface; profiles are [levels][columns], per-band arrays [bands][levels][columns], the three cloud
arrays [layers][columns][bands], as the component has them.

Tolerances are not chosen here: tests/golden/cork_sw_<case>.npz carries `tol_<field>`, measured by the maker from the reference
itself (16 x its largest deviation under +-1 ulp of every input, at least 1e-13, on the scale of cork_cases.deviations).  So that
no moved run crosses a discontinuity, no case has a zenith with |cos - 1e-4| < 1e-6, and wherever the delta-scaled single-scattering
albedo is positive |1 - (k mu0)^2| > 1e-3: check_case asserts both."""
import functools
import os

import numpy as np

import cork_cases as L

G, CPD, M_DRY, M_H2O, MOLAR_MASS = L.G, L.CPD, L.M_DRY, L.M_H2O, L.MOLAR_MASS
MIN_K, MIN_MU0, NIGHT = 1.0e-12, 1.0e-8, 1.0e-4
NLAYS = (1, 2, 30)
NCOLS = (1, 64, 65, 130)
BASE_TABLES = ("sw_earth", "sw_two_band", "sw_two_gas", "sw_premixed", "sw_no_rayleigh")
# The shape tables: made by the maker from a formula, every array float32, so that one file is run as a float table and, with k
# cast, as a double table.  name -> (gases, bands, g-points, nT, nP, nX, continuum, rayleigh)
SHAPE_TABLES = {"sw_g1": (("h2o",), 1, 1, 4, 4, 0, False, True), "sw_g3": (("effective",), 2, 3, 3, 3, 2, False, True), "sw_g5": (("h2o", "co2"), 2, 5, 3, 4, 0, False, False),
                "sw_g9_cont": (("effective",), 2, 9, 3, 3, 3, True, True), "sw_g16": (("effective",), 1, 16, 4, 3, 0, False, True)}
TABLES = BASE_TABLES + tuple(SHAPE_TABLES)
BASE_CASES = {"clear": "sw_two_band", "night": "sw_earth", "cloudy": "sw_no_rayleigh", "transparent": "sw_no_rayleigh", "resonance": "sw_no_rayleigh",
              "albedo": "sw_two_gas", "first_column_factor": "sw_premixed", "overcast": "sw_earth", "overcast_two_gas": "sw_two_gas", "overcast_g9_cont": "sw_g9_cont"}
# cloud over Rayleigh scattering, in sunlit and in dark columns alike: night's five kinds of sun, cloudy's cloud (without its dry and
# conservative layers), on a rank-6 float32 table, a two-gas double table and the continuum table of 9 g-points
OVERCAST = ("overcast", "overcast_two_gas", "overcast_g9_cont")
SHAPE_CASES = {name[3:]: name for name in SHAPE_TABLES}      # a clear atmosphere per shape table
CASES = dict(BASE_CASES, **SHAPE_CASES)
NG_BOUNDS = L.NG_BOUNDS
CLOUD = ("taucld", "ssacld", "asycld")
INPUTS = ("t", "p", "p_int", "zenith", "albedo", "earth_sun") + CLOUD      # and the gases of the table's rule
FIELDS = ("up", "dn", "tend", "hr", "up_band", "dn_band", "tau_band", "hr_band")
GOLDEN = L.GOLDEN
same_bits, deviations, within = L.same_bits, L.deviations, L.within


def table_path(name):
    return os.path.join(GOLDEN, "cork_sw_table_%s.npz" % name)


@functools.lru_cache(maxsize=None)
def table(name):
    """-> the fixture table as a dict of arrays, with rule (0 fully premixed, 1 premixed background, 2 per gas) and gases (the
    names of the gas inputs, in the library's order) as the reference's component derives them."""
    with np.load(table_path(name)) as z:
        t = {k: z[k] for k in z.files}
    names = [str(g) for g in t["gas_names"]]
    has_x = "h2o_vmr_grid" in t
    premixed_bg = (names == ["effective"] and has_x) or str(t.get("background_is_premixed", np.array(""))).lower() == "true"
    t["rule"] = 0 if names == ["effective"] and not has_x else 1 if premixed_bg else 2
    t["gases"] = [] if t["rule"] == 0 else ["h2o"] if t["rule"] == 1 else names
    return t


def kernel_ng(ngpt):
    return next(n for n in NG_BOUNDS if ngpt <= n)


def table_types(name):
    return ("f32", "f64") if name in SHAPE_TABLES else ("f32" if table(name)["k_coefficients"].dtype == np.float32 else "f64",)


# ---- the rules ----------------------------------------------------------------------------------------------------------------------
def pymax(a, b):
    return np.where(b > a, b, a)


def pymin(a, b):
    return np.where(b < a, b, a)


def gas_depth(tab, c, pressure_scale=1.0):
    """-> tau_abs [nband][ngpt][nlay][ncol] (k summed over the gases from 0.0, the continuum behind it) and dp [nlay][ncol]."""
    k = tab["k_coefficients"]
    ngas, nband, ngpt = k.shape[:3]
    assert k.ndim in (5, 6)
    t, p, p_int = c["t"], c["p"] * pressure_scale, c["p_int"] * pressure_scale
    nlay, ncol = t.shape
    iT, fT = L.bracket(np.asarray(tab["temperature_grid"], dtype=np.float64), t)
    iP, fP = L.bracket(np.asarray(tab["pressure_grid_log"], dtype=np.float64), np.log(np.maximum(p, 1.0)))
    dp = np.abs(p_int[1:] - p_int[:-1])
    rule = tab["rule"]
    if k.ndim == 6:
        x_grid = np.asarray(tab["h2o_vmr_grid"], dtype=np.float64)
        q = c["h2o"]
        x = q / np.maximum(q + (1.0 - q) * M_H2O, 1e-30)
        iX, fX = L.bracket(np.log(np.maximum(x_grid, 1e-30)), np.log(np.maximum(np.clip(x, float(x_grid[0]), float(x_grid[-1])), 1e-30)))
    amounts = []
    for ig in range(ngas):
        if rule == 2:
            name = tab["gases"][ig]
            qg = c[name] if name == "h2o" else c[name] * (MOLAR_MASS.get(name, M_DRY) / M_DRY)
            amounts.append(qg * dp / G)
        else:
            amounts.append(1.0 * dp / G if ig == 0 else np.zeros((nlay, ncol)))
    log_cont = None
    if "continuum_kappa" in tab and np.asarray(tab["continuum_kappa"]).ndim == 4 and k.ndim == 6 and rule == 1:
        log_cont = np.log(np.maximum(tab["continuum_kappa"], 1e-40))      # (rank 6: the reference takes the log in the file's own type)
    tau = np.zeros((nband, ngpt, nlay, ncol))
    for b in range(nband):
        contv = np.exp(L._txx(log_cont[b], iT, fT, iP, fP, iX, fX)) if log_cont is not None else None
        for g in range(ngpt):
            acc = np.zeros((nlay, ncol))
            for ig in range(ngas):
                kv = L._txx(k[ig, b, g], iT, fT, iP, fP, iX, fX) if k.ndim == 6 else L._tp(k[ig, b, g], iT, fT, iP, fP)
                acc += kv * amounts[ig]
            if contv is not None:
                acc += contv * amounts[0]
            tau[b, g] = acc
    return tau, dp


def delta_scale(tau, ssa, g):
    f = g * g
    with np.errstate(divide="ignore", invalid="ignore"):
        tau_s = tau * (1.0 - ssa * f)
        ssa_s = np.where((1.0 - ssa * f) > 1e-30, ssa * (1.0 - f) / (1.0 - ssa * f), 0.0)
        g_s = np.where((1.0 - f) > 1e-30, (g - f) / (1.0 - f), 0.0)
    return tau_s, ssa_s, g_s


def layer_operator(tau, w0, g, mu0, probe=None):
    """_sw_dif_and_source on arrays -> Rdif, Tdif, Rdir, Tdir, Tnoscat.  probe: a dict that collects what check_case asks about."""
    gamma1 = (8.0 - w0 * (5.0 + 3.0 * g)) * 0.25
    gamma2 = 3.0 * (w0 * (1.0 - g)) * 0.25
    k2 = (gamma1 - gamma2) * (gamma1 + gamma2)
    k = np.sqrt(pymax(k2, MIN_K))
    e1 = np.exp(-tau * k)
    e2 = e1 * e1
    RT = 1.0 / (k * (1.0 + e2) + gamma1 * (1.0 - e2))
    Rdif = RT * gamma2 * (1.0 - e2)
    Tdif = RT * 2.0 * k * e1
    mu0_s = pymax(mu0, MIN_MU0)
    Tnoscat = np.exp(-tau / mu0_s)
    k_mu = k * mu0_s
    den = 1.0 - k_mu * k_mu
    guard = np.abs(den) < 1e-30
    den = np.where(guard, 1e-30, den)
    RTd = w0 * RT / den
    gamma3 = (2.0 - 3.0 * mu0_s * g) * 0.25
    gamma4 = 1.0 - gamma3
    alpha1 = gamma1 * gamma4 + gamma2 * gamma3
    alpha2 = gamma1 * gamma3 + gamma2 * gamma4
    kg3, kg4 = k * gamma3, k * gamma4
    Rraw = RTd * ((1.0 - k_mu) * (alpha2 + kg3) - (1.0 + k_mu) * (alpha2 - kg3) * e2 - 2.0 * (kg3 - alpha2 * k_mu) * e1 * Tnoscat)
    Traw = -RTd * ((1.0 + k_mu) * (alpha1 + kg4) * Tnoscat - (1.0 - k_mu) * (alpha1 - kg4) * e2 * Tnoscat - 2.0 * (kg4 + alpha1 * k_mu) * e1)
    Rdir = pymax(0.0, pymin(Rraw, 1.0 - Tnoscat))
    Tdir = pymax(0.0, pymin(Traw, 1.0 - Tnoscat - Rdir))
    if probe is not None:
        day = np.broadcast_to(mu0 > NIGHT, tau.shape)
        add = lambda name, x: probe.__setitem__(name, probe.get(name, 0) + int(np.count_nonzero(x & day)))
        add("k_floor", k2 < MIN_K), add("den_guard", guard), add("layers", np.ones(tau.shape, dtype=bool))
        add("rdir_clamped", (Rraw < 0.0) | (Rraw > 1.0 - Tnoscat)), add("rdir_free", (Rraw > 0.0) & (Rraw < 1.0 - Tnoscat))
        add("tdir_clamped", (Traw < 0.0) | (Traw > 1.0 - Tnoscat - Rdir)), add("tdir_free", (Traw > 0.0) & (Traw < 1.0 - Tnoscat - Rdir))
        add("beam_underflow", Tnoscat == 0.0), add("source_zero", (Rdir == 0.0) & (Tdir == 0.0))
        sel = (w0 > 0.0) & day
        gap = np.where(sel, np.abs(1.0 - (k * mu0_s) ** 2), np.inf).min(axis=0)      # by column
        probe["gap_by_column"] = np.minimum(probe.get("gap_by_column", np.inf), gap)
        probe["resonance_gap"] = float(probe["gap_by_column"].min())
    return Rdif, Tdif, Rdir, Tdir, Tnoscat


def statement(tab, c, pressure_scale=1.0, probe=None):
    """tab: a table dict; c: the inputs (t, p [nlay][ncol], p_int [nlay+1][ncol], zenith, albedo, earth_sun [ncol], taucld, ssacld,
    asycld [nlay][ncol][nband] and the gases of the table's rule) -> dict of FIELDS."""
    tau_abs, dp = gas_depth(tab, c, pressure_scale)
    nband, ngpt, nlay, ncol = tau_abs.shape
    p_int = c["p_int"] * pressure_scale
    w = tab["gpoint_weights"]
    ray = tab.get("rayleigh_coefficient")
    solar = tab["solar_source_per_gpoint"]
    solar_flux = solar * solar.dtype.type(float(c["earth_sun"][0]))      # in the table's element type, the first column's factor
    mu0 = np.cos(c["zenith"])
    day = mu0 > NIGHT
    up_band, dn_band = np.zeros((nband, nlay + 1, ncol)), np.zeros((nband, nlay + 1, ncol))
    tau_band = np.zeros((nband, nlay, ncol))
    with np.errstate(all="ignore"):
        for b in range(nband):
            tau_c, ssa_c, g_c = (c[n][:, :, b] for n in CLOUD)
            for g in range(ngpt):
                tau, ssa = tau_abs[b, g], np.zeros((nlay, ncol))
                if ray is not None:
                    tau_ray = np.float64(ray[b]) * dp / G
                    tau = tau_abs[b, g] + tau_ray
                    ssa = np.where(tau > 0, tau_ray / tau, 0.0)
                tau_total = tau + tau_c
                scat_gas, scat_cloud = tau * ssa, tau_c * ssa_c
                scat_total = scat_gas + scat_cloud
                ssa_total = np.where(tau_total > 0, scat_total / tau_total, 0.0)
                g_total = np.where(scat_total > 0, (scat_gas * 0.0 + scat_cloud * g_c) / scat_total, 0.0)
                if probe is not None:
                    mixed = (scat_gas > 0) & (scat_cloud > 0)      # gas and cloud both scatter: g_total lies strictly between 0 and g_c
                    ratio = g_total[mixed] / g_c[mixed]
                    probe["g_mixed"] = probe.get("g_mixed", 0) + int(np.count_nonzero(mixed))
                    probe["g_not_between"] = probe.get("g_not_between", 0) + int(np.count_nonzero(~((0.0 < g_total[mixed]) & (g_total[mixed] < g_c[mixed]))))
                    probe["g_ratio_max"] = float(np.max(ratio, initial=probe.get("g_ratio_max", -np.inf)))      # of g_total / g_c
                    probe["g_ratio_min"] = float(np.min(ratio, initial=probe.get("g_ratio_min", np.inf)))
                    probe["ssa_fallback"] = probe.get("ssa_fallback", 0) + int(np.count_nonzero(~(tau_total > 0)))
                    probe["g_fallback"] = probe.get("g_fallback", 0) + int(np.count_nonzero(~(scat_total > 0)))
                    probe["w0_max"] = max(probe.get("w0_max", 0.0), float(ssa_total.max()))
                tau_s, ssa_s, g_s = delta_scale(tau_total, ssa_total, g_total)
                if probe is not None:
                    f = g_total * g_total
                    probe["delta_guards"] = probe.get("delta_guards", 0) + int(np.count_nonzero(~((1.0 - ssa_total * f) > 1e-30) & ~((1.0 - f) > 1e-30)))
                Rdif, Tdif, Rdir, Tdir, Tnoscat = layer_operator(tau_s, ssa_s, g_s, mu0[None, :], probe)
                beam = np.ones((nlay + 1, ncol))
                for j in range(nlay - 1, -1, -1):
                    beam[j] = Tnoscat[j] * beam[j + 1]
                src_up, src_dn = Rdir * beam[1:], Tdir * beam[1:]
                alb, src, denom = np.zeros((nlay + 1, ncol)), np.zeros((nlay + 1, ncol)), np.zeros((nlay, ncol))
                alb[0], src[0] = c["albedo"], beam[0] * c["albedo"]
                for j in range(nlay):
                    denom[j] = 1.0 / (1.0 - Rdif[j] * alb[j])
                    alb[j + 1] = Rdif[j] + Tdif[j] * Tdif[j] * alb[j] * denom[j]
                    src[j + 1] = src_up[j] + Tdif[j] * denom[j] * (src[j] + alb[j] * src_dn[j])
                fup, fdn = np.zeros((nlay + 1, ncol)), np.zeros((nlay + 1, ncol))
                fup[nlay] = fdn[nlay] * alb[nlay] + src[nlay]
                for j in range(nlay - 1, -1, -1):
                    fdn[j] = (Tdif[j] * fdn[j + 1] + Rdif[j] * src[j] + src_dn[j]) * denom[j]
                    fup[j] = fdn[j] * alb[j] + src[j]
                scale = np.float64(solar_flux[b, g]) * mu0 * np.float64(w[b, g])
                up_band[b] += np.where(day, fup * scale, 0.0)
                dn_band[b] += np.where(day, (beam + fdn) * scale, 0.0)
                tau_band[b] += np.float64(w[b, g]) * tau_total
    up, dn = np.zeros((nlay + 1, ncol)), np.zeros((nlay + 1, ncol))
    for b in range(nband):
        up += up_band[b]
        dn += dn_band[b]
    tend = L.heating(up - dn, p_int)
    hr_band = np.stack([L.heating(up_band[b] - dn_band[b], p_int) * 86400.0 for b in range(nband)])
    return dict(up=up, dn=dn, tend=tend, hr=tend * 86400.0, up_band=up_band, dn_band=dn_band, tau_band=tau_band, hr_band=hr_band)


# ---- the cases ----------------------------------------------------------------------------------------------------------------------
def _half():
    """-> (zenith, whether np.cos(zenith) is 0.5 exactly): the nextafter search from pi/3 for a cosine of exactly 0.5.  The doubles
    next to pi/3 straddle it under this numpy, so the search may end on the nearest one (cosine within an ulp of 0.5: k mu0 = 1 to
    within an ulp, the guard |1 - (k mu0)^2| < 1e-30 not taken).  The guard itself is taken by mu0 = 0.5 handed to the layer
    function directly: tests/test_cork_sw.py, the check program's `layer` mode."""
    z = best = np.float64(np.pi / 3.0)
    for _ in range(64):
        got = np.cos(z)
        if got == 0.5:
            return z, True
        if abs(got - 0.5) < abs(np.cos(best) - 0.5):
            best = z
        z = np.nextafter(z, -np.inf if got < 0.5 else np.inf)
    return best, False


def _inputs(name, nlay, ncol):
    tab = table(CASES[name])
    nband = tab["k_coefficients"].shape[1]
    shape = (nlay, ncol)
    p_int = L.pressures(nlay, ncol)
    colv, lev = np.arange(ncol), np.arange(nlay)[:, None]
    p = 0.5 * (p_int[:-1] + p_int[1:])
    t = 212.0 + 80.0 * (p / p_int[0]) ** 1.3 + 0.013 * colv[None, :] + 1.5 * np.sin(0.7 * lev + 0.3 * colv[None, :])
    frac = lambda x: np.mod(x, 1.0)
    c = dict(t=t, p=p, p_int=p_int, zenith=0.1 + 1.2 * frac(0.6180339887498949 * (colv + 1)), albedo=0.05 + 0.6 * frac(0.3819660112501051 * (colv + 1)),
             earth_sun=np.full(ncol, 1.0178), taucld=np.zeros(shape + (nband,)), ssacld=np.zeros(shape + (nband,)), asycld=np.zeros(shape + (nband,)))
    for ig, gas in enumerate(tab["gases"]):
        if gas == "h2o":
            c["h2o"] = L._spread(shape, 2.0e-6, 0.03, 2, log=True) if tab["rule"] == 1 else L._spread(shape, 1.0e-3, 0.02, 2, log=True)
        else:
            c[gas] = L._spread(shape, 2.0e-4, 8.0e-4, 3 + ig, log=True)
    if name == "night" or name in OVERCAST:      # among sunlit columns: the sun on the horizon, below it, and just above the threshold (cos = 2e-4)
        kinds = np.array([0.3, np.pi / 2.0, 2.0, np.arccos(2.0e-4), 1.0])
        c["zenith"] = kinds[colv % 5] + 1.0e-3 * (colv // 5) * (colv % 5 != 3)
    if name == "cloudy" or name in OVERCAST:
        # cloud in the layers with (k + column) % 3 == 0, depth, ssa and g by band (an overcast case: no more than that, the same in dark
        # and sunlit columns); cloudy, layer 1: conservative cloud in dry air (ssa = 1: the floor of k); layer 0: ssa = 1 and g = 1 in
        # dry air (both guards of the delta scaling); a low and a high sun by column
        bandv = np.arange(nband)[None, None, :]
        on = ((lev + colv[None, :]) % 3 == 0)[:, :, None] * np.ones(shape + (nband,))
        c["taucld"] = on * (0.5 + 2.0 * bandv + 0.05 * (colv[None, :, None] % 5))
        c["ssacld"] = on * (0.999 - 0.15 * bandv)
        c["asycld"] = on * (0.86 - 0.1 * bandv)
    if name == "cloudy":
        h2o = np.array(c["h2o"])
        for k_dry, g_dry in ((0, 1.0), (1, 0.8)):      # (from 3 layers on: below that every layer absorbs, and the column's heating is physical)
            if nlay >= 3:
                h2o[k_dry] = 0.0
                c["taucld"][k_dry], c["ssacld"][k_dry], c["asycld"][k_dry] = 3.0, 1.0, g_dry
        c["h2o"] = h2o
        if nlay > 5:      # a thin backscattering layer (g < 0): under the high sun Rdir comes out above 1 - Tnoscat, the clamp of Rdir is active
            c["taucld"][5], c["ssacld"][5], c["asycld"][5] = 0.1, 0.9, -0.8
        c["zenith"] = np.where(colv % 2 == 0, 0.2 + 0.01 * colv / max(ncol, 1), 1.45 + 0.0005 * colv)
    if name in ("transparent", "resonance"):      # no Rayleigh, no cloud: w0 = 0 and k = 2 everywhere
        if name == "transparent":      # and layers with no water vapour at all: tau = 0, both `where` fallbacks
            h2o = np.array(c["h2o"])
            h2o[(lev + colv[None, :]) % 2 == 0] = 0.0
            c["h2o"] = h2o
        else:
            c["zenith"] = np.where(colv % 2 == 0, _half()[0], c["zenith"])
    if name == "albedo":
        c["albedo"] = np.where(colv % 3 == 0, 0.0, np.where(colv % 3 == 1, 1.0, c["albedo"]))
    if name == "first_column_factor":
        c["earth_sun"] = 0.967 + 0.066 * frac(0.6180339887498949 * (colv + 3))
    c = {k: np.ascontiguousarray(x, dtype=np.float64) for k, x in c.items()}
    for _ in range(40):      # away from k mu0 = 1 wherever a layer scatters: a column that comes within 2e-3 gets a sun 0.01 rad lower
        probe = {}
        statement(tab, c, probe=probe)
        near = probe["gap_by_column"] <= 2e-3
        if not near.any():
            break
        c["zenith"] = np.where(near, c["zenith"] + 0.01, c["zenith"])
    return c


def gas_names(name):
    return list(table(CASES[name])["gases"])


def check_case(name, c, probe):
    """Asserts that a case does what its name says (c: inputs and the statement's outputs; probe: what the statement left in it)."""
    tab = table(CASES[name])
    nlay, ncol = c["t"].shape
    mu0 = np.cos(c["zenith"])
    for f in FIELDS:
        assert np.isfinite(c[f]).all(), (name, f)
    assert (np.abs(mu0 - NIGHT) >= 1e-6).all(), name
    assert probe.get("resonance_gap", np.inf) > 1e-3, (name, probe)
    dark = mu0 <= NIGHT
    for f in ("up", "dn", "up_band", "dn_band"):
        assert same_bits(c[f][..., dark], np.zeros_like(c[f][..., dark])), (name, f)
    big = nlay >= 2 and ncol >= 5
    k = tab["k_coefficients"]
    if name == "clear":
        assert k.ndim == 5 and k.dtype == np.float64 and tab["rule"] == 2 and "rayleigh_coefficient" in tab and not dark.any() and not c["taucld"].any()
        assert np.unique(c["zenith"]).size == ncol and np.unique(c["earth_sun"]).size == 1
    if name == "night":
        assert k.ndim == 6 and k.dtype == np.float32 and tab["rule"] == 1 and "rayleigh_coefficient" in tab and tab["solar_source_per_gpoint"].dtype == np.float32
    if name == "night" and big:
        kinds = np.arange(ncol) % 5
        assert dark[kinds == 1].all() and dark[kinds == 2].all() and not dark[(kinds != 1) & (kinds != 2)].any()
        assert (c["zenith"][kinds == 1] >= np.pi / 2).all() and (c["zenith"][kinds == 2] > np.pi / 2).all() and np.abs(mu0[kinds == 3] - 2e-4).max() < 1e-9
        assert probe["beam_underflow"] > 0 and (c["dn"][-1, ~dark] > 0).all()
        assert np.signbit(c["tend"][:, dark]).all() and (c["tend"][:, dark] == 0).all()      # -0.0: what the formula makes of zeros
    if name == "cloudy":
        assert k.ndim == 5 and tab["rule"] == 2 and "rayleigh_coefficient" not in tab      # (Rayleigh's g = 0 would keep g_total below 1)
        assert (c["taucld"] > 0).any()
        if nlay >= 3:
            assert probe["k_floor"] > 0 and probe["w0_max"] == 1.0
            assert (c["ssacld"][1] == 1.0).all() and (c["asycld"][1] == 0.8).all() and (c["h2o"][1] == 0.0).all()
            assert (c["ssacld"][0] == 1.0).all() and (c["asycld"][0] == 1.0).all() and probe["delta_guards"] > 0
        else:
            assert (c["h2o"] > 0).all() and probe["w0_max"] < 1.0
        if nlay >= 30 and ncol >= 4:
            assert (c["taucld"] == 0).any() and len({float(x) for x in c["ssacld"][3, 0]}) == k.shape[1]
            for which in ("rdir", "tdir"):      # each energy clamp active on some layers and inactive on others
                assert probe[which + "_clamped"] > 0 and probe[which + "_free"] > 0, (name, which, probe)
    if name in OVERCAST:
        assert "rayleigh_coefficient" in tab and (c["taucld"] > 0).any() and (c["ssacld"] < 1.0).all() and all((c[g] > 0).all() for g in tab["gases"])
        if name == "overcast":
            assert k.ndim == 6 and k.dtype == np.float32 and tab["rule"] == 1 and tab["solar_source_per_gpoint"].dtype == np.float32 and k.shape[1:3] == (3, 2)
        if name == "overcast_two_gas":
            assert k.ndim == 5 and k.dtype == np.float64 and tab["rule"] == 2 and tab["gases"] == ["h2o", "co2"]
        if name == "overcast_g9_cont":
            gases, nband, ngpt, nT, nP, nX, cont, rayleigh = SHAPE_TABLES[CASES[name]]
            assert CASES[name] in SHAPE_TABLES and k.shape == (1, nband, 9, nT, nP, nX) and kernel_ng(k.shape[2]) == 16 and tab["rule"] == 1
            assert np.asarray(tab["continuum_kappa"]).ndim == 4 and all(tab[a].dtype == np.float32 for a in tab if isinstance(tab[a], np.ndarray) and tab[a].dtype.kind == "f")
    if name in OVERCAST and big:
        kinds = np.arange(ncol) % 5
        assert dark[kinds == 1].all() and dark[kinds == 2].all() and not dark[(kinds != 1) & (kinds != 2)].any()
        assert probe["g_mixed"] > 0 and probe["g_not_between"] == 0 and 0.0 < probe["g_ratio_min"] <= probe["g_ratio_max"] < 1.0, (name, probe)
        assert probe["beam_underflow"] > 0 and (c["dn"][-1, ~dark] > 0).all()
        assert np.signbit(c["tend"][:, dark]).all() and (c["tend"][:, dark] == 0).all()      # -0.0: what the formula makes of zeros
        clouded = np.moveaxis(c["taucld"], -1, 0) > 0      # [band][layer][column], as tau_band
        assert clouded[:, :, dark].any()
        bare = statement(tab, dict(c, **{n: np.zeros_like(c[n]) for n in CLOUD}))["tau_band"]      # a dark column's depth is formed with its cloud
        at = clouded & dark[None, None, :]
        assert (c["tau_band"][at] > bare[at]).all() and same_bits(c["tau_band"][~clouded], bare[~clouded])
    if name == "transparent":
        assert "rayleigh_coefficient" not in tab and not c["taucld"].any() and probe["w0_max"] == 0.0
        if big:
            assert probe["ssa_fallback"] > 0 and probe["g_fallback"] > 0 and (c["tau_band"] == 0).any() and (c["tau_band"] > 0).any()
    if name == "resonance":
        assert "rayleigh_coefficient" not in tab and probe["w0_max"] == 0.0 and probe["source_zero"] == probe["layers"]
        exact = _half()[1]
        assert (np.abs(mu0[::2] - 0.5) <= (0.0 if exact else 1.2e-16)).all() and (probe["den_guard"] > 0) == exact
    if name == "albedo" and ncol >= 3:
        assert (c["albedo"] == 0.0).any() and (c["albedo"] == 1.0).any() and tab["gases"] == ["h2o", "co2"]
    if name == "first_column_factor":
        assert tab["rule"] == 0 and (ncol == 1 or np.unique(c["earth_sun"]).size > 1)
        uniform = dict(c, earth_sun=np.full(ncol, c["earth_sun"][0]))
        again = statement(tab, uniform)
        assert all(same_bits(again[f], c[f]) for f in FIELDS)
    if name in SHAPE_CASES:
        gases, nband, ngpt, nT, nP, nX, cont, rayleigh = SHAPE_TABLES[CASES[name]]
        assert k.shape == (len(gases), nband, ngpt, nT, nP) + (nX,) * (nX > 0) and ("continuum_kappa" in tab) == cont and ("rayleigh_coefficient" in tab) == rayleigh
        assert all(tab[a].dtype == np.float32 for a in tab if isinstance(tab[a], np.ndarray) and tab[a].dtype.kind == "f")


@functools.lru_cache(maxsize=None)
def cork_sw_case(name, nlay, ncol):
    """-> dict(the inputs; the statement's outputs).  Shared and read-only."""
    c, probe = _inputs(name, nlay, ncol), {}
    c.update(statement(table(CASES[name]), c, probe=probe))
    check_case(name, c, probe)
    for x in c.values():
        x.setflags(write=False)
    return c


@functools.lru_cache(maxsize=None)
def tolerances(name):
    """{field: tol} of tests/golden/cork_sw_<name>.npz: measured by the maker on the reference."""
    z = np.load(os.path.join(GOLDEN, "cork_sw_%s.npz" % name))
    return {f[4:]: float(z[f]) for f in z.files if f.startswith("tol_")}
