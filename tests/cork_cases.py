"""The table-driven correlated-k longwave (rrtmg_hip_cork_longwave and CorkLongwaveRadiation on it): the numpy statement of the
rules and the cases the tests run.

The statement is the rules of the reference's climt/_components/cork (optics/correlated_k.py, lw/kernels.py, lw/component.py,
common.py) in numpy's own operations on whole [layers][columns] arrays: every product, sum and quotient is the reference's, in
its order (the corner sums of _ck_txx7 / _txx / _tp, the gas sum from 0.0, the continuum behind it, the cloud depth behind that,
the g-sum and the band sum from 0.0); only the loops over columns and layers are numpy's.  numpy's array exp / log / pow may
differ from its scalar ones in the last bit, which the tolerances -- measured with inputs moved by an ulp -- are there for.
tests/golden/make_cork_golden.py runs the reference's own array_call and tests/test_cork_lw.py compares the statement with
what it returned.  Level 0 is the surface; profiles are [levels][columns], per-band arrays [bands][levels][columns], the cloud
depth [layers][columns][bands], as the component has them.

Tolerances are not chosen here.  tests/golden/cork_<case>.npz carries `tol_<field>`, measured by the maker from the reference
itself (its docstring has the rule); `tolerances` reads them and `deviations` states a result on their scale: relative to the
column's largest magnitude of the field, absolute where that is zero."""
import functools
import os

import numpy as np

SIGMA_SB, G, CPD = 5.670367e-8, 9.80665, 1004.64      # sympl's defaults, as CorkLongwaveRadiation asks for them
M_DRY = 28.970
MOLAR_MASS = {"h2o": 18.015, "co2": 44.010, "o3": 47.998, "ch4": 16.043, "n2o": 44.013, "o2": 31.998}
M_H2O = MOLAR_MASS["h2o"] / M_DRY
NLAYS = (1, 2, 30, 61)
NCOLS = (1, 64, 65, 130)
BASE_TABLES = ("earth4", "h2o_axis", "two_band", "two_gas", "premixed")      # derived from the reference's shipped tables
# The shape tables: made by the maker from a formula (its docstring), every array float32, so that one file is run as a float table
# and, with k cast, as a double table.  name -> (gases, bands, g-points, nT, nP, nX, nC, continuum)
GASES8 = ("co2", "nh3", "h2o", "o3", "ch4", "so2", "n2o", "o2")      # (nh3 and so2: not in MOLAR_MASS, their scale is 1.0)
SHAPE_TABLES = {"g1": (("h2o",), 1, 1, 5, 4, 0, 0, False), "g3_min": (("effective",), 3, 3, 2, 2, 2, 0, False), "g4_gases8": (GASES8, 2, 4, 4, 5, 0, 0, False),
                "g5_rank7": (("effective",), 2, 5, 3, 4, 3, 2, False), "g9": (("effective",), 2, 9, 5, 3, 0, 0, False),
                "g16_cont": (("effective",), 2, 16, 4, 4, 3, 3, True), "bands32": (("h2o", "co2"), 32, 2, 3, 5, 0, 0, False)}
TABLES = BASE_TABLES + tuple(SHAPE_TABLES)
# case -> (table, diffusivity factor)
BASE_CASES = {"earth": ("earth4", 1.66), "earth_d2": ("earth4", 2.0), "on_nodes": ("earth4", 1.66), "h2o_axis": ("h2o_axis", 1.66), "two_band": ("two_band", 1.66),
              "two_gas": ("two_gas", 1.66), "premixed": ("premixed", 1.66), "cloudy": ("earth4", 1.66), "emissivity": ("earth4", 1.66)}
# one atmosphere within the grids per shape table; `_spans`: past both ends of every axis; `_cloudy`: cloud and emissivity by band
SHAPE_CASES = {"g1": ("g1", 1.66), "g3_min": ("g3_min", 1.66), "g3_min_spans": ("g3_min", 1.66), "g4_gases8": ("g4_gases8", 1.66), "g5_rank7": ("g5_rank7", 1.66),
               "g5_rank7_spans": ("g5_rank7", 1.66), "g9": ("g9", 1.66), "g16_cont": ("g16_cont", 1.66), "g16_cont_spans": ("g16_cont", 1.66),
               "bands32": ("bands32", 1.66), "bands32_cloudy": ("bands32", 1.66)}
CASES = dict(BASE_CASES, **SHAPE_CASES)
SPANS = ("earth", "earth_d2", "g3_min_spans", "g5_rank7_spans", "g16_cont_spans")
# cork_band_kernel<NG, K>: NG is the first of these that holds the table's g-points -- the thresholds of cork_launch_band
# (climt_amd/csrc/rrtmg_cork.hip; run_bands of tools/cork_check.cpp has the same)
NG_BOUNDS = (1, 2, 4, 8, 16)
INPUTS = ("t", "p", "p_int", "tsfc", "emis", "taucld")          # and the gases of the table's rule: "h2o", "co2", ...
FIELDS = ("up", "dn", "tend", "hr", "up_band", "dn_band", "tau_band", "trans_band", "hr_band")
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


# ---- the tables ---------------------------------------------------------------------------------------------------------------------
def table_path(name):
    return os.path.join(GOLDEN, "cork_table_%s.npz" % name)


@functools.lru_cache(maxsize=None)
def table(name):
    """-> the fixture table as a dict of arrays, with what the statement needs of it: rule (0 fully premixed, 1 premixed
    background, 2 per gas), gases (the names of the gas inputs, in the library's order)."""
    with np.load(table_path(name)) as z:
        t = {k: z[k] for k in z.files}
    names = [str(g) for g in t["gas_names"]]
    has_x, has_c = "h2o_vmr_grid" in t, "co2_vmr_grid" in t
    t["rule"] = 0 if names == ["effective"] and not has_x else 1 if names == ["effective"] and has_x else 2
    t["gases"] = [] if t["rule"] == 0 else (["h2o"] + (["co2"] if has_c else [])) if t["rule"] == 1 else names
    return t


def kernel_ng(ngpt):
    return next(n for n in NG_BOUNDS if ngpt <= n)


def table_types(name):
    """-> the element types of k the tests run the table in: a shape table as stored and with k cast to double (every value is
    float32-exact), any other in the file's own."""
    return ("f32", "f64") if name in SHAPE_TABLES else ("f32" if table(name)["k_coefficients"].dtype == np.float32 else "f64",)


# ---- the rules ----------------------------------------------------------------------------------------------------------------------
def bracket(grid, v):
    """_ck_bracket on an array: searchsorted-left minus one, the index clamp, the fraction clamp."""
    n = grid.shape[0]
    i = np.clip(np.searchsorted(grid, v) - 1, 0, n - 2)
    f = (v - grid[i]) / (grid[i + 1] - grid[i])
    return i, np.where(f < 0.0, 0.0, np.where(f > 1.0, 1.0, f))


def _tp(base, iT, fT, iP, fP, *rest):
    """_tp: base [nT][nP] (or, with `rest` = trailing indices, the plane of them)."""
    v = lambda a, b: base[(a, b) + rest].astype(np.float64)
    return v(iT, iP) * (1.0 - fT) * (1.0 - fP) + v(iT + 1, iP) * fT * (1.0 - fP) + v(iT, iP + 1) * (1.0 - fT) * fP + v(iT + 1, iP + 1) * fT * fP


def _txx(base, iT, fT, iP, fP, iX, fX, *rest):
    x0 = _tp(base, iT, fT, iP, fP, iX, *rest)
    x1 = _tp(base, iT, fT, iP, fP, iX + 1, *rest)
    return x0 * (1.0 - fX) + x1 * fX


def heating(net, p_int):
    """compute_heating_rate: K/s."""
    return G / CPD * (net[1:] - net[:-1]) / (p_int[1:] - p_int[:-1])


def statement(tab, c, diffusivity=1.66, pressure_scale=1.0, probe=None):
    """tab: a table dict; c: the inputs (t, p [nlay][ncol], p_int [nlay+1][ncol], tsfc [ncol], emis [nband][ncol], taucld
    [nlay][ncol][nband] and the gases of the table's rule) -> dict of FIELDS.  probe: a dict that is given tau_min and tau_max,
    the smallest and the largest layer optical depth of any g-point before the cloud."""
    k = tab["k_coefficients"]
    ngas, nband, ngpt = k.shape[:3]
    t, p, p_int = c["t"], c["p"] * pressure_scale, c["p_int"] * pressure_scale
    nlay, ncol = t.shape
    t_grid, p_grid = np.asarray(tab["temperature_grid"], dtype=np.float64), np.asarray(tab["pressure_grid_log"], dtype=np.float64)
    iT, fT = bracket(t_grid, t)
    iP, fP = bracket(p_grid, np.log(np.maximum(p, 1.0)))
    dp = np.abs(p_int[1:] - p_int[:-1])
    rule = tab["rule"]
    if k.ndim >= 6:
        x_grid = np.asarray(tab["h2o_vmr_grid"], dtype=np.float64)
        q = c["h2o"]
        x = q / np.maximum(q + (1.0 - q) * M_H2O, 1e-30)
        iX, fX = bracket(np.log(np.maximum(x_grid, 1e-30)), np.log(np.maximum(np.clip(x, float(x_grid[0]), float(x_grid[-1])), 1e-30)))
    if k.ndim == 7:
        c_grid = np.asarray(tab["co2_vmr_grid"], dtype=np.float64)
        iC, fC = bracket(np.log(np.maximum(c_grid, 1e-30)), np.log(np.maximum(np.clip(c["co2"], float(c_grid[0]), float(c_grid[-1])), 1e-30)))
    amounts = []
    for ig in range(ngas):
        if rule == 2:
            name = tab["gases"][ig]
            qg = c[name] if name == "h2o" else c[name] * (MOLAR_MASS.get(name, M_DRY) / M_DRY)
            amounts.append(qg * dp / G)
        else:
            amounts.append(1.0 * dp / G if ig == 0 else np.zeros((nlay, ncol)))
    log_cont = None
    if "continuum_kappa" in tab and np.asarray(tab["continuum_kappa"]).ndim == 4 and k.ndim >= 6:
        cont = tab["continuum_kappa"]      # rank 7: the reference takes the log in float64; rank 6: in the file's own type
        log_cont = np.log(np.maximum(np.asarray(cont, dtype=np.float64), 1e-40)) if k.ndim == 7 else np.log(np.maximum(cont, 1e-40))
    w, pf = tab["gpoint_weights"], tab["planck_fraction"]
    iS, fS = bracket(t_grid, c["tsfc"])
    planck, planck_s = SIGMA_SB * t ** 4, SIGMA_SB * c["tsfc"] ** 4
    D = diffusivity
    up_band, dn_band = np.zeros((nband, nlay + 1, ncol)), np.zeros((nband, nlay + 1, ncol))
    tau_band = np.zeros((nband, nlay, ncol))
    for b in range(nband):
        contv = np.exp(_txx(log_cont[b], iT, fT, iP, fP, iX, fX)) if log_cont is not None else None
        for g in range(ngpt):
            tau = np.zeros((nlay, ncol))
            for ig in range(ngas):
                if k.ndim == 7:
                    c0 = _txx(k[ig, b, g], iT, fT, iP, fP, iX, fX, iC)
                    c1 = _txx(k[ig, b, g], iT, fT, iP, fP, iX, fX, iC + 1)
                    kv = np.exp(np.log(np.maximum(c0, 1e-40)) * (1.0 - fC) + np.log(np.maximum(c1, 1e-40)) * fC)
                elif k.ndim == 6:
                    kv = _txx(k[ig, b, g], iT, fT, iP, fP, iX, fX)
                else:
                    kv = _tp(k[ig, b, g], iT, fT, iP, fP)
                tau += kv * amounts[ig]
            if contv is not None:
                tau += contv * amounts[0]
            if probe is not None:
                probe["tau_min"], probe["tau_max"] = min(probe.get("tau_min", np.inf), float(tau.min())), max(probe.get("tau_max", 0.0), float(tau.max()))
            tau = tau + c["taucld"][:, :, b]
            src = (pf[b, g][iT].astype(np.float64) * (1.0 - fT) + pf[b, g][iT + 1].astype(np.float64) * fT) * planck
            wg = np.float64(w[b, g])
            cur = c["emis"][b] * ((pf[b, g][iS].astype(np.float64) * (1.0 - fS) + pf[b, g][iS + 1].astype(np.float64) * fS) * planck_s)
            up_band[b, 0] += wg * cur
            trans = np.exp(-D * tau)
            for j in range(nlay):
                cur = cur * trans[j] + src[j] * (1.0 - trans[j])
                up_band[b, j + 1] += wg * cur
            cur = np.zeros(ncol)
            for j in range(nlay - 1, -1, -1):
                cur = cur * trans[j] + src[j] * (1.0 - trans[j])
                dn_band[b, j] += wg * cur
            tau_band[b] += wg * tau
    up, dn = np.zeros((nlay + 1, ncol)), np.zeros((nlay + 1, ncol))
    for b in range(nband):
        up += up_band[b]
        dn += dn_band[b]
    tend = heating(up - dn, p_int)
    hr_band = np.stack([heating(up_band[b] - dn_band[b], p_int) * 86400.0 for b in range(nband)])
    return dict(up=up, dn=dn, tend=tend, hr=tend * 86400.0, up_band=up_band, dn_band=dn_band, tau_band=tau_band, trans_band=np.exp(-D * tau_band), hr_band=hr_band)


# ---- the cases ----------------------------------------------------------------------------------------------------------------------
def pressures(nlay, ncol):
    """-> p_int [nlay+1][ncol] in Pa: from 30 levels a sigma^1.5 grid up to 20 hPa; with fewer levels layers of 60 hPa."""
    base = 1.0e5 + 37.0 * np.arange(ncol)
    if nlay >= 30:
        sigma = (1.0 - np.arange(nlay + 1) / float(nlay)) ** 1.5
        return 2000.0 + sigma[:, None] * (base[None, :] - 2000.0)
    return base[None, :] - 6000.0 * np.arange(nlay + 1)[:, None]


def _spread(shape, lo, hi, phase, log=False):
    """Values over lo .. hi by a golden-ratio sequence over the flattened grid, offset by `phase`; with at least 8 points the two at
    flat positions 2 phase and 2 phase + 1 are lo and hi themselves."""
    n = int(np.prod(shape))
    u = np.mod((np.arange(n) + 1) * 0.6180339887498949 + 0.137 * phase, 1.0)
    if n >= 8:
        u[(2 * phase) % n], u[(2 * phase + 1) % n] = 0.0, 1.0
    v = np.exp(np.log(lo) + u * (np.log(hi) - np.log(lo))) if log else lo + u * (hi - lo)
    if n >= 8:
        v[(2 * phase) % n], v[(2 * phase + 1) % n] = lo, hi
    return v.reshape(shape)


def _on_node(node):
    """-> p with np.log(p) == node exactly (node >= 0)."""
    p = np.exp(np.float64(node))
    for _ in range(200):
        got = np.log(p)
        if got == node:
            return p
        p = np.nextafter(p, np.inf if got < node else -np.inf)
    raise AssertionError("no pressure whose log is the node %r" % node)


def _inputs(name, nlay, ncol):
    tab = table(CASES[name][0])
    nband = tab["k_coefficients"].shape[1]
    shape = (nlay, ncol)
    t_grid, p_grid = np.asarray(tab["temperature_grid"], dtype=np.float64), np.asarray(tab["pressure_grid_log"], dtype=np.float64)
    p_int = pressures(nlay, ncol)
    colv = np.arange(ncol)
    spans = name in SPANS
    if spans:      # past both ends of every axis
        t = _spread(shape, t_grid[0] - 12.0, t_grid[-1] + 12.0, 0)
        p = _spread(shape, 0.3 * np.exp(p_grid[0]), 3.0 * np.exp(p_grid[-1]), 1, log=True)
    elif name == "on_nodes":
        lev = np.arange(nlay)[:, None]
        t = t_grid[(lev + colv[None, :]) % t_grid.size]
        nodes = np.array([_on_node(x) for x in p_grid])
        p = nodes[(lev + 3 * colv[None, :]) % p_grid.size]
    else:      # an atmosphere: within the grids
        p = 0.5 * (p_int[:-1] + p_int[1:])
        t = 212.0 + 80.0 * (p / p_int[0]) ** 1.3 + 0.013 * colv[None, :] + 1.5 * np.sin(0.7 * np.arange(nlay)[:, None] + 0.3 * colv[None, :])
    c = dict(t=t, p=p, p_int=p_int, tsfc=(t[0] + 2.0 + 0.01 * (colv % 9)) * np.ones(ncol), emis=np.ones((nband, ncol)), taucld=np.zeros((nlay, ncol, nband)))
    for ig, gas in enumerate(tab["gases"]):
        if gas == "h2o" and tab["rule"] == 1:
            x_grid = np.asarray(tab["h2o_vmr_grid"], dtype=np.float64)
            c["h2o"] = _spread(shape, 0.05 * x_grid[0], 1.05, 2, log=True) if spans else _spread(shape, 2.0e-6, 0.03, 2, log=True)
        elif gas == "co2" and tab["rule"] == 1:
            c_grid = np.asarray(tab["co2_vmr_grid"], dtype=np.float64)
            c["co2"] = _spread(shape, 0.2 * c_grid[0], 2.0 * c_grid[-1], 3, log=True) if spans else _spread(shape, 2.0e-4, 1.0e-3, 3, log=True)
        elif gas == "h2o":
            c["h2o"] = _spread(shape, 1.0e-3, 0.02, 2, log=True)      # (no column so thin that its downward flux is rounding noise of the source)
        else:      # (the eight gases of g4_gases8: a phase each, none of them the water vapour's)
            c[gas] = _spread(shape, 2.0e-4, 8.0e-4, 3 + ig if len(tab["gases"]) > 2 else 3, log=True)
    if name in ("cloudy", "bands32_cloudy"):      # cloud in the layers k with (k + column) % 3 == 0, the depth by band; 1e3 in the lowest layer of band 0
        lev = np.arange(nlay)[:, None, None]
        cloud = ((lev + colv[None, :, None]) % 3 == 0) * (0.2 + 0.7 * np.arange(nband)[None, None, :] + 0.01 * (colv[None, :, None] % 5))
        cloud[0, :, 0] = 1.0e3
        c["taucld"] = cloud * np.ones((nlay, ncol, nband))
    if name in ("emissivity", "bands32_cloudy"):      # band 0 black, band 1 a mirror, the others in between and varying by column
        e = 0.5 + 0.45 * np.sin(0.37 * colv[None, :] + np.arange(nband)[:, None]) * np.ones((nband, ncol))
        e[0], e[1 % nband] = 1.0, 0.0
        c["emis"] = e
    return {k: np.ascontiguousarray(x, dtype=np.float64) for k, x in c.items()}


def check_case(name, c, probe=None):
    """Asserts that a case does what its name says (c: inputs and the statement's outputs; probe: what the statement left in it)."""
    tab = table(CASES[name][0])
    nlay, ncol = c["t"].shape
    for f in FIELDS:
        assert np.isfinite(c[f]).all(), (name, f)
    assert same_bits(c["dn_band"][:, -1], np.zeros_like(c["dn_band"][:, -1]))
    k = tab["k_coefficients"]
    big = nlay * ncol >= 60
    if name in ("earth", "earth_d2") and big:      # all eight clamps fire, and interior points exist
        q = c["h2o"]
        x = q / np.maximum(q + (1.0 - q) * M_H2O, 1e-30)
        axes = ((c["t"], np.asarray(tab["temperature_grid"], dtype=np.float64)), (np.log(np.maximum(c["p"], 1.0)), np.asarray(tab["pressure_grid_log"], dtype=np.float64)),
                (x, np.asarray(tab["h2o_vmr_grid"], dtype=np.float64)), (c["co2"], np.asarray(tab["co2_vmr_grid"], dtype=np.float64)))
        assert k.ndim == 7
        for v, grid in axes:
            assert (v <= grid[0]).any() and (v >= grid[-1]).any() and ((v > grid[0]) & (v < grid[-1])).any(), name
        assert (c["p"] < 1.0).any()      # below the floor of log(max(p, 1))
    if name == "earth_d2":
        assert CASES[name][1] == 2.0 and not same_bits(c["up"], cork_case("earth", nlay, ncol)["up"])
    if name == "on_nodes" and big:
        t_grid, p_grid = np.asarray(tab["temperature_grid"], dtype=np.float64), np.asarray(tab["pressure_grid_log"], dtype=np.float64)
        assert np.isin(c["t"], t_grid).all() and np.isin(np.log(np.maximum(c["p"], 1.0)), p_grid).all()
        for v, grid in ((c["t"], t_grid), (np.log(np.maximum(c["p"], 1.0)), p_grid)):
            assert (v == grid[0]).any() and (v == grid[-1]).any()
            i, f = bracket(grid, v)
            assert ((f == 0.0) | (f == 1.0)).all() and (np.searchsorted(grid, v) - 1 == -1).any()
    if name == "h2o_axis":
        assert k.ndim == 6 and "continuum_kappa" in tab and tab["rule"] == 1
    if name == "two_band":
        assert k.ndim == 5 and tab["rule"] == 2 and tab["gases"] == ["h2o"] and k.dtype == np.float64
    if name == "two_gas":
        assert k.ndim == 5 and tab["rule"] == 2 and tab["gases"] == ["h2o", "co2"] and k.shape[0] == 2
    if name == "premixed":
        assert k.ndim == 5 and tab["rule"] == 0 and tab["gases"] == []
    if name in SHAPE_CASES:
        gases, nband, ngpt, nT, nP, nX, nC, cont = SHAPE_TABLES[CASES[name][0]]
        assert k.shape == (len(gases), nband, ngpt, nT, nP) + (nX,) * (nX > 0) + (nC,) * (nC > 0) and ("continuum_kappa" in tab) == cont
        assert [str(g) for g in tab["gas_names"]] == list(gases) and tab["rule"] == (2 if gases[0] != "effective" else 1 if nX else 0)
        assert all(tab[a].dtype == np.float32 for a in tab if isinstance(tab[a], np.ndarray) and tab[a].dtype.kind == "f")
        assert same_bits(tab["gpoint_weights"].astype(np.float64).sum(axis=1), np.ones(nband))      # (multiples of 2^-10: the sum is exact)
        axes = [(c["t"], tab["temperature_grid"]), (np.log(np.maximum(c["p"], 1.0)), tab["pressure_grid_log"])]
        if nX:
            axes.append((c["h2o"] / np.maximum(c["h2o"] + (1.0 - c["h2o"]) * M_H2O, 1e-30), tab["h2o_vmr_grid"]))
        if nC:
            axes.append((c["co2"], tab["co2_vmr_grid"]))
        for i, (v, grid) in enumerate(axes):
            grid = np.asarray(grid, dtype=np.float64)
            steps = np.diff(np.log(grid) if i >= 2 else grid)      # (in the coordinate the axis is bracketed in)
            assert grid.size == 2 or steps.max() > 1.5 * steps.min()      # far from uniform
            if name in SPANS and big:      # every clamp fires, and interior points exist
                assert (v <= grid[0]).any() and (v >= grid[-1]).any() and ((v > grid[0]) & (v < grid[-1])).any(), name
            if name not in SPANS:
                assert ((v > grid[0]) & (v < grid[-1])).all(), name
        if name not in SPANS and nlay == 30:
            # on the 30 layers the reference ran: the gas optical depth of a layer spans 1e-3 .. 1e2 over the g-points, each end to within half a decade: lanes that
            # are nearly transparent and lanes that are opaque in one layer (one g-point: what the layers span, inside that range)
            lo, hi = probe["tau_min"], probe["tau_max"]
            assert (10 ** -3.5 <= lo <= 10 ** -2.5 and 10 ** 1.5 <= hi <= 10 ** 2.5) if ngpt > 1 else (1e-3 <= lo and hi <= 1e2 and hi >= 30.0 * lo), (name, lo, hi)
    if name in ("cloudy", "bands32_cloudy"):
        cloud = c["taucld"]
        assert (cloud > 0).any() and ((cloud == 0).any() or nlay * ncol < 6) and (cloud[0, :, 0] == 1.0e3).all()
        D = CASES[name][1]
        assert not np.exp(-D * 1.0e3)      # the transmittance underflows: the layer's flux is its source
        assert same_bits(c["trans_band"][0, 0], np.zeros(ncol))
    if name == "emissivity":
        assert (c["emis"][0] == 1.0).all() and (c["emis"][1 % c["emis"].shape[0]] == 0.0).all()
        if c["emis"].shape[0] > 1:
            assert same_bits(c["up_band"][1, 0], np.zeros(ncol))      # a mirror emits nothing


@functools.lru_cache(maxsize=None)
def cork_case(name, nlay, ncol):
    """-> dict(the inputs; the statement's outputs).  Shared and read-only."""
    c, probe = _inputs(name, nlay, ncol), {}
    c.update(statement(table(CASES[name][0]), c, CASES[name][1], probe=probe))
    check_case(name, c, probe)
    for x in c.values():
        x.setflags(write=False)
    return c


def gas_names(name):
    return list(table(CASES[name][0])["gases"])


# ---- comparing ----------------------------------------------------------------------------------------------------------------------
def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def deviations(got, c, fields=FIELDS):
    """got: dict with `fields` (one may be absent or None) -> {name: largest deviation over the columns (and bands)}, each
    relative to the column's largest magnitude of the field in `c` (over the levels and, for a per-band field, the bands: a
    band in which a column is nearly transparent is measured against the column's strong bands, not against its own rounding
    noise), absolute where that is zero."""
    dev = {}
    for name in fields:
        if got.get(name) is None:
            continue
        want = np.asarray(c[name])
        scale = np.abs(want).max(axis=tuple(range(want.ndim - 1)), keepdims=True)      # over the levels and, per-band fields, the bands
        diff = np.abs(np.asarray(got[name]).reshape(want.shape) - want)
        with np.errstate(invalid="ignore"):
            dev[name] = float(np.max(diff / np.where(scale > 0, scale, 1.0)))
    return dev


@functools.lru_cache(maxsize=None)
def tolerances(name):
    """{field: tol} of tests/golden/cork_<name>.npz: measured by the maker on the reference (16 x the largest deviation under +-1
    ulp of every input, at least 1e-13), on the scale of `deviations`."""
    z = np.load(os.path.join(GOLDEN, "cork_%s.npz" % name))
    return {f[4:]: float(z[f]) for f in z.files if f.startswith("tol_")}


def within(dev, tol):
    return all(v <= tol[k] for k, v in dev.items())
