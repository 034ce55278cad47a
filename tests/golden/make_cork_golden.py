"""Golden fixtures of the table-driven correlated-k longwave, from the reference's own code and tables.  Run by hand where a
checkout of the reference is at $CLIMT_REFERENCE (never by the tests, which read what this wrote):

    CLIMT_REFERENCE=<checkout> python tests/golden/make_cork_golden.py [shapes]

With `shapes` only the shape family is written (1b and its cases; cork_interface.json is written whole, for every table on disk):
the files of the other family stay what they are.

1. cork_table_<name>.npz -- data derived from the reference's shipped tables (climt/_data/cork/correlated_k): `earth4` the bands
   0, 5, 9, 13 of earth_low_res_lw.npz with every other axis whole (rank 7, continuum, float32); `h2o_axis` the same at CO2 node 5
   (rank 6); `two_band` test_2band_lw.npz as shipped (rank 5, float64, gas h2o); `two_gas` the same with a second gas "co2" whose k
   is 0.37 of the first's; `premixed` the same with gas_names ["effective"].
1b. the shape tables (cork_cases.SHAPE_TABLES: the sizes; here: the values) -- no data of the reference's, a formula: k = k_lo
   (k_hi / k_lo)^(u (1 - 0.04 gas)) with u = g / (ngpt - 1) (one g-point: 0.5), times a factor by gas (1 + 0.37 gas) and band (1 + 0.45 sin(0.9 band + 0.4 gas)), (T / 250)^(1.2 + 0.5 u + 0.03 band), exp((0.35 - 0.2 u) (log p - 10)),
   1 + 4 (1 + u) sqrt(X), (C / 4e-4)^(0.3 + 0.2 u): smooth, positive, another slope along every axis for every g-point, band and
   gas.  k_lo .. k_hi is 1e-2 .. 3 m^2/kg for a table by gas (from 3e-2 with two gases, from 4e-3 with eight) and 4e-5 .. 0.04 for one of air, which puts the optical depth of a
   layer of the cases' atmosphere at 1e-3 .. 1e2 over the g-points (cork_cases.check_case asserts it).  Weights: multiples of 2^-10
   that sum to 1 exactly, another set per band.  Planck fraction: the weight times a band share that moves to higher bands with T (a
   Gaussian in the band index, normalised over the bands) times a tilt over the g-points that grows with T - 250 and keeps the
   band's sum.  Continuum (g16_cont): 0.05 X^1.5 (1 + 0.3 band) (260 / T)^2 exp(0.2 (log p - 10)).  Grids: the steps of node i
   scaled by i + 0.35 sin(2.1 i), far from uniform; T 140 .. 350 K, log p of 1e3 .. 1.2e5 Pa, X 1e-6 .. 0.1 and CO2
   1e-4 .. 2e-3 spaced so in log.  Every array is rounded to float32 and stored as float32: the file is run as a float table and, k
   cast, as a double table, to the same bits.  The reference took every one of these shapes -- rank 6 and rank 7 without a continuum,
   eight gases of which two have no molar mass, 32 bands, two-node axes, float32 throughout -- without a complaint.
2. cork_<case>.npz -- cork/common.py, optics/correlated_k.py, lw/kernels.py and lw/component.py loaded WHERE THEY LIE and executed
   under plain numpy on the inputs of tests/cork_cases.py at 2, 30 and 61 layers x 4 columns (the shape family: 2 and 30): stub modules stand in for `sympl`
   (TendencyComponent is `object`, get_constant returns the constants of the cases), `numba` (njit the identity),
   `importlib_resources`, the reference's backend (prange = range), its initialization (set_num_longwave_bands does nothing) and
   the Parmentier optics (never called).  CorkLongwaveRadiation.array_call is called with the arrays under the aliases sympl would
   hand it.  Only data is written: the inputs, the reference's outputs and the tolerances.
   Tolerances: the reference is run RUNS = 16 times per shape with every input moved by a random +-1 ulp (an exact 0 stays 0);
   every interpolation is continuous across a bracket flip, so no run is discarded; tol_<field> = max(16 x the largest deviation
   from the unmoved run, 1e-13) on the scale of cork_cases.deviations, moved_<field> the deviation.
3. cork_interface.json -- the keyword defaults of CorkLongwaveRadiation.__init__ read off the reference's source with `ast`, and,
   for every fixture table, the three property dictionaries and num_longwave_bands the reference's class states for it.
"""
import ast
import importlib.util
import json
import multiprocessing
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import cork_cases as X  # noqa: E402

REF = os.environ["CLIMT_REFERENCE"]
SHAPES = ((2, 4), (30, 4), (61, 4))
SHAPE_FAMILY_SHAPES = ((2, 4), (30, 4))
RUNS = 16
CORK = os.path.join(REF, "climt", "_components", "cork")
SHIPPED = os.path.join(REF, "climt", "_data", "cork", "correlated_k")
CONSTANTS = {"stefan_boltzmann_constant": X.SIGMA_SB, "gravitational_acceleration": X.G, "heat_capacity_of_dry_air_at_constant_pressure": X.CPD}
OUT = {"up": "upwelling_longwave_flux_in_air", "dn": "downwelling_longwave_flux_in_air", "hr": "air_temperature_tendency_from_longwave",
       "up_band": "upwelling_longwave_flux_in_air_per_band", "dn_band": "downwelling_longwave_flux_in_air_per_band", "tau_band": "longwave_optical_depth_per_band",
       "trans_band": "longwave_transmittance_per_band", "hr_band": "air_temperature_tendency_from_longwave_per_band"}


def tables():
    with np.load(os.path.join(SHIPPED, "earth_low_res_lw.npz"), allow_pickle=True) as z:
        earth = {k: z[k] for k in z.files}
    with np.load(os.path.join(SHIPPED, "test_2band_lw.npz"), allow_pickle=True) as z:
        two = {k: z[k] for k in z.files}
    bands = [0, 5, 9, 13]
    e4 = dict(earth)
    e4["k_coefficients"] = earth["k_coefficients"][:, bands]
    for k in ("gpoint_weights", "planck_fraction", "continuum_kappa", "band_wavenumber_limits"):
        e4[k] = earth[k][bands]
    hx = dict(e4)
    hx["k_coefficients"] = e4["k_coefficients"][..., 5]
    del hx["co2_vmr_grid"]
    tg = dict(two)
    tg["k_coefficients"] = np.concatenate([two["k_coefficients"], 0.37 * two["k_coefficients"]], axis=0)
    tg["gas_names"] = np.array(["h2o", "co2"])
    pm = dict(two)
    pm["gas_names"] = np.array(["effective"])
    assert X.BASE_TABLES == ("earth4", "h2o_axis", "two_band", "two_gas", "premixed")
    for name, t in (("earth4", e4), ("h2o_axis", hx), ("two_band", two), ("two_gas", tg), ("premixed", pm)):
        np.savez_compressed(X.table_path(name), **{k: np.ascontiguousarray(v) for k, v in t.items()})
        print("table %-9s %7d bytes  k %s %s" % (name, os.path.getsize(X.table_path(name)), t["k_coefficients"].dtype, t["k_coefficients"].shape))


def _grid(lo, hi, n):
    """n nodes from lo to hi, the steps uneven."""
    i = np.arange(n)
    u = (i + 0.35 * np.sin(2.1 * i)) / (n - 1.0)
    u[0], u[-1] = 0.0, 1.0
    return lo + (hi - lo) * u


def shape_tables():
    for name, (gases, nband, ngpt, nT, nP, nX, nC, cont) in X.SHAPE_TABLES.items():
        ngas = len(gases)
        k_lo, k_hi = (4e-5, 0.04) if gases[0] == "effective" else (3e-2, 3.0) if ngas == 2 else (4e-3, 3.0) if ngas == 8 else (1e-2, 3.0)
        f32 = lambda a: np.ascontiguousarray(np.asarray(a, dtype=np.float64).astype(np.float32))
        t = {"temperature_grid": f32(_grid(140.0, 350.0, nT)), "pressure_grid_log": f32(_grid(np.log(1.0e3), np.log(1.2e5), nP)), "gas_names": np.array(list(gases))}
        if nX:
            t["h2o_vmr_grid"] = f32(np.exp(_grid(np.log(1e-6), np.log(0.1), nX)))
        if nC:
            t["co2_vmr_grid"] = f32(np.exp(_grid(np.log(1e-4), np.log(2e-3), nC)))
        ax = lambda a, pos: np.asarray(a, dtype=np.float64).reshape([-1 if i == pos else 1 for i in range(7)])
        ig, b, u = ax(np.arange(ngas), 0), ax(np.arange(nband), 1), ax(np.arange(ngpt) / (ngpt - 1.0) if ngpt > 1 else [0.5], 2)
        T, lp = ax(t["temperature_grid"], 3), ax(t["pressure_grid_log"], 4)
        x, cc = ax(t["h2o_vmr_grid"] if nX else [0.0], 5), ax(t["co2_vmr_grid"] if nC else [4e-4], 6)
        k = (k_lo * (k_hi / k_lo) ** (u * (1.0 - 0.04 * ig)) * (1.0 + 0.37 * ig) * (1.0 + 0.45 * np.sin(0.9 * b + 0.4 * ig))
             * (T / 250.0) ** (1.2 + 0.5 * u + 0.03 * b) * np.exp((0.35 - 0.2 * u) * (lp - 10.0)) * (1.0 + 4.0 * (1.0 + u) * np.sqrt(x)) * (cc / 4e-4) ** (0.3 + 0.2 * u))
        t["k_coefficients"] = f32(k.reshape(k.shape[:5] + (nX,) * (nX > 0) + (nC,) * (nC > 0)))
        raw = 1.0 + 0.6 * np.sin(1.3 * np.arange(ngpt)[None, :] + 0.7 * np.arange(nband)[:, None]) + 0.1 * np.arange(ngpt)[None, :]
        w = np.round(raw / raw.sum(axis=1, keepdims=True) * 1024.0) / 1024.0
        w[:, -1] += 1.0 - w.sum(axis=1)
        assert (w > 0).all() and (w.sum(axis=1) == 1.0).all() and (w * 1024.0 == np.round(w * 1024.0)).all()
        t["gpoint_weights"] = f32(w)
        Tg = np.asarray(t["temperature_grid"], dtype=np.float64)
        share = np.exp(-0.5 * ((np.arange(nband)[:, None] - (nband - 1.0) * (Tg[None, :] - 150.0) / 250.0) / (nband / 3.0 + 0.5)) ** 2)
        share /= share.sum(axis=0, keepdims=True)
        ug = np.arange(ngpt) / float(ngpt)
        tilt = 1.0 + 0.3 * (ug[None, :, None] - (w * ug[None, :]).sum(axis=1)[:, None, None]) * (Tg[None, None, :] - 250.0) / 250.0
        t["planck_fraction"] = f32(w[:, :, None] * share[:, None, :] * tilt)
        assert (t["planck_fraction"] > 0).all() and np.abs(t["planck_fraction"].astype(np.float64).sum(axis=(0, 1)) - 1.0).max() < 1e-6
        if cont:
            bb, TT, pp, xx = (np.asarray(a, dtype=np.float64).reshape([-1 if i == pos else 1 for i in range(4)])
                              for pos, a in enumerate((np.arange(nband), t["temperature_grid"], t["pressure_grid_log"], t["h2o_vmr_grid"])))
            t["continuum_kappa"] = f32(0.05 * xx ** 1.5 * (1.0 + 0.3 * bb) * (260.0 / TT) ** 2 * np.exp(0.2 * (pp - 10.0)))
        assert (t["k_coefficients"] > 0).all() and all(np.all(np.diff(t[g].astype(np.float64)) > 0) for g in t if g.endswith("_grid") or g.endswith("_log"))
        np.savez_compressed(X.table_path(name), **t)
        assert os.path.getsize(X.table_path(name)) < 200 * 1024
        print("table %-9s %7d bytes  k %s %s" % (name, os.path.getsize(X.table_path(name)), t["k_coefficients"].dtype, t["k_coefficients"].shape))


def reference():
    """-> the reference's CorkLongwaveRadiation class, loaded under the stubs."""
    def module(name, **members):
        m = sys.modules[name] = types.ModuleType(name)
        m.__path__ = []
        for k, v in members.items():
            setattr(m, k, v)
        return m
    module("sympl", TendencyComponent=object, get_constant=lambda name, units: CONSTANTS[name])
    module("numba", njit=lambda f=None, **kw: f if f is not None else (lambda g: g))
    module("importlib_resources")
    for pkg in ("climt", "climt._core", "climt._components", "climt._components.cork", "climt._components.cork.optics", "climt._components.cork.lw"):
        module(pkg)
    module("climt._core.backend", prange=range)
    module("climt._core.initialization", set_num_longwave_bands=lambda n: None)
    never = lambda *a, **k: (_ for _ in ()).throw(AssertionError("the Parmentier optics are not part of this"))
    module("climt._components.cork.optics.parmentier", compute_rosseland_mean_opacity=never, compute_thermal_opacities=never,
           load_freedman2014_coefficients=never, load_parmentier_coefficients=never, lookup_ratio_coefficients=never)
    mod = None
    for name, rel in (("common", "common.py"), ("optics.correlated_k", "optics/correlated_k.py"), ("lw.kernels", "lw/kernels.py"), ("lw.component", "lw/component.py")):
        full = "climt._components.cork." + name
        spec = importlib.util.spec_from_file_location(full, os.path.join(CORK, rel))
        mod = sys.modules[full] = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
    return mod.CorkLongwaveRadiation


def runner(cls, name):
    tab, D = X.CASES[name]
    comp = cls(optics="correlated_k", table=X.table_path(tab), diffusivity_factor=D)

    def run(c):
        state = {"T": np.array(c["t"]), "p": np.array(c["p"]), "p_int": np.array(c["p_int"]), "T_surf": np.array(c["tsfc"]), "emissivity": np.array(c["emis"]),
                 "tau_cloud_lw": np.array(c["taucld"])}
        state.update({g: np.array(c[g]) for g in X.gas_names(name)})
        tend, d = comp.array_call(state)
        out = {f: (np.moveaxis(d[n], -1, 0) if f.endswith("_band") else d[n]) for f, n in OUT.items()}
        return dict(out, tend=tend["T"])
    return run


def moved(c, names, rng):
    """Every input by a random +-1 ulp; an exact 0 stays 0."""
    out = {}
    for n in names:
        a = np.array(c[n])
        b = np.nextafter(a, np.where(rng.randint(0, 2, a.shape) == 1, np.inf, -np.inf))
        out[n] = np.where(a == 0.0, a, b)
    return out


def case(name):
    run = runner(reference(), name)
    names = X.INPUTS + tuple(X.gas_names(name))
    stored, worst, lines = {}, {}, []
    rng = np.random.RandomState(sum(map(ord, "cork" + name)))
    shapes = SHAPE_FAMILY_SHAPES if name in X.SHAPE_CASES else SHAPES
    for nlay, ncol in shapes:
        c = X.cork_case(name, nlay, ncol)
        ref = run(c)
        for _ in range(RUNS):
            for f, dev in X.deviations(run(moved(c, names, rng)), ref).items():
                worst[f] = max(worst.get(f, 0.0), dev)
        stored.update({"n%d_%s" % (nlay, k): c[k] for k in names})
        stored.update({"n%d_ref_%s" % (nlay, k): v for k, v in ref.items()})
        lines.append("cork %-10s nlay %2d  statement against the reference: largest deviation %.2e, bits equal %s" % (
            name, nlay, max(X.deviations(c, ref).values()), sorted(k for k in ref if X.same_bits(ref[k], c[k]))))
    tol = {f: max(16.0 * v, 1e-13) for f, v in worst.items()}
    np.savez_compressed(os.path.join(HERE, "cork_%s.npz" % name), nlays=np.array([s[0] for s in shapes], dtype=np.int32), constants=np.array([X.SIGMA_SB, X.G, X.CPD]),
                        diffusivity=np.float64(X.CASES[name][1]), **{"tol_" + f: np.float64(v) for f, v in tol.items()},
                        **{"moved_" + f: np.float64(v) for f, v in worst.items()}, **stored)
    lines.append("cork %-10s moved inputs: %s" % (name, ", ".join("%s %.1e" % (f, worst[f]) for f in sorted(tol))))
    return "\n".join(lines)


def interface():
    src = os.path.join(CORK, "lw", "component.py")
    node = next(n for n in ast.parse(open(src).read()).body if isinstance(n, ast.ClassDef) and n.name == "CorkLongwaveRadiation")
    init = next(i for i in node.body if isinstance(i, ast.FunctionDef) and i.name == "__init__")
    kernels = ast.parse(open(os.path.join(CORK, "lw", "kernels.py")).read())
    named = {n.targets[0].id: ast.literal_eval(n.value) for n in kernels.body if isinstance(n, ast.Assign) and isinstance(n.value, ast.Constant)}
    args = [a.arg for a in init.args.args[1:]]
    defaults = [named[d.id] if isinstance(d, ast.Name) else ast.literal_eval(d) for d in init.args.defaults]
    out = {"base": node.bases[0].id, "init": dict(zip(args[len(args) - len(defaults):], defaults)), "init_order": args, "class_diffusivity_factor": named["DIFFUSIVITY_FACTOR"],
           "tables": {}}
    cls = reference()
    for name in X.TABLES:
        comp = cls(optics="correlated_k", table=X.table_path(name))
        out["tables"][name] = {"input_properties": comp.input_properties, "tendency_properties": comp.tendency_properties,
                               "diagnostic_properties": comp.diagnostic_properties, "num_longwave_bands": int(comp.num_longwave_bands)}
    with open(os.path.join(HERE, "cork_interface.json"), "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    only_shapes = sys.argv[1:] == ["shapes"]
    assert only_shapes or not sys.argv[1:], "usage: make_cork_golden.py [shapes]"
    if not only_shapes:
        tables()
    shape_tables()
    interface()
    cases = list(X.SHAPE_CASES if only_shapes else X.CASES)
    with multiprocessing.Pool(min(len(cases), os.cpu_count() or 1)) as pool:
        for text in pool.imap(case, cases):
            print(text, flush=True)
