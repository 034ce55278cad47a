"""Golden fixtures of the table-driven correlated-k longwave, from the reference's own code and tables.  Run by hand where a
checkout of the reference is at $CLIMT_REFERENCE (never by the tests, which read what this wrote):

    CLIMT_REFERENCE=<checkout> python tests/golden/make_cork_golden.py

1. cork_table_<name>.npz -- data derived from the reference's shipped tables (climt/_data/cork/correlated_k): `earth4` the bands
   0, 5, 9, 13 of earth_low_res_lw.npz with every other axis whole (rank 7, continuum, float32); `h2o_axis` the same at CO2 node 5
   (rank 6); `two_band` test_2band_lw.npz as shipped (rank 5, float64, gas h2o); `two_gas` the same with a second gas "co2" whose k
   is 0.37 of the first's; `premixed` the same with gas_names ["effective"].
2. cork_<case>.npz -- cork/common.py, optics/correlated_k.py, lw/kernels.py and lw/component.py loaded WHERE THEY LIE and executed
   under plain numpy on the inputs of tests/cork_cases.py at 2, 30 and 61 layers x 4 columns: stub modules stand in for `sympl`
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
    for name, t in (("earth4", e4), ("h2o_axis", hx), ("two_band", two), ("two_gas", tg), ("premixed", pm)):
        np.savez_compressed(X.table_path(name), **{k: np.ascontiguousarray(v) for k, v in t.items()})
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
    for nlay, ncol in SHAPES:
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
    np.savez_compressed(os.path.join(HERE, "cork_%s.npz" % name), nlays=np.array([s[0] for s in SHAPES], dtype=np.int32), constants=np.array([X.SIGMA_SB, X.G, X.CPD]),
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
    tables()
    interface()
    with multiprocessing.Pool(min(len(X.CASES), os.cpu_count() or 1)) as pool:
        for text in pool.imap(case, list(X.CASES)):
            print(text, flush=True)
