"""Golden fixtures of the gray radiation path, from the reference's own code.  Run by hand where a checkout of the reference is at
$CLIMT_REFERENCE (never by the tests, which read what this wrote):

    CLIMT_REFERENCE=<checkout> python tests/golden/make_gray_golden.py

1. gray_<case>.npz, gsc_<case>.npz -- climt/_components/radiation.py and grid_scale_condensation.py loaded WHERE THEY LIE and
   executed under plain numpy on the inputs of tests/gray_cases.py at 2, 30 and 61 layers x 4 columns: stub modules stand in for
   `sympl` (the component base classes are `object`, get_constant returns the constants of the cases), for `numba` (njit the
   identity) and for the reference's backend (prange = range).  The reference's GrayLongwaveRadiation.array_call is called with
   the arrays under the aliases sympl would hand it, so the fluxes are `_gray_lw_kernel_np`'s and the tendency and the heating
   rate are the reference's own lines; Frierson06LongwaveOpticalDepth.array_call (`_frierson_tau_kernel_np`) gives `ref_depth`
   for the case's pressures and latitudes; GridScaleCondensation.array_call gives `_gsc_kernel_np`'s profiles and precipitation.
   Only data is written: the inputs, the reference's outputs, the margin of the condensation cases and the tolerances.
   Tolerances: the reference is run RUNS = 16 times per shape with every input moved by a random +-1 ulp (an exact 0 stays 0), and
   only runs with the same decisions (the condensation's saturated layers, by the statement) are kept; tol_<field> =
   max(16 x the largest deviation from the unmoved run, 1e-13) on the scale of gray_cases.deviations, moved_<field> the deviation.
2. gray_interface.json -- the property dictionaries and the keyword defaults of the three classes, read off the reference's source
   with `ast` (nothing is executed for this): names, dims, units, aliases and numbers only.
"""
import ast
import importlib.util
import json
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import gray_cases as X  # noqa: E402

REF = os.environ["CLIMT_REFERENCE"]
SHAPES = ((2, 4), (30, 4), (61, 4))
RUNS = 16
SOURCES = {"radiation": os.path.join(REF, "climt", "_components", "radiation.py"),
           "grid_scale_condensation": os.path.join(REF, "climt", "_components", "grid_scale_condensation.py")}
CONSTANTS = {"stefan_boltzmann_constant": X.SIGMA_SB, "gravitational_acceleration": X.G, "heat_capacity_of_dry_air_at_constant_pressure": X.CPD,
             "latent_heat_of_condensation": X.GSC_CONSTANTS["lv"], "gas_constant_of_dry_air": X.GSC_CONSTANTS["rd"],
             "gas_constant_of_vapor_phase": X.GSC_CONSTANTS["rh2o"], "density_of_liquid_phase": X.GSC_CONSTANTS["rhow"]}


def reference():
    """-> (gray(c) -> up, dn, tend, hr; depth(c) -> tau; gsc(c) -> t_new, q_new, precip), each the reference's array_call."""
    def module(name, **members):
        m = sys.modules[name] = types.ModuleType(name)
        m.__path__ = []
        for k, v in members.items():
            setattr(m, k, v)
        return m
    module("sympl", Stepper=object, TendencyComponent=object, DiagnosticComponent=object, get_constant=lambda name, units: CONSTANTS[name])
    module("numba", njit=lambda f=None, **kw: f if f is not None else (lambda g: g))
    for pkg in ("climt", "climt._core", "climt._components"):
        module(pkg)
    module("climt._core.backend", prange=range)
    mods = {}
    for name, path in SOURCES.items():
        spec = importlib.util.spec_from_file_location("climt._components." + name, path)
        mods[name] = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mods[name])
    rad, cond = mods["radiation"].GrayLongwaveRadiation(), mods["grid_scale_condensation"].GridScaleCondensation()
    tau = mods["radiation"].Frierson06LongwaveOpticalDepth()
    assert (tau._tau0e, tau._tau0p, tau._fl) == (X.FRIERSON["tau0e"], X.FRIERSON["tau0p"], X.FRIERSON["fl"])

    def gray(c):
        tend, d = rad.array_call({"sl": np.array(c["t"]), "tau": np.array(c["tau"]), "T_surface": np.array(c["tsfc"]), "p_interface": np.array(c["p_int"])})
        return dict(up=d["lw_up"], dn=d["lw_down"], tend=tend["sl"], hr=d["air_temperature_tendency_from_longwave"])

    def depth(c):
        d = tau.array_call({"air_pressure_on_interface_levels": np.array(c["p_int"]), "surface_air_pressure": np.array(c["ps"]), "latitude": np.array(c["lat"])})
        return dict(depth=d["longwave_optical_depth_on_interface_levels"])

    def gsc(c):
        d, new = cond.array_call({"air_temperature": np.array(c["t"]), "specific_humidity": np.array(c["q"]), "air_pressure": np.array(c["p"]),
                                  "air_pressure_on_interface_levels": np.array(c["p_int"])}, None)
        return dict(t_new=new["air_temperature"], q_new=new["specific_humidity"], precip=d["precipitation_amount"])
    return gray, depth, gsc


def moved(c, names, rng):
    """Every input by a random +-1 ulp; an exact 0 stays 0."""
    out = {}
    for n in names:
        a = np.array(c[n])
        b = np.nextafter(a, np.where(rng.randint(0, 2, a.shape) == 1, np.inf, -np.inf))
        out[n] = np.where(a == 0.0, a, b)
    return out


def measure(run, c, ref, names, fields, rng, worst, same_decisions=lambda m: True):
    kept = tries = 0
    while kept < RUNS:
        tries += 1
        assert tries <= 20 * RUNS, "no robust candidates"
        m = moved(c, names, rng)
        if not same_decisions(m):
            continue
        kept += 1
        for f, dev in X.deviations(run(m), ref, fields).items():
            worst[f] = max(worst.get(f, 0.0), dev)
    return tries


def save(path, stored, worst, **extra):
    tol = {f: max(16.0 * v, 1e-13) for f, v in worst.items()}
    np.savez_compressed(path, nlays=np.array([s[0] for s in SHAPES], dtype=np.int32), **{"tol_" + f: np.float64(v) for f, v in tol.items()},
                        **{"moved_" + f: np.float64(v) for f, v in worst.items()}, **extra, **stored)
    return tol


def cases(gray, depth, gsc):
    for name in X.GRAY_CASES:
        stored, worst = {}, {}
        rng = np.random.RandomState(sum(map(ord, "gray" + name)))
        for nlay, ncol in SHAPES:
            c = X.gray_case(name, nlay, ncol)
            ref = dict(gray(c), **depth(c))
            measure(gray, c, ref, X.GRAY_INPUTS, X.GRAY_FIELDS, rng, worst)
            measure(depth, c, ref, X.GRAY_INPUTS, ("depth",), rng, worst)
            stored.update({"n%d_%s" % (nlay, k): c[k] for k in X.GRAY_INPUTS})
            stored.update({"n%d_ref_%s" % (nlay, k): v for k, v in ref.items()})
            mine = dict(c, depth=X.frierson_statement(c["lat"], c["p_int"], c["ps"]))
            print("gray %-12s nlay %2d  statement against the reference: bits equal %s, largest deviation %.2e" % (
                name, nlay, {k: X.same_bits(ref[k], mine[k]) for k in ref}, max(X.deviations(mine, ref, X.GRAY_FIELDS + ("depth",)).values())))
        worst["tau"] = worst.pop("depth")
        tol = save(os.path.join(HERE, "gray_%s.npz" % name), stored, worst, constants=np.array([X.SIGMA_SB, X.G, X.CPD]),
                   frierson=np.array([X.FRIERSON[k] for k in ("tau0e", "tau0p", "fl")]))
        print("gray %-12s moved inputs: %s" % (name, ", ".join("%s %.1e" % (f, worst[f]) for f in sorted(tol))))
    for name in X.GSC_CASES:
        stored, worst, margin = {}, {}, np.inf
        rng = np.random.RandomState(sum(map(ord, "gsc" + name)))
        for nlay, ncol in SHAPES:
            c = X.gsc_case(name, nlay, ncol)
            ref = gsc(c)
            margin = min(margin, c["margin"])
            decided = c["saturated"].tobytes()
            measure(gsc, c, ref, X.GSC_INPUTS, X.GSC_FIELDS, rng, worst,
                    lambda m: X.gsc_statement(m["t"], m["q"], m["p"], m["p_int"])["saturated"].tobytes() == decided)
            stored.update({"n%d_%s" % (nlay, k): c[k] for k in X.GSC_INPUTS})
            stored.update({"n%d_ref_%s" % (nlay, k): v for k, v in ref.items()})
            print("gsc  %-18s nlay %2d  statement against the reference: bits equal %s, largest deviation %.2e" % (
                name, nlay, all(X.same_bits(ref[k], c[k]) for k in ref), max(X.deviations(c, ref, X.GSC_FIELDS).values())))
        tol = save(os.path.join(HERE, "gsc_%s.npz" % name), stored, worst, margin=np.float64(margin),
                   constants=np.array([X.GSC_CONSTANTS[k] for k in X.GSC_CONSTANT_NAMES]))
        print("gsc  %-18s margin %.2e  moved inputs: %s" % (name, margin, ", ".join("%s %.1e" % (f, worst[f]) for f in sorted(tol))))


def interface():
    """The class-level dictionaries and the defaults of __init__ of the three classes, by `ast`."""
    want = {"GrayLongwaveRadiation": "radiation", "Frierson06LongwaveOpticalDepth": "radiation", "GridScaleCondensation": "grid_scale_condensation"}
    out = {}
    for cls, src in want.items():
        tree = ast.parse(open(SOURCES[src]).read())
        node = next(n for n in tree.body if isinstance(n, ast.ClassDef) and n.name == cls)
        entry = {"base": node.bases[0].id, "init": {}}
        for item in node.body:
            if isinstance(item, ast.Assign) and item.targets[0].id.endswith("_properties"):
                entry[item.targets[0].id] = ast.literal_eval(item.value)
            if isinstance(item, ast.FunctionDef) and item.name == "__init__":
                args = [a.arg for a in item.args.args[1:]]
                entry["init"] = dict(zip(args[len(args) - len(item.args.defaults):], (ast.literal_eval(d) for d in item.args.defaults)))
                entry["init_order"] = args
        out[cls] = entry
    with open(os.path.join(HERE, "gray_interface.json"), "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(out, sort_keys=True)[:300], "...")


if __name__ == "__main__":
    cases(*reference())
    interface()
