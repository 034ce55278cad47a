"""Golden fixtures of the land surface, from the reference's own code.  Run by hand where a checkout of the reference is at
$CLIMT_REFERENCE (never by the tests, which read what this wrote):

    CLIMT_REFERENCE=<checkout> python tests/golden/make_land_surface_golden.py

1. bucket_<case>.npz, second_best_<case>.npz -- climt/_core/tridiagonal.py, the five process modules of
   climt/_components/second_best/processes/ and the two component files loaded WHERE THEY LIE and executed under plain numpy on
   the inputs of tests/land_surface_cases.py: stub modules stand in for `sympl` (the component base classes are `object`,
   get_constant returns the constants of the cases, initialize_numpy_arrays_with_properties makes zeros of the stated dims) and
   for the reference's backend (jit_compile the identity in both call forms).  The reference's array_call of both classes is
   called with the arrays as sympl would hand them over (the atmosphere [1][columns], the four radiative fluxes [columns][1], area
   types as strings).  Bucket: every case at 4 columns.  SecondBEST: every case at 2, 4 and 12 soil levels x 4 columns (2 is the
   smallest the reference reads dz from; it runs there).  Only data is written: the inputs, the reference's outputs and, for
   SecondBEST, the smallest margin of the case and the tolerances.
   Tolerances (SecondBEST; the Bucket rule has no libm call but sqrt and is compared bit for bit): RUNS = 16 runs per shape with
   every float input moved by a random +-1 ulp -- an exact 0 stays 0, and the exactly equal pairs of a case (ts == t_air, ps ==
   p_air) move together -- and only runs with the same decisions (land_surface_cases.decisions_key, by the statement) are kept.
   Each kept run is computed twice: by the reference's array_call on the moved inputs, and by the statement on the moved inputs
   with every result of exp, log, sqrt and pow moved by a further random +-1 ulp (the reference's `**` cannot be reached from
   outside; the statement has the reference's bits on the unmoved inputs, which this maker asserts).  tol_<field> = max(16 x the
   largest deviation of either from the unmoved reference, 1e-13) on the scale of land_surface_cases.deviations, moved_<field> the
   deviation.  The maker asserts the margin of every case (land_surface_cases.MIN_MARGIN).
2. land_surface_interface.json -- the property dictionaries, the bases and the keyword defaults (and their order) of the two
   classes and of BestSubsurfaceTransport, read off the reference's source with `ast` (nothing is executed for this): names, dims,
   units and numbers only.
"""
import ast
import datetime
import importlib.util
import json
import os
import sys
import types
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import land_surface_cases as X  # noqa: E402

REF = os.environ["CLIMT_REFERENCE"]
RUNS = 16
SHAPE_NCOL = 4
BEST_DIR = os.path.join(REF, "climt", "_components", "second_best")
PROCESSES = ("soil_properties", "albedo", "surface_layer", "fluxes", "subsurface")
SOURCES = {"BucketHydrology": os.path.join(REF, "climt", "_components", "bucket_hydrology", "component.py"), "SecondBEST": os.path.join(BEST_DIR, "component.py"),
           "BestSubsurfaceTransport": os.path.join(BEST_DIR, "processes", "subsurface.py")}
K = X.BEST_CONSTANTS
CONSTANTS = {"gas_constant_of_dry_air": K["rd"], "gravitational_acceleration": K["g"], "heat_capacity_of_dry_air_at_constant_pressure": K["cp"],
             "latent_heat_of_vaporization": K["lv"], "latent_heat_of_fusion": K["lf"], "density_of_liquid_water": K["rho_water"],
             "von_karman_constant": K["karman"], "freezing_temperature_of_liquid_phase": K["t_freeze"]}
assert (X.BUCKET_SCALARS["rd"], X.BUCKET_SCALARS["cp"], X.BUCKET_SCALARS["rho_water"]) == (K["rd"], K["cp"], K["rho_water"])
BUCKET_STATE = dict(t_air="air_temperature", q_air="specific_humidity", u="eastward_wind", v="northward_wind", p_air="air_pressure", ts="surface_temperature",
                    q_sfc="surface_specific_humidity", soil_moisture="lwe_thickness_of_soil_moisture_content", precip_conv="convective_precipitation_rate",
                    precip_strat="stratiform_precipitation_rate", density="surface_material_density", thickness="soil_layer_thickness",
                    heat_capacity="heat_capacity_of_soil", deep_moisture="deep_soil_moisture_content", deep_temperature="deep_soil_temperature")
BUCKET_RESULT = dict(ts_out="surface_temperature", soil_moisture_out="lwe_thickness_of_soil_moisture_content", deep_moisture_out="deep_soil_moisture_content",
                     deep_temperature_out="deep_soil_temperature", precip="precipitation_rate", lh="surface_upward_latent_heat_flux",
                     sh="surface_upward_sensible_heat_flux", evaporation="evaporation_rate", runoff="runoff_rate", deep_fraction="deep_soil_moisture_fraction")
BEST_STATE = dict(t_soil="soil_temperature", x_w="soil_liquid_water_content", x_i="soil_ice_content", height="height_on_soil_interface_levels",
                  t_air="air_temperature", q_air="specific_humidity", u="eastward_wind", v="northward_wind", p_air="air_pressure", ps="surface_air_pressure",
                  ts="surface_temperature", snow="surface_snow_thickness")
BEST_RESULT = dict(t_soil_out="soil_temperature", x_w_out="soil_liquid_water_content", x_i_out="soil_ice_content", ts_out="surface_temperature",
                   snow_out="surface_snow_thickness", sh="surface_upward_sensible_heat_flux", lh="surface_upward_latent_heat_flux", evaporation="evaporation_rate",
                   albedo_direct="surface_albedo_for_direct_shortwave", albedo_diffuse="surface_albedo_for_diffuse_shortwave",
                   cd_heat="surface_drag_coefficient_for_heat", cd_momentum="surface_drag_coefficient_for_momentum", t2m="air_temperature_at_2m",
                   q2m="specific_humidity_at_2m", u10="eastward_wind_at_10m", v10="northward_wind_at_10m")
FLUX_STATE = dict(sw_down="downwelling_shortwave_flux_in_air", lw_down="downwelling_longwave_flux_in_air", sw_up="upwelling_shortwave_flux_in_air",
                  lw_up="upwelling_longwave_flux_in_air")
MID = ("t_air", "q_air", "u", "v", "p_air")


def reference():
    """-> (bucket(name, c) -> BUCKET_FIELDS, best(name, c) -> BEST_FIELDS), each the reference's array_call."""
    def module(name, **members):
        m = sys.modules[name] = types.ModuleType(name)
        m.__path__ = []
        for k, v in members.items():
            setattr(m, k, v)
        return m

    def load(name, path):
        spec = importlib.util.spec_from_file_location(name, path)
        sys.modules[name] = m = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(m)
        return m

    def initialize(properties, state, input_properties):
        ncol = state["area_type"].shape[0]
        nodes = state["soil_temperature"].shape[0] if "soil_temperature" in state else 0
        return {n: np.zeros((nodes, ncol) if p["dims"][0] == "soil_interface_levels" else (ncol,)) for n, p in properties.items()}

    def jit_compile(f=None, **kw):
        return f if f is not None else (lambda g: g)
    module("sympl", Stepper=object, get_constant=lambda name, units: CONSTANTS[name], initialize_numpy_arrays_with_properties=initialize)
    for pkg in ("climt", "climt._core", "climt._components", "climt._components.second_best", "climt._components.bucket_hydrology"):
        module(pkg)
    module("climt._core.backend", jit_compile=jit_compile, prange=range)
    load("climt._core.tridiagonal", os.path.join(REF, "climt", "_core", "tridiagonal.py"))
    processes = module("climt._components.second_best.processes")
    for name in PROCESSES:
        m = load("climt._components.second_best.processes." + name, os.path.join(BEST_DIR, "processes", name + ".py"))
        for member in dir(m):
            if member.startswith("Best"):
                setattr(processes, member, getattr(m, member))
    bucket_module = load("climt._components.bucket_hydrology.component", SOURCES["BucketHydrology"])
    best_module = load("climt._components.second_best.component", SOURCES["SecondBEST"])

    def bucket(name, c):
        k = X.bucket_scalars(name)
        comp = bucket_module.BucketHydrology(num_layers=X.BUCKET_CASES[name], moisture_diffusion_timescale=X.BUCKET_OVERRIDES.get(name, {}).get("tau_m"),
                                             deep_drainage_timescale=k["tau_drain"])
        assert (comp._smax, comp._g, comp._c, float(comp._l), comp._deep_smax, comp._deep_ratio) == tuple(
            k[n] for n in ("soil_moisture_max", "beta_parameter", "bulk_coefficient", "lv", "deep_soil_moisture_max", "deep_ratio"))
        state = {long: (np.array(c[short])[None, :] if short in MID else np.array(c[short])) for short, long in BUCKET_STATE.items() if short in c}
        state.update({long: np.array(c[short])[:, None] for short, long in FLUX_STATE.items()})
        state["area_type"] = np.full(c["ts"].shape, "land")
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            d, o = comp.array_call(state, datetime.timedelta(seconds=c["dt"]))
        return {short: (o if short.endswith("_out") else d)[long] for short, long in BUCKET_RESULT.items() if short in X.BUCKET_FIELDS[X.BUCKET_CASES[name]]}

    def best(name, c):
        comp = best_module.SecondBEST(soil_type="sand" if name == "sand" else "clay")
        assert (comp._min_wind, comp._subsurface._kappa, comp._subsurface._cv) == (K["min_wind"], K["kappa_soil"], K["cv_soil"])
        state = {long: (np.array(c[short])[None, :] if short in MID else np.array(c[short])) for short, long in BEST_STATE.items()}
        state.update({long: np.array(c[short])[:, None] for short, long in FLUX_STATE.items()})
        state["area_type"] = X.AREA_NAMES[c["area_type"]]
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")      # (np.where evaluates the drag branch that is not taken)
            d, o = comp.array_call(state, datetime.timedelta(seconds=c["dt"]))
        return {short: (o if short.endswith("_out") else d)[long] for short, long in BEST_RESULT.items()}
    return bucket, best


def moved(c, rng):
    """Every float input by a random +-1 ulp; an exact 0 stays 0 and exactly equal pairs move together."""
    out = dict(c)
    step = lambda a: np.where(a == 0.0, a, np.nextafter(a, np.where(rng.randint(0, 2, a.shape) == 1, np.inf, -np.inf)))
    for n in X.BEST_INPUTS:
        if n != "area_type":
            out[n] = step(np.array(c[n]))
    for a, b in (("ts", "t_air"), ("ps", "p_air")):
        same = c[a] == c[b]
        out[b] = np.where(same, out[a], out[b])
    same = c["t_soil"][-1] == c["ts"]
    out["t_soil"][-1] = np.where(same, out["ts"], out["t_soil"][-1])
    return out


def bucket_cases(run):
    for name in X.BUCKET_CASES:
        c = X.bucket_case(name, SHAPE_NCOL)
        ref = run(name, c)
        layers = X.BUCKET_CASES[name]
        equal = all(X.same_bits(ref[f], c[f]) for f in X.BUCKET_FIELDS[layers])
        print("bucket   %-18s statement against the reference: bits equal %s" % (name, equal))
        assert equal
        np.savez_compressed(os.path.join(HERE, "bucket_%s.npz" % name), layers=np.int32(layers), dt=np.float64(c["dt"]),
                            **{k: c[k] for k in X.BUCKET_INPUTS if k in c}, **{"ref_" + k: v for k, v in ref.items()})


def best_cases(run):
    for name in X.BEST_CASES:
        stored, worst, margin, tried = {}, {}, np.inf, 0
        rng = np.random.RandomState(sum(map(ord, name)))
        k = X.best_constants(name)
        ulp = lambda x: np.nextafter(x, np.inf if rng.randint(0, 2) else -np.inf)
        for nlay in X.BEST_NLAYS:
            c = X.best_case(name, nlay, SHAPE_NCOL)
            ref = run(name, c)
            equal = all(X.same_bits(ref[f], c[f]) for f in X.BEST_FIELDS)
            assert equal, (name, nlay, X.deviations(c, ref, X.BEST_FIELDS))
            margin = min(margin, float(c["margin"].min()))
            decided = X.decisions_key(c)
            kept = 0
            while kept < RUNS:
                tried += 1
                assert tried <= 60 * RUNS, "no robust candidates"
                m = moved(c, rng)
                with warnings.catch_warnings():
                    warnings.simplefilter("ignore")
                    if X.decisions_key(X.best_statement(m, c["dt"], k)) != decided:
                        continue
                    other = X.best_statement(m, c["dt"], k, ulp=ulp)
                if X.decisions_key(other) != decided:
                    continue
                kept += 1
                for result in (run(name, dict(m, dt=c["dt"])), other):
                    for f, dev in X.deviations(result, ref, X.BEST_FIELDS).items():
                        worst[f] = max(worst.get(f, 0.0), dev)
            stored.update({"n%d_%s" % (nlay, key): c[key] for key in X.BEST_INPUTS})
            stored.update({"n%d_ref_%s" % (nlay, key): v for key, v in ref.items()})
            print("best     %-18s nodes %2d  statement against the reference: bits equal %s" % (name, nlay, equal))
        assert margin >= X.MIN_MARGIN
        tol = {f: max(16.0 * v, 1e-13) for f, v in worst.items()}
        np.savez_compressed(os.path.join(HERE, "second_best_%s.npz" % name), nlays=np.array(X.BEST_NLAYS, dtype=np.int32), dt=np.float64(X.BEST_DT),
                            margin=np.float64(margin), min_margin=np.float64(X.MIN_MARGIN), **{"tol_" + f: np.float64(v) for f, v in tol.items()},
                            **{"moved_" + f: np.float64(v) for f, v in worst.items()}, **stored)
        print("best     %-18s margin %.2e  runs tried %d  largest moved: %s" % (name, margin, tried, ", ".join("%s %.1e" % (f, worst[f]) for f in sorted(worst, key=worst.get)[-3:])))


def interface():
    """The class-level dictionaries, the bases and the defaults of __init__ of the classes, by `ast`."""
    out = {}
    for cls, path in SOURCES.items():
        tree = ast.parse(open(path).read())
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
    with open(os.path.join(HERE, "land_surface_interface.json"), "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    bucket, best = reference()
    bucket_cases(bucket)
    best_cases(best)
    interface()
