"""Golden fixtures of the snow/ice column, from the reference's own code.  Run by hand where a checkout of the reference is at
$CLIMT_REFERENCE (never by the tests, which read what this wrote):

    CLIMT_REFERENCE=<checkout> python tests/golden/make_surface_ice_golden.py

1. sea_ice_<case>.npz, land_ice_<case>.npz -- climt/_core/tridiagonal.py, climt/_core/snow_ice_column.py and the two component
   files loaded WHERE THEY LIE and executed under plain numpy on the inputs of tests/surface_ice_cases.py at 3, 10 and 30 nodes x
   4 columns: stub modules stand in for `sympl` (the component base classes are `object`, get_constant returns the constants of
   the cases, initialize_numpy_arrays_with_properties makes zeros of the stated dims) and for the reference's backend
   (jit_compile the identity in both call forms, prange = range).  The reference's array_call of both classes is called with the
   arrays as sympl would hand them over (the four radiative fluxes [columns][1], area types as strings).
   Only data is written: the inputs, the reference's outputs, the smallest margin of the case and the tolerances.
   Tolerances: the reference is run RUNS = 16 times per shape with every input moved by a random +-1 ulp (an exact 0 stays 0, and
   so does a surface temperature that has the bits of t_melt - eps: surface_ice_cases.py has why), and only runs with the same
   decisions (surface_ice_cases.DECISIONS, by the statement: the two rounded integers and snow_level among them) are kept;
   tol_<field> = max(16 x the largest deviation from the unmoved run, 1e-13) on the scale of surface_ice_cases.deviations,
   moved_<field> the deviation.  The maker asserts the margin of every case (surface_ice_cases.MIN_MARGIN).
2. surface_ice_interface.json -- the property dictionaries, the bases and the keyword defaults (and their order) of the two
   classes, read off the reference's source with `ast` (nothing is executed for this): names, dims, units and numbers only.
"""
import ast
import datetime
import importlib.util
import json
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import surface_ice_cases as X  # noqa: E402

REF = os.environ["CLIMT_REFERENCE"]
SHAPES = ((3, 4), (10, 4), (30, 4))
RUNS = 16
CORE = {"tridiagonal": os.path.join(REF, "climt", "_core", "tridiagonal.py"), "snow_ice_column": os.path.join(REF, "climt", "_core", "snow_ice_column.py")}
SOURCES = {"sea_ice": os.path.join(REF, "climt", "_components", "sea_ice", "component.py"),
           "land_ice": os.path.join(REF, "climt", "_components", "land_ice", "component.py")}
CLASSES = {"sea_ice": "SeaIce", "land_ice": "LandIce"}
K = X.CONSTANTS
CONSTANTS = {"thermal_conductivity_of_solid_phase_as_ice": K["k_ice"], "thermal_conductivity_of_solid_phase_as_snow": K["k_snow"],
             "density_of_solid_phase_as_ice": K["rho_ice"], "density_of_solid_phase_as_snow": K["rho_snow"],
             "heat_capacity_of_solid_phase_as_ice": K["c_ice"], "heat_capacity_of_solid_phase_as_snow": K["c_snow"],
             "latent_heat_of_fusion": K["lf"], "freezing_temperature_of_liquid_phase": K["t_melt"]}
AREA_NAMES = np.array(["land", "land_ice", "sea", "sea_ice"])
FLUX_NAMES = dict(sw_down="downwelling_shortwave_flux_in_air", lw_down="downwelling_longwave_flux_in_air", sw_up="upwelling_shortwave_flux_in_air",
                  lw_up="upwelling_longwave_flux_in_air", lh="surface_upward_latent_heat_flux", sh="surface_upward_sensible_heat_flux")


def reference():
    """-> {kind name: run(c) -> the FIELDS}, each the reference's array_call."""
    def module(name, **members):
        m = sys.modules[name] = types.ModuleType(name)
        m.__path__ = []
        for k, v in members.items():
            setattr(m, k, v)
        return m

    def initialize(properties, state, input_properties):
        ncol = state["area_type"].shape[0]
        nodes = state["snow_and_ice_temperature"].shape[0]
        return {n: np.zeros((nodes, ncol) if p["dims"][0] == "ice_interface_levels" else (ncol,)) for n, p in properties.items()}

    def jit_compile(f=None, **kw):
        return f if f is not None else (lambda g: g)
    module("sympl", Stepper=object, get_constant=lambda name, units: CONSTANTS[name], initialize_numpy_arrays_with_properties=initialize)
    for pkg in ("climt", "climt._core", "climt._components", "climt._components.sea_ice", "climt._components.land_ice"):
        module(pkg)
    module("climt._core.backend", jit_compile=jit_compile, prange=range)
    for name, path in CORE.items():
        spec = importlib.util.spec_from_file_location("climt._core." + name, path)
        sys.modules["climt._core." + name] = m = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(m)
    runs = {}
    for name, path in SOURCES.items():
        spec = importlib.util.spec_from_file_location("climt._components.%s.component" % name, path)
        m = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(m)
        comp = getattr(m, CLASSES[name])()
        kind = X.KINDS[name]
        assert (comp._max_height, comp._epsilon) == (X.MAX_HEIGHT, X.EPS)
        assert dict(albedo_snow=comp._albedo_snow, albedo_ice=comp._albedo_ice, albedo_melt=comp._albedo_melt) == X.ALBEDO[kind]

        def run(c, comp=comp, kind=kind):
            state = {long: (np.array(c[short])[:, None] if "flux_in_air" in long else np.array(c[short])) for short, long in FLUX_NAMES.items()}
            state.update({"surface_snow_thickness": np.array(c["snow"]), "area_type": AREA_NAMES[c["area_type"]],
                          "snow_and_ice_temperature": np.array(c["t"]), "height_on_ice_interface_levels": np.array(c["height"])})
            if kind == 0:
                state.update({"sea_ice_thickness": np.array(c["thick"]), "heat_flux_into_sea_water_due_to_sea_ice": np.array(c["base"])})
            else:
                state.update({"land_ice_thickness": np.array(c["thick"]), "soil_surface_temperature": np.array(c["base"])})
            d, o = comp.array_call(state, datetime.timedelta(seconds=c["dt"]))
            assert X.same_bits(d["surface_albedo_for_direct_shortwave"], d["surface_albedo_for_diffuse_shortwave"])
            return dict(t_out=o["snow_and_ice_temperature"], height_out=o["height_on_ice_interface_levels"], snow_out=o["surface_snow_thickness"],
                        thick_out=o["sea_ice_thickness" if kind == 0 else "land_ice_thickness"], tsfc_out=o["surface_temperature"],
                        base_flux_out=d["heat_flux_into_sea_water_due_to_sea_ice" if kind == 0 else "upward_heat_flux_at_ground_level_in_soil"],
                        cond_flux=d["surface_downward_heat_flux_in_sea_ice"] if kind == 0 else np.zeros(c["thick"].shape), albedo=d["surface_albedo_for_direct_shortwave"])
        runs[name] = run
    return runs


def moved(c, rng):
    """Every float input by a random +-1 ulp; an exact 0 stays 0, and so does a surface temperature with the bits of t_melt - eps."""
    out = dict(c)
    for n in X.INPUTS:
        if n == "area_type":
            continue
        a = np.array(c[n])
        b = np.nextafter(a, np.where(rng.randint(0, 2, a.shape) == 1, np.inf, -np.inf))
        keep = a == 0.0
        if n == "t":
            keep[-1] |= a[-1] == X.CONSTANTS["t_melt"] - X.EPS
        out[n] = np.where(keep, a, b)
    return out


def cases(runs):
    for kind_name, run in runs.items():
        kind = X.KINDS[kind_name]
        for name in X.CASES[kind]:
            stored, worst, margin, tried = {}, {}, np.inf, 0
            rng = np.random.RandomState(sum(map(ord, kind_name + name)))
            for nlay, ncol in SHAPES:
                c = X.ice_case(kind, name, nlay, ncol)
                if name == "mixed_types":      # the reference raises for the column that is too tall; none at 4 columns
                    assert not c["too_tall"].any()
                ref = run(c)
                margin = min(margin, float(c["margin"].min()))
                decided = X.decisions_key(c)
                kept = 0
                while kept < RUNS:
                    tried += 1
                    assert tried <= 60 * RUNS, "no robust candidates"
                    m = moved(c, rng)
                    if X.decisions_key(X.ice_statement(kind, *(m[k] for k in X.INPUTS), c["dt"])) != decided:
                        continue
                    kept += 1
                    for f, dev in X.deviations(run(m), ref, X.FIELDS).items():
                        worst[f] = max(worst.get(f, 0.0), dev)
                stored.update({"n%d_%s" % (nlay, k): c[k] for k in X.INPUTS})
                stored["n%d_dt" % nlay] = np.float64(c["dt"])
                stored.update({"n%d_ref_%s" % (nlay, k): v for k, v in ref.items()})
                print("%-8s %-18s nodes %2d  statement against the reference: bits equal %s, largest deviation %.2e" % (
                    kind_name, name, nlay, all(X.same_bits(ref[k], c[k]) for k in ref), max(X.deviations(c, ref, X.FIELDS).values())))
            assert margin >= X.MIN_MARGIN
            tol = {f: max(16.0 * v, 1e-13) for f, v in worst.items()}
            np.savez_compressed(os.path.join(HERE, "%s_%s.npz" % (kind_name, name)), nlays=np.array([s[0] for s in SHAPES], dtype=np.int32),
                                margin=np.float64(margin), min_margin=np.float64(X.MIN_MARGIN), constants=np.array([K[k] for k in sorted(K)]),
                                **{"tol_" + f: np.float64(v) for f, v in tol.items()}, **{"moved_" + f: np.float64(v) for f, v in worst.items()}, **stored)
            print("%-8s %-18s margin %.2e  runs tried %d  moved inputs: %s" % (kind_name, name, margin, tried, ", ".join("%s %.1e" % (f, worst[f]) for f in sorted(tol))))


def interface():
    """The class-level dictionaries, the bases and the defaults of __init__ of the two classes, by `ast`."""
    out = {}
    for src, cls in CLASSES.items():
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
    with open(os.path.join(HERE, "surface_ice_interface.json"), "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    cases(reference())
    interface()
