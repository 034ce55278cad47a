"""Golden fixtures of the simple boundary layer, from the reference's own code.  Run by hand where a checkout of the reference is
at $CLIMT_REFERENCE (never by the tests, which read what this wrote):

    CLIMT_REFERENCE=<checkout> python tests/golden/make_boundary_layer_golden.py

1. boundary_layer_<case>_<mode>.npz -- the reference's `_boundary_layer_kernel` (climt/_components/simple_boundary_layer/
   component.py, with climt/_core/tridiagonal.py) executed under plain numpy on the inputs of tests/boundary_layer_cases.py: stub
   modules stand in for `sympl` and for the reference's backend, with `jit_compile` the identity (bare and with arguments) and
   `prange = range`.  Only data is written: the inputs, the reference's four profiles and five diagnostics, and the decision
   margin of the case (the statement's: the reference does not report one).
2. climt_cache_TestSimpleBoundaryLayer-{column,3d}.npz -- the reference's golden caches TestSimpleBoundaryLayer-{column,3d}-{0,1}
   .cache (netCDF3; -0: the diagnostics; -1: the new state) in the layout of helpers.load_cache_case: "tend" holds the
   diagnostics, "diag" the outputs.
"""
import importlib.util
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import boundary_layer_cases as X  # noqa: E402

REF = os.environ["CLIMT_REFERENCE"]
SHAPE = (30, 8)      # layers, columns of every fixture: ~25 KB each


def reference_kernel():
    def module(name, **members):
        m = sys.modules[name] = types.ModuleType(name)
        m.__path__ = []
        for k, v in members.items():
            setattr(m, k, v)
        return m

    def jit_compile(*args, **kwargs):      # @jit_compile and @jit_compile(parallel=True)
        if len(args) == 1 and callable(args[0]) and not kwargs:
            return args[0]
        return lambda f: f

    def load(name, *path):
        spec = importlib.util.spec_from_file_location(name, os.path.join(REF, "climt", *path))
        mod = sys.modules[name] = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
        return mod
    module("sympl", Stepper=object, get_constant=None, initialize_numpy_arrays_with_properties=None)
    for pkg in ("climt", "climt._core", "climt._components", "climt._components.simple_boundary_layer"):
        module(pkg)
    module("climt._core.backend", jit_compile=jit_compile, prange=range)
    load("climt._core.tridiagonal", "_core", "tridiagonal.py")
    mod = load("climt._components.simple_boundary_layer.component", "_components", "simple_boundary_layer", "component.py")
    k = X.CONSTANTS
    params = mod.BoundaryLayerParams(Rd=k["rd"], Cp=k["cp"], g=k["g"], k=k["karman"], z0=k["z0"], fb=k["fb"], P0=k["p0"], Ric=k["ric"], Lv=k["lv"])

    def kernel(c, mode):
        nlay, ncol = c["t"].shape
        prof = {n: np.zeros((nlay, ncol)) for n in X.PROFILES}
        diag = {n: np.zeros(ncol) for n in X.DIAGNOSTICS}
        a = lambda n: np.array(c[n])
        with np.errstate(divide="ignore", invalid="ignore"):      # (C == 0: the damped K_b is 0 / (1 + inf))
            mod._boundary_layer_kernel(a("t"), a("ts"), a("p"), a("p_int"), a("ps"), a("q"), a("qs"), a("v"), a("u"), a("sh_in"), a("lh_in"),
                                       prof["t_new"], prof["q_new"], prof["v_new"], prof["u_new"], diag["stress_north"], diag["stress_east"],
                                       diag["height"], diag["sh"], diag["lh"], params, ncol, X.DT, mode)
        prof.update(diag)
        return prof
    return kernel


def cases():
    kernel = reference_kernel()
    for name in X.CASES:
        for mode in X.MODES:
            c = X.case(name, *SHAPE, mode)
            ref = kernel(c, mode)
            np.savez_compressed(os.path.join(HERE, "boundary_layer_%s_%d.npz" % (name, mode)), margin=np.float64(c["margin"]),
                                **{k: c[k] for k in X.INPUTS}, **{"ref_" + k: v for k, v in ref.items()})
            print(name, mode, "margin %.3e" % c["margin"], "statement equals the reference bit for bit:",
                  all(X.same_bits(ref[k], c[k]) for k in X.PROFILES + X.DIAGNOSTICS))


def caches():
    from scipy.io import netcdf_file
    for desc in ("column", "3d"):
        save = {}
        for grp, idx in (("tend", 0), ("diag", 1)):
            f = netcdf_file(os.path.join(REF, "tests", "cached_component_output", "TestSimpleBoundaryLayer-%s-%d.cache" % (desc, idx)), mmap=False)
            for k, v in f.variables.items():
                units = getattr(v, "units", b"")
                save["%s/%s/values" % (grp, k)] = np.array(v[...])
                save["%s/%s/dims" % (grp, k)] = np.array(",".join(v.dimensions))
                save["%s/%s/units" % (grp, k)] = np.array(units.decode("utf-8") if isinstance(units, bytes) else units)
        np.savez_compressed(os.path.join(HERE, "climt_cache_TestSimpleBoundaryLayer-%s.npz" % desc), **save)
        print(desc, sorted(k for k in save if k.endswith("values")), [save[k].shape for k in sorted(save) if k.endswith("values")])


if __name__ == "__main__":
    cases()
    caches()
