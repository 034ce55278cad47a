"""Golden fixtures of the dry convective adjustment, from the reference's own code.  Run by hand where a checkout of the
reference is at $CLIMT_REFERENCE (never by the tests, which read what this wrote):

    CLIMT_REFERENCE=<checkout> python tests/golden/make_dry_adjust_golden.py

1. dry_adjust_<case>.npz -- the reference's `_dry_adj_kernel_np` (climt/_components/dry_convection/component.py) executed under
   plain numpy on the inputs of tests/dry_adjust_cases.py: stub modules stand in for `sympl` and for the reference's backend,
   with `jit_compile` the identity and `prange = range`.  Only data is written: the inputs (t, q, p, p_int), the reference's
   outputs (t_new, q_new) and the decision margin of the case (the statement's: the reference does not report one).
2. climt_cache_TestDryConvection-{column,3d}.npz -- the reference's golden caches TestDryConvection-{column,3d}-{0,1}.cache
   (netCDF3; -0: the diagnostics, none; -1: the new state) in the layout of helpers.load_cache_case: "tend" holds the
   diagnostics, "diag" the outputs.  The caches pin the reference's default state, which the adjustment leaves as it is.
"""
import importlib.util
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import dry_adjust_cases as X  # noqa: E402

REF = os.environ["CLIMT_REFERENCE"]
SHAPE = (30, 8)      # layers, columns of every fixture: ~12 KB each


def reference_kernel():
    def module(name, **members):
        m = sys.modules[name] = types.ModuleType(name)
        m.__path__ = []
        for k, v in members.items():
            setattr(m, k, v)
        return m
    module("sympl", Stepper=object, get_constant=None)
    for pkg in ("climt", "climt._core", "climt._components", "climt._components.dry_convection"):
        module(pkg)
    module("climt._core.backend", jit_compile=lambda f: f, prange=range)
    path = os.path.join(REF, "climt", "_components", "dry_convection", "component.py")
    spec = importlib.util.spec_from_file_location("climt._components.dry_convection.component", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    k = X.CONSTANTS
    params = mod.DryAdjParams(Cpd=k["cpd"], Cvap=k["cvap"], Rdair=k["rd"], Pref=k["pref"], Rv=k["rv"])
    return lambda T, q, p, p_int: mod._dry_adj_kernel_np(T, q, p, p_int, params)


def cases():
    kernel = reference_kernel()
    for name in X.CASES:
        c = X.case(name, *SHAPE)
        t_new, q_new = kernel(np.array(c["t"]), np.array(c["q"]), np.array(c["p"]), np.array(c["p_int"]))
        np.savez_compressed(os.path.join(HERE, "dry_adjust_%s.npz" % name), t=c["t"], q=c["q"], p=c["p"], p_int=c["p_int"],
                            t_new=t_new, q_new=q_new, margin=np.float64(c["margin"]))
        print(name, "margin %.3e" % c["margin"], "statement equals the reference bit for bit:",
              X.same_bits(t_new, c["t_new"]) and X.same_bits(q_new, c["q_new"]))


def caches():
    from scipy.io import netcdf_file
    for desc in ("column", "3d"):
        save = {}
        for grp, idx in (("tend", 0), ("diag", 1)):
            f = netcdf_file(os.path.join(REF, "tests", "cached_component_output", "TestDryConvection-%s-%d.cache" % (desc, idx)), mmap=False)
            for k, v in f.variables.items():
                units = getattr(v, "units", b"")
                save["%s/%s/values" % (grp, k)] = np.array(v[...])
                save["%s/%s/dims" % (grp, k)] = np.array(",".join(v.dimensions))
                save["%s/%s/units" % (grp, k)] = np.array(units.decode("utf-8") if isinstance(units, bytes) else units)
        np.savez_compressed(os.path.join(HERE, "climt_cache_TestDryConvection-%s.npz" % desc), **save)
        print(desc, sorted(k for k in save if k.endswith("values")), [save[k].shape for k in sorted(save) if k.endswith("values")])


if __name__ == "__main__":
    cases()
    caches()
