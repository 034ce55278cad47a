"""Golden fixtures of the simple physics package, from the reference's own Fortran.  Run by hand where a checkout of the reference
is at $CLIMT_REFERENCE and `flang` (or $FC) is on the path (never by the tests, which read what this wrote):

    CLIMT_REFERENCE=<checkout> python tests/golden/make_simple_physics_golden.py

1. simple_physics_<case>_<switches>.npz -- climt/_lib/simple_physics/simple_physics_custom.f90 compiled WHERE IT LIES
   (`flang -fPIC -O2 -shared`) into a temporary directory outside the repository and loaded with ctypes through its two bind(c)
   entry points, set_fortran_constants and simple_physics.  The arrays are prepared exactly as the reference's binder
   (_simple_physics.pyx) prepares them: the levels flipped to top-down, `thickness` the difference of the flipped interface
   pressures, `1. / thickness`, the three outputs zeroed; the profiles are flipped back.  Inputs: the cases of
   tests/simple_physics_cases.py at SHAPES (2, 30 and 61 layers, 4 columns), every case under every switch set.  Only data is
   written: per shape the inputs (`n<nlay>_<input>`) and the reference's four profiles and three diagnostics
   (`n<nlay>_ref_<field>`; lh as the Fortran returns it, unclamped), and per file dt, the constants, the flags, the switches, the
   smallest decision margin (the statement's: the Fortran does not report one) and the tolerances.
   Tolerances are measured: the reference runs 16 more times per shape with every input moved by a random +-1 ulp (an exact 0 stays
   0, and so does an interface pressure exactly equal to pbltop, which pins a decision by itself); a candidate is kept only if the
   statement decides on it as on the unmoved inputs (the same saturated layers and the same branches).
   tol_<field> = max(16 x the largest deviation of the field over the 16 runs and the three shapes, 1e-13) on the scale of
   simple_physics_cases.deviations: relative to the column's largest magnitude of the field, absolute where that is zero.  The
   factor 16 covers the device's exp, log, pow and sqrt against libm, which the Fortran's own cannot be made to vary.
2. climt_cache_TestSimplePhysics-{column,3d}.npz -- the reference's golden caches TestSimplePhysics-{column,3d}-{0,1}.cache
   (netCDF3; -0: the diagnostics; -1: the new state) in the layout of helpers.load_cache_case: "tend" holds the diagnostics,
   "diag" the outputs.
"""
import ctypes as C
import os
import shutil
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import simple_physics_cases as X  # noqa: E402

REF = os.environ["CLIMT_REFERENCE"]
SHAPES = ((2, 4), (30, 4), (61, 4))
RUNS = 16


def reference():
    """-> run(c, switches, flags) -> dict of the reference's PROFILES and DIAGNOSTICS for the inputs c (level 0 at the surface)."""
    tmp = tempfile.mkdtemp(prefix="simple_physics_ref_")
    lib_path = os.path.join(tmp, "libsimple_physics_ref.so")
    fc = os.environ.get("FC") or shutil.which("flang") or shutil.which("amdflang")
    subprocess.check_call([fc, "-fPIC", "-O2", "-shared", "-module-dir", tmp, os.path.join(REF, "climt", "_lib", "simple_physics", "simple_physics_custom.f90"),
                           "-o", lib_path], cwd=tmp)
    lib = C.CDLL(lib_path)
    d, i = C.c_double, C.c_int32
    k = X.CONSTANTS
    lib.set_fortran_constants(*(C.byref(d(k[n])) for n in ("g", "cpair", "rair", "latvap", "rh2o", "radius", "omega", "rhow", "pbltop", "pblconst",
                                                              "c_heat", "cd0", "cd1", "cm")))
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)

    def run(c, switches, flags):
        do_lsc, do_pbl, do_surf = switches
        use_ts_ext, use_qsurf_ext, test = flags
        nlay, ncol = c["t"].shape
        flip = lambda a: np.ascontiguousarray(np.asarray(a, dtype=np.float64)[::-1, :])
        u, v, t, p, p_iface, q = (flip(c[n]) for n in ("u", "v", "t", "p", "p_int", "q"))
        thickness = np.zeros((nlay, ncol))
        for a in range(nlay):
            for b in range(ncol):
                thickness[a, b] = p_iface[a + 1, b] - p_iface[a, b]
        inv_thickness = 1. / thickness
        ps, ts, qsurf, lat = (np.array(c[n], dtype=np.float64) for n in ("ps", "ts", "qsurf", "lat"))
        precip, sh, lh = np.zeros(ncol), np.zeros(ncol), np.zeros(ncol)
        lib.simple_physics(C.byref(i(ncol)), C.byref(i(nlay)), C.byref(d(X.DT)), ptr(lat), ptr(t), ptr(q), ptr(u), ptr(v), ptr(p), ptr(p_iface),
                           ptr(thickness), ptr(inv_thickness), ptr(ps), ptr(precip), C.byref(i(test)), C.byref(i(do_lsc)), C.byref(i(do_pbl)),
                           C.byref(i(do_surf)), C.byref(i(use_ts_ext)), ptr(ts), C.byref(i(use_qsurf_ext)), ptr(qsurf), ptr(sh), ptr(lh))
        return dict(t_new=flip(t), q_new=flip(q), u_new=flip(u), v_new=flip(v), precl=precip, sh=sh, lh=lh)
    return run


def moved(c, rng):
    """Every input by a random +-1 ulp; an exact 0 stays 0, an interface exactly at pbltop stays there."""
    out = {}
    for n in X.INPUTS:
        a = np.array(c[n])
        b = np.nextafter(a, np.where(rng.randint(0, 2, a.shape) == 1, np.inf, -np.inf))
        keep = a == 0.0
        if n == "p_int":
            keep |= a == X.CONSTANTS["pbltop"]
        out[n] = np.where(keep, a, b)
    return out


def cases(run):
    for name in X.CASES:
        for sw, switches in X.SWITCHES.items():
            save, worst, margin = {}, {}, np.inf
            rng = np.random.RandomState(sum(map(ord, name + sw)))
            for nlay, ncol in SHAPES:
                c = X.case(name, nlay, ncol, sw)
                ref = run(c, switches, c["flags"])
                margin = min(margin, c["margin"])
                kept = tries = 0
                while kept < RUNS:
                    tries += 1
                    assert tries <= 20 * RUNS, (name, sw, nlay, "no robust candidates")
                    m = moved(c, rng)
                    if X.decisions(X.statement(*(m[k] for k in X.INPUTS), switches, c["flags"])) != X.decisions(c):
                        continue
                    kept += 1
                    for f, dev in X.deviations(run(m, switches, c["flags"]), ref).items():
                        worst[f] = max(worst.get(f, 0.0), dev)
                save.update({"n%d_%s" % (nlay, k): c[k] for k in X.INPUTS})
                save.update({"n%d_ref_%s" % (nlay, k): v for k, v in ref.items()})
                dev = X.deviations(c, ref)
                print("%-22s %-12s nlay %2d  statement against the reference: bits equal %s, largest deviation %.2e  (%d tries)" % (
                    name, sw, nlay, all(X.same_bits(ref[k], c[k]) for k in ref), max(dev.values()), tries))
            tol = {f: max(16.0 * worst[f], 1e-13) for f in X.PROFILES + X.DIAGNOSTICS}
            print("%-22s %-12s margin %.2e  moved inputs: %s" % (name, sw, margin, ", ".join("%s %.1e" % (f, worst[f]) for f in X.PROFILES + X.DIAGNOSTICS)))
            np.savez_compressed(os.path.join(HERE, "simple_physics_%s_%s.npz" % (name, sw)), dt=np.float64(X.DT), margin=np.float64(margin),
                                constants=np.array([X.CONSTANTS[n] for n in X.CONSTANT_NAMES]), flags=np.array(c["flags"], dtype=np.int32),
                                switches=np.array(switches, dtype=np.int32), nlays=np.array([s[0] for s in SHAPES], dtype=np.int32),
                                **{"tol_" + f: np.float64(v) for f, v in tol.items()}, **{"moved_" + f: np.float64(worst[f]) for f in tol}, **save)


def caches():
    from scipy.io import netcdf_file
    for desc in ("column", "3d"):
        save = {}
        for grp, idx in (("tend", 0), ("diag", 1)):
            f = netcdf_file(os.path.join(REF, "tests", "cached_component_output", "TestSimplePhysics-%s-%d.cache" % (desc, idx)), mmap=False)
            for k, v in f.variables.items():
                units = getattr(v, "units", b"")
                save["%s/%s/values" % (grp, k)] = np.array(v[...])
                save["%s/%s/dims" % (grp, k)] = np.array(",".join(v.dimensions))
                save["%s/%s/units" % (grp, k)] = np.array(units.decode("utf-8") if isinstance(units, bytes) else units)
        np.savez_compressed(os.path.join(HERE, "climt_cache_TestSimplePhysics-%s.npz" % desc), **save)
        print(desc, sorted(k for k in save if k.endswith("values")), [save[k].shape for k in sorted(save) if k.endswith("values")])


if __name__ == "__main__":
    cases(reference())
    caches()
