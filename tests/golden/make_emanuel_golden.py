"""Golden fixtures of the Emanuel convection scheme, from the reference's own code.  Run by hand where a checkout of the reference
is at $CLIMT_REFERENCE (never by the tests, which read what this wrote):

    CLIMT_REFERENCE=<checkout> python tests/golden/make_emanuel_golden.py

1. emanuel_<case>_<nlay>.npz -- the reference's numpy statement of the scheme (climt/_components/emanuel/pure_python.py, loaded by
   path: plain numpy, no sympl, no numba), `_convect` with ND = nlay, NL = nlay - 3, NTRA = 0, on COLUMNS columns per file.  Only data
   is written: the inputs, the eleven outputs of `_convect` (ref_*), dt, the sixteen parameters and eight constants used, and the
   tolerances tol_<field>.  The cases of tests/emanuel_cases.py are SEARCHED for in a family of synthetic soundings (the issue's
   T = max(200, 300 (p/1000)^0.19), q = rh q_sat (p/1000)^1.5, ph = 1000 linspace(1, 0.02), generalised by a two-slope temperature
   profile, the humidity exponent, the model top, a linear wind shear, cbmf_in and dt): a seeded random search, the first
   candidates whose reference outputs show the situation -- and stay robust -- are kept.
2. Tolerance, measured against the reference alone: every candidate is run 16 more times with the inputs moved by a random +-1 ulp
   (an input that is exactly 0, as the cbmf_in of several cases has to be, stays 0) and the module's exp, log and sqrt returning a random neighbour (nextafter) of their result.  A candidate is kept only if every
   such run has the same iflag and the same zero / nonzero pattern of the tendencies and stays within 1e-9 (tests/emanuel_cases.py:
   relative to the column's largest magnitude of the field, absolute where that is zero); tol_<field> = max(16 x the largest
   deviation over the file's columns, 1e-13).  What could not be produced at some nlay is reported at the end.
3. climt_cache_TestEmanuel-{column,3d}.npz -- the reference's golden caches TestEmanuel-{column,3d}-{0,1}.cache (netCDF3; -0: the
   tendencies; -1: the diagnostics) in the layout of helpers.load_cache_case.
"""
import importlib.util
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import emanuel_cases as X  # noqa: E402

REF = os.environ["CLIMT_REFERENCE"]
COLUMNS = 3
RUNS = 16
LIMIT = 1e-9
TRIES = 3000


def reference_module():
    spec = importlib.util.spec_from_file_location("emanuel_pure_python", os.path.join(REF, "climt", "_components", "emanuel", "pure_python.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


class NeighbourNumpy:
    """numpy, with exp, log and sqrt returning a random neighbour of their result."""

    def __init__(self, rng):
        self._rng = rng

    def __getattr__(self, name):
        return getattr(np, name)

    def _near(self, x):
        k = int(self._rng.integers(3)) - 1
        return x if k == 0 else np.nextafter(x, k * np.inf)

    def exp(self, x):
        return self._near(np.exp(x))

    def log(self, x):
        return self._near(np.log(x))

    def sqrt(self, x):
        return self._near(np.sqrt(x))


def convect(mod, scheme, c, dt):
    nlay = c["t"].shape[0]
    with np.errstate(all="ignore"):
        out = scheme._convect(c["t"], c["q"], c["qs"], c["u"], c["v"], c["p"], c["ph"], nlay, nlay - 3, 0, dt, float(c["cbmf"]), np.zeros((nlay, 1)))
    got = {n: np.array(out[i], dtype=np.float64) for i, n in enumerate(X.PROFILES)}
    got.update({n: np.float64(out[4 + i]) for i, n in enumerate(X.SCALARS)})
    got["iflag"] = int(out[10])
    return got


def sounding(nlay, rh, cbmf, k1=0.19, k2=0.19, p_break=0.0, a=1.5, top=0.02, shear=0.0, ts=300.0):
    """One column: T = ts (p/1000)^k1 below p_break hPa and continued with exponent k2 above, floored at 200 K."""
    ph = 1000.0 * np.linspace(1.0, top, nlay + 1)
    p = 0.5 * (ph[:-1] + ph[1:])
    t_low = ts * (p / 1000.0) ** k1
    pb = max(p_break, 1.0)
    t_high = ts * (pb / 1000.0) ** k1 * (p / pb) ** k2
    t = np.maximum(200.0, np.where(p >= p_break, t_low, t_high))
    qs = X.bolton_q_sat(t, p * 100.0, X.CONSTANTS["rd"], X.CONSTANTS["rv"])
    q = rh * qs * (p / 1000.0) ** a
    u = 5.0 + shear * (1000.0 - p) / 100.0
    v = -2.0 + 0.5 * shear * (1000.0 - p) / 100.0
    return dict(t=t, q=q, u=u, v=v, p=p, ph=ph, cbmf=np.float64(cbmf), qs=qs)


def draw(rng, case, nlay):
    """-> (sounding keywords, dt) of one candidate."""
    issue = [(0.95, 0.02), (0.8, 0.01), (0.8, 0.0)]
    wide = dict(rh=float(10 ** rng.uniform(-5, 0)), k1=rng.uniform(0.15, 0.36), k2=rng.uniform(0.05, 0.3), p_break=rng.uniform(300.0, 950.0),
                a=rng.uniform(0.0, 8.0), top=float(rng.choice([0.02, 0.3, 0.5])), cbmf=0.0)
    narrow = rng.integers(3) != 0      # two draws in three from the issue's own family
    if case == "no_origin":
        return (dict(rh=rng.uniform(0.002, 0.03), cbmf=0.02) if narrow else dict(wide, cbmf=0.02)), 600.0
    if case == "too_cold":
        return (dict(rh=rng.uniform(0.2, 0.4), cbmf=0.0) if narrow else wide), 600.0
    if case == "flag_only":
        return (dict(rh=rng.uniform(0.6, 0.9), cbmf=0.0) if narrow else wide), 600.0
    if case == "deep":
        rh, cbmf = issue[rng.integers(2)]
        return dict(rh=rh + rng.uniform(-0.03, 0.03), cbmf=cbmf, shear=1.0), 600.0      # (a uniform wind would leave fu, fv as rounding residue)
    if case == "freezing":
        return dict(rh=0.8 + rng.uniform(-0.05, 0.05), cbmf=0.01, shear=1.0), 600.0
    if case == "sheared":
        return dict(rh=rng.uniform(0.75, 1.0), cbmf=0.0, shear=rng.uniform(1.0, 4.0)), 600.0
    if case == "cfl":
        # long, but with damp dt / delt0 < 1: beyond dt = 3000 s the relaxation clips CBMF to 0 and no mass flux is left to violate the CFL
        return dict(rh=0.9 + rng.uniform(-0.05, 0.05), cbmf=rng.uniform(0.5, 20.0), shear=1.0), float(rng.choice([1200.0, 1800.0, 2400.0]))
    wide["cbmf"] = 0.02      # lcl_range, base_at_top
    return wide, 600.0


def shows(case, got, c, again):
    """Whether the reference's outputs show the situation; `again(cbmf)`: the same column with another cbmf_in."""
    zero = all(not got[n].any() for n in X.PROFILES)
    if case == "no_origin":
        return got["iflag"] == 0 and c["cbmf"] > 0 and got["cbmf_out"] == 0
    if case == "too_cold":
        return got["iflag"] == 0 and c["cbmf"] == 0 and got["cbmf_out"] == 0 and again(0.02)["iflag"] in (1, 4)
    if case == "lcl_range":
        return got["iflag"] == 2
    if case == "base_at_top":
        return got["iflag"] == 3
    if case == "deep":
        return got["iflag"] == 1 and got["precip"] > 0 and got["wd"] > 0
    if case == "flag_only":
        return got["iflag"] == 1 and zero and c["cbmf"] == 0 and got["cbmf_out"] == 0
    if case == "cfl":
        return got["iflag"] == 4
    live = got["fq"] != 0
    if case == "freezing":
        return got["iflag"] == 1 and got["precip"] > 0 and live.any() and c["t"][live].max() > 273.0 > c["t"][live].min()
    if case == "sheared":
        return got["iflag"] == 1 and c["cbmf"] == 0 and got["fu"].any() and got["fv"].any()
    raise KeyError(case)


def robustness(mod, scheme, c, dt, base, rng):
    """-> {field: largest deviation of RUNS perturbed runs}, or None where a run changes a decision or leaves LIMIT."""
    worst = {n: 0.0 for n in X.FIELDS}
    try:
        for _ in range(RUNS):
            moved = {}
            for n in X.INPUTS:
                x = np.asarray(c[n], dtype=np.float64)
                moved[n] = np.where(x == 0, x, np.nextafter(x, np.where(rng.integers(2, size=x.shape) == 1, np.inf, -np.inf)))      # (an exact 0 stays 0)
            mod.np = NeighbourNumpy(rng)
            got = convect(mod, scheme, moved, dt)
            if got["iflag"] != base["iflag"] or any(((got[n] != 0) != (base[n] != 0)).any() for n in X.PROFILES):
                return None
            column = lambda g: {n: (g[n].reshape(-1, 1) if g[n].ndim else g[n].reshape(1)) for n in X.FIELDS}
            for n, d in X.deviations(column(got), column(base)).items():
                worst[n] = max(worst[n], d)
            if max(worst.values()) > LIMIT:
                return None
    finally:
        mod.np = np
    return worst


def cases(only=()):
    mod = reference_module()
    scheme = mod.EmanuelConvectionPython()
    for n in X.PARAMETER_NAMES + X.CONSTANT_NAMES:      # the cases module states the reference's defaults
        assert getattr(scheme, X.REFERENCE_ATTRIBUTE[n]) == dict(X.PARAMETERS, **X.CONSTANTS)[n], n
    missing, report = [], []
    for case in X.CASES:
        if only and case not in only:
            continue
        for nlay in X.NLAYS:
            rng = np.random.default_rng([nlay, sorted(X.CASES).index(case)])
            kept, dt_kept, rejected = [], None, 0
            for _ in range(TRIES):
                kw, dt = draw(rng, case, nlay)
                if dt_kept is not None and dt != dt_kept:
                    continue
                c = sounding(nlay, **kw)
                got = convect(mod, scheme, c, dt)
                again = lambda cbmf: convect(mod, scheme, dict(c, cbmf=np.float64(cbmf)), dt)
                if not shows(case, got, c, again):
                    continue
                dev = robustness(mod, scheme, c, dt, got, rng)
                if dev is None:
                    rejected += 1
                    continue
                kept.append((c, got, dev))
                dt_kept = dt
                if len(kept) == COLUMNS:
                    break
            if len(kept) < COLUMNS:
                missing.append((case, nlay, len(kept), rejected))
                continue
            save = {n: np.stack([c[n] for c, _, _ in kept], axis=-1) for n in X.INPUTS}
            save.update({"ref_" + n: np.stack([g[n] for _, g, _ in kept], axis=-1) for n in X.FIELDS})
            save["ref_iflag"] = np.array([g["iflag"] for _, g, _ in kept], dtype=np.int32)
            measured = {n: max(d[n] for _, _, d in kept) for n in X.FIELDS}
            save.update({"tol_" + n: np.float64(max(16.0 * measured[n], 1e-13)) for n in X.FIELDS})
            save.update({"dev_" + n: np.float64(measured[n]) for n in X.FIELDS})
            save["dt"] = np.float64(dt_kept)
            save.update({n: np.float64(v) for n, v in dict(X.PARAMETERS, **X.CONSTANTS).items()})
            np.savez_compressed(os.path.join(HERE, "emanuel_%s_%d.npz" % (case, nlay)), **save)
            report.append("%-12s nlay %2d  iflag %s  precip %s  dt %g  knife-edge candidates rejected %d  largest perturbed deviation %.2e  largest tolerance %.2e"
                          % (case, nlay, save["ref_iflag"].tolist(), np.array2string(save["ref_precip"], precision=3), dt_kept, rejected,
                             max(measured.values()), max(float(save["tol_" + n]) for n in X.FIELDS)))
            print(report[-1], flush=True)
    for case, nlay, found, rejected in missing:
        print("NOT PRODUCED: %s at nlay %d (%d of %d columns found in %d candidates, %d rejected as knife-edge)" % (case, nlay, found, COLUMNS, TRIES, rejected))
    return missing


def caches():
    from scipy.io import netcdf_file
    for desc in ("column", "3d"):
        save = {}
        for grp, idx in (("tend", 0), ("diag", 1)):
            f = netcdf_file(os.path.join(REF, "tests", "cached_component_output", "TestEmanuel-%s-%d.cache" % (desc, idx)), mmap=False)
            for k, v in f.variables.items():
                units = getattr(v, "units", b"")
                save["%s/%s/values" % (grp, k)] = np.array(v[...])
                save["%s/%s/dims" % (grp, k)] = np.array(",".join(v.dimensions))
                save["%s/%s/units" % (grp, k)] = np.array(units.decode("utf-8") if isinstance(units, bytes) else units)
        np.savez_compressed(os.path.join(HERE, "climt_cache_TestEmanuel-%s.npz" % desc), **save)
        print(desc, sorted(k for k in save if k.endswith("values")), [save[k].shape for k in sorted(save) if k.endswith("values")])


if __name__ == "__main__":
    caches()
    cases(sys.argv[1:])      # (case names: only those are made again)
