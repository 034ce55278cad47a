"""Golden fixtures of the table-driven correlated-k two-stream shortwave, from the reference's own code and tables.  Run by hand
where a checkout of the reference is at $CLIMT_REFERENCE (never by the tests, which read what this wrote):

    CLIMT_REFERENCE=<checkout> python tests/golden/make_cork_sw_golden.py [case ...]

With case names only cork_sw_<case>.npz of those cases is written (2 below): the tables, the interface file and the files of every
other case stay what they are.  The sibling of make_cork_golden.py, whose stubs, `moved` and `_grid` it uses.

1. cork_sw_table_<name>.npz -- `sw_earth` earth_low_res_sw.npz as shipped (rank 6, float32, premixed background, Rayleigh);
   `sw_two_band` test_2band_sw.npz as shipped (rank 5, float64, gas h2o); `sw_two_gas` the same with a second gas "co2" whose k is
   0.37 of the first's; `sw_premixed` the same with gas_names ["effective"]; `sw_no_rayleigh` the same without
   rayleigh_coefficient.
1b. the shape tables (cork_sw_cases.SHAPE_TABLES: the sizes) -- a formula, as the longwave's shape tables: k = k_lo (k_hi / k_lo)^u
   with u = g / (ngpt - 1) (one g-point: 0.5), times factors by gas, band, T, log p and X; weights multiples of 2^-10 that sum to 1;
   solar_source_per_gpoint = 1361 x a band share x the weight; rayleigh_coefficient 2e-6 4^band; continuum (sw_g9_cont) as the
   longwave's.  Every array float32: run as a float table and, k cast, as a double table.
2. cork_sw_<case>.npz -- cork/common.py, optics/correlated_k.py, sw/kernels.py and sw/component.py loaded WHERE THEY LIE and
   executed under plain numpy (the stubs of make_cork_golden.reference) on the inputs of tests/cork_sw_cases.py at 2 and 30 layers
   x 4 columns.  CorkShortwaveRadiation.array_call is called with the arrays under the aliases sympl would hand it.  Only data is
   written: the inputs, the reference's outputs and the tolerances.
   Tolerances: the reference is run RUNS = 16 times per shape with every input moved by a random +-1 ulp (an exact 0 stays 0);
   tol_<field> = max(16 x the largest deviation from the unmoved run, 1e-13) on the scale of cork_cases.deviations.
   For `cloudy` the reference's own _delta_scale and _sw_dif_and_source are asked, layer by layer, whether each energy clamp is
   active (the returned value sits on a bound) and inactive somewhere: the case must show both with the reference alone.
3. cork_sw_interface.json -- the keyword defaults of CorkShortwaveRadiation.__init__ read off the reference's source with `ast`,
   and, for every fixture table, the three property dictionaries and num_shortwave_bands the reference's class states for it.
"""
import ast
import importlib.util
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
import cork_sw_cases as S  # noqa: E402
import make_cork_golden as M  # noqa: E402

SHAPES = ((2, 4), (30, 4))
RUNS = 16
OUT = {"up": "upwelling_shortwave_flux_in_air", "dn": "downwelling_shortwave_flux_in_air", "hr": "air_temperature_tendency_from_shortwave",
       "up_band": "upwelling_shortwave_flux_in_air_per_band", "dn_band": "downwelling_shortwave_flux_in_air_per_band", "tau_band": "shortwave_optical_depth_per_band",
       "hr_band": "air_temperature_tendency_from_shortwave_per_band"}
ALIAS = {"t": "T", "p": "p", "p_int": "p_int", "zenith": "zenith", "albedo": "albedo", "earth_sun": "earth_sun_factor", "taucld": "tau_cloud_sw", "ssacld": "ssa_cloud",
         "asycld": "g_cloud"}


def save(name, t):
    np.savez_compressed(S.table_path(name), **{k: np.ascontiguousarray(v) if np.ndim(v) else np.asarray(v) for k, v in t.items()})      # (a 0-d string stays 0-d)
    assert os.path.getsize(S.table_path(name)) < 200 * 1024
    print("table %-14s %7d bytes  k %s %s" % (name, os.path.getsize(S.table_path(name)), t["k_coefficients"].dtype, t["k_coefficients"].shape))


def tables():
    with np.load(os.path.join(M.SHIPPED, "earth_low_res_sw.npz"), allow_pickle=True) as z:
        earth = {k: z[k] for k in z.files}
    with np.load(os.path.join(M.SHIPPED, "test_2band_sw.npz"), allow_pickle=True) as z:
        two = {k: z[k] for k in z.files}
    tg = dict(two, k_coefficients=np.concatenate([two["k_coefficients"], 0.37 * two["k_coefficients"]], axis=0), gas_names=np.array(["h2o", "co2"]))
    pm = dict(two, gas_names=np.array(["effective"]))
    nr = {k: v for k, v in two.items() if k != "rayleigh_coefficient"}
    for name, t in (("sw_earth", earth), ("sw_two_band", two), ("sw_two_gas", tg), ("sw_premixed", pm), ("sw_no_rayleigh", nr)):
        save(name, t)


def shape_tables():
    for name, (gases, nband, ngpt, nT, nP, nX, cont, rayleigh) in S.SHAPE_TABLES.items():
        ngas = len(gases)
        k_lo, k_hi = (4e-6, 4e-3) if gases[0] == "effective" else (1e-3, 1.0)
        f32 = lambda a: np.ascontiguousarray(np.asarray(a, dtype=np.float64).astype(np.float32))
        t = {"temperature_grid": f32(M._grid(140.0, 350.0, nT)), "pressure_grid_log": f32(M._grid(np.log(1.0e3), np.log(1.2e5), nP)), "gas_names": np.array(list(gases))}
        if nX:
            t["h2o_vmr_grid"] = f32(np.exp(M._grid(np.log(1e-6), np.log(0.1), nX)))
        ax = lambda a, pos: np.asarray(a, dtype=np.float64).reshape([-1 if i == pos else 1 for i in range(6)])
        ig, b, u = ax(np.arange(ngas), 0), ax(np.arange(nband), 1), ax(np.arange(ngpt) / (ngpt - 1.0) if ngpt > 1 else [0.5], 2)
        T, lp, x = ax(t["temperature_grid"], 3), ax(t["pressure_grid_log"], 4), ax(t["h2o_vmr_grid"] if nX else [0.0], 5)
        k = (k_lo * (k_hi / k_lo) ** u * (1.0 + 0.37 * ig) * (1.0 + 0.45 * np.sin(0.9 * b + 0.4 * ig)) * (T / 250.0) ** (0.6 + 0.5 * u + 0.03 * b)
             * np.exp((0.35 - 0.2 * u) * (lp - 10.0)) * (1.0 + 4.0 * (1.0 + u) * np.sqrt(x)))
        t["k_coefficients"] = f32(k.reshape(k.shape[:5] + (nX,) * (nX > 0)))
        raw = 1.0 + 0.6 * np.sin(1.3 * np.arange(ngpt)[None, :] + 0.7 * np.arange(nband)[:, None]) + 0.1 * np.arange(ngpt)[None, :]
        w = np.round(raw / raw.sum(axis=1, keepdims=True) * 1024.0) / 1024.0
        w[:, -1] += 1.0 - w.sum(axis=1)
        assert (w > 0).all() and (w.sum(axis=1) == 1.0).all()
        t["gpoint_weights"] = f32(w)
        share = (1.0 + np.arange(nband)) / (1.0 + np.arange(nband)).sum()
        t["solar_source_per_gpoint"] = f32(1361.0 * share[:, None] * w)
        if rayleigh:
            t["rayleigh_coefficient"] = f32(2e-6 * 4.0 ** np.arange(nband))
        if cont:
            bb, TT, pp, xx = (np.asarray(a, dtype=np.float64).reshape([-1 if i == pos else 1 for i in range(4)])
                              for pos, a in enumerate((np.arange(nband), t["temperature_grid"], t["pressure_grid_log"], t["h2o_vmr_grid"])))
            t["continuum_kappa"] = f32(0.005 * xx ** 1.5 * (1.0 + 0.3 * bb) * (260.0 / TT) ** 2 * np.exp(0.2 * (pp - 10.0)))
        save(name, t)


def reference():
    """-> the reference's sw/component.py module's class and its sw/kernels.py module, loaded under make_cork_golden's stubs."""
    M.reference()      # the stubs, and common / optics.correlated_k loaded where they lie
    sys.modules["climt._core.initialization"].set_num_shortwave_bands = lambda n: None
    never = lambda *a, **k: (_ for _ in ()).throw(AssertionError("the Parmentier optics are not part of this"))
    for n in ("bond_albedo_from_fluxes",):
        setattr(sys.modules["climt._components.cork.optics.parmentier"], n, never)
    pkg = sys.modules.setdefault("climt._components.cork.sw", type(sys)("climt._components.cork.sw"))
    pkg.__path__ = []
    mods = {}
    for name, rel in (("sw.kernels", "sw/kernels.py"), ("sw.component", "sw/component.py")):
        full = "climt._components.cork." + name
        spec = importlib.util.spec_from_file_location(full, os.path.join(M.CORK, rel))
        mods[name] = sys.modules[full] = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mods[name])
    return mods["sw.component"].CorkShortwaveRadiation, mods["sw.kernels"]


def runner(cls, name):
    comp = cls(optics="correlated_k", table=S.table_path(S.CASES[name]))

    def run(c):
        state = {a: np.array(c[k]) for k, a in ALIAS.items()}
        state["T_surf"] = np.array(c["t"][0])
        state.update({g: np.array(c[g]) for g in S.gas_names(name)})
        tend, d = comp.array_call(state)
        out = {f: (np.moveaxis(d[n], -1, 0) if f.endswith("_band") else d[n]) for f, n in OUT.items()}
        return dict(out, tend=tend["T"])
    return run


def clamps_by_the_reference(kernels, c, tab):
    """The reference's own layer functions on the `cloudy` inputs -> how many layers sit on a bound of each clamp and how many inside."""
    tau_abs, dp = S.gas_depth(tab, c)
    nband, ngpt, nlay, ncol = tau_abs.shape
    count = dict(rdir_on=0, rdir_in=0, tdir_on=0, tdir_in=0)
    for b in range(nband):
        for g in range(ngpt):
            for i in range(ncol):
                mu0 = np.cos(c["zenith"][i])
                for k in range(nlay):
                    tau, ssa = tau_abs[b, g, k, i], 0.0
                    if "rayleigh_coefficient" in tab:
                        tau_ray = tab["rayleigh_coefficient"][b] * dp[k, i] / S.G
                        tau = tau_abs[b, g, k, i] + tau_ray
                        ssa = tau_ray / tau if tau > 0 else 0.0
                    tc, sc, gc = c["taucld"][k, i, b], c["ssacld"][k, i, b], c["asycld"][k, i, b]
                    tt, st = tau + tc, tau * ssa + tc * sc
                    ts, ws, gs = kernels._delta_scale(tt, st / tt if tt > 0 else 0.0, tc * sc * gc / st if st > 0 else 0.0)
                    Rdif, Tdif, Rdir, Tdir, Tn = kernels._sw_dif_and_source(ts, ws, gs, mu0)
                    count["rdir_on" if Rdir in (0.0, 1.0 - Tn) else "rdir_in"] += 1
                    count["tdir_on" if Tdir in (0.0, 1.0 - Tn - Rdir) else "tdir_in"] += 1
    return count


def case(name):
    cls, kernels = reference()
    run = runner(cls, name)
    names = S.INPUTS + tuple(S.gas_names(name))
    stored, worst, lines = {}, {}, []
    rng = np.random.RandomState(sum(map(ord, "cork_sw" + name)))
    for nlay, ncol in SHAPES:
        c = S.cork_sw_case(name, nlay, ncol)
        ref = run(c)
        for _ in range(RUNS):
            for f, dev in S.deviations(run(M.moved(c, names, rng)), ref, S.FIELDS).items():
                worst[f] = max(worst.get(f, 0.0), dev)
        stored.update({"n%d_%s" % (nlay, k): c[k] for k in names})
        stored.update({"n%d_ref_%s" % (nlay, k): v for k, v in ref.items()})
        lines.append("cork_sw %-20s nlay %2d  statement against the reference: largest deviation %.2e, bits equal %s" % (
            name, nlay, max(S.deviations(c, ref, S.FIELDS).values()), sorted(k for k in ref if S.same_bits(ref[k], c[k]))))
        if name == "cloudy" and nlay == 30:
            count = clamps_by_the_reference(kernels, c, S.table(S.CASES[name]))
            assert all(v > 0 for v in count.values()), count
            lines.append("cork_sw cloudy: the reference's own layer function: %s" % count)
    tol = {f: max(16.0 * v, 1e-13) for f, v in worst.items()}
    np.savez_compressed(os.path.join(HERE, "cork_sw_%s.npz" % name), nlays=np.array([s[0] for s in SHAPES], dtype=np.int32), constants=np.array([S.G, S.CPD]),
                        **{"tol_" + f: np.float64(v) for f, v in tol.items()}, **{"moved_" + f: np.float64(v) for f, v in worst.items()}, **stored)
    lines.append("cork_sw %-20s moved inputs: %s" % (name, ", ".join("%s %.1e" % (f, worst[f]) for f in sorted(tol))))
    return "\n".join(lines)


def interface():
    src = os.path.join(M.CORK, "sw", "component.py")
    node = next(n for n in ast.parse(open(src).read()).body if isinstance(n, ast.ClassDef) and n.name == "CorkShortwaveRadiation")
    init = next(i for i in node.body if isinstance(i, ast.FunctionDef) and i.name == "__init__")
    args = [a.arg for a in init.args.args[1:]]
    defaults = [ast.literal_eval(d) for d in init.args.defaults]
    popped = {}      # the keywords taken out of **kwargs: kwargs.pop("name", default)
    for n in ast.walk(init):
        if isinstance(n, ast.Call) and isinstance(n.func, ast.Attribute) and n.func.attr == "pop" and getattr(n.func.value, "id", "") == "kwargs":
            popped[ast.literal_eval(n.args[0])] = ast.literal_eval(n.args[1])
    out = {"base": node.bases[0].id, "init": dict(zip(args[len(args) - len(defaults):], defaults)), "init_order": args, "kwargs_popped": popped, "tables": {}}
    cls, _ = reference()
    for name in S.TABLES:
        comp = cls(optics="correlated_k", table=S.table_path(name))
        out["tables"][name] = {"input_properties": comp.input_properties, "tendency_properties": comp.tendency_properties,
                               "diagnostic_properties": comp.diagnostic_properties, "num_shortwave_bands": int(comp.num_shortwave_bands)}
    with open(os.path.join(HERE, "cork_sw_interface.json"), "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    only = sys.argv[1:]
    assert all(name in S.CASES for name in only), "usage: make_cork_sw_golden.py [case ...] with cases of %s" % sorted(S.CASES)
    if not only:
        tables()
        shape_tables()
        interface()
    for name in only or S.CASES:
        print(case(name), flush=True)
