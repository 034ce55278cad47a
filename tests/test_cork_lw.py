"""The table-driven correlated-k longwave on the CPU: the numpy statement (tests/cork_cases.py) against the reference's stored
outputs (tests/golden/cork_<case>.npz, made by tests/golden/make_cork_golden.py from the reference's own array_call) under the stored
tolerances; tools/cork_check.cpp -- the column rules of climt_amd/csrc/rrtmg_cork.h as the kernels run them, the row table, the
table checks and the gas refusals -- built with the host sanitizers, against the statement; the component's interface against
tests/golden/cork_interface.json for every fixture table; and what the component refuses.  The shape tables (X.SHAPE_TABLES: every
g-point bound of the kernel, padded and filled, every rank with and without a continuum, eight gases, 32 bands, two-node axes) run the
check program once as float and once as double tables, to the same bits; a coverage test holds the set of tables to all of that."""
import json
import os
import pickle
import subprocess

import numpy as np
import pytest

import climt_amd
from climt_amd import cork, initialization
from helpers import ROOT, assert_column_rows_agree, build_host_program, column_table_rows

import cork_cases as X


@pytest.fixture(autouse=True)
def band_count():
    """A CorkLongwaveRadiation sets the package's longwave band count, as the reference's does: put back what was there."""
    before = initialization._num_bands["longwave"]
    yield
    initialization._num_bands["longwave"] = before


class NoContext(object):
    """Stands where a Context would: these tests make no call."""


def component(table, **kw):
    return climt_amd.CorkLongwaveRadiation(optics="correlated_k", table=X.table_path(table) if table in X.TABLES else table, context=NoContext(), **kw)


# ---- the statement against the reference ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(X.CASES))
def test_statement_equals_the_reference_within_the_measured_tolerances(name):
    z = np.load(os.path.join(X.GOLDEN, "cork_%s.npz" % name))
    tol, tab, D = X.tolerances(name), X.table(X.CASES[name][0]), X.CASES[name][1]
    assert set(tol) == set(X.FIELDS) and all(v >= 1e-13 for v in tol.values()) and float(z["diffusivity"]) == D
    assert tuple(z["constants"]) == (X.SIGMA_SB, X.G, X.CPD)
    for nlay in z["nlays"]:
        names = X.INPUTS + tuple(X.gas_names(name))
        c = {k: z["n%d_%s" % (nlay, k)] for k in names}
        case = X.cork_case(name, int(nlay), c["t"].shape[1])
        assert all(X.same_bits(c[k], case[k]) for k in names), "the generator no longer makes the stored inputs"
        ref = {f: z["n%d_ref_%s" % (nlay, f)] for f in X.FIELDS}
        dev = X.deviations(X.statement(tab, c, D), ref)
        assert len(dev) == len(X.FIELDS)
        for f, v in dev.items():
            assert v <= tol[f], (name, int(nlay), f, v, tol[f])


@pytest.mark.parametrize("name", list(X.CASES))
def test_every_case_does_what_its_name_says_on_every_shape(name):
    for nlay in X.NLAYS:
        for ncol in X.NCOLS:
            c = X.cork_case(name, nlay, ncol)      # (check_case runs inside)
            assert c["up_band"].shape == (X.table(X.CASES[name][0])["k_coefficients"].shape[1], nlay + 1, ncol)


def test_statement_reads_pressures_in_other_units():
    c = dict(X.cork_case("two_band", 2, 4))
    mbar = dict(c, p=c["p"] / 100.0, p_int=c["p_int"] / 100.0)
    dev = X.deviations(X.statement(X.table("two_band"), mbar, pressure_scale=100.0), c)
    assert max(dev.values()) < 1e-12


# ---- the column rules as the kernels run them ---------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def cork_check(tmp_path_factory):
    return build_host_program(tmp_path_factory, "cork_check.cpp", sanitized=True, flags=("-ffp-contract=off",))


def check_input(name, c, k_is_f32=None):
    """The binary input of `cork_check run` for a case: what KTable prepares, in the reference's layout.  k_is_f32: the element
    type the program holds k in (None: the file's)."""
    kt = cork.KTable(X.table_path(X.CASES[name][0]))
    nlay, ncol = c["t"].shape
    nX, nC = (kt.k.shape[5] if kt.k.ndim >= 6 else 0), (kt.k.shape[6] if kt.k.ndim == 7 else 0)
    head = np.zeros(40)
    head[:13] = [ncol, nlay, kt.gas_rule, kt.ngas, kt.nband, kt.ngpt, kt.k.shape[3], kt.k.shape[4], nX, nC, kt.k.dtype == np.float32 if k_is_f32 is None else k_is_f32, kt.log_cont is not None, 1]
    head[13:13 + kt.ngas] = kt.gas_scale
    head[13 + kt.ngas:21] = 1.0
    head[21:27] = [X.M_H2O, X.SIGMA_SB, X.G, X.CPD, X.CASES[name][1], 1.0]
    head[27:29], head[29:31] = kt.x_clip or (0.0, 0.0), kt.c_clip or (0.0, 0.0)
    parts = [head, kt.k.astype(np.float64), kt.weights, kt.planck, kt.t_grid, kt.p_grid_log] + [x for x in (kt.x_grid_log, kt.c_grid_log, kt.log_cont) if x is not None]
    parts += [c[k] for k in ("t", "p", "p_int", "tsfc", "emis", "taucld")] + [c[g] for g in X.gas_names(name)]
    return np.concatenate([np.ravel(np.asarray(x, dtype=np.float64)) for x in parts])


def test_check_program_tables_plan_and_refusals(cork_check):
    from climt_amd import _lib
    table = column_table_rows(cork_check, "tables")
    rows = [[r[k] for k in ("entry", "io", "struct", "member", "extent", "type", "flag", "in_place_of")] for r in table]
    assert [r[3] for r in rows] == list(_lib.CORK_LONGWAVE_IN + _lib.CORK_LONGWAVE_OUT + _lib.CORK_LONGWAVE_DIAG)
    assert all((r[1] == "in") == (r[3] in _lib.CORK_LONGWAVE_IN) for r in rows)
    assert [r[3] for r in rows if r[6] == "required"] == ["t", "pmid", "pint", "tsfc", "emis", "up", "dn", "tend"]
    assert_column_rows_agree(table, "cork_longwave", "rrtmg_cork_longwave")      # names, direction, type and every extent, the band-multiplied ones among them
    assert {r["extent"] for r in table} == set(_lib.COLUMN_EXTENTS)      # this table has all six


def run_check(cork_check, tmp_path, name, c, k_is_f32=None):
    """`cork_check run` on a case -> the nine fields, having asserted what every run must keep: a clean exit, the tolerances of the
    statement, and bit for bit the ascending band sum and the two heating rates; and what the program's last line says it ran."""
    tol = X.tolerances(name)
    nlay, ncol = c["t"].shape
    src, dst = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    check_input(name, c, k_is_f32).tofile(src)
    out = subprocess.run([cork_check, "run", src, dst], stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True)
    assert out.returncode == 0 and out.stdout.startswith("ok"), out.stderr[-2000:]
    flat, got, at = np.fromfile(dst), {}, 0
    for f in X.FIELDS:
        got[f] = flat[at:at + c[f].size].reshape(c[f].shape)
        at += c[f].size
    assert at == flat.size
    for f, v in X.deviations(got, c).items():
        assert v <= tol[f], (name, nlay, ncol, k_is_f32, f, v, tol[f])
    # bit for bit: the ascending band sum, the two heating rates, the top
    up = np.zeros_like(got["up"])
    for b in range(got["up_band"].shape[0]):
        up += got["up_band"][b]
    assert X.same_bits(up, got["up"]) and X.same_bits(got["hr"], got["tend"] * 86400.0)
    assert X.same_bits(got["hr_band"], np.stack([X.heating(u - d, c["p_int"]) * 86400.0 for u, d in zip(got["up_band"], got["dn_band"])]))
    return got, out.stdout.strip().split("\n")[-1]


@pytest.mark.parametrize("name", list(X.BASE_CASES))
def test_check_program_runs_clean_and_agrees_with_the_statement(cork_check, tmp_path, name):
    for nlay, ncol in ((1, 1), (2, 65), (30, 5), (61, 3)):
        run_check(cork_check, tmp_path, name, X.cork_case(name, nlay, ncol))


@pytest.mark.parametrize("name", list(X.SHAPE_CASES))
def test_check_program_runs_a_shape_table_as_float_and_as_double_to_the_same_bits(cork_check, tmp_path, name):
    """Every stored value is float32-exact, so (double)float loses nothing: a bit of difference between the two instantiations is a
    stride or a conversion gone wrong."""
    tab = X.table(X.CASES[name][0])
    k = tab["k_coefficients"]
    for nlay, ncol in ((1, 1), (2, 65), (30, 5)):
        c = X.cork_case(name, nlay, ncol)
        as_float, line = run_check(cork_check, tmp_path, name, c, k_is_f32=1)
        as_double, line64 = run_check(cork_check, tmp_path, name, c, k_is_f32=0)
        assert line == line64 == "ok (cork, %d columns, %d layers, %d bands, %d g-points, rank %d, rule %d)" % (ncol, nlay, k.shape[1], k.shape[2], k.ndim, tab["rule"])
        for f in X.FIELDS:
            assert X.same_bits(as_float[f], as_double[f]), (name, nlay, ncol, f)


def test_the_tables_reach_every_instantiation_and_every_shape_the_kernels_branch_on():
    """cork_band_kernel<NG, K> over X.TABLES in the types the tests run them in (X.table_types): all ten (NG, K); every rank in both
    types; ranks 6 and 7 with and without a continuum; for every NG a table that fills it and (from 4 on: below that a table with
    fewer g-points takes a smaller NG) one that leaves lanes padded; eight gases; 32 bands; a two-node axis."""
    seen = [(name, X.table(name), typ) for name in X.TABLES for typ in X.table_types(name)]
    shape = lambda t: t["k_coefficients"].shape
    assert {(X.kernel_ng(shape(t)[2]), typ) for _, t, typ in seen} == {(ng, typ) for ng in X.NG_BOUNDS for typ in ("f32", "f64")}
    assert {(len(shape(t)), typ) for _, t, typ in seen} == {(rank, typ) for rank in (5, 6, 7) for typ in ("f32", "f64")}
    cont = lambda t: "continuum_kappa" in t and t["continuum_kappa"].ndim == 4
    assert {(len(shape(t)), cont(t)) for _, t, _ in seen if len(shape(t)) >= 6} == {(6, False), (6, True), (7, False), (7, True)}
    fills = {(X.kernel_ng(shape(t)[2]), shape(t)[2] == X.kernel_ng(shape(t)[2])) for _, t, _ in seen}
    assert fills == {(ng, True) for ng in X.NG_BOUNDS} | {(ng, False) for ng in X.NG_BOUNDS if ng >= 4}
    assert max(shape(t)[0] for _, t, _ in seen) == cork.MAX_GASES == 8 and max(shape(t)[1] for _, t, _ in seen) == cork.MAX_BANDS == 32
    assert max(shape(t)[2] for _, t, _ in seen) == cork.MAX_GPOINTS == X.NG_BOUNDS[-1]
    assert any(2 in shape(t)[3:] for _, t, _ in seen)
    # the thresholds above are the source's: cork_launch_band and cork_check's run_bands
    for path in (("climt_amd", "csrc", "rrtmg_cork.hip"), ("tools", "cork_check.cpp")):
        text = open(os.path.join(ROOT, *path)).read()
        for ng in X.NG_BOUNDS[:-1]:
            assert "n <= %d) " % ng in text, (path, ng)
        assert "<16, K>" in text


# ---- the component's interface ------------------------------------------------------------------------------------------------------
def test_interface_equals_the_reference_for_every_fixture_table():
    want = json.load(open(os.path.join(X.GOLDEN, "cork_interface.json")))
    import inspect
    sig = inspect.signature(climt_amd.CorkLongwaveRadiation.__init__)
    params = list(sig.parameters.values())[1:]
    assert [p.name for p in params[:len(want["init_order"])]] == want["init_order"]
    assert {p.name: p.default for p in params if p.name in want["init"]} == want["init"]
    assert [p.name for p in params[len(want["init_order"]):]] == ["device", "context", "kwargs"]
    assert climt_amd.CorkLongwaveRadiation._diffusivity_factor == want["class_diffusivity_factor"]
    assert want["base"] == "TendencyComponent" and issubclass(climt_amd.CorkLongwaveRadiation, climt_amd._sympl_compat.TendencyComponent)
    assert sorted(want["tables"]) == sorted(X.TABLES)
    for name, w in want["tables"].items():
        comp = component(name)
        assert comp.input_properties == w["input_properties"], name
        assert comp.tendency_properties == w["tendency_properties"] and comp.diagnostic_properties == w["diagnostic_properties"], name
        assert comp.num_longwave_bands == w["num_longwave_bands"] == initialization._num_bands["longwave"]
    assert "CorkLongwaveRadiation" in climt_amd.__all__


def test_eight_gases_are_stated_and_passed_in_table_order():
    want = json.load(open(os.path.join(X.GOLDEN, "cork_interface.json")))["tables"]["g4_gases8"]["input_properties"]
    comp = component("g4_gases8")
    cf = {"h2o": "specific_humidity", "co2": "mole_fraction_of_carbon_dioxide_in_air"}
    names = [cf.get(g, "mole_fraction_of_%s_in_air" % g) for g in X.GASES8]
    assert comp.gas_inputs() == names and len(set(names)) == 8 and set(names) <= set(want)
    stated = comp.input_properties
    assert stated == want and [n for n in stated if n in names] == names      # (the reference states them in table order too)
    assert [stated[n]["alias"] for n in names] == list(X.GASES8) == comp._ktable.gas_names
    assert [stated[n]["units"] for n in names] == ["kg/kg" if g == "h2o" else "mole/mole" for g in X.GASES8]
    scale = dict(zip(X.GASES8, comp._ktable.gas_scale))
    assert scale["h2o"] == scale["nh3"] == scale["so2"] == 1.0 and comp._ktable.gas_rule == 2
    for g in ("co2", "o3", "ch4", "n2o", "o2"):
        assert scale[g] == X.MOLAR_MASS[g] / X.M_DRY != 1.0, g
    assert X.gas_names("g4_gases8") == list(X.GASES8)


def test_pickle_keeps_the_class_default_of_the_diffusivity_factor():
    comp = component("two_band", diffusivity_factor=2.0)      # (holds a context object and, after a DeviceState call, handles: none is pickled)
    comp._handle_ds, comp._handle_ctx = 17, comp._ctx
    again = pickle.loads(pickle.dumps(comp))
    assert again._diffusivity_factor == 2.0 and again._handle is None and again.num_longwave_bands == 2
    assert not {"_ctx", "_handle_ds", "_handle_ctx"} & set(again.__dict__) and again._device == 0 and isinstance(comp._ctx, NoContext)
    del again.__dict__["_diffusivity_factor"]      # an instance pickled before the keyword existed
    assert again._diffusivity_factor == 1.66 and again.constants()["diffusivity"] == 1.66


def test_table_argument(tmp_path):
    arrays = dict(X.table("two_gas"))
    arrays.pop("rule"), arrays.pop("gases")
    comp = component(arrays)
    assert comp.gas_inputs() == ["specific_humidity", "mole_fraction_of_carbon_dioxide_in_air"] and comp._ktable.gas_scale == [1.0, 44.010 / 28.970]
    assert component("earth4").gas_inputs() == ["specific_humidity", "mole_fraction_of_carbon_dioxide_in_air"] and component("premixed").gas_inputs() == []
    assert component("earth4")._ktable.k.dtype == np.float32 and component("earth4")._ktable.log_cont.dtype == np.float64
    try:
        import climt  # noqa: F401
    except ImportError:
        with pytest.raises(FileNotFoundError, match="climt does not import"):
            component("earth_low_res_lw")
    pytest.importorskip("scipy")
    from scipy.io import netcdf_file
    path = str(tmp_path / "two_band.nc")
    with netcdf_file(path, "w") as nc:
        t = X.table("two_band")
        for dim, n in (("gas", 1), ("band", 2), ("gpt", 2), ("T", 5), ("P", 5)):
            nc.createDimension(dim, n)
        for name, dims in (("k_coefficients", ("gas", "band", "gpt", "T", "P")), ("gpoint_weights", ("band", "gpt")), ("planck_fraction", ("band", "gpt", "T")),
                           ("temperature_grid", ("T",)), ("pressure_grid_log", ("P",))):
            nc.createVariable(name, "d", dims)[:] = t[name]
        nc.gas_names = "h2o"
        nc.overlap_method = "additive"
    nc_table = component(path)._ktable
    assert X.same_bits(nc_table.k, t["k_coefficients"]) and nc_table.gas_names == ["h2o"] and nc_table.gas_rule == 2


# ---- refusals -----------------------------------------------------------------------------------------------------------------------
def test_what_is_not_built_is_refused_by_name():
    with pytest.raises(NotImplementedError, match="parmentier"):
        climt_amd.CorkLongwaveRadiation(context=NoContext())      # the reference's default optics
    with pytest.raises(NotImplementedError, match="diagnostics_level"):
        component("two_band", diagnostics_level=1)
    esft = dict(X.table("two_gas"), overlap_method=np.array("esft"))
    esft.pop("rule"), esft.pop("gases")
    with pytest.raises(NotImplementedError, match="esft"):
        component(esft)
    one = dict(X.table("two_band"), overlap_method=np.array("esft"))      # one gas: ESFT is the additive rule
    one.pop("rule"), one.pop("gases")
    assert component(one).num_longwave_bands == 2
    with pytest.raises(ValueError, match="Unknown optics"):
        climt_amd.CorkLongwaveRadiation(optics="line_by_line", context=NoContext())
    with pytest.raises(ValueError, match="needs table="):
        climt_amd.CorkLongwaveRadiation(optics="correlated_k", context=NoContext())


def test_inconsistent_tables_are_refused():
    def broken(name, **change):
        t = dict(X.table(name))
        t.pop("rule"), t.pop("gases")
        for k, v in change.items():
            if v is None:
                del t[k]
            else:
                t[k] = v(t[k]) if callable(v) else v
        return t
    cases = [
        ("gpoint_weights", broken("two_band", gpoint_weights=lambda w: w[:, :1])),
        ("planck_fraction", broken("two_band", planck_fraction=lambda x: x[..., :4])),
        ("temperature_grid", broken("two_band", temperature_grid=lambda g: g[:4])),
        ("strictly increase", broken("two_band", temperature_grid=lambda g: g[::-1])),
        ("strictly increase", broken("two_band", pressure_grid_log=lambda g: np.where(np.arange(g.size) == 2, g[1], g))),
        ("at least 2 nodes", broken("two_band", k_coefficients=lambda k: k[:, :, :, :1], planck_fraction=lambda x: x[..., :1], temperature_grid=lambda g: g[:1])),
        ("rank", broken("two_band", k_coefficients=lambda k: k[0])),
        ("gas names", broken("two_band", gas_names=np.array(["h2o", "co2"]))),
        ("is missing", broken("two_band", planck_fraction=None)),
        ("h2o_vmr_grid", broken("h2o_axis", h2o_vmr_grid=None)),
        ("h2o_vmr_grid", broken("h2o_axis", h2o_vmr_grid=lambda g: g[:5])),
        ("co2_vmr_grid", broken("earth4", co2_vmr_grid=None)),
        ("continuum_kappa", broken("h2o_axis", continuum_kappa=lambda x: x[:, :5])),
        ("premixed background", broken("h2o_axis", gas_names=np.array(["h2o"]))),
        ("at most", broken("two_band", k_coefficients=lambda k: np.repeat(k, 9, axis=2), gpoint_weights=lambda w: np.repeat(w, 9, axis=1),
                           planck_fraction=lambda x: np.repeat(x, 9, axis=1))),
    ]
    for match, t in cases:
        with pytest.raises(ValueError, match=match):
            component(t)


def test_a_missing_gas_is_refused_before_any_call():
    """A state that is complete but for the CO2 mole fraction a two-gas table needs: refused for that input, by name."""
    import datetime
    from climt_amd._sympl_compat import DataArray
    comp = component("two_gas")
    c = X.cork_case("two_gas", 2, 4)
    q = lambda x, dims, units: DataArray(np.array(x), dims=dims, attrs={"units": units})
    ml, il = ("mid_levels", "x"), ("interface_levels", "x")
    state = {"time": datetime.datetime(2000, 1, 1), "air_temperature": q(c["t"], ml, "degK"), "air_pressure": q(c["p"], ml, "Pa"),
             "air_pressure_on_interface_levels": q(c["p_int"], il, "Pa"), "surface_temperature": q(c["tsfc"], ("x",), "degK"),
             "surface_longwave_emissivity": q(c["emis"], ("num_longwave_bands", "x"), "dimensionless"),
             "longwave_optical_thickness_due_to_cloud": q(c["taucld"], ("mid_levels", "x", "num_longwave_bands"), "dimensionless"),
             "specific_humidity": q(c["h2o"], ml, "kg/kg")}
    with pytest.raises(Exception, match="mole_fraction_of_carbon_dioxide_in_air"):
        comp(state)
    assert not hasattr(NoContext, "cork_longwave")      # (and no call could have been made)
