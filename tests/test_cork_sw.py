"""The table-driven correlated-k two-stream shortwave on the CPU: the numpy statement (tests/cork_sw_cases.py) against the
reference's stored outputs (tests/golden/cork_sw_<case>.npz, made by tests/golden/make_cork_sw_golden.py from the reference's own
array_call) under the stored tolerances; every case on every shape; the component's interface against
tests/golden/cork_sw_interface.json for every fixture table; pickling; and what the component and KTable refuse."""
import inspect
import json
import os
import pickle

import numpy as np
import pytest

import climt_amd
from climt_amd import cork, initialization

import cork_sw_cases as S


@pytest.fixture(autouse=True)
def band_count():
    before = dict(initialization._num_bands)
    yield
    initialization._num_bands.update(before)


class NoContext(object):
    """Stands where a Context would: these tests make no call."""


def component(table, **kw):
    return climt_amd.CorkShortwaveRadiation(optics="correlated_k", table=S.table_path(table) if table in S.TABLES else table, context=NoContext(), **kw)


def plain(name):
    t = dict(S.table(name))
    t.pop("rule"), t.pop("gases")
    return t


@pytest.mark.parametrize("name", list(S.CASES))
def test_statement_equals_the_reference_within_the_measured_tolerances(name):
    z = np.load(os.path.join(S.GOLDEN, "cork_sw_%s.npz" % name))
    tol, tab = S.tolerances(name), S.table(S.CASES[name])
    assert set(tol) == set(S.FIELDS) and all(v >= 1e-13 for v in tol.values()) and tuple(z["constants"]) == (S.G, S.CPD)
    for nlay in z["nlays"]:
        names = S.INPUTS + tuple(S.gas_names(name))
        c = {k: z["n%d_%s" % (nlay, k)] for k in names}
        case = S.cork_sw_case(name, int(nlay), c["t"].shape[1])
        assert all(S.same_bits(c[k], case[k]) for k in names), "the generator no longer makes the stored inputs"
        ref = {f: z["n%d_ref_%s" % (nlay, f)] for f in S.FIELDS}
        dev = S.deviations(S.statement(tab, c), ref, S.FIELDS)
        assert len(dev) == len(S.FIELDS)
        for f, v in dev.items():
            assert v <= tol[f], (name, int(nlay), f, v, tol[f])


@pytest.mark.parametrize("name", list(S.CASES))
def test_every_case_does_what_its_name_says_on_every_shape(name):
    for nlay in S.NLAYS:
        for ncol in S.NCOLS:
            c = S.cork_sw_case(name, nlay, ncol)      # (check_case runs inside)
            assert c["up_band"].shape == (S.table(S.CASES[name])["k_coefficients"].shape[1], nlay + 1, ncol)


def test_the_tables_reach_every_instantiation_of_the_kernel():
    seen = {(S.kernel_ng(S.table(name)["k_coefficients"].shape[2]), typ) for name in S.TABLES for typ in S.table_types(name)}
    assert seen == {(ng, typ) for ng in S.NG_BOUNDS for typ in ("f32", "f64")}
    assert {S.table(name)["k_coefficients"].shape[2] for name in S.SHAPE_TABLES} == {1, 3, 5, 9, 16}
    assert any("continuum_kappa" in S.table(name) for name in S.SHAPE_TABLES)


def test_interface_equals_the_reference_for_every_fixture_table():
    want = json.load(open(os.path.join(S.GOLDEN, "cork_sw_interface.json")))
    params = list(inspect.signature(climt_amd.CorkShortwaveRadiation.__init__).parameters.values())[1:]
    assert [p.name for p in params[:len(want["init_order"])]] == want["init_order"]
    assert {p.name: p.default for p in params if p.name in want["init"]} == want["init"]
    assert [p.name for p in params[len(want["init_order"]):]] == ["device", "context", "kwargs"]
    assert want["kwargs_popped"] == {"bond_albedo_feedback": False, "diagnostics_level": 0}
    assert want["base"] == "TendencyComponent" and issubclass(climt_amd.CorkShortwaveRadiation, climt_amd._sympl_compat.TendencyComponent)
    assert sorted(want["tables"]) == sorted(S.TABLES)
    for name, w in want["tables"].items():
        comp = component(name, bond_albedo_feedback=False, diagnostics_level=0)
        assert comp.input_properties == w["input_properties"], name
        assert "surface_temperature" in comp.input_properties
        assert comp.tendency_properties == w["tendency_properties"] and comp.diagnostic_properties == w["diagnostic_properties"], name
        assert comp.num_shortwave_bands == w["num_shortwave_bands"] == initialization._num_bands["shortwave"]
    assert "CorkShortwaveRadiation" in climt_amd.__all__


def test_ktable_of_the_shortwave_kind():
    kt = cork.KTable(S.table_path("sw_earth"), kind="shortwave")
    assert kt.gas_rule == 1 and kt.solar_source.dtype == np.float32 and kt.rayleigh.shape == (3,) and kt.planck is None and kt.k.dtype == np.float32
    assert cork.KTable(S.table_path("sw_no_rayleigh"), kind="shortwave").rayleigh is None
    assert cork.KTable(S.table_path("sw_two_gas"), kind="shortwave").gas_scale == [1.0, 44.010 / 28.970]
    with pytest.raises(ValueError, match="solar_source_per_gpoint is missing"):
        cork.KTable({k: v for k, v in plain("sw_two_band").items() if k != "solar_source_per_gpoint"}, kind="shortwave")
    with pytest.raises(ValueError, match="solar_source_per_gpoint"):
        cork.KTable(dict(plain("sw_two_band"), solar_source_per_gpoint=np.ones((2, 3))), kind="shortwave")
    with pytest.raises(ValueError, match="rayleigh_coefficient"):
        cork.KTable(dict(plain("sw_two_band"), rayleigh_coefficient=np.ones(3)), kind="shortwave")
    with pytest.raises(ValueError, match="planck_fraction is missing"):
        cork.KTable(plain("sw_two_band"))      # the longwave kind still needs its Planck fraction
    import cork_cases as L
    rank7 = dict(L.table("earth4"), solar_source_per_gpoint=np.ones((4, 16), dtype=np.float32))
    rank7.pop("rule"), rank7.pop("gases")
    with pytest.raises(ValueError, match="fails on such a table at the first call"):
        cork.KTable(rank7, kind="shortwave")
    with pytest.raises(ValueError, match="kind"):
        cork.KTable(plain("sw_two_band"), kind="visible")


def test_pickle_drops_the_context_and_the_handles():
    comp = component("sw_two_band")
    comp._handle_ds, comp._handle_ctx = 17, comp._ctx
    again = pickle.loads(pickle.dumps(comp))
    assert again._handle is None and again.num_shortwave_bands == 2 and not {"_ctx", "_handle_ds", "_handle_ctx"} & set(again.__dict__) and again._device == 0
    assert again.gas_inputs() == ["specific_humidity"] and component("sw_premixed").gas_inputs() == [] and component("sw_earth").gas_inputs() == ["specific_humidity"]


def test_what_is_not_built_is_refused_by_name():
    with pytest.raises(NotImplementedError, match="parmentier"):
        climt_amd.CorkShortwaveRadiation(context=NoContext())      # the reference's default optics
    with pytest.raises(NotImplementedError, match="diagnostics_level"):
        component("sw_two_band", diagnostics_level=1)
    with pytest.raises(NotImplementedError, match="esft"):
        component(dict(plain("sw_two_gas"), overlap_method=np.array("esft")))
    assert component(dict(plain("sw_two_band"), overlap_method=np.array("esft"))).num_shortwave_bands == 2      # one gas: the additive rule
    with pytest.raises(ValueError, match="Unknown optics"):
        climt_amd.CorkShortwaveRadiation(optics="line_by_line", context=NoContext())
    with pytest.raises(ValueError, match="needs table="):
        climt_amd.CorkShortwaveRadiation(optics="correlated_k", context=NoContext())


# ---- the column rules as the kernels run them: tools/cork_sw_check.cpp under the host sanitizers --------------------------------------
from helpers import assert_column_rows_agree, build_host_program, column_table_rows  # noqa: E402
import subprocess  # noqa: E402


@pytest.fixture(scope="module")
def cork_sw_check(tmp_path_factory):
    return build_host_program(tmp_path_factory, "cork_sw_check.cpp", sanitized=True, flags=("-ffp-contract=off",))


def check_input(name, c, k_is_f32=None, max_chunk_cols=0, cloud=True, null_outputs=False):
    """The binary input of `cork_sw_check run` for a case: what KTable prepares, in the reference's layout."""
    kt = cork.KTable(S.table_path(S.CASES[name]), kind="shortwave")
    nlay, ncol = c["t"].shape
    nX = kt.k.shape[5] if kt.k.ndim == 6 else 0
    head = np.zeros(40)
    head[:15] = [ncol, nlay, kt.gas_rule, kt.ngas, kt.nband, kt.ngpt, kt.k.shape[3], kt.k.shape[4], nX, kt.k.dtype == np.float32 if k_is_f32 is None else k_is_f32,
                 kt.log_cont is not None, cloud, kt.rayleigh is not None, kt.solar_source.dtype == np.float32, max_chunk_cols]
    head[15:15 + kt.ngas] = kt.gas_scale
    head[15 + kt.ngas:23] = 1.0
    head[23:27] = [S.M_H2O, S.G, S.CPD, 1.0]
    head[31:33] = kt.x_clip or (0.0, 0.0)
    head[33] = null_outputs
    parts = [head, kt.k.astype(np.float64), kt.weights, kt.solar_source] + [x for x in (kt.rayleigh,) if x is not None] + [kt.t_grid, kt.p_grid_log]
    parts += [x for x in (kt.x_grid_log, kt.log_cont) if x is not None]
    parts += [c[k] for k in ("t", "p", "p_int", "zenith", "albedo", "earth_sun")] + ([c[k] for k in S.CLOUD] if cloud else []) + [c[g] for g in S.gas_names(name)]
    return np.concatenate([np.ravel(np.asarray(x, dtype=np.float64)) for x in parts])


def run_check(program, tmp_path, name, c, **kw):
    """`cork_sw_check run` on a case -> (the eight fields, the program's last line), having asserted a clean exit, the tolerances
    of the statement and, bit for bit, the ascending band sum and the two heating rates.  With null_outputs the kernel function is
    handed NULL for the five optional outputs and the program writes up, dn and tend alone: those three, under the tolerances."""
    tol = S.tolerances(name)
    fields = S.FIELDS[:3] if kw.get("null_outputs") else S.FIELDS
    src, dst = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    check_input(name, c, **kw).tofile(src)
    out = subprocess.run([program, "run", src, dst], stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True)
    assert out.returncode == 0 and out.stdout.startswith("ok"), out.stderr[-2000:]
    flat, got, at = np.fromfile(dst), {}, 0
    for f in fields:
        got[f] = flat[at:at + c[f].size].reshape(c[f].shape)
        at += c[f].size
    assert at == flat.size
    for f, v in S.deviations(got, c, fields).items():
        assert v <= tol[f], (name, c["t"].shape, kw, f, v, tol[f])
    dark = np.cos(c["zenith"]) <= S.NIGHT
    assert S.same_bits(got["tend"][..., dark], c["tend"][..., dark]), name      # the heating of zeros, sign included
    if kw.get("null_outputs"):
        assert "no optional outputs" in out.stdout
        return got, out.stdout.strip().split("\n")[-1]
    up = np.zeros_like(got["up"])
    for b in range(got["up_band"].shape[0]):
        up += got["up_band"][b]
    assert S.same_bits(up, got["up"]) and S.same_bits(got["hr"], got["tend"] * 86400.0)
    import cork_cases as L
    assert S.same_bits(got["hr_band"], np.stack([L.heating(u - d, c["p_int"]) * 86400.0 for u, d in zip(got["up_band"], got["dn_band"])]))
    for f in ("hr", "hr_band"):
        assert S.same_bits(got[f][..., dark], c[f][..., dark]), (name, f)
    return got, out.stdout.strip().split("\n")[-1]


def test_check_program_table_agrees_with_the_header_and_the_python_layer(cork_sw_check):
    from climt_amd import _lib
    table = column_table_rows(cork_sw_check, "tables")
    assert [r["member"] for r in table] == list(_lib.CORK_SHORTWAVE_IN + _lib.CORK_SHORTWAVE_OUT + _lib.CORK_SHORTWAVE_DIAG)
    assert [r["member"] for r in table if r["flag"] == "required"] == ["t", "pmid", "pint", "zenith", "albedo", "earth_sun", "up", "dn", "tend"]
    assert_column_rows_agree(table, "cork_shortwave", "rrtmg_cork_shortwave")


@pytest.mark.parametrize("name", list(S.BASE_CASES))
def test_check_program_runs_clean_and_agrees_with_the_statement(cork_sw_check, tmp_path, name):
    for nlay, ncol in ((1, 1), (2, 65), (30, 5)):
        run_check(cork_sw_check, tmp_path, name, S.cork_sw_case(name, nlay, ncol))


def test_check_program_chunks_change_no_bit(cork_sw_check, tmp_path):
    for name in ("night", "cloudy", "overcast"):
        c = S.cork_sw_case(name, 30, 65)
        whole, line = run_check(cork_sw_check, tmp_path, name, c)
        assert "65 columns in 1 chunks" in line
        for chunk, n in ((64, 2), (7, 10)):
            part, line = run_check(cork_sw_check, tmp_path, name, c, max_chunk_cols=chunk)
            assert "65 columns in %d chunks" % n in line and all(S.same_bits(part[f], whole[f]) for f in S.FIELDS), (name, chunk)
    c = S.cork_sw_case("clear", 30, 5)      # no cloud arrays: the zeros the reference mixes in
    assert all(S.same_bits(a, b) for a, b in zip(run_check(cork_sw_check, tmp_path, "clear", c, cloud=False)[0].values(), run_check(cork_sw_check, tmp_path, "clear", c)[0].values()))


def test_check_program_without_the_optional_outputs_takes_the_dark_exit_and_changes_no_bit(cork_sw_check, tmp_path):
    """`overcast` has cloud in its dark columns: with tau_band NULL their beam pass ends at once, with hr_band NULL the night block
    writes the two flux columns alone, and up_band and dn_band are buffers the caller never sees."""
    for nlay, ncol in ((30, 5), (1, 5)):
        c = S.cork_sw_case("overcast", nlay, ncol)
        dark = np.cos(c["zenith"]) <= S.NIGHT
        assert dark.sum() == 2 and (nlay == 1 or (c["taucld"][:, dark] > 0).any())      # (one layer: cloud in columns 0 and 3 alone)
        full, _ = run_check(cork_sw_check, tmp_path, "overcast", c)
        for chunk in (0, 2):
            bare, line = run_check(cork_sw_check, tmp_path, "overcast", c, null_outputs=True, max_chunk_cols=chunk)
            assert set(bare) == {"up", "dn", "tend"} and all(S.same_bits(bare[f], full[f]) for f in bare), (nlay, chunk)
            for f in ("up", "dn"):
                assert S.same_bits(bare[f][:, dark], np.zeros_like(bare[f][:, dark])), (nlay, f)


@pytest.mark.parametrize("name", [n for n in S.CASES if S.CASES[n] in S.SHAPE_TABLES])
def test_check_program_runs_a_shape_table_as_float_and_as_double_to_the_same_bits(cork_sw_check, tmp_path, name):
    for nlay, ncol in ((1, 1), (2, 65), (30, 5)):
        c = S.cork_sw_case(name, nlay, ncol)
        as_float, line = run_check(cork_sw_check, tmp_path, name, c, k_is_f32=1)
        as_double, line64 = run_check(cork_sw_check, tmp_path, name, c, k_is_f32=0)
        assert line == line64 and all(S.same_bits(as_float[f], as_double[f]) for f in S.FIELDS), (name, nlay, ncol)


def test_layer_function_takes_the_resonance_guard_and_both_sides_of_both_clamps(cork_sw_check, tmp_path):
    """cork_sw_delta_scale and cork_sw_layer driven directly.  mu0 = 0.5 with w0 = 0 (k = 2 exactly): |1 - (k mu0)^2| < 1e-30 is
    taken and the sources are 0 -- no zenith angle reaches it under a cosine that does not return 0.5 (cork_sw_cases._half).  A
    backscattering layer under a high sun puts Rdir above 1 - Tnoscat; conservative layers under a low sun put Tdir past its
    bound; a forward-scattering absorbing layer leaves both inside.  Every row agrees with the numpy statement."""
    rows = np.array([[0.7, 0.0, 0.0, 0.5], [3.0, 0.0, 0.3, 0.5],                      # the guard
                     [0.1, 0.9, -0.8, 0.98], [0.001, 1.0, -0.5, 0.98], [1.0, 0.999, -0.8, 0.5],      # Rdir clamped
                     [1e-6, 1.0, 0.0, 0.05], [1.0, 1.0, 0.86, 0.05], [10.0, 1.0, 0.5, 0.01],        # Tdir clamped
                     [0.5, 0.8, 0.7, 0.6], [2.0, 0.5, 0.3, 0.9],                                   # neither
                     [3.0, 1.0, 1.0, 0.4], [3.0, 1.0, 0.8, 0.4]])                                  # both delta-scale guards; the floor of k
    src, dst = str(tmp_path / "layer_in.bin"), str(tmp_path / "layer_out.bin")
    rows.tofile(src)
    out = subprocess.run([cork_sw_check, "layer", src, dst], stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True)
    assert out.returncode == 0 and out.stdout.startswith("ok"), out.stderr[-2000:]
    got = np.fromfile(dst).reshape(len(rows), 9)
    probes = []
    for i, (tau, ssa, g, mu0) in enumerate(rows):
        probe = {}
        ts, ws, gs = S.delta_scale(np.array([[tau]]), np.array([[ssa]]), np.array([[g]]))
        want = [ts, ws, gs] + list(S.layer_operator(ts, ws, gs, np.array([[mu0]]), probe))
        probes.append(probe)
        # The same operations; exp alone differs (cork_exp against numpy's: half an ulp each, 1.1e-16 together).  An ulp of e1 moves
        # 1 - e2 by 2 ulp / (1 - e2), and every output has 1 - e2 as a factor or in its denominator: the bound is 4e-16 times that
        # amplification -- 1 for an absorbing layer, up to 1 / (2 k tau) at the floor of k (k = 1e-6).
        g1, g2 = (8.0 - ws * (5.0 + 3.0 * gs)) * 0.25, 3.0 * (ws * (1.0 - gs)) * 0.25
        kk = np.sqrt(np.maximum((g1 - g2) * (g1 + g2), S.MIN_K))
        with np.errstate(divide="ignore"):
            bound = 4e-16 * max(1.0, float(1.0 / -np.expm1(-2.0 * kk * ts)[0, 0]) if float(ts[0, 0]) > 0 else 1.0)
        for j, w in enumerate(want):
            assert abs(got[i, j] - float(w[0, 0])) <= bound * max(1.0, abs(float(w[0, 0]))), (i, j, got[i, j], float(w[0, 0]), bound)
        assert got[i, 8] == probe["den_guard"], i
    assert [p["den_guard"] for p in probes[:2]] == [1, 1] and (got[:2, 5:7] == 0.0).all() and not got[2:, 8].any()
    assert all(p["rdir_clamped"] == 1 for p in probes[2:5]) and all(got[i, 5] in (0.0, 1.0 - got[i, 7]) for i in (2, 3, 4))
    assert all(p["tdir_clamped"] == 1 for p in probes[5:8]) and all(got[i, 6] in (0.0, 1.0 - got[i, 7] - got[i, 5]) for i in (5, 6, 7))
    assert all(p["rdir_free"] == 1 and p["tdir_free"] == 1 for p in probes[8:10])
    assert tuple(got[10, :3]) == (0.0, 0.0, 0.0) and probes[11]["k_floor"] == 1 and got[11, 1] == 1.0
