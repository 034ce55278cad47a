"""The simple physics package without a GPU: the exported symbol, the header and the ctypes layer; the property dictionaries and
keyword defaults; the argument checks of the C entry; the numpy statement (tests/simple_physics_cases.py) against fixtures made
by the reference's own Fortran and against the reference's caches; the budgets that pin the rule; the stand-alone host program
of the column rule (tools/simple_physics_check.cpp on csrc/rrtmg_simple_physics.h) against the statement -- once more under the
host sanitizers; and climt_amd.SimplePhysics on host states, the host program standing in for the context.

Measured (tests/golden/make_simple_physics_golden.py, flang -O2, glibc): the statement against the reference's Fortran is
bit-identical on all 165 fixtures (11 cases x 5 switch sets x 3 shapes).  The reference under +-1 ulp of every input moves by at
most 9.8e-16 (t), 3.7e-15 (q), 3.9e-15 (u), 6.7e-15 (v) of the column's largest magnitude, 1.2e-13 of the precipitation, 3.2e-12
of the sensible and 9.8e-14 of the latent heat flux; the stored tolerances are 16 x the figure of each file, at least 1e-13.
Host program against the statement (g++ -O1, glibc): bit-identical on every case x switch set x shape (880 runs)."""
import ctypes as C
import datetime
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

import climt_amd
from climt_amd import _lib
from climt_amd._sympl_compat import DataArray
from helpers import GOLDEN, ROOT, build_host_program, load_cache_case

import simple_physics_cases as X

SYMBOL = "rrtmg_hip_simple_physics"
HEADER_STRUCT = ("typedef struct { uint32_t struct_size; int32_t ncol, nlay, memspace; "
                 "int32_t do_lsc, do_pbl, do_surf_flux, use_ts_ext, use_qsurf_ext, test, clamp_latent_heat_flux, reserved; /* reserved: 0 */ "
                 "const double *t, *q, *u, *v, *pmid; /* [nlay][ncol] */ const double *pint; /* [nlay+1][ncol] */ "
                 "const double *ps, *ts, *qsurf, *lat; /* [ncol]; ts, qsurf, lat may be NULL where unread */ "
                 "double dt; double g, cpair, rair, latvap, rh2o, radius, omega, rhow, pbltop, pblconst, c_heat, cd0, cd1, cm; "
                 "double pressure_scale, ps_scale; "
                 "double *t_out, *q_out, *u_out, *v_out; /* [nlay][ncol]; each may be its own input (in place) */ "
                 "double *precl, *sh_out, *lh_out; /* [ncol]; each may be NULL */ } rrtmg_simple_physics;")
SHAPES = [(nlay, ncol) for nlay in X.NLAYS for ncol in X.NCOLS]
SWITCH_FIELDS = ("do_lsc", "do_pbl", "do_surf_flux", "use_ts_ext", "use_qsurf_ext", "test", "clamp_latent_heat_flux")
IN = ("t", "q", "u", "v", "pmid", "pint", "ps", "ts", "qsurf", "lat")
OUT = ("t_out", "q_out", "u_out", "v_out")
DIAG = ("precl", "sh_out", "lh_out")
SCALARS = ("dt",) + X.CONSTANT_NAMES + ("pressure_scale", "ps_scale")
DIAGNOSTIC_NAMES = {"stratiform_precipitation_rate": ("precl", "m s^-1"), "surface_upward_sensible_heat_flux": ("sh", "W m^-2"),
                    "surface_upward_latent_heat_flux": ("lh", "W m^-2")}
OUTPUT_NAMES = {"air_temperature": ("t_new", "degK"), "specific_humidity": ("q_new", "kg/kg"), "eastward_wind": ("u_new", "m s^-1"),
                "northward_wind": ("v_new", "m s^-1")}


def test_symbol_header_and_python_layer():
    syms = subprocess.check_output(["nm", "-D", "--defined-only", _lib.LIB_PATH]).decode()
    assert re.search(r" T %s\b" % SYMBOL, syms)
    hdr = open(os.path.join(ROOT, "include", "rrtmg_hip.h")).read()
    flat = " ".join(hdr.split())
    assert HEADER_STRUCT in flat
    assert "int rrtmg_hip_simple_physics(rrtmg_ctx *ctx, const rrtmg_simple_physics *a);" in flat
    assert "#define RRTMG_HIP_ABI_VERSION 5" in hdr      # probed by symbol
    assert "Probe for it by symbol; RRTMG_HIP_ABI_VERSION is unchanged." in flat.split("simple physics: large-scale condensation", 1)[1].split("rrtmg_simple_physics;", 1)[0]
    lib = _lib.load_library()
    assert hasattr(lib, SYMBOL) and lib.rrtmg_hip_abi_version() == 5
    assert lib.rrtmg_hip_simple_physics.argtypes == [C.c_void_p, C.POINTER(_lib.SimplePhysics)]
    # the ctypes struct, field for field against the header's declaration order
    p, d, i = C.c_void_p, C.c_double, C.c_int32
    want = ([("struct_size", C.c_uint32)] + [(n, i) for n in ("ncol", "nlay", "memspace") + SWITCH_FIELDS + ("reserved",)] + [(n, p) for n in IN]
            + [(n, d) for n in SCALARS] + [(n, p) for n in OUT + DIAG])
    assert [(n, t) for n, t in _lib.SimplePhysics._fields_] == want
    body = re.sub(r"/\*.*?\*/", "", HEADER_STRUCT.split("{", 1)[1].rsplit("}", 1)[0])
    declared = [n for n in re.findall(r"\*?(\w+)\s*[,;]", body)]
    assert declared == [n for n, _ in want]
    assert C.sizeof(_lib.SimplePhysics) == 48 + 10 * 8 + 17 * 8 + 7 * 8
    assert lib.rrtmg_hip_simple_physics(None, C.byref(_lib.SimplePhysics())) == 4      # a NULL context is an argument error
    sig = inspect.signature(_lib.Context.simple_physics)
    assert list(sig.parameters)[:14] == ["self", "t", "q", "u", "v", "pmid", "pint", "ps", "dt", "constants", "switches", "ts", "qsurf", "lat"]
    assert list(sig.parameters)[-3:] == ["memspace", "ncol", "nlay"]
    assert isinstance(_lib.Context.has_simple_physics, property)
    assert "SimplePhysics" in climt_amd.__all__ and climt_amd.SimplePhysics is climt_amd.simple_physics.SimplePhysics
    assert list(inspect.signature(climt_amd.device_state.simple_physics_device_call).parameters) == ["self", "ds", "timestep"]
    src = open(os.path.join(ROOT, "climt_amd", "csrc", "rrtmg_simple_physics.hip")).read()
    assert re.search(r"__launch_bounds__\(64\)\s+simple_physics_kernel", src)
    rule = open(os.path.join(ROOT, "climt_amd", "csrc", "rrtmg_simple_physics.h")).read()
    for text in (src, rule):
        code = re.sub(r"//[^\n]*", "", text)
        assert not re.search(r"\bwhile\b", code)      # every loop is a for bounded by nlay
    functions = re.findall(r"RRTMG_SIMPLE_PHYSICS_HD \w+ \w+\([^)]*\) \{\n(.*)", rule)
    assert len(functions) == 3 and all(f == "#pragma clang fp contract(off)" for f in functions)


def test_property_dictionaries_and_defaults_are_the_references():
    lev = lambda units, dim="mid_levels": {"dims": [dim, "*"], "units": units}
    col = lambda units: {"dims": ["*"], "units": units}
    S = climt_amd.SimplePhysics
    assert S.input_properties == {
        "air_temperature": lev("degK"), "air_pressure": lev("Pa"), "air_pressure_on_interface_levels": lev("Pa", "interface_levels"),
        "surface_air_pressure": col("Pa"), "surface_temperature": col("degK"), "specific_humidity": lev("kg/kg"),
        "northward_wind": lev("m s^-1"), "eastward_wind": lev("m s^-1"), "surface_specific_humidity": col("kg/kg"),
        "latitude": col("degrees_north")}
    assert S.diagnostic_properties == {"stratiform_precipitation_rate": col("m s^-1"), "surface_upward_latent_heat_flux": col("W m^-2"),
                                       "surface_upward_sensible_heat_flux": col("W m^-2")}
    assert S.output_properties == {"air_temperature": {"units": "degK"}, "specific_humidity": {"units": "kg/kg"},
                                   "northward_wind": {"units": "m s^-1"}, "eastward_wind": {"units": "m s^-1"}}
    sig = inspect.signature(S.__init__)
    defaults = {n: p.default for n, p in sig.parameters.items() if p.default is not inspect.Parameter.empty}
    assert defaults == dict(simulate_cyclone=False, large_scale_condensation=True, boundary_layer=True, surface_fluxes=True,
                            use_external_surface_temperature=True, use_external_surface_specific_humidity=False, top_of_boundary_layer=85000.0,
                            boundary_layer_influence_height=20000.0, drag_coefficient_heat_fluxes=0.0011, base_momentum_drag_coefficient=0.0007,
                            wind_dependent_momentum_drag_coefficient=0.000065, maximum_momentum_drag_coefficient=0.002, device=0, context=None)
    assert list(sig.parameters)[:13] == ["self", "simulate_cyclone", "large_scale_condensation", "boundary_layer", "surface_fluxes",
                                         "use_external_surface_temperature", "use_external_surface_specific_humidity", "top_of_boundary_layer",
                                         "boundary_layer_influence_height", "drag_coefficient_heat_fluxes", "base_momentum_drag_coefficient",
                                         "wind_dependent_momentum_drag_coefficient", "maximum_momentum_drag_coefficient"]
    c = S(context=object())
    assert c.constants() == X.CONSTANTS
    assert c.switches() == dict(do_lsc=1, do_pbl=1, do_surf_flux=1, use_ts_ext=1, use_qsurf_ext=0, test=0, clamp_latent_heat_flux=1)
    # the cyclone switch goes through as `test`: True selects the baroclinic wave's formula (kept as the reference has it)
    assert S(simulate_cyclone=True, use_external_surface_temperature=False, context=object()).switches()["test"] == 1
    with pytest.raises(ValueError, match="boundary_layer=True needs surface_fluxes=True.*nothing to reproduce"):
        S(surface_fluxes=False, context=object())
    assert S(surface_fluxes=False, boundary_layer=False, context=object()).switches()["do_surf_flux"] == 0
    # constants are asked for at every call; the three new names of the stand-in
    from climt_amd import _sympl_compat as sc
    assert c.constants()["radius"] == 6.37122e6 and c.constants()["omega"] == 7.292e-5 and c.constants()["rhow"] == 1000.0
    if hasattr(sc, "_constant_overrides"):
        sc.set_constant("density_of_liquid_water", 917.0, "kg/m^3")
        try:
            assert c.constants()["rhow"] == 917.0
        finally:
            sc._constant_overrides.clear()
        assert c.constants()["rhow"] == 1000.0


# ---- the C entry's argument checks (a context made without a GPU reports errors) ------------------------------------------------------
@pytest.fixture()
def bare_context():
    lib = _lib.load_library()
    h = C.c_void_p()
    lib.rrtmg_hip_create(C.byref(h), 0)
    assert h.value
    yield lib, h
    lib.rrtmg_hip_destroy(h)


def _args(ncol=4, nlay=3, **switches):
    """A well-formed struct over host memory (the checks under test come before anything is dereferenced or enqueued)."""
    a, keep = _lib.SimplePhysics(), {}
    a.struct_size, a.ncol, a.nlay, a.memspace = C.sizeof(_lib.SimplePhysics), ncol, nlay, 0
    for n, v in dict(dict(do_lsc=1, do_pbl=1, do_surf_flux=1, use_ts_ext=1, use_qsurf_ext=1, test=0), **switches).items():
        setattr(a, n, v)
    for n in IN + OUT + DIAG:
        keep[n] = np.zeros((nlay + 1) * ncol)
        setattr(a, n, keep[n].ctypes.data)
    a.dt, a.pressure_scale, a.ps_scale = X.DT, 1.0, 1.0
    for n, v in X.CONSTANTS.items():
        setattr(a, n, v)
    return a, keep


def test_the_entry_refuses_bad_arguments(bare_context):
    lib, h = bare_context
    call = lambda a: lib.rrtmg_hip_simple_physics(h, C.byref(a))
    message = lambda: lib.rrtmg_hip_last_error(h).decode()
    assert lib.rrtmg_hip_simple_physics(h, None) == 4 and "NULL argument struct" in message()
    for size in (0, C.sizeof(_lib.SimplePhysics) - 8, C.sizeof(_lib.SimplePhysics) + 8):
        a, keep = _args()
        a.struct_size = size
        assert call(a) == 4 and "struct_size" in message()
    for value in (0, -1):
        a, keep = _args()
        a.ncol = value
        assert call(a) == 4 and "ncol must be positive" in message()
    for value in (0, -3):
        a, keep = _args()
        a.nlay = value
        assert call(a) == 4 and "nlay must be at least 1" in message()
    for value in (-1, 2):
        a, keep = _args()
        a.memspace = value
        assert call(a) == 4 and "memspace" in message()
    # the refused combination: mixing without the surface step, whatever else is set
    for lsc in (0, 1):
        a, keep = _args(do_lsc=lsc, do_pbl=1, do_surf_flux=0)
        assert call(a) == 4 and "do_pbl needs do_surf_flux" in message() and "nothing to reproduce" in message()
    for field in IN[:7] + OUT:
        a, keep = _args()
        setattr(a, field, None)
        assert call(a) == 4 and "must be given" in message(), field
    # ts, qsurf and lat are required exactly where the switches have them read
    for field, on, off in (("ts", dict(use_ts_ext=1), dict(use_ts_ext=0)), ("qsurf", dict(use_qsurf_ext=1), dict(use_qsurf_ext=0)),
                           ("lat", dict(use_ts_ext=0, test=1), dict(use_ts_ext=0, test=0))):
        a, keep = _args(**on)
        setattr(a, field, None)
        assert call(a) == 4 and "%s must be given" % field in message(), field
        for unread in (off, dict(on, do_pbl=0, do_surf_flux=0)):
            a, keep = _args(**unread)
            setattr(a, field, None)
            a.ncol = 0      # past the pointer checks, the next refusal is the one reported: the NULL was accepted
            assert call(a) == 4 and "ncol must be positive" in message()
            a, keep = _args(**unread)
            setattr(a, field, None)
            a.t_out = keep["pmid"].ctypes.data
            assert call(a) == 4 and "t_out aliases an input" in message(), (field, unread)
    # an output over an input: only x_out == x is in place
    partner = dict(zip(OUT, ("t", "q", "u", "v")))
    for out in OUT + DIAG:
        for inp in IN:
            if partner.get(out) == inp:
                continue
            a, keep = _args(use_ts_ext=1 if inp != "lat" else 0, test=1)
            setattr(a, out, keep[inp].ctypes.data)
            assert call(a) == 4 and "%s aliases an input" % out in message(), (out, inp)
    a, keep = _args()
    a.t_out = keep["t"].ctypes.data + 8      # in place means exactly in place
    assert call(a) == 4 and "t_out aliases an input" in message()
    a, keep = _args()
    a.q_out = keep["t_out"].ctypes.data
    assert call(a) == 4 and "q_out overlaps t_out" in message()
    a, keep = _args()
    a.lh_out = keep["sh_out"].ctypes.data + 8
    assert call(a) == 4 and "lh_out overlaps sh_out" in message()


# ---- the numpy statement against the reference's own Fortran ----------------------------------------------------------------------
@pytest.mark.parametrize("sw", list(X.SWITCHES))
@pytest.mark.parametrize("name", X.CASES)
def test_statement_equals_the_reference_fixture(name, sw):
    """tests/golden/simple_physics_<case>_<switches>.npz: inputs at 2, 30 and 61 layers and what the reference's Fortran made of
    them behind the binder's preparation, with the tolerances measured on the reference itself."""
    z = np.load(os.path.join(GOLDEN, "simple_physics_%s_%s.npz" % (name, sw)))
    tol = X.tolerances(name, sw)
    assert float(z["dt"]) == X.DT and list(z["constants"]) == [X.CONSTANTS[n] for n in X.CONSTANT_NAMES]
    assert tuple(z["switches"]) == X.SWITCHES[sw] and list(z["nlays"]) == [2, 30, 61]
    assert float(z["margin"]) >= X.MIN_MARGIN
    assert all(v >= 1e-13 for v in tol.values()) and all(tol[f] == max(16.0 * float(z["moved_" + f]), 1e-13) for f in tol)
    worst, bits = 0.0, True
    for nlay in (2, 30, 61):
        c = X.case(name, nlay, z["n%d_t" % nlay].shape[1], sw)
        assert tuple(z["flags"]) == c["flags"]
        for k in X.INPUTS:
            assert X.same_bits(z["n%d_%s" % (nlay, k)], c[k]), k      # the fixture's inputs are the case builder's
        ref = {k: z["n%d_ref_%s" % (nlay, k)] for k in X.PROFILES + X.DIAGNOSTICS}
        dev = X.deviations(c, ref)
        assert set(dev) == set(X.PROFILES + X.DIAGNOSTICS)
        for k, v in dev.items():
            assert v <= tol[k], (nlay, k, v, tol[k])
        worst, bits = max(worst, max(dev.values())), bits and all(X.same_bits(ref[k], c[k]) for k in ref)
        if not X.SWITCHES[sw][2]:
            assert X.same_bits(ref["sh"], np.zeros_like(ref["sh"])) and X.same_bits(ref["lh"], np.zeros_like(ref["lh"]))      # exact +0.0
        if sw == "none":
            assert all(X.same_bits(ref[k + "_new"], c[k]) for k in "tquv") and X.same_bits(ref["precl"], np.zeros_like(ref["precl"]))
    print("%s, %s: statement against the reference, bits equal: %s, largest deviation / scale %.3e" % (name, sw, bits, worst))


@pytest.mark.parametrize("desc", ["column", "3d"])
def test_reference_cache_default_state(program, tmp_path, desc):
    """TestSimplePhysics-{column,3d}-{0,1}.cache: the diagnostics and the new state of the reference's default state (at rest,
    isothermal: what moves is the theta round trip of the mixing, 289.99999999999994 .. 290.00000000000006).  Here:
    get_default_state for the component on the cache's grid, through the component, to the reference's own criterion."""
    _, want_diag, want_out = load_cache_case("TestSimplePhysics", desc)
    assert set(want_out) == set(OUTPUT_NAMES) and set(want_diag) == set(DIAGNOSTIC_NAMES)
    nz, ny, nx = want_out["air_temperature"].values.shape
    sp = climt_amd.SimplePhysics(context=ProgramContext(program, tmp_path))
    state = climt_amd.get_default_state([sp], grid_state=climt_amd.get_grid(nx=nx, ny=ny, nz=nz))
    diagnostics, new_state = sp(state, datetime.timedelta(seconds=10))
    assert set(diagnostics) == set(want_diag) and set(new_state) == set(want_out)
    for got_all, want_all in ((diagnostics, want_diag), (new_state, want_out)):
        for name, want in want_all.items():
            got = got_all[name]
            assert climt_amd.device_state._same_units(got.attrs["units"], want.attrs["units"]), name
            g = np.transpose(got.values, [got.dims.index(d) for d in want.dims])
            assert g.shape == want.values.shape, name
            assert np.isclose(g, want.values, rtol=1e-8, atol=1e-8).all(), name      # the reference's own criterion (rtol 1e-8), its atol 1e-6 tightened
    t = new_state["air_temperature"].values
    assert 289.9999999999999 <= t.min() <= t.max() <= 290.0000000000001 and (t != 290.0).any()


# ---- physics that pins the rule ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["raining", "varied"])
def test_condensation_conserves_moist_enthalpy_and_rains_what_it_removes(name):
    k = X.CONSTANTS
    for nlay, ncol in ((1, 65), (2, 64), (30, 130), (61, 65)):
        c = X.case(name, nlay, ncol, "lsc")
        dT, dq = c["t_new"] - c["t"], c["q_new"] - c["q"]
        assert (dq[c["saturated"]] < 0).all() and not dq[~c["saturated"]].any() and not dT[~c["saturated"]].any()
        # per layer cpair dT + latvap dq = 0: each term is rounded to its field's ulp, ~3e-14 K and ~1e-18 on dT ~ 1 K
        residual = k["cpair"] * dT + k["latvap"] * dq
        assert float(np.abs(residual).max()) <= 4 * np.spacing(300.0) * k["cpair"], float(np.abs(residual).max())
        water = X.column_integrals(dq, c["p_int"]) / k["g"]
        rain = -c["precl"] * k["rhow"] * X.DT
        scale = X.column_integrals(np.abs(dq), c["p_int"]) / k["g"]
        wet = scale > 0
        assert (rain[~wet] == 0).all() and wet.any()
        # dq is q_new - q, rounded at the ulp of q ~ 1e-2 .. 1e-6 against dq / q ~ 5 %: 1e-13 of the column's |dq| with room
        assert float((np.abs(water - rain)[wet] / scale[wet]).max()) <= 1e-12


@pytest.mark.parametrize("name", ["breeze", "gale", "dew", "ice_and_water", "varied"])
def test_surface_fluxes_equal_the_columns_gain(name):
    """Surface fluxes only: the lowest layer's enthalpy and water gain are sh dt and lh dt of the UNCLAMPED fluxes (q takes the
    negative flux over dew), and nothing above it moves."""
    k = X.CONSTANTS
    for nlay, ncol in ((1, 65), (30, 130), (61, 64)):
        c = X.case(name, nlay, ncol, "surface")
        assert all(X.same_bits(c[x + "_new"][1:], c[x][1:]) for x in "tquv")
        dp = c["p_int"][0] - c["p_int"][1]
        # rho is formed from pmid and divided out through pint: the budget closes with the two densities' ratio, which is
        # (rho g / dp) * dp / (rho g) = 1 to three roundings; the differences t_new - t (~1e-2 K of 290) cost 1e-14 / 1e-2
        heat = k["cpair"] * (c["t_new"][0] - c["t"][0]) * dp / k["g"]
        water = k["latvap"] * (c["q_new"][0] - c["q"][0]) * dp / k["g"]
        for got, want, what in ((heat, c["sh"] * X.DT, "enthalpy"), (water, c["lh"] * X.DT, "water")):
            assert float(np.max(np.abs(got - want) / np.abs(want))) <= 1e-9, (name, nlay, ncol, what)
        if name == "dew":
            assert (c["lh"] < 0).all() and (c["q_new"][0] < c["q"][0]).all()
            clamped = X.statement(*(c[i] for i in X.INPUTS), c["switches"], c["flags"], clamp=True)
            assert not clamped["lh"].any() and X.same_bits(clamped["q_new"], c["q_new"])      # the diagnostic is clamped, q is not
        speed = np.hypot(c["u_new"][0], c["v_new"][0])
        assert (speed < np.hypot(c["u"][0], c["v"][0])).all()      # drag


# ---- the stand-alone host program -----------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def program(tmp_path_factory):
    return build_host_program(tmp_path_factory, "simple_physics_check.cpp", flags=["-ffp-contract=off"])


@pytest.fixture(scope="module")
def program_sanitized(tmp_path_factory):
    return build_host_program(tmp_path_factory, "simple_physics_check.cpp", sanitized=True, flags=["-ffp-contract=off"])


def run_program(exe, tmp_path, arrays, switches, flags, dt=X.DT, constants=X.CONSTANTS, in_place=False, clamp=0, pressure_scale=1.0, ps_scale=1.0):
    """arrays: the ten inputs in the order of X.INPUTS -> dict of the four profiles and three diagnostics."""
    fin, fout = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    nlay, ncol = arrays[0].shape
    head = [float(in_place)] + [float(x) for x in tuple(switches) + tuple(flags)] + [float(clamp), dt] + [constants[n] for n in X.CONSTANT_NAMES] + [pressure_scale, ps_scale]
    np.concatenate([np.array(head, dtype=np.float64)] + [np.asarray(v, dtype=np.float64).ravel() for v in arrays]).tofile(fin)
    r = subprocess.run([exe, str(ncol), str(nlay), fin, fout], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.startswith("ok"), (r.returncode, r.stdout, r.stderr)
    flat, nl = np.fromfile(fout), nlay * ncol
    assert flat.size == 4 * nl + 3 * ncol
    got = {n: flat[i * nl:(i + 1) * nl].reshape(nlay, ncol) for i, n in enumerate(X.PROFILES)}
    got.update({n: flat[4 * nl + i * ncol:4 * nl + (i + 1) * ncol] for i, n in enumerate(X.DIAGNOSTICS)})
    return got


def check_program(exe, tmp_path, name, nlay, ncol, sw, in_place):
    """-> (the largest deviation / tolerance from the statement, bits equal).  (The program itself checks in place == out of place.)"""
    c, tol = X.case(name, nlay, ncol, sw), X.tolerances(name, sw)
    got = run_program(exe, tmp_path, [c[k] for k in X.INPUTS], c["switches"], c["flags"], in_place=in_place)
    dev = X.deviations(got, c)
    assert len(dev) == 7
    for k, v in dev.items():
        assert v <= tol[k], (name, nlay, ncol, sw, k, v, tol[k])
    if sw == "none":
        assert all(X.same_bits(got[k + "_new"], c[k]) for k in "tquv") and X.same_bits(got["precl"], np.zeros(ncol))
    if not c["switches"][2]:
        assert X.same_bits(got["sh"], np.zeros(ncol)) and X.same_bits(got["lh"], np.zeros(ncol))
    return max(v / tol[k] for k, v in dev.items()), all(X.same_bits(got[k], c[k]) for k in got)


@pytest.mark.parametrize("name", X.CASES)
def test_host_program_equals_the_numpy_statement(program, tmp_path, name):
    worst, same, runs = 0.0, 0, 0
    for sw in X.SWITCHES:
        for i, (nlay, ncol) in enumerate(SHAPES):
            w, bits = check_program(program, tmp_path, name, nlay, ncol, sw, in_place=i % 2)
            worst, same, runs = max(worst, w), same + bits, runs + 1
    print("simple_physics_check, %s: largest deviation / tolerance from the statement %.3e, %d of %d runs bit-identical" % (name, worst, same, runs))


def test_host_program_under_the_address_and_undefined_behaviour_sanitizers(program_sanitized, tmp_path):
    """The same program built with -fsanitize=address,undefined and run stand-alone, clean."""
    for name in X.CASES:
        for sw in X.SWITCHES:
            for nlay, ncol in ((1, 1), (1, 65), (2, 64), (30, 65), (61, 130)):
                check_program(program_sanitized, tmp_path, name, nlay, ncol, sw, in_place=(nlay + len(sw)) % 2)


def test_host_program_clamp_and_pressure_scales(program, tmp_path):
    c = X.case("dew", 30, 65, "all")
    arrays = [c[k] for k in X.INPUTS]
    clamped = run_program(program, tmp_path, arrays, c["switches"], c["flags"], clamp=1)
    assert X.same_bits(clamped["lh"], np.zeros(65)) and all(X.same_bits(clamped[k], c[k]) for k in X.PROFILES + ("precl", "sh"))
    # pressures in mbar through the scales: the statement with the same scales, bit for bit
    mbar = [c[k] / 100.0 if k in ("p", "p_int", "ps") else c[k] for k in X.INPUTS]
    want = X.statement(*mbar, c["switches"], c["flags"], pressure_scale=100.0, ps_scale=100.0)
    got = run_program(program, tmp_path, mbar, c["switches"], c["flags"], pressure_scale=100.0, ps_scale=100.0)
    assert X.within(X.deviations(got, want), X.tolerances("dew", "all")) and all(X.same_bits(got[k], want[k]) for k in got)


# ---- the component on host states: the host program stands in for the context ------------------------------------------------------
class ProgramContext:
    """Context.simple_physics (host arrays) by the stand-alone host program."""

    def __init__(self, exe, tmp_path):
        self.exe, self.tmp_path, self.calls = exe, tmp_path, []

    def simple_physics(self, t, q, u, v, pmid, pint, ps, dt, constants, switches, ts=None, qsurf=None, lat=None, **kwargs):
        assert not kwargs and ts is not None and qsurf is not None and lat is not None
        self.calls.append((t.shape, dt, dict(constants), dict(switches)))
        got = run_program(self.exe, self.tmp_path, [t, q, u, v, pmid, pint, ps, ts, qsurf, lat],
                          [switches[n] for n in X.SWITCH_NAMES], [switches[n] for n in X.FLAGS], dt=dt, constants=constants,
                          clamp=switches["clamp_latent_heat_flux"])
        return got["t_new"], got["q_new"], got["u_new"], got["v_new"], dict(precl=got["precl"], sh_out=got["sh"], lh_out=got["lh"])


@pytest.mark.parametrize("name", ["varied", "dew", "internal_sst"])
def test_component_on_a_host_state_with_other_units_and_a_3d_grid(program, tmp_path, name):
    """Pressures in hPa / mbar and a (lat, lon) grid, levels LAST in the state's arrays: the component hands the rule
    [levels][columns] in Pa, the reference's constants, its switches and the time step in seconds, and returns the statement's
    numbers with the latent heat flux clamped."""
    nlay, ny, nx = 30, 5, 13
    c = X.case(name, nlay, ny * nx, "all")
    lev = lambda a: np.ascontiguousarray(np.transpose(a.reshape(a.shape[0], ny, nx), (1, 2, 0)))
    q3 = lambda a, dim, units, f=1.0: DataArray(lev(a) / f, dims=("lat", "lon", dim), attrs={"units": units})
    q2 = lambda a, units, f=1.0: DataArray(a.reshape(ny, nx) / f, dims=("lat", "lon"), attrs={"units": units})
    state = {"air_temperature": q3(c["t"], "mid_levels", "degK"), "specific_humidity": q3(c["q"], "mid_levels", "kg/kg"),
             "eastward_wind": q3(c["u"], "mid_levels", "m s^-1"), "northward_wind": q3(c["v"], "mid_levels", "m/s"),
             "air_pressure": q3(c["p"], "mid_levels", "hPa", 100.0), "air_pressure_on_interface_levels": q3(c["p_int"], "interface_levels", "mbar", 100.0),
             "surface_air_pressure": q2(c["ps"], "mbar", 100.0), "surface_temperature": q2(c["ts"], "degK"),
             "surface_specific_humidity": q2(c["qsurf"], "kg/kg"), "latitude": q2(c["lat"], "degrees_north"), "time": datetime.datetime(2000, 1, 1)}
    use_ts_ext, use_qsurf_ext, test = c["flags"]
    ctx = ProgramContext(program, tmp_path)
    sp = climt_amd.SimplePhysics(simulate_cyclone=bool(test), use_external_surface_temperature=bool(use_ts_ext),
                                 use_external_surface_specific_humidity=bool(use_qsurf_ext), context=ctx)
    diagnostics, new_state = sp(state, datetime.timedelta(seconds=X.DT))
    assert ctx.calls == [((nlay, ny * nx), X.DT, X.CONSTANTS, dict(do_lsc=1, do_pbl=1, do_surf_flux=1, use_ts_ext=use_ts_ext, use_qsurf_ext=use_qsurf_ext,
                                                                   test=test, clamp_latent_heat_flux=1))]
    # hPa -> Pa on the way in costs a rounding per pressure: the statement on the pressures the component formed
    back = lambda a: (a / 100.0) * 100.0
    want = X.statement(c["t"], c["q"], c["u"], c["v"], back(c["p"]), back(c["p_int"]), back(c["ps"]), c["ts"], c["qsurf"], c["lat"],
                       c["switches"], c["flags"], clamp=True)
    assert want["margin"] >= X.MIN_MARGIN and X.decisions(want) == X.decisions(c)
    assert set(new_state) == set(OUTPUT_NAMES) and set(diagnostics) == set(DIAGNOSTIC_NAMES)
    got = {}
    for n, (key, units) in OUTPUT_NAMES.items():
        x = new_state[n]
        assert x.attrs["units"] == units and set(x.dims) == {"mid_levels", "lat", "lon"}
        got[key] = np.transpose(x.values, [x.dims.index(d) for d in ("mid_levels", "lat", "lon")]).reshape(nlay, ny * nx)
    for n, (key, units) in DIAGNOSTIC_NAMES.items():
        x = diagnostics[n]
        assert x.attrs["units"] == units and tuple(x.dims) == ("lat", "lon")
        got[key] = x.values.reshape(ny * nx)
    dev = X.deviations(got, want)
    assert len(dev) == 7 and X.within(dev, X.tolerances(name, "all")), dev
    assert (got["lh"] >= 0).all() and not X.same_bits(got["t_new"], c["t"])
    if name == "dew":
        assert not got["lh"].any() and (c["lh"] < 0).all()
