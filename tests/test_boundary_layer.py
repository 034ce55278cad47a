"""The simple boundary layer without a GPU: the exported symbol, the header and the ctypes layer; the property dictionaries; the
argument checks of the C entry; the numpy statement (tests/boundary_layer_cases.py) against fixtures made by the reference's own
kernel; the budgets that pin the rule; the stand-alone host program of the column rule (tools/boundary_layer_check.cpp on
csrc/rrtmg_boundary_layer.h) against the statement -- once more under the host sanitizers; and climt_amd.SimpleBoundaryLayer on
host states, the host program standing in for the context.

Host program against the statement, largest deviation over every case x mode x shape (g++ -O1, glibc): 3.8e-16 of the column's
largest |T|, 333 of 360 runs bit-identical; the diagnostics bit-identical throughout."""
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

import boundary_layer_cases as X

SYMBOL = "rrtmg_hip_boundary_layer"
HEADER_STRUCT = ("typedef struct { uint32_t struct_size; int32_t ncol, nlay, memspace, flux_mode; "
                 "const double *t, *q, *u, *v, *pmid; /* [nlay][ncol] */ const double *pint; /* [nlay+1][ncol] */ "
                 "const double *ps, *ts, *qs; /* [ncol] */ const double *sh_in, *lh_in; /* [ncol]; required in mode 2, ignored otherwise */ "
                 "double dt; double rd, cp, g, lv, karman, z0, fb, p0, ric; double pressure_scale, ps_scale; "
                 "double *t_out, *q_out, *u_out, *v_out; /* [nlay][ncol]; each may be its own input (in place) */ "
                 "double *stress_north, *stress_east, *height, *sh_out, *lh_out; /* [ncol]; each may be NULL */ } rrtmg_boundary_layer;")
SHAPES = [(nlay, ncol) for nlay in X.NLAYS for ncol in X.NCOLS]
IN = ("t", "q", "u", "v", "pmid", "pint", "ps", "ts", "qs", "sh_in", "lh_in")
OUT = ("t_out", "q_out", "u_out", "v_out")
DIAG = ("stress_north", "stress_east", "height", "sh_out", "lh_out")
SCALARS = ("dt",) + X.CONSTANT_NAMES + ("pressure_scale", "ps_scale")
FLUXES = ("surface_upward_sensible_heat_flux", "surface_upward_latent_heat_flux")


def test_symbol_header_and_python_layer():
    syms = subprocess.check_output(["nm", "-D", "--defined-only", _lib.LIB_PATH]).decode()
    assert re.search(r" T %s\b" % SYMBOL, syms)
    hdr = open(os.path.join(ROOT, "include", "rrtmg_hip.h")).read()
    flat = " ".join(hdr.split())
    assert HEADER_STRUCT in flat
    assert "int rrtmg_hip_boundary_layer(rrtmg_ctx *ctx, const rrtmg_boundary_layer *a);" in flat
    assert "#define RRTMG_HIP_ABI_VERSION 5" in hdr      # probed by symbol
    assert "Probe for it by symbol; RRTMG_HIP_ABI_VERSION is unchanged." in flat.split("simple boundary layer", 1)[1].split("rrtmg_boundary_layer;", 1)[0]
    lib = _lib.load_library()
    assert hasattr(lib, SYMBOL) and lib.rrtmg_hip_abi_version() == 5
    assert lib.rrtmg_hip_boundary_layer.argtypes == [C.c_void_p, C.POINTER(_lib.BoundaryLayer)]
    # the ctypes struct, field for field against the header's declaration order
    p, d, i = C.c_void_p, C.c_double, C.c_int32
    want = ([("struct_size", C.c_uint32)] + [(n, i) for n in ("ncol", "nlay", "memspace", "flux_mode")] + [(n, p) for n in IN]
            + [(n, d) for n in SCALARS] + [(n, p) for n in OUT + DIAG])
    assert [(n, t) for n, t in _lib.BoundaryLayer._fields_] == want
    body = re.sub(r"/\*.*?\*/", "", HEADER_STRUCT.split("{", 1)[1].rsplit("}", 1)[0])
    declared = [n for n in re.findall(r"\*?(\w+)\s*[,;]", body)]
    assert declared == [n for n, _ in want]
    assert C.sizeof(_lib.BoundaryLayer) == 24 + 11 * 8 + 12 * 8 + 9 * 8
    assert lib.rrtmg_hip_boundary_layer(None, C.byref(_lib.BoundaryLayer())) == 4      # a NULL context is an argument error
    sig = inspect.signature(_lib.Context.boundary_layer)
    assert list(sig.parameters)[:15] == ["self", "t", "q", "u", "v", "pmid", "pint", "ps", "ts", "qs", "dt", "constants", "flux_mode", "sh_in", "lh_in"]
    assert list(sig.parameters)[-3:] == ["memspace", "ncol", "nlay"]
    assert isinstance(_lib.Context.has_boundary_layer, property)
    assert "SimpleBoundaryLayer" in climt_amd.__all__
    assert list(inspect.signature(climt_amd.device_state.boundary_layer_device_call).parameters) == ["self", "ds", "timestep"]
    src = open(os.path.join(ROOT, "climt_amd", "csrc", "rrtmg_boundary_layer.hip")).read()
    assert re.search(r"__launch_bounds__\(64\)\s+boundary_layer_kernel", src)
    rule = open(os.path.join(ROOT, "climt_amd", "csrc", "rrtmg_boundary_layer.h")).read()
    for text in (src, rule):
        code = re.sub(r"//[^\n]*", "", text)
        assert not re.search(r"\bwhile\b", code)      # every loop is a for bounded by nlay
    functions = re.findall(r"RRTMG_BOUNDARY_LAYER_HD \w+ \w+\([^)]*\) \{\n(.*)", rule)
    assert len(functions) == 3 and all(f == "#pragma clang fp contract(off)" for f in functions)


@pytest.mark.parametrize("mode", ["bulk", "external", None])
def test_property_dictionaries_are_the_references(mode):
    c = climt_amd.SimpleBoundaryLayer(surface_fluxes=mode, context=object())
    lev = lambda units, dim="mid_levels": {"dims": [dim, "*"], "units": units}
    col = lambda units: {"dims": ["*"], "units": units}
    inputs = {"air_temperature": lev("degK"), "specific_humidity": lev("kg/kg"), "air_pressure": lev("Pa"),
              "air_pressure_on_interface_levels": lev("Pa", "interface_levels"), "northward_wind": lev("m s^-1"), "eastward_wind": lev("m s^-1"),
              "surface_air_pressure": col("Pa"), "surface_temperature": col("degK"), "surface_specific_humidity": col("kg/kg")}
    diagnostics = {"northward_wind_stress": col("Pa"), "eastward_wind_stress": col("Pa"), "boundary_layer_height": col("m")}
    assert climt_amd.SimpleBoundaryLayer.input_properties == inputs and climt_amd.SimpleBoundaryLayer.diagnostic_properties == diagnostics
    if mode == "external":
        inputs.update({n: col("W m^-2") for n in FLUXES})
    if mode == "bulk":
        diagnostics.update({n: col("W m^-2") for n in FLUXES})
    assert c.input_properties == inputs and c.diagnostic_properties == diagnostics
    assert c.output_properties == {n: inputs[n] for n in ("air_temperature", "specific_humidity", "northward_wind", "eastward_wind")}
    assert c.constants() == X.CONSTANTS
    # the class dictionaries are untouched by an instance
    assert set(climt_amd.SimpleBoundaryLayer.input_properties) == set(inputs) - set(FLUXES)
    assert list(inspect.signature(c.array_call).parameters) == ["state", "timestep"]


def test_constructor_is_the_references():
    sig = inspect.signature(climt_amd.SimpleBoundaryLayer.__init__)
    defaults = {n: p.default for n, p in sig.parameters.items() if p.default is not inspect.Parameter.empty}
    assert defaults == dict(surface_fluxes="bulk", von_karman_constant=0.4, roughness_length=0.0000321, specific_fraction=0.1,
                            reference_pressure=100000, critical_richardson_number=1, device=0, context=None)
    assert list(sig.parameters)[:7] == ["self", "surface_fluxes", "von_karman_constant", "roughness_length", "specific_fraction",
                                        "reference_pressure", "critical_richardson_number"]
    for bad in ("Bulk", "none", 0, True):
        with pytest.raises(ValueError, match="surface_fluxes must be 'bulk', 'external' or None"):
            climt_amd.SimpleBoundaryLayer(surface_fluxes=bad, context=object())
    # constants are asked for at every call
    from climt_amd import _sympl_compat as sc
    c = climt_amd.SimpleBoundaryLayer(context=object(), roughness_length=0.01)
    assert c.constants()["z0"] == 0.01
    if hasattr(sc, "_constant_overrides"):
        sc.set_constant("gravitational_acceleration", 3.71, "m s^-2")
        try:
            assert c.constants()["g"] == 3.71
        finally:
            sc._constant_overrides.clear()
        assert c.constants()["g"] == 9.80665


# ---- the C entry's argument checks (a context made without a GPU reports errors) ------------------------------------------------------
@pytest.fixture()
def bare_context():
    lib = _lib.load_library()
    h = C.c_void_p()
    lib.rrtmg_hip_create(C.byref(h), 0)
    assert h.value
    yield lib, h
    lib.rrtmg_hip_destroy(h)


def _args(ncol=4, nlay=3, mode=2):
    """A well-formed struct over host memory (the checks under test come before anything is dereferenced or enqueued)."""
    a, keep = _lib.BoundaryLayer(), {}
    a.struct_size, a.ncol, a.nlay, a.memspace, a.flux_mode = C.sizeof(_lib.BoundaryLayer), ncol, nlay, 0, mode
    for n in IN + OUT + DIAG:
        keep[n] = np.zeros((nlay + 1) * ncol)
        setattr(a, n, keep[n].ctypes.data)
    a.dt, a.pressure_scale, a.ps_scale = X.DT, 1.0, 1.0
    for n, v in X.CONSTANTS.items():
        setattr(a, n, v)
    return a, keep


def test_the_entry_refuses_bad_arguments(bare_context):
    lib, h = bare_context
    call = lambda a: lib.rrtmg_hip_boundary_layer(h, C.byref(a))
    message = lambda: lib.rrtmg_hip_last_error(h).decode()
    assert lib.rrtmg_hip_boundary_layer(h, None) == 4 and "NULL argument struct" in message()
    for size in (0, C.sizeof(_lib.BoundaryLayer) - 8, C.sizeof(_lib.BoundaryLayer) + 8):
        a, keep = _args()
        a.struct_size = size
        assert call(a) == 4 and "struct_size" in message()
    for value in (0, -1):
        a, keep = _args()
        a.ncol = value
        assert call(a) == 4 and "ncol must be positive" in message()
    for value in (1, 0, -3):
        a, keep = _args()
        a.nlay = value
        assert call(a) == 4 and "nlay must be at least 2" in message() and "the reference indexes an empty array" in message()
    for value in (-1, 2):
        a, keep = _args()
        a.memspace = value
        assert call(a) == 4 and "memspace" in message()
    for value in (-1, 3):
        a, keep = _args()
        a.flux_mode = value
        assert call(a) == 4 and "flux_mode" in message()
    for field in IN[:9] + OUT:
        a, keep = _args()
        setattr(a, field, None)
        assert call(a) == 4 and "must be given" in message(), field
    for field in ("sh_in", "lh_in"):
        a, keep = _args(mode=2)
        setattr(a, field, None)
        assert call(a) == 4 and "sh_in and lh_in must be given with flux_mode 2" in message(), field
    for field in SCALARS:
        for value in (0.0, -1.0, float("nan")):
            a, keep = _args()
            setattr(a, field, value)
            assert call(a) == 4 and "must be positive" in message(), (field, value)
    for value in (1.0, 1.5):
        a, keep = _args()
        a.fb = value
        assert call(a) == 4 and "fb must lie inside (0, 1)" in message()
    # an output over an input: only x_out == x is in place
    partner = dict(zip(OUT, ("t", "q", "u", "v")))
    for out in OUT + DIAG:
        for inp in IN:
            if partner.get(out) == inp:
                continue
            a, keep = _args()
            setattr(a, out, keep[inp].ctypes.data)
            assert call(a) == 4 and "%s aliases an input" % out in message(), (out, inp)
    a, keep = _args()
    a.t_out = keep["t"].ctypes.data + 8      # in place means exactly in place
    assert call(a) == 4 and "t_out aliases an input" in message()
    a, keep = _args()
    a.v_out = keep["pint"].ctypes.data + 8 * 14      # the last row of pint: inside the array, not at its start
    assert call(a) == 4 and "v_out aliases an input" in message()
    a, keep = _args()
    a.q_out = keep["t_out"].ctypes.data
    assert call(a) == 4 and "q_out overlaps t_out" in message()
    a, keep = _args()
    a.lh_out = keep["sh_out"].ctypes.data + 8
    assert call(a) == 4 and "lh_out overlaps sh_out" in message()
    a, keep = _args()
    a.height = keep["u_out"].ctypes.data + 8
    assert call(a) == 4 and "height overlaps u_out" in message()


# ---- the numpy statement against the reference's own kernel ------------------------------------------------------------------------
@pytest.mark.parametrize("mode", X.MODES)
@pytest.mark.parametrize("name", X.CASES)
def test_statement_equals_the_reference_fixture(name, mode):
    """tests/golden/boundary_layer_<case>_<mode>.npz: inputs and what the reference's _boundary_layer_kernel made of them under
    plain numpy.  Not required bit for bit: the reference runs np.power on arrays where the statement runs scalar pow."""
    z = np.load(os.path.join(GOLDEN, "boundary_layer_%s_%d.npz" % (name, mode)))
    c = X.case(name, *z["t"].shape, mode)
    for k in X.INPUTS:
        assert X.same_bits(z[k], c[k]), k      # the fixture's inputs are the case builder's
    assert float(z["margin"]) >= X.MIN_MARGIN and float(z["margin"]) == c["margin"]
    ref = {k: z["ref_" + k] for k in X.PROFILES + X.DIAGNOSTICS}
    dev = X.deviations(ref, c)
    print("%s, mode %d: statement against the reference, bits equal: %s, largest deviation / scale %.3e" % (
        name, mode, all(X.same_bits(ref[k], c[k]) for k in ref), max(dev.values())))
    assert set(dev) == set(X.PROFILES + X.DIAGNOSTICS)
    for k, v in dev.items():
        assert v <= X.TOL, (k, v)
    if name == "decoupled" and mode == 0:
        assert all(X.same_bits(ref[k + "_new"], c[k]) for k in "tquv")


# ---- physics that pins the rule ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", X.CASES)
def test_budgets_close(name):
    """Mode 0 conserves sum(x dp) of all four fields; in modes 1 and 2 the column's enthalpy and water change by the sensible and
    latent flux (the diagnosed ones, resp. the prescribed ones) times dt, and its momentum by the stress times dt."""
    k = X.CONSTANTS
    for nlay, ncol in ((2, 65), (3, 1), (30, 130), (61, 63)):
        c = X.case(name, nlay, ncol, 0)
        for x in "tquv":
            before, after = X.column_integrals(c[x], c["p_int"]), X.column_integrals(c[x + "_new"], c["p_int"])
            scale = X.column_integrals(np.abs(c[x]), c["p_int"])
            assert float((np.abs(after - before) / scale).max()) <= 1e-12, (name, nlay, ncol, x)
        for mode in (1, 2):
            c = X.case(name, nlay, ncol, mode)
            # the change of a column integral as the integral of the change: the difference of two integrals of ~1e8 J m^-2 would
            # itself be uncertain by more than the bound on a change of ~1e4
            change = lambda x: X.column_integrals(c[x + "_new"] - c[x], c["p_int"]) / k["g"]
            sh, lh = (c["sh"], c["lh"]) if mode == 1 else (c["sh_in"], c["lh_in"])
            for got, want, what in ((k["cp"] * change("t"), sh * X.DT, "enthalpy"), (k["lv"] * change("q"), lh * X.DT, "water"),
                                    (-change("v"), c["stress_north"] * X.DT, "northward momentum"), (-change("u"), c["stress_east"] * X.DT, "eastward momentum")):
                larger = np.maximum(np.abs(got), np.abs(want))      # (both are exactly 0 where C == 0)
                worst = float(np.max(np.abs(got - want) / np.where(larger > 0, larger, 1.0)))
                assert worst <= 1e-10, (name, nlay, ncol, mode, what, worst)
    if name == "no_top":      # the quirk: nothing diffuses, the surface exchange acts on layer 0 alone
        c = X.case(name, 30, 65, 1)
        assert X.same_bits(c["t_new"][1:], c["t"][1:]) and (c["t_new"][0] > c["t"][0]).all() and (c["sh"] > 0).all()


# ---- the stand-alone host program -----------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def program(tmp_path_factory):
    return build_host_program(tmp_path_factory, "boundary_layer_check.cpp", flags=["-ffp-contract=off"])


@pytest.fixture(scope="module")
def program_sanitized(tmp_path_factory):
    return build_host_program(tmp_path_factory, "boundary_layer_check.cpp", sanitized=True, flags=["-ffp-contract=off"])


def run_program(exe, tmp_path, arrays, mode, dt=X.DT, constants=X.CONSTANTS, in_place=False, pressure_scale=1.0, ps_scale=1.0):
    """arrays: the eleven inputs in the order of X.INPUTS -> dict of the four profiles and five diagnostics."""
    fin, fout = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    nlay, ncol = arrays[0].shape
    head = [float(in_place), float(mode), dt] + [constants[n] for n in X.CONSTANT_NAMES] + [pressure_scale, ps_scale]
    np.concatenate([head] + [np.asarray(v, dtype=np.float64).ravel() for v in arrays]).tofile(fin)
    r = subprocess.run([exe, str(ncol), str(nlay), fin, fout], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.startswith("ok"), (r.returncode, r.stdout, r.stderr)
    flat, nl = np.fromfile(fout), nlay * ncol
    assert flat.size == 4 * nl + 5 * ncol
    got = {n: flat[i * nl:(i + 1) * nl].reshape(nlay, ncol) for i, n in enumerate(X.PROFILES)}
    got.update({n: flat[4 * nl + i * ncol:4 * nl + (i + 1) * ncol] for i, n in enumerate(X.DIAGNOSTICS)})
    return got


def check_program(exe, tmp_path, name, nlay, ncol, mode, in_place):
    """-> the largest deviation / scale from the statement.  (The program itself checks in place == out of place bit for bit.)"""
    c = X.case(name, nlay, ncol, mode)
    got = run_program(exe, tmp_path, [c[k] for k in X.INPUTS], mode, in_place=in_place)
    dev = X.deviations(got, c)
    assert len(dev) == 9
    for k, v in dev.items():
        assert v <= X.TOL, (name, nlay, ncol, mode, k, v)
    if name == "decoupled" and mode == 0:
        assert all(X.same_bits(got[k + "_new"], c[k]) for k in "tquv")
    return max(dev.values())


@pytest.mark.parametrize("name", X.CASES)
def test_host_program_equals_the_numpy_statement(program, tmp_path, name):
    worst = 0.0
    for mode in X.MODES:
        for i, (nlay, ncol) in enumerate(SHAPES):
            worst = max(worst, check_program(program, tmp_path, name, nlay, ncol, mode, in_place=i % 2))
    print("boundary_layer_check, %s: largest deviation / scale from the statement %.3e" % (name, worst))


def test_host_program_under_the_address_and_undefined_behaviour_sanitizers(program_sanitized, tmp_path):
    """The same program built with -fsanitize=address,undefined and run stand-alone, clean."""
    for name in X.CASES:
        for mode in X.MODES:
            for nlay, ncol in ((2, 1), (2, 65), (3, 64), (30, 63), (61, 130)):
                check_program(program_sanitized, tmp_path, name, nlay, ncol, mode, in_place=(nlay + mode) % 2)


# ---- the component on host states: the host program stands in for the context ------------------------------------------------------
class ProgramContext:
    """Context.boundary_layer (host arrays) by the stand-alone host program."""

    def __init__(self, exe, tmp_path):
        self.exe, self.tmp_path, self.calls = exe, tmp_path, []

    def boundary_layer(self, t, q, u, v, pmid, pint, ps, ts, qs, dt, constants, flux_mode, sh_in=None, lh_in=None, **kwargs):
        assert not kwargs and (flux_mode == 2) == (sh_in is not None) == (lh_in is not None)
        self.calls.append((t.shape, dt, dict(constants), flux_mode))
        zeros = np.zeros(t.shape[1])
        got = run_program(self.exe, self.tmp_path, [t, q, u, v, pmid, pint, ps, ts, qs, zeros if sh_in is None else sh_in, zeros if lh_in is None else lh_in],
                          flux_mode, dt=dt, constants=constants)
        return got["t_new"], got["q_new"], got["u_new"], got["v_new"], dict(
            stress_north=got["stress_north"], stress_east=got["stress_east"], height=got["height"], sh_out=got["sh"], lh_out=got["lh"])


@pytest.mark.parametrize("surface_fluxes", [None, "bulk", "external"])
def test_component_on_a_host_state_with_other_units_and_a_3d_grid(program, tmp_path, surface_fluxes):
    """Pressures in hPa / mbar and a (lat, lon) grid, levels LAST in the state's arrays: the component hands the rule
    [levels][columns] in Pa, the reference's constants and the time step in seconds with it, and returns the statement's numbers."""
    nlay, ny, nx = 30, 5, 13
    mode = {None: 0, "bulk": 1, "external": 2}[surface_fluxes]
    c = X.case("varied", nlay, ny * nx, mode)
    lev = lambda a: np.ascontiguousarray(np.transpose(a.reshape(a.shape[0], ny, nx), (1, 2, 0)))
    q3 = lambda a, dim, units, f=1.0: DataArray(lev(a) / f, dims=("lat", "lon", dim), attrs={"units": units})
    q2 = lambda a, units, f=1.0: DataArray(a.reshape(ny, nx) / f, dims=("lat", "lon"), attrs={"units": units})
    state = {"air_temperature": q3(c["t"], "mid_levels", "degK"), "specific_humidity": q3(c["q"], "mid_levels", "kg/kg"),
             "eastward_wind": q3(c["u"], "mid_levels", "m s^-1"), "northward_wind": q3(c["v"], "mid_levels", "m/s"),
             "air_pressure": q3(c["p"], "mid_levels", "hPa", 100.0), "air_pressure_on_interface_levels": q3(c["p_int"], "interface_levels", "mbar", 100.0),
             "surface_air_pressure": q2(c["ps"], "mbar", 100.0), "surface_temperature": q2(c["ts"], "degK"),
             "surface_specific_humidity": q2(c["qs"], "kg/kg"), "time": datetime.datetime(2000, 1, 1)}
    if mode == 2:
        state.update({FLUXES[0]: q2(c["sh_in"], "W m^-2"), FLUXES[1]: q2(c["lh_in"], "W m^-2")})
    ctx = ProgramContext(program, tmp_path)
    bl = climt_amd.SimpleBoundaryLayer(surface_fluxes=surface_fluxes, context=ctx)
    diagnostics, new_state = bl(state, datetime.timedelta(seconds=X.DT))
    assert ctx.calls == [((nlay, ny * nx), X.DT, X.CONSTANTS, mode)]
    # hPa -> Pa on the way in costs a rounding per pressure: the statement on the pressures the component formed
    back = lambda a: (a / 100.0) * 100.0
    want = X.statement(c["t"], c["q"], c["u"], c["v"], back(c["p"]), back(c["p_int"]), back(c["ps"]), c["ts"], c["qs"], mode, c["sh_in"], c["lh_in"])
    assert want["margin"] >= X.MIN_MARGIN
    want = dict(c, **want)
    names = {"air_temperature": ("t_new", "degK"), "specific_humidity": ("q_new", "kg/kg"), "eastward_wind": ("u_new", "m s^-1"),
             "northward_wind": ("v_new", "m s^-1")}
    assert set(new_state) == set(names)
    got = {}
    for name, (key, units) in names.items():
        x = new_state[name]
        assert x.attrs["units"] == units and set(x.dims) == {"mid_levels", "lat", "lon"}
        got[key] = np.transpose(x.values, [x.dims.index(d) for d in ("mid_levels", "lat", "lon")]).reshape(nlay, ny * nx)
    dnames = {"northward_wind_stress": ("stress_north", "Pa"), "eastward_wind_stress": ("stress_east", "Pa"), "boundary_layer_height": ("height", "m")}
    if mode == 1:
        dnames.update({FLUXES[0]: ("sh", "W m^-2"), FLUXES[1]: ("lh", "W m^-2")})
    assert set(diagnostics) == set(dnames)
    for name, (key, units) in dnames.items():
        x = diagnostics[name]
        assert x.attrs["units"] == units and tuple(x.dims) == ("lat", "lon")
        got[key] = x.values.reshape(ny * nx)
    dev = X.deviations(got, want)
    assert len(dev) == 4 + len(dnames)
    for k, v in dev.items():
        assert v <= X.TOL, (k, v)
    assert not X.same_bits(got["t_new"], c["t"])


@pytest.mark.parametrize("desc", ["column", "3d"])
def test_reference_cache_default_state(program, tmp_path, desc):
    """TestSimpleBoundaryLayer-{column,3d}-{0,1}.cache: the diagnostics and the new state of the reference's default state.
    Here: get_default_state for the component on the cache's grid, through the component, to the reference's own criterion."""
    _, want_diag, want_out = load_cache_case("TestSimpleBoundaryLayer", desc)
    assert set(want_out) == {"air_temperature", "specific_humidity", "northward_wind", "eastward_wind"}
    assert set(want_diag) == {"northward_wind_stress", "eastward_wind_stress", "boundary_layer_height"} | set(FLUXES)
    nz, ny, nx = want_out["air_temperature"].values.shape
    bl = climt_amd.SimpleBoundaryLayer(context=ProgramContext(program, tmp_path))
    state = climt_amd.get_default_state([bl], grid_state=climt_amd.get_grid(nx=nx, ny=ny, nz=nz))
    diagnostics, new_state = bl(state, datetime.timedelta(seconds=10))
    assert set(diagnostics) == set(want_diag) and set(new_state) == set(want_out)
    for got_all, want_all in ((diagnostics, want_diag), (new_state, want_out)):
        for name, want in want_all.items():
            got = got_all[name]
            assert climt_amd.device_state._same_units(got.attrs["units"], want.attrs["units"]), name      # ("W m^-2" is the cache's "W/m**2")
            g = np.transpose(got.values, [got.dims.index(d) for d in want.dims])
            assert g.shape == want.values.shape, name
            assert np.isclose(g, want.values, rtol=1e-8, atol=1e-8).all(), name      # the reference's own criterion (rtol 1e-8), its atol 1e-6 tightened
