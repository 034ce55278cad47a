"""The dry convective adjustment without a GPU: the exported symbol, the header and the ctypes layer; the argument checks of the C
entry; the numpy statement (tests/dry_adjust_cases.py) against fixtures made by the reference's own loop; the stand-alone host
program of the column sweep (tools/dry_adjust_check.cpp on csrc/rrtmg_dry_adjust.h) against the statement -- once more under the
host sanitizers; and climt_amd.DryConvectiveAdjustment on host states, the host program standing in for the context."""
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

import dry_adjust_cases as X

SYMBOL = "rrtmg_hip_dry_adjustment"
HEADER_STRUCT = ("typedef struct { uint32_t struct_size; int32_t ncol, nlay, memspace; const double *t, *q, *pmid; /* [nlay][ncol] */ "
                 "const double *pint; /* [nlay+1][ncol] */ double cpd, cvap, rd, rv, pref; "
                 "double *t_out, *q_out; /* [nlay][ncol]; t_out may be t, q_out may be q (in place) */ "
                 "int32_t *mixed_top; /* [ncol], or NULL */ } rrtmg_dry_adjust;")
SHAPES = [(nlay, ncol) for nlay in X.NLAYS for ncol in X.NCOLS]


def test_symbol_header_and_python_layer():
    syms = subprocess.check_output(["nm", "-D", "--defined-only", _lib.LIB_PATH]).decode()
    assert re.search(r" T %s\b" % SYMBOL, syms)
    hdr = open(os.path.join(ROOT, "include", "rrtmg_hip.h")).read()
    flat = " ".join(hdr.split())
    assert HEADER_STRUCT in flat
    assert "int rrtmg_hip_dry_adjustment(rrtmg_ctx *ctx, const rrtmg_dry_adjust *a);" in flat
    assert "#define RRTMG_HIP_ABI_VERSION 5" in hdr      # probed by symbol
    lib = _lib.load_library()
    assert hasattr(lib, SYMBOL) and lib.rrtmg_hip_abi_version() == 5
    assert lib.rrtmg_hip_dry_adjustment.argtypes == [C.c_void_p, C.POINTER(_lib.DryAdjust)]
    # the ctypes struct, field for field against the header's declaration order
    p, d, i = C.c_void_p, C.c_double, C.c_int32
    want = ([("struct_size", C.c_uint32), ("ncol", i), ("nlay", i), ("memspace", i), ("t", p), ("q", p), ("pmid", p), ("pint", p)]
            + [(n, d) for n in "cpd cvap rd rv pref".split()] + [("t_out", p), ("q_out", p), ("mixed_top", p)])
    assert [(n, t) for n, t in _lib.DryAdjust._fields_] == want
    body = re.sub(r"/\*.*?\*/", "", HEADER_STRUCT.split("{", 1)[1].rsplit("}", 1)[0])
    declared = [n for n in re.findall(r"\*?(\w+)\s*[,;]", body)]
    assert declared == [n for n, _ in want]
    assert C.sizeof(_lib.DryAdjust) == 16 + 4 * 8 + 5 * 8 + 3 * 8
    assert lib.rrtmg_hip_dry_adjustment(None, C.byref(_lib.DryAdjust())) == 4      # a NULL context is an argument error
    sig = inspect.signature(_lib.Context.dry_adjustment)
    assert list(sig.parameters) == ["self", "t", "q", "pmid", "pint", "constants", "t_out", "q_out", "mixed_top", "memspace", "ncol", "nlay"]
    assert isinstance(_lib.Context.has_dry_adjustment, property)
    assert "DryConvectiveAdjustment" in climt_amd.__all__
    assert list(inspect.signature(climt_amd.device_state.dry_adjustment_device_call).parameters) == ["self", "ds", "timestep"]
    src = open(os.path.join(ROOT, "climt_amd", "csrc", "rrtmg_dry_adjust.hip")).read()
    assert re.search(r"__launch_bounds__\(64\)\s+dry_adjust_kernel", src)
    for text in (src, open(os.path.join(ROOT, "climt_amd", "csrc", "rrtmg_dry_adjust.h")).read()):
        code = re.sub(r"//[^\n]*", "", text)
        assert not re.search(r"\bwhile\b", code)      # every loop is a for bounded by nlay


def test_property_dictionaries_are_the_references():
    c = climt_amd.DryConvectiveAdjustment
    lev = lambda units, dim: {"units": units, "dims": [dim, "*"]}
    assert c.input_properties == {
        "air_temperature": lev("degK", "mid_levels"), "air_pressure": lev("Pa", "mid_levels"),
        "air_pressure_on_interface_levels": dict(lev("Pa", "interface_levels"), alias="P_int"),
        "specific_humidity": lev("kg/kg", "mid_levels")}
    assert c.output_properties == {"air_temperature": {"units": "degK"}, "specific_humidity": {"units": "kg/kg"}}
    assert c.diagnostic_properties == {}
    assert c.constants() == X.CONSTANTS
    assert c.constants("mbar")["pref"] == pytest.approx(1013.2, rel=1e-15)
    assert "array_call" in vars(c) and list(inspect.signature(c.array_call).parameters) == ["self", "state", "time_step"]


# ---- the C entry's argument checks (a context made without a GPU reports errors) ------------------------------------------------------
@pytest.fixture()
def bare_context():
    lib = _lib.load_library()
    h = C.c_void_p()
    lib.rrtmg_hip_create(C.byref(h), 0)
    assert h.value
    yield lib, h
    lib.rrtmg_hip_destroy(h)


def _args(ncol=4, nlay=3):
    """A well-formed struct over host memory (the checks under test come before anything is dereferenced or enqueued)."""
    a, keep = _lib.DryAdjust(), {}
    a.struct_size, a.ncol, a.nlay, a.memspace = C.sizeof(_lib.DryAdjust), ncol, nlay, 0
    for n in ("t", "q", "pmid", "pint", "t_out", "q_out"):
        keep[n] = np.zeros((nlay + 1) * ncol)
        setattr(a, n, keep[n].ctypes.data)
    keep["mixed_top"] = np.zeros(ncol, dtype=np.int32)
    a.mixed_top = keep["mixed_top"].ctypes.data
    for n, v in X.CONSTANTS.items():
        setattr(a, n, v)
    return a, keep


def test_the_entry_refuses_bad_arguments(bare_context):
    lib, h = bare_context
    call = lambda a: lib.rrtmg_hip_dry_adjustment(h, C.byref(a))
    message = lambda: lib.rrtmg_hip_last_error(h).decode()
    assert lib.rrtmg_hip_dry_adjustment(h, None) == 4 and "NULL argument struct" in message()
    for size in (0, C.sizeof(_lib.DryAdjust) - 8, C.sizeof(_lib.DryAdjust) + 8):
        a, keep = _args()
        a.struct_size = size
        assert call(a) == 4 and "struct_size" in message()
    for field, value in (("ncol", 0), ("ncol", -1), ("nlay", 0), ("nlay", -3)):
        a, keep = _args()
        setattr(a, field, value)
        assert call(a) == 4 and "positive" in message()
    for value in (-1, 2):
        a, keep = _args()
        a.memspace = value
        assert call(a) == 4 and "memspace" in message()
    for field in ("t", "q", "pmid", "pint", "t_out", "q_out"):
        a, keep = _args()
        setattr(a, field, None)
        assert call(a) == 4 and "must be given" in message(), field
    for field, value in (("cpd", 0.0), ("rd", -287.0), ("pref", 0.0), ("pref", float("nan")), ("cvap", -1.0), ("rv", -1.0)):
        a, keep = _args()
        setattr(a, field, value)
        assert call(a) == 4 and "must be positive" in message(), field
    # an output over an input: only t_out == t and q_out == q are in place
    for out in ("t_out", "q_out", "mixed_top"):
        for inp in ("t", "q", "pmid", "pint"):
            if (out, inp) in (("t_out", "t"), ("q_out", "q")):
                continue
            a, keep = _args()
            setattr(a, out, keep[inp].ctypes.data)
            assert call(a) == 4 and "%s aliases an input" % out in message(), (out, inp)
    a, keep = _args()
    a.t_out = keep["t"].ctypes.data + 8      # in place means exactly in place
    assert call(a) == 4 and "t_out aliases an input" in message()
    a, keep = _args()
    a.q_out = keep["pint"].ctypes.data + 8 * 14      # the last row of pint: inside the array, not at its start
    assert call(a) == 4 and "q_out aliases an input" in message()
    a, keep = _args()
    a.q_out = keep["t_out"].ctypes.data
    assert call(a) == 4 and "q_out overlaps t_out" in message()
    a, keep = _args()
    a.mixed_top = keep["q_out"].ctypes.data + 8
    assert call(a) == 4 and "mixed_top overlaps q_out" in message()


# ---- the numpy statement against the reference's own loop ------------------------------------------------------------------------
@pytest.mark.parametrize("name", X.CASES)
def test_statement_equals_the_reference_fixture(name):
    """tests/golden/dry_adjust_<case>.npz: inputs and what the reference's _dry_adj_kernel_np made of them under plain numpy."""
    z = np.load(os.path.join(GOLDEN, "dry_adjust_%s.npz" % name))
    c = X.case(name, *z["t"].shape)
    for k in ("t", "q", "p", "p_int"):
        assert X.same_bits(z[k], c[k]), k      # the fixture's inputs are the case builder's
    assert float(z["margin"]) >= X.MIN_MARGIN and float(z["margin"]) == c["margin"]
    assert X.rel_err(c["t_new"], z["t_new"]) <= X.TOL
    assert float(np.abs(c["q_new"] - z["q_new"]).max()) <= X.TOL * max(float(np.abs(z["q_new"]).max()), 1e-300)
    # the same expressions on the same operands in the same order: in fact the same bits
    assert X.same_bits(c["t_new"], z["t_new"]) and X.same_bits(c["q_new"], z["q_new"])


@pytest.mark.parametrize("name", X.CASES)
def test_mixing_conserves_enthalpy_and_water(name):
    for nlay, ncol in ((2, 65), (30, 130), (61, 63)):
        c = X.case(name, nlay, ncol)
        h0, w0 = X.column_sums(c["t"], c["q"], c["p_int"])
        h1, w1 = X.column_sums(c["t_new"], c["q_new"], c["p_int"])
        assert float(np.abs(h1 / h0 - 1.0).max()) <= 1e-12
        assert float(np.abs(w1 - w0).max()) <= 1e-12 * float(np.abs(w0).max()) or not w0.any()


# ---- the stand-alone host program -----------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def program(tmp_path_factory):
    return build_host_program(tmp_path_factory, "dry_adjust_check.cpp", flags=["-ffp-contract=off"])


@pytest.fixture(scope="module")
def program_sanitized(tmp_path_factory):
    return build_host_program(tmp_path_factory, "dry_adjust_check.cpp", sanitized=True, flags=["-ffp-contract=off"])


def run_program(exe, tmp_path, t, q, p, p_int, in_place=False, constants=X.CONSTANTS):
    fin, fout = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    nlay, ncol = t.shape
    head = [float(in_place)] + [constants[n] for n in ("cpd", "cvap", "rd", "rv", "pref")]
    np.concatenate([head] + [np.asarray(v, dtype=np.float64).ravel() for v in (t, q, p, p_int)]).tofile(fin)
    r = subprocess.run([exe, str(ncol), str(nlay), fin, fout], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.startswith("ok"), (r.returncode, r.stdout, r.stderr)
    flat, nl = np.fromfile(fout), nlay * ncol
    assert flat.size == 2 * nl + ncol
    return flat[:nl].reshape(nlay, ncol), flat[nl:2 * nl].reshape(nlay, ncol), flat[2 * nl:].astype(np.int32)


def check_program(exe, tmp_path, name, nlay, ncol, in_place):
    """-> the largest relative deviation of T from the statement.  (The program itself checks in place == out of place bit for
    bit, and that a column no mixing wrote has the bits of its input.)"""
    c = X.case(name, nlay, ncol)
    t, q, top = run_program(exe, tmp_path, c["t"], c["q"], c["p"], c["p_int"], in_place)
    assert (top == c["mixed_top"]).all(), (name, nlay, ncol)
    err = X.rel_err(t, c["t_new"])
    assert err <= X.TOL, (name, nlay, ncol, err)
    assert float(np.abs(q - c["q_new"]).max()) <= X.TOL * max(float(np.abs(c["q_new"]).max()), 1e-300), (name, nlay, ncol)
    if name == "stable":
        assert X.same_bits(t, c["t"]) and X.same_bits(q, c["q"]) and (top == -1).all()
    return err


@pytest.mark.parametrize("name", X.CASES)
def test_host_program_equals_the_numpy_statement(program, tmp_path, name):
    worst = 0.0
    for i, (nlay, ncol) in enumerate(SHAPES):
        worst = max(worst, check_program(program, tmp_path, name, nlay, ncol, in_place=i % 2))
    print("dry_adjust_check, %s: largest relative deviation from the statement %.3e" % (name, worst))


def test_host_program_under_the_address_and_undefined_behaviour_sanitizers(program_sanitized, tmp_path):
    """The same program built with -fsanitize=address,undefined and run stand-alone, clean."""
    for name in X.CASES:
        for nlay, ncol in ((1, 1), (2, 65), (3, 64), (30, 63), (61, 130)):
            for in_place in (0, 1):
                check_program(program_sanitized, tmp_path, name, nlay, ncol, in_place)


# ---- the component on host states: the host program stands in for the context ------------------------------------------------------
class ProgramContext:
    """Context.dry_adjustment (host arrays) by the stand-alone host program."""

    def __init__(self, exe, tmp_path):
        self.exe, self.tmp_path, self.calls = exe, tmp_path, []

    def dry_adjustment(self, t, q, pmid, pint, constants, **kwargs):
        assert not kwargs
        self.calls.append((t.shape, dict(constants)))
        return run_program(self.exe, self.tmp_path, t, q, pmid, pint, constants=constants)


def test_component_on_a_host_state_with_other_units_and_a_3d_grid(program, tmp_path):
    """Pressures in hPa and a (lat, lon) grid, levels LAST in the state's arrays: the component hands the sweep [levels][columns]
    in Pa, the reference's constants with it, and returns the statement's numbers."""
    nlay, ny, nx = 30, 5, 13
    c = X.case("moist", nlay, ny * nx)
    to_state = lambda a: np.ascontiguousarray(np.transpose(a.reshape(a.shape[0], ny, nx), (1, 2, 0)))
    hpa = lambda a: to_state(a) / 100.0
    state = {"air_temperature": DataArray(to_state(c["t"]), dims=("lat", "lon", "mid_levels"), attrs={"units": "degK"}),
             "specific_humidity": DataArray(to_state(c["q"]), dims=("lat", "lon", "mid_levels"), attrs={"units": "kg/kg"}),
             "air_pressure": DataArray(hpa(c["p"]), dims=("lat", "lon", "mid_levels"), attrs={"units": "hPa"}),
             "air_pressure_on_interface_levels": DataArray(hpa(c["p_int"]), dims=("lat", "lon", "interface_levels"), attrs={"units": "mbar"}),
             "time": datetime.datetime(2000, 1, 1)}
    ctx = ProgramContext(program, tmp_path)
    dry = climt_amd.DryConvectiveAdjustment(context=ctx)
    diagnostics, new_state = dry(state, datetime.timedelta(minutes=10))
    assert diagnostics == {} and set(new_state) == {"air_temperature", "specific_humidity"}
    assert ctx.calls == [((nlay, ny * nx), X.CONSTANTS)]
    # hPa -> Pa on the way in costs a rounding per pressure: the statement on the pressures the component formed
    p, p_int = (c["p"] / 100.0) * 100.0, (c["p_int"] / 100.0) * 100.0
    t_new, q_new, margin, _ = X.statement(c["t"], c["q"], p, p_int)
    assert margin >= X.MIN_MARGIN
    for name, want, units in (("air_temperature", t_new, "degK"), ("specific_humidity", q_new, "kg/kg")):
        got = new_state[name]
        assert got.attrs["units"] == units and set(got.dims) == {"mid_levels", "lat", "lon"}
        g = np.transpose(got.values, [got.dims.index(d) for d in ("mid_levels", "lat", "lon")]).reshape(nlay, ny * nx)
        assert X.rel_err(g, want) <= X.TOL, name
    assert X.rel_err(t_new, c["t_new"]) < 1e-9 and not X.same_bits(state["air_temperature"].values, new_state["air_temperature"].values)


@pytest.mark.parametrize("desc", ["column", "3d"])
def test_reference_cache_default_state_is_left_as_it_is(program, tmp_path, desc):
    """TestDryConvection-{column,3d}-{0,1}.cache: no diagnostics, and the new state of the reference's default state -- which is
    that state.  Here: get_default_state for the component on the cache's grid, through the component."""
    _, none, out = load_cache_case("TestDryConvection", desc)
    assert none == {} and set(out) == {"air_temperature", "specific_humidity"}
    nz, ny, nx = out["air_temperature"].values.shape
    dry = climt_amd.DryConvectiveAdjustment(context=ProgramContext(program, tmp_path))
    state = climt_amd.get_default_state([dry], grid_state=climt_amd.get_grid(nx=nx, ny=ny, nz=nz))
    diagnostics, new_state = dry(state, datetime.timedelta(seconds=10))
    assert diagnostics == {}
    for name, want in out.items():
        got = new_state[name]
        assert got.attrs["units"] == want.attrs["units"]
        g = np.transpose(got.values, [got.dims.index(d) for d in want.dims])
        assert g.shape == want.values.shape and float(np.abs(g - want.values).max()) <= 1e-8      # the reference's own criterion
        s = state[name]
        assert X.same_bits(g, np.transpose(s.values, [s.dims.index(d) for d in want.dims]).astype(np.float64))
