"""The gray radiation path without a GPU: the exported symbols, the header and the ctypes layer; the property dictionaries and
keyword defaults against tests/golden/gray_interface.json (read off the reference's source by the maker); every refusal of the
three C entries; the numpy statements (tests/gray_cases.py) against fixtures made by the reference's own functions; the
stand-alone host program (tools/gray_check.cpp on csrc/rrtmg_gray.h) against the statements -- once more under the host
sanitizers; the three tables it prints against the header and climt_amd/_lib.py; and the three components on host states, the host
program standing in for the context.

Measured (tests/golden/make_gray_golden.py, numpy on glibc): the statements against the reference's _frierson_tau_kernel_np,
_gray_lw_kernel_np with the heating lines of array_call, and _gsc_kernel_np are bit-identical on all 36 fixtures (6 + 6 cases x 3
shapes), recurrences and heating lines included.  The reference under +-1 ulp of every input moves by at most 3.6e-15 (depth),
2.0e-14 (up), 2.3e-15 (dn; 4.8e-13 W m^-2 absolute where dn is zero), 4.7e-13 (tendency and heating rate: the isothermal case,
where the divergence is a small difference of large fluxes), 2.0e-16 (t), 2.0e-15 (q) of the column's largest magnitude and
7.8e-14 of the precipitation; the stored tolerances are 16 x the figure of each file, at least 1e-13.
Host program against the statements (g++ -O1, glibc): see what test_host_program_equals_the_numpy_statements prints."""
import ctypes as C
import datetime
import inspect
import json
import os
import re
import subprocess

import numpy as np
import pytest

import climt_amd
from climt_amd import _lib
from climt_amd._sympl_compat import DataArray
from helpers import GOLDEN, ROOT, assert_column_rows_agree, build_host_program, column_table_rows, header_pointer_members

import gray_cases as X

SYMBOLS = ("rrtmg_hip_frierson_optical_depth", "rrtmg_hip_gray_longwave", "rrtmg_hip_grid_scale_condensation")
HEADER_STRUCTS = {
    "rrtmg_frierson_optical_depth": ("typedef struct { uint32_t struct_size; int32_t ncol, nlay, memspace; const double *pint; /* [nlay+1][ncol] */ "
                                     "const double *ps, *lat; /* [ncol] */ double tau0e, tau0p, fl; double pressure_scale, ps_scale; "
                                     "double *tau; /* [nlay+1][ncol] */ } rrtmg_frierson_optical_depth;"),
    "rrtmg_gray_longwave": ("typedef struct { uint32_t struct_size; int32_t ncol, nlay, memspace; int32_t frierson, reserved; /* reserved: 0 */ "
                            "const double *t; /* [nlay][ncol] */ const double *tsfc; /* [ncol] */ "
                            "const double *pint, *tau; /* [nlay+1][ncol]; tau may be NULL with frierson 1 */ "
                            "const double *ps, *lat; /* [ncol]; each may be NULL with frierson 0 */ double tau0e, tau0p, fl, sigma_sb, g, cpd; "
                            "double pressure_scale, ps_scale; double *up, *dn; /* [nlay+1][ncol] */ double *tend; /* [nlay][ncol] */ "
                            "double *hr; /* [nlay][ncol], or NULL */ double *tau_out; /* [nlay+1][ncol], or NULL */ } rrtmg_gray_longwave;"),
    "rrtmg_grid_scale_condensation": ("typedef struct { uint32_t struct_size; int32_t ncol, nlay, memspace; const double *t, *q, *pmid; /* [nlay][ncol] */ "
                                      "const double *pint; /* [nlay+1][ncol] */ double cpd, lv, rd, rh2o, g, rhow; double pressure_scale; "
                                      "double *t_out, *q_out; /* [nlay][ncol]; each may be its own input (in place) */ "
                                      "double *precip; /* [ncol], or NULL */ } rrtmg_grid_scale_condensation;"),
}
STRUCTS = {"rrtmg_frierson_optical_depth": ("FRIERSON", _lib.FriersonOpticalDepth, "frierson_optical_depth"),
           "rrtmg_gray_longwave": ("GRAY_LONGWAVE", _lib.GrayLongwave, "gray_longwave"),
           "rrtmg_grid_scale_condensation": ("GRID_SCALE_CONDENSATION", _lib.GridScaleCondensation, "grid_scale_condensation")}
IN_PLACE = {"rrtmg_frierson_optical_depth": {}, "rrtmg_gray_longwave": {}, "rrtmg_grid_scale_condensation": {"t_out": "t", "q_out": "q"}}
SHAPES = [(nlay, ncol) for nlay in X.NLAYS for ncol in X.NCOLS]
TAU = "longwave_optical_depth_on_interface_levels"


def _tuples(prefix):
    return tuple(getattr(_lib, "%s_%s" % (prefix, k)) for k in ("IN", "OUT", "DIAG"))


def test_symbols_header_and_python_layer():
    syms = subprocess.check_output(["nm", "-D", "--defined-only", _lib.LIB_PATH]).decode()
    hdr = open(os.path.join(ROOT, "include", "rrtmg_hip.h")).read()
    flat = " ".join(hdr.split())
    assert "#define RRTMG_HIP_ABI_VERSION 5" in hdr      # probed by symbol
    lib = _lib.load_library()
    assert lib.rrtmg_hip_abi_version() == 5
    p, d, i = C.c_void_p, C.c_double, C.c_int32
    head = [("struct_size", C.c_uint32)] + [(n, i) for n in ("ncol", "nlay", "memspace")]
    scales = [("pressure_scale", d), ("ps_scale", d)]
    want = {"rrtmg_frierson_optical_depth": head + [(n, p) for n in ("pint", "ps", "lat")] + [(n, d) for n in ("tau0e", "tau0p", "fl")] + scales + [("tau", p)],
            "rrtmg_gray_longwave": head + [("frierson", i), ("reserved", i)] + [(n, p) for n in ("t", "tsfc", "pint", "tau", "ps", "lat")]
            + [(n, d) for n in ("tau0e", "tau0p", "fl", "sigma_sb", "g", "cpd")] + scales + [(n, p) for n in ("up", "dn", "tend", "hr", "tau_out")],
            "rrtmg_grid_scale_condensation": head + [(n, p) for n in ("t", "q", "pmid", "pint")] + [(n, d) for n in ("cpd", "lv", "rd", "rh2o", "g", "rhow")]
            + scales[:1] + [(n, p) for n in ("t_out", "q_out", "precip")]}
    for (struct, (prefix, ctype, entry)), symbol in zip(STRUCTS.items(), SYMBOLS):
        assert re.search(r" T %s\b" % symbol, syms) and symbol == "rrtmg_hip_" + entry
        assert HEADER_STRUCTS[struct] in flat
        assert "int %s(rrtmg_ctx *ctx, const %s *a);" % (symbol, struct) in flat
        assert "Probe for it by symbol; RRTMG_HIP_ABI_VERSION is unchanged. */ " + HEADER_STRUCTS[struct][:40] in flat
        assert getattr(lib, symbol).argtypes == [C.c_void_p, C.POINTER(ctype)]
        # the ctypes struct, field for field against the header's declaration order
        assert [(n, t) for n, t in ctype._fields_] == want[struct]
        body = re.sub(r"/\*.*?\*/", "", HEADER_STRUCTS[struct].split("{", 1)[1].rsplit("}", 1)[0])
        assert re.findall(r"\*?(\w+)\s*[,;]", body) == [n for n, _ in want[struct]]
        assert C.sizeof(ctype) == sum(C.sizeof(t) for _, t in want[struct])      # no padding
        assert getattr(lib, symbol)(None, C.byref(ctype())) == 4      # a NULL context is an argument error
        IN, OUT, DIAG = _tuples(prefix)
        assert [n for n, t in want[struct] if t is p] == list(IN + OUT + DIAG)
        assert (_lib.COLUMN_ARRAYS[entry]["IN"], _lib.COLUMN_ARRAYS[entry]["DIAG"]) == (IN, DIAG)
    assert isinstance(_lib.Context.has_gray_radiation, property)
    sig = inspect.signature(_lib.Context.gray_longwave)
    assert list(sig.parameters)[:9] == ["self", "t", "tsfc", "pint", "constants", "tau", "ps", "lat", "frierson"] and list(sig.parameters)[-3:] == ["memspace", "ncol", "nlay"]
    assert list(inspect.signature(_lib.Context.frierson_optical_depth).parameters)[:5] == ["self", "pint", "ps", "lat", "parameters"]
    assert list(inspect.signature(_lib.Context.grid_scale_condensation).parameters)[:6] == ["self", "t", "q", "pmid", "pint", "constants"]
    for name in ("GrayLongwaveRadiation", "Frierson06LongwaveOpticalDepth", "GridScaleCondensation"):
        assert name in climt_amd.__all__ and hasattr(climt_amd, name)
    src = open(os.path.join(ROOT, "climt_amd", "csrc", "rrtmg_gray.hip")).read()
    for kernel in ("frierson_kernel", "gray_longwave_kernel", "grid_scale_condensation_kernel"):
        assert re.search(r"__launch_bounds__\(64\)\s+%s" % kernel, src)
    assert src.count("column_head(") == 3 and src.count("column_required(") == 3 and src.count("column_call(") == 3 and src.count("column_launch(") == 3
    rule = open(os.path.join(ROOT, "climt_amd", "csrc", "rrtmg_gray.h")).read()
    for text in (src, rule):
        assert not re.search(r"\bwhile\b", re.sub(r"//[^\n]*", "", text))      # every loop is a for bounded by nlay
    assert "hip" not in re.sub(r"//[^\n]*", "", rule).lower().replace("__hipcc__", "")      # plain C++
    functions = re.findall(r"RRTMG_GRAY_HD \w+ \w+\([^)]*\) \{\n(.*)", rule)
    assert len(functions) == 5 and all(f == "#pragma clang fp contract(off)" for f in functions)


def test_property_dictionaries_and_defaults_are_the_references():
    ref = json.load(open(os.path.join(GOLDEN, "gray_interface.json")))
    assert set(ref) == {"GrayLongwaveRadiation", "Frierson06LongwaveOpticalDepth", "GridScaleCondensation"}
    from climt_amd import _sympl_compat as sc
    for name, r in ref.items():
        cls = getattr(climt_amd, name)
        assert getattr(sc, r["base"]) in cls.__mro__
        kinds = [k for k in r if k.endswith("_properties")]
        assert "input_properties" in kinds and len(kinds) == (2 if name == "Frierson06LongwaveOpticalDepth" else 3)
        for kind in kinds:
            assert getattr(cls, kind) == r[kind], (name, kind)
        sig = inspect.signature(cls.__init__)
        defaults = {n: p.default for n, p in sig.parameters.items() if p.default is not inspect.Parameter.empty}
        ours = dict(device=0, context=None, **({"optical_depth": None} if name == "GrayLongwaveRadiation" else {}))
        assert defaults == dict(r["init"], **ours), name
        order = [n for n in sig.parameters if n not in ours and sig.parameters[n].kind is inspect.Parameter.POSITIONAL_OR_KEYWORD]
        assert order == ["self"] + r.get("init_order", [])
    f = climt_amd.Frierson06LongwaveOpticalDepth(context=object())
    assert f.parameters() == X.FRIERSON and all(isinstance(v, float) for v in f.parameters().values())
    assert climt_amd.Frierson06LongwaveOpticalDepth(0.3, 7, 2, context=object()).parameters() == dict(fl=0.3, tau0e=7.0, tau0p=2.0)
    g = climt_amd.GrayLongwaveRadiation(context=object())
    assert g.constants() == X.GRAY_CONSTANTS and g.input_properties is climt_amd.GrayLongwaveRadiation.input_properties
    assert climt_amd.GridScaleCondensation(context=object()).constants() == X.GSC_CONSTANTS
    # the one keyword the reference lacks: the fused call reads the surface pressure and the latitude instead of the depth
    fused = climt_amd.GrayLongwaveRadiation(optical_depth=f, context=object())
    assert set(fused.input_properties) == (set(g.input_properties) - {TAU}) | {"surface_air_pressure", "latitude"}
    assert fused.input_properties["latitude"] == f.input_properties["latitude"] and fused.diagnostic_properties[TAU] == f.diagnostic_properties[TAU]
    assert set(fused.diagnostic_properties) == set(g.diagnostic_properties) | {TAU}
    assert TAU in climt_amd.GrayLongwaveRadiation.input_properties and TAU not in climt_amd.GrayLongwaveRadiation.diagnostic_properties
    with pytest.raises(TypeError, match="Frierson06LongwaveOpticalDepth"):
        climt_amd.GrayLongwaveRadiation(optical_depth=g, context=object())
    if hasattr(sc, "_constant_overrides"):      # constants are asked for at every call
        sc.set_constant("stefan_boltzmann_constant", 5.0e-8, "W/m^2/K^4")
        try:
            assert g.constants()["sigma_sb"] == 5.0e-8
        finally:
            sc._constant_overrides.clear()
        assert g.constants()["sigma_sb"] == X.SIGMA_SB


# ---- the C entries' argument checks (a context made without a GPU reports errors) -------------------------------------------------------
@pytest.fixture()
def bare_context():
    lib = _lib.load_library()
    h = C.c_void_p()
    lib.rrtmg_hip_create(C.byref(h), 0)
    assert h.value
    yield lib, h
    lib.rrtmg_hip_destroy(h)


def _args(struct, **scalars):
    """A well-formed struct over host memory, 4 columns by 3 layers (the checks under test come before anything is dereferenced
    or enqueued)."""
    prefix, ctype, _ = STRUCTS[struct]
    a, keep = ctype(), {}
    a.struct_size, a.ncol, a.nlay, a.memspace = C.sizeof(ctype), 4, 3, 0
    for n in sum(_tuples(prefix), ()):
        keep[n] = np.zeros(16)
        setattr(a, n, keep[n].ctypes.data)
    for n, t in ctype._fields_:
        if t is C.c_double:
            setattr(a, n, 1.0)
    for n, v in scalars.items():
        setattr(a, n, v)
    return a, keep


@pytest.mark.parametrize("struct", list(STRUCTS))
def test_the_entries_refuse_bad_arguments(bare_context, struct):
    lib, h = bare_context
    prefix, ctype, entry = STRUCTS[struct]
    fn = getattr(lib, "rrtmg_hip_" + entry)
    call = lambda a: fn(h, C.byref(a))
    message = lambda: lib.rrtmg_hip_last_error(h).decode()
    IN, OUT, DIAG = _tuples(prefix)
    assert fn(h, None) == 4 and message() == "%s: NULL argument struct" % entry
    for size in (0, C.sizeof(ctype) - 8, C.sizeof(ctype) + 8):
        a, keep = _args(struct, struct_size=size)
        assert call(a) == 4 and "struct_size %d, this library's %s has %d bytes" % (size, struct, C.sizeof(ctype)) in message()
    for field, values, text in (("ncol", (0, -1), "ncol must be positive"), ("nlay", (0, -3), "nlay must be at least 1"),
                                ("memspace", (-1, 2), "memspace must be 0 (host) or 1 (device)")):
        for value in values:
            a, keep = _args(struct, **{field: value})
            assert call(a) == 4 and message() == "%s: %s" % (entry, text)
    optional_in = ("tau", "ps", "lat") if entry == "gray_longwave" else ()
    required = [n for n in IN + OUT if n not in optional_in]
    given = "%s: %s and %s must be given" % (entry, ", ".join(required[:-1]), required[-1])
    for field in required:
        a, keep = _args(struct)
        setattr(a, field, None)
        assert call(a) == 4 and message() == given, field
    for field in DIAG:      # a NULL diagnostic is accepted: the next refusal is the one reported
        a, keep = _args(struct)
        setattr(a, field, None)
        setattr(a, OUT[-1], keep[IN[0]].ctypes.data)
        assert call(a) == 4 and "%s aliases an input" % OUT[-1] in message()
    # an output over an input: only x_out == x of the condensation is in place; an output over an earlier output
    outs = OUT + DIAG
    for out in outs:
        for inp in IN:
            if IN_PLACE[struct].get(out) == inp:
                continue
            a, keep = _args(struct, **({"frierson": 1 if inp in ("ps", "lat") else 0} if entry == "gray_longwave" else {}))
            setattr(a, out, keep[inp].ctypes.data)
            note = " (in place: exactly its own input)" if out in IN_PLACE[struct] else ""
            assert call(a) == 4 and message() == "%s: %s aliases an input%s" % (entry, out, note), (out, inp)
    for out, inp in IN_PLACE[struct].items():
        a, keep = _args(struct)
        setattr(a, out, keep[inp].ctypes.data + 8)      # in place means exactly in place
        assert call(a) == 4 and "%s aliases an input (in place: exactly its own input)" % out in message()
    for i, out in enumerate(outs):
        for earlier in outs[:i]:
            a, keep = _args(struct)
            setattr(a, out, keep[earlier].ctypes.data + 8)
            assert call(a) == 4 and message() == "%s: %s overlaps %s" % (entry, out, earlier)


def test_gray_longwave_refuses_what_its_switch_needs(bare_context):
    lib, h = bare_context
    call = lambda a: lib.rrtmg_hip_gray_longwave(h, C.byref(a))
    message = lambda: lib.rrtmg_hip_last_error(h).decode()
    for value in (-1, 2):
        a, keep = _args("rrtmg_gray_longwave", frierson=value)
        assert call(a) == 4 and "frierson must be 0" in message()
    for field in ("ps", "lat"):
        a, keep = _args("rrtmg_gray_longwave", frierson=1)
        setattr(a, field, None)
        assert call(a) == 4 and "ps and lat must be given with frierson 1" in message()
    a, keep = _args("rrtmg_gray_longwave", frierson=0)
    a.tau = None
    assert call(a) == 4 and "tau must be given with frierson 0" in message()
    # the array the switch leaves unread may be NULL, and where given takes no part in the aliasing check: the next refusal is reported
    for switch, unread in ((1, ("tau",)), (0, ("ps", "lat"))):
        for field in unread:
            a, keep = _args("rrtmg_gray_longwave", frierson=switch)
            setattr(a, field, None)
            a.hr = keep["t"].ctypes.data
            assert call(a) == 4 and "hr aliases an input" in message(), field
            a, keep = _args("rrtmg_gray_longwave", frierson=switch)
            a.up = keep[field].ctypes.data      # over an array that is not read: accepted
            a.dn = keep["t"].ctypes.data
            assert call(a) == 4 and "dn aliases an input" in message(), field


# ---- the numpy statements against the reference's own functions ------------------------------------------------------------------------
def _fixture(kind, name):
    z = np.load(os.path.join(GOLDEN, "%s_%s.npz" % (kind, name)))
    tol = X.tolerances(kind, name)
    assert list(z["nlays"]) == [2, 30, 61]
    assert all(v >= 1e-13 for v in tol.values()) and all(tol[f] == max(16.0 * float(z["moved_" + f]), 1e-13) for f in tol)
    return z, tol


@pytest.mark.parametrize("name", X.GRAY_CASES)
def test_gray_statements_equal_the_reference_fixture(name):
    """tests/golden/gray_<case>.npz: inputs at 2, 30 and 61 layers x 4 columns and what the reference's array_call made of them
    (fluxes, tendency, heating rate) and its Frierson depth of the same pressures and latitudes.  Expected and found: bit-identical."""
    z, tol = _fixture("gray", name)
    assert set(tol) == set(X.GRAY_FIELDS) | {"tau"}
    assert list(z["constants"]) == [X.SIGMA_SB, X.G, X.CPD] and list(z["frierson"]) == [X.FRIERSON[k] for k in ("tau0e", "tau0p", "fl")]
    for nlay in (2, 30, 61):
        c = X.gray_case(name, nlay, 4)
        for k in X.GRAY_INPUTS:
            assert X.same_bits(z["n%d_%s" % (nlay, k)], c[k]), k      # the fixture's inputs are the case builder's
        for k in X.GRAY_FIELDS:
            assert X.same_bits(z["n%d_ref_%s" % (nlay, k)], c[k]), (nlay, k)
        assert X.same_bits(z["n%d_ref_hr" % nlay], z["n%d_ref_tend" % nlay] * 86400.0)
        assert X.same_bits(z["n%d_ref_depth" % nlay], X.frierson_statement(c["lat"], c["p_int"], c["ps"]))
        assert X.same_bits(z["n%d_ref_dn" % nlay][-1], np.zeros(4))      # exact +0.0 at the top
    if name == "varied":
        assert list(z["n30_lat"]) == [-90.0, -30.0, 0.0, 90.0]
        depth = z["n30_ref_depth"]
        assert (depth[0] > 0).all() and (np.diff(depth, axis=0) > 0).all() and depth[-1, 2] > 5.9 and depth[-1, 0] < 1.5      # 0 below, tau_0 at the top


@pytest.mark.parametrize("name", X.GSC_CASES)
def test_condensation_statement_equals_the_reference_fixture(name):
    z, tol = _fixture("gsc", name)
    assert set(tol) == set(X.GSC_FIELDS) and float(z["margin"]) >= X.MIN_MARGIN
    assert list(z["constants"]) == [X.GSC_CONSTANTS[k] for k in X.GSC_CONSTANT_NAMES]
    margin = np.inf
    for nlay in (2, 30, 61):
        c = X.gsc_case(name, nlay, 4)
        margin = min(margin, c["margin"])
        for k in X.GSC_INPUTS:
            assert X.same_bits(z["n%d_%s" % (nlay, k)], c[k]), k
        for k in X.GSC_FIELDS:
            assert X.same_bits(z["n%d_ref_%s" % (nlay, k)], c[k]), (nlay, k)
        dry = ~c["saturated"]
        assert X.same_bits(z["n%d_ref_t_new" % nlay][dry], c["t"][dry]) and X.same_bits(z["n%d_ref_q_new" % nlay][dry], c["q"][dry])
        if name == "dry":
            assert X.same_bits(z["n%d_ref_precip" % nlay], np.zeros(4))      # exact +0.0
    assert margin == float(z["margin"])


@pytest.mark.parametrize("name", ["supersaturated", "alternate", "cold_stratosphere"])
def test_condensation_conserves_moist_enthalpy_and_rains_what_it_removes(name):
    k = X.GSC_CONSTANTS
    for nlay, ncol in ((1, 65), (30, 130), (61, 64)):
        c = X.gsc_case(name, nlay, ncol)
        dT, dq = c["t_new"] - c["t"], c["q_new"] - c["q"]
        # per layer cpd dT + lv dq = 0: each term is rounded to its field's ulp, ~6e-14 K on dT ~ 1 K
        assert float(np.abs(k["cpd"] * dT + k["lv"] * dq).max()) <= 4 * np.spacing(300.0) * k["cpd"]
        water = (dq * (c["p_int"][1:] - c["p_int"][:-1])).sum(axis=0) / k["g"]      # the reference's sign of the layer mass
        scale = (np.abs(dq) * np.abs(c["p_int"][1:] - c["p_int"][:-1])).sum(axis=0) / k["g"]
        wet = scale > 0
        assert wet.any() and float((np.abs(water + c["precip"] * k["rhow"])[wet] / scale[wet]).max()) <= 1e-12


# ---- the stand-alone host program ----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def program(tmp_path_factory):
    return build_host_program(tmp_path_factory, "gray_check.cpp", flags=["-ffp-contract=off"])


@pytest.fixture(scope="module")
def program_sanitized(tmp_path_factory):
    return build_host_program(tmp_path_factory, "gray_check.cpp", sanitized=True, flags=["-ffp-contract=off"])


def _run(exe, tmp_path, mode, nlay, ncol, head, arrays, sizes):
    fin, fout = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    np.concatenate([np.array(head, dtype=np.float64)] + [np.asarray(v, dtype=np.float64).ravel() for v in arrays]).tofile(fin)
    r = subprocess.run([exe, mode, str(ncol), str(nlay), fin, fout], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.startswith("ok"), (r.returncode, r.stdout, r.stderr)
    flat, got, at = np.fromfile(fout), {}, 0
    for name, shape in sizes:
        n = int(np.prod(shape))
        got[name] = flat[at:at + n].reshape(shape)
        at += n
    assert at == flat.size
    return got


def run_frierson(exe, tmp_path, p_int, ps, lat, parameters=X.FRIERSON, pressure_scale=1.0, ps_scale=1.0):
    nlev, ncol = p_int.shape
    head = [parameters["tau0e"], parameters["tau0p"], parameters["fl"], pressure_scale, ps_scale]
    return _run(exe, tmp_path, "frierson", nlev - 1, ncol, head, [p_int, ps, lat], [("tau", (nlev, ncol))])["tau"]


def run_gray(exe, tmp_path, c, fused=False, constants=X.GRAY_CONSTANTS, parameters=X.FRIERSON, pressure_scale=1.0, ps_scale=1.0):
    nlay, ncol = c["t"].shape
    head = [float(fused), parameters["tau0e"], parameters["tau0p"], parameters["fl"], constants["sigma_sb"], constants["g"], constants["cpd"], pressure_scale, ps_scale]
    il, ml = (nlay + 1, ncol), (nlay, ncol)
    return _run(exe, tmp_path, "gray", nlay, ncol, head, [c[k] for k in X.GRAY_INPUTS], [("up", il), ("dn", il), ("tend", ml), ("hr", ml), ("tau_out", il)])


def run_gsc(exe, tmp_path, c, in_place=False, constants=X.GSC_CONSTANTS, pressure_scale=1.0):
    nlay, ncol = c["t"].shape
    head = [float(in_place)] + [constants[k] for k in X.GSC_CONSTANT_NAMES] + [pressure_scale]
    return _run(exe, tmp_path, "gsc", nlay, ncol, head, [c[k] for k in X.GSC_INPUTS], [("t_new", (nlay, ncol)), ("q_new", (nlay, ncol)), ("precip", (ncol,))])


def check_gray(exe, tmp_path, name, nlay, ncol):
    """-> (largest deviation / tolerance from the statement, bits equal).  The program itself checks fused == depth then sweep."""
    c, tol = X.gray_case(name, nlay, ncol), X.tolerances("gray", name)
    got, fused = run_gray(exe, tmp_path, c), run_gray(exe, tmp_path, c, fused=True)
    depth = run_frierson(exe, tmp_path, c["p_int"], c["ps"], c["lat"])
    dev = X.deviations(got, c, X.GRAY_FIELDS)
    assert len(dev) == 4 and X.within(dev, tol), (name, nlay, ncol, dev, tol)
    assert X.same_bits(got["tau_out"], c["tau"]) and X.same_bits(fused["tau_out"], depth)
    assert X.same_bits(got["hr"], got["tend"] * 86400.0) and X.same_bits(got["dn"][-1], np.zeros(ncol))
    bits = all(X.same_bits(got[k], c[k]) for k in X.GRAY_FIELDS)
    if name in X.FUSED_CASES:      # the case's depth is the Frierson depth: the fused call against the same statement
        dev_f = X.deviations(dict(fused, tau=fused["tau_out"]), c, X.GRAY_FIELDS + ("tau",))
        assert len(dev_f) == 5 and X.within(dev_f, tol), (name, nlay, ncol, dev_f, tol)
        dev = {k: max(v, dev.get(k, 0.0)) for k, v in dev_f.items()}
        bits = bits and all(X.same_bits(fused[k], c[k]) for k in X.GRAY_FIELDS) and X.same_bits(depth, c["tau"])
    if name == "transparent":
        assert X.same_bits(got["dn"], np.zeros((nlay + 1, ncol))) and X.same_bits(got["up"], np.ones((nlay + 1, 1)) * got["up"][0][None, :])
    if name == "opaque":
        assert X.same_bits(got["up"][1:], got["dn"][:-1]) and X.same_bits(got["up"][0], got["up"][1])      # sigma T^4 of the layer; Ts = T[0]
    return max(v / tol[k] for k, v in dev.items()), bits


def check_gsc(exe, tmp_path, name, nlay, ncol, in_place):
    c, tol = X.gsc_case(name, nlay, ncol), X.tolerances("gsc", name)
    got = run_gsc(exe, tmp_path, c, in_place=in_place)
    dev = X.deviations(got, c, X.GSC_FIELDS)
    assert len(dev) == 3 and X.within(dev, tol), (name, nlay, ncol, dev, tol)
    dry = ~c["saturated"]
    assert X.same_bits(got["t_new"][dry], c["t"][dry]) and X.same_bits(got["q_new"][dry], c["q"][dry])
    assert X.same_bits(got["precip"][dry.all(axis=0)], np.zeros(int(dry.all(axis=0).sum())))      # exact +0.0
    return max(v / tol[k] for k, v in dev.items()), all(X.same_bits(got[k], c[k]) for k in X.GSC_FIELDS)


def test_host_program_equals_the_numpy_statements(program, tmp_path):
    for kind, names, check in (("gray", X.GRAY_CASES, check_gray), ("gsc", X.GSC_CASES, check_gsc)):
        for name in names:
            worst, same = 0.0, 0
            for i, (nlay, ncol) in enumerate(SHAPES):
                w, bits = check(program, tmp_path, name, nlay, ncol, *((i % 2,) if kind == "gsc" else ()))
                worst, same = max(worst, w), same + bits
            print("gray_check, %s %s: largest deviation / tolerance from the statement %.3e, %d of %d shapes bit-identical" % (kind, name, worst, same, len(SHAPES)))


def test_host_program_under_the_address_and_undefined_behaviour_sanitizers(program_sanitized, tmp_path):
    """The same program built with -fsanitize=address,undefined and run stand-alone, clean."""
    out = subprocess.run([program_sanitized, "tables"], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.endswith("ok\n"), out.stderr
    for nlay, ncol in ((1, 1), (1, 65), (2, 64), (30, 65), (61, 130)):
        for name in X.GRAY_CASES:
            check_gray(program_sanitized, tmp_path, name, nlay, ncol)
        for name in X.GSC_CASES:
            check_gsc(program_sanitized, tmp_path, name, nlay, ncol, (nlay + ncol) % 2)


def test_host_program_pressure_scales(program, tmp_path):
    """Pressures in mbar through the scales: the statements with the same scales, to the stored tolerances."""
    c = X.gray_case("varied", 30, 65)
    mbar = dict(c, p_int=c["p_int"] / 100.0, ps=c["ps"] / 100.0)
    want_tau = X.frierson_statement(mbar["lat"], mbar["p_int"], mbar["ps"], pressure_scale=100.0, ps_scale=100.0)
    want = X.gray_statement(mbar["t"], mbar["tsfc"], mbar["p_int"], want_tau, pressure_scale=100.0)
    got = run_gray(program, tmp_path, mbar, fused=True, pressure_scale=100.0, ps_scale=100.0)
    tol = X.tolerances("gray", "varied")
    assert X.within(X.deviations(dict(got, tau=got["tau_out"]), dict(want, tau=want_tau), X.GRAY_FIELDS + ("tau",)), tol)
    assert X.same_bits(run_frierson(program, tmp_path, mbar["p_int"], mbar["ps"], mbar["lat"], pressure_scale=100.0, ps_scale=100.0), got["tau_out"])
    g = X.gsc_case("alternate", 30, 65)
    gm = dict(g, p=g["p"] / 100.0, p_int=g["p_int"] / 100.0)
    want = X.gsc_statement(gm["t"], gm["q"], gm["p"], gm["p_int"], pressure_scale=100.0)
    assert want["margin"] >= X.MIN_MARGIN and X.same_bits(want["saturated"], g["saturated"])
    assert X.within(X.deviations(run_gsc(program, tmp_path, gm, pressure_scale=100.0), want, X.GSC_FIELDS), X.tolerances("gsc", "alternate"))


# ---- the tables the host program prints, by the rules of tests/test_call_arrays.py -------------------------------------------------------
@pytest.fixture(scope="module")
def tables(program):
    return column_table_rows(program, "tables")


def test_every_array_of_the_three_structs_is_one_row_of_its_table(tables):
    header = {(s, m): v for s in STRUCTS for m, v in header_pointer_members(s).items()}
    assert len(header) == 4 + 11 + 7
    printed = {(r["struct"], r["member"]): (r["io"] == "out", r["type"]) for r in tables}
    assert len(printed) == len(tables), "a member is listed twice"
    assert printed == header      # const <-> input, and the element type


def test_rows_agree_with_the_python_layer(tables):
    for struct, (prefix, ctype, entry) in STRUCTS.items():
        rows = [r for r in tables if r["struct"] == struct]
        IN, OUT, DIAG = _tuples(prefix)
        assert tuple(r["member"] for r in rows) == IN + OUT + DIAG and all(r["entry"] == entry for r in rows)
        assert all((r["io"] == "in") == (r["member"] in IN) for r in rows)
        assert all(r["flag"] == "required" for r in rows if r["member"] in OUT) and all(r["flag"] == "-" for r in rows if r["member"] in DIAG)
        assert [r["member"] for r in rows if r["io"] == "in" and r["flag"] == "-"] == (["tau", "ps", "lat"] if entry == "gray_longwave" else [])
        assert {r["member"]: r["in_place_of"] for r in rows if r["in_place_of"] != "-"} == IN_PLACE[struct]
        assert_column_rows_agree(rows, entry, struct)      # names, direction, type, in-place pairs and every extent
        assert all(t.name == "float64" for t in _lib.COLUMN_ARRAYS[entry]["dtype"].values()) and all(r["type"] == "f64" for r in rows)


def test_the_four_earlier_tables_are_printed_as_before(tmp_path_factory):
    """tools/column_call_check.cpp knows nothing of the new tables: its output is the four structs it had."""
    exe = build_host_program(tmp_path_factory, "column_call_check.cpp")
    out = subprocess.run([exe], stdout=subprocess.PIPE, universal_newlines=True, check=True).stdout.split("\n")
    assert out[-2:] == ["ok", ""] and len(out) - 2 == 7 + 20 + 20 + 17
    assert sorted({line.split()[2] for line in out[:-2]}) == ["rrtmg_boundary_layer", "rrtmg_dry_adjust", "rrtmg_emanuel", "rrtmg_simple_physics"]
    assert "gray" not in open(os.path.join(ROOT, "tools", "column_call_check.cpp")).read()


# ---- the components on host states: the host program stands in for the context -----------------------------------------------------------
class ProgramContext:
    """Context.frierson_optical_depth / gray_longwave / grid_scale_condensation (host arrays) by the stand-alone host program."""

    def __init__(self, exe, tmp_path):
        self.exe, self.tmp_path, self.calls = exe, tmp_path, []

    def frierson_optical_depth(self, pint, ps, lat, parameters, **kwargs):
        assert not kwargs
        self.calls.append(("frierson", pint.shape, dict(parameters)))
        return run_frierson(self.exe, self.tmp_path, pint, ps, lat, parameters)

    def gray_longwave(self, t, tsfc, pint, constants, tau=None, ps=None, lat=None, frierson=None, **kwargs):
        assert not kwargs and (tau is None) == (frierson is not None) and (ps is None) == (frierson is None) == (lat is None)
        self.calls.append(("gray", t.shape, dict(constants), frierson))
        zeros = np.zeros(pint.shape)
        c = dict(t=t, tsfc=tsfc, p_int=pint, tau=zeros if tau is None else tau, ps=zeros[0] if ps is None else ps, lat=zeros[0] if lat is None else lat)
        got = run_gray(self.exe, self.tmp_path, c, fused=frierson is not None, constants=constants, parameters=frierson or X.FRIERSON)
        d = dict(hr=got["hr"])
        if frierson is not None:
            d["tau_out"] = got["tau_out"]
        return got["up"], got["dn"], got["tend"], d

    def grid_scale_condensation(self, t, q, pmid, pint, constants, **kwargs):
        assert not kwargs
        self.calls.append(("gsc", t.shape, dict(constants)))
        got = run_gsc(self.exe, self.tmp_path, dict(t=t, q=q, p=pmid, p_int=pint), constants=constants)
        return got["t_new"], got["q_new"], dict(precip=got["precip"])


def host_state(c, g, ny, nx, tau=None):
    """Pressures in hPa / mbar and a (lat, lon) grid, levels LAST in the state's arrays."""
    lev = lambda a: np.ascontiguousarray(np.transpose(a.reshape(a.shape[0], ny, nx), (1, 2, 0)))
    q3 = lambda a, dim, units, f=1.0: DataArray(lev(a) / f, dims=("lat", "lon", dim), attrs={"units": units})
    q2 = lambda a, units, f=1.0: DataArray(a.reshape(ny, nx) / f, dims=("lat", "lon"), attrs={"units": units})
    state = {"air_temperature": q3(c["t"], "mid_levels", "degK"), "surface_temperature": q2(c["tsfc"], "degK"),
             "air_pressure": q3(g["p"], "mid_levels", "hPa", 100.0), "air_pressure_on_interface_levels": q3(c["p_int"], "interface_levels", "mbar", 100.0),
             "surface_air_pressure": q2(c["ps"], "mbar", 100.0), "latitude": q2(c["lat"], "degrees_north"),
             "specific_humidity": q3(g["q"], "mid_levels", "kg/kg"), "time": datetime.datetime(2000, 1, 1)}
    if tau is not None:
        state[TAU] = q3(tau, "interface_levels", "dimensionless")
    return state


def _levels(x, dim, ny, nx):
    return np.transpose(x.values, [x.dims.index(d) for d in (dim, "lat", "lon")]).reshape(-1, ny * nx)


def test_components_on_a_host_state_with_other_units_and_a_3d_grid(program, tmp_path):
    """The three components hand the rules [levels][columns] in Pa, the reference's constants and keyword parameters, and return
    the statements' numbers under the reference's names, dims and units; the fused component equals the two one after the other."""
    nlay, ny, nx = 30, 5, 13
    c, g = X.gray_case("varied", nlay, ny * nx), X.gsc_case("alternate", nlay, ny * nx)
    assert X.same_bits(c["p_int"], g["p_int"])
    back = lambda a: (a / 100.0) * 100.0      # hPa -> Pa on the way in costs a rounding per pressure
    ctx = ProgramContext(program, tmp_path)
    depth = climt_amd.Frierson06LongwaveOpticalDepth(context=ctx)
    state = host_state(c, g, ny, nx)
    d = depth(state)
    assert set(d) == {TAU} and d[TAU].attrs["units"] == "dimensionless" and set(d[TAU].dims) == {"interface_levels", "lat", "lon"}
    want_tau = X.frierson_statement(c["lat"], back(c["p_int"]), back(c["ps"]))
    tol = X.tolerances("gray", "varied")
    got_tau = _levels(d[TAU], "interface_levels", ny, nx)
    assert X.within(X.deviations(dict(tau=got_tau), dict(tau=want_tau), ("tau",)), tol)
    state.update(d)
    tendencies, diagnostics = climt_amd.GrayLongwaveRadiation(context=ctx)(state)
    fused_t, fused_d = climt_amd.GrayLongwaveRadiation(optical_depth=depth, context=ctx)(host_state(c, g, ny, nx))
    assert [call[0] for call in ctx.calls] == ["frierson", "gray", "gray"] and ctx.calls[0][1:] == ((nlay + 1, ny * nx), X.FRIERSON)
    assert ctx.calls[1][1:] == ((nlay, ny * nx), X.GRAY_CONSTANTS, None) and ctx.calls[2][1:] == ((nlay, ny * nx), X.GRAY_CONSTANTS, X.FRIERSON)
    want = X.gray_statement(c["t"], c["tsfc"], back(c["p_int"]), got_tau)
    names = {"upwelling_longwave_flux_in_air": ("up", "interface_levels", "W m^-2"), "downwelling_longwave_flux_in_air": ("dn", "interface_levels", "W m^-2"),
             "air_temperature_tendency_from_longwave": ("hr", "mid_levels", "degK day^-1")}
    assert set(diagnostics) == set(names) and set(fused_d) == set(names) | {TAU} and set(tendencies) == {"air_temperature"} == set(fused_t)
    assert tendencies["air_temperature"].attrs["units"] == "degK s^-1"
    got = {"tend": _levels(tendencies["air_temperature"], "mid_levels", ny, nx)}
    for n, (key, dim, units) in names.items():
        assert diagnostics[n].attrs["units"] == units and set(diagnostics[n].dims) == {dim, "lat", "lon"}
        got[key] = _levels(diagnostics[n], dim, ny, nx)
        assert X.same_bits(fused_d[n].values, diagnostics[n].values), n      # fused == the two components one after the other
    assert X.same_bits(fused_t["air_temperature"].values, tendencies["air_temperature"].values) and X.same_bits(fused_d[TAU].values, d[TAU].values)
    assert X.within(X.deviations(got, want, X.GRAY_FIELDS), tol)
    # the condensation: a Stepper, (diagnostics, new state)
    gsc = climt_amd.GridScaleCondensation(context=ctx)
    diag, new = gsc(state, datetime.timedelta(seconds=600))
    assert ctx.calls[-1] == ("gsc", (nlay, ny * nx), X.GSC_CONSTANTS)
    assert set(diag) == {"precipitation_amount"} and set(new) == {"air_temperature", "specific_humidity"}
    assert diag["precipitation_amount"].attrs["units"] == "kg m^-2" and tuple(diag["precipitation_amount"].dims) == ("lat", "lon")
    assert new["air_temperature"].attrs["units"] == "degK" and new["specific_humidity"].attrs["units"] == "kg/kg"
    want = X.gsc_statement(c["t"], g["q"], back(g["p"]), back(g["p_int"]))
    assert want["margin"] >= X.MIN_MARGIN
    got = dict(t_new=_levels(new["air_temperature"], "mid_levels", ny, nx), q_new=_levels(new["specific_humidity"], "mid_levels", ny, nx),
               precip=diag["precipitation_amount"].values.reshape(-1))
    assert X.within(X.deviations(got, want, X.GSC_FIELDS), X.tolerances("gsc", "alternate")) and want["saturated"].any()


def test_default_state_serves_the_gray_components():
    """get_default_state synthesises the optical depth, the surface pressure and the latitude that the gray components ask for."""
    comps = [climt_amd.GrayLongwaveRadiation(context=object()), climt_amd.Frierson06LongwaveOpticalDepth(context=object()), climt_amd.GridScaleCondensation(context=object())]
    state = climt_amd.get_default_state(comps, grid_state=climt_amd.get_grid(nx=1, ny=1, nz=10))
    for comp in comps:
        assert all(n in state for n in comp.input_properties)
    assert state[TAU].values.shape[state[TAU].dims.index("interface_levels")] == 11
