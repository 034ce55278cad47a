"""The land surface on the CPU: the symbols, header text and ctypes structs of rrtmg_hip_bucket_hydrology and rrtmg_hip_second_best;
BucketHydrology and SecondBEST against the reference's interface (tests/golden/land_surface_interface.json); every refusal of both
entries on a bare context; the numpy statements (tests/land_surface_cases.py) against the reference's own outputs
(tests/golden/bucket_<case>.npz, second_best_<case>.npz: both bit-identical, asserted, which is more than the stored tolerances
ask of SecondBEST); the stand-alone host program of the column rules (tools/land_surface_check.cpp on csrc/rrtmg_land_surface.h)
against the statements on every case and shape -- once more under the host sanitizers; the printed tables against the header and
_lib.COLUMN_ARRAYS; exact properties and the budgets on the program's own output; the NotImplementedError / ValueError contracts;
the two components on a host state.

Measured by the maker on the reference (+-1 ulp of every input and of every exp, log, sqrt and pow, 16 runs per shape with the
same decisions; all 48 tried runs of every case kept theirs), largest deviation on the scale of land_surface_cases.deviations:
soil temperature, water, surface temperature, albedos, t2m below 6e-15; drag coefficients 2.4e-13; sh 1.8e-13; lh and evaporation
9.4e-12 (the exfiltration limit is a difference of two powers); q2m 3.4e-14; 10 m wind 6.1e-14; x_i_out 1.0 in the `melting` case
only, where what is left of the ice is a rounding residue of 1e-19 against a column scale of the same size.  The tolerances are
16 x these, at least 1e-13.  Smallest margin of a case 4.0e-9 (MIN_MARGIN 1e-9)."""
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
from helpers import GOLDEN, ROOT, assert_column_rows_agree, build_host_program, column_table_rows, header_pointer_members

import land_surface_cases as X

ENTRIES = {"bucket_hydrology": ("rrtmg_bucket_hydrology", _lib.BucketHydrology, _lib.BUCKET_HYDROLOGY_IN, _lib.BUCKET_HYDROLOGY_OUT, _lib.BUCKET_HYDROLOGY_DIAG),
           "second_best": ("rrtmg_second_best", _lib.SecondBest, _lib.SECOND_BEST_IN, _lib.SECOND_BEST_OUT, _lib.SECOND_BEST_DIAG)}
DEEP = ("deep_moisture", "deep_temperature", "deep_moisture_out", "deep_temperature_out", "runoff", "deep_fraction")
IN_PLACE = {"bucket_hydrology": {n + "_out": n for n in ("ts", "soil_moisture", "deep_moisture", "deep_temperature")},
            "second_best": {n + "_out": n for n in ("t_soil", "x_w", "x_i", "ts", "snow")}}


def test_symbols_header_and_python_layer():
    lib = _lib.load_library()
    assert hasattr(lib, "rrtmg_hip_bucket_hydrology") and hasattr(lib, "rrtmg_hip_second_best") and lib.rrtmg_hip_abi_version() == 5
    text = open(os.path.join(ROOT, "include", "rrtmg_hip.h")).read()
    assert re.search(r"#define RRTMG_HIP_ABI_VERSION\s+5\b", text)
    flat = " ".join(re.sub(r"/\*.*?\*/", "", text, flags=re.S).split())
    assert "int rrtmg_hip_bucket_hydrology(rrtmg_ctx *ctx, const rrtmg_bucket_hydrology *a);" in flat
    assert "int rrtmg_hip_second_best(rrtmg_ctx *ctx, const rrtmg_second_best *a);" in flat
    assert "Probe for them by symbol; RRTMG_HIP_ABI_VERSION is unchanged." in " ".join(text.split())
    for entry, (strct, cls, IN, OUT, DIAG) in ENTRIES.items():
        body = re.search(r"typedef struct \{([^}]*)\} %s;" % strct, flat).group(1)
        members = []
        for decl in body.split(";"):      # the header's members in order are the ctypes fields in order
            members += [m.strip().lstrip("*").strip() for m in re.sub(r"^\s*(const\s+)?(double|int32_t|uint32_t)\s", "", decl).split(",") if m.strip()]
        names = [n for n, _ in cls._fields_]
        assert members == names, entry
        assert names[:4] == ["struct_size", "ncol", "nlay", "memspace"] and [n for n in names if n in IN + OUT + DIAG] == list(IN + OUT + DIAG)
        offset = 0
        for n, t in cls._fields_:      # no padding: every field begins where the one before it ends
            assert getattr(cls, n).offset == offset, (entry, n)
            offset += C.sizeof(t)
        assert offset == C.sizeof(cls)
        assert getattr(lib, "rrtmg_hip_" + entry).argtypes[1] == C.POINTER(cls)
        assert inspect.signature(getattr(_lib.Context, entry)).parameters["memspace"].default == 0
        assert isinstance(getattr(_lib.Context, "has_" + entry), property)
    assert C.sizeof(_lib.BucketHydrology) == 32 + 8 * (19 + 13 + 10) and C.sizeof(_lib.SecondBest) == 16 + 8 * (17 + 19 + 1 + 17)


def test_exports_property_dictionaries_and_defaults_are_the_references():
    want = json.load(open(os.path.join(GOLDEN, "land_surface_interface.json")))
    assert set(want) == {"BucketHydrology", "SecondBEST", "BestSubsurfaceTransport"}
    assert {"BucketHydrology", "SecondBEST", "BestSoilProperties", "BestSurfaceAlbedo", "BestSurfaceLayer", "BestSurfaceFluxes", "BestSubsurfaceTransport"} <= set(climt_amd.__all__)
    for cls in ("BucketHydrology", "SecondBEST"):
        ref, ours = want[cls], getattr(climt_amd, cls)
        assert ref["base"] == "Stepper" and issubclass(ours, climt_amd._sympl_compat.Stepper)
        for key in ("input_properties", "output_properties", "diagnostic_properties"):
            assert getattr(ours, key) == ref[key], (cls, key)
        p = inspect.signature(ours.__init__).parameters
        order = [n for n in ref["init_order"]]
        assert list(p)[1:1 + len(order)] == order and list(p)[1 + len(order):] == ["device", "context", "kwargs"]
        assert {n: p[n].default for n in ref["init"]} == ref["init"] and p["device"].default == 0 and p["context"].default is None
    p = inspect.signature(climt_amd.BestSubsurfaceTransport.__init__).parameters
    assert {n: p[n].default for n in want["BestSubsurfaceTransport"]["init"]} == want["BestSubsurfaceTransport"]["init"] == dict(thermal_conductivity=2.0, volumetric_heat_capacity=2.0e6)
    two, one = climt_amd.BucketHydrology(num_layers=2, context=object()), climt_amd.BucketHydrology(context=object())
    assert one.input_properties is climt_amd.BucketHydrology.input_properties      # the deep-soil properties are the instance's
    assert set(two.input_properties) - set(one.input_properties) == set(two.output_properties) - set(one.output_properties) == {"deep_soil_moisture_content", "deep_soil_temperature"}
    assert set(two.diagnostic_properties) - set(one.diagnostic_properties) == {"runoff_rate", "deep_soil_moisture_fraction"}


def test_constructor_contracts():
    with pytest.raises(ValueError, match=r"^num_layers must be 1 or 2$"):
        climt_amd.BucketHydrology(num_layers=3, context=object())
    classes = dict(soil_properties=climt_amd.BestSoilProperties, albedo=climt_amd.BestSurfaceAlbedo, surface_layer=climt_amd.BestSurfaceLayer,
                   fluxes=climt_amd.BestSurfaceFluxes, subsurface=climt_amd.BestSubsurfaceTransport)
    for name, cls in classes.items():
        climt_amd.SecondBEST(context=object(), **{name: cls()})
        for other in (object(), lambda *a: None, [c for c in classes.values() if c is not cls][0]()):
            with pytest.raises(NotImplementedError, match=name):
                climt_amd.SecondBEST(context=object(), **{name: other})
    comp = climt_amd.SecondBEST(soil_type="sand", minimum_wind_speed=0.5, subsurface=climt_amd.BestSubsurfaceTransport(1.5, 3.0e6), context=object())
    k = comp.constants()
    assert (k["kappa_soil"], k["cv_soil"], k["min_wind"], k["B"], k["K_H0"], k["colour"], k["texture"], k["psi_0"]) == (1.5, 3.0e6, 0.5, 4.0, 0.1, 1.0, 9.0, -0.2)
    assert set(k) == set(_lib.SECOND_BEST_CONSTANTS) and {n: climt_amd.SecondBEST(context=object()).constants()[n] for n in X.BEST_CONSTANTS} == X.BEST_CONSTANTS
    assert {n: v for n, v in climt_amd.BucketHydrology(context=object()).scalars().items()} == X.BUCKET_SCALARS
    get = climt_amd._sympl_compat.get_constant
    assert (get("latent_heat_of_vaporization", "J/kg"), get("von_karman_constant", "dimensionless"), get("density_of_liquid_water", "kg m^-3")) == (2.5e6, 0.4, 1000.0)


# ---- the refusals -------------------------------------------------------------------------------------------------------------------
@pytest.fixture()
def bare_context():
    lib = _lib.load_library()
    h = C.c_void_p()
    lib.rrtmg_hip_create(C.byref(h), 0)
    assert h.value
    yield lib, h
    lib.rrtmg_hip_destroy(h)


def _args(entry, **scalars):
    """A well-formed struct over host memory, 4 columns (the checks under test come before anything is dereferenced)."""
    strct, cls, IN, OUT, DIAG = ENTRIES[entry]
    a, keep = cls(), {}
    a.struct_size, a.ncol, a.nlay, a.memspace = C.sizeof(cls), 4, 1 if entry == "bucket_hydrology" else 2, 0
    for n in IN + OUT + DIAG:
        keep[n] = np.zeros(16)
        setattr(a, n, keep[n].ctypes.data)
    for n, t in cls._fields_:
        if t is C.c_double:
            setattr(a, n, 1.0)
    if entry == "bucket_hydrology":
        a.layers = 2
    for n, v in scalars.items():
        setattr(a, n, v)
    return a, keep


@pytest.mark.parametrize("entry", list(ENTRIES))
def test_the_entries_refuse_bad_arguments(bare_context, entry):
    lib, h = bare_context
    strct, cls, IN, OUT, DIAG = ENTRIES[entry]
    fn = getattr(lib, "rrtmg_hip_" + entry)
    call = lambda a: fn(h, C.byref(a))
    message = lambda: lib.rrtmg_hip_last_error(h).decode()
    size = C.sizeof(cls)
    assert fn(h, None) == 4 and message() == entry + ": NULL argument struct"
    for bad in (0, size - 8, size + 8):
        a, keep = _args(entry, struct_size=bad)
        assert call(a) == 4 and "struct_size %d, this library's %s has %d bytes" % (bad, strct, size) in message()
    bucket = entry == "bucket_hydrology"
    checks = [("ncol", (0, -1), "ncol must be positive"), ("memspace", (-1, 2), "memspace must be 0 (host) or 1 (device)"),
              ("dt", (0.0, -1.0, float("nan")), "dt must be positive"), ("reserved", (1, -1), "reserved must be 0"), ("reserved2", (1,), "reserved must be 0")]
    checks += [("nlay", (0, 2, -1), "nlay must be 1"), ("layers", (0, 3, -1), "layers must be 1 or 2"), ("tau_m", (0.0, -5.0, float("nan")), "tau_m must be positive with layers 2")] if bucket \
        else [("nlay", (1, 0, -3), "nlay must be at least 2")]
    for field, values, text in checks:
        for value in values:
            a, keep = _args(entry, **{field: value})
            assert call(a) == 4 and message().startswith(entry + ": " + text), (field, value, message())
    required = tuple(n for n in IN + OUT if n not in DEEP)
    given = "%s: %s and %s must be given" % (entry, ", ".join(required[:-1]), required[-1])
    for field in required:
        a, keep = _args(entry)
        setattr(a, field, None)
        assert call(a) == 4 and message() == given, field
    if bucket:
        for field in DEEP[:4]:      # required with two layers, not looked at with one
            a, keep = _args(entry)
            setattr(a, field, None)
            assert call(a) == 4 and message() == "bucket_hydrology: deep_moisture, deep_temperature, deep_moisture_out and deep_temperature_out must be given with layers 2"
            a, keep = _args(entry, layers=1, dt=0.0)
            setattr(a, field, None)
            assert call(a) == 4 and message() == "bucket_hydrology: dt must be positive"
        a, keep = _args(entry, layers=1, tau_m=0.0, dt=0.0)      # tau_m is not looked at with one layer
        assert call(a) == 4 and message() == "bucket_hydrology: dt must be positive"
        a, keep = _args(entry, layers=1, dt=0.0)                 # nor is an overlap among the two-layer rows
        a.deep_moisture_out = keep["ts"].ctypes.data
        assert call(a) == 4 and message() == "bucket_hydrology: dt must be positive"
    for field in DIAG:      # a NULL diagnostic is accepted: the next refusal is the one reported
        a, keep = _args(entry)
        setattr(a, field, None)
        a.ts_out = keep["sw_up"].ctypes.data
        assert call(a) == 4 and message() == entry + ": ts_out aliases an input (in place: exactly its own input)"
    note = " (in place: exactly its own input)"
    for out in OUT + DIAG:
        for inp in IN:
            if IN_PLACE[entry].get(out) == inp:
                continue
            a, keep = _args(entry, dt=0.0)      # the aliasing refusal comes before the entry's own
            setattr(a, out, keep[inp].ctypes.data)
            assert call(a) == 4 and message() == "%s: %s aliases an input%s" % (entry, out, note if out in IN_PLACE[entry] else ""), (out, inp)
    for out, inp in IN_PLACE[entry].items():
        a, keep = _args(entry)
        setattr(a, out, keep[inp].ctypes.data + 8)      # in place means exactly in place
        assert call(a) == 4 and message() == "%s: %s aliases an input%s" % (entry, out, note)
    outs = OUT + DIAG
    for i, out in enumerate(outs):
        for earlier in outs[:i]:
            a, keep = _args(entry)
            setattr(a, out, keep[earlier].ctypes.data + 8)
            assert call(a) == 4 and message() == "%s: %s overlaps %s" % (entry, out, earlier)


# ---- the statements against the reference ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(X.BUCKET_CASES))
def test_bucket_statement_equals_the_reference_fixture(name):
    """The reference's own array_call on the inputs in the file against the statement on the same inputs: the same bits.  And the
    inputs in the file are what the case builder makes today."""
    z, built = X.fixture("bucket", name), X.bucket_case(name, 4)
    layers = int(z["layers"])
    assert layers == X.BUCKET_CASES[name] and float(z["dt"]) == built["dt"]
    c = {k: z[k] for k in X.BUCKET_INPUTS if k in z.files}
    assert set(c) == {k for k in X.BUCKET_INPUTS if k in built} and all(X.same_bits(c[k], built[k]) for k in c)
    s = X.bucket_statement(layers, c, float(z["dt"]), X.bucket_scalars(name))
    assert {f[4:] for f in z.files if f.startswith("ref_")} == set(X.BUCKET_FIELDS[layers])
    for f in X.BUCKET_FIELDS[layers]:
        assert X.same_bits(s[f], z["ref_" + f]), f


@pytest.mark.parametrize("name", X.BEST_CASES)
def test_second_best_statement_equals_the_reference_fixture(name):
    z = X.fixture("second_best", name)
    assert float(z["margin"]) >= float(z["min_margin"]) == X.MIN_MARGIN
    tol = X.tolerances(name)
    assert set(tol) == set(X.BEST_FIELDS) and all(v >= 1e-13 for v in tol.values()), tol
    assert all(v <= 1e-9 for f, v in tol.items() if f != "x_i_out"), tol      # (the residue of the `melting` case: the module's docstring)
    worst = 0.0
    for nlay in z["nlays"]:
        c = {k: z["n%d_%s" % (nlay, k)] for k in X.BEST_INPUTS}
        built = X.best_case(name, int(nlay), 4)
        assert float(z["dt"]) == built["dt"] and all(X.same_bits(c[k], built[k]) for k in X.BEST_INPUTS)
        with np.errstate(all="ignore"):
            s = X.best_statement(c, float(z["dt"]), X.best_constants(name))
        ref = {f: z["n%d_ref_%s" % (nlay, f)] for f in X.BEST_FIELDS}
        dev = X.deviations(s, ref, X.BEST_FIELDS)
        worst = max(worst, max(dev.values()))
        assert X.within(dev, tol), (nlay, dev)
        assert all(X.same_bits(s[f], ref[f]) for f in X.BEST_FIELDS), nlay      # the same libm: the same bits
    print("second_best %s: largest deviation of the statement from the reference %.1e" % (name, worst))


# ---- the host program -----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def program(tmp_path_factory):
    return build_host_program(tmp_path_factory, "land_surface_check.cpp", flags=["-ffp-contract=off"])


@pytest.fixture(scope="module")
def program_sanitized(tmp_path_factory):
    return build_host_program(tmp_path_factory, "land_surface_check.cpp", sanitized=True, flags=["-ffp-contract=off"])


def _run(exe, tmp_path, argv, head, arrays):
    src, dst = os.path.join(str(tmp_path), "land_in.bin"), os.path.join(str(tmp_path), "land_out.bin")
    np.concatenate([np.array(head, dtype=np.float64)] + [np.asarray(x, dtype=np.float64).reshape(-1) for x in arrays]).tofile(src)
    out = subprocess.run([exe] + [str(x) for x in argv] + [src, dst], stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True)
    assert out.returncode == 0 and out.stdout.startswith("ok"), out.stderr[-2000:]
    return np.fromfile(dst)


def run_bucket_program(exe, tmp_path, layers, arrays, dt, k, pressure_scale=1.0):
    ncol = arrays["ts"].shape[0]
    head = [layers, 0.0 if k["tau_drain"] is None else 1.0, dt] + [0.0 if k[n] is None else k[n] for n in _lib.BUCKET_HYDROLOGY_SCALARS] + [pressure_scale]
    flat = _run(exe, tmp_path, ["bucket", ncol], head, [arrays.get(n, np.zeros(ncol)) for n in _lib.BUCKET_HYDROLOGY_IN])
    names = _lib.BUCKET_HYDROLOGY_OUT + _lib.BUCKET_HYDROLOGY_DIAG
    assert flat.size == len(names) * ncol
    return {n: flat[i * ncol:(i + 1) * ncol] for i, n in enumerate(names) if layers == 2 or n not in DEEP}


def run_best_program(exe, tmp_path, arrays, dt, k, pressure_scale=1.0, ps_scale=1.0):
    nlay, ncol = arrays["t_soil"].shape
    head = [dt] + [k[n] for n in _lib.SECOND_BEST_CONSTANTS] + [pressure_scale, ps_scale]
    flat, got, at = _run(exe, tmp_path, ["best", ncol, nlay], head, [arrays[n] for n in _lib.SECOND_BEST_IN]), {}, 0
    for n in _lib.SECOND_BEST_OUT + _lib.SECOND_BEST_DIAG:
        shape = (nlay, ncol) if n in ("t_soil_out", "x_w_out", "x_i_out") else (ncol,)
        got[n] = flat[at:at + int(np.prod(shape))].reshape(shape)
        at += int(np.prod(shape))
    assert at == flat.size
    got["flags"] = got["flags"].astype(np.int32)
    return got


def check_bucket_program(exe, tmp_path, name, ncol):
    c = X.bucket_case(name, ncol)
    got = run_bucket_program(exe, tmp_path, c["layers"], c, c["dt"], c["scalars"])
    assert set(got) == set(X.BUCKET_FIELDS[c["layers"]])
    for f in got:
        assert X.same_bits(got[f], c[f]), (name, ncol, f)      # no libm call but sqrt: the statement's bits
    return X.bucket_budgets(c, got)


def check_best_program(exe, tmp_path, name, nlay, ncol):
    c = X.best_case(name, nlay, ncol)
    got = run_best_program(exe, tmp_path, c, c["dt"], X.best_constants(name))
    dev = X.deviations(got, c, X.BEST_FIELDS)
    assert X.within(dev, X.tolerances(name)), (name, nlay, ncol, dev)
    X.check_best_exact_properties(c, got, X.tolerances(name))      # on the program's own output: the decisions, what no tolerance covers, water and ice per node
    return all(X.same_bits(got[f], c[f]) for f in X.BEST_FIELDS), max(dev.values())


def test_host_program_equals_the_bucket_statement_and_closes_the_budgets(program, tmp_path):
    """Every case and shape bit for bit; and on the program's own output the water budget of both layer counts and the one-layer
    energy budget close to rounding (land_surface_cases.bucket_budgets: 8 x 2^-52 of the larger side, from the operation count)."""
    worst = dict(water=0.0, energy=0.0)
    for name in X.BUCKET_CASES:
        for ncol in X.NCOLS:
            b = check_bucket_program(program, tmp_path, name, ncol)
            worst = {k: max(worst[k], b[k]) for k in worst}
    print("bucket, host program: 13 cases x 4 shapes bit-identical; budgets: water %.2f, energy %.2f x 2^-52 of their scales" % (worst["water"], worst["energy"]))
    assert worst["water"] <= 8.0 and worst["energy"] <= 8.0


def test_host_program_equals_the_second_best_statement(program, tmp_path):
    """Every case and shape: within the stored tolerances, the decisions and the exact properties on the program's own output (the
    program itself holds in place == out of place == without the optional outputs, bit for bit)."""
    runs = [check_best_program(program, tmp_path, name, nlay, ncol) for name in X.BEST_CASES for nlay in X.BEST_NLAYS for ncol in X.NCOLS]
    print("second_best, host program: %d of %d runs bit-identical to the statement, largest deviation %.1e" % (sum(r[0] for r in runs), len(runs), max(r[1] for r in runs)))
    assert len(runs) == 15 * 12


def test_host_program_under_the_address_and_undefined_behaviour_sanitizers(program_sanitized, tmp_path):
    for nlay, ncol in ((2, 1), (2, 65), (4, 64), (12, 130)):
        for name in ("mixed_types", "calm", "no_ice_no_water", "freezing"):
            check_best_program(program_sanitized, tmp_path, name, nlay, ncol)
        for name in ("saturated_dry", "dries_out", "drainage", "overflow"):
            check_bucket_program(program_sanitized, tmp_path, name, ncol)
    out = subprocess.run([program_sanitized, "tables"], stdout=subprocess.PIPE, universal_newlines=True, check=True).stdout
    assert out.endswith("ok\n")


def test_tables_agree_with_the_header_and_the_python_layer(program):
    every = column_table_rows(program, "tables")
    assert [r["entry"] for r in every] == ["bucket_hydrology"] * 29 + ["second_best"] * 34
    for entry, (strct, cls, IN, OUT, DIAG) in ENTRIES.items():
        rows = [r for r in every if r["entry"] == entry]
        assert all(r["struct"] == strct for r in rows) and tuple(r["member"] for r in rows) == IN + OUT + DIAG
        assert {r["member"]: (r["io"] == "out", r["type"]) for r in rows} == header_pointer_members(strct)
        assert all((r["io"] == "in") == (r["member"] in IN) for r in rows)
        assert all((r["flag"] == "required") == (r["member"] in IN + OUT and r["member"] not in DEEP) for r in rows)
        arrays = _lib.COLUMN_ARRAYS[entry]
        assert (arrays["IN"], arrays["DIAG"]) == (IN, DIAG) and not any(r["extent"] == "[nlay+1][ncol]" for r in rows)
        assert_column_rows_agree(rows, entry, strct)      # names, direction, type, in-place pairs and every extent
        assert {r["member"]: r["in_place_of"] for r in rows if r["in_place_of"] != "-"} == IN_PLACE[entry] == dict(arrays["in_place"])
    assert all(r["extent"] == "[ncol]" for r in every if r["entry"] == "bucket_hydrology")
    assert "land_surface" not in open(os.path.join(ROOT, "tools", "column_call_check.cpp")).read()


def test_pressure_scales_of_the_host_program(program, tmp_path):
    """Pressures in hPa with scale 100 give the bits of pressures in Pa with scale 1 where the conversion is exact (whole hPa)."""
    c = {k: np.array(v) for k, v in X.best_case("unstable_day", 4, 65).items() if isinstance(v, np.ndarray)}
    c["p_air"], c["ps"] = np.round(c["p_air"] / 100.0) * 100.0, np.round(c["ps"] / 100.0) * 100.0
    k = X.best_constants()
    pa = run_best_program(program, tmp_path, c, X.BEST_DT, k)
    hpa = run_best_program(program, tmp_path, dict(c, p_air=c["p_air"] / 100.0, ps=c["ps"] / 100.0), X.BEST_DT, k, pressure_scale=100.0, ps_scale=100.0)
    assert all(X.same_bits(pa[f], hpa[f]) for f in pa)
    b = {k2: np.array(v) for k2, v in X.bucket_case("below_beta", 65).items() if isinstance(v, np.ndarray)}
    b["p_air"] = np.round(b["p_air"] / 100.0) * 100.0
    pa = run_bucket_program(program, tmp_path, 1, b, X.BUCKET_DT, X.bucket_scalars("below_beta"))
    hpa = run_bucket_program(program, tmp_path, 1, dict(b, p_air=b["p_air"] / 100.0), X.BUCKET_DT, X.bucket_scalars("below_beta"), pressure_scale=100.0)
    assert all(X.same_bits(pa[f], hpa[f]) for f in pa)


# ---- the components on host states: the host program stands in for the context ------------------------------------------------------------
class ProgramContext:
    """Context.bucket_hydrology and Context.second_best (host arrays) by the stand-alone host program."""

    def __init__(self, exe, tmp_path):
        self.exe, self.tmp_path, self.calls = exe, tmp_path, []

    def bucket_hydrology(self, layers, arrays, dt, scalars, **kwargs):
        assert not kwargs
        self.calls.append(("bucket", layers, dt, dict(scalars)))
        got = run_bucket_program(self.exe, self.tmp_path, layers, arrays, dt, scalars)
        return {n: got[n] for n in _lib.BUCKET_HYDROLOGY_OUT if n in got}, {n: got[n] for n in _lib.BUCKET_HYDROLOGY_DIAG if n in got}

    def second_best(self, arrays, dt, constants, **kwargs):
        assert not kwargs and arrays["area_type"].dtype == np.int32
        self.calls.append(("best", arrays["t_soil"].shape, dt, dict(constants)))
        got = run_best_program(self.exe, self.tmp_path, arrays, dt, constants)
        return {n: got[n] for n in _lib.SECOND_BEST_OUT}, {n: got[n] for n in _lib.SECOND_BEST_DIAG}


@pytest.mark.parametrize("name", ["below_beta", "drainage"])
def test_bucket_hydrology_on_a_host_state_with_a_3d_grid(program, tmp_path, name):
    ny, nx = 5, 13
    c = X.bucket_case(name, ny * nx)
    ctx = ProgramContext(program, tmp_path)
    comp = climt_amd.BucketHydrology(num_layers=c["layers"], deep_drainage_timescale=c["scalars"]["tau_drain"], context=ctx)
    diag, new = comp(X.bucket_host_state(c, ny, nx), datetime.timedelta(seconds=c["dt"]))
    assert ctx.calls == [("bucket", c["layers"], c["dt"], c["scalars"])]
    assert set(diag) == set(comp.diagnostic_properties) and set(new) >= set(comp.output_properties)
    from climt_amd.bucket_hydrology import DIAGNOSTIC_NAMES, OUTPUT_NAMES
    for short, long in list(comp.names(OUTPUT_NAMES).items()) + list(comp.names(DIAGNOSTIC_NAMES).items()):
        q = (new if short.endswith("_out") else diag)[long]
        prop = (comp.output_properties if short.endswith("_out") else comp.diagnostic_properties)[long]
        assert X.same_bits(q.values.reshape(-1), c[short]) and q.attrs["units"] == prop["units"] and set(q.dims) == {"lat", "lon"}, long


def test_second_best_on_a_host_state_with_a_3d_grid(program, tmp_path):
    ny, nx, n = 5, 13, 4
    c = X.best_case("mixed_types", n, ny * nx)
    ctx = ProgramContext(program, tmp_path)
    comp = climt_amd.SecondBEST(context=ctx)
    diag, new = comp(X.best_host_state(c, ny, nx), datetime.timedelta(seconds=c["dt"]))
    assert ctx.calls == [("best", (n, ny * nx), c["dt"], X.best_constants())]
    assert set(diag) == set(comp.diagnostic_properties) and set(new) >= set(comp.output_properties)
    from climt_amd.second_best import DIAGNOSTIC_NAMES, OUTPUT_NAMES
    got = {}
    for short, long in list(OUTPUT_NAMES.items()) + list(DIAGNOSTIC_NAMES.items()):
        q = (new if short.endswith("_out") else diag)[long]
        prop = (comp.output_properties if short.endswith("_out") else comp.diagnostic_properties)[long]
        soil = "soil_interface_levels" in prop["dims"]
        assert q.attrs["units"] == prop["units"] and set(q.dims) == ({"lat", "lon"} | ({"soil_interface_levels"} if soil else set())), long
        got[short] = np.transpose(q.values, [q.dims.index(d) for d in ("soil_interface_levels", "lat", "lon")]).reshape(n, -1) if soil else q.values.reshape(-1)
    assert X.within(X.deviations(got, c, X.BEST_FIELDS), X.tolerances("mixed_types"))
    assert X.same_bits(comp.flags.reshape(-1), c["flags"])


def test_default_state_serves_every_input():
    comps = [climt_amd.BucketHydrology(num_layers=2, context=object()), climt_amd.SecondBEST(context=object())]
    state = climt_amd.get_default_state(comps, grid_state=climt_amd.get_grid(nx=1, ny=1, nz=10))
    for comp in comps:
        assert all(n in state for n in comp.input_properties), [n for n in comp.input_properties if n not in state]
    assert state["soil_temperature"].dims[0] == "soil_interface_levels"
