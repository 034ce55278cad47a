"""The snow/ice column on the CPU: rrtmg_hip_surface_ice's symbol, header text and ctypes struct; SeaIce and LandIce against the
reference's interface (tests/golden/surface_ice_interface.json); every refusal of the entry on a bare context; the numpy
statements (tests/surface_ice_cases.py) against the reference's own outputs (tests/golden/sea_ice_<case>.npz, land_ice_<case>.npz:
bit-identical, asserted); the stand-alone host program of the column rule (tools/surface_ice_check.cpp on
csrc/rrtmg_surface_ice.h) against the statements on every case and shape -- once more under the host sanitizers; the printed table
against the header and _lib.COLUMN_ARRAYS; exact properties and the energy budget on the program's own output
(surface_ice_cases.check_exact_properties, energy_budget); the reference's zero-forcing energy check; the two components on a host state.

Measured by the maker on the reference (+-1 ulp of every input, 16 runs per shape with the same decisions; all 48 tried runs of
every case kept theirs), largest deviation on the scale of surface_ice_cases.deviations: t_out 4.4e-15, tsfc_out 2.2e-15, height_out
5.0e-16, thick_out and snow_out 2.2e-16, base_flux_out 3.5e-16 (sea ice, rounded to 1e-6) and 1.4e-11 (land ice: a difference of
two temperatures over a layer of 0.15 mm), cond_flux 4.0e-12, albedo 0.  The tolerances are 16 x these, at least 1e-13.  Smallest
margin of a case 4.05e-13 (MIN_MARGIN 1e-13).  The host program is bit-identical to the statements on every case and shape (the
test prints the count and asserts the stored tolerances)."""
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

import surface_ice_cases as X

ENTRY, STRUCT = "surface_ice", "rrtmg_surface_ice"
IN, OUT, DIAG = _lib.SURFACE_ICE_IN, _lib.SURFACE_ICE_OUT, _lib.SURFACE_ICE_DIAG
IN_PLACE = {"t_out": "t", "height_out": "height", "thick_out": "thick", "snow_out": "snow", "base_flux_out": "base"}
ALL_CASES = [(kn, name) for kn, kind in X.KINDS.items() for name in X.CASES[kind]]


def test_symbol_header_and_python_layer():
    lib = _lib.load_library()
    assert hasattr(lib, "rrtmg_hip_surface_ice") and lib.rrtmg_hip_abi_version() == 5
    text = open(os.path.join(ROOT, "include", "rrtmg_hip.h")).read()
    assert re.search(r"#define RRTMG_HIP_ABI_VERSION\s+5\b", text)
    flat = " ".join(re.sub(r"/\*.*?\*/", "", text, flags=re.S).split())
    assert ("typedef struct { uint32_t struct_size; int32_t ncol, nlay, memspace; int32_t kind, reserved; const double *t, *height; "
            "const double *thick, *snow, *base; const double *sw_down, *lw_down, *sw_up, *lw_up, *lh, *sh; const int32_t *area_type; double dt; "
            "double rho_ice, rho_snow, c_ice, c_snow, k_ice, k_snow, lf, t_melt, eps, max_height, albedo_snow, albedo_ice, albedo_melt; "
            "double *t_out, *height_out; double *thick_out, *snow_out, *tsfc_out; double *base_flux_out; double *cond_flux, *albedo; "
            "int32_t *flags; } rrtmg_surface_ice;") in flat
    assert "int rrtmg_hip_surface_ice(rrtmg_ctx *ctx, const rrtmg_surface_ice *a);" in flat
    assert "Probe for it by symbol; RRTMG_HIP_ABI_VERSION is unchanged." in " ".join(text.split()).split("sea ice and land ice: one implicit", 1)[1].split("rrtmg_surface_ice;", 1)[0]
    names = [n for n, _ in _lib.SurfaceIce._fields_]
    assert names == (["struct_size", "ncol", "nlay", "memspace", "kind", "reserved"] + list(IN) + ["dt"] + list(_lib.SURFACE_ICE_CONSTANTS) + list(OUT + DIAG))
    offset = 0
    for n, t in _lib.SurfaceIce._fields_:      # no padding: every field begins where the one before it ends
        assert getattr(_lib.SurfaceIce, n).offset == offset, n
        offset += C.sizeof(t)
    assert offset == C.sizeof(_lib.SurfaceIce) == 24 + 8 * (12 + 1 + 13 + 9)
    assert lib.rrtmg_hip_surface_ice.argtypes[1] == C.POINTER(_lib.SurfaceIce)
    assert "Context.has_surface_ice" in str(_lib.Context.has_surface_ice.fget.__qualname__) and inspect.signature(_lib.Context.surface_ice).parameters["memspace"].default == 0


def test_exports_property_dictionaries_and_defaults_are_the_references():
    want = json.load(open(os.path.join(GOLDEN, "surface_ice_interface.json")))
    assert set(want) == {"SeaIce", "LandIce"} and {"SeaIce", "LandIce"} <= set(climt_amd.__all__)
    for cls, ref in want.items():
        ours = getattr(climt_amd, cls)
        assert ref["base"] == "Stepper" and issubclass(ours, climt_amd._sympl_compat.Stepper)
        for key in ("input_properties", "output_properties", "diagnostic_properties"):
            assert getattr(ours, key) == ref[key], (cls, key)
        p = inspect.signature(ours.__init__).parameters
        assert list(p)[1:1 + len(ref["init_order"])] == ref["init_order"] and list(p)[1 + len(ref["init_order"]):] == ["device", "context", "kwargs"]
        assert {n: p[n].default for n in ref["init"]} == ref["init"] and p["device"].default == 0 and p["context"].default is None
    assert want["SeaIce"]["init"]["albedo_ice"] == 0.5 and want["LandIce"]["init"]["albedo_ice"] == 0.6


# ---- the refusals -------------------------------------------------------------------------------------------------------------------
@pytest.fixture()
def bare_context():
    lib = _lib.load_library()
    h = C.c_void_p()
    lib.rrtmg_hip_create(C.byref(h), 0)
    assert h.value
    yield lib, h
    lib.rrtmg_hip_destroy(h)


def _args(**scalars):
    """A well-formed struct over host memory, 4 columns by 3 nodes (the checks under test come before anything is dereferenced)."""
    a, keep = _lib.SurfaceIce(), {}
    a.struct_size, a.ncol, a.nlay, a.memspace = C.sizeof(_lib.SurfaceIce), 4, 3, 0
    for n in IN + OUT + DIAG:
        keep[n] = np.zeros(16)
        setattr(a, n, keep[n].ctypes.data)
    for n, t in _lib.SurfaceIce._fields_:
        if t is C.c_double:
            setattr(a, n, 1.0)
    for n, v in scalars.items():
        setattr(a, n, v)
    return a, keep


def test_the_entry_refuses_bad_arguments(bare_context):
    lib, h = bare_context
    fn = lib.rrtmg_hip_surface_ice
    call = lambda a: fn(h, C.byref(a))
    message = lambda: lib.rrtmg_hip_last_error(h).decode()
    size = C.sizeof(_lib.SurfaceIce)
    assert fn(h, None) == 4 and message() == "surface_ice: NULL argument struct"
    for bad in (0, size - 8, size + 8):
        a, keep = _args(struct_size=bad)
        assert call(a) == 4 and "struct_size %d, this library's rrtmg_surface_ice has %d bytes" % (bad, size) in message()
    for field, values, text in (("ncol", (0, -1), "ncol must be positive"), ("nlay", (2, 0, -3), "nlay must be at least 3"),
                                ("memspace", (-1, 2), "memspace must be 0 (host) or 1 (device)"), ("kind", (-1, 2), "kind must be 0 (sea ice) or 1 (land ice)"),
                                ("reserved", (1, -1), "reserved must be 0"), ("dt", (0.0, -1.0, float("nan")), "dt must be positive")):
        for value in values:
            a, keep = _args(**{field: value})
            assert call(a) == 4 and message().startswith("surface_ice: " + text), (field, value, message())
    required = IN + OUT
    given = "surface_ice: %s and %s must be given" % (", ".join(required[:-1]), required[-1])
    for field in required:
        a, keep = _args()
        setattr(a, field, None)
        assert call(a) == 4 and message() == given, field
    for field in DIAG:      # a NULL diagnostic is accepted: the next refusal is the one reported
        a, keep = _args()
        setattr(a, field, None)
        setattr(a, "tsfc_out", keep["lh"].ctypes.data)
        assert call(a) == 4 and message() == "surface_ice: tsfc_out aliases an input"
    note = " (in place: exactly its own input)"
    for out in OUT + DIAG:
        for inp in IN:
            if IN_PLACE.get(out) == inp:
                continue
            a, keep = _args(kind=0)
            setattr(a, out, keep[inp].ctypes.data)
            assert call(a) == 4 and message() == "surface_ice: %s aliases an input%s" % (out, note if out in IN_PLACE else ""), (out, inp)
    for out, inp in IN_PLACE.items():
        a, keep = _args(kind=0)
        setattr(a, out, keep[inp].ctypes.data + 8)      # in place means exactly in place
        assert call(a) == 4 and message() == "surface_ice: %s aliases an input%s" % (out, note)
    outs = OUT + DIAG
    for i, out in enumerate(outs):
        for earlier in outs[:i]:
            a, keep = _args()
            setattr(a, out, keep[earlier].ctypes.data + 8)
            assert call(a) == 4 and message() == "surface_ice: %s overlaps %s" % (out, earlier)
    a, keep = _args(kind=1)      # the soil temperature is not stepped
    a.base_flux_out = keep["base"].ctypes.data
    assert call(a) == 4 and message().startswith("surface_ice: base_flux_out aliases an input (kind 1")


# ---- the statements against the reference ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind_name,name", ALL_CASES)
def test_statement_equals_the_reference_fixture(kind_name, name):
    """The reference's own array_call on the inputs in the file, against the statement on the same inputs: the same bits.  And the
    inputs in the file are what the case builder makes today."""
    z, kind = X.fixture(kind_name, name), X.KINDS[kind_name]
    assert float(z["margin"]) >= float(z["min_margin"]) == X.MIN_MARGIN
    tol = X.tolerances(kind_name, name)
    assert set(tol) == set(X.FIELDS) and all(1e-13 <= v <= 1e-9 for v in tol.values()), tol
    for nlay in z["nlays"]:
        c = {k: z["n%d_%s" % (nlay, k)] for k in X.INPUTS}
        dt = float(z["n%d_dt" % nlay])
        built = X.ice_case(kind, name, int(nlay), 4)
        assert dt == built["dt"] and all(X.same_bits(c[k], built[k]) for k in X.INPUTS)
        s = X.ice_statement(kind, *(c[k] for k in X.INPUTS), dt)
        assert (s["margin"] >= X.MIN_MARGIN).all()
        for f in X.FIELDS:
            assert X.same_bits(s[f], z["n%d_ref_%s" % (nlay, f)]), (nlay, f)


# ---- the host program -----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def program(tmp_path_factory):
    return build_host_program(tmp_path_factory, "surface_ice_check.cpp", flags=["-ffp-contract=off"])


@pytest.fixture(scope="module")
def program_sanitized(tmp_path_factory):
    return build_host_program(tmp_path_factory, "surface_ice_check.cpp", sanitized=True, flags=["-ffp-contract=off"])


def run_program(exe, tmp_path, kind, c, dt, k=None):
    k = X.constants(kind) if k is None else k
    nlay, ncol = c["t"].shape
    head = [float(kind), float(dt)] + [float(k[n]) for n in _lib.SURFACE_ICE_CONSTANTS]
    src, dst = os.path.join(str(tmp_path), "ice_in.bin"), os.path.join(str(tmp_path), "ice_out.bin")
    np.concatenate([np.array(head)] + [np.asarray(c[n], dtype=np.float64).reshape(-1) for n in X.INPUTS]).tofile(src)
    out = subprocess.run([exe, "run", str(ncol), str(nlay), src, dst], stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True)
    assert out.returncode == 0 and out.stdout.startswith("ok"), out.stderr[-2000:]
    flat, got, at = np.fromfile(dst), {}, 0
    for n in ("t_out", "height_out", "thick_out", "snow_out", "tsfc_out", "base_flux_out", "cond_flux", "albedo", "flags"):
        size = nlay * ncol if n in ("t_out", "height_out") else ncol
        got[n] = flat[at:at + size].reshape((nlay, ncol) if size > ncol or n in ("t_out", "height_out") else (ncol,))
        at += size
    assert at == flat.size
    got["flags"] = got["flags"].astype(np.int32)
    return got


def check_program(exe, tmp_path, kind_name, name, nlay, ncol):
    kind = X.KINDS[kind_name]
    c = X.ice_case(kind, name, nlay, ncol)
    got = run_program(exe, tmp_path, kind, c, c["dt"])
    dev = X.deviations(got, c, X.FIELDS)
    assert X.within(dev, X.tolerances(kind_name, name)), (kind_name, name, nlay, ncol, dev)
    assert X.same_bits(got["flags"], c["flags"]), (kind_name, name, nlay, ncol)      # the decisions, exactly
    X.check_exact_properties(kind, name, c, got)      # on the program's own output: what no tolerance covers
    X.energy_budget(kind, c, got)
    return all(X.same_bits(got[f], c[f]) for f in X.FIELDS)


def test_host_program_equals_the_numpy_statements(program, tmp_path):
    """Every case and shape: within the stored tolerances, flags exactly (the program itself holds in place == out of place == without
    the optional outputs, bit for bit)."""
    runs = [check_program(program, tmp_path, kn, name, nlay, ncol) for kn, name in ALL_CASES for nlay in X.NLAYS for ncol in X.NCOLS]
    print("host program: %d of %d runs bit-identical to the statements" % (sum(runs), len(runs)))
    assert len(runs) == 22 * 12


def test_host_program_under_the_address_and_undefined_behaviour_sanitizers(program_sanitized, tmp_path):
    for nlay, ncol in ((3, 1), (3, 65), (10, 64), (30, 130)):
        for kn, name in (("sea_ice", "mixed_types"), ("land_ice", "mixed_types"), ("sea_ice", "melts_away"), ("land_ice", "melt_reverts")):
            check_program(program_sanitized, tmp_path, kn, name, nlay, ncol)
    out = subprocess.run([program_sanitized, "tables"], stdout=subprocess.PIPE, universal_newlines=True, check=True).stdout
    assert out.endswith("ok\n")


def test_table_agrees_with_the_header_and_the_python_layer(program):
    rows = column_table_rows(program, "tables")
    assert all(r["entry"] == ENTRY and r["struct"] == STRUCT for r in rows)
    assert tuple(r["member"] for r in rows) == IN + OUT + DIAG
    assert {r["member"]: (r["io"] == "out", r["type"]) for r in rows} == header_pointer_members(STRUCT)
    assert all((r["io"] == "in") == (r["member"] in IN) for r in rows)
    assert all(r["flag"] == "required" for r in rows if r["member"] in IN + OUT) and all(r["flag"] == "-" for r in rows if r["member"] in DIAG)
    arrays = _lib.COLUMN_ARRAYS[ENTRY]
    assert (arrays["IN"], arrays["DIAG"]) == (IN, DIAG) and not any(r["extent"] == "[nlay+1][ncol]" for r in rows)
    assert_column_rows_agree(rows, ENTRY, STRUCT)      # names, direction, type, in-place pairs and every extent
    assert sorted(n for n, t in arrays["dtype"].items() if t.name == "int32") == sorted(r["member"] for r in rows if r["type"] == "i32") == ["area_type", "flags"]
    assert {r["member"]: r["in_place_of"] for r in rows if r["in_place_of"] != "-"} == IN_PLACE == dict(arrays["in_place"])


def test_the_four_earlier_tables_are_printed_as_before(tmp_path_factory):
    """tools/column_call_check.cpp knows nothing of the new table (one more ColumnMember specialisation changes nothing it prints)."""
    exe = build_host_program(tmp_path_factory, "column_call_check.cpp")
    out = subprocess.run([exe], stdout=subprocess.PIPE, universal_newlines=True, check=True).stdout.split("\n")
    assert out[-2:] == ["ok", ""] and len(out) - 2 == 7 + 20 + 20 + 17
    assert sorted({line.split()[2] for line in out[:-2]}) == ["rrtmg_boundary_layer", "rrtmg_dry_adjust", "rrtmg_emanuel", "rrtmg_simple_physics"]
    assert all(line.split()[5] == "f64" or line.split()[1] == "out" for line in out[:-2])      # no int32 input among them
    assert "surface_ice" not in open(os.path.join(ROOT, "tools", "column_call_check.cpp")).read()


def test_energy_budget_of_the_host_program_on_cold_sea_ice(program, tmp_path):
    """The budget of surface_ice_cases.energy_budget on the `cold` sea-ice columns (and the two basal cases), through the host
    program: the change of the interior heat content equals the two Crank-Nicolson face fluxes x dt, and lf rho x growth closes
    against base_flux_out x dt.  Measured (also on the kernel, tests/test_surface_ice_gpu.py): interior residual at most 4e-7 J m^-2,
    2.5 x 2^-52 of sum hc dz (1 + 4 r) max|T| (asserted at 16 x 2^-52, from the row's operation count); the growth relation to 4
    ulps of lf rho thick.  The whole column's sum(rho c T dz) + lf rho growth does NOT close against the boundary fluxes x dt: the
    folded boundary rows hold the boundary nodes to the new gradient alone, and the face fluxes differ from the net flux by up to
    110 W m^-2 and from base_flux_out by up to 84 W m^-2 on these cases (printed).  The reference's tests/test_conservation.py says
    the same and closes only the zero-forcing step; that one is the next test, with its tolerance."""
    worst = {}
    for name in ("cold", "basal_growth", "basal_melt"):
        for nlay in X.NLAYS:
            for ncol in X.NCOLS:
                c = X.ice_case(0, name, nlay, ncol)
                got = run_program(program, tmp_path, 0, c, c["dt"])
                b = X.energy_budget(0, c, got)
                assert b["columns"] == ncol and b["growth"] > 0.0      # every column took part, and the ice grew or thinned
                worst = {k: max(worst.get(k, 0.0), v) for k, v in b.items()}
    print("energy budget, host program: interior residual %.1e J m^-2 (%.2f x 2^-52 of the rows' scale); not closing: |F_top - net| up to %.0f, "
          "|F_base - base_flux_out| up to %.0f W m^-2" % (worst["residual"], worst["ratio"], worst["face_gap"], worst["base_gap"]))
    assert worst["ratio"] <= X.BUDGET_FACTOR and worst["face_gap"] > 1.0      # (the gap is real: the full budget is not claimed)


def test_reference_zero_forcing_energy_check_through_the_host_program(program, tmp_path):
    """tests/test_conservation.py of the reference (TestSeaIceEnergyConservation): 2 m of sea ice at 260 K, every flux zero, one
    second: rho c h mean(T) changes by the forcing x dt to atol = 1.0 J m^-2 (rtol 0), the reference's own tolerance -- here on the
    host program's output, where the step must also be an exact no-op."""
    n, ncol = 30, 4
    zeros = np.zeros(ncol)
    c = dict(t=np.full((n, ncol), 260.0), height=np.zeros((n, ncol)), thick=np.full(ncol, 2.0), snow=zeros, base=zeros, area_type=np.full(ncol, 3, dtype=np.int32),
             **{f: zeros for f in X.FLUXES})
    got = run_program(program, tmp_path, 0, c, 1.0)
    amount = lambda h, t: X.CONSTANTS["rho_ice"] * X.CONSTANTS["c_ice"] * h * t.mean(axis=0)
    assert (got["flags"] == 1).all()
    assert np.isclose(amount(got["thick_out"], got["t_out"]) - amount(c["thick"], c["t"]), got["base_flux_out"] * 1.0, rtol=0, atol=1.0).all()
    assert X.same_bits(got["t_out"], c["t"]) and X.same_bits(got["thick_out"], c["thick"]) and X.same_bits(got["base_flux_out"], zeros)


# ---- the components on host states: the host program stands in for the context ------------------------------------------------------------
class ProgramContext:
    """Context.surface_ice (host arrays) by the stand-alone host program."""

    def __init__(self, exe, tmp_path):
        self.exe, self.tmp_path, self.calls = exe, tmp_path, []

    def surface_ice(self, kind, t, height, thick, snow, base, fluxes, area_type, dt, constants, **kwargs):
        assert not kwargs and area_type.dtype == np.int32
        self.calls.append((kind, t.shape, dt, dict(constants)))
        c = dict(t=t, height=height, thick=thick, snow=snow, base=base, area_type=area_type, **fluxes)
        got = run_program(self.exe, self.tmp_path, kind, c, dt, constants)
        return {n: got[n] for n in OUT}, {n: got[n] for n in DIAG}


host_state, _without_the_tall_column = X.host_state, X.without_the_tall_column


@pytest.mark.parametrize("kind_name", list(X.KINDS))
def test_components_on_a_host_state_with_a_3d_grid(program, tmp_path, kind_name):
    kind, ny, nx, n = X.KINDS[kind_name], 5, 13, 10
    c, tall = _without_the_tall_column(X.ice_case(kind, "mixed_types", n, ny * nx))
    want = X.ice_statement(kind, *(c[k] for k in X.INPUTS), c["dt"])
    ctx = ProgramContext(program, tmp_path)
    comp = (climt_amd.SeaIce if kind == 0 else climt_amd.LandIce)(context=ctx)
    diag, new = comp(host_state(kind, c, ny, nx), datetime.timedelta(seconds=c["dt"]))
    assert ctx.calls == [(kind, (n, ny * nx), c["dt"], X.constants(kind))]
    assert set(diag) == set(comp.diagnostic_properties) and set(new) >= set(comp.output_properties)
    col = lambda q: q.values.reshape(-1)
    nodes = lambda q: np.transpose(q.values, [q.dims.index(d) for d in ("ice_interface_levels", "lat", "lon")]).reshape(n, -1)
    thick_name = "sea_ice_thickness" if kind == 0 else "land_ice_thickness"
    flux_name = "heat_flux_into_sea_water_due_to_sea_ice" if kind == 0 else "upward_heat_flux_at_ground_level_in_soil"
    got = dict(t_out=nodes(new["snow_and_ice_temperature"]), height_out=nodes(new["height_on_ice_interface_levels"]), thick_out=col(new[thick_name]),
               snow_out=col(new["surface_snow_thickness"]), tsfc_out=col(new["surface_temperature"]), base_flux_out=col(diag[flux_name]),
               cond_flux=col(diag["surface_downward_heat_flux_in_sea_ice"]) if kind == 0 else np.zeros(ny * nx), albedo=col(diag["surface_albedo_for_direct_shortwave"]))
    assert X.within(X.deviations(got, want, X.FIELDS), X.tolerances(kind_name, "mixed_types"))
    assert X.same_bits(diag["surface_albedo_for_direct_shortwave"].values, diag["surface_albedo_for_diffuse_shortwave"].values)
    for name, prop in list(comp.output_properties.items()) + list(comp.diagnostic_properties.items()):
        q = (new if name in comp.output_properties else diag)[name]
        assert q.attrs["units"] == prop["units"] and set(q.dims) == ({"lat", "lon"} | ({"ice_interface_levels"} if "ice_interface_levels" in prop["dims"] else set())), name


@pytest.mark.parametrize("kind_name", list(X.KINDS))
def test_a_column_taller_than_the_maximum_raises_the_references_error(kind_name):
    kind, ny, nx = X.KINDS[kind_name], 5, 13
    c = X.ice_case(kind, "mixed_types", 3, ny * nx)
    assert c["too_tall"].sum() == 1
    comp = (climt_amd.SeaIce if kind == 0 else climt_amd.LandIce)(context=object())
    with pytest.raises(ValueError, match=r"^Total height exceeds maximum value of 10 m\.$"):
        comp(host_state(kind, c, ny, nx), datetime.timedelta(seconds=60))
    roomy = (climt_amd.SeaIce if kind == 0 else climt_amd.LandIce)(maximum_snow_ice_height=0.25, context=object())
    with pytest.raises(ValueError, match=r"^Total height exceeds maximum value of 0.25 m\.$"):
        roomy(host_state(kind, c, ny, nx), datetime.timedelta(seconds=60))


def test_default_state_serves_every_input():
    comps = [climt_amd.SeaIce(context=object()), climt_amd.LandIce(context=object()), climt_amd.SlabSurface(context=object())]
    state = climt_amd.get_default_state(comps, grid_state=climt_amd.get_grid(nx=1, ny=1, nz=10))
    for comp in comps:
        assert all(n in state for n in comp.input_properties), [n for n in comp.input_properties if n not in state]
    assert state["snow_and_ice_temperature"].dims[0] == "ice_interface_levels"
