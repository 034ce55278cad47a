"""The array tables of a call (csrc/rrtmg_call_arrays.h) against the public header and the Python layer, on the CPU:
tools/call_arrays_check.cpp prints the tables (and checks their extent functions and group predicates itself); here the set of
(struct, member) pairs it prints is the set of grid-array members of the six call structs parsed from include/rrtmg_hip.h, and
the standard outputs are SW_OUT / LW_OUT of climt_amd/_lib.py.  A member added to the header without a row in the tables
fails here.  The same for the tables of the four column components (csrc/rrtmg_column_call.h): tools/column_call_check.cpp
prints them, and every pointer member of rrtmg_dry_adjust, rrtmg_boundary_layer, rrtmg_emanuel and rrtmg_simple_physics is one
row, named as the *_IN, *_OUT and *_DIAG tuples of climt_amd/_lib.py name it."""
import os
import re
import shutil
import subprocess

import pytest

from climt_amd._lib import LW_BAND_FLUXES, LW_OUT, SW_BAND_FLUXES, SW_COMPONENTS, SW_OUT
from helpers import ROOT, assert_column_rows_agree, build_host_program, column_table_rows, header_pointer_members

STRUCTS = ("rrtmg_sw_args", "rrtmg_sw_surface", "rrtmg_sw_components", "rrtmg_sw_band_fluxes", "rrtmg_lw_args", "rrtmg_lw_band_fluxes")
# double pointers of the structs that are deliberately in no table, each with its reason
NOT_A_CALL_ARRAY = {
    ("rrtmg_sw_args", "tlev"): "the shortwave never reads interface temperatures (the member exists for symmetry with the longwave)",
    ("rrtmg_sw_args", "tsfc"): "the shortwave never reads the surface temperature",
    ("rrtmg_sw_args", "bndsolvar"): "[14] on the host under either memspace: a scalar setting (sw_scalar_setup), not a grid array",
    ("rrtmg_sw_args", "indsolvar"): "[2] on the host under either memspace, IN/OUT: a scalar setting, not a grid array",
}


def header_members():
    """-> {(struct, member): is_output} for every `double *` / `const double *` member of the six structs."""
    text = open(os.path.join(ROOT, "include", "rrtmg_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    found = {}
    for s in STRUCTS:
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (s, s), text, flags=re.S).group(1)
        for const, names in re.findall(r"^\s*(const\s+)?double\s+([^;()]*\*[^;()]*);", body, flags=re.M):
            for n in names.split(","):
                n = n.strip()
                assert n.startswith("*") and "*" not in n[1:], (s, n)
                found[(s, n[1:].strip())] = not const
    return found


@pytest.fixture(scope="module")
def tables(tmp_path_factory):
    hipcc = shutil.which("hipcc") or os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "bin", "hipcc")
    exe = build_host_program(tmp_path_factory, "call_arrays_check.cpp", compiler=[hipcc, "--offload-arch=gfx950", "--offload-host-only"])
    out = subprocess.run([exe], stdout=subprocess.PIPE, universal_newlines=True, check=True).stdout.split("\n")
    assert out[-2:] == ["ok", ""]
    rows = [dict(zip(("spectrum", "io", "struct", "member", "name", "wname", "extent", "k", "group", "flag"), line.split())) for line in out[:-2]]
    assert all(len(r) == 10 for r in rows)
    return rows


COLUMN_STRUCTS = {"rrtmg_dry_adjust": "DRY_ADJUST", "rrtmg_boundary_layer": "BOUNDARY_LAYER", "rrtmg_emanuel": "EMANUEL", "rrtmg_simple_physics": "SIMPLE_PHYSICS"}


@pytest.fixture(scope="module")
def column_tables(tmp_path_factory):
    """The rows tools/column_call_check.cpp prints (it checks the staging plan and the aliasing refusals itself): plain C++, no HIP."""
    return column_table_rows(build_host_program(tmp_path_factory, "column_call_check.cpp"))


def test_every_array_of_a_column_struct_is_one_row_of_its_table(column_tables):
    header = {(s, m): v for s in COLUMN_STRUCTS for m, v in header_pointer_members(s).items()}
    assert len(header) == 7 + 20 + 20 + 17
    printed = {(r["struct"], r["member"]): (r["io"] == "out", r["type"]) for r in column_tables}
    assert len(printed) == len(column_tables), "a member is listed twice"
    assert set(printed) == set(header), (sorted(set(header) - set(printed)), sorted(set(printed) - set(header)))
    assert printed == header      # const <-> input, and the element type


def test_column_rows_agree_with_the_python_layer(column_tables):
    from climt_amd import _lib
    for struct, prefix in COLUMN_STRUCTS.items():
        rows = [r for r in column_tables if r["struct"] == struct]
        IN, OUT, DIAG = (getattr(_lib, "%s_%s" % (prefix, k)) for k in ("IN", "OUT", "DIAG"))
        last = ("cbmf_out",) if struct == "rrtmg_emanuel" else ()      # behind the diagnostics in the struct; neither list has it
        assert tuple(r["member"] for r in rows) == IN + OUT + DIAG + last
        assert all((r["io"] == "in") == (r["member"] in IN) for r in rows)
        assert all(r["flag"] == "required" for r in rows if r["member"] in OUT + last) and all(r["flag"] == "-" for r in rows if r["member"] in DIAG)
        assert {r["member"]: r["in_place_of"] for r in rows if r["in_place_of"] != "-"} == (
            {"cbmf_out": "cbmf"} if last else {n: n[:-4] for n in OUT})
        arrays = _lib.COLUMN_ARRAYS[rows[0]["entry"]]
        assert (arrays["IN"], arrays["DIAG"]) == (IN, DIAG)
        assert_column_rows_agree(rows, rows[0]["entry"], struct)      # names, direction, type, in-place pairs and every extent
        assert {"[ncol]", "[nlay+1][ncol]", "[nlay][ncol]"} >= {r["extent"] for r in rows}


def test_every_grid_array_of_the_header_is_in_a_table(tables):
    header = header_members()
    assert len(header) > 80 and all(k in header for k in NOT_A_CALL_ARRAY)
    printed = {(r["struct"], r["member"]): r["io"] == "out" for r in tables}
    assert len(printed) == len(tables), "a member is listed twice"
    expected = {k: v for k, v in header.items() if k not in NOT_A_CALL_ARRAY}
    assert set(printed) == set(expected), (sorted(set(expected) - set(printed)), sorted(set(printed) - set(expected)))
    assert printed == expected      # const double * <-> input, double * <-> output
    for r in tables:
        assert r["struct"].startswith("rrtmg_%s_" % r["spectrum"])


def test_work_buffer_names_are_unique_within_a_list(tables):
    for spectrum in ("sw", "lw"):
        for io in ("in", "out"):
            names = [r["name"] for r in tables if r["spectrum"] == spectrum and r["io"] == io]
            assert len(set(names)) == len(names)
        staged = [r["wname"] for r in tables if r["spectrum"] == spectrum and r["io"] == "out"]
        assert len(set(staged)) == len(staged) and all(n.startswith("o.") or n.startswith("ob.") for n in staged)


def test_outputs_agree_with_the_python_layer(tables):
    for spectrum, std, extra in (("sw", SW_OUT, ()), ("lw", LW_OUT, (("duflx_dt", 1), ("duflxc_dt", 1)))):
        outs = [r for r in tables if r["spectrum"] == spectrum and r["io"] == "out" and r["struct"].endswith("_args")]
        levels = {"[nlay+1][N]": 1, "[nlay][N]": 0}
        assert [(r["member"], levels[r["extent"]]) for r in outs] == list(std) + list(extra)
        assert [r["name"] for r in outs] == ["o%d" % k for k in range(len(outs))]
        assert [r["flag"] for r in outs] == ["required"] * len(std) + ["-"] * len(extra)
    by_struct = lambda s: [r["member"] for r in tables if r["struct"] == s]
    assert by_struct("rrtmg_sw_components") == list(SW_COMPONENTS)
    assert by_struct("rrtmg_sw_band_fluxes") == list(SW_BAND_FLUXES) and by_struct("rrtmg_lw_band_fluxes") == list(LW_BAND_FLUXES)
    assert all(r["extent"] == "[k*nrow][N]" and r["k"] == ("14" if r["spectrum"] == "sw" else "16") for r in tables if r["struct"].endswith("band_fluxes"))
