"""The Python side of the eleven column components on the CPU, with no library and no device: Context.dry_adjustment ...
Context.second_best (climt_amd/_lib.py) are driven against a recording stand-in (tests/column_call_python_cases.py), under both
calling modes -- made-up device pointers with memspace=1, host arrays at the entry's smallest legal shape -- and what they put
into their structs, return and refuse is compared with tests/golden/column_call_python.json.  That file was recorded at commit
49b6b10, when cork_longwave still carried its own copy of both halves of Context._column_call and an array's extent came from
membership in two name lists; it pins every pointer binding, allocation, in-place outcome and message text across the change
to one table-driven path."""
import ctypes as C
import json
import os

import pytest

import column_call_python_cases as X
from climt_amd import _lib
from helpers import GOLDEN


@pytest.fixture(scope="module")
def golden():
    return json.load(open(os.path.join(GOLDEN, "column_call_python.json")))


def test_the_variants_cover_the_eleven_methods_in_both_modes(golden):
    assert sorted(golden) == sorted(X.VARIANTS)
    methods = {v[0] for v in X.VARIANTS.values()}
    assert len(methods) == 11 and all(callable(getattr(_lib.Context, m)) for m in methods)
    for name, g in golden.items():
        assert {"device", "host", "host, no diagnostics"} <= set(g["calls"]), name
        assert g["scalars"]["memspace"] == 1 and g["calls"]["host"]["scalars_differ"] == {"memspace": 0} and "scalars_differ" not in g["calls"]["device"]
        assert g["scalars"]["ncol"] == X.NCOL and g["scalars"]["nlay"] == X.VARIANTS[name][2]
        assert all(len(c["pointers"] if isinstance(c["pointers"], str) else c["pointers"][0]) == len(g["pointer_members"].split()) for c in g["calls"].values() if "as" not in c)
        assert all(text.startswith("ValueError: ") or text == "accepted" for text in g["refusals"])
    assert {X.VARIANTS[n][0] for n, g in golden.items() if g["refusals"]} == methods and golden["bucket_hydrology_1"]["refusals"] and golden["bucket_hydrology_2"]["refusals"]
    assert [n for n, g in golden.items() if "accepted" in g["refusals"]] == ["frierson_optical_depth"]      # (its grid IS pint's)


@pytest.mark.parametrize("name", list(X.VARIANTS))
def test_structs_returns_and_refusals_are_what_was_recorded(golden, name):
    got, want = X.record_variant(name), golden[name]
    assert sorted(got) == sorted(want) and got["pointer_members"] == want["pointer_members"] and got["scalars"] == want["scalars"]
    for kind in ("calls", "refusals"):
        assert sorted(got[kind]) == sorted(want[kind])
        for k in want[kind]:
            assert got[kind][k] == want[kind][k], (name, kind, k)


def test_the_stand_in_is_called_once_with_a_struct_of_the_entrys_type():
    for name, (method, *_rest) in X.VARIANTS.items():
        v, lib = X.Variant(name), X.RecordingLibrary()
        ctx = X.make_context(lib)
        v.call(ctx, {n: v.array(n) for n in v.IN}, {n: None for n in v.OUT}, None)
        (symbol, a), = lib.calls
        assert symbol == "rrtmg_hip_" + method and a.struct_size == C.sizeof(type(a)) and (a.ncol, a.nlay) == (X.NCOL, v.nlay)
