"""CPU tests of the shortwave call without the clear-sky outputs (rrtmg_hip_set_sw_clear_sky, Context.set_sw_clear_sky,
RRTMGShortwave(clear_sky_diagnostics=False)): the C-ABI surface, the Python layer on the stand-in context, and the new mode of
sw_solve_thread on the host (tests/emu, clear_sky = 0) against the committed reference-Fortran fixtures."""
import ctypes as C
import inspect
import json
import os
import re
import subprocess

import numpy as np
import pytest

import climt_amd
from climt_amd.rrtmg import shortwave
from helpers import GOLDEN, REF_CASES, ROOT, EmuContext, emu_sw, load_cache_case, load_opt_case, load_ref_case, maxdiff

RRTMG_ERR_ARG = 4
TIGHT = 5.0e-9      # W m^-2 (K day^-1 for swhr): tests/test_sw_components_gpu.py
ALLSKY = ("swuflx", "swdflx", "swhr")
CLEAR = ("swuflxc", "swdflxc", "swhrc")


def test_library_exports_the_symbol_with_the_declared_signature():
    from climt_amd._lib import LIB_PATH, Context, load_library
    assert os.path.exists(LIB_PATH), "run __graft_entry__.build() first"
    syms = subprocess.run(["nm", "-D", "--defined-only", LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert " rrtmg_hip_set_sw_clear_sky\n" in syms
    hdr = open(os.path.join(ROOT, "include", "rrtmg_hip.h")).read()
    code = re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", "", hdr, flags=re.S))
    assert "int rrtmg_hip_set_sw_clear_sky(rrtmg_ctx *ctx, int on);" in code
    assert re.search(r"#define RRTMG_HIP_ABI_VERSION 5\b", hdr)      # no struct changed: callers probe by symbol
    lib = load_library()
    assert lib.rrtmg_hip_set_sw_clear_sky.argtypes == [C.c_void_p, C.c_int]
    assert callable(Context.set_sw_clear_sky)
    h = C.c_void_p()
    lib.rrtmg_hip_create(C.byref(h), 0)      # (without a GPU: an error status, and a context that takes settings)
    assert h.value
    try:
        assert lib.rrtmg_hip_set_sw_clear_sky(h, 0) == 0 and lib.rrtmg_hip_set_sw_clear_sky(h, 1) == 0
    finally:
        lib.rrtmg_hip_destroy(h)
    assert lib.rrtmg_hip_set_sw_clear_sky(None, 0) == RRTMG_ERR_ARG


def test_header_states_the_contract():
    hdr = open(os.path.join(ROOT, "include", "rrtmg_hip.h")).read()
    m = re.search(r"/\*((?:(?!\*/).)*?)\*/\s*int rrtmg_hip_set_sw_clear_sky", hdr, flags=re.S)
    assert m, "rrtmg_hip_set_sw_clear_sky has no header comment"
    text = re.sub(r"\s+\*?\s*", " ", m.group(1))
    for words in ("may be NULL", "not one element is written", "neither downloaded nor touched", "RRTMG_ERR_ARG", "rrtmg_hip_radiation_fluxes"):
        assert words in text, words


class RecordingContext(EmuContext):
    def __init__(self, device=0):
        super().__init__(device)
        self.handed, self.outs = [], []

    def set_sw_night_skip(self, on=True):
        pass

    def set_sw_clear_sky(self, on=True):
        self.handed.append(on)

    def sw_fluxes(self, inp, mcica=False, out=None, memspace=0):
        self.outs.append(sorted(out))
        full = dict(out)
        for k in CLEAR:      # (the stand-in computes all six)
            full.setdefault(k, np.zeros_like(out["swhr" if k == "swhrc" else "swuflx"]))
        return super().sw_fluxes(inp, mcica=mcica, out=full, memspace=memspace)


@pytest.fixture
def recording_context(monkeypatch):
    made = []

    def mk(device):
        made.append(RecordingContext(device))
        return made[-1]
    monkeypatch.setattr(shortwave, "make_context", mk)
    return made


def test_kwarg_drops_exactly_three_diagnostics(recording_context):
    cls = climt_amd.RRTMGShortwave
    ref = json.load(open(os.path.join(GOLDEN, "reference_interface.json")))["RRTMGShortwave"]
    assert inspect.signature(cls.__init__).parameters["clear_sky_diagnostics"].default is True
    plain, allsky = cls(), cls(clear_sky_diagnostics=False)
    assert plain.diagnostic_properties is cls.diagnostic_properties and cls(clear_sky_diagnostics=True).diagnostic_properties is cls.diagnostic_properties
    assert json.loads(json.dumps(cls.diagnostic_properties)) == ref["diagnostic_properties"]      # the class attribute stays
    gone = set(cls.diagnostic_properties) - set(allsky.diagnostic_properties)
    assert gone == set(shortwave.CLEAR_SKY_DIAGNOSTICS) and len(gone) == 3 and all(k.endswith("_assuming_clear_sky") for k in gone)
    assert set(allsky.diagnostic_properties) <= set(cls.diagnostic_properties)
    assert all(allsky.diagnostic_properties[k] == cls.diagnostic_properties[k] for k in allsky.diagnostic_properties)
    assert allsky.diagnostic_properties == cls.diagnostic_properties_for(clear_sky_diagnostics=False)
    assert allsky.input_properties is cls.input_properties and allsky.tendency_properties is cls.tendency_properties


@pytest.mark.parametrize("other", ["flux_components", "band_fluxes"])
def test_kwarg_refuses_components_and_bands(recording_context, other):
    with pytest.raises(ValueError, match=other):
        climt_amd.RRTMGShortwave(clear_sky_diagnostics=False, **{other: True})
    climt_amd.RRTMGShortwave(clear_sky_diagnostics=True, **{other: True})


def test_setting_is_handed_to_the_context_before_every_call(recording_context):
    state, _, _ = load_cache_case("TestRRTMGShortwave", "column")
    allsky, plain = climt_amd.RRTMGShortwave(clear_sky_diagnostics=False), climt_amd.RRTMGShortwave()
    ca, cp = recording_context
    t0, d0 = plain(state)
    t1, d1 = allsky(state)
    allsky(state)
    plain(state)
    assert ca.handed == [False, False] and cp.handed == [True, True]
    assert ca.outs[0] == sorted(ALLSKY) and cp.outs[0] == sorted(ALLSKY + CLEAR)      # three arrays handed over, not six
    assert set(d0) - set(d1) == set(shortwave.CLEAR_SKY_DIAGNOSTICS)
    assert all(np.array_equal(d0[k].values, d1[k].values) for k in d1) and np.array_equal(t0["air_temperature"].values, t1["air_temperature"].values)


def test_a_context_without_the_setting_serves_the_default_only(monkeypatch):
    class Old(EmuContext):
        def set_sw_night_skip(self, on=True):
            pass
    monkeypatch.setattr(shortwave, "make_context", lambda device: Old(device))
    state, _, _ = load_cache_case("TestRRTMGShortwave", "column")
    climt_amd.RRTMGShortwave()(state)
    with pytest.raises(RuntimeError, match="set_sw_clear_sky"):
        climt_amd.RRTMGShortwave(clear_sky_diagnostics=False)(state)


# ---- the new mode of sw_solve_thread on the host -------------------------------------------------------------------------------
def sw_allsky_only(inp, mcica):
    """helpers.emu_sw without the clear-sky outputs on the inputs `inp` -> {swuflx, swdflx, swhr}, NaN where nothing was written."""
    nlay, ncol = inp["play"].shape
    return emu_sw(inp, mcica, clear_sky=False, out={k: np.full((nlay + (k != "swhr"), ncol), np.nan) for k in ALLSKY})[0]


CLOUDY_REF = tuple(n for n in REF_CASES if not n.startswith("clear"))


def test_cloudy_reference_cases_are_the_mcica_and_overcast_ones():
    assert CLOUDY_REF == ("overcast_L60", "mcica_kiss_random", "mcica_kiss_maxrand", "mcica_mt_max")


@pytest.mark.parametrize("case", CLOUDY_REF)
def test_emulated_allsky_only_mode_vs_reference_fixture(case):
    """One column at a time through sw_solve_item in the all-sky-only mode, then sw_flux_level / sw_heat_layer restricted to the
    all-sky outputs: within TIGHT of the reference Fortran, and the clear-sky half of the scratch slab is never written (the
    emulation unit poisons it and checks)."""
    c, mcica, exp = load_ref_case(case)
    assert (np.asarray(c["cldfr"]) > 0).any()
    out = sw_allsky_only(c, mcica)
    for k in ALLSKY:
        assert np.isfinite(out[k]).all(), k
        d = maxdiff(out[k], exp["sw"][k])
        print("%s %s: max |emulated - reference| = %.3e" % (case, k, d))
        assert d <= TIGHT, (case, k, d)
    assert float(np.abs(out["swdflx"] - exp["sw"]["swdflxc"]).max()) > 1.0      # (the clouds matter: all-sky != clear-sky here)


@pytest.mark.parametrize("request_", [dict(components=("dirdflx", "difdflx")), dict(bands=("up", "dn")), dict(bands=("dndir",), levels="boundaries")])
def test_emulated_allsky_only_mode_refuses_components_and_bands(request_):
    """As sw_fluxes_impl: flux components and band fluxes need the clear-sky stream."""
    from climt_amd._lib import RRTMGError
    c, mcica, _ = load_ref_case("overcast_L60")
    with pytest.raises(RRTMGError) as e:
        emu_sw(c, mcica, clear_sky=False, **request_)
    assert e.value.code == RRTMG_ERR_ARG, (e.value.code, str(e.value))
    emu_sw(c, mcica, **request_)      # (the default mode serves the same request)


def test_emulated_allsky_only_mode_with_ecmwf_aerosols_vs_reference_fixture():
    """iaer = 6 (the six ECMWF aerosol types, mixed per band in the driver's set-up) on the cloudy option fixture: the all-sky
    outputs within TIGHT of the reference Fortran, as in the default mode (tests/test_device_functions_emulated.py)."""
    spectrum, mcica, c, exp = load_opt_case("sw_aer6_mcica")
    assert spectrum == "sw" and c["iaer"] == 6 and (np.asarray(c["cldfr"]) > 0).any() and np.asarray(c["ecaer"]).max() > 0.0
    out = sw_allsky_only(c, mcica)
    for k in ALLSKY:
        assert np.isfinite(out[k]).all(), k
        d = maxdiff(out[k], exp[k])
        print("sw_aer6_mcica %s: max |emulated - reference| = %.3e" % (k, d))
        assert d <= TIGHT, (k, d)
    assert float(np.abs(out["swdflx"] - exp["swdflxc"]).max()) > 1.0      # (the clouds matter)


def _body(src, head):
    """Statements of the function whose definition line starts with `head`, up to its closing brace at column 0."""
    i = src.index(head)
    i = src.index("{\n", i) + 2
    return src[i:src.index("\n}\n", i)].splitlines()


def test_allsky_cloudy_kernel_carries_the_cloudy_kernel_body():
    """sw_solve_cloudy_allsky_kernel carries a copy of sw_solve_cloudy_kernel's body (as tests/test_sw_components.py holds
    sw_solve_cloudy_body to it): with its own workgroup shape written as the default kernel's, the two agree but for the mode."""
    src = open(os.path.join(ROOT, "climt_amd", "csrc", "rrtmg_sw.hip")).read()
    a = _body(src, "__global__ void __launch_bounds__(64 * kC4Waves) __attribute__((amdgpu_waves_per_eu(2, 2))) sw_solve_cloudy_kernel(")
    b = _body(src, "__global__ void __launch_bounds__(64 * kAsWaves)")
    b = [x.replace("kAsWaves", "kC4Waves").replace("kAsGroupsPerBlock", "kC4GroupsPerBlock") for x in b]
    assert len(a) == len(b) > 10
    diff = [(x, y) for x, y in zip(a, b) if x != y]
    assert diff == [("  sw_solve_item<true, true>(d, T, sh_exp, item, col, scr, 64, sink, sh_k);",
                     "  sw_solve_item<true, true, true>(d, T, sh_exp, item, col, scr, 64, sink, sh_k);")], diff
