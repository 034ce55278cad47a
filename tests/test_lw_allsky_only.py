"""CPU tests of the longwave call without the clear-sky outputs (rrtmg_hip_set_lw_clear_sky, Context.set_lw_clear_sky,
RRTMGLongwave(clear_sky_diagnostics=False)): the C-ABI surface, the Python layer on the stand-in context, and the one-stream
mode of lw_solve_thread on the host (tests/emu, clear_sky = 0) against the committed reference-Fortran fixtures."""
import ctypes as C
import inspect
import json
import os
import re
import subprocess

import numpy as np
import pytest

import band_cases as B
import climt_amd
from climt_amd.rrtmg import longwave
from helpers import GOLDEN, LWMR_CASES, REF_CASES, ROOT, EmuContext, emu_lw, load_cache_case, load_lwmr_case, load_ref_case, maxdiff

RRTMG_ERR_ARG = 4
TIGHT = 5.0e-9      # W m^-2 (K day^-1 for hr): the project's bound against the reference Fortran (tests/test_gpu_parity.py)
ALLSKY = ("uflx", "dflx", "hr")
CLEAR = ("uflxc", "dflxc", "hrc")


def test_library_exports_the_symbol_with_the_declared_signature():
    from climt_amd._lib import LIB_PATH, Context, load_library
    assert os.path.exists(LIB_PATH), "run __graft_entry__.build() first"
    syms = subprocess.run(["nm", "-D", "--defined-only", LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert " rrtmg_hip_set_lw_clear_sky\n" in syms
    hdr = open(os.path.join(ROOT, "include", "rrtmg_hip.h")).read()
    code = re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", "", hdr, flags=re.S))
    assert "int rrtmg_hip_set_lw_clear_sky(rrtmg_ctx *ctx, int on);" in code
    assert re.search(r"#define RRTMG_HIP_ABI_VERSION 5\b", hdr)      # no struct changed: callers probe by symbol
    lib = load_library()
    assert lib.rrtmg_hip_set_lw_clear_sky.argtypes == [C.c_void_p, C.c_int]
    assert callable(Context.set_lw_clear_sky) and isinstance(Context.has_lw_clear_sky, property)
    h = C.c_void_p()
    lib.rrtmg_hip_create(C.byref(h), 0)      # (without a GPU: an error status, and a context that takes settings)
    assert h.value
    try:
        assert lib.rrtmg_hip_set_lw_clear_sky(h, 0) == 0 and lib.rrtmg_hip_set_lw_clear_sky(h, 1) == 0
        assert lib.rrtmg_hip_set_sw_clear_sky(h, 0) == 0 and lib.rrtmg_hip_set_lw_clear_sky(h, 1) == 0      # (independent switches)
    finally:
        lib.rrtmg_hip_destroy(h)
    assert lib.rrtmg_hip_set_lw_clear_sky(None, 0) == RRTMG_ERR_ARG


def test_header_states_the_contract():
    hdr = open(os.path.join(ROOT, "include", "rrtmg_hip.h")).read()
    m = re.search(r"/\*((?:(?!\*/).)*?)\*/\s*int rrtmg_hip_set_lw_clear_sky", hdr, flags=re.S)
    assert m, "rrtmg_hip_set_lw_clear_sky has no header comment"
    text = re.sub(r"\s+\*?\s*", " ", m.group(1))
    for words in ("may be NULL", "not one element is written", "neither downloaded nor touched", "RRTMG_ERR_ARG", "rrtmg_hip_radiation_fluxes"):
        assert words in text, words


class RecordingContext(EmuContext):
    def __init__(self, device=0):
        super().__init__(device)
        self.handed, self.outs = [], []

    def set_lw_clear_sky(self, on=True):
        self.handed.append(on)

    def lw_fluxes(self, inp, mcica=False, out=None, memspace=0, bands=None):
        self.outs.append(sorted(out))
        full = dict(out)
        for k in CLEAR:      # (the stand-in computes all six, and eight with idrv)
            full.setdefault(k, np.zeros_like(out["hr" if k == "hrc" else "uflx"]))
        if "duflx_dt" in out:
            full.setdefault("duflxc_dt", np.zeros_like(out["duflx_dt"]))
        return super().lw_fluxes(inp, mcica=mcica, out=full, memspace=memspace)


@pytest.fixture
def recording_context(monkeypatch):
    made = []

    def mk(device):
        made.append(RecordingContext(device))
        return made[-1]
    monkeypatch.setattr(longwave, "make_context", mk)
    monkeypatch.setenv("RRTMG_HIP_ALLOW_SYNTHETIC_LW", "1")
    return made


def test_kwarg_drops_exactly_three_diagnostics(recording_context):
    cls = climt_amd.RRTMGLongwave
    ref = json.load(open(os.path.join(GOLDEN, "reference_interface.json")))["RRTMGLongwave"]
    assert inspect.signature(cls.__init__).parameters["clear_sky_diagnostics"].default is True
    plain, allsky = cls(), cls(clear_sky_diagnostics=False)
    assert plain.diagnostic_properties is cls.diagnostic_properties and cls(clear_sky_diagnostics=True).diagnostic_properties is cls.diagnostic_properties
    assert json.loads(json.dumps(cls.diagnostic_properties)) == ref["diagnostic_properties"]      # the class attribute stays
    gone = set(cls.diagnostic_properties) - set(allsky.diagnostic_properties)
    assert gone == set(longwave.CLEAR_SKY_DIAGNOSTICS) and len(gone) == 3 and all(k.endswith("_assuming_clear_sky") for k in gone)
    assert set(allsky.diagnostic_properties) <= set(cls.diagnostic_properties)
    assert all(allsky.diagnostic_properties[k] == cls.diagnostic_properties[k] for k in allsky.diagnostic_properties)
    assert allsky.diagnostic_properties == cls.diagnostic_properties_for(clear_sky_diagnostics=False)
    assert allsky.tendency_properties is cls.tendency_properties
    assert cls.diagnostic_properties_for(True) == dict(cls.diagnostic_properties, **{k: longwave._prop(longwave._BIL, "W m^-2") for k in longwave.BAND_FLUX_DIAGNOSTICS})


def test_kwarg_refuses_clear_sky_bands_and_allows_all_sky_ones(recording_context):
    cls = climt_amd.RRTMGLongwave
    with pytest.raises(ValueError, match="band_fluxes"):
        cls(clear_sky_diagnostics=False, band_fluxes=True)
    for name in longwave.CLEAR_SKY_BAND_DIAGNOSTICS:
        with pytest.raises(ValueError, match="band_fluxes"):
            cls(clear_sky_diagnostics=False, band_fluxes=[name])
    assert len(longwave.CLEAR_SKY_BAND_DIAGNOSTICS) == 2
    cls(clear_sky_diagnostics=True, band_fluxes=True)
    allsky_bands = [k for k in longwave.BAND_FLUX_DIAGNOSTICS if k not in longwave.CLEAR_SKY_BAND_DIAGNOSTICS]
    comp = cls(clear_sky_diagnostics=False, band_fluxes=allsky_bands)
    assert set(comp.diagnostic_properties) == (set(cls.diagnostic_properties) - set(longwave.CLEAR_SKY_DIAGNOSTICS)) | set(allsky_bands)
    with pytest.raises(ValueError, match="unknown"):
        cls(band_fluxes=["no_such_flux_by_band"])


@pytest.mark.parametrize("idrv", [False, True])
def test_setting_is_handed_to_the_context_before_every_call(recording_context, idrv):
    state, _, _ = load_cache_case("TestRRTMGLongwave", "column")
    allsky = climt_amd.RRTMGLongwave(clear_sky_diagnostics=False, calculate_change_up_flux=idrv)
    plain = climt_amd.RRTMGLongwave(calculate_change_up_flux=idrv)
    ca, cp = recording_context
    t0, d0 = plain(state)
    t1, d1 = allsky(state)
    allsky(state)
    plain(state)
    assert ca.handed == [False, False] and cp.handed == [True, True]
    dr, drc = (("duflx_dt",), ("duflxc_dt",)) if idrv else ((), ())
    assert ca.outs[0] == sorted(ALLSKY + dr) and cp.outs[0] == sorted(ALLSKY + CLEAR + dr + drc)      # three arrays, not six (four, not eight)
    assert len(ca.outs[0]) == (4 if idrv else 3) and len(cp.outs[0]) == (8 if idrv else 6)
    assert set(d0) - set(d1) == set(longwave.CLEAR_SKY_DIAGNOSTICS)
    assert all(np.array_equal(d0[k].values, d1[k].values) for k in d1) and np.array_equal(t0["air_temperature"].values, t1["air_temperature"].values)
    assert allsky.change_in_clear_sky_upward_flux_with_surface_temperature is None
    if idrv:
        assert plain.change_in_clear_sky_upward_flux_with_surface_temperature is not None
        assert np.array_equal(allsky.change_in_upward_flux_with_surface_temperature, plain.change_in_upward_flux_with_surface_temperature)
    else:
        assert allsky.change_in_upward_flux_with_surface_temperature is None


def test_a_context_without_the_setting_serves_the_default_only(monkeypatch):
    monkeypatch.setattr(longwave, "make_context", lambda device: EmuContext(device))
    monkeypatch.setenv("RRTMG_HIP_ALLOW_SYNTHETIC_LW", "1")
    state, _, _ = load_cache_case("TestRRTMGLongwave", "column")
    climt_amd.RRTMGLongwave()(state)
    with pytest.raises(RuntimeError, match="set_lw_clear_sky"):
        climt_amd.RRTMGLongwave(clear_sky_diagnostics=False)(state)


def test_context_passes_null_for_the_absent_outputs():
    """Context._lw_structs after set_lw_clear_sky(False): a clear-sky member of rrtmg_lw_args is NULL where `out` leaves it out
    or holds None; an array that `out` does hold is handed over as it is (the library ignores it: tests/test_lw_allsky_only_gpu.py)."""
    from climt_amd._lib import Context
    ctx = Context.__new__(Context)      # (no library call is made: only the struct is filled)
    inp = dict(play=np.ones((3, 2)), idrv=1)
    ctx.lw_clear_sky = False
    a, _, out = ctx._lw_structs(inp, False, None, 0, None, "all", [])
    assert sorted(out) == sorted(ALLSKY + ("duflx_dt",))
    assert a.uflx and a.dflx and a.hr and a.duflx_dt and not (a.uflxc or a.dflxc or a.hrc or a.duflxc_dt)
    given = dict(out, uflxc=None, hrc=np.zeros((3, 2)), duflxc_dt=12345)
    a, _, _ = ctx._lw_structs(inp, False, given, 0, None, "all", [])
    assert not (a.uflxc or a.dflxc) and a.hrc == given["hrc"].ctypes.data and a.duflxc_dt == 12345
    ctx.lw_clear_sky = True
    a, _, out = ctx._lw_structs(inp, False, None, 0, None, "all", [])
    assert len(out) == 8 and all(getattr(a, k) for k in out)


# ---- the one-stream mode of lw_solve_thread on the host ------------------------------------------------------------------------
def lw_allsky_only(inp, mcica, **kwargs):
    """helpers.emu_lw without the clear-sky outputs on the inputs `inp` -> ({uflx, dflx, hr[, duflx_dt]}, NaN where nothing was
    written; band arrays | None)."""
    nlay, ncol = inp["play"].shape
    out = {k: np.full((nlay + (k != "hr"), ncol), np.nan) for k in ALLSKY + (("duflx_dt",) if inp.get("idrv") else ())}
    return emu_lw(inp, mcica, clear_sky=False, out=out, **kwargs)


CLOUDY_REF = tuple(n for n in REF_CASES if not n.startswith("clear"))


def check_against_reference(case, out, exp, keys):
    for k in keys:
        assert np.isfinite(out[k]).all(), k
        d = maxdiff(out[k], exp[k])
        print("%s %s: max |emulated - reference| = %.3e" % (case, k, d))
        assert d <= TIGHT, (case, k, d)
    assert float(np.abs(out["dflx"] - exp["dflxc"]).max()) > 1.0      # (the clouds matter: all-sky != clear-sky here)
    assert float(np.abs(exp["dflx"] - exp["dflxc"]).max()) > 1.0


@pytest.mark.parametrize("case", CLOUDY_REF)
def test_emulated_allsky_only_mode_vs_reference_fixture(case):
    """One column at a time through lw_solve_item in the one-stream mode, then lw_flux_level_allsky / lw_heat_layer_allsky:
    within TIGHT of the reference Fortran; the emulation unit poisons what the mode does not own -- the partial planes behind
    the compact layout's, the scratch behind the item's rows -- and fails if any of it changed (the clear-sky output pointers
    are NULL)."""
    assert CLOUDY_REF == ("overcast_L60", "mcica_kiss_random", "mcica_kiss_maxrand", "mcica_mt_max")
    c, mcica, exp = load_ref_case(case)
    assert (np.asarray(c["cldfr"]) > 0).any()
    check_against_reference(case, lw_allsky_only(c, mcica)[0], exp["lw"], ALLSKY)


@pytest.mark.parametrize("case", LWMR_CASES)
def test_emulated_allsky_only_mode_vs_rtrnmr_fixture(case):
    """The same through MR = true (non-McICA maximum / random overlap, rtrnmr); maxrand_idrv also checks duflx_dt."""
    assert LWMR_CASES == ("maxrand", "maxrand_idrv", "maximum")
    c, exp = load_lwmr_case(case)
    out = lw_allsky_only(c, False)[0]
    assert ("duflx_dt" in out) == (case == "maxrand_idrv")
    check_against_reference(case, out, exp, ALLSKY + (("duflx_dt",) if "duflx_dt" in out else ()))


CLOUDY_BAND_CASES = tuple(n for n in B.LW_CASES if B.CASES[n][0]["cloudy"])


@pytest.mark.parametrize("case", CLOUDY_BAND_CASES)
def test_emulated_allsky_only_band_fluxes_vs_reference_fixture(case):
    """lw_band_level_allsky, the per-thread rule of lw_bandflux_allsky_kernel, on LwPartSinkAllsky's planes: up and dn by band
    within TIGHT of the reference's own band sums (tests/golden/ref_bands_<case>.npz), and summing to uflx / dflx of the same
    run within band_cases.SUM_BOUND; the clear-sky members are refused, as by the library."""
    from climt_amd._lib import RRTMGError
    assert CLOUDY_BAND_CASES == ("lw_mcica_kiss_random", "lw_maxrand", "lw_cloudy_L100")
    c, mcica, bb, exp = B.load_case(case)
    assert (np.asarray(c["cldfr"]) > 0).any()
    out, band = lw_allsky_only(c, mcica, bands=("up", "dn"))
    for m in ("up", "dn"):
        k = B.BROADBAND["lw"][m]
        assert np.isfinite(band[m]).all() and band[m].min() >= 0.0, m
        d = maxdiff(band[m], exp[m])
        print("%s %s by band: max |emulated - reference| = %.3e" % (case, m, d))
        assert d <= TIGHT, (case, m, d)
        assert maxdiff(out[k], bb[k]) <= TIGHT, (case, k)
        assert np.all(np.abs(band[m].sum(axis=0) - out[k]) <= B.SUM_BOUND * np.abs(out[k])), (case, m)
    assert float(np.abs(band["dn"] - exp["dnc"]).max()) > 1.0      # (the clouds matter, band by band too)
    _, two = lw_allsky_only(c, mcica, bands=("up", "dn"), levels="boundaries")
    nlay = c["play"].shape[0]
    assert all(np.array_equal(two[m], band[m][:, [0, nlay]]) for m in ("up", "dn"))
    for members in (("upc",), ("up", "dnc")):
        with pytest.raises(RRTMGError) as e:
            lw_allsky_only(c, mcica, bands=members)
        assert e.value.code == RRTMG_ERR_ARG, (e.value.code, str(e.value))


def _body(src, head):
    """Statements of the function whose definition line starts with `head`, up to its closing brace at column 0."""
    i = src.index("\n", src.index(head)) + 1
    return src[i:src.index("\n}\n", i)].splitlines()


def test_allsky_solve_kernel_carries_the_solve_kernel_body():
    """lw_solve_all_kernel keeps its own body (its ISA must not move) and lw_solve_all_allsky_kernel carries a copy of it: the
    two agree line for line but for the sink and the mode (comments aside)."""
    import re
    src = open(os.path.join(ROOT, "climt_amd", "csrc", "rrtmg_lw.hip")).read()
    head = "__global__ void __launch_bounds__(64 * kLwWgWaves) __attribute__((amdgpu_waves_per_eu(2))) "
    strip = lambda lines: [re.sub(r"\s*//.*", "", x) for x in lines if not x.strip().startswith("//")]
    a, b = strip(_body(src, head + "lw_solve_all_kernel(")), strip(_body(src, head + "lw_solve_all_allsky_kernel("))
    a = [x for x in a if x != "  constexpr bool kLdsK = true;"]
    assert len(a) == len(b) > 10
    diff = [(x, y) for x, y in zip(a, b) if x != y]
    assert diff == [("  LwPartSink sink = lw_part_sink(d, slot, col);", "  LwPartSinkAllsky sink = lw_part_sink_allsky(d, slot, col);"),
                    ("  lw_solve_item<CLD, MR, kLdsK>(d, T, item, col, scr, 64, sink, sh_k);", "  lw_solve_item<CLD, MR, true, CLD>(d, T, item, col, scr, 64, sink, sh_k);")], diff
