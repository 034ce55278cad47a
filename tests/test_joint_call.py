"""CPU tests of the joint shortwave + longwave host call: the C surface (symbols, header), and climt_amd.radiation_step on a
recording stand-in context -- one radiation_fluxes call whose two argument sets are what sw_fluxes / lw_fluxes receive from
the two separate component calls, the shared state arrays being the very same objects in both."""
import os
import re
import subprocess

import numpy as np
import pytest

import climt_amd
from climt_amd import _lib
from climt_amd.rrtmg import longwave, shortwave
from helpers import ROOT

SHARED_STATE_INPUTS = ("play", "plev", "tlay", "h2o", "o3", "co2", "ch4", "n2o", "o2", "cldfr", "cicewp", "cliqwp", "reice", "reliq")


def test_symbols_header_and_abi_version():
    syms = subprocess.check_output(["nm", "-D", "--defined-only", _lib.LIB_PATH]).decode()
    assert re.search(r" T rrtmg_hip_radiation_fluxes\b", syms) and re.search(r" T rrtmg_hip_radiation_last\b", syms)
    hdr = open(os.path.join(ROOT, "include", "rrtmg_hip.h")).read()
    flat = " ".join(hdr.split())
    assert "int rrtmg_hip_radiation_fluxes(rrtmg_ctx *ctx, const rrtmg_radiation_call *call);" in flat
    assert "int rrtmg_hip_radiation_last(rrtmg_ctx *ctx, int *arrays_shared, long long *bytes_uploaded, long long *bytes_shared);" in flat
    body = re.search(r"typedef struct rrtmg_radiation_call \{(.*?)\} rrtmg_radiation_call;", hdr, re.S).group(1)
    members = re.findall(r"^\s*(?:const )?(\w+) \*?(\w+);", body, re.M)
    assert members == [("int", "struct_size"), ("rrtmg_sw_args", "sw"), ("rrtmg_sw_surface", "sw_surface"), ("rrtmg_sw_components", "sw_components"),
                       ("rrtmg_sw_band_fluxes", "sw_bands"), ("rrtmg_lw_args", "lw"), ("rrtmg_lw_band_fluxes", "lw_bands")]
    assert [n for n, _ in _lib.RadiationCall._fields_] == [m for _, m in members]
    assert "#define RRTMG_HIP_ABI_VERSION 5" in hdr
    lib = _lib.load_library()
    assert lib.rrtmg_hip_abi_version() == 5 and hasattr(lib, "rrtmg_hip_radiation_fluxes")


class RecordingContext:
    """Stand-in for climt_amd._lib.Context: records every flux call and writes a recognisable pattern into the outputs."""

    def __init__(self, device=0, synthetic=False):
        self.device, self.synthetic, self.calls, self.night = device, synthetic, [], []

    def set_constants(self, **k):
        pass

    def sw_init(self, cpdair, blob=None):
        pass

    def lw_init(self, cpdair, blob=None):
        pass

    def lw_tables_synthetic(self):
        return self.synthetic

    def set_sw_night_skip(self, on=True):
        self.night.append(bool(on))

    @staticmethod
    def _write(kw, base):
        for group in ("out", "components", "bands"):
            for i, (k, v) in enumerate(sorted((kw.get(group) or {}).items())):
                v[...] = base + i + np.arange(v.size).reshape(v.shape) * 1.0e-3

    def sw_fluxes(self, **kw):
        self.calls.append(("sw_fluxes", kw))
        self._write(kw, 100.0)

    def lw_fluxes(self, **kw):
        self.calls.append(("lw_fluxes", kw))
        self._write(kw, 200.0)

    def radiation_fluxes(self, sw, lw):
        self.calls.append(("radiation_fluxes", dict(sw=sw, lw=lw)))
        self._write(sw, 100.0)
        self._write(lw, 200.0)


@pytest.fixture
def recording(monkeypatch):
    ctx = RecordingContext()
    monkeypatch.setattr(shortwave, "make_context", lambda device: ctx)
    monkeypatch.setattr(longwave, "make_context", lambda device: ctx)
    return ctx


def default_state(sw, lw):
    return climt_amd.get_default_state([sw, lw], grid_state=climt_amd.get_grid(nx=4, ny=3, nz=10))


def same_arguments(joint, separate, what):
    """Same keys; arrays equal in value (outputs excepted: the pool hands out other buffers), flags and scales equal."""
    assert set(joint) == set(separate), what
    for k in separate:
        a, b = joint[k], separate[k]
        if isinstance(b, dict):
            same_arguments(a, b, what + "." + k)
        elif isinstance(b, np.ndarray):
            assert isinstance(a, np.ndarray) and a.shape == b.shape and a.dtype == b.dtype, (what, k)
            if not re.search(r"\.(out|components|bands)$", what):
                assert np.array_equal(a, b), (what, k)
        else:
            assert type(a) is type(b) and a == b, (what, k, a, b)


CASES = {
    "default": (dict(), dict()),
    "mcica_twister": (dict(mcica=True), dict(mcica=True)),
    "mcica_kissvec": (dict(mcica=True, random_number_generator="kissvec"), dict(mcica=True, random_number_generator="kissvec")),
    "components_bands_albedo": (dict(flux_components=True, band_fluxes=True, spectral_surface_albedo=True), dict(band_fluxes=True)),
    "change_up_flux": (dict(), dict(calculate_change_up_flux=True)),
}


@pytest.mark.parametrize("case", list(CASES))
def test_one_library_call_with_the_arguments_of_the_two_separate_calls(recording, case):
    skw, lkw = CASES[case]
    sw, lw = climt_amd.RRTMGShortwave(**skw), climt_amd.RRTMGLongwave(**lkw)
    state = default_state(sw, lw)
    np.random.seed(3)
    want_sw, want_lw = sw(state), lw(state)
    separate = dict(recording.calls)
    assert [n for n, _ in recording.calls] == ["sw_fluxes", "lw_fluxes"]
    seeds = (getattr(sw, "_permute_seed", None), getattr(lw, "_permute_seed", None))
    lw.change_in_upward_flux_with_surface_temperature = lw.change_in_clear_sky_upward_flux_with_surface_temperature = None
    del recording.calls[:], recording.night[:]
    np.random.seed(3)
    got_sw, got_lw = climt_amd.radiation_step(sw, lw, state)
    assert [n for n, _ in recording.calls] == ["radiation_fluxes"] and recording.night == [False]
    joint = recording.calls[0][1]
    same_arguments(joint["sw"], separate["sw_fluxes"], "sw")
    same_arguments(joint["lw"], separate["lw_fluxes"], "lw")
    assert (getattr(sw, "_permute_seed", None), getattr(lw, "_permute_seed", None)) == seeds
    if "mcica" in case:
        assert seeds[0] is not None and seeds[0] != seeds[1]      # drawn shortwave first, then longwave
        assert joint["sw"]["inp"]["permuteseed"] == seeds[0] and joint["lw"]["inp"]["permuteseed"] == seeds[1]
    # the shared state quantities are the same OBJECTS in both argument sets (that is what the library's table matches) ...
    si, li = joint["sw"]["inp"], joint["lw"]["inp"]
    for k in SHARED_STATE_INPUTS:
        assert isinstance(si[k], np.ndarray) and si[k] is li[k], k
    assert all(si.get(k) == li.get(k) for k in ("pressure_scale", "water_path_scale", "h2o_mul", "h2o_div"))
    # ... which two separate calls do not give
    assert any(separate["sw_fluxes"]["inp"][k] is not separate["lw_fluxes"]["inp"][k] for k in SHARED_STATE_INPUTS)
    # what follows the library call ran: the shortwave's copy, the longwave's alias, the duflx_dt attributes
    for (gt, gd), (wt, wd), name in ((got_sw, want_sw, "shortwave"), (got_lw, want_lw, "longwave")):
        for g, w in ((gt, wt), (gd, wd)):
            assert list(g) == list(w)
            for k in w:
                assert type(g[k]) is type(w[k]) and g[k].dims == w[k].dims and g[k].attrs == w[k].attrs, k
                assert np.array_equal(g[k].values, w[k].values), (name, k)
        tend, diag = gt["air_temperature"].values, gd["air_temperature_tendency_from_" + name].values
        assert np.array_equal(tend, diag) and np.shares_memory(tend, diag) == (name == "longwave")
    if case == "change_up_flux":
        assert lw.change_in_upward_flux_with_surface_temperature is joint["lw"]["out"]["duflx_dt"]
        assert lw.change_in_clear_sky_upward_flux_with_surface_temperature is joint["lw"]["out"]["duflxc_dt"]
    else:
        assert lw.change_in_upward_flux_with_surface_temperature is None


def test_night_skip_is_applied_before_the_call(recording):
    sw, lw = climt_amd.RRTMGShortwave(skip_night_columns=True), climt_amd.RRTMGLongwave()
    climt_amd.radiation_step(sw, lw, default_state(sw, lw))
    assert recording.night == [True] and [n for n, _ in recording.calls] == ["radiation_fluxes"]


def test_refusals(monkeypatch):
    made = []

    def mk(device):
        made.append(RecordingContext(device))
        return made[-1]
    monkeypatch.setattr(shortwave, "make_context", mk)
    monkeypatch.setattr(longwave, "make_context", mk)
    sw, lw = climt_amd.RRTMGShortwave(), climt_amd.RRTMGLongwave(device=1)
    state = default_state(sw, lw)
    with pytest.raises(ValueError, match="different contexts or devices"):
        climt_amd.radiation_step(sw, lw, state)
    with pytest.raises(ValueError, match="RRTMGShortwave and an RRTMGLongwave"):
        climt_amd.radiation_step(lw, sw, state)
    assert all(not c.calls for c in made)
    # a DeviceState has its own overlapped path
    ctx = RecordingContext()
    monkeypatch.setattr(shortwave, "make_context", lambda device: ctx)
    monkeypatch.setattr(longwave, "make_context", lambda device: ctx)
    sw, lw = climt_amd.RRTMGShortwave(), climt_amd.RRTMGLongwave()
    ds = climt_amd.DeviceState.__new__(climt_amd.DeviceState)
    with pytest.raises(ValueError, match="DeviceState"):
        climt_amd.radiation_step(sw, lw, ds)
    assert not ctx.calls
    # a longwave on synthetic tables that has not been allowed to run keeps its existing error: there is no such component
    monkeypatch.delenv("RRTMG_HIP_ALLOW_SYNTHETIC_LW", raising=False)
    monkeypatch.setattr(longwave, "make_context", lambda device: RecordingContext(device, synthetic=True))
    with pytest.raises(RuntimeError, match="SYNTHETIC"):
        climt_amd.RRTMGLongwave()


def test_context_radiation_fluxes_refuses_unknown_keywords():
    ctx = object.__new__(_lib.Context)
    import threading
    ctx._lock, ctx.lib = threading.RLock(), _lib.load_library()
    with pytest.raises(TypeError, match="memspace"):
        ctx.radiation_fluxes(sw=dict(inp={}, memspace=1), lw=dict(inp={}))
    with pytest.raises(TypeError, match="'inp'"):
        ctx.radiation_fluxes(sw=dict(inp={}), lw=dict(mcica=True))
