"""CPU tests of the shortwave's opt-in night-column skip (rrtmg_hip_set_sw_night_skip / rrtmg_hip_sw_night_last,
Context.set_sw_night_skip, RRTMGShortwave(skip_night_columns=True)): the C-ABI surface, the Python layer on the stand-in
context, and the numpy statement of "night tile" that the GPU tests (tests/test_night_skip_gpu.py) hold the kernels to."""
import ctypes as C
import json
import os
import re
import subprocess

import numpy as np
import pytest

import climt_amd
from climt_amd import night
from climt_amd.rrtmg import shortwave
from helpers import GOLDEN, ROOT, EmuContext, load_cache_case

RRTMG_ERR_ARG = 4


def test_library_exports_the_two_symbols_with_the_declared_signatures():
    """Both symbols are exported, declared in the header as the issue states them, RRTMG_HIP_ABI_VERSION is unchanged (callers
    probe by symbol), and they answer on a context of a machine without a GPU: off by default, 0 / 0 reported."""
    from climt_amd._lib import LIB_PATH, load_library
    assert os.path.exists(LIB_PATH), "run __graft_entry__.build() first"
    syms = subprocess.run(["nm", "-D", "--defined-only", LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert " rrtmg_hip_set_sw_night_skip\n" in syms and " rrtmg_hip_sw_night_last\n" in syms
    hdr = open(os.path.join(ROOT, "include", "rrtmg_hip.h")).read()
    code = re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", "", hdr, flags=re.S))
    assert "int rrtmg_hip_set_sw_night_skip(rrtmg_ctx *ctx, int on);" in code
    assert "int rrtmg_hip_sw_night_last(rrtmg_ctx *ctx, int *night_tiles, int *night_columns);" in code
    assert re.search(r"#define RRTMG_HIP_ABI_VERSION 5\b", hdr)
    lib = load_library()
    assert lib.rrtmg_hip_set_sw_night_skip.argtypes == [C.c_void_p, C.c_int]
    assert lib.rrtmg_hip_sw_night_last.argtypes == [C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_int)]
    h = C.c_void_p()
    lib.rrtmg_hip_create(C.byref(h), 0)      # (without a GPU: an error status, and a context that can report errors)
    assert h.value
    try:
        t, c = C.c_int(-1), C.c_int(-1)
        assert lib.rrtmg_hip_sw_night_last(h, C.byref(t), C.byref(c)) == 0 and (t.value, c.value) == (0, 0)
        assert lib.rrtmg_hip_set_sw_night_skip(h, 1) == 0
        t, c = C.c_int(-1), C.c_int(-1)      # no shortwave call has completed: nothing skipped
        assert lib.rrtmg_hip_sw_night_last(h, C.byref(t), C.byref(c)) == 0 and (t.value, c.value) == (0, 0)
        assert lib.rrtmg_hip_set_sw_night_skip(h, 0) == 0
        assert lib.rrtmg_hip_sw_night_last(h, None, C.byref(c)) == RRTMG_ERR_ARG
        assert lib.rrtmg_hip_sw_night_last(h, C.byref(t), None) == RRTMG_ERR_ARG
    finally:
        lib.rrtmg_hip_destroy(h)
    assert lib.rrtmg_hip_set_sw_night_skip(None, 1) == RRTMG_ERR_ARG
    assert lib.rrtmg_hip_sw_night_last(None, C.byref(t), C.byref(c)) == RRTMG_ERR_ARG


def test_header_and_documents_state_the_granularity_and_the_status_code_rule():
    hdr = open(os.path.join(ROOT, "include", "rrtmg_hip.h")).read()
    m = re.search(r"/\*((?:(?!\*/).)*?)\*/\s*int rrtmg_hip_set_sw_night_skip", hdr, flags=re.S)
    assert m, "rrtmg_hip_set_sw_night_skip has no header comment"
    text = re.sub(r"\s+\*?\s*", " ", m.group(1))
    for words in ("coszen <= 0", "64", "mixed tile", "status code", "never column-sorted", "NaN"):
        assert words in text, words
    for doc, words in (("INTEGRATION.md", "rrtmg_hip_sw_night_last"), ("INTEGRATION.md", "rrtmg_hip_set_sw_night_skip"),
                       ("README.md", "rrtmg_hip_set_sw_night_skip"), ("DESIGN.md", "night_skip_ab")):
        assert words in open(os.path.join(ROOT, doc)).read(), (doc, words)
    # the measurement is IN the design document: the four rows of tools/night_skip_ab.py, no template token left
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "@@" not in design
    for row in ("512x256x60", "1440x90x100", "128x64x60", "8192x60"):
        assert re.search(r"^\|[^|\n]*%s" % row, design, flags=re.M), row
    table = open(os.path.join(ROOT, "profiles", "night_skip_ab.txt")).read()
    assert all(r in table for r in ("global512", "global1440", "small128", "allday"))


def _body(src, head):
    """Statements of the function whose definition line starts with `head`, up to its closing brace at column 0."""
    i = src.index(head)
    i = src.index("{\n", i) + 2
    return src[i:src.index("\n}\n", i)].splitlines()


def test_night_preparation_kernel_carries_the_preparation_kernel_body():
    """sw_prep_fused_kernel keeps its own body (its ISA must not move); behind its night test sw_prep_fused_night_kernel runs
    a copy of it: from the first phase on the two must agree line for line (as tests/test_sw_components.py holds the two
    cloudy solve bodies together), and the copy declares the same wave index and LDS."""
    src = open(os.path.join(ROOT, "climt_amd", "csrc", "rrtmg_sw.hip")).read()
    a = _body(src, "__global__ void __launch_bounds__(64 * kPrepWaves) sw_prep_fused_kernel(")
    b = _body(src, "__global__ void __launch_bounds__(64 * kPrepWaves) sw_prep_fused_night_kernel(")
    ta, tb = a[a.index("  if (act)"):], b[b.index("  if (act)"):]
    assert len(ta) > 10 and ta == tb, [(x, y) for x, y in zip(ta, tb) if x != y]
    strip = lambda lines: [re.sub(r"\s*//.*", "", x) for x in lines]
    head_b = strip(b[:b.index("  if (act)")])
    for decl in ("  __shared__ int sh_cld;", "  extern __shared__ int sh_idx[];", "  const int w = threadIdx.x >> 6;"):
        assert decl in head_b, decl
    assert "    return;" in head_b      # the night exit comes first


class RecordingContext(EmuContext):
    """The stand-in context of the host-layer tests, with the switch: it records what the component hands over."""

    def __init__(self, device=0):
        super().__init__(device)
        self.handed = []

    def set_sw_night_skip(self, on=True):
        self.handed.append(on)


@pytest.fixture
def recording_context(monkeypatch):
    made = []

    def mk(device):
        made.append(RecordingContext(device))
        return made[-1]
    monkeypatch.setattr(shortwave, "make_context", mk)
    return made


def test_option_leaves_attributes_and_property_dictionaries_alone(recording_context):
    ref = json.load(open(os.path.join(GOLDEN, "reference_interface.json")))["RRTMGShortwave"]
    cls = climt_amd.RRTMGShortwave
    plain, skip = cls(), cls(skip_night_columns=True)
    for name in ("input_properties", "diagnostic_properties", "tendency_properties"):
        assert getattr(skip, name) is getattr(cls, name) and getattr(plain, name) is getattr(cls, name)
        assert json.loads(json.dumps(getattr(skip, name))) == ref[name]
    for name, val in ref.items():
        if name != "__init__":
            assert getattr(skip, name) == val and getattr(plain, name) == val, name
    import inspect
    assert inspect.signature(cls.__init__).parameters["skip_night_columns"].default is False
    # with the other options: their dictionaries, nothing added by this one
    both = cls(skip_night_columns=True, flux_components=True, band_fluxes=True, spectral_surface_albedo=True)
    assert both.diagnostic_properties == cls.diagnostic_properties_for(True, band_fluxes=True)
    assert both.input_properties == cls.input_properties_for(True)


def test_option_is_handed_to_the_context_before_every_call(recording_context, caplog):
    state, _, _ = load_cache_case("TestRRTMGShortwave", "column")
    skip = climt_amd.RRTMGShortwave(skip_night_columns=True)
    plain = climt_amd.RRTMGShortwave()
    cs, cp = recording_context
    assert cs.handed == [] and cp.handed == []
    with caplog.at_level("INFO"):
        t0, d0 = plain(state)
        assert cp.handed == [False]
        t1, d1 = skip(state)
        assert cs.handed == [True]
        skip(state)
        plain(state)
    assert cs.handed == [True, True] and cp.handed == [False, False]
    assert caplog.text == ""          # no new log message
    # (the stand-in computes what the default does: the hand-over is all this layer adds)
    assert set(d0) == set(d1) and all(np.array_equal(d0[k].values, d1[k].values) for k in d0)


def test_a_context_without_the_switch_serves_the_default_only(monkeypatch):
    monkeypatch.setattr(shortwave, "make_context", lambda device: EmuContext(device))
    state, _, _ = load_cache_case("TestRRTMGShortwave", "column")
    climt_amd.RRTMGShortwave()(state)
    with pytest.raises(RuntimeError, match="set_sw_night_skip"):
        climt_amd.RRTMGShortwave(skip_night_columns=True)(state)


def test_numpy_statement_of_night_tile():
    # a ragged last tile that is all night: 64 day columns, then 10 night ones
    c = np.concatenate([np.full(64, 0.5), np.full(10, -0.2)])
    assert night.night_tiles(c).tolist() == [False, True] and night.mixed_tiles(c).tolist() == [False, False]
    assert night.night_counts(c) == (1, 10)
    # ... and a ragged last tile with one day column is mixed
    c[70] = 1e-300
    assert night.night_tiles(c).tolist() == [False, False] and night.mixed_tiles(c).tolist() == [False, True]
    assert night.night_counts(c) == (0, 9)
    # 0.0 and -0.0 are night
    z = np.zeros(64)
    z[1::2] = -0.0
    assert np.signbit(z[1]) and not np.signbit(z[0])
    assert night.night_columns(z).all() and night.night_tiles(z).tolist() == [True] and night.night_counts(z) == (1, 64)
    # NaN is day: one NaN among night columns makes the tile mixed
    n = np.full(64, -1.0)
    n[17] = np.nan
    assert not night.night_columns(n)[17] and night.night_columns(n).sum() == 63
    assert night.night_tiles(n).tolist() == [False] and night.mixed_tiles(n).tolist() == [True]
    # a single day column in a tile makes the tile mixed; its neighbours are untouched
    g = np.full(192, -0.3)
    g[64 + 5] = 0.25
    assert night.night_tiles(g).tolist() == [True, False, True] and night.mixed_tiles(g).tolist() == [False, True, False]
    assert night.night_counts(g) == (2, 191)
    # below the reference's clamp but above zero: day
    assert not night.night_columns(np.array([1e-11, 1e-10, 5e-324])).any()
    # all day; shapes other than 1-d are taken column by column in memory order
    assert night.night_counts(np.full((4, 40), 0.1)) == (0, 0) and night.night_tiles(np.full((4, 40), 0.1)).shape == (3,)
    assert night.night_counts(np.full((2, 64), -0.1)) == (2, 128)


def test_component_cosine_sets_with_the_sun():
    """Instellation clamps the zenith angle to pi/2, and cos of the double nearest pi/2 is +6e-17: the cosine a night-skipping
    instance hands over is 0.0 from pi/2 on and np.cos() -- the default instance's -- below."""
    f = climt_amd.RRTMGShortwave.night_coszen
    z = np.array([0.0, 1.0, np.nextafter(0.5 * np.pi, 0.0), 0.5 * np.pi, np.nextafter(0.5 * np.pi, 4.0), 2.0, np.pi])
    got = f(z)
    assert np.cos(0.5 * np.pi) > 0.0
    assert np.array_equal(got[:3], np.cos(z[:3])) and np.all(got[:3] > 0.0)
    assert np.all(got[3:] == 0.0) and not np.signbit(got[3:]).any()
    assert night.night_columns(got).tolist() == [False, False, False, True, True, True, True]
    assert f(np.full((2, 3), 0.3)).shape == (2, 3)
