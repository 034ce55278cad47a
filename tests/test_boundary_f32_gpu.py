"""The float32 boundary on the GPU (rrtmg_hip_{sw,lw,radiation}_fluxes_f32): the results are the bits of the fp64 entry point on
the widened inputs, each output rounded once to float32 -- with device and host pointers, at 4-byte alignment, under every
option that modifies a call -- and nothing outside an output's n * 4 bytes is written.  Inputs: the project's seeded columns
rounded to float32, 13 layers (odd element counts), 1 / 65 / 136 columns (one lane; a tile plus one; two tiles and a ragged one)."""
import ctypes as C

import numpy as np
import pytest

from climt_amd import _lib
from climt_amd._hip import DeviceArray
from climt_amd._lib import LW_OUT, LW_OUT_CLEAR, SW_BAND_FLUXES, SW_COMPONENTS, SW_OUT, SW_OUT_ALLSKY, LW_BAND_FLUXES, RRTMGError
from climt_amd.distributed import slice_columns
from climt_amd.synthetic import make_columns, overcast

pytestmark = pytest.mark.gpu

BASE = dict(icld=1, iaer=0, adjes=1.0, dyofyr=1, scon=1367.0, isolvar=0, inflg=2, iceflg=1, liqflg=1)
NLAY, GUARD = 13, 16
# the project's bounds against the live reference (tests/test_gpu_parity.py): TIGHT for the longwave, the shortwave's live-oracle
# bound (test_randomised_shapes_and_flags_against_emulation) for the shortwave; on top, per element, the half-ulp of the ONE
# rounding to float32: 2**-24 * |reference|
TIGHT, SW_LIVE = 5.0e-9, 1.0e-6
POISON = {np.dtype(np.float32): np.uint32(0x7FC0BEEF), np.dtype(np.float64): np.uint64(0x7FF8DEADBEEF0123)}
_BITS = {np.dtype(np.float32): np.uint32, np.dtype(np.float64): np.uint64}


def columns(ncol, mode, nlay=NLAY, seed=None):
    """-> (x32, x64): the seeded columns rounded to float32, and the same values widened (exact).  mode: "clear" | "mcica" | "mt"."""
    c = make_columns(ncol, nlay, cloudy=mode != "clear", seed=900 + ncol if seed is None else seed)
    c.pop("lat", None)
    c.update(BASE)
    if mode != "clear":
        c.update(irng=1 if mode == "mt" else 0, permuteseed=77, icld=2)
    x32 = {k: (v.astype(np.float32) if isinstance(v, np.ndarray) else v) for k, v in c.items()}
    return x32, widened(x32)


def widened(x32):
    return {k: (v.astype(np.float64) if isinstance(v, np.ndarray) else v) for k, v in x32.items()}


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(_BITS[a.dtype])


class DeviceCall:
    """One device-pointer call: every input one element into a larger allocation (4-byte alignment only under float32), every
    output one element plus GUARD poisoned elements in, GUARD more behind it.  launch(), then collect() -> the outputs, after
    checking that every input allocation and every guard kept its bits."""

    def __init__(self, ctx, which, c, dtype, mcica, components=(), bands=(), band_levels="all", surface=None):
        self.ctx, self.which, self.mcica, self.band_levels = ctx, which, mcica, band_levels
        self.dtype = np.dtype(dtype)
        nlay, ncol = c["play"].shape
        self.inputs, self.outputs = [], {}
        self.inp = dict(nlay=nlay, ncol=ncol)
        for k, v in c.items():
            self.inp[k] = self._input(v) if isinstance(v, np.ndarray) and k not in ("bndsolvar", "indsolvar") else v
        self.surface = None if surface is None else {k: self._input(v) for k, v in surface.items()}
        if which == "sw":
            clear = getattr(ctx, "sw_clear_sky", True)
            self.out = {k: self._output(k, (nlay + lev, ncol)) for k, lev in SW_OUT if clear or k in SW_OUT_ALLSKY}
        else:
            clear = getattr(ctx, "lw_clear_sky", True)
            self.out = {k: self._output(k, (nlay + lev, ncol)) for k, lev in LW_OUT if clear or k not in LW_OUT_CLEAR}
            if c.get("idrv"):
                self.out["duflx_dt"] = self._output("duflx_dt", (nlay + 1, ncol))
                if clear:
                    self.out["duflxc_dt"] = self._output("duflxc_dt", (nlay + 1, ncol))
        nrow = 2 if band_levels == "boundaries" else nlay + 1
        self.components = {k: self._output("c." + k, (nlay + 1, ncol)) for k in components} or None
        self.bands = {k: self._output("b." + k, (14 if which == "sw" else 16, nrow, ncol)) for k in bands} or None

    def _input(self, v):
        host = np.empty(v.size + 1, self.dtype)
        host.view(_BITS[self.dtype])[0] = POISON[self.dtype]
        host[1:] = v.ravel()
        d = DeviceArray.from_host(host)
        self.inputs.append((d, host))
        return d.ptr + self.dtype.itemsize

    def _output(self, name, shape):
        n = int(np.prod(shape))
        host = np.empty(1 + GUARD + n + GUARD, self.dtype)
        host.view(_BITS[self.dtype])[:] = POISON[self.dtype]
        d = DeviceArray.from_host(host)
        self.outputs[name] = (d, shape)
        return d.ptr + self.dtype.itemsize * (1 + GUARD)

    def launch(self):
        kw = dict(mcica=self.mcica, out=self.out, memspace=1, precision=self.dtype.name)
        if self.bands:
            kw.update(bands=self.bands, band_levels=self.band_levels)
        if self.which == "sw":
            self.ctx.sw_fluxes(self.inp, components=self.components, surface=self.surface, **kw)
        else:
            self.ctx.lw_fluxes(self.inp, **kw)
        return self

    def collect(self):
        for d, host in self.inputs:
            assert np.array_equal(bits(d.download()), bits(host)), "an input buffer changed"
        res = {}
        for name, (d, shape) in self.outputs.items():
            got, n = d.download(), int(np.prod(shape))
            guards = np.concatenate([bits(got)[:1 + GUARD], bits(got)[1 + GUARD + n:]])
            assert len(guards) == 1 + 2 * GUARD and (guards == POISON[self.dtype]).all(), "guard of %s overwritten" % name
            res[name] = got[1 + GUARD:1 + GUARD + n].reshape(shape)
        return res


def device_call(ctx, which, c, dtype, mcica, **kw):
    return DeviceCall(ctx, which, c, dtype, mcica, **kw).launch().collect()


def host_call(ctx, which, c, dtype, mcica, **kw):
    """A host-pointer call -> every output (components as "c.<name>", bands as "b.<name>"); the inputs must keep their bits."""
    dtype = np.dtype(dtype)
    before = {k: v.copy() for k, v in c.items() if isinstance(v, np.ndarray)}
    nlay, ncol = c["play"].shape
    comps = {k: np.zeros((nlay + 1, ncol), dtype) for k in kw.pop("components", ())} or None
    nrow = 2 if kw.get("band_levels") == "boundaries" else nlay + 1
    bands = {k: np.zeros((14 if which == "sw" else 16, nrow, ncol), dtype) for k in kw.pop("bands", ())} or None
    if bands:
        kw.update(bands=bands)
    else:
        kw.pop("band_levels", None)
    if which == "sw":
        res = dict(ctx.sw_fluxes(c, mcica=mcica, components=comps, precision=dtype.name, **kw))
    else:
        res = dict(ctx.lw_fluxes(c, mcica=mcica, precision=dtype.name, **kw))
    for k, v in before.items():
        assert np.array_equal(bits(c[k]), bits(v)), "input %s changed" % k
    res.update({"c." + k: v for k, v in (comps or {}).items()})
    res.update({"b." + k: v for k, v in (bands or {}).items()})
    assert all(v.dtype == dtype for v in res.values())
    return res


def same_as_rounded(got32, want64, what=""):
    assert set(got32) == set(want64), (what, sorted(got32), sorted(want64))
    for k, v in want64.items():
        assert got32[k].dtype == np.float32 and v.dtype == np.float64, (what, k)
        assert np.array_equal(bits(got32[k]), bits(v.astype(np.float32))), (what, k, float(np.abs(got32[k] - v).max()))


CASES = [(n, m) for n in (1, 65, 136) for m in ("clear", "mcica")] + [(136, "mt")]
_fp64, _oracle = {}, {}


def fp64_reference(ctx, which, ncol, mode, idrv):
    """The fp64 entry point on the widened inputs (host pointers), once per case."""
    key = (which, ncol, mode, idrv)
    if key not in _fp64:
        _, x64 = columns(ncol, mode)
        _fp64[key] = host_call(ctx, which, dict(x64, idrv=idrv) if which == "lw" else x64, np.float64, mode != "clear")
    return _fp64[key]


@pytest.mark.parametrize("pointers", ["device", "host"])
@pytest.mark.parametrize("ncol,mode", CASES)
def test_same_bits_as_the_fp64_call_rounded_once(gpu_ctx, ncol, mode, pointers):
    """1 + 2: all six outputs (eight with idrv), both spectra; device pointers 4-byte aligned only, guards and inputs intact."""
    x32, _ = columns(ncol, mode)
    call = device_call if pointers == "device" else host_call
    mcica = mode != "clear"
    same_as_rounded(call(gpu_ctx, "sw", x32, np.float32, mcica), fp64_reference(gpu_ctx, "sw", ncol, mode, 0), "sw")
    for idrv in (0, 1):
        got = call(gpu_ctx, "lw", dict(x32, idrv=idrv), np.float32, mcica)
        assert len(got) == (8 if idrv else 6)
        same_as_rounded(got, fp64_reference(gpu_ctx, "lw", ncol, mode, idrv), "lw idrv %d" % idrv)


@pytest.mark.parametrize("ncol,mode", [c for c in CASES if c[1] != "mt"])
def test_against_the_live_reference(gpu_ctx, ncol, mode):
    """3: the reference (oracle/_ref) fed the widened inputs; bound = the project's bound for that comparison + 2**-24 |reference|."""
    from helpers import live_oracle
    x32, x64 = columns(ncol, mode)
    mcica = mode != "clear"
    rsw, rlw, kind = live_oracle(x64, mcica, chunk=256, procs=1)
    assert kind == "reference"
    for which, ref, bound in (("sw", rsw, SW_LIVE), ("lw", rlw, TIGHT)):
        got = device_call(gpu_ctx, which, x32, np.float32, mcica)
        for k, r in ref.items():
            err = np.abs(got[k].astype(np.float64) - r)
            worst = float((err - 2.0 ** -24 * np.abs(r)).max())
            print("%s %s %d %s: max(|f32 - reference| - 2^-24 |reference|) = %.3e (bound %.1e)" % (which, k, ncol, mode, worst, bound))
            assert (err <= bound + 2.0 ** -24 * np.abs(r)).all(), (which, k, worst)


def test_subnormal_input_and_subnormal_results(gpu_ctx):
    """4: a cloud ice path of 1e-41f (subnormal) survives the widening; shortwave fluxes that land in the float32 subnormal
    range narrow as numpy does.  (The driver clamps coszen at 1e-10, as the reference does, so the smallest cosine alone leaves
    fluxes of ~4e-8 W m^-2: the Earth-Sun factor adjes, a by-value double, scales them down into the subnormal range.)"""
    x32, _ = columns(136, "mcica")
    lay, col = np.argwhere(x32["cldfr"] > 0)[0]
    x32["cicewp"][lay, col] = np.float32(1e-41)
    assert 0 < x32["cicewp"][lay, col] < np.finfo(np.float32).tiny
    x64 = widened(x32)
    assert x64["cicewp"][lay, col] == float(np.float32(1e-41))
    for which in ("sw", "lw"):
        want = host_call(gpu_ctx, which, x64, np.float64, True)
        same_as_rounded(device_call(gpu_ctx, which, x32, np.float32, True), want, which)
        same_as_rounded(host_call(gpu_ctx, which, x32, np.float32, True), want, which)
    y32, _ = columns(65, "clear")
    y32["coszen"][:] = np.float32(1e-10)
    y32["coszen"][::3] = np.float32(3e-7)
    y32.update(adjes=1.0e-33, dyofyr=0)      # (dyofyr 0: the flux adjustment is adjes as given, not the day's Earth-Sun distance)
    want = host_call(gpu_ctx, "sw", widened(y32), np.float64, False)
    tiny = float(np.finfo(np.float32).tiny)
    surface = np.abs(want["swdflx"][0])
    assert ((surface > 2.0 ** -149) & (surface < tiny)).any(), "no surface flux in the float32 subnormal range: %r" % (surface[:6],)
    got = device_call(gpu_ctx, "sw", y32, np.float32, False)
    same_as_rounded(got, want, "subnormal results")
    sub = (got["swdflx"] != 0) & (np.abs(got["swdflx"]) < np.float32(tiny))
    assert sub.any()      # denormals survived the narrowing on the device
    same_as_rounded(host_call(gpu_ctx, "sw", y32, np.float32, False), want, "subnormal results, host")


def test_night_columns_are_positive_zero(gpu_ctx):
    x32, x64 = columns(136, "mcica")
    night = np.zeros(136, bool); night[5:70] = True; night[100::7] = True
    x32["coszen"][night] = 0.0
    x64 = widened(x32)
    gpu_ctx.set_sw_night_skip(True)
    try:
        want = device_call(gpu_ctx, "sw", x64, np.float64, True)
        for call in (device_call, host_call):
            got = call(gpu_ctx, "sw", x32, np.float32, True)
            same_as_rounded(got, want)
            for k, v in got.items():
                assert (bits(v[:, night]) == 0).all(), k      # +0.0f exactly
                assert (v[:, ~night] != 0).any(), k
    finally:
        gpu_ctx.set_sw_night_skip(False)


# ---- 5: options compose ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("levels", ["all", "boundaries"])
def test_components_and_band_fluxes(gpu_ctx, levels):
    x32, x64 = columns(136, "mcica")
    kw = dict(components=SW_COMPONENTS, bands=SW_BAND_FLUXES, band_levels=levels)
    want = device_call(gpu_ctx, "sw", x64, np.float64, True, **kw)
    assert len(want) == 6 + 8 + 6
    same_as_rounded(device_call(gpu_ctx, "sw", x32, np.float32, True, **kw), want)
    same_as_rounded(host_call(gpu_ctx, "sw", x32, np.float32, True, **kw), want)
    kw = dict(bands=LW_BAND_FLUXES, band_levels=levels)
    want = device_call(gpu_ctx, "lw", x64, np.float64, True, **kw)
    same_as_rounded(device_call(gpu_ctx, "lw", x32, np.float32, True, **kw), want)
    same_as_rounded(host_call(gpu_ctx, "lw", x32, np.float32, True, **kw), want)


def test_per_band_albedo_as_float32(gpu_ctx):
    x32, x64 = columns(136, "mcica")
    rng = np.random.default_rng(5)
    s32 = dict(albdir=rng.uniform(0.03, 0.4, (14, 136)).astype(np.float32), albdif=rng.uniform(0.03, 0.4, (14, 136)).astype(np.float32))
    s64 = {k: v.astype(np.float64) for k, v in s32.items()}
    want = device_call(gpu_ctx, "sw", x64, np.float64, True, surface=s64)
    plain = fp64_reference(gpu_ctx, "sw", 136, "mcica", 0)
    assert not np.array_equal(want["swuflx"], plain["swuflx"])      # the albedo by band is what was used
    same_as_rounded(device_call(gpu_ctx, "sw", x32, np.float32, True, surface=s32), want)
    same_as_rounded(host_call(gpu_ctx, "sw", x32, np.float32, True, surface=s32), want)


def test_clear_sky_streams_off_with_null_outputs(gpu_ctx):
    x32, x64 = columns(136, "mcica")
    gpu_ctx.set_sw_clear_sky(False); gpu_ctx.set_lw_clear_sky(False)
    try:
        for which, n in (("sw", 3), ("lw", 3)):
            want = device_call(gpu_ctx, which, x64, np.float64, True)
            assert len(want) == n      # (the clear-sky members of the struct are NULL)
            same_as_rounded(device_call(gpu_ctx, which, x32, np.float32, True), want)
            same_as_rounded(host_call(gpu_ctx, which, x32, np.float32, True), want)
        want = device_call(gpu_ctx, "lw", dict(x64, idrv=1), np.float64, True)
        assert len(want) == 4
        same_as_rounded(device_call(gpu_ctx, "lw", dict(x32, idrv=1), np.float32, True), want)
    finally:
        gpu_ctx.set_sw_clear_sky(True); gpu_ctx.set_lw_clear_sky(True)


def test_column_sort(gpu_ctx):
    x32, x64 = columns(136, "mcica")
    assert (x32["cldfr"] > 0).any(axis=0).any() and not (x32["cldfr"] > 0).any(axis=0).all()      # both kinds of column
    gpu_ctx.set_column_sort(True)
    try:
        for which in ("sw", "lw"):
            same_as_rounded(device_call(gpu_ctx, which, x32, np.float32, True), device_call(gpu_ctx, which, x64, np.float64, True), which)
    finally:
        gpu_ctx.set_column_sort(False)


def test_day_pack_with_a_terminator(gpu_ctx):
    x32, _ = columns(136, "mcica")
    lon = np.arange(136) * (2.0 * np.pi / 136)
    x32["coszen"] = np.maximum(np.cos(lon + 0.3), 0.0).astype(np.float32)      # a terminator: day and night columns in every tile
    night = x32["coszen"] <= 0
    assert 30 < night.sum() < 106
    x64 = widened(x32)
    gpu_ctx.set_sw_night_skip(True); gpu_ctx.set_sw_night_pack(True)
    try:
        want = device_call(gpu_ctx, "sw", x64, np.float64, True, components=SW_COMPONENTS)
        counts = gpu_ctx.sw_night_last()
        got = device_call(gpu_ctx, "sw", x32, np.float32, True, components=SW_COMPONENTS)
        assert gpu_ctx.sw_night_last() == counts and counts[1] == int(night.sum())
        same_as_rounded(got, want)
        assert all((bits(v[:, night]) == 0).all() for v in got.values())
    finally:
        gpu_ctx.set_sw_night_pack(False); gpu_ctx.set_sw_night_skip(False)


def test_deferred_mode(gpu_ctx):
    x32, x64 = columns(136, "mcica")
    want = {w: device_call(gpu_ctx, w, x64, np.float64, True) for w in ("sw", "lw")}
    gpu_ctx.set_deferred(True)
    try:
        sw = DeviceCall(gpu_ctx, "sw", x32, np.float32, True).launch()
        lw = DeviceCall(gpu_ctx, "lw", x32, np.float32, True).launch()
        gpu_ctx.synchronize()
        same_as_rounded(sw.collect(), want["sw"], "sw")
        same_as_rounded(lw.collect(), want["lw"], "lw")
    finally:
        gpu_ctx.set_deferred(False)


def test_two_shards_equal_the_whole(gpu_ctx):
    x32, x64 = columns(136, "mcica")
    for which in ("sw", "lw"):
        whole = device_call(gpu_ctx, which, x32, np.float32, True)
        same_as_rounded(whole, fp64_reference(gpu_ctx, which, 136, "mcica", 0), which)
        parts = [device_call(gpu_ctx, which, dict(slice_columns(x32, lo, hi), shard_col0=lo, shard_ncol=136), np.float32, True) for lo, hi in ((0, 64), (64, 136))]
        for k, v in whole.items():
            assert np.array_equal(bits(np.concatenate([p[k] for p in parts], axis=1)), bits(v)), (which, k)


# ---- 6: the host path -----------------------------------------------------------------------------------------------------------
def test_unit_factors_on_float32_host_arrays(gpu_ctx):
    x32, _ = columns(136, "mcica")
    raw = dict(x32)
    raw["play"] = (x32["play"] * np.float32(100.0)).astype(np.float32); raw["plev"] = (x32["plev"] * np.float32(100.0)).astype(np.float32)
    raw["cicewp"] = (x32["cicewp"] / np.float32(1000.0)).astype(np.float32); raw["cliqwp"] = (x32["cliqwp"] / np.float32(1000.0)).astype(np.float32)
    raw["h2o"] = (x32["h2o"] * np.float32(18.02 / 28.964)).astype(np.float32)
    raw.update(pressure_scale=0.01, water_path_scale=1000.0, h2o_mul=28.964, h2o_div=18.02)
    for which in ("sw", "lw"):
        want = host_call(gpu_ctx, which, widened(raw), np.float64, True)      # the fp64 call applies the same factors to the same doubles
        same_as_rounded(host_call(gpu_ctx, which, raw, np.float32, True), want, which)
        plain = fp64_reference(gpu_ctx, which, 136, "mcica", 0)
        # the factors were applied: the clear-sky fluxes (no kissvec seeds from the re-rounded pressures in them) are those of the call
        # on arrays in the library's own units, to the rounding of the raw arrays
        k = "swdflxc" if which == "sw" else "dflxc"
        assert float(np.abs(want[k] - plain[k]).max()) < 1.0e-2


def test_uniform_and_all_zero_arrays_cross_the_scan_threshold(gpu_ctx):
    """2176 x 61 = 132 736 elements >= kScanMin: a uniform gas array is filled on the device, an all-(+0.0f) taucld is absent;
    then one -0.0f in it makes it present."""
    x32, _ = columns(2176, "mcica", nlay=61)
    assert x32["co2"].size >= 1 << 17 and (bits(x32["co2"]) == bits(x32["co2"]).flat[0]).all()
    x32["taucld"] = np.zeros((61, 2176, 16), np.float32)
    for minus in (False, True):
        if minus:
            x32["taucld"][40, 1234, 7] = np.float32(-0.0)
            assert bits(x32["taucld"]).any()
        want = host_call(gpu_ctx, "lw", widened(x32), np.float64, True)
        same_as_rounded(host_call(gpu_ctx, "lw", x32, np.float32, True), want, "minus zero %s" % minus)


def test_joint_call_equals_the_separate_calls(gpu_ctx):
    x32, x64 = columns(136, "mcica")
    sw, lw = host_call(gpu_ctx, "sw", x32, np.float32, True), host_call(gpu_ctx, "lw", x32, np.float32, True)
    jsw, jlw = gpu_ctx.radiation_fluxes(sw=dict(inp=x32, mcica=True), lw=dict(inp=x32, mcica=True), precision="float32")
    n32, up32, sh32 = gpu_ctx.radiation_last()
    for got, want in ((jsw, sw), (jlw, lw)):
        assert set(got) == set(want)
        for k in want:
            assert got[k].dtype == np.float32 and np.array_equal(bits(got[k]), bits(want[k])), k
    gpu_ctx.radiation_fluxes(sw=dict(inp=x64, mcica=True), lw=dict(inp=x64, mcica=True))
    n64, up64, sh64 = gpu_ctx.radiation_last()
    assert n32 == n64 and n32 > 0
    # every array of this size is structured (below the scan threshold): uploaded once, 4 bytes per element
    sw_names = "play plev tlay h2o o3 co2 ch4 n2o o2 asdir aldir asdif aldif coszen cldfr cicewp cliqwp reice reliq".split()
    lw_only = "tsfc tlev cfc11 cfc12 cfc22 ccl4 emis".split()
    elements = sum(x32[k].size for k in sw_names + lw_only)
    assert up32 == 4 * elements and up64 == 8 * elements and sh32 * 2 == sh64


# ---- 7, 8: errors, and the default path untouched ----------------------------------------------------------------------------------
def test_refusals_leave_the_context_usable(gpu_ctx):
    x32, x64 = columns(65, "mcica")
    before = {w: host_call(gpu_ctx, w, x64, np.float64, True) for w in ("sw", "lw")}

    def unchanged():
        for w in ("sw", "lw"):
            again = host_call(gpu_ctx, w, x64, np.float64, True)
            assert all(np.array_equal(bits(again[k]), bits(before[w][k])) for k in again), w

    for which in ("sw", "lw"):
        with pytest.raises(RRTMGError) as e:      # a unit factor with device pointers
            device_call(gpu_ctx, which, dict(x32, pressure_scale=0.01), np.float32, True)
        assert e.value.code == 4
        unchanged()
        with pytest.raises(RRTMGError) as e:      # a required input that is NULL
            device_call(gpu_ctx, which, {k: v for k, v in x32.items() if k != "tlay"}, np.float32, True)
        assert e.value.code == 4
        with pytest.raises(RRTMGError) as e:
            host_call(gpu_ctx, which, {k: v for k, v in x32.items() if k != "o3"}, np.float32, True)
        assert e.value.code == 4
        unchanged()
    # a bad struct_size in an optional struct, through the raw entry points
    keep = []
    dt = _lib.PRECISIONS["float32"]
    a, _, c, b, _ = gpu_ctx._sw_structs(x32, True, None, 0, {"dirdflx": np.zeros((NLAY + 1, 65), np.float32)}, {"up": np.zeros((14, NLAY + 1, 65), np.float32)}, "all", None, keep, dt)
    c.struct_size = 8
    assert gpu_ctx.lib.rrtmg_hip_sw_fluxes_f32(gpu_ctx.h, C.byref(a), None, C.byref(c), C.byref(b)) == 4
    c.struct_size = C.sizeof(c); b.struct_size = 3
    assert gpu_ctx.lib.rrtmg_hip_sw_fluxes_f32(gpu_ctx.h, C.byref(a), None, C.byref(c), C.byref(b)) == 4
    la, lb, _ = gpu_ctx._lw_structs(x32, True, None, 0, {"up": np.zeros((16, NLAY + 1, 65), np.float32)}, "all", keep, dt)
    lb.struct_size = 0
    assert gpu_ctx.lib.rrtmg_hip_lw_fluxes_f32(gpu_ctx.h, C.byref(la), C.byref(lb)) == 4
    a.struct_size = 12
    assert gpu_ctx.lib.rrtmg_hip_sw_fluxes_f32(gpu_ctx.h, C.byref(a), None, None, None) == 4
    unchanged()


def test_fp64_call_after_f32_calls_is_the_fresh_context_s(gpu_ctx):
    from oracle.ref_driver import CONSTANTS, CPDAIR
    x32, x64 = columns(136, "mcica")
    for which in ("sw", "lw"):
        device_call(gpu_ctx, which, x32, np.float32, True); host_call(gpu_ctx, which, x32, np.float32, True)
    after = {w: (host_call(gpu_ctx, w, x64, np.float64, True), device_call(gpu_ctx, w, x64, np.float64, True)) for w in ("sw", "lw")}
    fresh = _lib.Context(0)
    try:
        fresh.set_constants(**CONSTANTS); fresh.sw_init(CPDAIR); fresh.lw_init(CPDAIR)
        for w in ("sw", "lw"):
            for got, call in zip(after[w], (host_call, device_call)):
                want = call(fresh, w, x64, np.float64, True)
                assert all(np.array_equal(bits(got[k]), bits(want[k])) for k in want), w
    finally:
        fresh.close()
