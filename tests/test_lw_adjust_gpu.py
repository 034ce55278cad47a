"""The longwave between radiation calls on the GPU (run with -m gpu on an MI355X): rrtmg_hip_lw_adjust_surface against the numpy
statement of tests/lw_adjust_cases.py bit for bit, dT = 0 against the flux call's own outputs, first-order accuracy against a
second full call, IntermittentLongwave on a host state and on a DeviceState, and the stream ordering of a deferred context."""
import datetime

import numpy as np
import pytest

import climt_amd
from climt_amd import _hip
from climt_amd.rrtmg.common import physical_constants

import lw_adjust_cases as X

pytestmark = pytest.mark.gpu

OUT = ("uflx", "hr", "uflxc", "hrc")


def device_adjust(ctx, c, clear=True, in_place=False, pressure_scale=0.0, synchronize=True):
    """One rrtmg_hip_lw_adjust_surface call on uploaded copies of the arrays of `c` -> ({name: array}, the device arrays)."""
    nlev, ncol = c["uflx"].shape
    d = {k: _hip.DeviceArray.from_host(c[k]) for k in ("tsfc_call", "tsfc_now", "plev", "uflx", "dflx", "duflx_dt") + (("uflxc", "dflxc", "duflxc_dt") if clear else ())}
    streams = []
    for up, dn, du, hr in X.STREAMS[:2 if clear else 1]:
        d[up + "_out"] = d[up] if in_place else _hip.DeviceArray.from_host(np.full((nlev, ncol), np.nan))
        d[hr + "_out"] = _hip.DeviceArray.from_host(np.full((nlev - 1, ncol), np.nan))
        streams.append((d[up], d[dn], d[du], d[up + "_out"], d[hr + "_out"]))
    ctx.lw_adjust_surface(ncol, nlev - 1, d["tsfc_call"], d["tsfc_now"], d["plev"], streams[0], streams[1] if clear else None, pressure_scale=pressure_scale)
    if synchronize:
        ctx.synchronize()
    return {k: d[k + "_out"].download() for k in OUT[:4 if clear else 2]}, d


# ---- 1. bits against numpy -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("in_place", [False, True], ids=["out_of_place", "in_place"])
@pytest.mark.parametrize("clear", [True, False], ids=["both_streams", "all_sky_only"])
def test_kernel_equals_the_numpy_statement_bit_for_bit(gpu_ctx, clear, in_place):
    assert gpu_ctx.has_lw_adjust
    for ncol in (1, 63, 64, 65, 136, 257):
        for nlay in (1, 2, X.CHUNK - 1, X.CHUNK, X.CHUNK + 1, 60):
            c = X.case(ncol, nlay)
            got, d = device_adjust(gpu_ctx, c, clear, in_place)
            want = X.want(c, clear)
            assert set(got) == set(want)
            for k in want:
                assert not np.isnan(got[k]).any(), (ncol, nlay, k)
                assert X.same_bits(got[k], want[k]), (ncol, nlay, k, float(np.abs(got[k] - want[k]).max()))
            for k in ("tsfc_call", "tsfc_now", "plev", "dflx", "duflx_dt") + (() if in_place else ("uflx",)):
                assert X.same_bits(d[k].download(), c[k]), (ncol, nlay, k)      # the inputs are only read
    # plev in Pa with the flux call's pressure_scale
    c = X.case(136, X.CHUNK + 1, pascal=True)
    got, _ = device_adjust(gpu_ctx, c, clear, in_place, pressure_scale=0.01)
    for k, w in X.want(c, clear, pressure_scale=0.01).items():
        assert X.same_bits(got[k], w), k


# ---- 2, 3. real flux calls -------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def flux_calls(gpu_ctx):
    """Per state: the call at tsfc (idrv = 1) and the call at tsfc + dT, explicit tlev held fixed, same McICA seed -- computed once."""
    cache = {}

    def get(name):
        if name not in cache:
            c, mcica = X.flux_state(name)
            dT = X.surface_change()
            base = gpu_ctx.lw_fluxes(c, mcica=mcica)
            moved = dict(c, tsfc=c["tsfc"] + dT)
            full = gpu_ctx.lw_fluxes(moved, mcica=mcica)
            cache[name] = (c, dT, base, full)
        return cache[name]
    return get


def kept_arrays(c, base, tsfc_now):
    return dict(tsfc_call=c["tsfc"], tsfc_now=tsfc_now, plev=c["plev"], **{k: base[k] for k in ("uflx", "dflx", "duflx_dt", "uflxc", "dflxc", "duflxc_dt")})


@pytest.mark.parametrize("name", list(X.STATES))
def test_no_change_of_the_surface_returns_the_calls_own_bits(gpu_ctx, flux_calls, name):
    c, _, base, _ = flux_calls(name)
    assert float(np.abs(base["duflx_dt"]).max()) > 1.0 and float(base["uflx"].min()) > 50.0
    for in_place in (False, True):
        got, _ = device_adjust(gpu_ctx, kept_arrays(c, base, c["tsfc"].copy()), True, in_place)
        for k in OUT:
            assert X.same_bits(got[k], base[k]), (name, in_place, k, float(np.abs(got[k] - base[k]).max()))


@pytest.mark.parametrize("name", list(X.STATES))
def test_first_order_accuracy_against_the_full_call(gpu_ctx, flux_calls, name):
    """Per column with |dT| >= 0.5 K and for uflx, uflxc, hr, hrc: max over levels |adjusted - full(tsfc + dT)| <= 5 % of max over
    levels |unadjusted - full(tsfc + dT)| + 1e-9.  The bound is the issue's, derived: the neglected term is 1/2 (B''/B') dT, about
    1.6 % at 3 K in the window bands near 288 K, with a threefold margin for the band weighting of the synthetic k-tables.  The
    host emulation of the existing code gives a worst ratio of 0.0174 at these states (docs/EXPERIMENTS.md), inside the bound."""
    c, dT, base, full = flux_calls(name)
    got, _ = device_adjust(gpu_ctx, kept_arrays(c, base, c["tsfc"] + dT))
    assert (np.abs(dT) >= 0.5).sum() > 60 and (dT == 0.0).sum() >= 30
    for k, (err, ref) in X.first_order_ratios(base, full, got, dT).items():
        worst = float((err / ref).max())
        print("%s %s: worst ratio %.4f, smallest reference %.3e" % (name, k, worst, float(ref.min())))
        assert ref.min() > 1e-3, (name, k)      # the full call did move
        assert np.all(err <= 0.05 * ref + 1e-9), (name, k, worst)
    still = dT == 0.0
    for k in OUT:
        assert X.same_bits(got[k][:, still], base[k][:, still]), (name, k)      # dT = 0: still the call's bits


# ---- 4, 5. the wrapper ------------------------------------------------------------------------------------------------------------------
NX, NLAY = 33, 9
STEP = datetime.timedelta(minutes=60)
UPDATE = 3 * STEP
START = datetime.datetime(2000, 3, 20, 6, 0)
WARMING = (0.0, 1.25, -2.5, 0.75)      # K added to the surface temperature before steps 1..4


class Spy(climt_amd.RRTMGLongwave):
    calls = 0

    def array_call(self, state):
        self.calls += 1
        return super().array_call(state)


def make_state(lw):
    state = climt_amd.get_default_state([lw], grid_state=climt_amd.get_grid(nx=NX, ny=1, nz=NLAY))
    p = state["air_pressure"].values
    state["air_temperature"].values[:] = np.maximum(200.0, 290.0 * (p / 1.0e5) ** 0.19)
    state["specific_humidity"].values[:] = 0.012 * (p / 1.0e5) ** 3
    state["surface_temperature"].values[:] = 288.0 + np.linspace(-4.0, 4.0, NX).reshape(state["surface_temperature"].values.shape)
    cld = (p > 4.0e4) & (p < 8.5e4)
    state["cloud_area_fraction_in_atmosphere_layer"].values[:] = np.where(cld, 0.4, 0.0)
    state["mass_content_of_cloud_liquid_water_in_atmosphere_layer"].values[:] = np.where(cld, 0.03, 0.0)
    state["time"] = START
    return state


def warm(state, i):
    """The test's own change of the surface between steps: uniform in step, a ramp by column (some columns do not move)."""
    ts = state["surface_temperature"].values
    ramp = np.linspace(0.0, 1.0, NX).reshape(ts.shape)
    ramp[..., ::5] = 0.0
    ts += WARMING[i] * ramp


def heatfac(lw):
    k = physical_constants()
    return k["grav"] * k["secdy"] / (lw._Cpd * 1.e2)


def run_host(options, seed=5):
    """Four wrapper calls on a host state (update every three steps), checked against the component's own output and the numpy
    statement -> the outputs by call."""
    spy = Spy(calculate_change_up_flux=True, allow_synthetic_tables=True, **options)
    reference = climt_amd.RRTMGLongwave(calculate_change_up_flux=True, allow_synthetic_tables=True, **options)
    clear = options.get("clear_sky_diagnostics", True)
    state = make_state(spy)
    wrapper = climt_amd.IntermittentLongwave(spy, UPDATE)
    outputs, kept = [], None
    for i in range(4):
        state["time"] = START + i * STEP
        warm(state, i)
        if i % 3 == 0:
            np.random.seed(seed + i)
        tendencies, diagnostics = wrapper(state, STEP)
        assert spy.calls == 1 + i // 3, (i, spy.calls)      # the wrapped component ran at steps 1 and 4 only
        assert (len(diagnostics) == 6) == clear and len(diagnostics) in (3, 6)
        assert np.shares_memory(tendencies["air_temperature"].values, diagnostics["air_temperature_tendency_from_longwave"].values)      # one array
        if i % 3 == 0:      # an update: the component's own bits, names, dims and attrs
            np.random.seed(seed + i)
            want_t, want_d = reference(state)
            assert set(diagnostics) == set(want_d) and set(tendencies) == set(want_t)
            for k, w in list(want_d.items()) + list(want_t.items()):
                g = diagnostics[k] if k in diagnostics else tendencies[k]
                assert tuple(g.dims) == tuple(w.dims) and g.attrs["units"] == w.attrs["units"], k
                assert X.same_bits(np.asarray(g.values), np.asarray(w.values)), (i, k)
            shape2 = lambda a: np.asarray(a.values, dtype=np.float64).reshape(a.values.shape[0], -1)
            plev, scale = reference._interface_pressure_of_call
            kept = dict(tsfc_call=state["surface_temperature"].values.reshape(-1).copy(), plev=np.array(plev, dtype=np.float64).reshape(NLAY + 1, -1), scale=scale,
                        uflx=shape2(want_d["upwelling_longwave_flux_in_air"]), dflx=shape2(want_d["downwelling_longwave_flux_in_air"]),
                        duflx_dt=np.array(reference.change_in_upward_flux_with_surface_temperature))
            if clear:
                kept.update(uflxc=shape2(want_d["upwelling_longwave_flux_in_air_assuming_clear_sky"]), dflxc=shape2(want_d["downwelling_longwave_flux_in_air_assuming_clear_sky"]),
                            duflxc_dt=np.array(reference.change_in_clear_sky_upward_flux_with_surface_temperature))
        else:      # in between: the numpy statement on the update's kept arrays
            want = X.want(dict(kept, tsfc_now=state["surface_temperature"].values.reshape(-1)), clear, heatfac=heatfac(spy), pressure_scale=kept["scale"])
            names = dict(uflx="upwelling_longwave_flux_in_air", hr="air_temperature_tendency_from_longwave",
                         uflxc="upwelling_longwave_flux_in_air_assuming_clear_sky", hrc="air_temperature_tendency_from_longwave_assuming_clear_sky")
            for k, w in want.items():
                g = np.asarray(diagnostics[names[k]].values)
                assert X.same_bits(g.reshape(w.shape), w), (i, k, float(np.abs(g.reshape(w.shape) - w).max()))
            for k in ("dflx", "dflxc")[:2 if clear else 1]:
                name = "downwelling_longwave_flux_in_air" + ("_assuming_clear_sky" if k == "dflxc" else "")
                assert X.same_bits(np.asarray(diagnostics[name].values).reshape(kept[k].shape), kept[k]), (i, k)
            moved = np.abs(np.asarray(diagnostics["upwelling_longwave_flux_in_air"].values).reshape(kept["uflx"].shape) - kept["uflx"]).max(axis=0)
            assert (moved > 0.5).sum() > 10 and (moved == 0.0).sum() >= 5      # the correction is there, and absent where the surface stood still
        outputs.append({"tendencies": tendencies, "diagnostics": diagnostics})
    return outputs, state


HOST_OPTIONS = {"default": {}, "all_sky_only": dict(clear_sky_diagnostics=False),
                "mcica": dict(mcica=True, random_number_generator="kissvec", cloud_overlap_method="maximum_random")}


@pytest.fixture(scope="module")
def host_runs():
    return {}


@pytest.mark.parametrize("which", list(HOST_OPTIONS))
def test_wrapper_on_a_host_state(host_runs, which):
    host_runs[which] = run_host(HOST_OPTIONS[which])
    outputs = host_runs[which][0]
    if which == "all_sky_only":
        assert not any("clear_sky" in k for k in outputs[0]["diagnostics"])
        if "default" not in host_runs:
            host_runs["default"] = run_host(HOST_OPTIONS["default"])
        for i in range(4):      # the all-sky bits of the default instance
            for k, g in outputs[i]["diagnostics"].items():
                assert X.same_bits(np.asarray(g.values), np.asarray(host_runs["default"][0][i]["diagnostics"][k].values)), (i, k)


@pytest.mark.parametrize("which", list(HOST_OPTIONS))
def test_wrapper_on_a_device_state_gives_the_host_path_bits(host_runs, which):
    if which not in host_runs:
        host_runs[which] = run_host(HOST_OPTIONS[which])
    host, _ = host_runs[which]
    lw = climt_amd.RRTMGLongwave(calculate_change_up_flux=True, allow_synthetic_tables=True, **HOST_OPTIONS[which])
    wrapper = climt_amd.IntermittentLongwave(lw, UPDATE)
    state = make_state(lw)
    ds = climt_amd.DeviceState.from_host(state, [wrapper])
    try:
        last = None
        for i in range(4):
            ds["time"] = START + i * STEP
            warm(state, i)      # the test changes the surface on the host and puts it into the state
            ds.put_host("surface_temperature", state["surface_temperature"], lw.input_properties["surface_temperature"])
            own = ds["surface_temperature"]
            before = own.buf.download()
            if i % 3 == 0:
                np.random.seed(5 + i)
            tendencies, diagnostics = wrapper(ds, STEP)
            assert getattr(ds, "_lw_inflight", False)      # consumers join the longwave's stream
            pool = {id(q) for q in wrapper._pool.values()}
            assert all(id(q) in pool for q in list(tendencies.values()) + list(diagnostics.values()))
            assert tendencies["air_temperature"] is diagnostics["air_temperature_tendency_from_longwave"]
            adjusted = {diagnostics[k].ptr for k in diagnostics if "downwelling" not in k}
            if last is not None:      # two alternating sets: the last step's arrays are still intact
                assert adjusted.isdisjoint(last)
            last = adjusted
            ds.ctx.synchronize()
            assert ds["surface_temperature"] is own and X.same_bits(own.buf.download(), before)      # the state's own buffer: unchanged
            assert set(diagnostics) == set(host[i]["diagnostics"])
            for k, q in diagnostics.items():
                w = np.asarray(host[i]["diagnostics"][k].values)
                assert X.same_bits(q.buf.download().reshape(w.shape), w), (i, k)
    finally:
        ds.close()


# ---- 6. stream ordering ---------------------------------------------------------------------------------------------------------------
def test_deferred_flux_call_and_adjustment_need_no_host_synchronise(gpu_ctx):
    """Deferred context: the flux call (device pointers, idrv = 1) and the adjustment are enqueued back to back on the longwave's
    stream, then ONE synchronize: the bits of the non-deferred sequence."""
    c, mcica = X.flux_state("mcica_L60")
    nlay, ncol = c["play"].shape
    tsfc_now = c["tsfc"] + X.surface_change()

    def sequence(deferred):
        prev = gpu_ctx.set_deferred(deferred)
        try:
            inp = {k: _hip.DeviceArray.from_host(v) for k, v in c.items() if isinstance(v, np.ndarray) and k in _LW_INPUTS}
            flags = {k: v for k, v in c.items() if not isinstance(v, np.ndarray)}
            out = {k: _hip.DeviceArray((nlay + (0 if k in ("hr", "hrc") else 1), ncol)) for k in ("uflx", "dflx", "hr", "uflxc", "dflxc", "hrc", "duflx_dt", "duflxc_dt")}
            adj = {k: _hip.DeviceArray((nlay + (0 if k in ("hr", "hrc") else 1), ncol)) for k in OUT}
            now = _hip.DeviceArray.from_host(tsfc_now)
            gpu_ctx.lw_fluxes(dict(flags, ncol=ncol, nlay=nlay, **{k: v.ptr for k, v in inp.items()}), mcica=mcica, out={k: v.ptr for k, v in out.items()}, memspace=1)
            gpu_ctx.lw_adjust_surface(ncol, nlay, inp["tsfc"], now, inp["plev"], (out["uflx"], out["dflx"], out["duflx_dt"], adj["uflx"], adj["hr"]),
                                      (out["uflxc"], out["dflxc"], out["duflxc_dt"], adj["uflxc"], adj["hrc"]))
            gpu_ctx.synchronize()
            return {k: v.download() for k, v in adj.items()}, {k: v.download() for k, v in out.items()}
        finally:
            gpu_ctx.set_deferred(prev)

    plain, plain_call = sequence(False)
    deferred, deferred_call = sequence(True)
    assert float(np.abs(plain["uflx"] - plain_call["uflx"]).max()) > 1.0
    for k in OUT:
        assert X.same_bits(deferred[k], plain[k]), k
    for k in plain_call:
        assert X.same_bits(deferred_call[k], plain_call[k]), k
    want = X.want(dict(tsfc_call=c["tsfc"], tsfc_now=tsfc_now, plev=c["plev"], **{k: plain_call[k] for k in ("uflx", "dflx", "duflx_dt", "uflxc", "dflxc", "duflxc_dt")}))
    for k in OUT:
        assert X.same_bits(plain[k], want[k]), k


_LW_INPUTS = ("play", "plev", "tlay", "tlev", "tsfc", "h2o", "o3", "co2", "ch4", "n2o", "o2", "cfc11", "cfc12", "cfc22", "ccl4", "emis", "cldfr", "cicewp", "cliqwp", "reice", "reliq")
