"""The shortwave between radiation calls on the GPU (run with -m gpu on an MI355X): rrtmg_hip_mean_coszen against the numpy
statement of tests/intermittent_cases.py, its additivity over sub-intervals and its short-interval limit, rrtmg_hip_scale_columns
bit for bit, and IntermittentShortwave on a host state and a DeviceState."""
import ctypes as C
import datetime

import numpy as np
import pytest

import climt_amd
from climt_amd import _hip, _lib
from climt_amd.instellation import host_columns, interval_centuries

import intermittent_cases as X

pytestmark = pytest.mark.gpu

NCOL, NLAY = 130, 6
UPDATE, STEP = datetime.timedelta(hours=3), datetime.timedelta(minutes=30)
START = datetime.datetime(2000, 3, 20, 4, 40)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


# ---- 1. the kernel against the numpy statement -------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(X.INTERVALS))
def test_mean_coszen_equals_the_numpy_statement(gpu_ctx, name):
    assert gpu_ctx.has_intermittent
    t0, t1 = X.interval_centuries(name)
    zen, ins = np.empty(X.NCOL), np.empty(X.NCOL)
    mean, frac = gpu_ctx.mean_coszen(X.LAT, X.LON, t0, t1, out_zenith=zen, out_insolation=ins)
    X.check_mean_coszen(mean, frac, X.WANT[name], "memspace 0, %s:" % name)
    assert np.array_equal(bits(ins), bits(mean * frac))
    assert np.all(zen[mean == 0.0] == 0.5 * np.pi) and np.abs(np.cos(zen) - mean)[mean > 0.0].max() <= 1e-15
    # device pointers: the same bits
    dev = {k: _hip.DeviceArray.from_host(v) for k, v in (("lat", X.LAT), ("lon", X.LON))}
    out = {k: _hip.DeviceArray((X.NCOL,)) for k in ("mean", "frac", "zen", "ins")}
    gpu_ctx.mean_coszen(dev["lat"].ptr, dev["lon"].ptr, t0, t1, out_mean=out["mean"].ptr, out_fraction=out["frac"].ptr, memspace=1, ncol=X.NCOL,
                        out_zenith=out["zen"].ptr, out_insolation=out["ins"].ptr)
    gpu_ctx.synchronize()
    for k, v in (("mean", mean), ("frac", frac), ("zen", zen), ("ins", ins)):
        assert np.array_equal(bits(out[k].download()), bits(v)), k
    # the two optional outputs left out
    m2, f2 = gpu_ctx.mean_coszen(X.LAT, X.LON, t0, t1)
    assert np.array_equal(bits(m2), bits(mean)) and np.array_equal(bits(f2), bits(frac))


def test_intervals_that_are_refused(gpu_ctx):
    t0, day = X.centuries(X.T0), 1.0 / 36525.0
    for t1 in (t0, t0 - 0.1 * day, t0 + 0.5 * day * 1.001, t0 + day):
        with pytest.raises(_lib.RRTMGError) as e:
            gpu_ctx.mean_coszen(X.LAT, X.LON, t0, t1)
        assert e.value.code == 4
    with pytest.raises(_lib.RRTMGError) as e:
        gpu_ctx.mean_coszen(X.LAT, X.LON, 0.0, 0.0, sun=(0.4, 0.9, 1.0, 7.0))
    assert e.value.code == 4
    mean, _ = gpu_ctx.mean_coszen(X.LAT, X.LON, t0, X.centuries(X.T0 + datetime.timedelta(hours=12)))      # the context stays usable
    assert mean.max() > 0.5


# ---- 2. additivity: the energy statement ---------------------------------------------------------------------------------------------
def test_six_steps_add_up_to_the_interval(gpu_ctx):
    """sum mu_i f_i D_i over six 30-minute steps = mu f D of the 3 hours, per column, to 1e-12 D.  One fixed declination for all
    seven calls (rrtmg_hip_mean_coszen_sun): taken at each interval's own midpoint it would drift by up to 0.4 degrees / day."""
    sin_dec, cos_dec, g0, D = X.interval_sun(*X.interval_centuries("3h"))
    whole = np.empty(X.NCOL)
    gpu_ctx.mean_coszen(X.LAT, X.LON, 0.0, 0.0, out_insolation=whole, sun=(sin_dec, cos_dec, g0, D))
    total, part = np.zeros(X.NCOL), np.empty(X.NCOL)
    for i in range(6):
        gpu_ctx.mean_coszen(X.LAT, X.LON, 0.0, 0.0, out_insolation=part, sun=(sin_dec, cos_dec, g0 + i * (D / 6.0), D / 6.0))
        total += part * (D / 6.0)
    worst = float(np.abs(total - whole * D).max())
    print("additivity: max |sum - whole| = %.3e (bound %.3e)" % (worst, 1e-12 * D))
    assert whole.max() > 0.5 and worst <= 1e-12 * D


# ---- 3. the short-interval limit -----------------------------------------------------------------------------------------------------
def test_sixty_seconds_is_the_instantaneous_zenith_angle(gpu_ctx):
    """|d cos(zenith) / dt| <= omega = 7.3e-5 rad/s (the hour angle's rate; the declination's is four orders below), so the mean
    over 60 s lies within omega * 60 s of the value at t0 -- on columns that are in daylight throughout."""
    t0, t1 = X.interval_centuries("60s")
    mean, frac = gpu_ctx.mean_coszen(X.LAT, X.LON, t0, t1)
    instant = np.cos(gpu_ctx.zenith_angle(X.LAT, X.LON, t0))
    day = (frac == 1.0) & (instant > 0.05)
    assert day.sum() > 60
    worst = float(np.abs(mean - instant)[day].max())
    print("60 s: max |mean - instant| = %.3e (bound %.3e)" % (worst, 7.3e-5 * 60.0))
    assert worst <= 7.3e-5 * 60.0


# ---- 4. the rescale ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("in_place", [False, True], ids=["out_of_place", "in_place"])
def test_scale_columns_equals_numpy_bit_for_bit(gpu_ctx, in_place):
    num, den, arrays = X.scale_case(NCOL, NLAY)
    assert [a.shape[0] for a in arrays] == [7, 7, 7, 7, 6, 6]
    dnum, dden = _hip.DeviceArray.from_host(num), _hip.DeviceArray.from_host(den)
    src = [_hip.DeviceArray.from_host(a) for a in arrays]
    dst = src if in_place else [_hip.DeviceArray.from_host(np.full(a.shape, np.nan)) for a in arrays]
    gpu_ctx.scale_columns(dnum, dden, [(s, d, a.shape[0]) for s, d, a in zip(src, dst, arrays)])      # ONE call, one launch
    gpu_ctx.synchronize()
    zero = X.scale_factor(num, den) == 0.0
    assert zero.sum() >= 6
    for s, d, a in zip(src, dst, arrays):
        got, want = d.download(), X.scale_columns(a, num, den)
        both_nan = np.isnan(got) & np.isnan(want)
        assert not both_nan[:, zero].any() and np.array_equal(bits(got)[~both_nan], bits(want)[~both_nan])
        assert np.all(got[:, zero] == 0.0) and not np.signbit(got[:, zero]).any()
        if not in_place:
            back = s.download()
            assert np.array_equal(bits(back)[~np.isnan(a)], bits(a)[~np.isnan(a)])      # the source is only read
    # 17 entries in one call
    table = (_lib.ScaleEntry * 17)()
    for e in table:
        e.src, e.dst, e.rows = src[0].ptr, dst[0].ptr, 7
    assert gpu_ctx.lib.rrtmg_hip_scale_columns(gpu_ctx.h, NCOL, C.c_void_p(dnum.ptr), C.c_void_p(dden.ptr), 17, table) == 4
    assert gpu_ctx.lib.rrtmg_hip_scale_columns(gpu_ctx.h, NCOL, C.c_void_p(dnum.ptr), C.c_void_p(dden.ptr), 0, table) == 4


# ---- 5 - 7. the wrapper --------------------------------------------------------------------------------------------------------------
class Spy(climt_amd.RRTMGShortwave):
    calls = 0

    def array_call(self, state):
        self.calls += 1
        return super().array_call(state)


def make_state(sw, cloud):
    sun = climt_amd.Instellation()
    state = climt_amd.get_default_state([sun, sw], grid_state=climt_amd.get_grid(nx=NCOL, ny=1, nz=NLAY))
    p = state["air_pressure"].values
    state["air_temperature"].values[:] = np.maximum(200.0, 290.0 * (p / 1.0e5) ** 0.19)
    state["specific_humidity"].values[:] = 0.012 * (p / 1.0e5) ** 3
    if cloud:
        cld = (p > 4.0e4) & (p < 8.5e4)
        state["cloud_area_fraction_in_atmosphere_layer"].values[:] = np.where(cld, 0.4, 0.0)
        state["mass_content_of_cloud_liquid_water_in_atmosphere_layer"].values[:] = np.where(cld, 0.03, 0.0)
    state["time"] = START
    return sun, state


def expected(ctx, reference, sun, state, update_time, now, seed):
    """What the wrapper must return at `now`: the plain component's output for the update's interval-mean zenith angle, scaled
    in numpy by the step's factor -> ({group: {name: array}}, the columns without sun in the update interval)."""
    at_update = dict(state, time=update_time)
    at_update["zenith_angle"] = sun.interval_mean(at_update, UPDATE)["zenith_angle"]
    np.random.seed(seed)
    tendencies, diagnostics = reference(at_update)
    lat, lon = host_columns(state)
    mu_rad, _ = ctx.mean_coszen(lat, lon, *interval_centuries(update_time, UPDATE))
    ins = np.empty(lat.shape)
    ctx.mean_coszen(lat, lon, *interval_centuries(now, STEP), out_insolation=ins)
    scaled = lambda group: {k: X.scale_columns(np.asarray(v.values).reshape(-1, NCOL), ins, mu_rad).reshape(np.shape(v.values)) for k, v in group.items()}
    return {"tendencies": scaled(tendencies), "diagnostics": scaled(diagnostics)}, mu_rad == 0.0, X.scale_factor(ins, mu_rad)


def run_host(options, cloud, ncalls, seed=11):
    """`ncalls` wrapper calls on a host state, each compared bit for bit with `expected` -> the outputs, by call."""
    spy, reference = Spy(**options), climt_amd.RRTMGShortwave(**options)
    sun, state = make_state(spy, cloud)
    wrapper = climt_amd.IntermittentShortwave(spy, sun, UPDATE)
    outputs, update_time, seen = [], None, 0
    for i in range(ncalls):
        now = START + i * STEP
        state["time"] = now
        np.random.seed(seed + (i // 6))
        tendencies, diagnostics = wrapper(state, STEP)
        if i % 6 == 0:
            update_time, seen = now, seen + 1
        assert spy.calls == seen, (i, spy.calls)      # the wrapped component ran on calls 1 and 7 only
        want, dark, s = expected(spy._ctx, reference, sun, state, update_time, now, seed + (i // 6))
        assert dark.sum() > 10 and (~dark).sum() > 10 and (s > 0.0).sum() > 10
        got = {"tendencies": tendencies, "diagnostics": diagnostics}
        for group in want:
            assert set(got[group]) == set(want[group]) and (group == "tendencies" or len(want[group]) >= 6)
            for name, w in want[group].items():
                g = np.asarray(got[group][name].values)
                assert g.shape == w.shape and not np.isnan(g).any(), (i, name)
                assert np.array_equal(bits(g), bits(w)), (i, name, float(np.abs(g - w).max()))
                assert np.all(g[..., dark.reshape(g.shape[-2:])] == 0.0) and not np.signbit(g[..., dark.reshape(g.shape[-2:])]).any(), (i, name)
        assert float(diagnostics["downwelling_shortwave_flux_in_air"].values.max()) > 100.0 or i % 6 > 3
        outputs.append(got)
    return outputs, state, sun


HOST_OPTIONS = {"default": {}, "skip_pack": dict(skip_night_columns=True, pack_day_columns=True)}


@pytest.fixture(scope="module")
def host_runs():
    return {}


@pytest.mark.parametrize("which", list(HOST_OPTIONS))
def test_wrapper_on_a_host_state(host_runs, which):
    """130 columns on the equator at an equinox dawn -- day, night and both terminators -- update 3 h, step 30 min, seven calls."""
    host_runs[which] = run_host(HOST_OPTIONS[which], False, 7)
    first = host_runs[which][0]
    # the scaled output changes from step to step (the sun moves), and is not the plain component's
    a, b = (np.asarray(first[i]["diagnostics"]["downwelling_shortwave_flux_in_air"].values) for i in (0, 1))
    assert not np.array_equal(a, b)


@pytest.mark.parametrize("which", list(HOST_OPTIONS))
def test_wrapper_on_a_device_state_gives_the_host_path_bits(host_runs, which):
    """The same seven calls on a DeviceState: the host path's bits, and every returned handle lives in the wrapper's own pools
    (nothing is downloaded between the calls: the only copies are this test's)."""
    if which not in host_runs:
        host_runs[which] = run_host(HOST_OPTIONS[which], False, 7)
    host, state, sun = host_runs[which]
    sw = climt_amd.RRTMGShortwave(**HOST_OPTIONS[which])
    wrapper = climt_amd.IntermittentShortwave(sw, sun, UPDATE)
    state = dict(state, time=START)
    ds = climt_amd.DeviceState.from_host(state, [sun, wrapper])
    try:
        handles = []
        for i in range(7):
            ds["time"] = START + i * STEP
            np.random.seed(11 + (i // 6))
            tendencies, diagnostics = wrapper(ds, STEP)
            pool = {id(q) for q in wrapper._pool.values()}
            assert all(id(q) in pool for q in list(tendencies.values()) + list(diagnostics.values()))
            assert not any(q is k for q in diagnostics.values() for k in wrapper._kept[1].values())      # scaled, not the kept ones
            handles.append((tendencies, diagnostics))
            if i:      # two alternating sets: the last step's arrays are still intact
                assert {q.ptr for q in diagnostics.values()}.isdisjoint({q.ptr for q in handles[i - 1][1].values()})
            ds.ctx.synchronize()
            for group, arrays in (("tendencies", tendencies), ("diagnostics", diagnostics)):
                assert set(arrays) == set(host[i][group])
                for name, q in arrays.items():
                    g, w = q.buf.download().reshape(-1, NCOL), np.asarray(host[i][group][name].values).reshape(-1, NCOL)
                    assert np.array_equal(bits(g), bits(w)), (i, name, float(np.abs(g - w).max()))
    finally:
        ds.close()


def test_wrapper_with_mcica_scales_all_six_outputs():
    """McICA, kissvec, cloud in every column: one update and two calls in between; the clear-sky outputs scale like the others."""
    outputs, _, _ = run_host(dict(mcica=True, random_number_generator="kissvec", cloud_overlap_method="maximum_random"), True, 3)
    d = outputs[0]["diagnostics"]
    assert len(d) == 6
    clear, allsky = (np.asarray(d[k].values) for k in ("downwelling_shortwave_flux_in_air_assuming_clear_sky", "downwelling_shortwave_flux_in_air"))
    assert clear[0].max() > 100.0 and np.abs(clear[0] - allsky[0]).max() > 10.0      # the cloud is seen at the surface
