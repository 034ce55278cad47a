"""The simple physics package on the GPU: simple_physics_kernel (rrtmg_hip_simple_physics) against the numpy statement
(tests/simple_physics_cases.py) on every case, switch set and shape; what must hold bit for bit -- NULL diagnostics, in place,
host against device pointers, a block of columns alone, columns of different branches in one wave, all switches off, the
component on a DeviceState (pressures resident in Pa and in mbar); the flux diagnostics as resident inputs of SlabSurface; and
examples/radiative_convective.py with SimplePhysics in both modes.

Values against the statement: the tolerances stored in tests/golden/simple_physics_<case>_<switches>.npz, measured by the maker
on the reference's Fortran (16 x its largest deviation under +-1 ulp of every input, at least 1e-13), on the scales of
X.deviations.  Every case has a decision margin >= 1e-9, so no decision can differ; what remains is the device's exp, log, pow
and sqrt against libm's.  The largest deviations are printed by the first test (docs/EXPERIMENTS.md S has the figures)."""
import datetime
import importlib.util
import os

import numpy as np
import pytest

import climt_amd
from climt_amd import _hip
from climt_amd._sympl_compat import DataArray
from helpers import ROOT, maxdiff

import simple_physics_cases as X

pytestmark = pytest.mark.gpu

FLUXES = ("surface_upward_sensible_heat_flux", "surface_upward_latent_heat_flux")
RAIN = "stratiform_precipitation_rate"
DIAG = ("precl", "sh_out", "lh_out")
NAMES = ("air_temperature", "specific_humidity", "eastward_wind", "northward_wind")
COLUMN_INPUTS = dict(ts="ts", qsurf="qsurf", lat="lat")


@pytest.fixture(scope="module")
def ctx():
    from climt_amd.rrtmg.common import make_context
    return make_context(0)


def _switches(c, clamp=0):
    return dict(zip(X.SWITCH_NAMES + X.FLAGS, tuple(c["switches"]) + tuple(c["flags"])), clamp_latent_heat_flux=clamp)


def _result(t, q, u, v, d):
    got = dict(t_new=t, q_new=q, u_new=u, v_new=v)
    if d:
        got.update({k: d.get(n) for k, n in zip(X.DIAGNOSTICS, DIAG)})
    return got


def host_call(ctx, c, clamp=0, **kw):
    return _result(*ctx.simple_physics(c["t"], c["q"], c["u"], c["v"], c["p"], c["p_int"], c["ps"], X.DT, X.CONSTANTS, _switches(c, clamp),
                                       ts=c["ts"], qsurf=c["qsurf"], lat=c["lat"], **kw))


def device_call(ctx, c, in_place=False):
    """Device pointers -> the results on the host."""
    nlay, ncol = c["t"].shape
    d = {k: _hip.DeviceArray.from_host(np.ascontiguousarray(c[k])) for k in X.INPUTS}
    out = [d[k] if in_place else _hip.DeviceArray((nlay, ncol)) for k in "tquv"]
    diag = {n: _hip.DeviceArray((ncol,)) for n in DIAG}
    ctx.simple_physics(d["t"], d["q"], d["u"], d["v"], d["p"], d["p_int"], d["ps"], X.DT, X.CONSTANTS, _switches(c), ts=d["ts"], qsurf=d["qsurf"],
                       lat=d["lat"], t_out=out[0], q_out=out[1], u_out=out[2], v_out=out[3], diagnostics=diag, memspace=1, ncol=ncol, nlay=nlay)
    ctx.synchronize()
    if not in_place:      # the inputs of an out-of-place call are only read
        assert all(X.same_bits(d[k].download(), c[k]) for k in X.INPUTS)
    return _result(*(o.download() for o in out), {n: x.download() for n, x in diag.items()})


def same(a, b):
    return all(X.same_bits(a[k], b[k]) for k in a)


@pytest.mark.parametrize("sw", list(X.SWITCHES))
@pytest.mark.parametrize("name", X.CASES)
def test_kernel_equals_the_statement_on_every_shape(ctx, name, sw):
    worst, tol = {}, X.tolerances(name, sw)
    for nlay in X.NLAYS:
        for ncol in X.NCOLS:
            c = X.case(name, nlay, ncol, sw)
            got = host_call(ctx, c)
            dev = X.deviations(got, c)
            assert len(dev) == 7
            for k, v in dev.items():
                worst[k] = max(worst.get(k, 0.0), v)
    print("simple_physics_kernel, %s, %s: largest deviation from the statement (tolerance) %s" % (
        name, sw, ", ".join("%s %.2e (%.1e)" % (k, v, tol[k]) for k, v in sorted(worst.items()))))
    for k, v in worst.items():
        assert v <= tol[k], (name, sw, k, v, tol[k])


def test_every_diagnostic_pointer_may_be_null(ctx):
    for name, sw, nlay, ncol in (("varied", "all", 30, 65), ("raining", "lsc", 2, 130), ("dew", "surface", 61, 1), ("gale", "surface_pbl", 1, 64)):
        c = X.case(name, nlay, ncol, sw)
        full, bare = host_call(ctx, c), host_call(ctx, c, diagnostics=None)
        assert set(bare) == set(X.PROFILES) and all(X.same_bits(bare[k], full[k]) for k in bare)
        some = host_call(ctx, c, diagnostics=dict(precl=np.empty(ncol), lh_out=np.empty(ncol)))
        assert X.same_bits(some["precl"], full["precl"]) and X.same_bits(some["lh"], full["lh"]) and some["sh"] is None
        assert same({k: some[k] for k in X.PROFILES}, bare)


def test_each_optional_array_left_out_leaves_the_others_their_bits(ctx):
    """Host pointers, 65 columns (two tiles, one live lane in the second) by 2 layers, all three processes: the staging buffer of
    a call is laid out over the arrays that are given, so every diagnostic, and every one of ts, qsurf and lat that the switches
    leave unread, is in turn left out of an otherwise full call.  What is still asked for has the bits of the full call, in the
    caller's own arrays, and the inputs keep theirs."""
    c = X.case("varied", 2, 65, "all")
    before = {k: np.array(c[k]) for k in X.INPUTS}
    s = _switches(c)
    read = dict(ts=s["use_ts_ext"] == 1, qsurf=s["use_qsurf_ext"] == 1, lat=s["use_ts_ext"] != 1 and s["test"] == 1)
    assert s["do_surf_flux"] == 1 and not all(read.values())
    full = host_call(ctx, c)
    for left_out in DIAG + tuple(n for n in read if not read[n]):
        diag = {n: np.full(65, -7.0) for n in DIAG if n != left_out}
        columns = {n: c[n] for n in read if n != left_out}
        got = _result(*ctx.simple_physics(c["t"], c["q"], c["u"], c["v"], c["p"], c["p_int"], c["ps"], X.DT, X.CONSTANTS, s, diagnostics=diag, **columns))
        for key, n in zip(X.DIAGNOSTICS, DIAG):
            assert got[key] is (None if n == left_out else diag[n])
        assert all(X.same_bits(got[k], full[k]) for k in got if got[k] is not None), left_out
        assert all(X.same_bits(c[k], before[k]) for k in X.INPUTS), left_out


@pytest.mark.parametrize("sw", list(X.SWITCHES))
def test_in_place_host_and_device_pointers_agree_bit_for_bit(ctx, sw):
    for name, nlay, ncol in (("varied", 1, 1), ("raining", 30, 130), ("varied", 61, 65), ("gale", 2, 64)):
        c = X.case(name, nlay, ncol, sw)
        want = host_call(ctx, c)
        # host arrays, in place
        io = {k: np.array(c[k]) for k in "tquv"}
        got = host_call(ctx, dict(c, **io), t_out=io["t"], q_out=io["q"], u_out=io["u"], v_out=io["v"])
        assert got["t_new"] is io["t"] and same(got, want)
        # device pointers, out of place and in place
        for in_place in (False, True):
            assert same(device_call(ctx, c, in_place), want), (name, nlay, ncol, in_place)


def test_a_block_of_columns_alone_equals_the_block_inside_the_whole(ctx):
    for name, sw in (("varied", "all"), ("raining", "lsc"), ("gale", "surface_pbl")):
        c = X.case(name, 30, 130, sw)
        whole = host_call(ctx, c)
        for a, b in ((1, 2), (37, 101), (63, 130), (5, 69)):
            part = dict(c, **{k: np.ascontiguousarray(c[k][..., a:b]) for k in X.INPUTS})
            got = host_call(ctx, part)
            assert all(X.same_bits(got[k], whole[k][..., a:b]) for k in got), (name, sw, a, b)


def test_columns_of_different_branches_in_one_wave_do_not_disturb_each_other(ctx):
    # a dry, calm column among varied ones
    for nlay, ncol in ((30, 65), (61, 130)):
        c, d = X.case("varied", nlay, ncol, "all"), X.case("dry_calm", nlay, ncol, "all")
        mixed = dict(c, **{k: np.array(c[k]) for k in X.INPUTS})
        for k in X.INPUTS:
            mixed[k][..., 17] = d[k][..., 17]
        got = host_call(ctx, mixed)
        assert all(X.same_bits(got[k + "_new"][:, 17], mixed[k][:, 17]) for k in "quv")
        assert got["precl"][17] == 0 and got["sh"][17] == 0 and got["lh"][17] == 0
        alone = host_call(ctx, c)
        others = np.arange(ncol) != 17
        assert all(X.same_bits(got[k][..., others], alone[k][..., others]) for k in got)
        assert not X.same_bits(got["u_new"][:, 16], mixed["u"][:, 16])
    # gale and breeze mixed in one launch (the gale case: even columns) against their separate launches
    for sw in ("surface", "all"):
        g, b = X.case("gale", 30, 130, sw), X.case("breeze", 30, 130, sw)
        even, odd = np.arange(130) % 2 == 0, np.arange(130) % 2 == 1
        assert all(X.same_bits(g[k][..., odd], b[k][..., odd]) for k in X.INPUTS)      # the odd columns ARE the breeze's
        mixed, breeze = host_call(ctx, g), host_call(ctx, b)
        gale = host_call(ctx, dict(g, **{k: np.ascontiguousarray(g[k][..., even]) for k in X.INPUTS}))
        assert all(X.same_bits(mixed[k][..., odd], breeze[k][..., odd]) and X.same_bits(mixed[k][..., even], gale[k]) for k in mixed)


def test_all_switches_off_returns_the_inputs_bits(ctx):
    for name, nlay, ncol in (("varied", 30, 65), ("raining", 61, 130), ("dry_calm", 1, 1)):
        c = X.case(name, nlay, ncol, "none")
        got = host_call(ctx, c)
        assert all(X.same_bits(got[k + "_new"], c[k]) for k in "tquv")
        zero = np.zeros(ncol)
        assert X.same_bits(got["precl"], zero) and X.same_bits(got["sh"], zero) and X.same_bits(got["lh"], zero)      # exact +0.0
    c = X.case("raining", 30, 65, "lsc")      # surface fluxes off: the two flux outputs are exact +0.0
    got = host_call(ctx, c)
    assert X.same_bits(got["sh"], np.zeros(65)) and X.same_bits(got["lh"], np.zeros(65)) and got["precl"].any()
    c = X.case("dew", 30, 65, "surface")      # the clamp: the diagnostic alone
    raw, clamped = host_call(ctx, c), host_call(ctx, c, clamp=1)
    assert (raw["lh"] < 0).all() and X.same_bits(clamped["lh"], np.zeros(65)) and same({k: clamped[k] for k in X.PROFILES}, {k: raw[k] for k in X.PROFILES})


def _state(c, ny, nx, pressure_units="Pa"):
    """[levels][lat][lon]: resident as the host path hands it to the library; the pressures in `pressure_units`."""
    f = {"Pa": 1.0, "mbar": 100.0}[pressure_units]
    lev = lambda a, dim, units, div=1.0: DataArray(a.reshape(a.shape[0], ny, nx) / div, dims=(dim, "lat", "lon"), attrs={"units": units})
    col = lambda a, units, div=1.0: DataArray(a.reshape(ny, nx) / div, dims=("lat", "lon"), attrs={"units": units})
    return {"air_temperature": lev(c["t"], "mid_levels", "degK"), "specific_humidity": lev(c["q"], "mid_levels", "kg/kg"),
            "eastward_wind": lev(c["u"], "mid_levels", "m s^-1"), "northward_wind": lev(c["v"], "mid_levels", "m s^-1"),
            "air_pressure": lev(c["p"], "mid_levels", pressure_units, f),
            "air_pressure_on_interface_levels": lev(c["p_int"], "interface_levels", pressure_units, f),
            "surface_air_pressure": col(c["ps"], pressure_units, f), "surface_temperature": col(c["ts"], "degK"),
            "surface_specific_humidity": col(c["qsurf"], "kg/kg"), "latitude": col(c["lat"], "degrees_north"),
            "time": datetime.datetime(2000, 1, 1)}


class ResidentPressureUnits:
    """A component listed first in DeviceState.from_host so that the pressures become resident in its units."""

    def __init__(self, units):
        self.input_properties = {"air_pressure": {"dims": ["mid_levels", "*"], "units": units},
                                 "air_pressure_on_interface_levels": {"dims": ["interface_levels", "*"], "units": units},
                                 "surface_air_pressure": {"dims": ["*"], "units": units}}


@pytest.mark.parametrize("units", ["Pa", "mbar"])
@pytest.mark.parametrize("name", ["varied", "internal_sst"])
def test_component_on_a_device_state_equals_the_host_state_bit_for_bit(ctx, name, units):
    c = X.case(name, 30, 65, "all")
    use_ts_ext, use_qsurf_ext, test = c["flags"]
    sp = climt_amd.SimplePhysics(simulate_cyclone=bool(test), use_external_surface_temperature=bool(use_ts_ext),
                                 use_external_surface_specific_humidity=bool(use_qsurf_ext), context=ctx)
    dt = datetime.timedelta(seconds=X.DT)
    state = _state(c, 5, 13, units)
    diagnostics, new_state = sp(state, dt)
    if units == "Pa":
        got = {key: new_state[n].values.reshape(30, 65) for n, key in zip(NAMES, X.PROFILES)}
        got.update(precl=diagnostics[RAIN].values.ravel(), sh=diagnostics[FLUXES[0]].values.ravel())
        assert X.within(X.deviations(got, c), X.tolerances(name, "all"))
        lh = diagnostics[FLUXES[1]].values.ravel()
        assert (lh >= 0).all() and np.allclose(lh, np.maximum(c["lh"], 0.0), rtol=1e-10, atol=0)
    with climt_amd.DeviceState.from_host(state, [ResidentPressureUnits(units), sp], context=ctx) as ds:
        assert ds["air_pressure"].units == units and ds["surface_air_pressure"].units == units
        before = {n: ds[n] for n in NAMES}
        diag_d, ds2 = sp(ds, dt)
        assert ds2 is ds and set(diag_d) == set(diagnostics)
        assert all(isinstance(x, climt_amd.DeviceQuantity) and tuple(x.dims) == ("*",) for x in diag_d.values())
        assert all(ds[n] is not before[n] and isinstance(ds[n], climt_amd.DeviceQuantity) for n in NAMES)      # rebound to work buffers
        ds.update(diag_d)
        for n in NAMES + tuple(diag_d):
            got, want = ds.download(n), (new_state.get(n) if n in new_state else diagnostics[n])
            assert got.dims == want.dims and got.attrs["units"] == want.attrs["units"], n
            assert X.same_bits(got.values, want.values), n
        first = {n: ds[n] for n in NAMES}
        kept = {n: ds[n].buf.download() for n in NAMES}
        assert all(X.same_bits(before[n].buf.download().reshape(30, 65), c[k]) for n, k in zip(NAMES, "tquv"))      # the previous arrays stay
        # the next step: the other set of buffers, the first step's arrays intact
        ds.step_count += 1
        sp(ds, dt)
        assert all(ds[n] is not first[n] and ds[n].ptr != first[n].ptr for n in NAMES)
        ds.ctx.synchronize()
        assert all(X.same_bits(first[n].buf.download(), kept[n]) for n in NAMES)
        host2 = dict(state)
        host2.update(new_state)
        _, new_state2 = sp(host2, dt)
        for n in NAMES:
            assert X.same_bits(ds.download(n).values, new_state2[n].values), n


def test_device_call_refuses_a_state_of_another_shape(ctx):
    c = X.case("varied", 30, 65, "all")
    sp = climt_amd.SimplePhysics(context=ctx)
    with climt_amd.DeviceState.from_host(_state(c, 5, 13), [sp], context=ctx) as ds:
        q = ds["air_pressure_on_interface_levels"]
        ds["air_pressure_on_interface_levels"] = climt_amd.DeviceQuantity(q.buf, (30, 65), q.dims, q.units)
        with pytest.raises(ValueError, match="do not belong to one grid"):
            sp(ds, datetime.timedelta(seconds=X.DT))
        ds["air_pressure_on_interface_levels"] = climt_amd.DeviceQuantity(q.buf, q.shape, ("*", "interface_levels"), q.units)
        with pytest.raises(ValueError, match="resident as"):
            sp(ds, datetime.timedelta(seconds=X.DT))


def test_slab_surface_takes_the_resident_flux_diagnostics(ctx):
    """The two flux diagnostics of SimplePhysics, still in HBM, as the inputs of SlabSurface's device call: the slab's tendency
    equals the one of the host path fed with the downloaded fluxes (the tolerance of tests/test_boundary_layer_gpu.py)."""
    c = X.case("breeze", 30, 65, "all")
    sp, slab = climt_amd.SimplePhysics(context=ctx), climt_amd.SlabSurface()
    state = climt_amd.get_default_state([slab], grid_state=climt_amd.get_grid(nx=13, ny=5, nz=30))
    for n, x in _state(c, 5, 13).items():      # the profiles and surface values into the slab's default state
        if n != "time":
            state[n] = x
    for n in ("downwelling_shortwave_flux_in_air", "downwelling_longwave_flux_in_air"):
        state[n].values[...] = 150.0
    dt = datetime.timedelta(seconds=X.DT)
    diagnostics, _ = sp(state, dt)
    assert np.abs(diagnostics[FLUXES[0]].values).min() > 1.0
    tend_without, _ = slab(state)      # (the default state's fluxes: zero)
    host = dict(state)
    host.update(diagnostics)
    tend_h, _ = slab(host)
    want = np.asarray(tend_h["surface_temperature"].values, dtype=np.float64).reshape(-1)
    assert np.abs(want - np.asarray(tend_without["surface_temperature"].values).reshape(-1)).min() > 0.0
    with climt_amd.DeviceState.from_host(state, [slab, sp], context=ctx) as ds:
        diag_d, _ = sp(ds, dt)
        ds.update(diag_d)
        assert ds[FLUXES[0]] is diag_d[FLUXES[0]] and ds[FLUXES[0]].dims == ("*",) and ds[FLUXES[0]].units == "W m^-2"
        tend_d, _ = slab(ds)
        ds["tend"] = tend_d["surface_temperature"]
        got = ds.download("tend").values.reshape(-1)
    assert maxdiff(got, want) <= 1e-12 * float(np.abs(want).max())


def test_radiative_convective_example_with_simple_physics_in_both_modes():
    """Three steps of examples/radiative_convective.py with simple_physics=True on a host state and on a DeviceState: the state of
    the two modes to the tolerance of the example's own test (tests/test_dry_adjustment_gpu.py); it rains and the surface
    evaporates from step 0; the flag is exclusive with the boundary layer's; the run without the flag is unchanged."""
    spec = importlib.util.spec_from_file_location("radiative_convective", os.path.join(ROOT, "examples", "radiative_convective.py"))
    ex = importlib.util.module_from_spec(spec); spec.loader.exec_module(ex)
    first_h, end_h = ex.run(3, device_resident=False, simple_physics=True)
    first_d, end_d = ex.run(3, device_resident=True, simple_physics=True)
    for first in (first_h, first_d):
        assert "upwelling_longwave_flux_in_air" in first and RAIN in first
        assert float(first[RAIN].values.min()) > 0.0 and float(first[FLUXES[1]].values.min()) > 0.0
    for name in (RAIN,) + FLUXES:
        assert maxdiff(first_h[name].values.ravel(), first_d[name].values.ravel()) <= 1e-9 * max(1.0, float(np.abs(first_h[name].values).max()))
    for name in ("air_temperature", "specific_humidity", "surface_temperature", "eastward_wind", "northward_wind", RAIN) + FLUXES:
        h, d = end_h[name], end_d[name]
        g = np.transpose(d.values, [d.dims.index(x) for x in h.dims])
        assert np.all(np.isfinite(h.values)) and maxdiff(h.values, g) <= 1e-9, (name, maxdiff(h.values, g))
    assert float(end_h["eastward_wind"].values.ravel()[0]) < 5.0      # drag on the lowest layer
    with pytest.raises(ValueError, match="exclusive"):
        ex.run(1, boundary_layer=True, simple_physics=True)
    # the run without the flag is another run: there the wind stays at rest and nothing rains
    _, plain = ex.run(3, device_resident=False)
    assert RAIN not in plain and ("eastward_wind" not in plain or not np.any(plain["eastward_wind"].values))
