"""The simple boundary layer on the GPU: boundary_layer_kernel (rrtmg_hip_boundary_layer) against the numpy statement
(tests/boundary_layer_cases.py) on every case, mode and shape; what must hold bit for bit -- in place, host against device
pointers, a block of columns alone, a decoupled column without surface exchange, the component on a DeviceState (pressures
resident in Pa and in mbar); the flux diagnostics as resident inputs of SlabSurface; and examples/radiative_convective.py with
the boundary layer in both modes.

Values against the statement: X.TOL = 1e-12 on the scales of X.deviations (derived in tests/boundary_layer_cases.py).  Every case
has a decision margin >= 1e-9, so no decision can differ; what remains is the device's pow and log against libm's."""
import datetime
import importlib.util
import os

import numpy as np
import pytest

import climt_amd
from climt_amd import _hip
from climt_amd._sympl_compat import DataArray
from helpers import ROOT, maxdiff

import boundary_layer_cases as X

pytestmark = pytest.mark.gpu

FLUXES = ("surface_upward_sensible_heat_flux", "surface_upward_latent_heat_flux")
DIAG = ("stress_north", "stress_east", "height", "sh_out", "lh_out")


@pytest.fixture(scope="module")
def ctx():
    from climt_amd.rrtmg.common import make_context
    return make_context(0)


def _result(t, q, u, v, d):
    got = dict(t_new=t, q_new=q, u_new=u, v_new=v)
    if d:
        got.update({k: d.get(n) for k, n in zip(X.DIAGNOSTICS, DIAG)})
    return got


def host_call(ctx, c, mode, **kw):
    fluxes = dict(sh_in=c["sh_in"], lh_in=c["lh_in"]) if mode == 2 else {}
    return _result(*ctx.boundary_layer(c["t"], c["q"], c["u"], c["v"], c["p"], c["p_int"], c["ps"], c["ts"], c["qs"], X.DT, X.CONSTANTS, mode, **fluxes, **kw))


def device_call(ctx, c, mode, in_place=False):
    """Device pointers -> the results on the host."""
    nlay, ncol = c["t"].shape
    d = {k: _hip.DeviceArray.from_host(np.ascontiguousarray(c[k])) for k in X.INPUTS}
    out = [d[k] if in_place else _hip.DeviceArray((nlay, ncol)) for k in "tquv"]
    diag = {n: _hip.DeviceArray((ncol,)) for n in DIAG}
    fluxes = dict(sh_in=d["sh_in"], lh_in=d["lh_in"]) if mode == 2 else {}
    ctx.boundary_layer(d["t"], d["q"], d["u"], d["v"], d["p"], d["p_int"], d["ps"], d["ts"], d["qs"], X.DT, X.CONSTANTS, mode,
                       t_out=out[0], q_out=out[1], u_out=out[2], v_out=out[3], diagnostics=diag, memspace=1, ncol=ncol, nlay=nlay, **fluxes)
    ctx.synchronize()
    if not in_place:      # the inputs of an out-of-place call are only read
        assert all(X.same_bits(d[k].download(), c[k]) for k in "tquv")
    return _result(*(o.download() for o in out), {n: x.download() for n, x in diag.items()})


def same(a, b):
    return all(X.same_bits(a[k], b[k]) for k in a)


@pytest.mark.parametrize("mode", X.MODES)
@pytest.mark.parametrize("name", X.CASES)
def test_kernel_equals_the_statement_on_every_shape(ctx, name, mode):
    worst = {}
    for nlay in X.NLAYS:
        for ncol in X.NCOLS:
            c = X.case(name, nlay, ncol, mode)
            got = host_call(ctx, c, mode)
            dev = X.deviations(got, c)
            assert len(dev) == 9
            for k, v in dev.items():
                worst[k] = max(worst.get(k, 0.0), v)
            # count and height through the diagnostics: h is z[count - 1] of the statement's own search (z[n - 1] where it found none)
            for k, v in dev.items():
                assert v <= X.TOL, (name, mode, nlay, ncol, k, v)
    print("boundary_layer_kernel, %s, mode %d: largest deviation / scale from the statement %s" % (
        name, mode, ", ".join("%s %.2e" % kv for kv in sorted(worst.items()))))


def test_every_diagnostic_pointer_may_be_null(ctx):
    for name, mode, nlay, ncol in (("varied", 1, 30, 65), ("heated", 2, 3, 130), ("calm", 0, 61, 1)):
        c = X.case(name, nlay, ncol, mode)
        full, bare = host_call(ctx, c, mode), host_call(ctx, c, mode, diagnostics=None)
        assert set(bare) == set(X.PROFILES) and all(X.same_bits(bare[k], full[k]) for k in bare)
        some = host_call(ctx, c, mode, diagnostics=dict(height=np.empty(ncol), lh_out=np.empty(ncol)))
        assert X.same_bits(some["height"], full["height"]) and X.same_bits(some["lh"], full["lh"]) and some["sh"] is None


@pytest.mark.parametrize("mode", (1, 2))
def test_each_diagnostic_left_out_leaves_the_others_their_bits(ctx, mode):
    """Host pointers, 65 columns (two tiles, one live lane in the second) by 3 layers, bulk fluxes and prescribed ones (sh_in and
    lh_in are staged as well): the staging buffer of a call is laid out over the arrays that are given, so every diagnostic in
    turn is left out of an otherwise full call.  What is still asked for has the bits of the full call, in the caller's own
    arrays, and the inputs keep theirs."""
    c = X.case("varied", 3, 65, mode)
    before = {k: np.array(c[k]) for k in X.INPUTS}
    full = host_call(ctx, c, mode)
    for left_out, key in zip(DIAG, X.DIAGNOSTICS):
        diag = {n: np.full(65, -7.0) for n in DIAG if n != left_out}
        got = host_call(ctx, c, mode, diagnostics=diag)
        assert got[key] is None and all(got[k] is diag[n] for k, n in zip(X.DIAGNOSTICS, DIAG) if n != left_out)
        assert all(X.same_bits(got[k], full[k]) for k in got if k != key), left_out
        assert all(X.same_bits(c[k], before[k]) for k in X.INPUTS), left_out


@pytest.mark.parametrize("mode", X.MODES)
def test_in_place_host_and_device_pointers_agree_bit_for_bit(ctx, mode):
    for name, nlay, ncol in (("varied", 3, 1), ("heated", 30, 130), ("varied", 61, 65), ("calm", 2, 64)):
        c = X.case(name, nlay, ncol, mode)
        want = host_call(ctx, c, mode)
        # host arrays, in place
        io = {k: np.array(c[k]) for k in "tquv"}
        got = host_call(ctx, dict(c, **io), mode, t_out=io["t"], q_out=io["q"], u_out=io["u"], v_out=io["v"])
        assert got["t_new"] is io["t"] and same(got, want)
        # device pointers, out of place and in place
        for in_place in (False, True):
            assert same(device_call(ctx, c, mode, in_place), want), (name, nlay, ncol, in_place)


def test_a_block_of_columns_alone_equals_the_block_inside_the_whole(ctx):
    for name, mode in (("varied", 1), ("varied", 2), ("calm", 0)):
        c = X.case(name, 30, 130, mode)
        whole = host_call(ctx, c, mode)
        for a, b in ((1, 2), (37, 101), (63, 130), (5, 69)):
            part = {k: np.ascontiguousarray(c[k][..., a:b]) for k in X.INPUTS}
            got = host_call(ctx, part, mode)
            assert all(X.same_bits(got[k], whole[k][..., a:b]) for k in got), (name, mode, a, b)


def test_a_decoupled_column_without_surface_exchange_keeps_its_bits(ctx):
    for nlay, ncol in ((2, 1), (30, 65), (61, 130)):
        c = X.case("decoupled", nlay, ncol, 0)
        got = host_call(ctx, c, 0)
        assert all(X.same_bits(got[k + "_new"], c[k]) for k in "tquv")
        assert not got["stress_north"].any() and not got["sh"].any()
    # one decoupled column among coupled ones
    c, d = X.case("heated", 30, 65, 0), X.case("decoupled", 30, 65, 0)
    mixed = {k: np.array(c[k]) for k in X.INPUTS}
    for k in X.INPUTS:
        mixed[k][..., 17] = d[k][..., 17]
    got = host_call(ctx, mixed, 0)
    assert all(X.same_bits(got[k + "_new"][:, 17], mixed[k][:, 17]) for k in "tquv")
    assert not X.same_bits(got["u_new"][:, 16], mixed["u"][:, 16])


def _state(c, ny, nx, mode, pressure_units="Pa"):
    """[levels][lat][lon]: resident as the host path hands it to the library; the pressures in `pressure_units`."""
    f = {"Pa": 1.0, "mbar": 100.0}[pressure_units]
    lev = lambda a, dim, units, div=1.0: DataArray(a.reshape(a.shape[0], ny, nx) / div, dims=(dim, "lat", "lon"), attrs={"units": units})
    col = lambda a, units, div=1.0: DataArray(a.reshape(ny, nx) / div, dims=("lat", "lon"), attrs={"units": units})
    state = {"air_temperature": lev(c["t"], "mid_levels", "degK"), "specific_humidity": lev(c["q"], "mid_levels", "kg/kg"),
             "eastward_wind": lev(c["u"], "mid_levels", "m s^-1"), "northward_wind": lev(c["v"], "mid_levels", "m s^-1"),
             "air_pressure": lev(c["p"], "mid_levels", pressure_units, f),
             "air_pressure_on_interface_levels": lev(c["p_int"], "interface_levels", pressure_units, f),
             "surface_air_pressure": col(c["ps"], pressure_units, f), "surface_temperature": col(c["ts"], "degK"),
             "surface_specific_humidity": col(c["qs"], "kg/kg"), "time": datetime.datetime(2000, 1, 1)}
    if mode == 2:
        state.update({FLUXES[0]: col(c["sh_in"], "W m^-2"), FLUXES[1]: col(c["lh_in"], "W m^-2")})
    return state


class ResidentPressureUnits:
    """A component listed first in DeviceState.from_host so that the pressures become resident in its units."""

    def __init__(self, units):
        self.input_properties = {"air_pressure": {"dims": ["mid_levels", "*"], "units": units},
                                 "air_pressure_on_interface_levels": {"dims": ["interface_levels", "*"], "units": units},
                                 "surface_air_pressure": {"dims": ["*"], "units": units}}


@pytest.mark.parametrize("units", ["Pa", "mbar"])
@pytest.mark.parametrize("surface_fluxes", [None, "bulk", "external"])
def test_component_on_a_device_state_equals_the_host_state_bit_for_bit(ctx, surface_fluxes, units):
    mode = {None: 0, "bulk": 1, "external": 2}[surface_fluxes]
    c = X.case("varied", 30, 65, mode)
    bl = climt_amd.SimpleBoundaryLayer(surface_fluxes=surface_fluxes, context=ctx)
    dt = datetime.timedelta(seconds=X.DT)
    state = _state(c, 5, 13, mode, units)
    diagnostics, new_state = bl(state, dt)
    if units == "Pa":
        got = dict(t_new=new_state["air_temperature"].values.reshape(30, 65), q_new=new_state["specific_humidity"].values.reshape(30, 65),
                   u_new=new_state["eastward_wind"].values.reshape(30, 65), v_new=new_state["northward_wind"].values.reshape(30, 65))
        assert max(X.deviations(got, c).values()) <= X.TOL
    names = ("air_temperature", "specific_humidity", "eastward_wind", "northward_wind")
    with climt_amd.DeviceState.from_host(state, [ResidentPressureUnits(units), bl], context=ctx) as ds:
        assert ds["air_pressure"].units == units and ds["surface_air_pressure"].units == units
        before = {n: ds[n] for n in names}
        diag_d, ds2 = bl(ds, dt)
        assert ds2 is ds and set(diag_d) == set(diagnostics)
        assert all(ds[n] is not before[n] and isinstance(ds[n], climt_amd.DeviceQuantity) for n in names)      # rebound to work buffers
        ds.update(diag_d)
        for n in names + tuple(diag_d):
            got, want = ds.download(n), (new_state.get(n) if n in new_state else diagnostics[n])
            assert got.dims == want.dims and got.attrs["units"] == want.attrs["units"], n
            assert X.same_bits(got.values, want.values), n
        first = {n: ds[n] for n in names}
        kept = {n: ds[n].buf.download() for n in names}
        assert all(X.same_bits(before[n].buf.download().reshape(30, 65), c[k]) for n, k in zip(names, "tquv"))      # the previous arrays stay
        # the next step: the other set of buffers, the first step's arrays intact
        ds.step_count += 1
        bl(ds, dt)
        assert all(ds[n] is not first[n] and ds[n].ptr != first[n].ptr for n in names)
        ds.ctx.synchronize()
        assert all(X.same_bits(first[n].buf.download(), kept[n]) for n in names)
        host2 = dict(state)
        host2.update(new_state)
        _, new_state2 = bl(host2, dt)
        for n in names:
            assert X.same_bits(ds.download(n).values, new_state2[n].values), n


def test_device_call_refuses_a_state_of_another_shape(ctx):
    c = X.case("varied", 30, 65, 1)
    bl = climt_amd.SimpleBoundaryLayer(context=ctx)
    state = _state(c, 5, 13, 1)
    with climt_amd.DeviceState.from_host(state, [bl], context=ctx) as ds:
        q = ds["air_pressure_on_interface_levels"]
        ds["air_pressure_on_interface_levels"] = climt_amd.DeviceQuantity(q.buf, (30, 65), q.dims, q.units)
        with pytest.raises(ValueError, match="do not belong to one grid"):
            bl(ds, datetime.timedelta(seconds=X.DT))
        ds["air_pressure_on_interface_levels"] = climt_amd.DeviceQuantity(q.buf, q.shape, ("*", "interface_levels"), q.units)
        with pytest.raises(ValueError, match="resident as"):
            bl(ds, datetime.timedelta(seconds=X.DT))


def test_slab_surface_takes_the_resident_flux_diagnostics(ctx):
    """The two flux diagnostics of the boundary layer, still in HBM, as the inputs of SlabSurface's device call: the slab's
    tendency equals the one of the host path fed with the downloaded fluxes."""
    c = X.case("heated", 30, 65, 1)
    bl, slab = climt_amd.SimpleBoundaryLayer(context=ctx), climt_amd.SlabSurface()
    state = climt_amd.get_default_state([slab], grid_state=climt_amd.get_grid(nx=13, ny=5, nz=30))
    for n, x in _state(c, 5, 13, 1).items():      # the boundary layer's profiles and surface values into the slab's default state
        if n != "time":
            state[n] = x
    for n in ("downwelling_shortwave_flux_in_air", "downwelling_longwave_flux_in_air"):
        state[n].values[...] = 150.0
    dt = datetime.timedelta(seconds=X.DT)
    diagnostics, _ = bl(state, dt)
    assert np.abs(diagnostics[FLUXES[0]].values).min() > 1.0
    tend_without, _ = slab(state)      # (the default state's fluxes: zero)
    host = dict(state)
    host.update(diagnostics)
    tend_h, _ = slab(host)
    want = np.asarray(tend_h["surface_temperature"].values, dtype=np.float64).reshape(-1)
    assert np.abs(want - np.asarray(tend_without["surface_temperature"].values).reshape(-1)).min() > 0.0
    with climt_amd.DeviceState.from_host(state, [slab, bl], context=ctx) as ds:
        diag_d, _ = bl(ds, dt)
        ds.update(diag_d)
        assert ds[FLUXES[0]] is diag_d[FLUXES[0]] and ds[FLUXES[0]].dims == ("*",) and ds[FLUXES[0]].units == "W m^-2"
        tend_d, _ = slab(ds)
        ds["tend"] = tend_d["surface_temperature"]
        got = ds.download("tend").values.reshape(-1)
    assert maxdiff(got, want) <= 1e-12 * float(np.abs(want).max())


def test_radiative_convective_example_with_the_boundary_layer_in_both_modes():
    """Three steps of examples/radiative_convective.py with boundary_layer=True on a host state and on a DeviceState: the state of
    the two modes to the tolerance of the example's own test (tests/test_dry_adjustment_gpu.py); the surface exchanges heat with
    the column from step 0."""
    spec = importlib.util.spec_from_file_location("radiative_convective", os.path.join(ROOT, "examples", "radiative_convective.py"))
    ex = importlib.util.module_from_spec(spec); spec.loader.exec_module(ex)
    first_h, end_h = ex.run(3, device_resident=False, boundary_layer=True)
    first_d, end_d = ex.run(3, device_resident=True, boundary_layer=True)
    for first in (first_h, first_d):
        assert "upwelling_longwave_flux_in_air" in first and "boundary_layer_height" in first
        assert float(np.abs(first[FLUXES[0]].values).min()) > 0.0
    assert maxdiff(first_h[FLUXES[0]].values.ravel(), first_d[FLUXES[0]].values.ravel()) <= 1e-9
    for name in ("air_temperature", "specific_humidity", "surface_temperature", "eastward_wind", "northward_wind") + FLUXES:
        h, d = end_h[name], end_d[name]
        g = np.transpose(d.values, [d.dims.index(x) for x in h.dims])
        assert np.all(np.isfinite(h.values)) and maxdiff(h.values, g) <= 1e-9, (name, maxdiff(h.values, g))
    # the run without the flag is another run: there the wind stays at rest and no flux reaches the slab
    _, plain = ex.run(3, device_resident=False)
    assert "eastward_wind" not in plain or not np.any(plain["eastward_wind"].values)
    assert float(end_h["eastward_wind"].values.ravel()[0]) < 5.0      # drag on the lowest layer
