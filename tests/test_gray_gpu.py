"""The gray radiation path on the GPU: frierson_kernel, gray_longwave_kernel and grid_scale_condensation_kernel against the numpy
statements (tests/gray_cases.py) on every case and shape; what must hold bit for bit -- the fused call against the depth followed
by the sweep, hr = tend * 86400, the transparent and opaque identities, unsaturated layers and dry columns, NULL optionals, host
against device pointers and in place, a block of columns alone, a saturated column among dry ones; the components on a
DeviceState (pressures resident in Pa and in mbar); and examples/radiative_convective.py with each new flag in both modes.

Values against the statements: the tolerances stored in tests/golden/gray_<case>.npz and gsc_<case>.npz, measured by the maker on
the reference itself (16 x its largest deviation under +-1 ulp of every input, at least 1e-13), on the scales of X.deviations.
Every condensation case has a decision margin >= 1e-9, so no decision can differ; what remains is the device's exp, pow and sin
against numpy's.  The largest deviations are printed by the first two tests (docs/EXPERIMENTS.md W has the figures)."""
import datetime
import importlib.util
import os

import numpy as np
import pytest

import climt_amd
from climt_amd import _hip
from climt_amd._sympl_compat import DataArray
from helpers import ROOT, maxdiff

import gray_cases as X

pytestmark = pytest.mark.gpu

TAU = "longwave_optical_depth_on_interface_levels"
GRAY_OUT = ("up", "dn", "tend", "hr", "tau_out")


@pytest.fixture(scope="module")
def ctx():
    from climt_amd.rrtmg.common import make_context
    return make_context(0)


def gray_call(ctx, c, fused=False, **kw):
    """Host pointers -> dict of up, dn, tend, hr and (fused) tau_out."""
    which = dict(ps=c["ps"], lat=c["lat"], frierson=X.FRIERSON) if fused else dict(tau=c["tau"])
    up, dn, tend, d = ctx.gray_longwave(c["t"], c["tsfc"], c["p_int"], X.GRAY_CONSTANTS, **which, **kw)
    return dict(up=up, dn=dn, tend=tend, **(d or {}))


def depth_call(ctx, c):
    return ctx.frierson_optical_depth(c["p_int"], c["ps"], c["lat"], X.FRIERSON)


def gsc_call(ctx, c, **kw):
    t, q, d = ctx.grid_scale_condensation(c["t"], c["q"], c["p"], c["p_int"], X.GSC_CONSTANTS, **kw)
    return dict(t_new=t, q_new=q, **({"precip": d["precip"]} if d and "precip" in d else {}))


def same(a, b, keys=None):
    return all(X.same_bits(a[k], b[k]) for k in (keys or a))


@pytest.mark.parametrize("name", X.GRAY_CASES)
def test_gray_kernels_equal_the_statements_on_every_shape(ctx, name):
    worst, tol = {}, X.tolerances("gray", name)
    for nlay in X.NLAYS:
        for ncol in X.NCOLS:
            c = X.gray_case(name, nlay, ncol)
            got, fused, depth = gray_call(ctx, c), gray_call(ctx, c, fused=True), depth_call(ctx, c)
            devs = [X.deviations(got, c, X.GRAY_FIELDS)]
            assert len(devs[0]) == 4
            # exact, on every case and shape: the fused call IS the depth followed by the sweep on it; the heating rate; the top
            two = gray_call(ctx, dict(c, tau=depth))
            assert X.same_bits(fused["tau_out"], depth) and same(two, fused, X.GRAY_FIELDS), (name, nlay, ncol)
            assert X.same_bits(got["hr"], got["tend"] * 86400.0) and X.same_bits(got["dn"][-1], np.zeros(ncol))
            if name in X.FUSED_CASES:      # the case's depth is the Frierson depth: depth and fused call against the same statement
                devs.append(X.deviations(dict(fused, tau=depth), c, X.GRAY_FIELDS + ("tau",)))
                assert len(devs[1]) == 5
            if name == "transparent":
                assert X.same_bits(got["dn"], np.zeros((nlay + 1, ncol))) and X.same_bits(got["up"], np.ones((nlay + 1, 1)) * got["up"][0][None, :])
            if name == "opaque":      # exp underflows: every level carries sigma T^4 of the layer next to it, bit for bit (Ts = T[0])
                assert X.same_bits(got["up"][1:], got["dn"][:-1]) and X.same_bits(got["up"][0], got["up"][1])
            for dev in devs:
                for k, v in dev.items():
                    worst[k] = max(worst.get(k, 0.0), v)
    print("gray_longwave_kernel / frierson_kernel, %s: largest deviation from the statement (tolerance) %s" % (
        name, ", ".join("%s %.2e (%.1e)" % (k, v, tol[k]) for k, v in sorted(worst.items()))))
    for k, v in worst.items():
        assert v <= tol[k], (name, k, v, tol[k])


@pytest.mark.parametrize("name", X.GSC_CASES)
def test_condensation_kernel_equals_the_statement_on_every_shape(ctx, name):
    worst, tol = {}, X.tolerances("gsc", name)
    for nlay in X.NLAYS:
        for ncol in X.NCOLS:
            c = X.gsc_case(name, nlay, ncol)
            got = gsc_call(ctx, c)
            dev = X.deviations(got, c, X.GSC_FIELDS)
            assert len(dev) == 3
            for k, v in dev.items():
                worst[k] = max(worst.get(k, 0.0), v)
            dry = ~c["saturated"]      # unsaturated layers keep their input bits; all-dry columns rain exact +0.0
            assert X.same_bits(got["t_new"][dry], c["t"][dry]) and X.same_bits(got["q_new"][dry], c["q"][dry])
            assert X.same_bits(got["precip"][dry.all(axis=0)], np.zeros(int(dry.all(axis=0).sum())))
            assert (got["t_new"][~dry] > c["t"][~dry]).all() and (got["q_new"][~dry] < c["q"][~dry]).all()
    print("grid_scale_condensation_kernel, %s: largest deviation from the statement (tolerance) %s" % (
        name, ", ".join("%s %.2e (%.1e)" % (k, v, tol[k]) for k, v in sorted(worst.items()))))
    for k, v in worst.items():
        assert v <= tol[k], (name, k, v, tol[k])


def test_every_optional_pointer_null_in_turn_leaves_the_others_their_bits(ctx):
    """Host pointers, 65 columns (two tiles, one live lane in the second): the staging buffer of a call is laid out over the arrays
    that are given, so every optional array is in turn left out of an otherwise full call."""
    for nlay in (2, 30):
        c = X.gray_case("varied", nlay, 65)
        before = {k: np.array(c[k]) for k in X.GRAY_INPUTS}
        for fused in (False, True):
            full = gray_call(ctx, c, fused=fused)
            optional = ("hr", "tau_out") if fused else ("hr",)
            assert set(full) == {"up", "dn", "tend"} | set(optional)
            for left_out in optional + (None,):
                shapes = dict(hr=(nlay, 65), tau_out=(nlay + 1, 65))
                diag = {n: np.full(shapes[n], -7.0) for n in ("hr", "tau_out") if n != left_out}      # (unfused: tau_out copies the depth read)
                got = gray_call(ctx, c, fused=fused, diagnostics=diag)
                assert all(got[n] is diag[n] for n in diag) and left_out not in got
                assert same(got, dict(full, tau_out=full.get("tau_out", c["tau"]))), (nlay, fused, left_out)
            bare = gray_call(ctx, c, fused=fused, diagnostics=None)
            assert set(bare) == {"up", "dn", "tend"} and same(bare, full)
            assert all(X.same_bits(c[k], before[k]) for k in X.GRAY_INPUTS)
        g = X.gsc_case("alternate", nlay, 65)
        full, bare = gsc_call(ctx, g), gsc_call(ctx, g, diagnostics=None)
        assert set(bare) == {"t_new", "q_new"} and same(bare, full) and "precip" in full


def test_host_pointers_device_pointers_and_in_place_agree_bit_for_bit(ctx):
    for name, nlay, ncol in (("varied", 1, 1), ("zero_dtau", 30, 130), ("decreasing", 61, 65), ("opaque", 2, 64)):
        c = X.gray_case(name, nlay, ncol)
        d = {k: _hip.DeviceArray.from_host(np.ascontiguousarray(c[k])) for k in X.GRAY_INPUTS}
        il, ml = (nlay + 1, ncol), (nlay, ncol)
        for fused in (False, True):
            want = gray_call(ctx, c, fused=fused)
            out = {n: _hip.DeviceArray(il if n in ("up", "dn", "tau_out") else ml) for n in GRAY_OUT}
            which = dict(ps=d["ps"], lat=d["lat"], frierson=X.FRIERSON) if fused else dict(tau=d["tau"])
            ctx.gray_longwave(d["t"], d["tsfc"], d["p_int"], X.GRAY_CONSTANTS, up=out["up"], dn=out["dn"], tend=out["tend"],
                              diagnostics=dict(hr=out["hr"], tau_out=out["tau_out"]), memspace=1, ncol=ncol, nlay=nlay, **which)
            ctx.synchronize()
            got = {n: x.download() for n, x in out.items()}
            assert same(dict(want, tau_out=want.get("tau_out", c["tau"])), got), (name, nlay, ncol, fused)
            assert all(X.same_bits(d[k].download(), c[k]) for k in X.GRAY_INPUTS)      # only read
        tau = _hip.DeviceArray(il)
        ctx.frierson_optical_depth(d["p_int"], d["ps"], d["lat"], X.FRIERSON, tau=tau, memspace=1, ncol=ncol, nlay=nlay)
        ctx.synchronize()
        assert X.same_bits(tau.download(), depth_call(ctx, c))
    for name, nlay, ncol in (("alternate", 1, 1), ("supersaturated", 30, 130), ("cold_stratosphere", 61, 65), ("top_only", 2, 64)):
        c = X.gsc_case(name, nlay, ncol)
        want = gsc_call(ctx, c)
        io = {k: np.array(c[k]) for k in "tq"}      # host arrays, in place
        got = gsc_call(ctx, dict(c, **io), t_out=io["t"], q_out=io["q"])
        assert got["t_new"] is io["t"] and same(got, want)
        for in_place in (False, True):
            d = {k: _hip.DeviceArray.from_host(np.ascontiguousarray(c[k])) for k in X.GSC_INPUTS}
            out = [d[k] if in_place else _hip.DeviceArray((nlay, ncol)) for k in "tq"]
            precip = _hip.DeviceArray((ncol,))
            ctx.grid_scale_condensation(d["t"], d["q"], d["p"], d["p_int"], X.GSC_CONSTANTS, t_out=out[0], q_out=out[1], diagnostics=dict(precip=precip),
                                        memspace=1, ncol=ncol, nlay=nlay)
            ctx.synchronize()
            assert same(dict(t_new=out[0].download(), q_new=out[1].download(), precip=precip.download()), want), (name, in_place)
            if not in_place:
                assert all(X.same_bits(d[k].download(), c[k]) for k in X.GSC_INPUTS)


def test_a_block_of_columns_alone_equals_the_block_inside_the_whole(ctx):
    c, g = X.gray_case("varied", 30, 130), X.gsc_case("alternate", 30, 130)
    whole, whole_f, whole_g = gray_call(ctx, c), gray_call(ctx, c, fused=True), gsc_call(ctx, g)
    for a, b in ((1, 2), (37, 101), (63, 130), (5, 69)):
        part = {k: np.ascontiguousarray(c[k][..., a:b]) for k in X.GRAY_INPUTS}
        for fused, want in ((False, whole), (True, whole_f)):
            got = gray_call(ctx, part, fused=fused)
            assert all(X.same_bits(got[k], want[k][..., a:b]) for k in got), (a, b, fused)
        got = gsc_call(ctx, {k: np.ascontiguousarray(g[k][..., a:b]) for k in X.GSC_INPUTS})
        assert all(X.same_bits(got[k], whole_g[k][..., a:b]) for k in got), (a, b)


def test_a_saturated_column_among_dry_ones_does_not_disturb_its_neighbours(ctx):
    for nlay, ncol in ((30, 65), (61, 130)):
        dry, wet = X.gsc_case("dry", nlay, ncol), X.gsc_case("supersaturated", nlay, ncol)
        mixed = {k: np.array(dry[k]) for k in X.GSC_INPUTS}
        for k in X.GSC_INPUTS:
            mixed[k][..., 17] = wet[k][..., 17]
        got, alone = gsc_call(ctx, mixed), gsc_call(ctx, wet)
        others = np.arange(ncol) != 17
        assert X.same_bits(got["t_new"][:, others], dry["t"][:, others]) and X.same_bits(got["q_new"][:, others], dry["q"][:, others])
        assert X.same_bits(got["precip"][others], np.zeros(ncol - 1)) and got["precip"][17] < 0
        assert all(X.same_bits(got[k][..., 17], alone[k][..., 17]) for k in got)


# ---- the components on a DeviceState ---------------------------------------------------------------------------------------------------
def _state(c, g, ny, nx, pressure_units="Pa", tau=None):
    """[levels][lat][lon]: resident as the host path hands it to the library; the pressures in `pressure_units`."""
    f = {"Pa": 1.0, "mbar": 100.0}[pressure_units]
    lev = lambda a, dim, units, div=1.0: DataArray(a.reshape(a.shape[0], ny, nx) / div, dims=(dim, "lat", "lon"), attrs={"units": units})
    col = lambda a, units, div=1.0: DataArray(a.reshape(ny, nx) / div, dims=("lat", "lon"), attrs={"units": units})
    state = {"air_temperature": lev(g["t"], "mid_levels", "degK"), "specific_humidity": lev(g["q"], "mid_levels", "kg/kg"),
             "surface_temperature": col(c["tsfc"], "degK"), "air_pressure": lev(g["p"], "mid_levels", pressure_units, f),
             "air_pressure_on_interface_levels": lev(c["p_int"], "interface_levels", pressure_units, f),
             "surface_air_pressure": col(c["ps"], pressure_units, f), "latitude": col(c["lat"], "degrees_north"), "time": datetime.datetime(2000, 1, 1)}
    if tau is not None:
        state[TAU] = lev(tau, "interface_levels", "dimensionless")
    return state


class ResidentPressureUnits:
    """A component listed first in DeviceState.from_host so that the pressures become resident in its units."""

    def __init__(self, units):
        self.input_properties = {"air_pressure": {"dims": ["mid_levels", "*"], "units": units},
                                 "air_pressure_on_interface_levels": {"dims": ["interface_levels", "*"], "units": units},
                                 "surface_air_pressure": {"dims": ["*"], "units": units}}


@pytest.mark.parametrize("units", ["Pa", "mbar"])
def test_components_on_a_device_state_equal_the_host_state_bit_for_bit(ctx, units):
    c, g = X.gray_case("varied", 30, 65), X.gsc_case("alternate", 30, 65)
    depth = climt_amd.Frierson06LongwaveOpticalDepth(context=ctx)
    gray, fused, gsc = climt_amd.GrayLongwaveRadiation(context=ctx), climt_amd.GrayLongwaveRadiation(optical_depth=depth, context=ctx), climt_amd.GridScaleCondensation(context=ctx)
    dt = datetime.timedelta(seconds=600)
    state = _state(c, g, 5, 13, units)
    host_tau = depth(state)
    state.update(host_tau)
    host_t, host_d = gray(state)
    host_ft, host_fd = fused(state)
    host_diag, host_new = gsc(state, dt)
    assert X.same_bits(host_fd[TAU].values, host_tau[TAU].values) and all(X.same_bits(host_fd[n].values, host_d[n].values) for n in host_d)
    if units == "Pa":
        tol = X.tolerances("gsc", "alternate")
        got = dict(t_new=host_new["air_temperature"].values.reshape(30, 65), q_new=host_new["specific_humidity"].values.reshape(30, 65),
                   precip=host_diag["precipitation_amount"].values.ravel())
        assert X.within(X.deviations(got, g, X.GSC_FIELDS), tol)
    with climt_amd.DeviceState.from_host(state, [ResidentPressureUnits(units), depth, gray, fused, gsc], context=ctx) as ds:
        assert ds["air_pressure_on_interface_levels"].units == units and ds["surface_air_pressure"].units == units
        dev_tau = depth(ds)
        assert set(dev_tau) == {TAU} and isinstance(dev_tau[TAU], climt_amd.DeviceQuantity) and tuple(dev_tau[TAU].dims) == ("interface_levels", "*")
        ds.update(dev_tau)
        dev_t, dev_d = gray(ds)
        dev_ft, dev_fd = fused(ds)
        assert set(dev_d) == set(host_d) and set(dev_fd) == set(host_fd) and set(dev_t) == {"air_temperature"} == set(dev_ft)
        assert all(isinstance(x, climt_amd.DeviceQuantity) for x in list(dev_d.values()) + list(dev_fd.values()) + list(dev_t.values()) + list(dev_ft.values()))
        assert dev_t["air_temperature"].units == "degK s^-1" and dev_d["upwelling_longwave_flux_in_air"].dims == ("interface_levels", "*")
        for tag, dev, host in (("tau", dev_tau, host_tau), ("gray", dict(dev_d, tendency=dev_t["air_temperature"]), dict(host_d, tendency=host_t["air_temperature"])),
                               ("fused", dict(dev_fd, tendency=dev_ft["air_temperature"]), dict(host_fd, tendency=host_ft["air_temperature"]))):
            for n, q in dev.items():
                ds["probe"] = q
                got = ds.download("probe")
                assert got.dims == host[n].dims and got.attrs["units"] == host[n].attrs["units"], (tag, n)
                assert X.same_bits(got.values, host[n].values), (tag, n)
        before = {n: ds[n] for n in ("air_temperature", "specific_humidity")}
        dev_diag, ds2 = gsc(ds, dt)
        assert ds2 is ds and set(dev_diag) == {"precipitation_amount"} and tuple(dev_diag["precipitation_amount"].dims) == ("*",)
        assert all(ds[n] is not before[n] and isinstance(ds[n], climt_amd.DeviceQuantity) for n in before)      # rebound to work buffers
        ds.update(dev_diag)
        for n, want in list(host_new.items()) + list(host_diag.items()):
            got = ds.download(n)
            assert got.dims == want.dims and got.attrs["units"] == want.attrs["units"] and X.same_bits(got.values, want.values), n
        assert X.same_bits(before["air_temperature"].buf.download().reshape(30, 65), g["t"])      # the previous arrays stay
        first = {n: ds[n] for n in before}
        ds.step_count += 1
        gsc(ds, dt)
        assert all(ds[n] is not first[n] and ds[n].ptr != first[n].ptr for n in before)      # the next step: the other set of buffers


def test_device_adams_bashforth_takes_the_gray_tendency(ctx):
    c, g = X.gray_case("varied", 30, 65), X.gsc_case("dry", 30, 65)
    fused = climt_amd.GrayLongwaveRadiation(optical_depth=climt_amd.Frierson06LongwaveOpticalDepth(context=ctx), context=ctx)
    dt = datetime.timedelta(seconds=600)
    state = _state(c, g, 5, 13)
    tend, _ = fused(state)
    want = state["air_temperature"].values + 600.0 * tend["air_temperature"].values
    with climt_amd.DeviceState.from_host(state, [fused], context=ctx) as ds:
        diagnostics, ds = climt_amd.DeviceAdamsBashforth([fused])(ds, dt)
        assert TAU in diagnostics
        got = ds.download("air_temperature").values
    assert maxdiff(got, want) <= 4 * np.spacing(300.0)


def test_device_calls_refuse_a_state_of_another_shape(ctx):
    c, g = X.gray_case("varied", 30, 65), X.gsc_case("alternate", 30, 65)
    depth = climt_amd.Frierson06LongwaveOpticalDepth(context=ctx)
    gray, fused, gsc = climt_amd.GrayLongwaveRadiation(context=ctx), climt_amd.GrayLongwaveRadiation(optical_depth=depth, context=ctx), climt_amd.GridScaleCondensation(context=ctx)
    dt = datetime.timedelta(seconds=600)
    with climt_amd.DeviceState.from_host(_state(c, g, 5, 13, tau=c["tau"]), [depth, gray, fused, gsc], context=ctx) as ds:
        q = ds["air_pressure_on_interface_levels"]
        ds["air_pressure_on_interface_levels"] = climt_amd.DeviceQuantity(q.buf, (30, 65), q.dims, q.units)
        for call in (lambda: gray(ds), lambda: fused(ds), lambda: gsc(ds, dt)):      # (the depth alone has no second array of levels)
            with pytest.raises(ValueError, match="do not belong to one grid"):
                call()
        ds["air_pressure_on_interface_levels"] = climt_amd.DeviceQuantity(q.buf, q.shape, ("*", "interface_levels"), q.units)
        for call in (lambda: gray(ds), lambda: fused(ds), lambda: gsc(ds, dt), lambda: depth(ds)):
            with pytest.raises(ValueError, match="resident as"):
                call()
        ds["air_pressure_on_interface_levels"] = q
        lat = ds["latitude"]
        ds["latitude"] = climt_amd.DeviceQuantity(lat.buf, lat.shape, lat.dims, "radians")
        with pytest.raises(ValueError):
            fused(ds)


# ---- the example -----------------------------------------------------------------------------------------------------------------------
def test_radiative_convective_example_with_each_new_flag_in_both_modes():
    """Three steps of examples/radiative_convective.py with gray_longwave and with grid_scale_condensation on a host state and on a
    DeviceState: the two modes to the tolerance of the example's own test (tests/test_dry_adjustment_gpu.py, 1e-9); the
    condensation flag is exclusive with simple_physics; the run without the flags is unchanged."""
    spec = importlib.util.spec_from_file_location("radiative_convective", os.path.join(ROOT, "examples", "radiative_convective.py"))
    ex = importlib.util.module_from_spec(spec); spec.loader.exec_module(ex)
    names = ("air_temperature", "specific_humidity", "surface_temperature")
    runs = {}
    for flag, extra in (("gray_longwave", (TAU, "upwelling_longwave_flux_in_air", "air_temperature_tendency_from_longwave")),
                        ("grid_scale_condensation", ("precipitation_amount",))):
        first_h, end_h = ex.run(3, device_resident=False, **{flag: True})
        first_d, end_d = ex.run(3, device_resident=True, **{flag: True})
        runs[flag] = end_h
        for n in extra:
            assert n in first_h and n in first_d
            h, d = first_h[n], first_d[n]
            assert maxdiff(h.values.ravel(), np.transpose(d.values, [d.dims.index(x) for x in h.dims]).ravel()) <= 1e-9 * max(1.0, float(np.abs(h.values).max())), n
        for n in names + extra:
            h, d = end_h[n], end_d[n]
            gd = np.transpose(d.values, [d.dims.index(x) for x in h.dims])
            assert np.all(np.isfinite(h.values)) and maxdiff(h.values, gd) <= 1e-9 * max(1.0, float(np.abs(h.values).max())), (flag, n, maxdiff(h.values, gd))
        if flag == "gray_longwave":
            depth = first_h[TAU].values.ravel()
            # (the default state's surface pressure IS the lowest interface's: sigma = 1 and the depth there a rounding of zero)
            assert abs(depth[0]) < 1e-12 and (np.diff(depth) > 0).all() and 5.0 < depth[-1] < 6.0
            assert "upwelling_longwave_flux_in_air_assuming_clear_sky" not in first_h
        else:
            assert float(first_h["precipitation_amount"].values.ravel()[0]) < 0.0      # it condenses from step 0 (the reference's sign)
    with pytest.raises(ValueError, match="exclusive"):
        ex.run(1, simple_physics=True, grid_scale_condensation=True)
    # the run without the flags is another run: RRTMG's longwave with its clear-sky stream, no optical depth, no precipitation
    first, plain = ex.run(3, device_resident=False)
    assert TAU not in plain and "precipitation_amount" not in plain and "upwelling_longwave_flux_in_air_assuming_clear_sky" in first
    assert maxdiff(plain["air_temperature"].values, runs["gray_longwave"]["air_temperature"].values) > 1e-6
