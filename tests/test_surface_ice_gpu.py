"""The snow/ice column on the GPU: surface_ice_kernel against the numpy statements (tests/surface_ice_cases.py) on every case x
NLAYS x NCOLS of both kinds, to the tolerances the maker measured on the reference (tests/golden/sea_ice_<case>.npz,
land_ice_<case>.npz); every optional pointer NULL in turn; host pointers, device pointers and in place; a block of columns alone;
neighbours; SeaIce and LandIce on a DeviceState against the host state; and examples/radiative_convective.py with sea_ice in both
modes.  Shapes no larger than (30, 130); every test takes a second or two.

Measured on an MI355X: every case x NLAYS x NCOLS of both kinds (264 host-pointer calls) bit-identical to the statements, largest
deviation 0 in every field, flags equal to the statements' decisions; the exact properties and the energy budget of
surface_ice_cases hold on the kernel's own output (interior residual at most 2.5 x 2^-52 of the rows' scale, asserted at 16); the file: 37 passed in 3.2 s (docs/EXPERIMENTS.md X).  The first
test prints the largest deviations and whether all were bit-identical."""
import datetime
import importlib.util
import os

import numpy as np
import pytest

import climt_amd
from climt_amd import _hip, _lib
from helpers import ROOT, maxdiff

import surface_ice_cases as X

host_state, _without_the_tall_column = X.host_state, X.without_the_tall_column

pytestmark = pytest.mark.gpu
OUT, DIAG = _lib.SURFACE_ICE_OUT, _lib.SURFACE_ICE_DIAG
ALL_CASES = [(kn, name) for kn, kind in X.KINDS.items() for name in X.CASES[kind]]


@pytest.fixture(scope="module")
def ctx():
    from climt_amd.rrtmg.common import make_context
    return make_context(0)


def call(ctx, kind, c, k=None, **kw):
    o, d = ctx.surface_ice(kind, c["t"], c["height"], c["thick"], c["snow"], c["base"], X.fluxes_of(c), c["area_type"], c["dt"], X.constants(kind) if k is None else k, **kw)
    return dict(o, **d)


def device_call(ctx, kind, c, in_place=False, diagnostics=DIAG):
    """Device pointers -> the outputs as host arrays."""
    n, ncol = c["t"].shape
    up = {k: _hip.DeviceArray.from_host(np.ascontiguousarray(c[k])) for k in X.INPUTS}
    shape = lambda name: (n, ncol) if name in ("t_out", "height_out") else (ncol,)
    outs = {name: _hip.DeviceArray(shape(name), np.float64) for name in OUT}
    if in_place:
        outs.update(t_out=up["t"], height_out=up["height"], thick_out=up["thick"], snow_out=up["snow"])
        if kind == 0:
            outs["base_flux_out"] = up["base"]
    diag = {name: _hip.DeviceArray((ncol,), np.int32 if name == "flags" else np.float64) for name in diagnostics}
    ctx.surface_ice(kind, up["t"].ptr, up["height"].ptr, up["thick"].ptr, up["snow"].ptr, up["base"].ptr, {k: up[k].ptr for k in X.FLUXES}, up["area_type"].ptr,
                    c["dt"], X.constants(kind), diagnostics={k: v.ptr for k, v in diag.items()}, memspace=1, ncol=ncol, nlay=n, **{k: v.ptr for k, v in outs.items()})
    ctx.synchronize()
    got = {k: v.download().reshape(shape(k)) for k, v in outs.items()}
    got.update({k: v.download().reshape(-1) for k, v in diag.items()})
    if not in_place:      # the inputs are only read
        assert all(X.same_bits(up[k].download().reshape(np.shape(c[k])), c[k]) for k in X.INPUTS)
    return got


@pytest.mark.parametrize("kind_name,name", ALL_CASES)
def test_kernel_equals_the_statement_on_every_shape(ctx, kind_name, name):
    kind, tol, worst, same, ratio = X.KINDS[kind_name], X.tolerances(kind_name, name), {}, True, 0.0
    for nlay in X.NLAYS:
        for ncol in X.NCOLS:
            c = X.ice_case(kind, name, nlay, ncol)
            got = call(ctx, kind, c)
            dev = X.deviations(got, c, X.FIELDS)
            worst = {f: max(worst.get(f, 0.0), v) for f, v in dev.items()}
            same = same and all(X.same_bits(got[f], c[f]) for f in X.FIELDS)
            assert X.same_bits(got["flags"], c["flags"]), (nlay, ncol)      # the decisions, exactly
            X.check_exact_properties(kind, name, c, got)      # on the kernel's own output: what no tolerance covers
            budget = X.energy_budget(kind, c, got)            # the interior rows' budget and the growth relation (asserted inside)
            ratio = max(ratio, budget["ratio"])
    print("%s %s: largest deviations %s; all bit-identical: %s; interior energy residual %.2f x 2^-52 of the rows' scale" % (
        kind_name, name, {f: "%.1e" % v for f, v in worst.items() if v}, same, ratio))
    assert X.within(worst, tol), (worst, tol)


@pytest.mark.parametrize("kind_name", list(X.KINDS))
def test_every_optional_pointer_null_in_turn_leaves_the_others_their_bits(ctx, kind_name):
    kind = X.KINDS[kind_name]
    c = X.ice_case(kind, "mixed_types", 10, 65)
    full = device_call(ctx, kind, c)
    for skip in DIAG + (None,):
        names = tuple(n for n in DIAG if n != skip) if skip else ()
        got = device_call(ctx, kind, c, diagnostics=names)
        assert all(X.same_bits(got[k], full[k]) for k in OUT + names), skip


@pytest.mark.parametrize("kind_name", list(X.KINDS))
def test_host_pointers_device_pointers_and_in_place_agree_bit_for_bit(ctx, kind_name):
    kind = X.KINDS[kind_name]
    for nlay, ncol in ((3, 1), (10, 64), (30, 65), (30, 130)):
        c = X.ice_case(kind, "mixed_types", nlay, ncol)
        host, dev, dev_in_place = call(ctx, kind, c), device_call(ctx, kind, c), device_call(ctx, kind, c, in_place=True)
        mine = {k: np.array(c[k]) for k in ("t", "height", "thick", "snow", "base")}
        host_in_place = call(ctx, kind, dict(c, **mine), t_out=mine["t"], height_out=mine["height"], thick_out=mine["thick"], snow_out=mine["snow"],
                             **(dict(base_flux_out=mine["base"]) if kind == 0 else {}))
        assert host_in_place["t_out"] is mine["t"] and host_in_place["thick_out"] is mine["thick"]
        for other in (dev, dev_in_place, host_in_place):
            assert all(X.same_bits(other[k], host[k]) for k in OUT + DIAG), (nlay, ncol)


@pytest.mark.parametrize("kind_name", list(X.KINDS))
def test_a_block_of_columns_alone_equals_the_block_inside_the_whole(ctx, kind_name):
    kind = X.KINDS[kind_name]
    c = X.ice_case(kind, "mixed_types", 30, 130)
    whole = call(ctx, kind, c)
    for lo, hi in ((1, 2), (37, 101), (63, 130), (5, 69)):
        part = {k: np.ascontiguousarray(c[k][..., lo:hi]) for k in X.INPUTS}
        got = call(ctx, kind, dict(part, dt=c["dt"]))
        assert all(X.same_bits(got[k], whole[k][..., lo:hi]) for k in OUT + DIAG), (lo, hi)


@pytest.mark.parametrize("kind_name", list(X.KINDS))
def test_one_column_among_others_does_not_disturb_its_neighbours(ctx, kind_name):
    """One melting column among cold ones, and one active column among inactive ones: every column has the bits it has alone with
    its like, and the flags are the statement's decisions."""
    kind = X.KINDS[kind_name]
    cold, melting = X.ice_case(kind, "cold", 10, 65), X.ice_case(kind, "melting", 10, 65)
    dt = min(cold["dt"], melting["dt"])
    mixed = {k: np.array(cold[k]) for k in X.INPUTS}
    for k in X.INPUTS:
        mixed[k][..., 33] = melting[k][..., 33]
    got = call(ctx, kind, dict(mixed, dt=dt))
    alone_cold, alone_melting = call(ctx, kind, dict(cold, dt=dt)), call(ctx, kind, dict(melting, dt=dt))
    keep = np.arange(65) != 33
    want = X.ice_statement(kind, *(mixed[k] for k in X.INPUTS), dt)
    assert X.same_bits(got["flags"], want["flags"]) and want["melting"].sum() == 1
    for k in OUT + DIAG:
        assert X.same_bits(got[k][..., keep], alone_cold[k][..., keep]) and X.same_bits(got[k][..., 33], alone_melting[k][..., 33]), k
    lone = {k: np.array(cold[k]) for k in X.INPUTS}
    lone["area_type"][:] = 2
    lone["area_type"][40] = cold["area_type"][40]
    got = call(ctx, kind, dict(lone, dt=cold["dt"]))
    alone = call(ctx, kind, cold)
    keep = np.arange(65) != 40
    assert (got["flags"][keep] == 0).all() and got["flags"][40] == 1
    assert all(X.same_bits(got[k][..., 40], alone[k][..., 40]) for k in OUT + DIAG)
    for k, src in (("t_out", "t"), ("height_out", "height"), ("thick_out", "thick"), ("snow_out", "snow")):
        assert X.same_bits(got[k][..., keep], lone[src][..., keep])
    zeros = np.zeros(64)
    assert X.same_bits(got["albedo"][keep], zeros) and X.same_bits(got["cond_flux"][keep], zeros)
    assert X.same_bits(got["base_flux_out"][keep], lone["base"][keep] if kind == 0 else zeros) and X.same_bits(got["tsfc_out"][keep], lone["t"][-1][keep])


# ---- the components on a DeviceState -------------------------------------------------------------------------------------------------
def _component(kind, ctx, **kw):
    return (climt_amd.SeaIce if kind == 0 else climt_amd.LandIce)(context=ctx, **kw)


def _download(ds, name, q, like):
    ds[name] = q
    d = ds.download(name)
    return np.transpose(d.values, [d.dims.index(x) for x in like.dims]), d


@pytest.mark.parametrize("kind_name", list(X.KINDS))
def test_components_on_a_device_state_equal_the_host_state_bit_for_bit(ctx, kind_name):
    """Dims and units included; the next step is bound to the other buffer set and the state's previous arrays stay what they were."""
    kind, ny, nx, n = X.KINDS[kind_name], 5, 13, 10
    c, _ = _without_the_tall_column(X.ice_case(kind, "mixed_types", n, ny * nx))
    comp, dt = _component(kind, ctx), datetime.timedelta(seconds=c["dt"])
    state = host_state(kind, c, ny, nx)
    diag_h, new_h = comp(state, dt)
    with climt_amd.DeviceState.from_host(state, [comp], context=ctx) as ds:
        before = ds["snow_and_ice_temperature"]
        diag_d, back = comp(ds, dt)
        assert back is ds and set(diag_d) == set(diag_h) and ds["snow_and_ice_temperature"] is not before
        first = ds["snow_and_ice_temperature"]
        for name, h in list(new_h.items()) + list(diag_h.items()):
            values, d = _download(ds, name, diag_d[name] if name in diag_d else ds[name], h)
            assert X.same_bits(values, h.values) and d.attrs["units"] == h.attrs["units"] and set(d.dims) == set(h.dims), name
        assert X.same_bits(before.buf.download().reshape(n, -1), c["t"])      # the previous array is what it was
        ds.step_count += 1
        comp(ds, dt)
        second = ds["snow_and_ice_temperature"]
        ds.step_count += 1
        comp(ds, dt)
        assert second is not first and ds["snow_and_ice_temperature"] is first      # two alternating buffer sets
        flags = comp.device_flags.buf.download().reshape(-1)
        assert ((flags & 1) != 0).any() and ((flags & 1) == 0).any()


def test_sea_ice_then_slab_surface_on_a_device_state_equals_the_host_pair(ctx):
    ny, nx, n = 5, 13, 10
    c, _ = _without_the_tall_column(X.ice_case(0, "mixed_types", n, ny * nx))
    ice, slab, dt = _component(0, ctx), climt_amd.SlabSurface(context=ctx), datetime.timedelta(seconds=c["dt"])
    state = climt_amd.get_default_state([ice, slab], grid_state=climt_amd.get_grid(nx=nx, ny=ny, nz=3))
    mine = host_state(0, c, ny, nx)
    for name, q in mine.items():
        if name != "time" and name in state and "interface_levels" not in q.dims:
            state[name] = q
    for name in ("downwelling_shortwave_flux_in_air", "downwelling_longwave_flux_in_air", "upwelling_shortwave_flux_in_air", "upwelling_longwave_flux_in_air"):
        d = state[name]
        d.values[...] = -5.0
        index = [slice(None)] * d.values.ndim
        index[d.dims.index("interface_levels")] = 0
        d.values[tuple(index)] = np.transpose(mine[name].values[..., 0].reshape(ny, nx), [("lat", "lon").index(x) for x in d.dims if x != "interface_levels"])
    diag_h, new_h = ice(state, dt)
    host = dict(state)
    host.update(diag_h); host.update(new_h)
    tend_h, slab_h = slab(host)
    with climt_amd.DeviceState.from_host(state, [ice, slab], context=ctx) as ds:
        diag_d, _ = ice(ds, dt)
        ds.update(diag_d)
        tend_d, slab_d = slab(ds)
        for name, h in (("surface_temperature", tend_h["surface_temperature"]), ("depth_of_slab_surface", slab_h["depth_of_slab_surface"])):
            values, _ = _download(ds, "check_" + name, tend_d[name] if name in tend_d else slab_d[name], h)
            assert X.same_bits(values, h.values), name
        assert np.isfinite(tend_h["surface_temperature"].values).all()


@pytest.mark.parametrize("kind_name", list(X.KINDS))
def test_check_maximum_height_on_a_device_state(ctx, kind_name):
    kind, ny, nx = X.KINDS[kind_name], 5, 13
    c = X.ice_case(kind, "mixed_types", 3, ny * nx)
    tall = c["too_tall"] == 1
    assert tall.sum() == 1
    comp, dt = _component(kind, ctx), datetime.timedelta(seconds=c["dt"])
    state = host_state(kind, c, ny, nx)
    with climt_amd.DeviceState.from_host(state, [comp], context=ctx) as ds:
        with pytest.raises(ValueError, match=r"^Total height exceeds maximum value of 10 m\.$"):
            comp(ds, dt)
        with pytest.raises(ValueError, match=r"^Total height exceeds maximum value of 10 m\.$"):
            comp(ds, dt, check_maximum_height=True)
        comp(ds, dt, check_maximum_height=False)      # nothing is downloaded; the column is left as it was and flagged
        flags = comp.device_flags.buf.download().reshape(-1)
        assert X.same_bits(flags, c["flags"]) and (flags[tall] == 4).all()
        assert X.same_bits(ds["snow_and_ice_temperature"].buf.download().reshape(3, -1), c["t_out"])


def test_device_calls_refuse_a_state_of_another_shape(ctx):
    ny, nx, n = 5, 13, 10
    c, _ = _without_the_tall_column(X.ice_case(0, "mixed_types", n, ny * nx))
    comp, dt = _component(0, ctx), datetime.timedelta(seconds=60)
    with climt_amd.DeviceState.from_host(host_state(0, c, ny, nx), [comp], context=ctx) as ds:
        good = dict(ds)
        q = ds["snow_and_ice_temperature"]
        ds["snow_and_ice_temperature"] = climt_amd.device_state.DeviceQuantity(q.buf, (ny * nx, n), ("*", "ice_interface_levels"), q.units)
        with pytest.raises(ValueError, match="is resident as"):
            comp(ds, dt)
        ds.update(good)
        h = ds["height_on_ice_interface_levels"]
        ds["height_on_ice_interface_levels"] = climt_amd.device_state.DeviceQuantity(h.buf, (n - 1, ny * nx), h.dims, h.units)
        with pytest.raises(ValueError, match="do not belong to one grid"):
            comp(ds, dt)
        ds.update(good)
        f = ds["downwelling_longwave_flux_in_air"]
        ds["downwelling_longwave_flux_in_air"] = climt_amd.device_state.DeviceQuantity(f.buf, (ny * nx, 2), ("*", "interface_levels"), f.units)
        with pytest.raises(ValueError, match=r"must be resident as \[interface_levels\]\[\*\]"):
            comp(ds, dt)
        ds.update(good)
        del ds["area_type"]
        with pytest.raises(KeyError, match="area_type"):
            comp(ds, dt)


# ---- the example -----------------------------------------------------------------------------------------------------------------------
def test_radiative_convective_example_with_sea_ice_in_both_modes():
    """Three steps of examples/radiative_convective.py with sea_ice on a host state and on a DeviceState: the two modes to the
    tolerance of the example's own test (tests/test_dry_adjustment_gpu.py, 1e-9); the run without the flag is unchanged."""
    spec = importlib.util.spec_from_file_location("radiative_convective", os.path.join(ROOT, "examples", "radiative_convective.py"))
    ex = importlib.util.module_from_spec(spec); spec.loader.exec_module(ex)
    names = ("air_temperature", "surface_temperature", "snow_and_ice_temperature", "sea_ice_thickness", "surface_snow_thickness", "height_on_ice_interface_levels")
    extra = ("heat_flux_into_sea_water_due_to_sea_ice", "surface_downward_heat_flux_in_sea_ice", "surface_albedo_for_direct_shortwave")
    first_h, end_h = ex.run(3, device_resident=False, sea_ice=True)
    first_d, end_d = ex.run(3, device_resident=True, sea_ice=True)
    for n in extra:
        h, d = first_h[n], first_d[n]
        assert maxdiff(h.values.ravel(), np.transpose(d.values, [d.dims.index(x) for x in h.dims]).ravel()) <= 1e-9 * max(1.0, float(np.abs(h.values).max())), n
    for n in names + extra:
        h, d = end_h[n], end_d[n]
        gd = np.transpose(d.values, [d.dims.index(x) for x in h.dims])
        assert np.all(np.isfinite(h.values)) and maxdiff(h.values, gd) <= 1e-9 * max(1.0, float(np.abs(h.values).max())), (n, maxdiff(h.values, gd))
    assert float(first_h["surface_albedo_for_direct_shortwave"].values.ravel()[0]) == 0.8      # snow on top, not melting at step 0
    assert float(end_h["surface_albedo_for_direct_shortwave"].values.ravel()[0]) in (0.8, 0.2)  # (the surface warms under a 300 K atmosphere)
    assert abs(float(end_h["sea_ice_thickness"].values.ravel()[0]) - 2.0) < 1e-2
    first, plain = ex.run(3, device_resident=False)
    assert "surface_downward_heat_flux_in_sea_ice" not in plain and float(plain["surface_temperature"].values.ravel()[0]) > 290.0
    assert maxdiff(plain["air_temperature"].values, end_h["air_temperature"].values) > 1e-6
