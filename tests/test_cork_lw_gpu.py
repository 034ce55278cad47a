"""The table-driven correlated-k longwave on the GPU: cork_band_kernel and cork_broadband_kernel against the numpy statement
(tests/cork_cases.py) on every case and shape under the tolerances stored in tests/golden/cork_<case>.npz (measured by the maker on
the reference itself: 16 x its largest deviation under +-1 ulp of every input, at least 1e-13, on the scale of X.deviations); what
must hold bit for bit -- the ascending band sum, both heating rates, +0.0 at the top, a block of columns alone, host against
device pointers, NULL optionals, read-only inputs, a repeated call, two resident tables; and the component on a host state and
on a DeviceState with the pressures resident in Pa and in mbar (the first DeviceAdamsBashforth step against t + dt * tend); and
examples/radiative_convective.py with cork_longwave in both modes.  The first test prints the largest deviation per field."""
import datetime
import importlib.util
import os
import types

import numpy as np
import pytest

import climt_amd
from climt_amd import _hip, cork, initialization
from climt_amd._sympl_compat import DataArray

from helpers import ROOT, maxdiff

import cork_cases as X

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def band_count():
    before = initialization._num_bands["longwave"]
    yield
    initialization._num_bands["longwave"] = before


@pytest.fixture(scope="module")
def ctx():
    from climt_amd.rrtmg.common import make_context
    return make_context(0)


@pytest.fixture(scope="module")
def handles(ctx):
    """Every fixture table resident at once on the module's context."""
    tables = {name: cork.KTable(X.table_path(name)) for name in X.TABLES}
    return {name: (kt, kt.upload(ctx)) for name, kt in tables.items()}


def constants(name):
    return dict(m_h2o=X.M_H2O, sigma_sb=X.SIGMA_SB, g=X.G, cpd=X.CPD, diffusivity=X.CASES[name][1])


def call(ctx, handles, name, c, **kw):
    kt, handle = handles[X.CASES[name][0]]
    gases = [c[g] for g in X.gas_names(name)]
    up, dn, tend, d = ctx.cork_longwave(handle, kt.nband, c["t"], c["p"], c["p_int"], c["tsfc"], c["emis"], constants(name), kt.gas_rule, gases=gases,
                                        gas_scale=kt.gas_scale, taucld=c["taucld"], **kw)
    return dict(up=up, dn=dn, tend=tend, **(d or {}))


def same(a, b, keys=None):
    return all(X.same_bits(a[k], b[k]) for k in (keys or a))


@pytest.mark.parametrize("name", list(X.BASE_CASES))
def test_kernels_equal_the_statement_on_every_shape(ctx, handles, name):
    worst, tol = {}, X.tolerances(name)
    for nlay in X.NLAYS:
        for ncol in X.NCOLS:
            c = X.cork_case(name, nlay, ncol)
            got = call(ctx, handles, name, c)
            dev = X.deviations(got, c)
            assert len(dev) == len(X.FIELDS)
            # exact, on every case and shape: the ascending band sum, the two heating rates, the top of the downward sweep
            up, dn = np.zeros_like(got["up"]), np.zeros_like(got["dn"])
            for b in range(got["up_band"].shape[0]):
                up += got["up_band"][b]
                dn += got["dn_band"][b]
            assert X.same_bits(up, got["up"]) and X.same_bits(dn, got["dn"]), (name, nlay, ncol)
            assert X.same_bits(got["hr"], got["tend"] * 86400.0)
            assert X.same_bits(got["hr_band"], np.stack([X.heating(u - d, c["p_int"]) * 86400.0 for u, d in zip(got["up_band"], got["dn_band"])]))
            assert X.same_bits(got["dn_band"][:, -1], np.zeros((got["dn_band"].shape[0], ncol)))
            for k, v in dev.items():
                worst[k] = max(worst.get(k, 0.0), v)
    print("cork_band_kernel, %s: largest deviation from the statement (tolerance) %s" % (name, ", ".join("%s %.2e (%.1e)" % (k, v, tol[k]) for k, v in sorted(worst.items()))))
    for k, v in worst.items():
        assert v <= tol[k], (name, k, v, tol[k])


@pytest.mark.parametrize("lo,hi,ncol", [(1, 2, 65), (37, 101, 130), (63, 130, 130)])
def test_a_block_of_columns_alone_equals_the_block_inside_the_whole(ctx, handles, lo, hi, ncol):
    for name in ("earth", "cloudy", "two_gas"):
        c = X.cork_case(name, 30, ncol)
        whole = call(ctx, handles, name, c)
        part = call(ctx, handles, name, {k: np.ascontiguousarray(v[..., lo:hi, :] if k == "taucld" else v[..., lo:hi]) for k, v in c.items() if k not in X.FIELDS})
        assert all(X.same_bits(part[f], whole[f][..., lo:hi]) for f in X.FIELDS), name


def test_host_pointers_equal_device_pointers_and_inputs_are_only_read(ctx, handles):
    for name in ("earth", "two_gas", "premixed"):
        kt, handle = handles[X.CASES[name][0]]
        c = X.cork_case(name, 30, 65)
        host = call(ctx, handles, name, c)
        names = ("t", "p", "p_int", "tsfc", "emis", "taucld") + tuple(X.gas_names(name))
        dev = {k: _hip.DeviceArray.from_host(np.ascontiguousarray(c[k])) for k in names}
        out = {f: _hip.DeviceArray(c[f].shape, np.float64) for f in X.FIELDS}
        ctx.cork_longwave(handle, kt.nband, dev["t"], dev["p"], dev["p_int"], dev["tsfc"], dev["emis"], constants(name), kt.gas_rule, gases=[dev[g] for g in X.gas_names(name)],
                          gas_scale=kt.gas_scale, taucld=dev["taucld"], up=out["up"], dn=out["dn"], tend=out["tend"],
                          diagnostics={f: out[f] for f in X.FIELDS[3:]}, memspace=1, ncol=65, nlay=30)
        ctx.synchronize()
        assert all(X.same_bits(out[f].download().reshape(c[f].shape), host[f]) for f in X.FIELDS), name
        assert all(X.same_bits(dev[k].download().reshape(c[k].shape), c[k]) for k in names), name
        again = call(ctx, handles, name, c)      # the same handle repeats its bits
        assert same(again, host)


def test_every_optional_output_null_in_turn_leaves_the_others_their_bits(ctx, handles):
    c = X.cork_case("cloudy", 30, 65)
    full = call(ctx, handles, "cloudy", c)
    optional = X.FIELDS[3:]
    for skip in optional + (None,):
        d = {f: np.empty(c[f].shape) for f in optional if f != skip} if skip else False
        got = call(ctx, handles, "cloudy", c, diagnostics=d)
        assert set(got) == set(X.FIELDS) - ({skip} if skip else set(optional)) and same(got, full, list(got)), skip


def test_refusals_come_before_anything_is_read(ctx, handles):
    from climt_amd._lib import RRTMGError
    c = X.cork_case("two_gas", 2, 4)
    kt, handle = handles["two_gas"]
    base = dict(gases=[c["h2o"], c["co2"]], gas_scale=kt.gas_scale, taucld=c["taucld"])
    args = (c["t"], c["p"], c["p_int"], c["tsfc"], c["emis"], constants("two_gas"), kt.gas_rule)
    with pytest.raises(RRTMGError, match="gas array is missing"):
        ctx.cork_longwave(handle, 2, *args, **dict(base, gases=[c["h2o"], None]))
    other = climt_amd.Context(0)
    with pytest.raises(RRTMGError, match="not one of this context"):
        other.cork_longwave(handle, 2, *args, **base)
    with pytest.raises(RRTMGError, match="gas_rule"):
        ctx.cork_longwave(handle, 2, *args[:-1], 3, **base)
    with pytest.raises(RRTMGError, match="overlaps|aliases"):
        up = np.empty((3, 4))
        ctx.cork_longwave(handle, 2, *args, up=up, dn=up, **base)
    with pytest.raises(RRTMGError, match="H2O axis needs gas_rule 1"):
        ctx.cork_longwave(handles["h2o_axis"][1], 4, c["t"], c["p"], c["p_int"], c["tsfc"], np.ones((4, 4)), constants("two_gas"), 2, gases=[c["h2o"]])
    with pytest.raises(RRTMGError, match="strictly increase"):
        ctx.cork_table_create(kt.k, kt.weights, kt.planck, kt.t_grid[::-1].copy(), kt.p_grid_log)
    extra = kt.upload(ctx)      # a further table comes and goes; the others stay what they were
    ctx.cork_table_destroy(extra)
    with pytest.raises(RRTMGError, match="not a table of this context"):
        ctx.cork_table_destroy(extra)
    assert same(call(ctx, handles, "two_gas", c), call(ctx, handles, "two_gas", c))


def test_radiative_convective_example_with_cork_longwave_in_both_modes():
    """Three steps of examples/radiative_convective.py with cork_longwave on a host state and on a DeviceState: the two modes to the
    tolerance of the example's own test (tests/test_dry_adjustment_gpu.py, 1e-9); exclusive with gray_longwave; the run without
    the flag is what it is with the flag left at None, bit for bit, and is RRTMG's."""
    spec = importlib.util.spec_from_file_location("radiative_convective", os.path.join(ROOT, "examples", "radiative_convective.py"))
    ex = importlib.util.module_from_spec(spec); spec.loader.exec_module(ex)
    table = X.table_path("earth4")
    names = ("air_temperature", "specific_humidity", "surface_temperature")
    extra = ("upwelling_longwave_flux_in_air", "downwelling_longwave_flux_in_air", "air_temperature_tendency_from_longwave",
             "upwelling_longwave_flux_in_air_per_band", "longwave_optical_depth_per_band", "air_temperature_tendency_from_longwave_per_band")
    first_h, end_h = ex.run(3, device_resident=False, cork_longwave=table)
    first_d, end_d = ex.run(3, device_resident=True, cork_longwave=table)
    close = lambda h, d: maxdiff(h.values, np.transpose(d.values, [d.dims.index(x) for x in h.dims])) <= 1e-9 * max(1.0, float(np.abs(h.values).max()))
    for n in extra:
        assert n in first_h and n in first_d and close(first_h[n], first_d[n]), n
    for n in names + extra:
        assert np.all(np.isfinite(end_h[n].values)) and close(end_h[n], end_d[n]), n
    assert "num_longwave_bands" in first_h["upwelling_longwave_flux_in_air_per_band"].dims and first_h["upwelling_longwave_flux_in_air_per_band"].values.size == 4 * 31
    assert "upwelling_longwave_flux_in_air_assuming_clear_sky" not in first_h      # RRTMG's longwave did not run
    olr = float(first_h["upwelling_longwave_flux_in_air"].values.ravel()[-1])
    assert 50.0 < olr < 500.0
    with pytest.raises(ValueError, match="exclusive"):
        ex.run(1, cork_longwave=table, gray_longwave=True)
    initialization._num_bands["longwave"] = None      # (what a process that never made the component has)
    plain_first, plain_end = ex.run(3)
    none_first, none_end = ex.run(3, cork_longwave=None)
    assert set(plain_end) == set(none_end) and all(X.same_bits(plain_end[n].values, none_end[n].values) for n in plain_end if n != "time")
    assert "upwelling_longwave_flux_in_air_assuming_clear_sky" in plain_first and "longwave_optical_depth_per_band" not in plain_first
    assert not X.same_bits(plain_end["air_temperature"].values, end_h["air_temperature"].values)


CASE_KEYS = {"T": "t", "p": "p", "p_int": "p_int", "T_surf": "tsfc", "emissivity": "emis", "tau_cloud_lw": "taucld"}      # alias -> the case's key; a gas: its alias


def state_of(comp, c):
    """A host state of the case `c` as the component states its inputs: names, dimensions and units are its input_properties."""
    s = {"time": datetime.datetime(2000, 1, 1)}
    for n, p in comp.input_properties.items():
        s[n] = DataArray(np.array(c[CASE_KEYS.get(p["alias"], p["alias"])]), dims=tuple("x" if d == "*" else d for d in p["dims"]), attrs={"units": p["units"]})
    return s


HOST_NAMES = {"up": "upwelling_longwave_flux_in_air", "dn": "downwelling_longwave_flux_in_air", "hr": "air_temperature_tendency_from_longwave",
              "up_band": "upwelling_longwave_flux_in_air_per_band", "dn_band": "downwelling_longwave_flux_in_air_per_band", "tau_band": "longwave_optical_depth_per_band",
              "trans_band": "longwave_transmittance_per_band", "hr_band": "air_temperature_tendency_from_longwave_per_band"}


@pytest.mark.parametrize("name", ["earth", "two_gas", "premixed", "cloudy"])
def test_component_on_a_host_state_and_on_a_device_state(ctx, handles, name):
    c = X.cork_case(name, 30, 65)
    direct = call(ctx, handles, name, c)
    comp = climt_amd.CorkLongwaveRadiation(optics="correlated_k", table=X.table_path(X.CASES[name][0]), diffusivity_factor=X.CASES[name][1], context=ctx)
    state = state_of(comp, c)
    tend, diag = comp(state)
    assert X.same_bits(tend["air_temperature"].values, direct["tend"]) and set(diag) == set(HOST_NAMES.values())
    for f, n in HOST_NAMES.items():
        v = diag[n].values
        assert X.same_bits(np.moveaxis(v, -1, 0) if f.endswith("_band") else v, direct[f]), (name, f)
        assert tuple(diag[n].dims)[-1 if f.endswith("_band") else 0] == ("num_longwave_bands" if f.endswith("_band") else diag[n].dims[0])
    for units, factor in (("Pa", 1.0), ("mbar", 0.01)):
        s = dict(state)
        for n in ("air_pressure", "air_pressure_on_interface_levels"):
            s[n] = DataArray(state[n].values * factor, dims=state[n].dims, attrs={"units": units})
        props = {n: dict(p, units=units) if n.startswith("air_pressure") else p for n, p in comp.input_properties.items()}
        with climt_amd.DeviceState.from_host(s, [types.SimpleNamespace(input_properties=props)], context=ctx) as ds:
            t_dev, d_dev = comp(ds)
            ctx.synchronize()
            got = dict(tend=t_dev["air_temperature"].buf.download().reshape(direct["tend"].shape),
                       **{f: d_dev[n].buf.download().reshape(direct[f].shape) for f, n in HOST_NAMES.items()})
            if factor == 1.0:
                assert same(got, direct), name
            else:      # p * 100 on the device against the host's Pa: one rounding of the pressures
                assert max(X.deviations(got, direct).values()) < 1e-9
                assert same(got, call(ctx, handles, name, dict(c, p=c["p"] * factor, p_int=c["p_int"] * factor), pressure_scale=100.0))
            stepper = climt_amd.DeviceAdamsBashforth(comp)      # the first Adams-Bashforth step is t + dt * tend of the tendency just checked
            stepper(ds, datetime.timedelta(minutes=10))
            ctx.synchronize()
            stepped = ds["air_temperature"].buf.download().reshape(c["t"].shape)
            euler = c["t"] + 600.0 * got["tend"]
            assert np.abs(stepped - euler).max() <= 2 * np.finfo(float).eps * np.abs(euler).max() and np.abs(stepped - c["t"]).max() > 1e-6, name
    if name == "earth":      # a state of another shape: four bands of emissivity and cloud depth under a table of two
        two = climt_amd.CorkLongwaveRadiation(optics="correlated_k", table=X.table_path("two_band"), context=ctx)
        with climt_amd.DeviceState.from_host(state, [comp], context=ctx) as ds:
            with pytest.raises(ValueError, match="do not belong to one grid"):
                two(ds)
