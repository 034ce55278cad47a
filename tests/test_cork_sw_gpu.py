"""The table-driven correlated-k two-stream shortwave on the GPU: cork_sw_band_kernel and the band reduction against the numpy
statement (tests/cork_sw_cases.py) on every case and shape under the tolerances stored in tests/golden/cork_sw_<case>.npz; what must
hold bit for bit -- the ascending band sum, both heating rates, the night zeros, a block of columns alone, chunked against
unchunked (whole waves, partial waves, single columns), host against device pointers, NULL optionals with and without dark columns,
a call after calls of other shapes, read-only inputs, float against double shape tables, a longwave and a shortwave table resident
together; pressures in mbar against the statement's own pressure_scale; every ABI refusal; and the component on a host state.  The first test prints the largest
deviation per field."""
import datetime

import numpy as np
import pytest

import climt_amd
from climt_amd import _hip, cork, initialization
from climt_amd._sympl_compat import DataArray

import cork_cases as L
import cork_sw_cases as S

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def band_count():
    before = dict(initialization._num_bands)
    yield
    initialization._num_bands.update(before)


@pytest.fixture(scope="module")
def ctx():
    from climt_amd.rrtmg.common import make_context
    return make_context(0)


@pytest.fixture(scope="module")
def handles(ctx):
    """Every fixture table resident at once on the module's context; a shape table also with k cast to double ("<name>:f64")."""
    out = {}
    for name in S.TABLES:
        kt = cork.KTable(S.table_path(name), kind="shortwave")
        out[name] = (kt, kt.upload(ctx))
        if name in S.SHAPE_TABLES:
            kd = cork.KTable(S.table_path(name), kind="shortwave")
            kd.k = kd.k.astype(np.float64)
            out[name + ":f64"] = (kd, kd.upload(ctx))
    return out


CONSTANTS = dict(m_h2o=S.M_H2O, g=S.G, cpd=S.CPD)


def call(ctx, handles, name, c, table=None, **kw):
    kt, handle = handles[table or S.CASES[name]]
    cloud = kw.pop("cloud", tuple(c[n] for n in S.CLOUD))
    up, dn, tend, d = ctx.cork_shortwave(handle, kt.nband, c["t"], c["p"], c["p_int"], c["zenith"], c["albedo"], c["earth_sun"], CONSTANTS, kt.gas_rule,
                                         gases=[c[g] for g in S.gas_names(name)], gas_scale=kt.gas_scale, cloud=cloud, **kw)
    return dict(up=up, dn=dn, tend=tend, **(d or {}))


def same(a, b, keys=None):
    return all(S.same_bits(a[k], b[k]) for k in (keys or a))


@pytest.mark.parametrize("name", list(S.CASES))
def test_kernels_equal_the_statement_on_every_shape(ctx, handles, name):
    worst, tol = {}, S.tolerances(name)
    for nlay in S.NLAYS:
        for ncol in S.NCOLS:
            c = S.cork_sw_case(name, nlay, ncol)
            got = call(ctx, handles, name, c)
            dev = S.deviations(got, c, S.FIELDS)
            assert len(dev) == len(S.FIELDS)
            up, dn = np.zeros_like(got["up"]), np.zeros_like(got["dn"])
            for b in range(got["up_band"].shape[0]):
                up += got["up_band"][b]
                dn += got["dn_band"][b]
            assert S.same_bits(up, got["up"]) and S.same_bits(dn, got["dn"]), (name, nlay, ncol)
            assert S.same_bits(got["hr"], got["tend"] * 86400.0)
            assert S.same_bits(got["hr_band"], np.stack([L.heating(u - d, c["p_int"]) * 86400.0 for u, d in zip(got["up_band"], got["dn_band"])]))
            dark = np.cos(c["zenith"]) <= S.NIGHT
            for f in ("up", "dn", "up_band", "dn_band"):      # +0.0, bit for bit; the heating of zeros is the statement's, sign included
                assert S.same_bits(got[f][..., dark], np.zeros_like(got[f][..., dark])), (name, f)
            for f in ("tend", "hr", "hr_band"):
                assert S.same_bits(got[f][..., dark], c[f][..., dark]), (name, f)
            if S.CASES[name] in S.SHAPE_TABLES:      # the double instantiation on the same float32-exact values: the same bits
                assert same(call(ctx, handles, name, c, table=S.CASES[name] + ":f64"), got), (name, nlay, ncol)
            for k, v in dev.items():
                worst[k] = max(worst.get(k, 0.0), v)
    print("cork_sw_band_kernel, %s: largest deviation from the statement (tolerance) %s" % (name, ", ".join("%s %.2e (%.1e)" % (k, v, tol[k]) for k, v in sorted(worst.items()))))
    for k, v in worst.items():
        assert v <= tol[k], (name, k, v, tol[k])


def part_of(c, lo, hi):
    return {k: np.ascontiguousarray(v[..., lo:hi, :] if k in S.CLOUD else v[..., lo:hi]) for k, v in c.items() if k not in S.FIELDS}


@pytest.mark.parametrize("lo,hi,ncol", [(1, 2, 65), (37, 101, 130), (63, 130, 130)])
def test_a_block_of_columns_alone_equals_the_block_inside_the_whole(ctx, handles, lo, hi, ncol):
    for name in ("clear", "night", "cloudy", "overcast"):      # (uniform earth_sun: the first column's factor is the block's too)
        c = S.cork_sw_case(name, 30, ncol)
        whole, part = call(ctx, handles, name, c), call(ctx, handles, name, part_of(c, lo, hi))
        assert all(S.same_bits(part[f], whole[f][..., lo:hi]) for f in S.FIELDS), name


def test_chunks_of_64_columns_equal_the_unchunked_call(ctx, handles):
    """Whole waves (64), single columns (1), and chunks that end in a partial wave: 7 (19 chunks, the last of 4 columns) and 65 (two
    chunks that each end in a wave of one thread)."""
    for name in ("night", "cloudy", "g16", "overcast", "overcast_g9_cont"):
        c = S.cork_sw_case(name, 30, 130)
        whole = call(ctx, handles, name, c)
        for chunk in (64, 1, 7, 65):
            assert same(call(ctx, handles, name, c, max_chunk_cols=chunk), whole), (name, chunk)


@pytest.mark.parametrize("chunk", [0, 7])
def test_a_call_reads_nothing_that_calls_of_other_shapes_left_in_the_work_space(ctx, handles, chunk):
    """overcast, then cloudy on the same grid, then one column of one layer, then overcast again: a dark column or a chunk's tail
    that read rows of the work space another call wrote would differ."""
    c = S.cork_sw_case("overcast", 30, 130)
    first = call(ctx, handles, "overcast", c, max_chunk_cols=chunk)
    call(ctx, handles, "cloudy", S.cork_sw_case("cloudy", 30, 130), max_chunk_cols=chunk)
    call(ctx, handles, "clear", S.cork_sw_case("clear", 1, 1), max_chunk_cols=chunk)
    assert same(call(ctx, handles, "overcast", c, max_chunk_cols=chunk), first)
    tol = S.tolerances("overcast")
    assert all(v <= tol[f] for f, v in S.deviations(first, c, S.FIELDS).items())


def test_first_column_factor_scales_every_column(ctx, handles):
    c = S.cork_sw_case("first_column_factor", 30, 65)
    uniform = dict(c, earth_sun=np.full(65, c["earth_sun"][0]))
    assert same(call(ctx, handles, "first_column_factor", c), call(ctx, handles, "first_column_factor", uniform))


def test_host_pointers_equal_device_pointers_and_inputs_are_only_read(ctx, handles):
    for name in ("night", "cloudy", "albedo"):
        kt, handle = handles[S.CASES[name]]
        c = S.cork_sw_case(name, 30, 65)
        host = call(ctx, handles, name, c)
        names = S.INPUTS + tuple(S.gas_names(name))
        dev = {k: _hip.DeviceArray.from_host(np.ascontiguousarray(c[k])) for k in names}
        out = {f: _hip.DeviceArray(c[f].shape, np.float64) for f in S.FIELDS}
        ctx.cork_shortwave(handle, kt.nband, dev["t"], dev["p"], dev["p_int"], dev["zenith"], dev["albedo"], dev["earth_sun"], CONSTANTS, kt.gas_rule,
                           gases=[dev[g] for g in S.gas_names(name)], gas_scale=kt.gas_scale, cloud=tuple(dev[n] for n in S.CLOUD), up=out["up"], dn=out["dn"],
                           tend=out["tend"], diagnostics={f: out[f] for f in S.FIELDS[3:]}, memspace=1, ncol=65, nlay=30)
        ctx.synchronize()
        assert all(S.same_bits(out[f].download().reshape(c[f].shape), host[f]) for f in S.FIELDS), name
        assert all(S.same_bits(dev[k].download().reshape(c[k].shape), c[k]) for k in names), name
        assert same(call(ctx, handles, name, c), host)


def test_every_optional_output_null_in_turn_leaves_the_others_their_bits(ctx, handles):
    c = S.cork_sw_case("cloudy", 30, 65)
    full = call(ctx, handles, "cloudy", c)
    optional = S.FIELDS[3:]
    for skip in optional + (None,):
        d = {f: np.empty(c[f].shape) for f in optional if f != skip} if skip else False
        got = call(ctx, handles, "cloudy", c, diagnostics=d)
        assert set(got) == set(S.FIELDS) - ({skip} if skip else set(optional)) and same(got, full, list(got)), skip
    zeros = call(ctx, handles, "clear", S.cork_sw_case("clear", 30, 65))      # no cloud arrays: the zeros the reference mixes in
    assert same(call(ctx, handles, "clear", S.cork_sw_case("clear", 30, 65), cloud=None), zeros)


@pytest.mark.parametrize("nlay", [30, 1])
def test_every_optional_output_null_in_turn_over_dark_columns(ctx, handles, nlay):
    """`overcast` has dark columns, from two layers on with cloud in them: with tau_band NULL their beam pass ends at its first
    layer, with hr_band NULL the night block writes the flux zeros alone, with up_band or dn_band NULL those zeros go to the entry's
    own buffers."""
    c = S.cork_sw_case("overcast", nlay, 65)
    dark = np.cos(c["zenith"]) <= S.NIGHT
    assert dark.sum() == 26 and (nlay == 1 or (c["taucld"][:, dark] > 0).any())
    full = call(ctx, handles, "overcast", c)
    optional = S.FIELDS[3:]
    for skip in optional + (None,):
        d = {f: np.empty(c[f].shape) for f in optional if f != skip} if skip else False
        got = call(ctx, handles, "overcast", c, diagnostics=d)
        assert set(got) == set(S.FIELDS) - ({skip} if skip else set(optional)) and same(got, full, list(got)), skip
        for f in ("up", "dn"):
            assert S.same_bits(got[f][:, dark], np.zeros_like(got[f][:, dark])), (skip, f)
        assert S.same_bits(got["tend"][:, dark], c["tend"][:, dark]) and np.signbit(got["tend"][:, dark]).all(), skip


@pytest.mark.parametrize("name", ["overcast", "overcast_two_gas"])
def test_pressures_in_mbar_equal_the_statement_with_its_own_pressure_scale(ctx, handles, name):
    """p and p_int times 0.01 with pressure_scale 100 on both sides: Rayleigh's dp, the log-pressure bracket and both heating rates
    go through the scale.  The statement under the case's stored tolerances, the identities bit for bit."""
    c = S.cork_sw_case(name, 30, 65)
    mbar = dict({k: c[k] for k in S.INPUTS + tuple(S.gas_names(name))}, p=c["p"] * 0.01, p_int=c["p_int"] * 0.01)
    want = S.statement(S.table(S.CASES[name]), mbar, pressure_scale=100.0)
    got = call(ctx, handles, name, mbar, pressure_scale=100.0)
    dev, tol = S.deviations(got, want, S.FIELDS), S.tolerances(name)
    print("cork_sw_band_kernel, %s in mbar: largest deviation from the statement (tolerance) %s" % (name, ", ".join("%s %.2e (%.1e)" % (k, v, tol[k]) for k, v in sorted(dev.items()))))
    assert len(dev) == len(S.FIELDS)
    up, dn = np.zeros_like(got["up"]), np.zeros_like(got["dn"])
    for b in range(got["up_band"].shape[0]):
        up += got["up_band"][b]
        dn += got["dn_band"][b]
    assert S.same_bits(up, got["up"]) and S.same_bits(dn, got["dn"])
    assert S.same_bits(got["hr"], got["tend"] * 86400.0)
    assert S.same_bits(got["hr_band"], np.stack([L.heating(u - d, mbar["p_int"] * 100.0) * 86400.0 for u, d in zip(got["up_band"], got["dn_band"])]))
    dark = np.cos(c["zenith"]) <= S.NIGHT
    assert dark.any()
    for f in ("up", "dn", "up_band", "dn_band"):
        assert S.same_bits(got[f][..., dark], np.zeros_like(got[f][..., dark])), (name, f)
    for f in ("tend", "hr", "hr_band"):
        assert S.same_bits(got[f][..., dark], want[f][..., dark]), (name, f)
    for k, v in dev.items():
        assert v <= tol[k], (name, k, v, tol[k])


def test_refusals_come_before_anything_is_read(ctx, handles):
    from climt_amd._lib import RRTMGError
    c = S.cork_sw_case("albedo", 2, 4)
    kt, handle = handles["sw_two_gas"]
    args = (c["t"], c["p"], c["p_int"], c["zenith"], c["albedo"], c["earth_sun"], CONSTANTS, kt.gas_rule)
    base = dict(gases=[c["h2o"], c["co2"]], gas_scale=kt.gas_scale)
    with pytest.raises(RRTMGError, match="gas array is missing"):
        ctx.cork_shortwave(handle, 2, *args, **dict(base, gases=[c["h2o"], None]))
    with pytest.raises(RRTMGError, match="not one of this context"):
        climt_amd.Context(0).cork_shortwave(handle, 2, *args, **base)
    with pytest.raises(RRTMGError, match="gas_rule"):
        ctx.cork_shortwave(handle, 2, *args[:-1], 3, **base)
    with pytest.raises(RRTMGError, match="overlaps|aliases"):
        up = np.empty((3, 4))
        ctx.cork_shortwave(handle, 2, *args, up=up, dn=up, **base)
    with pytest.raises(RRTMGError, match="together or not at all"):
        ctx.cork_shortwave(handle, 2, *args, cloud=(c["taucld"], None, c["asycld"]), **base)
    with pytest.raises(RRTMGError, match="max_chunk_cols"):
        ctx.cork_shortwave(handle, 2, *args, max_chunk_cols=-1, **base)
    with pytest.raises(RRTMGError, match="H2O axis needs gas_rule 1"):
        ctx.cork_shortwave(handles["sw_earth"][1], 3, *args[:-1], 2, gases=[c["h2o"]])
    # a longwave table and a shortwave table resident together, each refused by the other's call
    lw = cork.KTable(L.table_path("two_band"))
    lw_handle = lw.upload(ctx)
    with pytest.raises(RRTMGError, match="is a longwave table"):
        ctx.cork_shortwave(lw_handle, 2, *args, **base)
    lc = L.cork_case("two_band", 2, 4)
    lw_args = (2, lc["t"], lc["p"], lc["p_int"], lc["tsfc"], lc["emis"], dict(m_h2o=L.M_H2O, sigma_sb=L.SIGMA_SB, g=L.G, cpd=L.CPD, diffusivity=1.66), lw.gas_rule)
    with pytest.raises(RRTMGError, match="is a shortwave table"):
        ctx.cork_longwave(handles["sw_two_band"][1], *lw_args, gases=[lc["h2o"]], gas_scale=lw.gas_scale)
    up, dn, tend, _ = ctx.cork_longwave(lw_handle, *lw_args, gases=[lc["h2o"]], gas_scale=lw.gas_scale)
    assert S.same_bits(up, np.asarray(up)) and max(L.deviations(dict(up=up, dn=dn, tend=tend), lc, ("up", "dn", "tend")).values()) <= max(L.tolerances("two_band").values())
    assert same(call(ctx, handles, "albedo", c), call(ctx, handles, "albedo", c))
    # the table's own refusals
    with pytest.raises(RRTMGError, match="strictly increase"):
        ctx.cork_sw_table_create(kt.k, kt.weights, kt.solar_source, kt.t_grid[::-1].copy(), kt.p_grid_log)
    with pytest.raises(ValueError, match="rank 7"):
        ctx.cork_sw_table_create(np.ones((1, 2, 2, 5, 5, 2, 2)), kt.weights, kt.solar_source, kt.t_grid, kt.p_grid_log)
    ctx.cork_table_destroy(lw_handle)
    extra = kt.upload(ctx)      # a further shortwave table comes and goes through the one destroy
    ctx.cork_table_destroy(extra)
    with pytest.raises(RRTMGError, match="not a table of this context"):
        ctx.cork_table_destroy(extra)


CASE_KEYS = {"T": "t", "p": "p", "p_int": "p_int", "zenith": "zenith", "albedo": "albedo", "earth_sun_factor": "earth_sun", "tau_cloud_sw": "taucld", "ssa_cloud": "ssacld",
             "g_cloud": "asycld"}
HOST_NAMES = {"up": "upwelling_shortwave_flux_in_air", "dn": "downwelling_shortwave_flux_in_air", "hr": "air_temperature_tendency_from_shortwave",
              "up_band": "upwelling_shortwave_flux_in_air_per_band", "dn_band": "downwelling_shortwave_flux_in_air_per_band", "tau_band": "shortwave_optical_depth_per_band",
              "hr_band": "air_temperature_tendency_from_shortwave_per_band"}


@pytest.mark.parametrize("name", ["night", "cloudy", "albedo", "first_column_factor"])
def test_component_on_a_host_state_equals_the_direct_call(ctx, handles, name):
    c = S.cork_sw_case(name, 30, 65)
    direct = call(ctx, handles, name, c)
    comp = climt_amd.CorkShortwaveRadiation(optics="correlated_k", table=S.table_path(S.CASES[name]), context=ctx)
    state = {"time": datetime.datetime(2000, 1, 1)}
    for n, p in comp.input_properties.items():
        value = c["t"][0] if p["alias"] == "T_surf" else c[CASE_KEYS.get(p["alias"], p["alias"])]
        state[n] = DataArray(np.array(value), dims=tuple("x" if d == "*" else d for d in p["dims"]), attrs={"units": p["units"]})
    tend, diag = comp(state)
    assert S.same_bits(tend["air_temperature"].values, direct["tend"]) and set(diag) == set(HOST_NAMES.values())
    for f, n in HOST_NAMES.items():
        v = diag[n].values
        assert S.same_bits(np.moveaxis(v, -1, 0) if f.endswith("_band") else v, direct[f]), (name, f)


@pytest.mark.parametrize("name", ["night", "cloudy", "albedo"])
def test_component_on_a_device_state_in_pa_and_in_mbar(ctx, handles, name):
    """The state resident in HBM: bit-equal to the direct call with the pressures in Pa; in mbar the library multiplies by 100 on the
    device -- one rounding of the pressures against the host's Pa, and the bits of the direct call on those arrays."""
    import types
    c = S.cork_sw_case(name, 30, 65)
    direct = call(ctx, handles, name, c)
    comp = climt_amd.CorkShortwaveRadiation(optics="correlated_k", table=S.table_path(S.CASES[name]), context=ctx)
    state = {"time": datetime.datetime(2000, 1, 1)}
    for n, p in comp.input_properties.items():
        value = c["t"][0] if p["alias"] == "T_surf" else c[CASE_KEYS.get(p["alias"], p["alias"])]
        state[n] = DataArray(np.array(value), dims=tuple("x" if d == "*" else d for d in p["dims"]), attrs={"units": p["units"]})
    for units, factor in (("Pa", 1.0), ("mbar", 0.01)):
        s = dict(state)
        for n in ("air_pressure", "air_pressure_on_interface_levels"):
            s[n] = DataArray(state[n].values * factor, dims=state[n].dims, attrs={"units": units})
        props = {n: dict(p, units=units) if n.startswith("air_pressure") else p for n, p in comp.input_properties.items()}
        with climt_amd.DeviceState.from_host(s, [types.SimpleNamespace(input_properties=props)], context=ctx) as ds:
            for repeat in range(2):      # the two alternating sets of work buffers
                t_dev, d_dev = comp(ds)
                ctx.synchronize()
                got = dict(tend=t_dev["air_temperature"].buf.download().reshape(direct["tend"].shape),
                           **{f: d_dev[n].buf.download().reshape(direct[f].shape) for f, n in HOST_NAMES.items()})
                assert tuple(d_dev[HOST_NAMES["up_band"]].dims)[0] == "num_shortwave_bands"
                if factor == 1.0:
                    assert same(got, direct), (name, repeat)
                else:
                    assert max(S.deviations(got, direct, S.FIELDS).values()) < 1e-9
                    assert same(got, call(ctx, handles, name, dict(c, p=c["p"] * factor, p_int=c["p_int"] * factor), pressure_scale=100.0)), (name, repeat)


def test_radiative_convective_example_with_cork_shortwave_in_both_modes():
    """Three steps of examples/radiative_convective.py with cork_shortwave on a host state and on a DeviceState: the two modes to the
    tolerance of the example's own tests (1e-9); the run without the flag is what it is with the flag left at None, bit for bit,
    and is RRTMG's."""
    import importlib.util
    import os
    from helpers import ROOT, maxdiff
    spec = importlib.util.spec_from_file_location("radiative_convective", os.path.join(ROOT, "examples", "radiative_convective.py"))
    ex = importlib.util.module_from_spec(spec); spec.loader.exec_module(ex)
    table = S.table_path("sw_earth")
    names = ("air_temperature", "specific_humidity", "surface_temperature")
    extra = ("upwelling_shortwave_flux_in_air", "downwelling_shortwave_flux_in_air", "air_temperature_tendency_from_shortwave",
             "upwelling_shortwave_flux_in_air_per_band", "shortwave_optical_depth_per_band", "air_temperature_tendency_from_shortwave_per_band")
    first_h, end_h = ex.run(3, device_resident=False, cork_shortwave=table)
    first_d, end_d = ex.run(3, device_resident=True, cork_shortwave=table)
    close = lambda h, d: maxdiff(h.values, np.transpose(d.values, [d.dims.index(x) for x in h.dims])) <= 1e-9 * max(1.0, float(np.abs(h.values).max()))
    for n in extra:
        assert n in first_h and n in first_d and close(first_h[n], first_d[n]), n
    for n in names + extra:
        assert np.all(np.isfinite(end_h[n].values)) and close(end_h[n], end_d[n]), n
    assert "num_shortwave_bands" in first_h["upwelling_shortwave_flux_in_air_per_band"].dims and first_h["upwelling_shortwave_flux_in_air_per_band"].values.size == 3 * 31
    assert "upwelling_shortwave_flux_in_air_assuming_clear_sky" not in first_h      # RRTMG's shortwave did not run
    toa = float(first_h["downwelling_shortwave_flux_in_air"].values.ravel()[-1])
    assert 100.0 < toa < 1500.0
    initialization._num_bands["shortwave"] = None      # (what a process that never made the component has)
    plain_first, plain_end = ex.run(3)
    none_first, none_end = ex.run(3, cork_shortwave=None)
    assert set(plain_end) == set(none_end) and all(S.same_bits(plain_end[n].values, none_end[n].values) for n in plain_end if n != "time")
    assert "upwelling_shortwave_flux_in_air_assuming_clear_sky" in plain_first and "shortwave_optical_depth_per_band" not in plain_first
    assert not S.same_bits(plain_end["air_temperature"].values, end_h["air_temperature"].values)
