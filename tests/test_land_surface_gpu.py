"""The land surface on the GPU: bucket_hydrology_kernel and second_best_kernel against the numpy statements
(tests/land_surface_cases.py) on every case x shape through Context.* with host pointers -- the Bucket bit for bit (its rule has
no libm call but sqrt), SecondBEST to the tolerances the maker measured on the reference (tests/golden/second_best_<case>.npz)
with the decisions (flags) exactly; and on one representative case per entry: device pointers, in place, every optional pointer
NULL in turn, a column alone against the column inside 130, and the component on a DeviceState against the component on the host
state with nothing uploaded or downloaded by the call.  Shapes no larger than (12, 130); every test takes a second or two.  The
first SecondBEST test prints the largest deviations and how many runs were bit-identical."""
import datetime

import numpy as np
import pytest

import climt_amd
from climt_amd import _hip, _lib
from helpers import ROOT  # noqa: F401

import land_surface_cases as X

pytestmark = pytest.mark.gpu
B_IN, B_OUT, B_DIAG = _lib.BUCKET_HYDROLOGY_IN, _lib.BUCKET_HYDROLOGY_OUT, _lib.BUCKET_HYDROLOGY_DIAG
S_IN, S_OUT, S_DIAG = _lib.SECOND_BEST_IN, _lib.SECOND_BEST_OUT, _lib.SECOND_BEST_DIAG
DEEP = ("deep_moisture", "deep_temperature", "deep_moisture_out", "deep_temperature_out", "runoff", "deep_fraction")
SOIL_OUT = ("t_soil_out", "x_w_out", "x_i_out")


@pytest.fixture(scope="module")
def ctx():
    from climt_amd.rrtmg.common import make_context
    return make_context(0)


def bucket_call(ctx, c, **kw):
    o, d = ctx.bucket_hydrology(c["layers"], {n: c[n] for n in B_IN if n in c}, c["dt"], c["scalars"], **kw)
    return dict(o, **d)


def best_call(ctx, c, name="", **kw):
    o, d = ctx.second_best({n: c[n] for n in S_IN}, c["dt"], X.best_constants(name), **kw)
    return dict(o, **d)


def bucket_device_call(ctx, c, in_place=False, diagnostics=None):
    """Device pointers -> the outputs as host arrays."""
    ncol, deep = c["ts"].shape[0], c["layers"] == 2
    diagnostics = tuple(n for n in B_DIAG if deep or n not in DEEP) if diagnostics is None else diagnostics
    up = {n: _hip.DeviceArray.from_host(np.ascontiguousarray(c[n])) for n in B_IN if n in c}
    outs = {n: (up[n[:-4]] if in_place else _hip.DeviceArray((ncol,), np.float64)) for n in B_OUT if deep or n not in DEEP}
    diag = {n: _hip.DeviceArray((ncol,), np.float64) for n in diagnostics}
    ctx.bucket_hydrology(c["layers"], {n: x.ptr for n, x in up.items()}, c["dt"], c["scalars"], outs={n: x.ptr for n, x in outs.items()},
                         diagnostics={n: x.ptr for n, x in diag.items()}, memspace=1, ncol=ncol)
    ctx.synchronize()
    got = {n: x.download().reshape(-1) for n, x in list(outs.items()) + list(diag.items())}
    if not in_place:      # the inputs are only read
        assert all(X.same_bits(up[n].download().reshape(-1), c[n]) for n in up)
    return got


def best_device_call(ctx, c, name="", in_place=False, diagnostics=S_DIAG):
    n, ncol = c["t_soil"].shape
    up = {k: _hip.DeviceArray.from_host(np.ascontiguousarray(c[k])) for k in S_IN}
    shape = lambda k: (n, ncol) if k in SOIL_OUT else (ncol,)
    outs = {k: (up[k[:-4]] if in_place else _hip.DeviceArray(shape(k), np.float64)) for k in S_OUT}
    diag = {k: _hip.DeviceArray((ncol,), np.int32 if k == "flags" else np.float64) for k in diagnostics}
    ctx.second_best({k: x.ptr for k, x in up.items()}, c["dt"], X.best_constants(name), outs={k: x.ptr for k, x in outs.items()},
                    diagnostics={k: x.ptr for k, x in diag.items()}, memspace=1, ncol=ncol, nlay=n)
    ctx.synchronize()
    got = {k: x.download().reshape(shape(k)) for k, x in outs.items()}
    got.update({k: x.download().reshape(-1) for k, x in diag.items()})
    if not in_place:
        assert all(X.same_bits(up[k].download().reshape(np.shape(c[k])), c[k]) for k in S_IN)
    return got


# ---- every case and shape ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(X.BUCKET_CASES))
def test_bucket_kernel_has_the_statements_bits_on_every_shape(ctx, name):
    for ncol in X.NCOLS:
        c = X.bucket_case(name, ncol)
        got = bucket_call(ctx, c)
        assert set(got) == set(X.BUCKET_FIELDS[c["layers"]])
        for f in got:
            assert X.same_bits(got[f], c[f]), (ncol, f, float(np.abs(got[f] - c[f]).max()))
        X.bucket_budgets(c, got)      # on the kernel's own output


@pytest.mark.parametrize("name", X.BEST_CASES)
def test_second_best_kernel_equals_the_statement_on_every_shape(ctx, name):
    tol, worst, same, runs = X.tolerances(name), {}, 0, 0
    for nlay in X.BEST_NLAYS:
        for ncol in X.NCOLS:
            c = X.best_case(name, nlay, ncol)
            got = best_call(ctx, c, name)
            dev = X.deviations(got, c, X.BEST_FIELDS)
            worst = {f: max(worst.get(f, 0.0), v) for f, v in dev.items()}
            same, runs = same + all(X.same_bits(got[f], c[f]) for f in X.BEST_FIELDS), runs + 1
            assert X.same_bits(got["flags"], c["flags"]), (nlay, ncol)      # the decisions, exactly
            X.check_best_exact_properties(c, got, tol)      # on the kernel's own output: what no tolerance covers, water and ice per node
    print("second_best %s: largest deviations %s; %d of %d runs bit-identical" % (name, {f: "%.1e" % v for f, v in worst.items() if v}, same, runs))
    assert X.within(worst, tol), (worst, tol)


# ---- one representative case per entry -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["below_beta", "drainage"])
def test_bucket_device_pointers_in_place_and_null_diagnostics_agree_bit_for_bit(ctx, name):
    for ncol in (1, 65, 130):
        c = X.bucket_case(name, ncol)
        host, dev, dev_in_place = bucket_call(ctx, c), bucket_device_call(ctx, c), bucket_device_call(ctx, c, in_place=True)
        mine = {n: np.array(c[n]) for n in ("ts", "soil_moisture", "deep_moisture", "deep_temperature") if n in c}
        host_in_place = bucket_call(ctx, dict(c, **mine), outs={n + "_out": x for n, x in mine.items()})
        assert host_in_place["ts_out"] is mine["ts"]
        for other in (dev, dev_in_place, host_in_place):
            assert set(other) == set(host) and all(X.same_bits(other[f], host[f]) for f in host), ncol
    full = bucket_device_call(ctx, c)
    diag = tuple(n for n in B_DIAG if n in full)
    for skip in diag + (None,):
        names = tuple(n for n in diag if n != skip) if skip else ()
        got = bucket_device_call(ctx, c, diagnostics=names)
        assert all(X.same_bits(got[f], full[f]) for f in got) and set(got) == set(full) - (set(diag) - set(names)), skip


def test_second_best_device_pointers_in_place_and_null_diagnostics_agree_bit_for_bit(ctx):
    for nlay, ncol in ((2, 1), (4, 64), (12, 65), (12, 130)):
        c = X.best_case("mixed_types", nlay, ncol)
        host, dev, dev_in_place = best_call(ctx, c), best_device_call(ctx, c), best_device_call(ctx, c, in_place=True)
        mine = {n: np.array(c[n]) for n in ("t_soil", "x_w", "x_i", "ts", "snow")}
        host_in_place = best_call(ctx, dict(c, **mine), outs={n + "_out": x for n, x in mine.items()})
        assert host_in_place["t_soil_out"] is mine["t_soil"] and host_in_place["ts_out"] is mine["ts"]
        for other in (dev, dev_in_place, host_in_place):
            assert all(X.same_bits(other[f], host[f]) for f in S_OUT + S_DIAG), (nlay, ncol)
    full = best_device_call(ctx, c)
    for skip in S_DIAG + (None,):
        names = tuple(n for n in S_DIAG if n != skip) if skip else ()
        got = best_device_call(ctx, c, diagnostics=names)
        assert all(X.same_bits(got[f], full[f]) for f in S_OUT + names), skip


def test_a_column_alone_has_the_bits_of_the_column_inside_130(ctx):
    """Tile-edge indexing: columns 0, 63, 64, 65, 127, 128, 129 of the 130-column call, each run alone."""
    c = X.best_case("mixed_types", 12, 130)
    whole = best_call(ctx, c)
    b = X.bucket_case("drainage", 130)
    whole_b = bucket_call(ctx, b)
    for col in (0, 63, 64, 65, 127, 128, 129):
        part = {k: np.ascontiguousarray(c[k][..., col:col + 1]) for k in S_IN}
        got = best_call(ctx, dict(part, dt=c["dt"]))
        assert all(X.same_bits(got[f], whole[f][..., col:col + 1]) for f in S_OUT + S_DIAG), col
        part = {k: np.ascontiguousarray(b[k][col:col + 1]) for k in B_IN}
        got = bucket_call(ctx, dict(part, dt=b["dt"], layers=2, scalars=b["scalars"]))
        assert all(X.same_bits(got[f], whole_b[f][col:col + 1]) for f in got), col


# ---- the components on a DeviceState -------------------------------------------------------------------------------------------------
def _count_transfers(monkeypatch):
    count = dict(up=0, down=0)
    up, down = _hip.DeviceArray.upload, _hip.DeviceArray.download
    monkeypatch.setattr(_hip.DeviceArray, "upload", lambda self, arr: (count.__setitem__("up", count["up"] + 1), up(self, arr))[1])
    monkeypatch.setattr(_hip.DeviceArray, "download", lambda self: (count.__setitem__("down", count["down"] + 1), down(self))[1])
    return count


def _compare(ds, diag_d, new_h, diag_h):
    for name, h in list(new_h.items()) + list(diag_h.items()):
        ds["check"] = diag_d[name] if name in diag_d else ds[name]
        d = ds.download("check")
        values = np.transpose(d.values, [d.dims.index(x) for x in h.dims])
        assert X.same_bits(values, h.values) and d.attrs["units"] == h.attrs["units"] and set(d.dims) == set(h.dims), name


@pytest.mark.parametrize("name", ["below_beta", "drainage"])
def test_bucket_hydrology_on_a_device_state_equals_the_host_state_bit_for_bit(ctx, monkeypatch, name):
    ny, nx = 5, 13
    c = X.bucket_case(name, ny * nx)
    comp = climt_amd.BucketHydrology(num_layers=c["layers"], deep_drainage_timescale=c["scalars"]["tau_drain"], context=ctx)
    dt, state = datetime.timedelta(seconds=c["dt"]), X.bucket_host_state(c, ny, nx)
    diag_h, new_h = comp(state, dt)
    assert X.same_bits(new_h["surface_temperature"].values.reshape(-1), c["ts_out"])
    with climt_amd.DeviceState.from_host(state, [comp], context=ctx) as ds:
        before = ds["surface_temperature"]
        count = _count_transfers(monkeypatch)
        diag_d, back = comp(ds, dt)
        assert count == dict(up=0, down=0)      # nothing leaves or enters HBM in the call
        assert back is ds and set(diag_d) == set(diag_h) and ds["surface_temperature"] is not before
        _compare(ds, diag_d, new_h, diag_h)
        assert X.same_bits(before.buf.download().reshape(-1), c["ts"])      # the previous array is what it was


def test_second_best_on_a_device_state_equals_the_host_state_bit_for_bit(ctx, monkeypatch):
    ny, nx, n = 5, 13, 4
    c = X.best_case("mixed_types", n, ny * nx)
    comp, dt = climt_amd.SecondBEST(context=ctx), datetime.timedelta(seconds=c["dt"])
    state = X.best_host_state(c, ny, nx)
    diag_h, new_h = comp(state, dt)
    assert X.same_bits(comp.flags.reshape(-1), c["flags"])
    with climt_amd.DeviceState.from_host(state, [comp], context=ctx) as ds:
        before = ds["soil_temperature"]
        assert before.dims[0] == "soil_interface_levels" and before.shape == (n, ny * nx)
        count = _count_transfers(monkeypatch)
        diag_d, back = comp(ds, dt)
        assert count == dict(up=0, down=0)      # nothing leaves or enters HBM in the call
        assert back is ds and set(diag_d) == set(diag_h) and ds["soil_temperature"] is not before
        _compare(ds, diag_d, new_h, diag_h)
        assert X.same_bits(before.buf.download().reshape(n, -1), c["t_soil"])      # the previous array is what it was
        assert X.same_bits(comp.device_flags.buf.download().reshape(-1), c["flags"])
        first = ds["soil_temperature"]
        ds.step_count += 1
        comp(ds, dt)
        second = ds["soil_temperature"]
        ds.step_count += 1
        comp(ds, dt)
        assert second is not first and ds["soil_temperature"] is first      # two alternating buffer sets


def test_pressures_resident_in_the_radiations_units_are_read_through_the_scales(ctx):
    """A DeviceState shared with the radiation holds its pressures in mbar (whoever asks first decides).  Both device calls read
    them as they are resident and hand the library Pa per resident unit; with whole-hPa pressures the conversion is exact, so the
    result has the bits of the host state in Pa."""
    ny, nx, n = 5, 13, 4
    DQ = climt_amd.device_state.DeviceQuantity
    for which in ("best", "bucket"):
        c = {k: (np.array(v) if isinstance(v, np.ndarray) else v) for k, v in (X.best_case("mixed_types", n, ny * nx) if which == "best" else X.bucket_case("drainage", ny * nx)).items()}
        c["p_air"] = np.round(c["p_air"] / 100.0) * 100.0
        if which == "best":
            c["ps"] = np.round(c["ps"] / 100.0) * 100.0
            comp, state = climt_amd.SecondBEST(context=ctx), X.best_host_state(c, ny, nx)
        else:
            comp, state = climt_amd.BucketHydrology(num_layers=2, deep_drainage_timescale=c["scalars"]["tau_drain"], context=ctx), X.bucket_host_state(c, ny, nx)
        dt = datetime.timedelta(seconds=c["dt"])
        diag_h, new_h = comp(state, dt)
        with climt_amd.DeviceState.from_host(state, [comp], context=ctx) as ds:
            for name in ("air_pressure", "surface_air_pressure")[:2 if which == "best" else 1]:
                q = ds[name]
                ds[name] = DQ(_hip.DeviceArray.from_host(q.buf.download() / 100.0), q.shape, q.dims, "mbar")
            diag_d, _ = comp(ds, dt)
            _compare(ds, diag_d, new_h, diag_h)


@pytest.mark.parametrize("land_surface", ["bucket", "second_best"])
def test_radiative_convective_example_over_land_in_both_modes(land_surface):
    """Three steps of examples/radiative_convective.py over land, with the RRTMG radiation in the component list (so the pressures
    are resident in mbar), on a host state and on a DeviceState: the two modes to the tolerance of the example's own tests
    (tests/test_dry_adjustment_gpu.py, 1e-9); the run without the flag does not have the land diagnostics."""
    import importlib.util
    import os
    from helpers import maxdiff
    spec = importlib.util.spec_from_file_location("radiative_convective", os.path.join(ROOT, "examples", "radiative_convective.py"))
    ex = importlib.util.module_from_spec(spec); spec.loader.exec_module(ex)
    first_h, end_h = ex.run(3, device_resident=False, land_surface=land_surface)
    first_d, end_d = ex.run(3, device_resident=True, land_surface=land_surface)
    extra = ("surface_upward_sensible_heat_flux", "surface_upward_latent_heat_flux", "evaporation_rate")
    names = ("air_temperature", "surface_temperature") + (("lwe_thickness_of_soil_moisture_content",) if land_surface == "bucket" else
                                                          ("soil_temperature", "soil_liquid_water_content", "soil_ice_content", "surface_albedo_for_direct_shortwave"))
    close = lambda h, d: maxdiff(h.values, np.transpose(d.values, [d.dims.index(x) for x in h.dims])) <= 1e-9 * max(1.0, float(np.abs(h.values).max()))
    for n in extra:
        assert np.all(np.isfinite(first_h[n].values)) and close(first_h[n], first_d[n]), n
    for n in names + extra:
        assert np.all(np.isfinite(end_h[n].values)) and close(end_h[n], end_d[n]), n
    assert float(first_h["surface_upward_sensible_heat_flux"].values.ravel()[0]) != 0.0      # the land surface exchanged heat at step 0
    with pytest.raises(ValueError, match="exclusive"):
        ex.run(1, land_surface=land_surface, sea_ice=True)
