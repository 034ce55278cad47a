"""The Emanuel convection scheme on the GPU: emanuel_kernel (rrtmg_hip_emanuel_convection) against the fixtures of the reference's own
numpy statement (tests/golden/emanuel_<case>_<nlay>.npz) on every case, layer count and tile-edge column count, each field within
the tolerance its fixture carries and iflag exactly; and what must hold bit for bit -- the cases interleaved column by column,
host against device pointers, cbmf in place, NULL diagnostics, a chunked call; qs formed by the kernel; the component on a
DeviceState with the pressures resident in Pa and in mbar; examples/radiative_convective.py --moist-convection in both modes.

Measured on an MI355X: iflag exact everywhere, every early exit bit-identical to its fixture; largest deviation 2.1e-13 (deep,
precip), largest deviation / tolerance 1.4e-2 (deep)."""
import datetime
import importlib.util
import os

import numpy as np
import pytest

import climt_amd
from climt_amd import _hip
from helpers import ROOT, maxdiff

import emanuel_cases as X
from test_emanuel import DIAG, DNAMES, FIXTURES, MISSING, NAMES, grid_state

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    from climt_amd.rrtmg.common import make_context
    return make_context(0)


def _result(ft, fq, fu, fv, cbmf_out, d):
    got = dict(ft=ft, fq=fq, fu=fu, fv=fv, cbmf_out=cbmf_out)
    got.update({n: d.get(n) for n in DIAG})
    return got


def host_call(ctx, a, f, use_qs=True, **kw):
    return _result(*ctx.emanuel_convection(a["t"], a["q"], a["u"], a["v"], a["p"], a["ph"], a["cbmf"], float(f["dt"]), X.parameters(f), X.constants(f),
                                           qs=a["qs"] if use_qs else None, **kw))


def device_call(ctx, a, f, in_place=False):
    """Device pointers -> the results on the host."""
    nlay, ncol = a["t"].shape
    d = {k: _hip.DeviceArray.from_host(np.ascontiguousarray(a[k])) for k in X.INPUTS}
    out = [_hip.DeviceArray((nlay, ncol)) for _ in range(4)]
    cb = d["cbmf"] if in_place else _hip.DeviceArray((ncol,))
    diag = {n: _hip.DeviceArray((ncol,)) for n in DIAG[:5]}
    diag.update(iflag=_hip.DeviceArray((ncol,), np.int32), ft_per_day=_hip.DeviceArray((nlay, ncol)))
    ctx.emanuel_convection(d["t"], d["q"], d["u"], d["v"], d["p"], d["ph"], d["cbmf"], float(f["dt"]), X.parameters(f), X.constants(f), qs=d["qs"],
                           ft=out[0], fq=out[1], fu=out[2], fv=out[3], cbmf_out=cb, diagnostics=diag, memspace=1, ncol=ncol, nlay=nlay)
    ctx.synchronize()
    assert all(X.same_bits(d[k].download(), a[k]) for k in X.INPUTS if not (in_place and k == "cbmf"))      # the inputs are only read
    return _result(*(o.download() for o in out), cb.download(), {n: x.download() for n, x in diag.items()})


def same(a, b, keys=None):
    return all(X.same_bits(np.asarray(a[k], dtype=np.float64), np.asarray(b[k], dtype=np.float64)) for k in (keys or a))


@pytest.mark.parametrize("case", X.CASES)
def test_kernel_agrees_with_every_fixture_on_every_shape(ctx, case):
    worst, dev = 0.0, {}
    for nlay in X.NLAYS:
        if (case, nlay) in MISSING:
            continue
        f = X.load(case, nlay)
        for ncol in X.NCOLS:
            got = host_call(ctx, X.tile(f, ncol), f)
            worst = max(worst, X.check(got, f, ncol, (case, nlay, ncol)))
            assert X.same_bits(got["ft_per_day"], got["ft"] * 86400.0)
            for n, v in X.deviations(got, X.reference(f, ncol)).items():
                dev[n] = max(dev.get(n, 0.0), v)
    print("emanuel_kernel, %s: largest deviation / tolerance %.3e; largest deviation %s" % (case, worst, ", ".join("%s %.2e" % kv for kv in sorted(dev.items()))))


@pytest.mark.parametrize("nlay", X.NLAYS)
def test_interleaved_cases_equal_their_single_case_results_bit_for_bit(ctx, nlay):
    """One call with the cases (of one dt) interleaved column by column: a tile holds every exit side by side."""
    cases = [c for c in X.CASES if (c, nlay) not in MISSING and c != "cfl"]
    ncol = 130
    fs = [X.load(c, nlay) for c in cases]
    singles = [host_call(ctx, X.tile(f, ncol), f) for f in fs]
    pick = np.arange(ncol) % len(cases)
    mixed = {k: np.ascontiguousarray(np.choose(pick, [X.tile(f, ncol)[k] for f in fs])) for k in X.INPUTS}
    got = host_call(ctx, mixed, fs[0])
    assert sorted(set(got["iflag"].tolist())) == [0, 1, 2, 3]
    for i, single in enumerate(singles):
        cols = pick == i
        assert all(X.same_bits(np.asarray(got[k], dtype=np.float64)[..., cols], np.asarray(single[k], dtype=np.float64)[..., cols]) for k in got), cases[i]


def test_host_and_device_pointers_and_cbmf_in_place_agree_bit_for_bit(ctx):
    for case, nlay, ncol in (("deep", 8, 1), ("sheared", 30, 130), ("cfl", 61, 65), ("too_cold", 10, 64)):
        f = X.load(case, nlay)
        a = X.tile(f, ncol)
        want = host_call(ctx, a, f)
        cb = np.array(a["cbmf"])
        got = host_call(ctx, dict(a, cbmf=cb), f, cbmf_out=cb)      # host arrays, cbmf in place
        assert got["cbmf_out"] is cb and same(got, want)
        for in_place in (False, True):
            assert same(device_call(ctx, a, f, in_place), want), (case, nlay, ncol, in_place)


def test_every_diagnostic_pointer_may_be_null(ctx):
    for case, nlay, ncol in (("deep", 30, 65), ("freezing", 61, 130), ("lcl_range", 8, 1)):
        f = X.load(case, nlay)
        a = X.tile(f, ncol)
        full, bare = host_call(ctx, a, f), host_call(ctx, a, f, diagnostics=None)
        keys = X.PROFILES + ("cbmf_out",)
        assert all(bare[n] is None for n in DIAG) and same(bare, full, keys)
        some = host_call(ctx, a, f, diagnostics=dict(precip=np.empty(ncol), iflag=np.empty(ncol, dtype=np.int32)))
        assert same(some, full, keys + ("precip", "iflag")) and some["cape"] is None


def test_each_diagnostic_left_out_leaves_the_others_their_bits(ctx):
    """Host pointers, 65 columns (two tiles, one live lane in the second): the staging buffer of a call is laid out over the arrays
    that are given, so every diagnostic in turn is left out of an otherwise full call, with qs handed over and with qs left to the
    kernel (which changes the numbers, so each is compared with the full call of its own kind).  At 5 layers, the entry's minimum
    plus one, where every column leaves by an early exit, and at 8, where the "deep" columns convect.  What is still asked for has
    the bits of the full call, in the caller's own arrays, and the inputs keep theirs."""
    f = X.load("deep", 8)
    deep = X.tile(f, 65)
    shallow = {k: deep[k] if k == "cbmf" else np.ascontiguousarray(deep[k][:6 if k == "ph" else 5]) for k in X.INPUTS}
    for a in (shallow, deep):
        before = {k: np.array(a[k]) for k in X.INPUTS}
        for use_qs in (True, False):
            full = host_call(ctx, a, f, use_qs)
            assert (full["iflag"] == 1).all() == (a is deep)
            for left_out in DIAG:
                diag = {n: np.full(full[n].shape, -7, dtype=full[n].dtype) for n in DIAG if n != left_out}
                got = host_call(ctx, a, f, use_qs, diagnostics=diag)
                assert got[left_out] is None and all(got[n] is diag[n] for n in diag)
                assert same(got, full, [k for k in full if k != left_out]), (a["t"].shape, use_qs, left_out)
                assert all(X.same_bits(a[k], before[k]) for k in X.INPUTS)


def test_qs_formed_by_the_kernel(ctx):
    """qs = NULL: the kernel's own bolton_q_sat (device exp) against the numpy one handed over -- within the fixtures' tolerances."""
    for case, nlay in FIXTURES:
        f = X.load(case, nlay)
        X.check(host_call(ctx, X.tile(f, 65), f, use_qs=False), f, 65, (case, nlay, "qs formed"))


def test_a_chunked_call_equals_the_unchunked_call_bit_for_bit(monkeypatch):
    """A second context with the scratch budget forced below two tiles of work space (RRTMG_HIP_MAX_SCRATCH_BYTES): three launches
    over one tile of slabs each."""
    from climt_amd import _lib
    f = X.load("deep", 30)
    a = X.tile(f, 130)
    per_tile = 64 * 8 * (22 * 31 + 6 * 26 * 27)
    monkeypatch.setenv("RRTMG_HIP_MAX_SCRATCH_BYTES", str(per_tile + per_tile // 2))
    small = _lib.Context(0)
    monkeypatch.delenv("RRTMG_HIP_MAX_SCRATCH_BYTES")
    whole = _lib.Context(0)
    try:
        got, want = host_call(small, a, f), host_call(whole, a, f)
        assert same(got, want) and X.check(got, f, 130) <= 1.0
        mixed = dict(a)      # and with an early exit in every tile
        g = X.tile(X.load("no_origin", 30), 130)
        for k in X.INPUTS:
            mixed[k] = np.array(a[k]); mixed[k][..., ::7] = g[k][..., ::7]
        assert same(host_call(small, mixed, f), host_call(whole, mixed, f))
    finally:
        small.close()
        whole.close()


class ResidentPressureUnits:
    """A component listed first in DeviceState.from_host so that the pressures become resident in its units."""

    def __init__(self, units):
        self.input_properties = {"air_pressure": {"dims": ["mid_levels", "*"], "units": units},
                                 "air_pressure_on_interface_levels": {"dims": ["interface_levels", "*"], "units": units}}


@pytest.mark.parametrize("units", ["Pa", "mbar"])
def test_component_on_a_device_state_equals_the_host_state_bit_for_bit(ctx, units):
    """The standard of the boundary-layer tests: the DeviceState path and the host component agree bit for bit, the pressures
    resident in Pa (read through pressure_scale = 0.01, the rounding the host path's unit conversion makes) and in mbar."""
    case, nlay, ny, nx = "sheared", 30, 5, 13
    f = X.load(case, nlay)
    comp = climt_amd.EmanuelConvection(context=ctx)
    dt = datetime.timedelta(seconds=float(f["dt"]))
    state = grid_state(f, ny, nx, units)
    tendencies, diagnostics = comp(state, dt)
    assert (diagnostics["convective_state"].values == 1).all() and (diagnostics["convective_precipitation_rate"].values > 0).any()
    with climt_amd.DeviceState.from_host(state, [ResidentPressureUnits(units), comp], context=ctx) as ds:
        assert ds["air_pressure"].units == units and ds["air_temperature"].dims == ("mid_levels", "*")
        before = ds["cloud_base_mass_flux"]
        tend_d, diag_d = comp(ds, dt)
        assert set(tend_d) == set(NAMES) and set(diag_d) == set(DNAMES) | {"air_temperature_tendency_from_convection"}
        assert all(isinstance(x, climt_amd.DeviceQuantity) for x in list(tend_d.values()) + list(diag_d.values()))      # they stay in HBM
        assert ds["cloud_base_mass_flux"] is diag_d["cloud_base_mass_flux"] and ds["cloud_base_mass_flux"] is not before      # rebound
        for name, want in list(tendencies.items()) + list(diagnostics.items()):
            ds["probe"] = (tend_d if name in tendencies else diag_d)[name]
            got = ds.download("probe")
            assert got.attrs["units"] == want.attrs["units"], name
            g = np.transpose(got.values, [got.dims.index(d) for d in want.dims])
            assert X.same_bits(g.astype(np.float64), want.values.astype(np.float64)), name


def test_radiative_convective_example_with_moist_convection_in_both_modes():
    """Three steps of examples/radiative_convective.py with moist_convection=True on a host state and on a DeviceState, to the
    tolerance of the example's own tests; it rains from step 0, and the run without the flag knows nothing of it."""
    spec = importlib.util.spec_from_file_location("radiative_convective", os.path.join(ROOT, "examples", "radiative_convective.py"))
    ex = importlib.util.module_from_spec(spec); spec.loader.exec_module(ex)
    first_h, end_h = ex.run(3, device_resident=False, moist_convection=True)
    first_d, end_d = ex.run(3, device_resident=True, moist_convection=True)
    for first in (first_h, first_d):
        assert int(first["convective_state"].values.ravel()[0]) == 1 and float(first["convective_precipitation_rate"].values.ravel()[0]) > 0.0
    assert maxdiff(first_h["convective_precipitation_rate"].values.ravel(), first_d["convective_precipitation_rate"].values.ravel()) <= 1e-9
    for name in ("air_temperature", "specific_humidity", "surface_temperature", "eastward_wind", "northward_wind", "cloud_base_mass_flux",
                 "convective_precipitation_rate"):
        h, d = end_h[name], end_d[name]
        g = np.transpose(d.values, [d.dims.index(x) for x in h.dims])
        assert np.all(np.isfinite(h.values)) and maxdiff(h.values, g) <= 1e-9, (name, maxdiff(h.values, g))
    _, plain = ex.run(3, device_resident=False)
    assert "convective_precipitation_rate" not in plain
