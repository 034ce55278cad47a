"""GPU tests of the shortwave surface albedo by band (rrtmg_hip_sw_fluxes_surface; run with -m gpu on an MI355X): the
committed reference fixtures (tests/albedo_cases.py) through host and device pointers, the identity with the plain call when
the per-band arrays follow the band rule, band independence, the surface closure by band, the struct rules, and
RRTMGShortwave(spectral_surface_albedo=True) on a host state, a DeviceState and a two-block ShardedRadiation."""
import ctypes as C

import numpy as np
import pytest

import albedo_cases as A
import band_cases as B
from helpers import maxdiff

pytestmark = pytest.mark.gpu

TIGHT = 5.0e-9       # the project's bound for committed fixtures (tests/test_gpu_parity.py)
BASE = dict(icld=1, iaer=0, adjes=1.0, dyofyr=1, scon=1367.0, isolvar=0, inflg=2, iceflg=1, liqflg=1)
SW_COMPONENTS = ("dirdflx", "difdflx", "dirdnuv", "difdnuv", "dirdnir", "difdnir", "dirdflxc", "difdflxc")
BROADBAND = ("asdir", "asdif", "aldir", "aldif")


def _device_call(ctx, c, mcica, surface=None, bands=False, components=False):
    """The call on device pointers -> (plain outputs, band arrays, components), downloaded."""
    from climt_amd import _hip
    from climt_amd._lib import SW_OUT
    nlay, ncol = c["play"].shape
    dev = {k: _hip.DeviceArray.from_host(v) for k, v in c.items() if isinstance(v, np.ndarray)}
    args = {k: v.ptr for k, v in dev.items()}
    args.update({k: v for k, v in c.items() if not isinstance(v, np.ndarray)}); args.update(ncol=ncol, nlay=nlay)
    out = {k: _hip.DeviceArray((nlay + lev, ncol)) for k, lev in SW_OUT}
    band = {m: _hip.DeviceArray(v.shape) for m, v in B.band_arrays("sw", nlay, ncol).items()} if bands else {}
    comp = {k: _hip.DeviceArray((nlay + 1, ncol)) for k in SW_COMPONENTS} if components else {}
    sdev = {k: _hip.DeviceArray.from_host(v) for k, v in (surface or {}).items() if v is not None}
    kw = {}
    if bands:
        kw.update(bands={m: v.ptr for m, v in band.items()})
    if components:
        kw.update(components={k: v.ptr for k, v in comp.items()})
    if surface is not None:
        kw.update(surface={k: v.ptr for k, v in sdev.items()})
    ctx.sw_fluxes(args, mcica=mcica, out={k: v.ptr for k, v in out.items()}, memspace=1, **kw)
    ctx.synchronize()
    return {k: v.download() for k, v in out.items()}, {m: v.download() for m, v in band.items()}, {k: v.download() for k, v in comp.items()}


@pytest.mark.parametrize("case", list(A.CASES))
def test_surface_vs_reference_fixture(gpu_ctx, case):
    """The six outputs against the reference's solver with the same per-band albedos: host pointers, device pointers, and
    with the four broadband pointers absent."""
    c, mcica, exp = A.load_case(case)
    plain, surface = A.split_surface(c)
    out = gpu_ctx.sw_fluxes(plain, mcica=mcica, surface=surface)
    for k in A.OUTPUTS:
        d = maxdiff(out[k], exp[k])
        print(case, k, "host pointers: max |GPU - reference| = %.3e" % d)
        assert d <= TIGHT, (case, k, d)
    dout, _, _ = _device_call(gpu_ctx, plain, mcica, surface=surface)
    for k in A.OUTPUTS:
        d = maxdiff(dout[k], exp[k])
        print(case, k, "device pointers: max |GPU - reference| = %.3e" % d)
        assert d <= TIGHT, (case, k, d)
        assert np.array_equal(dout[k], out[k]), (case, k)
    bare = {k: v for k, v in plain.items() if k not in BROADBAND}
    again = gpu_ctx.sw_fluxes(bare, mcica=mcica, surface=surface)
    assert all(np.array_equal(again[k], out[k]) for k in out)
    keyed = gpu_ctx.sw_fluxes(c, mcica=mcica)      # the keys albdir / albdif of the input dict mean the same
    assert all(np.array_equal(keyed[k], out[k]) for k in out)


def _grid(ncol, nlay, seed, mcica, clear=False):
    from climt_amd.synthetic import make_columns, overcast
    c = make_columns(ncol, nlay, cloudy=not clear, seed=seed); c.pop("lat")
    if not clear:
        for t in range(0, (ncol + 63) // 64, 4):      # every fourth 64-column tile cloud-free: both solve variants in one call
            for k in ("cldfr", "cliqwp", "cicewp"):
                c[k][:, t * 64:(t + 1) * 64] = 0.0
        if not mcica:
            c = overcast(c)
    c.update(BASE); c.update(irng=0, permuteseed=11, icld=0 if clear else (2 if mcica else 1))
    return c


@pytest.mark.parametrize("ncol,nlay,mcica,clear", [(700, 40, False, True), (1000, 40, True, False), (16384, 60, True, False)])
def test_band_rule_arrays_are_the_plain_call(gpu_ctx, ncol, nlay, mcica, clear):
    """Identity: per-band arrays built by the band rule from the four broadband inputs give the bits of the plain call -- the
    six outputs, the eight components, every band member -- on a clear grid, a McICA grid with mixed clear / cloudy tiles and
    a multi-chunk grid; host and device pointers; each member on its own too."""
    c = _grid(ncol, nlay, 31, mcica, clear)
    ruled = dict(zip(("albdir", "albdif"), A.band_rule(c)))
    comp0 = {k: np.zeros((nlay + 1, ncol)) for k in SW_COMPONENTS}
    band0 = B.band_arrays("sw", nlay, ncol)
    plain = gpu_ctx.sw_fluxes(c, mcica=mcica, components=comp0, bands=band0)
    bare_plain = gpu_ctx.sw_fluxes(c, mcica=mcica)
    assert all(np.array_equal(bare_plain[k], plain[k]) for k in plain)
    comp1 = {k: np.zeros((nlay + 1, ncol)) for k in SW_COMPONENTS}
    band1 = B.band_arrays("sw", nlay, ncol)
    got = gpu_ctx.sw_fluxes({k: v for k, v in c.items() if k not in BROADBAND}, mcica=mcica, components=comp1, bands=band1, surface=ruled)
    assert all(np.array_equal(got[k], plain[k]) for k in plain)
    assert all(np.array_equal(comp1[k], comp0[k]) for k in comp0)
    assert all(np.array_equal(band1[m], band0[m]) for m in band0)
    assert float(plain["swuflx"].max()) > 1.0 and float(band0["up"].max()) > 0.1
    only = gpu_ctx.sw_fluxes(c, mcica=mcica, surface=ruled)      # without components and bands
    assert all(np.array_equal(only[k], plain[k]) for k in plain)
    if ncol <= 1000:
        for one in ({"albdir": ruled["albdir"]}, {"albdif": ruled["albdif"]}, {"albdir": None, "albdif": None}):
            half = gpu_ctx.sw_fluxes(c, mcica=mcica, surface=one)
            assert all(np.array_equal(half[k], plain[k]) for k in plain), list(one)
        dout, dband, dcomp = _device_call(gpu_ctx, c, mcica, surface=ruled, bands=True, components=True)
        assert all(np.array_equal(dout[k], plain[k]) for k in plain)
        assert all(np.array_equal(dcomp[k], comp0[k]) for k in comp0) and all(np.array_equal(dband[m], band0[m]) for m in band0)


def test_band_independence(gpu_ctx):
    """Changing the albedo of band k only leaves every other band's rows bit-identical; band k's surface `up` changes
    wherever the band delivers anything to the surface (the 38000-50000 cm^-1 band does not: ozone)."""
    c = _grid(256, 40, 33, True)
    rng = np.random.default_rng(5)
    surface = {"albdir": rng.uniform(0.02, 0.95, (14, 256)), "albdif": rng.uniform(0.02, 0.95, (14, 256))}
    base = B.band_arrays("sw", 40, 256)
    gpu_ctx.sw_fluxes(c, mcica=True, bands=base, surface=surface)
    nlit = 0
    for k in range(14):
        s2 = {m: v.copy() for m, v in surface.items()}
        s2["albdir"][k] = 0.5 * s2["albdir"][k] + 0.01
        s2["albdif"][k] = 0.5 * s2["albdif"][k] + 0.01
        band = B.band_arrays("sw", 40, 256)
        gpu_ctx.sw_fluxes(c, mcica=True, bands=band, surface=s2)
        others = [b for b in range(14) if b != k]
        for m in ("up", "dn", "dndir"):
            assert np.array_equal(band[m][others], base[m][others]), (k, m)
        lit = base["up"][k, 0] > 1.0e-6
        assert np.all(band["up"][k, 0][lit] != base["up"][k, 0][lit]), k
        nlit += bool(lit.any())
    assert nlit >= 10


@pytest.mark.parametrize("case", ["clear_L60", "overcast_L60", "aer10_overcast", "overcast_L100", "lowsun_night"])
def test_surface_closure_by_band(gpu_ctx, case):
    """At the surface row of the band outputs, up_b == albdir_b * dndir_b + albdif_b * (dn_b - dndir_b): in the clear-sky
    stream, and with the all-sky members on overcast non-McICA columns.  Per g-point this is an identity of the adding
    method's surface formulas; checked where up_b > 1e-6 W m^-2, relative bound band_cases.SUM_BOUND = 256 x 2^-53 (the
    reference's own band values leave 5.4 x 2^-53; the device reciprocal is documented at <= 2.2e-15, about 20 x 2^-53)."""
    c, mcica, _ = A.load_case(case)
    plain, surface = A.split_surface(c)
    nlay, ncol = plain["play"].shape
    band = B.band_arrays("sw", nlay, ncol, "boundaries")
    gpu_ctx.sw_fluxes(plain, mcica=mcica, bands=band, band_levels="boundaries", surface=surface)
    streams = [("upc", "dnc", "dndirc")] + ([("up", "dn", "dndir")] if "overcast" in case else [])
    for members in streams:
        up, dn, dr = (band[m][:, 0] for m in members)
        want = surface["albdir"] * dr + surface["albdif"] * (dn - dr)
        ok = up > 1.0e-6
        worst = float((np.abs(up - want)[ok] / up[ok]).max())
        print(case, members[0], "worst closure residual = %.2f x 2^-53 over %d (band, column) pairs" % (worst / B.EPS, int(ok.sum())))
        assert ok.sum() >= 14
        assert worst <= B.SUM_BOUND, (case, members, worst / B.EPS)


def test_struct_rules(gpu_ctx):
    from climt_amd._lib import SwArgs, SwSurface
    lib = gpu_ctx.lib
    keep = np.full((14, 64), 0.3)
    a = SwArgs(); a.struct_size = C.sizeof(SwArgs)
    bad = SwSurface(); bad.struct_size = C.sizeof(SwSurface) - 8; bad.albdir = keep.ctypes.data
    assert lib.rrtmg_hip_sw_fluxes_surface(gpu_ctx.h, C.byref(a), C.byref(bad), None, None) == 4
    assert "rrtmg_sw_surface: struct_size" in lib.rrtmg_hip_last_error(gpu_ctx.h).decode()
    c = _grid(64, 20, 3, False)
    from climt_amd._lib import RRTMGError
    with pytest.raises(RRTMGError):      # a member missing and its broadband pair missing
        gpu_ctx.sw_fluxes({k: v for k, v in c.items() if k not in BROADBAND}, surface={"albdir": keep})
    with pytest.raises(KeyError):
        gpu_ctx.sw_fluxes(c, surface={"albedo": keep})
    with pytest.raises(ValueError):
        gpu_ctx.sw_fluxes(c, surface={"albdir": keep.T})
    # column sort on: a call with a surface struct is not sorted, the bits stay; deferred mode returns once enqueued
    c = _grid(512, 40, 35, True)
    rng = np.random.default_rng(6)
    surface = {"albdir": rng.uniform(0.02, 0.95, (14, 512)), "albdif": rng.uniform(0.02, 0.95, (14, 512))}
    want, _, _ = _device_call(gpu_ctx, c, True, surface=surface)
    host = gpu_ctx.sw_fluxes(c, mcica=True, surface=surface)
    assert all(np.array_equal(host[k], want[k]) for k in want)
    try:
        gpu_ctx.set_column_sort(True)
        got, _, _ = _device_call(gpu_ctx, c, True, surface=surface)
    finally:
        gpu_ctx.set_column_sort(False)
    assert all(np.array_equal(got[k], want[k]) for k in want)
    prev = gpu_ctx.set_deferred(True)
    try:
        got, _, _ = _device_call(gpu_ctx, c, True, surface=surface)
    finally:
        gpu_ctx.set_deferred(prev)
    assert all(np.array_equal(got[k], want[k]) for k in want)


@pytest.mark.parametrize("mcica", [False, True])
def test_component_on_host_state_device_state_and_plain_instance(mcica):
    """RRTMGShortwave(spectral_surface_albedo=True): host state == DeviceState, bit for bit; with the two quantities filled by
    the band rule it returns what the default instance returns on the four broadband ones."""
    import climt_amd
    from climt_amd._sympl_compat import DataArray
    from climt_amd.rrtmg import shortwave
    from helpers import load_cache_case
    state = load_cache_case("TestRRTMGShortwaveMCICA", "3d")[0]
    kw = dict(mcica=mcica, cloud_overlap_method="maximum_random" if mcica else "clear_only", random_number_generator="kissvec")
    sw = shortwave.RRTMGShortwave(spectral_surface_albedo=True, **kw)
    plain = shortwave.RRTMGShortwave(**kw)
    assert sw.input_properties == shortwave.RRTMGShortwave.input_properties_for(True)
    assert plain.input_properties is shortwave.RRTMGShortwave.input_properties
    one = state["surface_albedo_for_direct_shortwave"]
    rule = shortwave.SPECTRAL_ALBEDO_BAND_RULE

    def by_band(member, values=None):
        v = np.stack([np.asarray(state[rule[member][b]].values, dtype=np.float64) for b in range(14)]) if values is None else values
        return DataArray(np.ascontiguousarray(v), dims=("num_shortwave_bands",) + tuple(one.dims), attrs={"units": "dimensionless"})
    ruled = dict(state)
    for name, member in shortwave.SPECTRAL_ALBEDO_INPUTS.items():
        ruled[name] = by_band(member)
    np.random.seed(3)
    t0, d0 = plain(state)
    np.random.seed(3)
    t1, d1 = sw(ruled)
    for k in d0:
        assert np.array_equal(np.asarray(d1[k].values), np.asarray(d0[k].values)), k
    assert np.array_equal(np.asarray(t1["air_temperature"].values), np.asarray(t0["air_temperature"].values))
    rng = np.random.default_rng(9)
    free = dict(state)
    for name in shortwave.SPECTRAL_ALBEDO_INPUTS:
        free[name] = by_band(None, rng.uniform(0.02, 0.95, (14,) + tuple(one.shape)))
    np.random.seed(3)
    _, host = sw(free)
    assert not np.array_equal(np.asarray(host["upwelling_shortwave_flux_in_air"].values), np.asarray(d0["upwelling_shortwave_flux_in_air"].values))
    ds = climt_amd.DeviceState.from_host(free, [sw])
    np.random.seed(3)
    _, dev = sw(ds)
    ds.ctx.synchronize()
    for k in host:
        d = dev[k]
        got = d.buf.download().reshape(d.shape)
        assert np.array_equal(got, np.asarray(host[k].values).reshape(got.shape)), k
    ds.close()
    default = climt_amd.get_default_state([sw])
    assert all(k in default for k in shortwave.SPECTRAL_ALBEDO_INPUTS) and not any(k in default for k in shortwave.BROADBAND_ALBEDO_INPUTS)
    sw(default)


def test_two_block_shard_equals_the_whole(gpu_ctx):
    """ShardedRadiation slices albdir / albdif with the other inputs: two blocks on one GPU == the unsharded call."""
    from climt_amd.distributed import ShardedRadiation

    class Comm:
        world = 2

        def __init__(self, rank):
            self.rank = rank

        def wait(self):
            pass
    N, L = 1000, 40
    c = _grid(N, L, 37, True)
    rng = np.random.default_rng(7)
    c["albdir"], c["albdif"] = rng.uniform(0.02, 0.95, (14, N)), rng.uniform(0.02, 0.95, (14, N))
    want = gpu_ctx.sw_fluxes(c, mcica=True)
    base = gpu_ctx.sw_fluxes({k: v for k, v in c.items() if k not in ("albdir", "albdif")}, mcica=True)
    assert not np.array_equal(want["swuflx"], base["swuflx"])
    parts = []
    for rank in (0, 1):
        sr = ShardedRadiation(gpu_ctx, Comm(rank), N, L, gather="none")
        sr.set_inputs(c)
        parts.append(sr.local_host(sr.step(mcica=True)))
        sr.close()
    assert parts[0]["swuflx"].shape[1] + parts[1]["swuflx"].shape[1] == N and parts[0]["swuflx"].shape[1] % 64 == 0
    for k in want:
        assert np.array_equal(np.concatenate([p[k] for p in parts], axis=1), want[k]), k
