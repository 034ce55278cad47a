"""GPU tests of the fluxes by band (rrtmg_hip_sw_fluxes_bands, rrtmg_hip_lw_fluxes_bands; run with -m gpu on an MI355X): the
committed reference fixtures (tests/band_cases.py), the plain outputs unchanged by the band path, the `levels` modes, subsets
of the members, identities on large grids, chunking, shards, column sort, the refused requests, and band_fluxes=True of the
two components on a host state and a DeviceState."""
import ctypes as C

import numpy as np
import pytest

import band_cases as B
from helpers import maxdiff

pytestmark = pytest.mark.gpu

TIGHT = 5.0e-9       # the project's bound for committed fixtures (tests/test_gpu_parity.py)
BASE = dict(icld=1, iaer=0, adjes=1.0, dyofyr=1, scon=1367.0, isolvar=0, inflg=2, iceflg=1, liqflg=1)
SW_COMPONENTS = ("dirdflx", "difdflx", "dirdnuv", "difdnuv", "dirdnir", "difdnir", "dirdflxc", "difdflxc")


def _call(ctx, which):
    return ctx.sw_fluxes if which == "sw" else ctx.lw_fluxes


@pytest.mark.parametrize("case", list(B.CASES))
def test_bands_vs_reference_fixture(gpu_ctx, case):
    """Every member, both `levels`, and the plain outputs of the same call, against the reference."""
    which = case[:2]
    c, mcica, bb, exp = B.load_case(case)
    nlay, ncol = c["play"].shape
    band = B.band_arrays(which, nlay, ncol)
    out = _call(gpu_ctx, which)(c, mcica=mcica, bands=band)
    for m in B.MEMBERS[which]:
        d = maxdiff(band[m], exp[m])
        print(case, m, "max |GPU - reference| = %.3e" % d)
        assert d <= TIGHT, (case, m, d)
    for k, v in bb.items():
        assert maxdiff(out[k], v) <= TIGHT, (case, k, maxdiff(out[k], v))
    two = B.band_arrays(which, nlay, ncol, "boundaries")
    out2 = _call(gpu_ctx, which)(c, mcica=mcica, bands=two, band_levels="boundaries")
    for m in B.MEMBERS[which]:
        assert maxdiff(two[m][:, 0], exp[m][:, 0]) <= TIGHT and maxdiff(two[m][:, 1], exp[m][:, nlay]) <= TIGHT, (case, m)
        assert np.array_equal(two[m][:, 0], band[m][:, 0]) and np.array_equal(two[m][:, 1], band[m][:, nlay]), (case, m)
    assert all(np.array_equal(out2[k], out[k]) for k in out)


def _grid(ncol, nlay, seed, mcica, icld=None):
    from climt_amd.synthetic import make_columns, overcast
    c = make_columns(ncol, nlay, cloudy=True, seed=seed); c.pop("lat")
    # every fourth 64-column tile cloud-free: both solve variants in one call
    for t in range(0, (ncol + 63) // 64, 4):
        for k in ("cldfr", "cliqwp", "cicewp"):
            c[k][:, t * 64:(t + 1) * 64] = 0.0
    if not mcica:
        c = overcast(c)
    c.update(BASE); c.update(irng=0, permuteseed=11, icld=icld if icld is not None else (2 if mcica else 1))
    return c


def _device_call(ctx, which, c, mcica, bands=True, levels="all", components=False):
    """The call on device pointers -> (plain outputs, band arrays, components), downloaded."""
    from climt_amd import _hip
    from climt_amd._lib import LW_OUT, SW_OUT
    nlay, ncol = c["play"].shape
    dev = {k: _hip.DeviceArray.from_host(v) for k, v in c.items() if isinstance(v, np.ndarray)}
    args = {k: v.ptr for k, v in dev.items()}
    args.update({k: v for k, v in c.items() if not isinstance(v, np.ndarray)}); args.update(ncol=ncol, nlay=nlay)
    out = {k: _hip.DeviceArray((nlay + lev, ncol)) for k, lev in (SW_OUT if which == "sw" else LW_OUT)}
    band = {m: _hip.DeviceArray(v.shape) for m, v in B.band_arrays(which, nlay, ncol, levels).items()} if bands else {}
    comp = {k: _hip.DeviceArray((nlay + 1, ncol)) for k in SW_COMPONENTS} if components else {}
    kw = {}
    if bands:
        kw.update(bands={m: v.ptr for m, v in band.items()}, band_levels=levels)
    if components:
        kw.update(components={k: v.ptr for k, v in comp.items()})
    _call(ctx, which)(args, mcica=mcica, out={k: v.ptr for k, v in out.items()}, memspace=1, **kw)
    ctx.synchronize()
    return {k: v.download() for k, v in out.items()}, {m: v.download() for m, v in band.items()}, {k: v.download() for k, v in comp.items()}


@pytest.mark.parametrize("which,mcica", [("sw", False), ("sw", True), ("lw", False), ("lw", True)])
def test_plain_outputs_unchanged(gpu_ctx, which, mcica):
    """The plain outputs of a band call (and of a components + bands call) are the bits of a plain call: host and device
    pointers; the band arrays are the same bits through both kinds of pointers."""
    c = _grid(700, 40, 21, mcica)
    call = _call(gpu_ctx, which)
    plain = call(c, mcica=mcica)
    band = B.band_arrays(which, 40, 700)
    withb = call(c, mcica=mcica, bands=band)
    assert all(np.array_equal(withb[k], plain[k]) for k in plain)
    dplain, _, _ = _device_call(gpu_ctx, which, c, mcica, bands=False)
    dout, dband, _ = _device_call(gpu_ctx, which, c, mcica)
    assert all(np.array_equal(dout[k], plain[k]) and np.array_equal(dplain[k], plain[k]) for k in plain)
    assert all(np.array_equal(dband[m], band[m]) for m in band)
    if which == "sw":
        comp = {k: np.zeros((41, 700)) for k in SW_COMPONENTS}
        conly = {k: np.zeros((41, 700)) for k in SW_COMPONENTS}
        call(c, mcica=mcica, components=conly)
        band2 = B.band_arrays(which, 40, 700)
        both = call(c, mcica=mcica, components=comp, bands=band2)
        assert all(np.array_equal(both[k], plain[k]) for k in plain)
        assert all(np.array_equal(comp[k], conly[k]) for k in comp) and all(np.array_equal(band2[m], band[m]) for m in band)
        dout, dband, dcomp = _device_call(gpu_ctx, which, c, mcica, components=True)
        assert all(np.array_equal(dout[k], plain[k]) for k in plain)
        assert all(np.array_equal(dcomp[k], conly[k]) for k in comp) and all(np.array_equal(dband[m], band[m]) for m in band)
    # an empty request is the plain call
    assert all(np.array_equal(call(c, mcica=mcica, bands={})[k], plain[k]) for k in plain)


def _sum_bound(which, out, band):
    for m, k in B.BROADBAND[which].items():
        assert band[m].min() >= 0.0, m
        err = np.abs(band[m].sum(axis=0) - out[k])
        assert np.all(err <= B.SUM_BOUND * np.abs(out[k])), (which, m, float((err / np.maximum(np.abs(out[k]), 1e-300)).max()))


def _identities(which, c, out, band, comp=None):
    nlay = c["play"].shape[0]
    _sum_bound(which, out, band)
    clear = ~(c["cldfr"] > 0).any(axis=0)
    assert clear.any() and not clear.all()
    assert np.array_equal(band["upc"][:, :, clear], band["up"][:, :, clear])
    assert np.array_equal(band["dnc"][:, :, clear], band["dn"][:, :, clear])
    if which == "sw":
        assert np.all(band["dndir"] <= band["dn"] + 1e-9) and np.all(band["dndirc"] <= band["dnc"] + 1e-9)
        assert np.array_equal(band["dndirc"][:, :, clear], band["dndir"][:, :, clear])
        assert np.array_equal(band["dndir"][:, nlay], band["dn"][:, nlay])      # nothing diffuse comes in at the top
        # bands 9..12 are the UV/visible bands of the components
        uv, uvdir = comp["dirdnuv"] + comp["difdnuv"], comp["dirdnuv"]
        assert np.all(np.abs(band["dn"][9:13].sum(axis=0) - uv) <= B.SUM_BOUND * np.abs(uv))
        assert np.all(np.abs(band["dndir"][9:13].sum(axis=0) - uvdir) <= B.SUM_BOUND * np.abs(uvdir))
    else:
        assert np.all(band["dn"][:, nlay] == 0.0)      # no downward longwave at the top


@pytest.mark.parametrize("which,ncol,nlay,mcica,icld", [("sw", 16384, 60, True, 2), ("sw", 4096, 100, False, 1),
                                                         ("lw", 16384, 60, True, 1), ("lw", 4096, 100, False, 2), ("lw", 4096, 60, False, 1)])
def test_identities_on_large_grids(gpu_ctx, which, ncol, nlay, mcica, icld):
    c = _grid(ncol, nlay, 23, mcica, icld)
    band = B.band_arrays(which, nlay, ncol)
    comp = {k: np.zeros((nlay + 1, ncol)) for k in ("dirdnuv", "difdnuv")} if which == "sw" else None
    kw = dict(components=comp) if comp else {}
    out = _call(gpu_ctx, which)(c, mcica=mcica, bands=band, **kw)
    _identities(which, c, out, band, comp)


def test_longwave_clear_sky_and_night_columns(gpu_ctx):
    c = _grid(256, 60, 29, False)
    c.update(icld=0)
    band = B.band_arrays("lw", 60, 256)
    out = gpu_ctx.lw_fluxes(c, bands=band)
    _sum_bound("lw", out, band)
    assert np.array_equal(band["upc"], band["up"]) and np.array_equal(band["dnc"], band["dn"])
    c = _grid(256, 60, 29, True)
    cz = c["coszen"].copy(); cz[::3] = 0.0; cz[1::3] = -0.2
    c["coszen"] = cz
    band = B.band_arrays("sw", 60, 256)
    gpu_ctx.sw_fluxes(c, mcica=True, bands=band)
    for m in B.MEMBERS["sw"]:      # night: zero, as far as the reference's clamp of cos(zenith) at 1e-10 lets it be (B.NIGHT_ZERO)
        assert np.all(np.abs(band[m][:, :, ::3]) <= B.NIGHT_ZERO) and np.all(np.abs(band[m][:, :, 1::3]) <= B.NIGHT_ZERO), m
    assert band["dn"][:, :, 2::3].max() > 1.0


@pytest.mark.parametrize("which", ["sw", "lw"])
def test_chunks_shards_subsets_and_sort(gpu_ctx, monkeypatch, which):
    from climt_amd._lib import Context
    from climt_amd.distributed import slice_columns
    from helpers import CONSTANTS, CPDAIR
    c = _grid(1000, 40, 25, True)
    call = _call(gpu_ctx, which)
    full = B.band_arrays(which, 40, 1000)
    call(c, mcica=True, bands=full)
    # tile-aligned shards: kissvec, and the Mersenne twister (one positional stream: shard_col0 / shard_ncol place the shard)
    for irng in (0, 1):
        cc = dict(c, irng=irng)
        whole = full
        if irng:
            whole = B.band_arrays(which, 40, 1000)
            call(cc, mcica=True, bands=whole)
        for lo, hi in ((0, 384), (384, 1000)):
            sub = slice_columns(cc, lo, hi); sub.update(shard_col0=lo, shard_ncol=1000)
            part = B.band_arrays(which, 40, hi - lo)
            call(sub, mcica=True, bands=part)
            assert all(np.array_equal(part[m], whole[m][:, :, lo:hi]) for m in part), (irng, lo, hi)
    # a subset of the members
    some = B.band_arrays(which, 40, 1000, members=("upc", "dndir") if which == "sw" else ("dn",))
    call(c, mcica=True, bands=some)
    assert all(np.array_equal(some[m], full[m]) for m in some)
    two = B.band_arrays(which, 40, 1000, "boundaries", members=("dn",))
    call(c, mcica=True, bands=two, band_levels="boundaries")
    assert np.array_equal(two["dn"][:, 0], full["dn"][:, 0]) and np.array_equal(two["dn"][:, 1], full["dn"][:, 40])
    # column sort on: band calls are not sorted, the bits stay
    try:
        gpu_ctx.set_column_sort(True)
        _, sorted_band, _ = _device_call(gpu_ctx, which, c, True)
    finally:
        gpu_ctx.set_column_sort(False)
    assert all(np.array_equal(sorted_band[m], full[m]) for m in full)
    # smaller column chunks, in a fresh context
    monkeypatch.setenv("RRTMG_HIP_CHUNK_TILES", "2")
    small = Context(0); small.set_constants(**CONSTANTS)
    (small.sw_init if which == "sw" else small.lw_init)(CPDAIR)
    ch = B.band_arrays(which, 40, 1000)
    (small.sw_fluxes if which == "sw" else small.lw_fluxes)(c, mcica=True, bands=ch)
    small.close()
    assert all(np.array_equal(ch[m], full[m]) for m in full)


def test_bad_requests_are_refused(gpu_ctx):
    from climt_amd._lib import LwArgs, LwBandFluxes, SwArgs, SwBandFluxes
    c = _grid(64, 20, 3, False)
    lib = gpu_ctx.lib
    keep = np.zeros((16, 21, 64))
    for S, A, fn in ((SwBandFluxes, SwArgs, lambda a, b: lib.rrtmg_hip_sw_fluxes_bands(gpu_ctx.h, C.byref(a), None, C.byref(b))),
                     (LwBandFluxes, LwArgs, lambda a, b: lib.rrtmg_hip_lw_fluxes_bands(gpu_ctx.h, C.byref(a), C.byref(b)))):
        a = A(); a.struct_size = C.sizeof(A)
        bad = S(); bad.struct_size = C.sizeof(S) - 8; bad.up = keep.ctypes.data
        assert fn(a, bad) != 0 and "struct_size" in lib.rrtmg_hip_last_error(gpu_ctx.h).decode()
        bad = S(); bad.struct_size = C.sizeof(S); bad.levels = 2; bad.up = keep.ctypes.data
        assert fn(a, bad) != 0 and "levels" in lib.rrtmg_hip_last_error(gpu_ctx.h).decode()
        bad = S(); bad.struct_size = C.sizeof(S); bad.levels = -1      # refused even without a member
        assert fn(a, bad) != 0 and "levels" in lib.rrtmg_hip_last_error(gpu_ctx.h).decode()
    with pytest.raises(KeyError):
        gpu_ctx.sw_fluxes(c, bands={"upwards": np.zeros((14, 21, 64))})
    with pytest.raises(KeyError):
        gpu_ctx.lw_fluxes(c, bands={"dndir": np.zeros((16, 21, 64))})
    with pytest.raises(ValueError):
        gpu_ctx.lw_fluxes(c, bands={"up": np.zeros((16, 21, 64))}, band_levels="top")
    for which in ("sw", "lw"):      # the context stays usable
        band = B.band_arrays(which, 20, 64)
        out = _call(gpu_ctx, which)(c, bands=band)
        _sum_bound(which, out, band)
    from climt_amd._lib import band_limits
    lo, hi = band_limits("lw")      # the longwave weights its bands with hi - lo
    assert np.array_equal(gpu_ctx.get_table("lw/wvn/delwave"), hi - lo)


@pytest.mark.parametrize("mcica", [False, True])
def test_components_on_device_state_equal_host(mcica):
    import climt_amd
    from climt_amd.rrtmg import longwave, shortwave
    from helpers import load_cache_case
    states = {"sw": load_cache_case("TestRRTMGShortwaveMCICA", "3d")[0], "lw": load_cache_case("TestRRTMGLongwaveMCICA", "3d")[0]}
    sw = shortwave.RRTMGShortwave(mcica=mcica, cloud_overlap_method="maximum_random" if mcica else "clear_only",
                                  random_number_generator="kissvec", band_fluxes=True)
    lw = longwave.RRTMGLongwave(mcica=mcica, cloud_overlap_method="random", random_number_generator="kissvec", band_fluxes=True,
                                allow_synthetic_tables=True)
    assert sw.diagnostic_properties == shortwave.RRTMGShortwave.diagnostic_properties_for(band_fluxes=True)
    assert lw.diagnostic_properties == longwave.RRTMGLongwave.diagnostic_properties_for(band_fluxes=True)
    assert shortwave.RRTMGShortwave(mcica=mcica).diagnostic_properties is shortwave.RRTMGShortwave.diagnostic_properties
    assert longwave.RRTMGLongwave(mcica=mcica, allow_synthetic_tables=True).diagnostic_properties is longwave.RRTMGLongwave.diagnostic_properties
    for comp, mod, nband, dim, broadband in ((sw, shortwave, 14, "num_shortwave_bands", "downwelling_shortwave_flux_in_air"),
                                             (lw, longwave, 16, "num_longwave_bands", "upwelling_longwave_flux_in_air")):
        state = states["sw" if comp is sw else "lw"]
        np.random.seed(3)
        _, host = comp(state)
        ds = climt_amd.DeviceState.from_host(state, [comp])
        np.random.seed(3)
        _, dev = comp(ds)
        ds.ctx.synchronize()
        for k in list(mod.BAND_FLUX_DIAGNOSTICS) + [broadband]:
            h, d = host[k], dev[k]
            got = d.buf.download().reshape(d.shape)
            if k != broadband:
                assert h.dims[0] == dim and h.dims[1] == "interface_levels" and h.values.shape[0] == nband, (k, h.dims)
                assert tuple(d.dims) == (dim, "interface_levels", "*") and got.shape[0] == nband
            assert np.array_equal(got, np.asarray(h.values).reshape(got.shape)), k
        by_band = np.asarray(host[broadband + "_by_band"].values)
        total = np.asarray(host[broadband].values)
        assert np.all(np.abs(by_band.sum(axis=0) - total) <= B.SUM_BOUND * np.abs(total))
        assert float(np.abs(by_band).max()) > 1.0
        ds.close()
