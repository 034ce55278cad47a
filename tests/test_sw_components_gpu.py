"""GPU tests of the shortwave flux components (rrtmg_hip_sw_fluxes_components; run with -m gpu on an MI355X): the committed
reference fixtures (tests/swcomp_cases.py), the plain outputs unchanged by the components path, identities on large grids,
chunking, shards, column sort, subsets of the members, struct_size, and RRTMGShortwave(flux_components=True) on a DeviceState."""
import ctypes as C

import numpy as np
import pytest

import swcomp_cases as S
from helpers import maxdiff

pytestmark = pytest.mark.gpu

TIGHT = 5.0e-9
BASE = dict(icld=1, iaer=0, adjes=1.0, dyofyr=1, scon=1367.0, isolvar=0, inflg=2, iceflg=1, liqflg=1)


def _comp(nlay, ncol, want=S.COMPONENTS):
    return {k: np.zeros((nlay + 1, ncol)) for k in want}


@pytest.mark.parametrize("case", list(S.CASES))
def test_components_vs_reference_fixture(gpu_ctx, case):
    c, mcica, exp = S.load_case(case)
    nlay, ncol = c["play"].shape
    comp = _comp(nlay, ncol)
    out = gpu_ctx.sw_fluxes(c, mcica=mcica, components=comp)
    for k in S.COMPONENTS:
        assert maxdiff(comp[k], exp[k]) <= TIGHT, (case, k, maxdiff(comp[k], exp[k]))
    for k in S.BROADBAND:
        assert maxdiff(out[k], exp[k]) <= TIGHT, (case, k)


def _grid(ncol, nlay, seed, mcica):
    from climt_amd.synthetic import make_columns, overcast
    c = make_columns(ncol, nlay, cloudy=True, seed=seed); c.pop("lat")
    # every fourth 64-column tile cloud-free: both solve variants in one call
    for t in range(0, (ncol + 63) // 64, 4):
        for k in ("cldfr", "cliqwp", "cicewp"):
            c[k][:, t * 64:(t + 1) * 64] = 0.0
    if not mcica:
        c = overcast(c)
    c.update(BASE); c.update(irng=0, permuteseed=11, icld=2 if mcica else 1)
    return c


def _device_call(ctx, c, mcica, want=S.COMPONENTS, plain=False):
    from climt_amd import _hip
    from climt_amd._lib import SW_OUT
    nlay, ncol = c["play"].shape
    dev = {k: _hip.DeviceArray.from_host(v) for k, v in c.items() if isinstance(v, np.ndarray)}
    args = {k: v.ptr for k, v in dev.items()}
    args.update({k: v for k, v in c.items() if not isinstance(v, np.ndarray)}); args.update(ncol=ncol, nlay=nlay)
    out = {k: _hip.DeviceArray((nlay + lev, ncol)) for k, lev in SW_OUT}
    comp = {k: _hip.DeviceArray((nlay + 1, ncol)) for k in want}
    ctx.sw_fluxes(args, mcica=mcica, out={k: v.ptr for k, v in out.items()}, memspace=1,
                  components=None if plain else {k: v.ptr for k, v in comp.items()})
    ctx.synchronize()
    return {k: v.download() for k, v in out.items()}, ({} if plain else {k: v.download() for k, v in comp.items()})


@pytest.mark.parametrize("mcica", [False, True])
def test_plain_outputs_unchanged(gpu_ctx, mcica):
    """The six outputs of a components call are the bits of a plain call: host and device pointers."""
    c = _grid(700, 40, 21, mcica)
    plain = gpu_ctx.sw_fluxes(c, mcica=mcica)
    comp = _comp(40, 700)
    withc = gpu_ctx.sw_fluxes(c, mcica=mcica, components=comp)
    assert all(np.array_equal(withc[k], plain[k]) for k in plain)
    dplain, _ = _device_call(gpu_ctx, c, mcica, plain=True)
    dout, dcomp = _device_call(gpu_ctx, c, mcica)
    assert all(np.array_equal(dout[k], plain[k]) and np.array_equal(dplain[k], plain[k]) for k in plain)
    assert all(np.array_equal(dcomp[k], comp[k]) for k in comp)


def _identities(c, out, comp, mcica):
    nlay = c["play"].shape[0]
    for k in ("difdflx", "difdnuv", "difdnir", "difdflxc"):
        assert comp[k].min() >= -1e-9, (k, comp[k].min())
    assert np.array_equal(comp["difdflx"], out["swdflx"] - comp["dirdflx"])
    assert np.array_equal(comp["difdflxc"], out["swdflxc"] - comp["dirdflxc"])
    assert np.all(comp["difdflx"][nlay] == 0.0)
    for a, b, t in (("dirdnuv", "dirdnir", "dirdflx"), ("difdnuv", "difdnir", "difdflx")):
        s = comp[a] + comp[b]
        assert np.all(np.abs(s - comp[t]) <= 1e-10 * np.maximum(np.abs(comp[t]), 1e-3)), (t, maxdiff(s, comp[t]))
    clear = ~(c["cldfr"] > 0).any(axis=0)
    assert clear.any()
    assert np.array_equal(comp["dirdflxc"][:, clear], comp["dirdflx"][:, clear])
    assert np.array_equal(comp["difdflxc"][:, clear], comp["difdflx"][:, clear])


@pytest.mark.parametrize("ncol,nlay,mcica", [(16384, 60, True), (4096, 100, False)])
def test_identities_on_large_grids(gpu_ctx, ncol, nlay, mcica):
    c = _grid(ncol, nlay, 23, mcica)
    comp = _comp(nlay, ncol)
    out = gpu_ctx.sw_fluxes(c, mcica=mcica, components=comp)
    _identities(c, out, comp, mcica)


def test_chunks_shards_subsets_and_sort(gpu_ctx, monkeypatch):
    from climt_amd._lib import Context
    from climt_amd.distributed import slice_columns
    from helpers import CONSTANTS, CPDAIR
    c = _grid(1000, 40, 25, True)
    full = _comp(40, 1000)
    gpu_ctx.sw_fluxes(c, mcica=True, components=full)
    # tile-aligned shards
    for lo, hi in ((0, 384), (384, 1000)):
        sub = slice_columns(c, lo, hi); sub.update(shard_col0=lo, shard_ncol=1000)
        part = _comp(40, hi - lo)
        gpu_ctx.sw_fluxes(sub, mcica=True, components=part)
        assert all(np.array_equal(part[k], full[k][:, lo:hi]) for k in part), (lo, hi)
    # a subset of the members
    some = _comp(40, 1000, ("dirdnir", "difdflxc"))
    gpu_ctx.sw_fluxes(c, mcica=True, components=some)
    assert all(np.array_equal(some[k], full[k]) for k in some)
    # column sort on: components calls are not sorted, the bits stay
    try:
        gpu_ctx.set_column_sort(True)
        _, sorted_comp = _device_call(gpu_ctx, c, True)
    finally:
        gpu_ctx.set_column_sort(False)
    assert all(np.array_equal(sorted_comp[k], full[k]) for k in full)
    # smaller column chunks
    monkeypatch.setenv("RRTMG_HIP_CHUNK_TILES", "2")
    small = Context(0); small.set_constants(**CONSTANTS); small.sw_init(CPDAIR)
    ch = _comp(40, 1000)
    small.sw_fluxes(c, mcica=True, components=ch)
    small.close()
    assert all(np.array_equal(ch[k], full[k]) for k in full)


def test_struct_size_is_checked(gpu_ctx):
    from climt_amd._lib import RRTMGError, SwArgs, SwComponents
    c = _grid(64, 20, 3, False)
    lib = gpu_ctx.lib
    bad = SwComponents(); bad.struct_size = C.sizeof(SwComponents) - 8
    a = SwArgs(); a.struct_size = C.sizeof(SwArgs)
    rc = lib.rrtmg_hip_sw_fluxes_components(gpu_ctx.h, C.byref(a), C.byref(bad))
    assert rc != 0 and "struct_size" in lib.rrtmg_hip_last_error(gpu_ctx.h).decode()
    with pytest.raises(KeyError):
        gpu_ctx.sw_fluxes(c, components={"dirdflux": np.zeros((21, 64))})
    plain = gpu_ctx.sw_fluxes(c)                   # the context stays usable; an empty request is the plain call
    assert all(np.array_equal(gpu_ctx.sw_fluxes(c, components={})[k], plain[k]) for k in plain)
    assert not isinstance(RRTMGError(1, "x"), KeyError)


@pytest.mark.parametrize("mcica", [False, True])
def test_component_on_device_state_equals_host(mcica):
    import climt_amd
    from climt_amd.rrtmg.shortwave import FLUX_COMPONENT_DIAGNOSTICS, RRTMGShortwave
    from helpers import load_cache_case
    state, _, _ = load_cache_case("TestRRTMGShortwaveMCICA", "3d")
    sw = RRTMGShortwave(mcica=mcica, cloud_overlap_method="maximum_random" if mcica else "clear_only",
                        random_number_generator="kissvec", flux_components=True)
    assert sw.diagnostic_properties == RRTMGShortwave.diagnostic_properties_for(True)
    assert RRTMGShortwave(mcica=mcica).diagnostic_properties is RRTMGShortwave.diagnostic_properties
    np.random.seed(3)
    _, host = sw(state)
    ds = climt_amd.DeviceState.from_host(state, [sw])
    np.random.seed(3)
    _, dev = sw(ds)
    ds.ctx.synchronize()
    for k in list(FLUX_COMPONENT_DIAGNOSTICS) + ["downwelling_shortwave_flux_in_air"]:
        h, d = host[k], dev[k]
        assert h.dims[0] == "interface_levels"
        got = d.buf.download().reshape(d.shape)
        assert np.array_equal(got, np.asarray(h.values).reshape(got.shape)), k
    assert float(np.abs(np.asarray(host["downwelling_diffuse_shortwave_flux_in_air"].values)).max()) > 1.0
    ds.close()
