"""GPU tests of the longwave call without the clear-sky outputs (rrtmg_hip_set_lw_clear_sky(ctx, 0); run with -m gpu on an
MI355X): the committed reference-Fortran fixtures, the default call of the same library on grids without a fixture, chunks,
shards, the column sort, the joint and the deferred call, band fluxes, the switch back and the component.

Bounds: TIGHT against a fixture (the project's bound against the reference Fortran).  Against the default call of the same
library both calls are within TIGHT of the reference, so 2 x TIGHT would follow without a new number; the largest difference
measured over this file on an MI355X is 0 in every case (cloudy tiles included: the one-stream instantiation performs the
total-sky operations of the two-stream one), so equality is asserted, and every comparison prints the difference it found."""
import numpy as np
import pytest

from helpers import CONSTANTS, CPDAIR, LWMR_CASES, REF_CASES, load_lwmr_case, load_ref_case, maxdiff

pytestmark = pytest.mark.gpu

TIGHT = 5.0e-9
ALLSKY = ("uflx", "dflx", "hr")
CLEAR = ("uflxc", "dflxc", "hrc")
RRTMG_ERR_ARG = 4
FLAGS = dict(iaer=0, inflg=2, iceflg=1, liqflg=1, irng=0, permuteseed=11)


def _context():
    from climt_amd._lib import Context
    ctx = Context(0)
    ctx.set_constants(**CONSTANTS)
    ctx.lw_init(CPDAIR)
    return ctx


@pytest.fixture(scope="module")
def as_ctx():
    """A context of its own with the longwave clear-sky outputs off (gpu_ctx, which the whole session shares, keeps its default)."""
    ctx = _context()
    ctx.set_lw_clear_sky(False)
    yield ctx
    ctx.close()


def _shape(c):
    return (c["nlay"], c["ncol"]) if "ncol" in c else c["play"].shape


def _keys(c, keys):
    """The output names of a call: `keys`, and the derivative arrays that go with them under idrv."""
    if not c.get("idrv"):
        return tuple(keys)
    return tuple(keys) + ("duflx_dt",) + (("duflxc_dt",) if "uflxc" in keys else ())


def _nan(nlay, ncol, k):
    return np.full((nlay + (k not in ("hr", "hrc")), ncol), np.nan)


def host_call(ctx, c, mcica, keys=ALLSKY + CLEAR, **kw):
    """One host-pointer call into NaN-filled arrays for `keys` -> {name: array}."""
    nlay, ncol = _shape(c)
    out = {k: _nan(nlay, ncol, k) for k in _keys(c, keys)}
    ctx.lw_fluxes(c, mcica=mcica, out=out, **kw)
    return out


def device_call(ctx, c, mcica, keys=ALLSKY + CLEAR, deferred=False):
    """One device-pointer call into NaN-filled device buffers for `keys` -> {name: downloaded array}."""
    from climt_amd import _hip
    nlay, ncol = _shape(c)
    dev = {k: _hip.DeviceArray.from_host(v) for k, v in c.items() if isinstance(v, np.ndarray)}
    args = {k: v.ptr for k, v in dev.items()}
    args.update({k: v for k, v in c.items() if not isinstance(v, np.ndarray)}); args.update(ncol=ncol, nlay=nlay)
    dout = {k: _hip.DeviceArray.from_host(_nan(nlay, ncol, k)) for k in _keys(c, keys)}
    if deferred:
        ctx.set_deferred(True)
    try:
        ctx.lw_fluxes(args, mcica=mcica, out={k: v.ptr for k, v in dout.items()}, memspace=1)
        ctx.synchronize()      # (deferred mode: raises if the call left an error)
    finally:
        if deferred:
            ctx.set_deferred(False)
    return {k: v.download() for k, v in dout.items()}


def assert_clear_untouched(out, what=""):
    """The NaN pattern the clear-sky arrays were filled with is still there, bit for bit."""
    for k in out:
        if k in CLEAR or k == "duflxc_dt":
            assert np.array_equal(out[k].view(np.uint64), np.full(out[k].shape, np.nan).view(np.uint64)), (what, k, "a clear-sky output was written")


def _allsky(out):
    return [k for k in out if k in ALLSKY or k == "duflx_dt"]


def assert_close(got, want, bound, what=""):
    worst = 0.0
    for k in _allsky(got):
        assert np.isfinite(got[k]).all(), (what, k)
        d = maxdiff(got[k], want[k])
        worst = max(worst, d)
        print("%s %s: max |d| = %.3e (bound %.1e)" % (what, k, d, bound))
        assert d <= bound, (what, k, d)
    return worst


def assert_vs_default(got, want, what=""):
    """Against the default call of the same library: the difference is printed, and the bits are demanded (measured: 0)."""
    for k in _allsky(got):
        assert np.isfinite(got[k]).all(), (what, k)
        d = maxdiff(got[k], want[k])
        print("%s %s: max |d| vs the default call = %.3e" % (what, k, d))
        assert np.array_equal(got[k], want[k]), (what, k, d)


def assert_same_bits(got, want, what=""):
    for k in _allsky(got):
        assert np.array_equal(got[k], want[k]), (what, k, maxdiff(got[k], want[k]))


def _fixtures():
    return [("ref", n) for n in REF_CASES if not n.startswith("clear")] + [("lwmr", n) for n in LWMR_CASES]


def _load(kind, case):
    if kind == "ref":
        c, mcica, exp = load_ref_case(case)
        return c, mcica, exp["lw"]
    c, exp = load_lwmr_case(case)
    return c, False, exp


# ---- 1. fixtures ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,case", _fixtures())
def test_fixtures(gpu_ctx, as_ctx, kind, case):
    c, mcica, exp = _load(kind, case)
    assert (np.asarray(c["cldfr"]) > 0).any() and float(np.abs(exp["dflx"] - exp["dflxc"]).max()) > 1.0
    host = host_call(as_ctx, c, mcica)
    assert ("duflx_dt" in host) == (case == "maxrand_idrv")
    assert_close(host, exp, TIGHT, case + " host vs reference")
    assert_clear_untouched(host, case + " host")
    dev = device_call(as_ctx, c, mcica)
    assert_close(dev, exp, TIGHT, case + " device vs reference")
    assert_clear_untouched(dev, case + " device")
    assert_same_bits(dev, host, case)
    assert_vs_default(host, host_call(gpu_ctx, c, mcica), case)
    # the clear-sky pointers NULL: status 0 (an exception otherwise), the same bits
    assert_same_bits(host_call(as_ctx, c, mcica, keys=ALLSKY), host, case + " NULL host")
    assert_same_bits(device_call(as_ctx, c, mcica, keys=ALLSKY), host, case + " NULL device")


# ---- 2. mixed grid ---------------------------------------------------------------------------------------------------------------
def _grid(ncol, nlay, seed):
    """Tile 0 cloud-free, the other full tiles with cloud, and of the ragged last tile's columns only the last one cloudy."""
    from climt_amd.synthetic import make_columns
    c = make_columns(ncol, nlay, cloudy=True, seed=seed); c.pop("lat")
    src = 64 + int(np.argmax((c["cldfr"][:, 64:128] > 0).sum(axis=0)))      # the cloudiest column of tile 1
    last = (ncol - 1) // 64 * 64
    for k in ("cldfr", "cliqwp", "cicewp"):
        c[k][:, :64] = 0.0
        if last >= 128:
            c[k][:, last:] = 0.0
            c[k][:, ncol - 1] = c[k][:, src]
    c.update(FLAGS)
    return c


def _mixed(variant):
    c = _grid(130, 30, 27)
    mcica = variant.startswith("mcica")
    c.update({"mcica_random": dict(icld=1), "mcica_maxrand": dict(icld=2), "rtrnmr_idrv": dict(icld=2, idrv=1), "random_fractional": dict(icld=1)}[variant])
    cld = c["cldfr"]
    assert not (cld[:, :64] > 0).any() and (cld[:, 64:128] > 0).any() and not (cld[:, 128] > 0).any() and (cld[:, 129] > 0).any()
    if not mcica:
        frac = cld[cld > 0]
        assert ((frac > 1.0e-6) & (frac < 1.0)).any()      # fractional cloud: the cfrac / efclfrac blend, rtrnmr's overlap factors
    return c, mcica


MIXED = ("mcica_random", "mcica_maxrand", "rtrnmr_idrv", "random_fractional")


@pytest.mark.parametrize("variant", MIXED)
def test_mixed_grid_against_the_default_call(gpu_ctx, as_ctx, variant):
    """130 columns x 30 layers: a cloud-free tile, a cloudy one, a ragged one of two columns (one cloudy); 30 layers leave a
    2-layer tail in the upward sweep's 4-layer blocks."""
    c, mcica = _mixed(variant)
    want = host_call(gpu_ctx, c, mcica)
    got = host_call(as_ctx, c, mcica)
    assert ("duflx_dt" in got) == (variant == "rtrnmr_idrv")
    for k in _allsky(got):      # the cloud-free tile runs the same device functions in both calls
        assert np.array_equal(got[k][:, :64], want[k][:, :64]), (variant, k)
    assert_vs_default(got, want, variant)      # ... and the tiles with cloud, in the one-stream instantiation, the same operations
    assert_clear_untouched(got, variant)
    assert float(np.abs(want["dflx"] - want["dflxc"]).max()) > 1.0
    dev = device_call(as_ctx, c, mcica)
    assert_same_bits(dev, got, variant + " device")
    assert_clear_untouched(dev, variant + " device")


# ---- 3. mask-word boundary ---------------------------------------------------------------------------------------------------------
def test_two_mask_words(gpu_ctx, as_ctx):
    from climt_amd.synthetic import make_columns
    c = make_columns(66, 70, cloudy=True, seed=31); c.pop("lat")
    c.update(FLAGS); c.update(icld=2)
    # (the generator's clouds stay below layer 64 of 70: the cloud fields of layers 8-13 once more in layers 62-67, so that set
    #  mask bits sit on both sides of the word boundary)
    for k in ("cldfr", "cliqwp", "cicewp"):
        c[k][62:68] = c[k][8:14]
    assert (c["cldfr"][64:] > 0).any() and (c["cldfr"][:64] > 0).any() and (c["cldfr"][62:64] > 0).any()
    assert (c["cldfr"][:, :64] > 0).any() and (c["cldfr"][:, 64:] > 0).any()      # both tiles with cloud
    want = host_call(gpu_ctx, c, True)
    got = host_call(as_ctx, c, True)
    assert_vs_default(got, want, "66x70")
    assert_clear_untouched(got)
    assert float(np.abs(want["dflx"] - want["dflxc"]).max()) > 1.0


# ---- 4. chunks and shards ---------------------------------------------------------------------------------------------------------
def test_chunks_and_shards(as_ctx, monkeypatch):
    from climt_amd.distributed import slice_columns
    c, _ = _mixed("mcica_maxrand")
    c.update(irng=1, permuteseed=1234)      # the Mersenne twister: one positional stream over the whole grid
    whole = host_call(as_ctx, c, True)
    parts = []
    for lo, hi in ((0, 64), (64, 130)):
        sub = slice_columns(c, lo, hi); sub.update(shard_col0=lo, shard_ncol=130)
        parts.append(host_call(as_ctx, sub, True))
        assert_clear_untouched(parts[-1], (lo, hi))
    for k in ALLSKY:
        assert np.array_equal(np.concatenate([p[k] for p in parts], axis=1), whole[k]), k
    monkeypatch.setenv("RRTMG_HIP_CHUNK_TILES", "1")
    small = _context()
    try:
        small.set_lw_clear_sky(False)
        ch = host_call(small, c, True)
        assert small.kernel_launches("lw") >= 3      # 3 tiles in chunks of 1
        ch_dev = device_call(small, c, True)
    finally:
        small.close()
    assert_same_bits(ch, whole, "chunks")
    assert_same_bits(ch_dev, whole, "chunks, device")
    assert_clear_untouched(ch, "chunks")
    assert_clear_untouched(ch_dev, "chunks, device")


# ---- 5. column sort ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", ["mcica_random", "rtrnmr_idrv"])
def test_column_sort(as_ctx, variant):
    """The column sort runs the call on a permuted copy: no scatter entry for the absent outputs (the NaN pattern stays), a
    cloudy column the bits of the unsorted call, a cloud-free column within the sort's 1e-10 (it may change solve variant)."""
    c, mcica = _mixed(variant)
    cloudy = (c["cldfr"] > 0).any(axis=0)
    want = device_call(as_ctx, c, mcica)
    as_ctx.set_column_sort(True)
    try:
        got = device_call(as_ctx, c, mcica)
        null = device_call(as_ctx, c, mcica, keys=ALLSKY)
    finally:
        as_ctx.set_column_sort(False)
    assert_clear_untouched(got, variant)
    for k in _allsky(got):
        assert np.isfinite(got[k]).all(), k
        assert np.array_equal(got[k][:, cloudy], want[k][:, cloudy]), k
        assert maxdiff(got[k][:, ~cloudy], want[k][:, ~cloudy]) <= 1.0e-10, k
    assert_same_bits(null, got, variant + " NULL")


# ---- 6. joint and deferred ---------------------------------------------------------------------------------------------------------
def test_joint_and_deferred(gpu_ctx, as_ctx):
    from climt_amd._lib import SW_OUT
    c, _ = _mixed("mcica_maxrand")
    c.update(dyofyr=1, scon=1367.0, isolvar=0, adjes=1.0)
    nlay, ncol = c["play"].shape
    sw_keys = [k for k, _ in SW_OUT]
    nan_sw = lambda: {k: np.full((nlay + lev, ncol), np.nan) for k, lev in SW_OUT}
    ctx = _context()
    try:
        ctx.sw_init(CPDAIR)
        # longwave switch 0, shortwave switch 1
        ctx.set_lw_clear_sky(False)
        lw_sep = host_call(ctx, c, True)
        sw_sep = ctx.sw_fluxes(c, mcica=True, out=nan_sw())
        lw_out = {k: _nan(nlay, ncol, k) for k in ALLSKY + CLEAR}
        sw_out = nan_sw()
        ctx.radiation_fluxes(sw=dict(inp=c, mcica=True, out=sw_out), lw=dict(inp=c, mcica=True, out=lw_out))
        assert_same_bits(lw_out, lw_sep, "joint, lw 0 / sw 1")
        assert_clear_untouched(lw_out, "joint")
        assert all(np.array_equal(sw_out[k], sw_sep[k]) for k in sw_keys)      # all six shortwave outputs, the default's
        assert_same_bits(lw_sep, host_call(as_ctx, c, True), "two contexts")
        # the other way round
        ctx.set_lw_clear_sky(True); ctx.set_sw_clear_sky(False)
        lw_sep = host_call(ctx, c, True)
        sw_sep = ctx.sw_fluxes(c, mcica=True, out={k: v for k, v in nan_sw().items() if not k.endswith("c")})
        lw_out = {k: _nan(nlay, ncol, k) for k in ALLSKY + CLEAR}
        sw_out = nan_sw()
        ctx.radiation_fluxes(sw=dict(inp=c, mcica=True, out=sw_out), lw=dict(inp=c, mcica=True, out=lw_out))
        for k in ALLSKY + CLEAR:
            assert np.array_equal(lw_out[k], lw_sep[k]), k
        want = host_call(gpu_ctx, c, True)
        for k in ALLSKY + CLEAR:      # the longwave of a context whose SHORTWAVE switch is 0 is the default longwave
            assert np.array_equal(lw_out[k], want[k]), k
        for k in sw_keys:
            if k.endswith("c"):
                assert np.isnan(sw_out[k]).all(), k
            else:
                assert np.array_equal(sw_out[k], sw_sep[k]), k
    finally:
        ctx.close()
    plain = host_call(as_ctx, c, True)
    dev = device_call(as_ctx, c, True, deferred=True)      # (synchronize() inside raises on an error)
    assert_same_bits(dev, plain, "deferred")
    assert_clear_untouched(dev, "deferred")


# ---- 7. band fluxes -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("levels", ["all", "boundaries"])
def test_band_fluxes(gpu_ctx, as_ctx, levels):
    from climt_amd._lib import RRTMGError
    c, mcica = _mixed("mcica_maxrand")
    nlay, ncol = c["play"].shape
    nrow = 2 if levels == "boundaries" else nlay + 1
    band = lambda *names: {n: np.full((16, nrow, ncol), np.nan) for n in names}
    never = _context()
    try:
        never.set_lw_clear_sky(False)
        untouched = host_call(never, c, mcica)
    finally:
        never.close()
    before = host_call(as_ctx, c, mcica)
    for names in (("upc",), ("dnc",), ("up", "dn", "upc", "dnc")):
        b = band(*names)
        with pytest.raises(RRTMGError) as e:
            host_call(as_ctx, c, mcica, bands=b, band_levels=levels)
        assert e.value.code == RRTMG_ERR_ARG and "rrtmg_hip_set_lw_clear_sky" in str(e.value), str(e.value)
        assert all(np.isnan(v).all() for v in b.values())
    with pytest.raises(RRTMGError) as e:      # ... and through the joint call, before the shortwave is enqueued
        cj = dict(c, dyofyr=1, scon=1367.0, isolvar=0, adjes=1.0)
        as_ctx.sw_init(CPDAIR)
        as_ctx.radiation_fluxes(sw=dict(inp=cj, mcica=True), lw=dict(inp=cj, mcica=True, bands=band("upc"), band_levels=levels))
    assert e.value.code == RRTMG_ERR_ARG
    after = host_call(as_ctx, c, mcica)      # the context is the one that never saw the error
    assert_same_bits(after, before, "after the refusals")
    assert_same_bits(after, untouched, "a context that never saw the error")
    # up / dn only: served
    b = band("up", "dn")
    got = host_call(as_ctx, c, mcica, bands=b, band_levels=levels)
    assert_same_bits(got, before, "with bands")
    assert_clear_untouched(got, "with bands")
    wb = band("up", "dn", "upc", "dnc")
    want = host_call(gpu_ctx, c, mcica, bands=wb, band_levels=levels)
    for n in ("up", "dn"):
        assert np.isfinite(b[n]).all(), n
        d = maxdiff(b[n], wb[n])
        print("bands %s %s: max |d| vs the default call = %.3e" % (levels, n, d))
        assert np.array_equal(b[n], wb[n]), (n, d)      # cloud-free tile and tiles with cloud alike
    rows = (0, nlay) if levels == "boundaries" else range(nlay + 1)
    assert maxdiff(b["up"].sum(axis=0), got["uflx"][list(rows)]) <= 1.0e-9      # the bands add up to the broadband flux
    one = band("dn")      # a single member, device pointers
    from climt_amd import _hip
    dn_dev = _hip.DeviceArray.from_host(one["dn"])
    dev = {k: _hip.DeviceArray.from_host(v) for k, v in c.items() if isinstance(v, np.ndarray)}
    args = {k: v.ptr for k, v in dev.items()}
    args.update({k: v for k, v in c.items() if not isinstance(v, np.ndarray)}); args.update(ncol=ncol, nlay=nlay)
    dout = {k: _hip.DeviceArray.from_host(_nan(nlay, ncol, k)) for k in ALLSKY}
    as_ctx.lw_fluxes(args, mcica=mcica, out={k: v.ptr for k, v in dout.items()}, memspace=1, bands={"dn": dn_dev.ptr}, band_levels=levels)
    as_ctx.synchronize()
    assert np.array_equal(dn_dev.download().reshape(b["dn"].shape), b["dn"])


# ---- 8. switch back ---------------------------------------------------------------------------------------------------------------
def test_switch_back(gpu_ctx):
    c, mcica = _mixed("rtrnmr_idrv")
    never = host_call(gpu_ctx, c, mcica)
    ctx = _context()
    try:
        ctx.set_lw_clear_sky(False)
        host_call(ctx, c, mcica)
        ctx.set_lw_clear_sky(True)
        back = host_call(ctx, c, mcica)
        back_dev = device_call(ctx, c, mcica)
    finally:
        ctx.close()
    assert set(back) == set(ALLSKY + CLEAR + ("duflx_dt", "duflxc_dt"))
    for k in back:      # all six arrays (eight with idrv) written, with the bits of a context that never saw the switch
        assert np.isfinite(back[k]).all() and np.isfinite(back_dev[k]).all(), k
        assert np.array_equal(back[k], never[k]) and np.array_equal(back_dev[k], never[k]), k


# ---- 9. component -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mcica", [False, True])
def test_component_on_host_and_device_state(mcica):
    import climt_amd
    from climt_amd.rrtmg.longwave import CLEAR_SKY_DIAGNOSTICS, RRTMGLongwave
    from helpers import load_cache_case
    state, _, _ = load_cache_case("TestRRTMGLongwaveMCICA", "3d")
    kw = dict(mcica=mcica, cloud_overlap_method="maximum_random", random_number_generator="kissvec", calculate_change_up_flux=not mcica,
              allow_synthetic_tables=True)
    plain, allsky = RRTMGLongwave(**kw), RRTMGLongwave(clear_sky_diagnostics=False, **kw)
    np.random.seed(3)
    t0, d0 = plain(state)
    np.random.seed(3)
    t1, d1 = allsky(state)
    np.random.seed(3)
    t2, d2 = plain(state)      # the shared context is switched back by the default instance
    assert set(d0) - set(d1) == set(CLEAR_SKY_DIAGNOSTICS) and set(d1) <= set(d0) and set(t1) == set(t0)
    assert float(np.abs(d0["downwelling_longwave_flux_in_air"].values).max()) > 1.0
    for k in d1:
        assert d1[k].dims == d0[k].dims and d1[k].attrs == d0[k].attrs
        assert np.array_equal(d1[k].values, d0[k].values), (k, maxdiff(d1[k].values, d0[k].values))
    assert np.array_equal(t1["air_temperature"].values, t0["air_temperature"].values)
    assert all(np.array_equal(d2[k].values, d0[k].values) for k in d0)
    assert allsky.change_in_clear_sky_upward_flux_with_surface_temperature is None
    if not mcica:
        assert plain.change_in_clear_sky_upward_flux_with_surface_temperature is not None
        assert np.array_equal(allsky.change_in_upward_flux_with_surface_temperature, plain.change_in_upward_flux_with_surface_temperature)
    ds = climt_amd.DeviceState.from_host(state, [allsky])
    try:
        np.random.seed(3)
        tdev, ddev = allsky(ds)
        ds.ctx.synchronize()
        assert set(ddev) == set(d1)
        assert allsky.change_in_clear_sky_upward_flux_with_surface_temperature is None
        for k in d1:
            got = ddev[k].buf.download().reshape(ddev[k].shape)
            assert np.array_equal(got, np.asarray(d0[k].values).reshape(got.shape)), k
            assert np.array_equal(got, np.asarray(d1[k].values).reshape(got.shape)), k
    finally:
        ds.close()


@pytest.mark.parametrize("sw_clear,lw_clear", [(True, False), (False, True), (False, False)])
def test_component_through_radiation_step(sw_clear, lw_clear):
    import climt_amd
    sw = climt_amd.RRTMGShortwave(clear_sky_diagnostics=sw_clear)
    lw = climt_amd.RRTMGLongwave(allow_synthetic_tables=True, clear_sky_diagnostics=lw_clear)
    state = climt_amd.get_default_state([sw, lw], grid_state=climt_amd.get_grid(nx=16, ny=5, nz=28))
    (t_sw, d_sw), (t_lw, d_lw) = climt_amd.radiation_step(sw, lw, state)
    t1, d1 = sw(state)
    t2, d2 = lw(state)
    assert set(d_sw) == set(d1) == set(sw.diagnostic_properties) and set(d_lw) == set(d2) == set(lw.diagnostic_properties)
    assert len(d_lw) == (6 if lw_clear else 3) and len(d_sw) == (6 if sw_clear else 3)
    assert all(np.array_equal(d_sw[k].values, d1[k].values) for k in d1) and all(np.array_equal(d_lw[k].values, d2[k].values) for k in d2)
    assert np.array_equal(t_sw["air_temperature"].values, t1["air_temperature"].values)
    assert np.array_equal(t_lw["air_temperature"].values, t2["air_temperature"].values)
    plain = climt_amd.RRTMGLongwave(allow_synthetic_tables=True)
    t3, d3 = plain(state)
    for k in d_lw:
        assert np.array_equal(d_lw[k].values, d3[k].values), (k, maxdiff(d_lw[k].values, d3[k].values))
    assert np.array_equal(t_lw["air_temperature"].values, t3["air_temperature"].values)
