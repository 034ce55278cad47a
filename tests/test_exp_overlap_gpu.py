"""GPU tests of exponential and exponential-random McICA overlap (icld 4, 5 with rrtmg_hip_set_mcica_overlap_alpha; run with -m gpu
on an MI355X).  The mask call against the numpy statement of the definition from raw draws (tests/exp_overlap_cases.py), both
generators, bit for bit; the in-call generation against mask call + cldfmcl; the live reference fed with the restated mask;
shards; the column sort and the day pack; the error paths; rrtmg_hip_overlap_alpha against numpy; the components on a DeviceState.

Bounds.  Masks are integer work: equality.  Two calls of the same library on the same mask bits: equality.  Against the reference
Fortran: the bounds of tests/test_gpu_parity.py (0.01 W m^-2, 0.001 K day^-1, and the 5e-9 the device path is held to there).
rrtmg_hip_overlap_alpha: 1e-13 absolute -- two transcendental functions of a few ulp each feed an exponent of magnitude <~ 10."""
import os

import numpy as np
import pytest

from helpers import CONSTANTS, CPDAIR, ROOT, maxdiff

import exp_overlap_cases as X

pytestmark = pytest.mark.gpu

FLUX_TOL, HR_TOL, TIGHT = 1.0e-2, 1.0e-3, 5.0e-9
RRTMG_ERR_ARG, RRTMG_ERR_ICLD = 4, 15
BASE = dict(iaer=0, adjes=1.0, dyofyr=1, scon=1367.0, isolvar=0, inflg=2, iceflg=1, liqflg=1)
OUT = {"sw": ("swuflx", "swdflx", "swhr", "swuflxc", "swdflxc", "swhrc"), "lw": ("uflx", "dflx", "hr", "uflxc", "dflxc", "hrc")}
RD_OVER_G = 287.0 / 9.80665


@pytest.fixture(scope="module")
def module_ctx():
    """A context of its own: the rank correlations belong to a context, and gpu_ctx is shared by the whole session."""
    from climt_amd._lib import Context
    ctx = Context(0)
    ctx.set_constants(**CONSTANTS)
    ctx.sw_init(CPDAIR)
    ctx.lw_init(CPDAIR)
    yield ctx
    ctx.close()


@pytest.fixture
def ctx(module_ctx):
    yield module_ctx
    module_ctx.set_mcica_overlap_alpha("both", None)
    module_ctx.set_column_sort(False); module_ctx.set_sw_night_skip(False); module_ctx.set_sw_night_pack(False)


def _columns(ncol, nlay, seed=41):
    from climt_amd.synthetic import make_columns
    c = make_columns(ncol, nlay, cloudy=True, seed=seed)
    c.pop("lat")
    c.update(BASE)
    return c


def _call(ctx, which, c, device=False):
    """One flux call into NaN-filled outputs, host or device pointers -> {name: array}."""
    nlay, ncol = c["play"].shape
    shape = lambda k: (nlay + (0 if k.endswith(("hr", "hrc")) else 1), ncol)
    fn = ctx.sw_fluxes if which == "sw" else ctx.lw_fluxes
    if not device:
        out = {k: np.full(shape(k), np.nan) for k in OUT[which]}
        fn(c, mcica=True, out=out)
        return out
    from climt_amd import _hip
    dev = {k: _hip.DeviceArray.from_host(v) for k, v in c.items() if isinstance(v, np.ndarray) and k not in ("bndsolvar", "indsolvar")}
    args = {k: v for k, v in c.items() if k not in dev}
    args.update({k: v.ptr for k, v in dev.items()}); args.update(ncol=ncol, nlay=nlay)
    dout = {k: _hip.DeviceArray.from_host(np.full(shape(k), np.nan)) for k in OUT[which]}
    fn(args, mcica=True, out={k: v.ptr for k, v in dout.items()}, memspace=1)
    ctx.synchronize()
    return {k: v.download() for k, v in dout.items()}


def _same(a, b, what):
    for k in a:
        assert np.isfinite(a[k]).all(), (what, k)
        assert np.array_equal(a[k], b[k]), (what, k, maxdiff(a[k], b[k]))


def _bits(cldfmcl):
    """the library's [nlay][ncol][nsub] of 0 / 1 -> bool [nsub][nlay][ncol]"""
    assert np.isin(cldfmcl, (0.0, 1.0)).all()
    return cldfmcl.transpose(2, 0, 1) > 0.5


# ---- 5. the mask call against the numpy statement --------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", X.SHAPES, ids=lambda s: "%dx%d" % s)
def test_kissvec_mask_call_equals_the_numpy_statement(ctx, shape):
    ncol, nlay = shape
    play, _ = X.pressures(ncol, nlay)
    draws = X.kiss_draws(play, 684 + 140 * 2 * nlay)
    cldfr = X.cloud_field(ncol, nlay)
    for kind in X.ALPHA_KINDS:
        alpha = X.alpha_field(kind, ncol, nlay)
        ctx.set_mcica_overlap_alpha("both", alpha)
        for which in ("sw", "lw"):
            for seed in (0, 684):
                got = {icld: _bits(ctx.mcica_mask(which, play, cldfr, icld, seed, 0)) for icld in (4, 5)}
                for icld in (4, 5):
                    want = X.kiss_exp_mask(draws, cldfr, alpha, icld, X.NSUB[which], seed)
                    assert np.array_equal(got[icld], want), (kind, which, seed, icld, int((got[icld] != want).sum()))
                assert (kind == "zero") == np.array_equal(got[4], got[5]), (kind, which, seed)


@pytest.mark.parametrize("ncol,nlay,draws_mb", [(70, 33, None), (70, 130, None), (70, 33, 1)], ids=["70x33", "70x130-lds-over-64KB", "70x33-sub-column-groups"])
def test_mersenne_twister_mask_call_equals_the_numpy_statement(ctx, monkeypatch, ncol, nlay, draws_mb):
    """numpy's MT19937 with legacy integer seeding gives the raw words; the restatement of the conversion is first pinned against
    the existing icld = 1 mask.  70 x 130 stages 64 x 261 words = 66 816 bytes of LDS (over the 64 KB a kernel has unasked); with
    RRTMG_HIP_MT_DRAWS_MB = 1 the sub-columns of 70 x 33 are worked off in groups of 56."""
    if draws_mb:
        monkeypatch.setenv("RRTMG_HIP_MT_DRAWS_MB", str(draws_mb))
    play, _ = X.pressures(ncol, nlay)
    cldfr = X.cloud_field(ncol, nlay)
    seed = 209652396
    for which in ("sw", "lw"):
        assert np.array_equal(_bits(ctx.mcica_mask(which, play, cldfr, 1, seed, 1)), X.mt_random_mask(seed, cldfr, X.NSUB[which])), which
    for kind in (X.ALPHA_KINDS if nlay == 33 else ("random",)):
        alpha = X.alpha_field(kind, ncol, nlay)
        ctx.set_mcica_overlap_alpha("both", alpha)
        for which in ("sw", "lw"):
            got = {icld: _bits(ctx.mcica_mask(which, play, cldfr, icld, seed, 1)) for icld in (4, 5)}
            for icld in (4, 5):
                want = X.mt_exp_mask(seed, cldfr, alpha, icld, X.NSUB[which])
                assert np.array_equal(got[icld], want), (kind, which, icld, int((got[icld] != want).sum()))
            assert (kind == "zero") == np.array_equal(got[4], got[5]), (kind, which)


# ---- 6. in-call generation = mask call + cldfmcl ---------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def case136():
    c = _columns(136, 33)
    alpha = X.overlap_alpha_numpy(c["play"], c["tlay"], 2000.0, RD_OVER_G)
    return c, alpha


@pytest.mark.parametrize("irng", [0, 1], ids=["kissvec", "mersenne_twister"])
@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
def test_in_call_generation_equals_mask_call_plus_cldfmcl(ctx, case136, irng, device):
    c, alpha = case136
    c = dict(c, icld=5, irng=irng, permuteseed=684 if irng == 0 else 4711)
    ctx.set_mcica_overlap_alpha("both", alpha)
    for which in ("sw", "lw"):
        mask = ctx.mcica_mask(which, c["play"], c["cldfr"], 5, c["permuteseed"], irng)
        assert 0.02 < mask.mean() < 0.5
        inside = _call(ctx, which, c, device)
        given = _call(ctx, which, dict(c, cldfmcl=mask), device)
        _same(inside, given, (which, irng, device))
        # ... and the mode matters: maximum-random overlap on the same call gives other fluxes
        other = _call(ctx, which, dict(c, icld=2), device)
        assert maxdiff(inside[OUT[which][0]], other[OUT[which][0]]) > 1.0e-3, which


# ---- 7. the live reference fed with the restated mask ------------------------------------------------------------------------------
def _check(out, exp, tight=TIGHT):
    for k in exp:
        d = maxdiff(out[k], exp[k])
        print("%s: max |d| = %.3e" % (k, d))
        assert d <= (HR_TOL if k.endswith(("hr", "hrc")) else FLUX_TOL), (k, d)
        assert d <= tight, (k, d)


def test_in_call_fluxes_against_the_reference_fed_with_the_restated_mask(ctx, case136):
    """The reference's McICA entry takes its sub-columns as arguments: cldfmcl is the numpy statement of the definition, the
    sub-column water paths are the layer's where the bit is set (what its generator leaves there).  Against the in-call
    icld = 5 fluxes and heating rates of the library, at the bounds of the McICA live-oracle tests of tests/test_gpu_parity.py."""
    from oracle import ref_driver
    c, alpha = case136
    c = dict(c, icld=5, irng=0, permuteseed=684)
    nlay, ncol = c["play"].shape
    ctx.set_mcica_overlap_alpha("both", alpha)
    got = {w: _call(ctx, w, c) for w in ("sw", "lw")}
    draws = X.kiss_draws(c["play"], 684 + 140 * 2 * nlay)
    masks = {w: X.as_cldfmcl(X.kiss_exp_mask(draws, c["cldfr"], alpha, 5, X.NSUB[w], 684)) for w in ("sw", "lw")}
    if ref_driver.available("sw") and ref_driver.available("lw"):
        from tools.pack_tables import read_blob
        from tools.synth_lw_tables import fill_reference_from_blob
        rsw = ref_driver.RefSW()
        blob = read_blob(os.path.join(ROOT, "climt_amd", "data", "rrtmg_lw_data.bin"))
        rlw = ref_driver.RefLW(); rlw.init(fill_tables=lambda r: fill_reference_from_blob(r, blob))
        cr = dict(c, icld=2)      # (the reference knows 1..3; under McICA the flux call asks only whether there are clouds)
        exp = {}
        for w, ref in (("sw", rsw), ("lw", rlw)):
            s = ref.subcol(dict(cr, icld=1))      # the arrays in the reference's layout; the cloud fields are replaced below
            m = masks[w]
            s["cldfmcl"] = m
            s["ciwpmcl"] = np.ascontiguousarray(m * c["cicewp"][:, :, None]); s["clwpmcl"] = np.ascontiguousarray(m * c["cliqwp"][:, :, None])
            s["taucmcl"] = np.zeros_like(m)
            s["reicmcl"] = np.ascontiguousarray(c["reice"]); s["relqmcl"] = np.ascontiguousarray(c["reliq"])
            exp[w] = ref.fluxes(cr, mcica=True, subcol=s)
    else:
        from helpers import EmuContext, require_reference_oracle
        require_reference_oracle("port")
        emu = EmuContext()
        exp = {"sw": emu.sw_fluxes(dict(c, icld=2, cldfmcl=masks["sw"]), mcica=True), "lw": emu.lw_fluxes(dict(c, icld=2, cldfmcl=masks["lw"]), mcica=True)}
    for w in ("sw", "lw"):
        _check(got[w], {k: exp[w][k] for k in OUT[w]})


# ---- 8. shards ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("irng", [0, 1], ids=["kissvec", "mersenne_twister"])
def test_blocks_of_a_sharded_grid_equal_the_whole_grid(ctx, irng):
    """200 columns as blocks of 128 + 72 (shard_col0 / shard_ncol), each block with its own columns of alpha set on the context
    before its call -- what the owner of a block does."""
    from climt_amd.distributed import slice_columns
    c = dict(_columns(200, 33, seed=43), icld=5, irng=irng, permuteseed=99)
    alpha = X.overlap_alpha_numpy(c["play"], c["tlay"], 1500.0, RD_OVER_G)
    ctx.set_mcica_overlap_alpha("both", alpha)
    whole = {w: _call(ctx, w, c) for w in ("sw", "lw")}
    for lo, hi in ((0, 128), (128, 200)):
        sub = slice_columns(c, lo, hi); sub.update(shard_col0=lo, shard_ncol=200)
        ctx.set_mcica_overlap_alpha("both", np.ascontiguousarray(alpha[:, lo:hi]))
        for w in ("sw", "lw"):
            _same(_call(ctx, w, sub), {k: v[:, lo:hi] for k, v in whole[w].items()}, (w, irng, lo))


# ---- 9. the column sort, the night skip and the day pack -----------------------------------------------------------------------------
def test_column_sort_and_day_pack_keep_the_bits(ctx):
    """200 x 33, kissvec, device pointers; a third of the columns is night.  Both modes choose a solve variant per 64-column tile
    of their internal copy, and the two variants differ in the last place, so each is compared on a grid where it leaves every
    column its variant.  The sort: tile 1 (columns 64..127) is cloud-free and runs the clear-sky variant in the plain call
    already, every other column has a cloud; the sort moves tile 1 to the front.  The skip and the pack: a cloud in every column;
    day columns keep the plain call's bits, night columns are zero."""
    full = dict(_columns(200, 33, seed=47), icld=5, irng=0, permuteseed=7)
    bare = ~(full["cldfr"] > 0).any(axis=0)
    full["cldfr"][5:8, bare] = 0.5; full["cliqwp"][5:8, bare] = 40.0; full["cicewp"][5:8, bare] = 0.0
    assert (full["cldfr"] > 0).any(axis=0).all()
    night = (np.arange(200) % 3) == 1
    night[128:192] = True      # tile 2 is night altogether
    full["coszen"] = np.where(night, -0.2, np.maximum(full["coszen"], 0.1))
    alpha = X.overlap_alpha_numpy(full["play"], full["tlay"], 2000.0, RD_OVER_G)
    ctx.set_mcica_overlap_alpha("both", alpha)
    c = dict(full, **{k: full[k].copy() for k in ("cldfr", "cliqwp", "cicewp")})
    for k in ("cldfr", "cliqwp", "cicewp"):
        c[k][:, 64:128] = 0.0
    plain = {w: _call(ctx, w, c, device=True) for w in ("sw", "lw")}
    ctx.set_column_sort(True)
    for w in ("sw", "lw"):
        _same(_call(ctx, w, c, device=True), plain[w], ("sorted", w))
    # That the sorted path is the one taken: on the grid as make_columns leaves it, cloud-free columns sit inside cloudy tiles.
    # The sort moves them into tiles of their own, where they run the clear-sky variant -- the bits of a call that holds those
    # columns only, which in the shortwave are not the bits of the plain call (the variants differ in the last place) -- while
    # the cloudy columns keep theirs.
    mixed = dict(_columns(200, 33, seed=47), icld=5, irng=0, permuteseed=7, coszen=full["coszen"])
    cloudy = (mixed["cldfr"] > 0).any(axis=0)
    assert 20 < (~cloudy).sum() < 120 and all((~cloudy[t:t + 64]).any() and cloudy[t:t + 64].any() for t in (0, 64, 128))
    srt = _call(ctx, "sw", mixed, device=True)
    ctx.set_column_sort(False)
    unsorted = _call(ctx, "sw", mixed, device=True)
    only_clear = {k: (np.ascontiguousarray(v[..., ~cloudy]) if isinstance(v, np.ndarray) and v.shape[-1] == 200 else v) for k, v in mixed.items()}
    ctx.set_mcica_overlap_alpha("sw", np.ascontiguousarray(alpha[:, ~cloudy]))
    clr = _call(ctx, "sw", only_clear, device=True)
    ctx.set_mcica_overlap_alpha("sw", alpha)
    for k in srt:
        assert np.array_equal(srt[k][:, cloudy], unsorted[k][:, cloudy]), k
        assert np.array_equal(srt[k][:, ~cloudy], clr[k]), k
        assert maxdiff(srt[k], unsorted[k]) <= 1.0e-10, k
    assert not np.array_equal(srt["swuflx"][:, ~cloudy], unsorted["swuflx"][:, ~cloudy])      # (measured: 5.7e-14 W m^-2)
    # the night-column skip and the day pack, with the counts that say they ran
    plain_sw = _call(ctx, "sw", full, device=True)
    assert ctx.sw_night_last() == (0, 0)
    ctx.set_sw_night_skip(True)
    skip = _call(ctx, "sw", full, device=True)
    assert ctx.sw_night_last() == (1, int(night.sum()))      # tile 2, and every night column
    ctx.set_sw_night_skip(False)
    ctx.set_sw_night_pack(True)
    pack = _call(ctx, "sw", full, device=True)
    nday = int((~night).sum())
    assert ctx.sw_night_last() == (4 - (nday + 63) // 64, int(night.sum())) and 4 - (nday + 63) // 64 == 2      # the day columns fill two tiles
    for name, got in (("skip", skip), ("pack", pack)):
        for k in got:
            d = maxdiff(got[k][:, ~night], plain_sw[k][:, ~night])
            assert np.array_equal(got[k][:, ~night], plain_sw[k][:, ~night]), (name, k, d)
            # (a night column is exact zeros under either option; the plain call clamps coszen and leaves ~1e-8 W m^-2 there)
            assert not got[k][:, night].any(), (name, k)
    assert float(np.abs(plain_sw["swdflx"][:, ~night]).max()) > 100.0


# ---- 10. errors ------------------------------------------------------------------------------------------------------------------------
def test_errors_and_the_cleared_setting(ctx, case136):
    from climt_amd._lib import RRTMGError
    c, alpha = case136
    c = dict(c, icld=5, irng=0, permuteseed=3)
    small = dict(_columns(70, 33), icld=5, irng=0, permuteseed=3)
    ctx.set_mcica_overlap_alpha("both", alpha)
    for w in ("sw", "lw"):
        fn = ctx.sw_fluxes if w == "sw" else ctx.lw_fluxes
        with pytest.raises(RRTMGError) as e:      # another shape than the stored one
            fn(small, mcica=True)
        assert e.value.code == RRTMG_ERR_ARG
        with pytest.raises(RRTMGError) as e:      # there is no non-McICA exponential overlap
            fn(dict(c, cldfr=(c["cldfr"] > 0.5).astype(float)), mcica=False)
        assert e.value.code == RRTMG_ERR_ARG
        with pytest.raises(RRTMGError) as e:
            ctx.mcica_mask(w, small["play"], small["cldfr"], 5, 3, 0)
        assert e.value.code == RRTMG_ERR_ARG
    # set for one spectrum only: the other runs as on the parent
    as2 = {w: _call(ctx, w, dict(c, icld=2)) for w in ("sw", "lw")}
    ctx.set_mcica_overlap_alpha("lw", None)
    _same(_call(ctx, "lw", c), as2["lw"], "lw cleared")
    assert maxdiff(_call(ctx, "sw", c)["swuflx"], as2["sw"]["swuflx"]) > 1.0e-3
    # cleared: icld = 5 is reset to 2 in a flux call, and the mask call answers the reference's error
    ctx.set_mcica_overlap_alpha("both", None)
    for w in ("sw", "lw"):
        _same(_call(ctx, w, c), as2[w], (w, "cleared"))
        with pytest.raises(RRTMGError) as e:
            ctx.mcica_mask(w, c["play"], c["cldfr"], 5, 3, 0)
        assert e.value.code == RRTMG_ERR_ICLD
    # the context is usable afterwards, with and without the setting
    ctx.set_mcica_overlap_alpha("sw", alpha)
    assert np.isfinite(_call(ctx, "sw", c)["swhr"]).all()


# ---- 11. rrtmg_hip_overlap_alpha; the components on a DeviceState ------------------------------------------------------------------------
def test_overlap_alpha_against_numpy(ctx):
    from climt_amd import _hip
    ncol, nlay = 70, 33
    play, tlay = X.pressures(ncol, nlay)
    want = X.overlap_alpha_numpy(play, tlay, 2000.0, RD_OVER_G)
    host = ctx.overlap_alpha(play, tlay, 2000.0, RD_OVER_G)
    dp, dt, da = _hip.DeviceArray.from_host(play), _hip.DeviceArray.from_host(tlay), _hip.DeviceArray.from_host(np.full((nlay, ncol), np.nan))
    ctx.overlap_alpha(dp.ptr, dt.ptr, 2000.0, RD_OVER_G, out=da.ptr, memspace=1, ncol=ncol, nlay=nlay)
    ctx.synchronize()
    dev = da.download()
    for name, got in (("host", host), ("device", dev)):
        d = float(np.abs(got - want).max())
        print("overlap_alpha %s pointers: max |d| = %.3e" % (name, d))
        assert d <= 1.0e-13, (name, d)
        assert np.all(got[0] == 1.0)
        assert np.all((got[1:] > 0.0) & (got[1:] < 1.0))
    assert np.array_equal(host, dev)
    # a device array is copied in stream order: the caller may overwrite it at once
    c = dict(_columns(ncol, nlay), icld=4, irng=0, permuteseed=5)
    ctx.set_mcica_overlap_alpha("sw", want)
    by_host = ctx.mcica_mask("sw", c["play"], c["cldfr"], 4, 5, 0)
    da2 = _hip.DeviceArray.from_host(want)
    ctx.set_mcica_overlap_alpha("sw", da2.ptr, memspace=1, ncol=ncol, nlay=nlay)
    da2.upload(np.zeros((nlay, ncol)))
    assert np.array_equal(ctx.mcica_mask("sw", c["play"], c["cldfr"], 4, 5, 0), by_host)


def test_components_on_a_device_state_equal_the_host_state():
    """RRTMGShortwave / RRTMGLongwave with cloud_overlap_method="exponential_random" on a DeviceState -- alpha from
    rrtmg_hip_overlap_alpha with device pointers, set in stream order -- against the same components on the host state (alpha
    through the host-pointer calls).  The alpha arrays are equal bit for bit, and the fluxes agree to the round-off of the
    derived inputs (the bound of test_device_resident_radiation_step_equals_the_host_path).  Then the masks' consequence bit
    for bit: the device-pointer calls repeated with alpha downloaded from the device and set by hand equal the first ones in
    every output."""
    import climt_amd
    from climt_amd.rrtmg.common import make_context
    kw = dict(mcica=True, random_number_generator="kissvec", cloud_overlap_method="exponential_random", cloud_overlap_decorrelation_length=1800.0)
    sw, lw = climt_amd.RRTMGShortwave(**kw), climt_amd.RRTMGLongwave(allow_synthetic_tables=True, **kw)
    state = climt_amd.get_default_state([sw, lw], grid_state=climt_amd.get_grid(nx=17, ny=8, nz=33))
    p = state["air_pressure"].values
    state["air_temperature"].values[:] = np.maximum(200.0, 290.0 * (p / 1.0e5) ** 0.19)
    state["specific_humidity"].values[:] = 0.012 * (p / 1.0e5) ** 3
    cld = ((p > 4.0e4) & (p < 6.0e4)) | ((p > 7.0e4) & (p < 8.5e4))
    state["cloud_area_fraction_in_atmosphere_layer"].values[:] = np.where(cld, 0.4, 0.0)
    state["mass_content_of_cloud_liquid_water_in_atmosphere_layer"].values[:] = np.where(cld, 0.03, 0.0)
    state["zenith_angle"].values[:] = 0.6
    names = {"sw": ("upwelling_shortwave_flux_in_air", "downwelling_shortwave_flux_in_air", "air_temperature_tendency_from_shortwave"),
             "lw": ("upwelling_longwave_flux_in_air", "downwelling_longwave_flux_in_air", "air_temperature_tendency_from_longwave")}
    ctx = make_context(0)
    ds = None
    try:
        np.random.seed(5)
        host = {"sw": sw(state)[1], "lw": lw(state)[1]}
        nlay, ncol = 33, 17 * 8
        # (what the context holds beforehand is wrong for both spectra: a device path that set nothing, or the other spectrum's
        #  slot, would draw other masks)
        ctx.set_mcica_overlap_alpha("both", np.zeros((nlay, ncol)))
        np.random.seed(5)
        ds = climt_amd.DeviceState.from_host(state, [sw, lw])
        dsw = sw(ds)[1]; dlw = lw(ds)[1]
        ds.update(dsw); ds.update(dlw)
        ctx.synchronize()
        pl = ds.need("air_pressure", sw.input_properties["air_pressure"]).buf.download()
        tl = ds.need("air_temperature", sw.input_properties["air_temperature"]).buf.download()
        assert pl.shape == (nlay, ncol) and tl.shape == (nlay, ncol)
        want = ctx.overlap_alpha(pl, tl, 1800.0, RD_OVER_G)
        assert float(np.abs(want - X.overlap_alpha_numpy(pl, tl, 1800.0, RD_OVER_G)).max()) <= 1.0e-13
        ctx.synchronize()
        for w in ("sw", "lw"):
            got = ds.work(("d.overlap_alpha", w), (nlay, ncol), ("mid_levels", "*"), "dimensionless").buf.download()
            assert np.array_equal(got, want), w
            for n in names[w]:
                h, d = host[w][n], ds.download(n)
                g = np.transpose(d.values, [d.dims.index(x) for x in h.dims])
                scale = max(1.0, float(np.abs(h.values).max()))
                print("%s: max |d| = %.3e" % (n, maxdiff(g, h.values)))
                assert g.shape == h.values.shape and maxdiff(g, h.values) <= 1.0e-9 * scale, (n, maxdiff(g, h.values))
        assert float(np.abs(host["sw"]["downwelling_shortwave_flux_in_air"].values).max()) > 100.0
        # The same device-pointer calls again with alpha DOWNLOADED from the device and set by hand, the components' own alpha
        # step bypassed: every output keeps its bits.
        outputs = sorted(set(dsw) | set(dlw))
        assert len(outputs) >= 12
        first = {n: np.array(ds.download(n).values) for n in outputs}
        by_hand = {w: ds.work(("d.overlap_alpha", w), (nlay, ncol), ("mid_levels", "*"), "dimensionless").buf.download() for w in ("sw", "lw")}
        ctx.set_mcica_overlap_alpha("both", np.zeros((nlay, ncol)))
        for w in ("sw", "lw"):
            ctx.set_mcica_overlap_alpha(w, by_hand[w])
        from climt_amd import device_state
        own_step = device_state._device_overlap
        device_state._device_overlap = lambda *a, **k: None
        try:
            np.random.seed(5)
            dsw2 = sw(ds)[1]; dlw2 = lw(ds)[1]
            ds.update(dsw2); ds.update(dlw2)
        finally:
            device_state._device_overlap = own_step
        for n in outputs:
            again = np.array(ds.download(n).values)
            assert np.isfinite(again).all() and np.array_equal(again, first[n]), (n, maxdiff(again, first[n]))
        # ... and alpha matters: with the zeros left in place the same calls give other fluxes
        ctx.set_mcica_overlap_alpha("both", np.zeros((nlay, ncol)))
        device_state._device_overlap = lambda *a, **k: None
        try:
            np.random.seed(5)
            ds.update(sw(ds)[1])
        finally:
            device_state._device_overlap = own_step
        assert maxdiff(np.array(ds.download("upwelling_shortwave_flux_in_air").values), first["upwelling_shortwave_flux_in_air"]) > 1.0e-3
    finally:
        if ds is not None:
            ds.close()      # (hands the shared context back in the mode it was found in)
        ctx.set_mcica_overlap_alpha("both", None)
