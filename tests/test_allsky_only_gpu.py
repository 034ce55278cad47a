"""GPU tests of the shortwave call without the clear-sky outputs (rrtmg_hip_set_sw_clear_sky(ctx, 0); run with -m gpu on an
MI355X): the committed reference-Fortran fixtures, the default call of the same library on grids without a fixture, chunks,
shards, the night options, the column sort, the joint and the deferred call, the switch back, the refusals and the component.

Bounds: TIGHT against a fixture (tests/test_sw_components_gpu.py); 5e-8 against the default call, the bound
tests/test_gpu_parity.py uses for the shortwave on random grids (reftra near k mu0 = 1): the two solve instantiations may
contract differently, so bits are demanded only where both calls run the same kernel."""
import numpy as np
import pytest

from helpers import CONSTANTS, CPDAIR, OPT_CASES, REF_CASES, load_opt_case, load_ref_case, maxdiff
from test_sw_components_gpu import _grid

pytestmark = pytest.mark.gpu

TIGHT = 5.0e-9
VS_DEFAULT = 5.0e-8
ALLSKY = ("swuflx", "swdflx", "swhr")
CLEAR = ("swuflxc", "swdflxc", "swhrc")
RRTMG_ERR_ARG = 4


def _context():
    from climt_amd._lib import Context
    ctx = Context(0)
    ctx.set_constants(**CONSTANTS)
    ctx.sw_init(CPDAIR)
    try:
        ctx.lw_init(CPDAIR)
    except Exception:
        pass
    return ctx


@pytest.fixture(scope="module")
def as_ctx():
    """A context of its own with the clear-sky outputs off (gpu_ctx, which the whole session shares, keeps its default)."""
    ctx = _context()
    ctx.set_sw_clear_sky(False)
    yield ctx
    ctx.close()


def _shape(c):
    return (c["nlay"], c["ncol"]) if "ncol" in c else c["play"].shape


def host_call(ctx, c, mcica, keys=ALLSKY + CLEAR, **kw):
    """One host-pointer call into NaN-filled arrays for `keys` -> {name: array}."""
    nlay, ncol = _shape(c)
    out = {k: np.full((nlay + (not k.startswith("swhr")), ncol), np.nan) for k in keys}
    ctx.sw_fluxes(c, mcica=mcica, out=out, **kw)
    return out


def device_call(ctx, c, mcica, keys=ALLSKY + CLEAR, deferred=False):
    """One device-pointer call into NaN-filled device buffers for `keys` -> {name: downloaded array}."""
    from climt_amd import _hip
    nlay, ncol = _shape(c)
    dev = {k: _hip.DeviceArray.from_host(v) for k, v in c.items() if isinstance(v, np.ndarray)}
    args = {k: v.ptr for k, v in dev.items()}
    args.update({k: v for k, v in c.items() if not isinstance(v, np.ndarray)}); args.update(ncol=ncol, nlay=nlay)
    dout = {k: _hip.DeviceArray.from_host(np.full((nlay + (not k.startswith("swhr")), ncol), np.nan)) for k in keys}
    if deferred:
        ctx.set_deferred(True)
    try:
        ctx.sw_fluxes(args, mcica=mcica, out={k: v.ptr for k, v in dout.items()}, memspace=1)
        ctx.synchronize()
    finally:
        if deferred:
            ctx.set_deferred(False)
    return {k: v.download() for k, v in dout.items()}


def assert_clear_untouched(out, what=""):
    for k in CLEAR:
        assert np.isnan(out[k]).all(), (what, k, "a clear-sky output was written")


def assert_close(got, want, bound, what=""):
    for k in ALLSKY:
        assert np.isfinite(got[k]).all(), (what, k)
        d = maxdiff(got[k], want[k])
        print("%s %s: max |d| = %.3e (bound %.1e)" % (what, k, d, bound))
        assert d <= bound, (what, k, d)


def assert_same_bits(got, want, what=""):
    for k in ALLSKY:
        assert np.array_equal(got[k], want[k]), (what, k, maxdiff(got[k], want[k]))


def _cloudy_fixtures():
    cases = [("ref", n) for n in REF_CASES if not n.startswith("clear")]
    cases += [("opt", n) for n in OPT_CASES if n.startswith("sw_") and not n.endswith("_clear")]
    return cases


def test_the_fixture_list_holds_the_cloudy_shortwave_cases():
    names = [n for _, n in _cloudy_fixtures()]
    assert {"overcast_L60", "mcica_kiss_random", "mcica_kiss_maxrand", "mcica_mt_max"} <= set(names)
    assert sum(n.startswith("sw_") for n in names) >= 6
    for n in OPT_CASES:      # nothing cloudy was filtered out by its name
        if n.startswith("sw_") and n.endswith("_clear"):
            _, _, c, _ = load_opt_case(n)
            assert c.get("icld", 1) == 0 or not (np.asarray(c["cldfr"]) > 0).any(), n


# ---- 1. fixtures ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,case", _cloudy_fixtures())
def test_fixtures(as_ctx, kind, case):
    if kind == "ref":
        c, mcica, exp = load_ref_case(case)
        exp = exp["sw"]
    else:
        _, mcica, c, exp = load_opt_case(case)
    assert (np.asarray(c["cldfr"]) > 0).any()
    host = host_call(as_ctx, c, mcica)
    assert_close(host, exp, TIGHT, case + " host")
    assert_clear_untouched(host, case + " host")
    dev = device_call(as_ctx, c, mcica)
    assert_close(dev, exp, TIGHT, case + " device")
    assert_clear_untouched(dev, case + " device")
    assert_same_bits(dev, host, case)
    # the three pointers NULL: status 0 (an exception otherwise), the same bits
    assert_same_bits(host_call(as_ctx, c, mcica, keys=ALLSKY), host, case + " NULL host")
    assert_same_bits(device_call(as_ctx, c, mcica, keys=ALLSKY), host, case + " NULL device")


# ---- 2. mixed grid ---------------------------------------------------------------------------------------------------------------
def _fractional(c):
    """The non-McICA grid with cloud fractions other than 0 and 1 (icld 1): the zclear * clear + zc * cloudy branch.  The library
    refuses, as the reference does, a fraction inside (1e-6, 1 - 1e-6) (RRTMG_ERR_PARTIAL_CLOUD, test_drawn_fractions_are_refused
    below), so the fractions are the ones it serves: 1 - 5e-7 and 5e-7 by turns (both operators mixed), and 5e-13 in every
    seventh cloudy layer (at most 1e-12: no cloud operator, the (0, 0, 1, 1) mix)."""
    f = dict(c)
    lay = np.arange(c["cldfr"].shape[0])[:, None] + np.arange(c["cldfr"].shape[1])[None, :]
    frac = np.where(lay % 7 == 0, 5.0e-13, np.where(lay % 2 == 0, 1.0 - 5.0e-7, 5.0e-7))
    f["cldfr"] = np.where(c["cldfr"] > 0, frac, 0.0)
    return f


def test_drawn_fractions_are_refused(gpu_ctx, as_ctx):
    """Cloud fractions as climt_amd.synthetic draws them are partial cloud to the non-McICA shortwave, with either setting."""
    from climt_amd._lib import RRTMGError
    from climt_amd.synthetic import make_columns
    c = _grid(128, 20, 27, False)
    c["cldfr"] = np.where(c["cldfr"] > 0, np.clip(make_columns(128, 20, cloudy=True, seed=29)["cldfr"], 0.05, 0.95), 0.0)
    for ctx in (gpu_ctx, as_ctx):
        with pytest.raises(RRTMGError) as e:
            host_call(ctx, c, False)
        assert e.value.code == 10


@pytest.mark.parametrize("variant", ["mcica", "overcast", "fractional"])
def test_mixed_grid_against_the_default_call(gpu_ctx, as_ctx, variant):
    mcica = variant == "mcica"
    c = _grid(200, 20, 27, mcica)      # 4 tiles, tile 0 cloud-free, the last one ragged (8 columns)
    if variant == "fractional":
        c = _fractional(c)
        frac = c["cldfr"][c["cldfr"] > 0]
        assert frac.size and frac.min() > 0.0 and frac.max() < 1.0 and c["icld"] == 1
        assert (frac > 0.5).any() and ((frac > 1.0e-12) & (frac < 0.5)).any() and (frac <= 1.0e-12).any()
    want = host_call(gpu_ctx, c, mcica)
    got = host_call(as_ctx, c, mcica)
    assert_close(got, want, VS_DEFAULT, variant)
    assert_clear_untouched(got, variant)
    free = np.zeros(200, dtype=bool); free[:64] = True      # the cloud-free tile ran sw_solve_all_kernel<false> in both calls
    assert not (c["cldfr"][:, free] > 0).any() and (c["cldfr"][:, ~free] > 0).any()
    for k in ALLSKY:
        assert np.array_equal(got[k][:, free], want[k][:, free]), (variant, k)
    assert float(np.abs(want["swdflx"] - want["swdflxc"]).max()) > 1.0
    assert_same_bits(device_call(as_ctx, c, mcica), got, variant + " device")


# ---- 3. mask-word boundary ---------------------------------------------------------------------------------------------------------
def test_two_mask_words(gpu_ctx, as_ctx):
    c = _grid(130, 70, 31, True)
    # (the generator's clouds stay below layer 64 of 70: the cloud fields of layers 8-13 once more in layers 62-67, so that set
    #  mask bits sit on both sides of the word boundary)
    for k in ("cldfr", "cliqwp", "cicewp", "reliq", "reice"):
        c[k] = np.array(c[k]); c[k][62:68] = c[k][8:14]
    assert (c["cldfr"][64:] > 0).any() and (c["cldfr"][:64] > 0).any() and (c["cldfr"][62:64] > 0).any()
    want = host_call(gpu_ctx, c, True)
    got = host_call(as_ctx, c, True)
    assert_close(got, want, VS_DEFAULT, "130x70")
    assert_clear_untouched(got)


# ---- 4. chunks and shards ---------------------------------------------------------------------------------------------------------
def test_chunks_and_shards(as_ctx, monkeypatch):
    from climt_amd.distributed import slice_columns
    c = _grid(320, 20, 33, True)
    whole = host_call(as_ctx, c, True)
    parts = []
    for lo, hi in ((0, 128), (128, 320)):
        sub = slice_columns(c, lo, hi); sub.update(shard_col0=lo, shard_ncol=320)
        parts.append(host_call(as_ctx, sub, True))
        assert_clear_untouched(parts[-1], (lo, hi))
    for k in ALLSKY:
        assert np.array_equal(np.concatenate([p[k] for p in parts], axis=1), whole[k]), k
    monkeypatch.setenv("RRTMG_HIP_CHUNK_TILES", "2")
    small = _context()
    try:
        small.set_sw_clear_sky(False)
        ch = host_call(small, c, True)
        assert small.kernel_launches("sw") >= 2      # 5 tiles in chunks of 2
    finally:
        small.close()
    assert_same_bits(ch, whole, "chunks")
    assert_clear_untouched(ch, "chunks")


# ---- 5. night ---------------------------------------------------------------------------------------------------------------------
def _night_grid():
    c = _grid(320, 20, 35, True)
    cz = np.full(320, 0.55)
    cz[64:128] = -0.3            # a night tile
    cz[150:200] = -0.1           # night columns in two mixed tiles
    cz[300:] = 0.0               # the ragged end of the last tile
    c["coszen"] = cz
    return c, cz <= 0.0


def test_night_skip(as_ctx):
    c, dark = _night_grid()
    off = host_call(as_ctx, c, True)
    as_ctx.set_sw_night_skip(True)
    try:
        on = host_call(as_ctx, c, True)
        tiles, cols = as_ctx.sw_night_last()
        dev = device_call(as_ctx, c, True)
    finally:
        as_ctx.set_sw_night_skip(False)
    assert (tiles, cols) == (1, int(dark.sum()))
    for got in (on, dev):
        assert_clear_untouched(got, "night skip")
        for k in ALLSKY:
            assert np.array_equal(got[k][:, ~dark], off[k][:, ~dark]), k
            z = got[k][:, dark]
            assert np.all(z == 0.0) and not np.signbit(z).any(), k
    assert np.all(off["swdflx"][-1, dark] > 0.0)      # (without the skip the night columns receive the clamped sun)


@pytest.mark.parametrize("option", ["night_pack", "column_sort"])
def test_permuted_calls(as_ctx, option):
    """The day-column pack and the column sort run the call on a permuted copy: no gather or scatter entry for the three absent
    outputs (the sentinels stay), results those of the unpermuted call to the bound (a column may change tile, and with it solve kernel)."""
    c, dark = _night_grid()
    if option == "column_sort":
        c["coszen"] = np.full(320, 0.55)
        dark = np.zeros(320, dtype=bool)
    want = device_call(as_ctx, c, True)
    setter = as_ctx.set_sw_night_pack if option == "night_pack" else as_ctx.set_column_sort
    setter(True)
    try:
        got = device_call(as_ctx, c, True)
        null = device_call(as_ctx, c, True, keys=ALLSKY)
    finally:
        setter(False)
    assert_clear_untouched(got, option)
    for k in ALLSKY:
        assert np.isfinite(got[k]).all(), k
        d = maxdiff(got[k][:, ~dark], want[k][:, ~dark])
        print("%s %s: max |d| = %.3e" % (option, k, d))
        assert d <= VS_DEFAULT, (option, k, d)
        assert np.all(got[k][:, dark] == 0.0), k
    assert_same_bits(null, got, option + " NULL")


# ---- 6. joint and deferred ---------------------------------------------------------------------------------------------------------
def test_joint_and_deferred(gpu_ctx, as_ctx):
    from climt_amd._lib import LW_OUT
    c = _grid(200, 20, 37, True)
    nlay, ncol = c["play"].shape
    plain = host_call(as_ctx, c, True)
    nan = lambda lev: np.full((nlay + lev, ncol), np.nan)
    lw_want = gpu_ctx.lw_fluxes(c, mcica=True, out={k: nan(lev) for k, lev in LW_OUT})
    sw_out = {k: nan(not k.startswith("swhr")) for k in ALLSKY + CLEAR}
    lw_out = {k: nan(lev) for k, lev in LW_OUT}
    as_ctx.radiation_fluxes(sw=dict(inp=c, mcica=True, out=sw_out), lw=dict(inp=c, mcica=True, out=lw_out))
    assert_same_bits(sw_out, plain, "joint")
    assert_clear_untouched(sw_out, "joint")
    for k, _ in LW_OUT:
        assert np.array_equal(lw_out[k], lw_want[k]), k
    dev = device_call(as_ctx, c, True, deferred=True)
    assert_same_bits(dev, plain, "deferred")
    assert_clear_untouched(dev, "deferred")


# ---- 7. switch back ---------------------------------------------------------------------------------------------------------------
def test_switch_back(gpu_ctx):
    c = _grid(200, 20, 39, True)
    never = host_call(gpu_ctx, c, True)
    ctx = _context()
    try:
        ctx.set_sw_clear_sky(False)
        host_call(ctx, c, True)
        ctx.set_sw_clear_sky(True)
        back = host_call(ctx, c, True)
        back_dev = device_call(ctx, c, True)
    finally:
        ctx.close()
    for k in ALLSKY + CLEAR:
        assert np.array_equal(back[k], never[k]) and np.array_equal(back_dev[k], never[k]), k


# ---- 8. refusals ---------------------------------------------------------------------------------------------------------------------
def test_refusals(as_ctx):
    from climt_amd._lib import RRTMGError
    c = _grid(128, 20, 41, True)
    want = host_call(as_ctx, c, True)
    comp = {"dirdflx": np.full((21, 128), np.nan)}
    band = {"dn": np.full((14, 21, 128), np.nan)}
    for kw in (dict(components=comp), dict(bands=band), dict(components=comp, bands=band),
               dict(components=comp, surface={"albdir": np.full((14, 128), 0.2)})):
        with pytest.raises(RRTMGError) as e:
            host_call(as_ctx, c, True, **kw)
        assert e.value.code == RRTMG_ERR_ARG and "rrtmg_hip_set_sw_clear_sky" in str(e.value), str(e.value)
    assert np.isnan(comp["dirdflx"]).all() and np.isnan(band["dn"]).all()
    nlay, ncol = c["play"].shape
    with pytest.raises(RRTMGError) as e:      # ... and through the joint call
        as_ctx.radiation_fluxes(sw=dict(inp=c, mcica=True, components=comp), lw=dict(inp=c, mcica=True))
    assert e.value.code == RRTMG_ERR_ARG
    assert_same_bits(host_call(as_ctx, c, True), want, "after the refusals")
    # the surface struct alone is served
    albdir = np.full((14, 128), 0.2)
    got = host_call(as_ctx, c, True, surface={"albdir": albdir})
    assert_clear_untouched(got)
    assert np.isfinite(got["swuflx"]).all()
    assert maxdiff(got["swuflx"], want["swuflx"]) > 1.0e-3


# ---- 9. component -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mcica", [False, True])
def test_component_on_host_and_device_state(mcica):
    import climt_amd
    from climt_amd.rrtmg.shortwave import CLEAR_SKY_DIAGNOSTICS, RRTMGShortwave
    from helpers import load_cache_case
    state, _, _ = load_cache_case("TestRRTMGShortwaveMCICA", "3d")
    kw = dict(mcica=mcica, cloud_overlap_method="maximum_random" if mcica else "clear_only", random_number_generator="kissvec")
    plain, allsky = RRTMGShortwave(**kw), RRTMGShortwave(clear_sky_diagnostics=False, **kw)
    np.random.seed(3)
    t0, d0 = plain(state)
    np.random.seed(3)
    t1, d1 = allsky(state)
    np.random.seed(3)
    t2, d2 = plain(state)      # the shared context is switched back by the default instance
    assert set(d0) - set(d1) == set(CLEAR_SKY_DIAGNOSTICS) and set(d1) <= set(d0) and set(t1) == set(t0)
    assert float(np.abs(d0["downwelling_shortwave_flux_in_air"].values).max()) > 1.0
    for k in d1:
        assert d1[k].dims == d0[k].dims and d1[k].attrs == d0[k].attrs
        assert maxdiff(d1[k].values, d0[k].values) <= VS_DEFAULT, k
    assert maxdiff(t1["air_temperature"].values, t0["air_temperature"].values) <= VS_DEFAULT
    assert all(np.array_equal(d2[k].values, d0[k].values) for k in d0)
    ds = climt_amd.DeviceState.from_host(state, [allsky])
    try:
        np.random.seed(3)
        tdev, ddev = allsky(ds)
        ds.ctx.synchronize()
        assert set(ddev) == set(d1)
        for k in d1:
            got = ddev[k].buf.download().reshape(ddev[k].shape)
            assert maxdiff(got, np.asarray(d0[k].values).reshape(got.shape)) <= VS_DEFAULT, k
            assert np.array_equal(got, np.asarray(d1[k].values).reshape(got.shape)), k
    finally:
        ds.close()


def test_component_through_radiation_step():
    import climt_amd
    from helpers import load_cache_case
    state, _, _ = load_cache_case("TestRRTMGShortwaveMCICA", "3d")
    sw = climt_amd.RRTMGShortwave(clear_sky_diagnostics=False)
    lw = climt_amd.RRTMGLongwave(allow_synthetic_tables=True)
    state = climt_amd.get_default_state([sw, lw], grid_state=climt_amd.get_grid(nx=16, ny=5, nz=28))
    (t_sw, d_sw), (t_lw, d_lw) = climt_amd.radiation_step(sw, lw, state)
    t1, d1 = sw(state)
    t2, d2 = lw(state)
    assert set(d_sw) == set(d1) == set(sw.diagnostic_properties)
    assert all(np.array_equal(d_sw[k].values, d1[k].values) for k in d1) and all(np.array_equal(d_lw[k].values, d2[k].values) for k in d2)
    assert np.array_equal(t_sw["air_temperature"].values, t1["air_temperature"].values)
