"""GPU tests of the shortwave's opt-in day-column pack (rrtmg_hip_set_sw_night_pack; run with -m gpu on an MI355X).

Inputs are climt_amd.synthetic.make_columns with coszen overwritten by a terminator field on a longitude-fastest grid of 128
longitudes: both tiles of every latitude row are mixed, so the night-column skip alone finds no night tile.  What the packed
copy looks like and what sw_night_last reports are climt_amd.night.packed_order / packed_counts (tests/test_night_pack.py
checks them by hand).  The contract: night columns +0.0 in every output; a day column's outputs are the bits of a call with
the skip off on the day columns alone (ncol = nday); against the whole grid with the skip off a cloudy day column keeps its
bits and a cloud-free one stays within 1e-10 (it may change solve variant: the column sort's bound, tests/test_gpu_parity.py);
a call that is not eligible gives the tile skip's bits and counts."""
import numpy as np
import pytest

from climt_amd import night

pytestmark = pytest.mark.gpu

BASE = dict(icld=1, iaer=0, adjes=1.0, dyofyr=1, scon=1367.0, isolvar=0, inflg=2, iceflg=1, liqflg=1)
SW_COMPONENTS = ("dirdflx", "difdflx", "dirdnuv", "difdnuv", "dirdnir", "difdnir", "dirdflxc", "difdflxc")
SW_BANDS = ("up", "dn", "upc", "dnc", "dndir", "dndirc")
NLON, NLAT, NLAY = 128, 5, 20
VARIANT_TOL = 1.0e-10      # cloud-free column in the other solve variant: the bound of the column-sort test


def terminator(nlon, nlat, shift=20.3):
    """coszen [nlat * nlon], longitude fastest: cos(lat) cos(lon - lon0).  With nlon = 128 the night half of a row is 64
    consecutive longitudes that start 20 columns into a tile: both tiles of every row are mixed."""
    lon = 2.0 * np.pi * (np.arange(nlon) + 0.5) / nlon
    lat = np.deg2rad(np.linspace(-75.0, 75.0, nlat))
    return np.ascontiguousarray((np.cos(lat)[:, None] * np.cos(lon - 2.0 * np.pi * shift / nlon)[None, :]).ravel())


def check_field(coszen, no_night_tile=True):
    """Asserted on the CPU first: day and night columns both present, and (where claimed) not one night tile for the skip."""
    dark = night.night_columns(coszen)
    assert dark.any() and not dark.all()
    if no_night_tile:
        assert night.night_tiles(coszen).sum() == 0
    return dark


def grid(nlon, nlat, nlay, seed, mcica, icld, iaer=0, irng=0):
    from climt_amd.synthetic import make_columns, overcast
    ncol = nlon * nlat
    c = make_columns(ncol, nlay, cloudy=True, seed=seed); c.pop("lat")
    for t in range(0, (ncol + 63) // 64, 5):      # every fifth tile cloud-free: both solve variants in one call
        for k in ("cldfr", "cliqwp", "cicewp"):
            c[k][:, t * 64:(t + 1) * 64] = 0.0
    if not mcica:
        c = overcast(c)
    c.update(BASE); c.update(irng=irng, permuteseed=11, icld=icld, iaer=iaer)
    rng = np.random.default_rng(seed + 1000)
    if iaer == 10:
        shape = (14, nlay, ncol)
        c.update(tauaer=0.02 * rng.uniform(0.0, 1.0, shape), ssaaer=rng.uniform(0.8, 0.99, shape), asmaer=rng.uniform(0.5, 0.8, shape))
    if iaer == 6:
        c["ecaer"] = rng.uniform(0.0, 0.08, (6, nlay, ncol))
    c["coszen"] = terminator(nlon, nlat)
    return c


def columns(c, sel):
    """The call on the columns `sel` (an index array or a slice) of c, in that order."""
    return {k: (np.ascontiguousarray(v[..., sel]) if isinstance(v, np.ndarray) and k != "indsolvar" else v) for k, v in c.items()}


def band_albedo_inputs(c):
    from climt_amd.rrtmg.shortwave import albedo_by_band_rule
    albdir, albdif = albedo_by_band_rule(c["asdir"], c["asdif"], c["aldir"], c["aldif"])
    f = np.linspace(0.7, 1.3, 14)[:, None]
    return {"albdir": np.ascontiguousarray(albdir * f), "albdif": np.ascontiguousarray(albdif * f[::-1])}


def run(ctx, c, mcica, switch, mode="device", extras=True, levels="all", surface=None, sort=False):
    """One shortwave call -> ({name: array}, (night tiles, night columns)).  switch: off | skip | pack | both (skip and pack);
    mode: host | device | deferred.  Every output starts as NaN, so an element the call did not write shows."""
    from climt_amd import _hip
    from climt_amd._lib import SW_OUT
    nlay, ncol = c["play"].shape
    nrow = 2 if levels == "boundaries" else nlay + 1
    ctx.set_sw_night_skip(switch in ("skip", "both"))
    ctx.set_sw_night_pack(switch in ("pack", "both"))
    ctx.set_column_sort(sort)
    nan = lambda *shape: np.full(shape, np.nan)
    try:
        if mode == "host":
            out = {k: nan(nlay + lev, ncol) for k, lev in SW_OUT}
            comp = {k: nan(nlay + 1, ncol) for k in SW_COMPONENTS} if extras else None
            band = {k: nan(14, nrow, ncol) for k in SW_BANDS} if extras else None
            out = dict(ctx.sw_fluxes(c, mcica=mcica, out=out, components=comp, bands=band, band_levels=levels, surface=surface))
        else:
            dev = {k: _hip.DeviceArray.from_host(v) for k, v in c.items() if isinstance(v, np.ndarray) and k != "indsolvar"}
            args = {k: v.ptr for k, v in dev.items()}
            args.update({k: v for k, v in c.items() if k not in dev}); args.update(ncol=ncol, nlay=nlay)
            dsurf = {k: _hip.DeviceArray.from_host(v) for k, v in surface.items()} if surface else None
            dout = {k: _hip.DeviceArray.from_host(nan(nlay + lev, ncol)) for k, lev in SW_OUT}
            comp = {k: _hip.DeviceArray.from_host(nan(nlay + 1, ncol)) for k in SW_COMPONENTS} if extras else None
            band = {k: _hip.DeviceArray.from_host(nan(14, nrow, ncol)) for k in SW_BANDS} if extras else None
            if mode == "deferred":
                ctx.set_deferred(True)
            try:
                ctx.sw_fluxes(args, mcica=mcica, out={k: v.ptr for k, v in dout.items()}, memspace=1,
                              components={k: v.ptr for k, v in comp.items()} if extras else None,
                              bands={k: v.ptr for k, v in band.items()} if extras else None, band_levels=levels,
                              surface={k: v.ptr for k, v in dsurf.items()} if surface else None)
                ctx.synchronize()
            finally:
                if mode == "deferred":
                    ctx.set_deferred(False)
            out = {k: v.download() for k, v in dout.items()}
            comp = {k: v.download() for k, v in comp.items()} if extras else None
            band = {k: v.download() for k, v in band.items()} if extras else None
        counts = ctx.sw_night_last()
    finally:
        ctx.set_sw_night_skip(False); ctx.set_sw_night_pack(False); ctx.set_column_sort(False)
    if extras:
        out.update({"comp." + k: v for k, v in comp.items()}); out.update({"band." + k: v for k, v in band.items()})
    return out, counts


def check_night_zero(on, dark, what=""):
    for k, b in on.items():
        assert not np.isnan(b).any(), (what, k, "an element was not written")
        z = b[..., dark]
        assert np.all(z == 0.0) and not np.signbit(z).any(), (what, k, "night columns not +0.0")


def check_equal(want, got, cols, what=""):
    assert set(want) == set(got)
    for k in want:
        assert np.array_equal(want[k][..., cols], got[k][..., cols]), (what, k)


def test_headline_128_longitudes_every_tile_mixed(gpu_ctx):
    """640 columns = 10 tiles, all mixed: the skip saves no tile, the pack half of them."""
    c = grid(NLON, NLAT, NLAY, 61, False, 0)
    dark = check_field(c["coszen"])
    assert c["coszen"].size == 640 and night.mixed_tiles(c["coszen"]).all()
    want = night.packed_counts(c["coszen"])
    assert want[0] > 0 and want == (10 - (640 - int(dark.sum()) + 63) // 64, int(dark.sum()))
    off, n_off = run(gpu_ctx, c, False, "off")
    assert n_off == (0, 0) and np.all(off["swdflx"][-1, dark] > 0.0)
    skip, n_skip = run(gpu_ctx, c, False, "skip")
    assert n_skip == (0, int(dark.sum()))
    for switch in ("pack", "both"):
        on, n_on = run(gpu_ctx, c, False, switch)
        assert n_on == want, (switch, n_on, want)
        check_night_zero(on, dark, switch)
        check_equal(off, on, ~dark, switch)
        check_equal(skip, on, slice(None), switch)


VARIANTS = {
    "clear_sky": dict(mcica=False, icld=0),
    "overcast_icld1": dict(mcica=False, icld=1),
    "mcica_kissvec_icld2": dict(mcica=True, icld=2, irng=0),
    "mcica_kissvec_icld3_iaer10": dict(mcica=True, icld=3, irng=0, iaer=10),
}


@pytest.mark.parametrize("name", list(VARIANTS))
def test_day_columns_are_the_day_only_call(gpu_ctx, name):
    v = dict(VARIANTS[name])
    mcica = v.pop("mcica")
    c = grid(NLON, NLAT, NLAY, 63, mcica, **v)
    dark = check_field(c["coszen"])
    day = np.flatnonzero(~dark)
    cloudy = (c["cldfr"] > 0.0).any(axis=0) if v["icld"] else np.zeros(dark.size, dtype=bool)
    if v["icld"]:
        assert (cloudy & ~dark).any() and (~cloudy & ~dark).any()
    want = night.packed_counts(c["coszen"])
    for mode, levels in (("device", "all"), ("deferred", "all"), ("device", "boundaries"), ("deferred", "boundaries")):
        if mode == "device":
            whole, _ = run(gpu_ctx, c, mcica, "off", levels=levels)
            alone, n0 = run(gpu_ctx, columns(c, day), mcica, "off", levels=levels)
            assert n0 == (0, 0)
        on, n_on = run(gpu_ctx, c, mcica, "pack", mode=mode, levels=levels)
        what = (name, mode, levels)
        assert n_on == want, what
        check_night_zero(on, dark, what)
        worst = 0.0
        for k in on:
            assert np.array_equal(on[k][..., day], alone[k]), (what, k, "not the bits of the day-only call")
            assert np.array_equal(on[k][..., cloudy & ~dark], whole[k][..., cloudy & ~dark]), (what, k, "cloudy day column moved")
            free = ~cloudy & ~dark
            d = float(np.abs(on[k][..., free] - whole[k][..., free]).max())
            worst = max(worst, d)
            assert d <= VARIANT_TOL, (what, k, d)
        print("%s: cloud-free day columns against the whole grid, max |d| = %.3e" % (what, worst))


def test_surface_albedo_by_band(gpu_ctx):
    c = grid(NLON, NLAT, NLAY, 65, False, 0)
    dark = check_field(c["coszen"])
    surface = band_albedo_inputs(c)
    off, _ = run(gpu_ctx, c, False, "off", surface=surface)
    plain, _ = run(gpu_ctx, c, False, "off")
    assert not np.array_equal(off["swuflx"], plain["swuflx"])      # the per-band rows are read
    on, n = run(gpu_ctx, c, False, "pack", surface=surface)
    assert n == night.packed_counts(c["coszen"])
    check_night_zero(on, dark)
    check_equal(off, on, ~dark)
    # and with the broadband pointers absent, as the header allows when both members are given
    bare = {k: v for k, v in c.items() if k not in ("asdir", "asdif", "aldir", "aldif")}
    on2, _ = run(gpu_ctx, bare, False, "pack", surface=surface)
    check_equal(on, on2, slice(None))


def test_shapes(gpu_ctx):
    base = grid(NLON, 4, NLAY, 67, False, 0)

    def both(c, what, want=None):
        dark = night.night_columns(c["coszen"])
        off, _ = run(gpu_ctx, c, False, "off")
        on, n = run(gpu_ctx, c, False, "pack")
        assert n == night.packed_counts(c["coszen"]) and (want is None or n == want), (what, n)
        check_night_zero(on, dark, what)
        check_equal(off, on, ~dark, what)
        return on
    # a ragged last tile
    c = columns(base, slice(0, 500))
    check_field(c["coszen"], no_night_tile=False)
    on500 = both(c, "ragged")
    # the day columns fill their tiles exactly: no replica slot
    c = columns(base, slice(0, 300))
    cz = np.full(300, -0.4); cz[np.arange(128) * 2 + 7] = np.linspace(0.05, 1.0, 128)
    c["coszen"] = cz
    both(c, "nday = 128", (5 - 2, 172))
    # all night
    c["coszen"] = np.where(np.arange(300) % 2 == 0, -0.5, -0.0)
    on = both(c, "all night", (5, 300))
    assert all(np.all(v == 0.0) for v in on.values())
    # all day
    c["coszen"] = np.linspace(0.05, 1.0, 300)
    both(c, "all day", (0, 0))
    # one day column
    cz = np.full(300, -0.2); cz[211] = 0.7
    c["coszen"] = cz
    both(c, "one day column", (5 - 1, 299))
    # a random permutation of the columns: the permuted outputs, bit for bit (clear sky: one solve variant)
    perm = np.random.default_rng(5).permutation(500)
    onp, n = run(gpu_ctx, columns(columns(base, slice(0, 500)), perm), False, "pack")
    assert n[1] == int(night.night_columns(base["coszen"][:500]).sum())
    for k in on500:
        assert np.array_equal(onp[k], on500[k][..., perm]), k


def test_calls_that_are_not_eligible_run_as_the_tile_skip(gpu_ctx):
    def same(c, mcica, mode, what):
        a = dict(c); b = dict(c)
        if "indsolvar" in c:
            a["indsolvar"] = c["indsolvar"].copy(); b["indsolvar"] = c["indsolvar"].copy()
        skip, n_skip = run(gpu_ctx, a, mcica, "skip", mode=mode)
        pack, n_pack = run(gpu_ctx, b, mcica, "pack", mode=mode)
        assert n_pack == n_skip == night.night_counts(c["coszen"]), (what, n_pack, n_skip)
        check_equal(skip, pack, slice(None), what)
        return a, b
    c = grid(NLON, NLAT, NLAY, 69, True, 2, irng=1)
    check_field(c["coszen"])
    same(c, True, "device", "twister")
    c = grid(NLON, NLAT, NLAY, 69, False, 0)
    c.update(isolvar=1, solcycfrac=0.3, indsolvar=np.array([1.1, 0.9]))
    a, b = same(c, False, "device", "amplitudes")
    assert np.array_equal(a["indsolvar"], b["indsolvar"]) and not np.array_equal(b["indsolvar"], c["indsolvar"])
    c = grid(NLON, NLAT, NLAY, 69, False, 0)
    same(c, False, "host", "host pointers")
    c = columns(c, slice(0, 64))
    assert night.mixed_tiles(c["coszen"]).tolist() == [True]
    same(c, False, "device", "one tile")


def test_status_codes(gpu_ctx):
    """An out-of-range ice radius (RRTMG_ERR_ICE_RADIUS, 11) in ONE column: in a night column status 0 and the clean bits, in
    a day column the code of the call with the skip off; then the context reproduces a clean call bit for bit."""
    from climt_amd._lib import RRTMGError
    c = grid(NLON, NLAT, NLAY, 71, True, 2)
    dark = check_field(c["coszen"])
    icy = (c["cicewp"] * (c["cldfr"] > 0)).sum(axis=0) > 0.0
    day_col, night_col = int(np.flatnonzero(icy & ~dark)[0]), int(np.flatnonzero(icy & dark)[0])
    clean, want = run(gpu_ctx, c, True, "pack", extras=False)
    assert want == night.packed_counts(c["coszen"])
    bad = dict(c); bad["reice"] = c["reice"].copy(); bad["reice"][:, night_col] = 500.0
    with pytest.raises(RRTMGError) as e:      # (with the skip alone the column sits in a mixed tile and is checked)
        run(gpu_ctx, bad, True, "skip", extras=False)
    assert e.value.code == 11
    got, n = run(gpu_ctx, bad, True, "pack", extras=False)      # status 0: no exception
    assert n == want
    check_equal(clean, got, slice(None))
    bad = dict(c); bad["reice"] = c["reice"].copy(); bad["reice"][:, day_col] = 500.0
    codes = []
    for switch in ("off", "pack"):
        with pytest.raises(RRTMGError) as e:
            run(gpu_ctx, bad, True, switch, extras=False)
        codes.append(e.value.code)
        assert "ICE RADIUS OUT OF BOUNDS" in str(e.value), switch
    assert codes == [11, 11]
    again, n = run(gpu_ctx, c, True, "pack", extras=False)
    assert n == want
    check_equal(clean, again, slice(None))


def test_switch_off_again_and_the_column_sort(gpu_ctx):
    c = grid(NLON, NLAT, NLAY, 73, True, 2)
    dark = check_field(c["coszen"])
    off, _ = run(gpu_ctx, c, True, "off", extras=False)
    on, n = run(gpu_ctx, c, True, "pack", extras=False)
    assert n == night.packed_counts(c["coszen"])
    again, n0 = run(gpu_ctx, c, True, "off", extras=False)
    assert n0 == (0, 0)
    check_equal(off, again, slice(None))
    # with the column sort also on the call runs packed, not sorted: the packed call's bits and counts
    both, n2 = run(gpu_ctx, c, True, "pack", extras=False, sort=True)
    assert n2 == n
    check_equal(on, both, slice(None))
    check_night_zero(both, dark)


def test_component_on_a_device_state():
    """RRTMGShortwave(skip_night_columns=True, pack_day_columns=True) through a DeviceState on a 128 x 4 grid (cloud-free
    default state: one solve variant): the skip instance's outputs bit for bit, and the packed counts."""
    import climt_amd
    sun = climt_amd.Instellation()
    skip = climt_amd.RRTMGShortwave(skip_night_columns=True)
    pack = climt_amd.RRTMGShortwave(skip_night_columns=True, pack_day_columns=True)
    state = climt_amd.get_default_state([sun, skip], grid_state=climt_amd.get_grid(nx=128, ny=4, nz=28))
    assert float(np.abs(state["cloud_area_fraction_in_atmosphere_layer"].values).max()) == 0.0
    ds = climt_amd.DeviceState.from_host(state, [sun, skip])
    try:
        ds.update(sun(ds))

        def call(comp):
            _, diag = comp(ds)
            ds.ctx.synchronize()
            return {k: q.buf.download().reshape(q.shape) for k, q in diag.items()}
        s_skip = call(skip)
        n_skip = ds.ctx.sw_night_last()
        s_pack = call(pack)
        n_pack = ds.ctx.sw_night_last()
        s_skip2 = call(skip)
        assert ds.ctx.sw_night_last() == n_skip
        z = ds.download("zenith_angle").values.ravel()
        cz = skip.night_coszen(z)
        dark = night.night_columns(cz)
        assert dark.sum() > 64 and (~dark).sum() > 64
        assert n_skip == night.night_counts(cz)
        assert n_pack == night.packed_counts(cz) and n_pack[0] > n_skip[0], (n_pack, n_skip)
        for k in s_skip:
            assert np.array_equal(s_skip[k], s_pack[k]), k
            assert np.array_equal(s_skip[k], s_skip2[k]), k
            assert np.all(s_pack[k][..., dark] == 0.0), k
    finally:
        ds.close()
