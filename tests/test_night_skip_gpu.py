"""GPU tests of the shortwave's opt-in night-column skip (rrtmg_hip_set_sw_night_skip; run with -m gpu on an MI355X).

Inputs are climt_amd.synthetic.make_columns with coszen overwritten by a terminator field, cos(lat) cos(lon - lon0) on a
longitude-fastest grid; what counts as a night column / tile is climt_amd.night (tests/test_night_skip.py checks it by hand).
With the option on every output of a day column must keep the bits of the same call with it off, and every output of a night
column must be +0.0.

Not covered: ShardedRadiation on two gloo ranks (the multi-rank tests of this suite run on the CPU emulation, which has no
night path); the one-rank RCCL form of the existing sharded GPU tests is here instead."""
import numpy as np
import pytest

from climt_amd import night

pytestmark = pytest.mark.gpu

BASE = dict(icld=1, iaer=0, adjes=1.0, dyofyr=1, scon=1367.0, isolvar=0, inflg=2, iceflg=1, liqflg=1)
SW_COMPONENTS = ("dirdflx", "difdflx", "dirdnuv", "difdnuv", "dirdnir", "difdnir", "dirdflxc", "difdflxc")
SW_BANDS = ("up", "dn", "upc", "dnc", "dndir", "dndirc")
NLON = 512


def terminator(nlon, nlat, shift=20.3):
    """coszen [nlat * nlon], longitude fastest: cos(lat) cos(lon - lon0), the sun over longitude index `shift`.  With nlon = 512
    the night half of a row is 256 consecutive longitudes that start 20 columns into a tile: of the row's 8 tiles 3 are night,
    2 mixed and 3 day."""
    lon = 2.0 * np.pi * (np.arange(nlon) + 0.5) / nlon
    lat = np.deg2rad(np.linspace(-75.0, 75.0, nlat))
    return np.ascontiguousarray((np.cos(lat)[:, None] * np.cos(lon - 2.0 * np.pi * shift / nlon)[None, :]).ravel())


def check_shares(coszen, nlon):
    """The field skips something and leaves something: >= 1/3 of the tiles night, >= 1 mixed tile per latitude row, the rest day."""
    nt, mx = night.night_tiles(coszen), night.mixed_tiles(coszen)
    assert 3 * nt.sum() >= nt.size, (int(nt.sum()), nt.size)
    per_row = nlon // 64
    assert nlon % 64 == 0 and np.all(mx.reshape(-1, per_row).sum(axis=1) >= 1)
    day = ~nt & ~mx
    assert day.sum() >= 1 and nt.sum() + mx.sum() + day.sum() == nt.size
    dark = night.night_columns(coszen)
    assert np.all(coszen[~dark] > 0.0)
    return dark


def grid(nlon, nlat, nlay, seed, mcica, icld, iaer=0, irng=0):
    from climt_amd.synthetic import make_columns, overcast
    ncol = nlon * nlat
    c = make_columns(ncol, nlay, cloudy=True, seed=seed); c.pop("lat")
    # every fifth 64-column tile cloud-free: both solve variants in one call, on both sides of the terminator
    for t in range(0, (ncol + 63) // 64, 5):
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


def band_albedo_inputs(c):
    from climt_amd.rrtmg.shortwave import albedo_by_band_rule
    albdir, albdif = albedo_by_band_rule(c["asdir"], c["asdif"], c["aldir"], c["aldif"])
    f = np.linspace(0.7, 1.3, 14)[:, None]
    return {"albdir": np.ascontiguousarray(albdir * f), "albdif": np.ascontiguousarray(albdif * f[::-1])}


def run(ctx, c, mcica, skip, mode="host", extras=True, levels="all", surface=None):
    """One shortwave call -> ({name: array}, (night tiles, night columns)); names: the six plain outputs, and with `extras`
    comp.<member> and band.<member>.  mode: host | device | deferred (device pointers, collected by synchronize())."""
    from climt_amd import _hip
    from climt_amd._lib import SW_OUT
    nlay, ncol = c["play"].shape
    nrow = 2 if levels == "boundaries" else nlay + 1
    ctx.set_sw_night_skip(skip)
    try:
        if mode == "host":
            comp = {k: np.full((nlay + 1, ncol), np.nan) for k in SW_COMPONENTS} if extras else None
            band = {k: np.full((14, nrow, ncol), np.nan) for k in SW_BANDS} if extras else None
            out = dict(ctx.sw_fluxes(c, mcica=mcica, components=comp, bands=band, band_levels=levels, surface=surface))
        else:
            dev = {k: _hip.DeviceArray.from_host(v) for k, v in c.items() if isinstance(v, np.ndarray)}
            args = {k: v.ptr for k, v in dev.items()}
            args.update({k: v for k, v in c.items() if not isinstance(v, np.ndarray)}); args.update(ncol=ncol, nlay=nlay)
            dsurf = {k: _hip.DeviceArray.from_host(v) for k, v in surface.items()} if surface else None
            dout = {k: _hip.DeviceArray((nlay + lev, ncol)) for k, lev in SW_OUT}
            comp = {k: _hip.DeviceArray((nlay + 1, ncol)) for k in SW_COMPONENTS} if extras else None
            band = {k: _hip.DeviceArray((14, nrow, ncol)) for k in SW_BANDS} if extras else None
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
        ctx.set_sw_night_skip(False)
    if extras:
        out.update({"comp." + k: v for k, v in comp.items()}); out.update({"band." + k: v for k, v in band.items()})
    return out, counts


def check_on_against_off(off, on, dark, what=""):
    """Day columns: the bits of the off-run.  Night columns: +0.0 everywhere."""
    assert set(off) == set(on)
    for k in off:
        a, b = off[k], on[k]
        assert not np.isnan(b).any(), (what, k)
        assert np.array_equal(a[..., ~dark], b[..., ~dark]), (what, k, "day columns moved")
        z = b[..., dark]
        assert np.all(z == 0.0) and not np.signbit(z).any(), (what, k, "night columns not +0.0")


VARIANTS = {
    "clear_sky": dict(mcica=False, icld=0),
    "overcast_icld1": dict(mcica=False, icld=1),
    "mcica_kissvec_icld2": dict(mcica=True, icld=2, irng=0),
    "mcica_twister_icld1": dict(mcica=True, icld=1, irng=1),
    "mcica_kissvec_icld3": dict(mcica=True, icld=3, irng=0),
    "mcica_twister_icld3_iaer6": dict(mcica=True, icld=3, irng=1, iaer=6),
    "mcica_kissvec_icld2_iaer10": dict(mcica=True, icld=2, irng=0, iaer=10),
    "overcast_icld2_iaer6": dict(mcica=False, icld=2, iaer=6),
}


@pytest.mark.parametrize("name", list(VARIANTS))
def test_off_on_comparison_all_variants_and_memspaces(gpu_ctx, name):
    """512 x 16 columns x 60 layers, components, band fluxes (both `levels`) and the albedo by band all requested; host
    pointers, device pointers and deferred mode.  sw_night_last is the numpy helper's counts for every on-call, 0 / 0 for off."""
    v = dict(VARIANTS[name])
    mcica = v.pop("mcica")
    c = grid(NLON, 16, 60, 31, mcica, **v)
    dark = check_shares(c["coszen"], NLON)
    want = night.night_counts(c["coszen"])
    assert want[0] >= 16 * 3 and want[1] == 16 * 256
    surface = band_albedo_inputs(c)
    off, n_off = run(gpu_ctx, c, mcica, False, surface=surface)
    assert n_off == (0, 0)
    # the test discriminates: without the skip the night columns receive the clamped sun
    assert np.all(off["swdflx"][-1, dark] > 0.0) and np.all(off["band.dn"][:, -1][:, dark].sum(axis=0) > 0.0)
    assert float(off["swdflx"][-1, ~dark].max()) > 100.0
    for mode in ("host", "device", "deferred"):
        on, n_on = run(gpu_ctx, c, mcica, True, mode=mode, surface=surface)
        assert n_on == want, (name, mode, n_on, want)
        check_on_against_off(off, on, dark, (name, mode))
    # the two boundary rows only; and the plain call (no components, bands or surface struct)
    off2, _ = run(gpu_ctx, c, mcica, False, levels="boundaries", surface=surface)
    on2, n2 = run(gpu_ctx, c, mcica, True, mode="device", levels="boundaries", surface=surface)
    assert n2 == want
    check_on_against_off(off2, on2, dark, (name, "boundaries"))
    assert all(np.array_equal(off2["band." + m][:, 1], off["band." + m][:, 60]) for m in SW_BANDS)
    offp, n0 = run(gpu_ctx, c, mcica, False, extras=False)
    onp, n1 = run(gpu_ctx, c, mcica, True, extras=False)
    assert n0 == (0, 0) and n1 == want
    check_on_against_off(offp, onp, dark, (name, "plain"))
    # off after on: the switch leaves nothing behind
    again, n_again = run(gpu_ctx, c, mcica, False, extras=False)
    assert n_again == (0, 0) and all(np.array_equal(again[k], offp[k]) for k in offp)


def test_live_reference_day_columns_and_its_own_night_values(gpu_ctx):
    """2048 columns (512 x 4) through the reference Fortran (oracle/_ref).  Day columns with the skip on stay within the bound
    of tests/test_gpu_parity.py::test_against_live_oracle_at_larger_size for the shortwave: FLUX_TOL / HR_TOL and `tight=5.0e-8`
    (quoted from there, with its reasoning: reftra near k mu0 = 1).  The reference's own night values satisfy
    |F| <= 1e-10 * scon * adjes * (1 + 1e-6): its driver clamps coszen to 1e-10 and nothing in a column can exceed the
    incoming beam, so our zeros are within that of the reference.  dyofyr = 0 here, so that the Earth-Sun factor IS adjes."""
    from oracle import ref_driver
    from test_gpu_parity import FLUX_TOL, HR_TOL
    from helpers import maxdiff, require_reference_oracle
    c = grid(NLON, 4, 60, 99, True, 2)
    c.update(dyofyr=0, adjes=1.0, permuteseed=684)
    dark = check_shares(c["coszen"], NLON)
    if ref_driver.available("sw"):
        rsw = ref_driver.RefSW()
        parts = []
        for s in range(0, 2048, 256):      # (the reference keeps (ngpt, ncol, nlay) automatics on the stack)
            sub = {k: (v[..., s:s + 256] if isinstance(v, np.ndarray) else v) for k, v in c.items()}
            parts.append(rsw.fluxes(sub, mcica=True))
        exp = {k: np.concatenate([p[k] for p in parts], axis=1) for k in ("swuflx", "swdflx", "swhr", "swuflxc", "swdflxc", "swhrc")}
    else:
        from oracle.port_driver import PortSW
        require_reference_oracle("port")
        exp = PortSW().fluxes(c, mcica=True)
    on, counts = run(gpu_ctx, c, True, True, extras=False)
    assert counts == night.night_counts(c["coszen"])
    for k, e in exp.items():
        d = maxdiff(on[k][:, ~dark], e[:, ~dark])
        print("live reference, day columns, %s: max |d| = %.3e" % (k, d))
        assert d <= (HR_TOL if k.endswith(("hr", "hrc")) else FLUX_TOL), (k, d)
        assert d <= 5.0e-8, (k, d)
    bound = 1.0e-10 * c["scon"] * c["adjes"] * (1.0 + 1.0e-6)
    for k in ("swuflx", "swdflx", "swuflxc", "swdflxc"):
        worst = float(np.abs(exp[k][:, dark]).max())
        print("live reference, its night columns, %s: max |F| = %.6e (bound %.6e)" % (k, worst, bound))
        assert worst <= bound, (k, worst, bound)
        assert np.all(on[k][:, dark] == 0.0)
    assert float(exp["swdflx"][-1, dark].min()) > 0.0


def test_shapes_ragged_chunks_all_night_all_day(gpu_ctx):
    # ncol not a multiple of 64, the last (short) tile all night, the one before it mixed
    c = grid(64, 6, 40, 41, True, 2)
    c = {k: (np.ascontiguousarray(v[..., :343]) if isinstance(v, np.ndarray) else v) for k, v in c.items()}
    cz = np.full(343, 0.6); cz[100:140] = -0.1; cz[300:] = -0.4
    c["coszen"] = cz
    assert night.night_tiles(cz).tolist() == [False, False, False, False, False, True] and night.mixed_tiles(cz)[4]
    off, _ = run(gpu_ctx, c, True, False)
    on, n = run(gpu_ctx, c, True, True)
    assert n == (1, 83)
    check_on_against_off(off, on, night.night_columns(cz), "ragged")
    # more than one column chunk: 512 x 33 = 16 896 columns = 264 tiles, chunks of 128 (a grid of one kind of tile: one with
    # both kinds is given chunks of up to 2048 tiles)
    c = grid(NLON, 33, 60, 43, False, 0)
    dark = check_shares(c["coszen"], NLON)
    off, _ = run(gpu_ctx, c, False, False, extras=False)
    on, n = run(gpu_ctx, c, False, True, mode="device", extras=False)
    assert n == night.night_counts(c["coszen"]) and n[0] >= 99
    assert gpu_ctx.kernel_launches("sw") >= 2
    check_on_against_off(off, on, dark, "chunks")
    # an all-night grid: everything zero, every tile a night tile
    c = grid(64, 11, 40, 45, True, 2)
    c = {k: (np.ascontiguousarray(v[..., :700]) if isinstance(v, np.ndarray) else v) for k, v in c.items()}
    c["coszen"] = np.where(np.arange(700) % 2 == 0, -0.5, -0.0)
    on, n = run(gpu_ctx, c, True, True)
    assert n == (11, 700)
    for k, v in on.items():
        assert np.all(v == 0.0) and not np.signbit(v).any(), k
    # an all-day grid: bit-equal to off, no night tile
    c["coszen"] = np.full(700, 0.3); c["coszen"][5] = 0.25; c["coszen"][6] = 1.0e-300
    off, _ = run(gpu_ctx, c, True, False)
    on, n = run(gpu_ctx, c, True, True)
    assert n == (0, 0) and all(np.array_equal(off[k], on[k]) for k in off)


def test_nan_coszen_is_day(gpu_ctx):
    """A NaN cosine is not night: the column is solved as without the skip (whatever that gives), its tile is not a night tile."""
    c = grid(64, 2, 30, 47, False, 0)
    cz = np.full(128, -0.2); cz[70] = np.nan
    c["coszen"] = cz
    off, _ = run(gpu_ctx, c, False, False, extras=False)
    on, n = run(gpu_ctx, c, False, True, extras=False)
    assert n == (1, 127)
    dark = night.night_columns(cz)
    for k in off:
        assert np.array_equal(off[k][:, 70], on[k][:, 70], equal_nan=True), k
        assert np.all(on[k][:, dark] == 0.0), k


@pytest.mark.parametrize("blocks", [((0, 768), (768, 2048)), ((0, 512), (512, 1472), (1472, 2048))])
def test_tile_aligned_shards_equal_the_whole_with_the_twister(gpu_ctx, blocks):
    from climt_amd.distributed import slice_columns
    c = grid(NLON, 4, 40, 51, True, 2, irng=1)
    dark = check_shares(c["coszen"], NLON)
    whole, n = run(gpu_ctx, c, True, True)
    assert n == night.night_counts(c["coszen"])
    off, _ = run(gpu_ctx, c, True, False)
    check_on_against_off(off, whole, dark, "whole")
    parts, tiles, cols = [], 0, 0
    for lo, hi in blocks:
        sub = slice_columns(c, lo, hi); sub.update(shard_col0=lo, shard_ncol=2048)
        p, (t, k) = run(gpu_ctx, sub, True, True)
        parts.append(p); tiles += t; cols += k
    assert (tiles, cols) == n
    for k in whole:
        assert np.array_equal(np.concatenate([p[k] for p in parts], axis=-1), whole[k]), k


def test_status_codes(gpu_ctx):
    """An out-of-range ice radius (RRTMG_ERR_ICE_RADIUS, 11: tests/helpers.py STOP_CASES) in ONE column.  In a day column: the
    same code with the skip on as off, and the context then reproduces a clean call bit for bit.  The same value inside a night
    tile: status 0 and zeros."""
    from climt_amd._lib import RRTMGError
    c = grid(NLON, 2, 40, 53, True, 2)
    dark = check_shares(c["coszen"], NLON)
    tiles = night.night_tiles(c["coszen"])
    icy = (c["cicewp"] * (c["cldfr"] > 0)).sum(axis=0) > 0.0
    in_night_tile = np.repeat(tiles, 64)
    day_col = int(np.flatnonzero(icy & ~dark)[0])
    night_col = int(np.flatnonzero(icy & in_night_tile)[0])
    clean_off, _ = run(gpu_ctx, c, True, False, extras=False)
    clean_on, want = run(gpu_ctx, c, True, True, extras=False)
    bad = dict(c); bad["reice"] = c["reice"].copy(); bad["reice"][:, day_col] = 500.0
    for skip in (False, True):
        with pytest.raises(RRTMGError) as e:
            run(gpu_ctx, bad, True, skip, extras=False)
        assert e.value.code == 11 and "ICE RADIUS OUT OF BOUNDS" in str(e.value), skip
    again, n = run(gpu_ctx, c, True, True, extras=False)
    assert n == want and all(np.array_equal(again[k], clean_on[k]) for k in again)
    bad = dict(c); bad["reice"] = c["reice"].copy(); bad["reice"][:, night_col] = 500.0
    with pytest.raises(RRTMGError) as e:      # (without the skip the night column is solved, and checked)
        run(gpu_ctx, bad, True, False, extras=False)
    assert e.value.code == 11
    got, n = run(gpu_ctx, bad, True, True, extras=False)      # status 0: no exception
    assert n == want and all(np.array_equal(got[k], clean_on[k]) for k in got)
    check_on_against_off(clean_off, got, dark, "bad input in a night tile")


def test_component_on_a_host_state():
    """RRTMGShortwave(skip_night_columns=True) on a host state with zenith angles on both sides of 90 degrees."""
    import climt_amd
    plain, skip = climt_amd.RRTMGShortwave(), climt_amd.RRTMGShortwave(skip_night_columns=True)
    state = climt_amd.get_default_state([plain], grid_state=climt_amd.get_grid(nx=64, ny=6, nz=28))
    z = state["zenith_angle"].values
    z[:] = np.deg2rad(np.linspace(20.0, 160.0, z.size)).reshape(z.shape)
    dark = skip.night_coszen(z) <= 0.0
    assert dark.any() and not dark.all() and np.array_equal(dark, z >= 0.5 * np.pi)
    t0, d0 = plain(state)
    t1, d1 = skip(state)
    t2, d2 = plain(state)      # the shared context is switched back by the default instance
    for got, want, again in ((t1, t0, t2), (d1, d0, d2)):
        assert set(got) == set(want)
        for k in want:
            a, b = want[k], got[k]
            assert a.dims == b.dims and a.attrs == b.attrs
            hor = tuple(a.dims.index(x) for x in state["zenith_angle"].dims)
            av, bv = np.moveaxis(a.values, hor, (-2, -1)), np.moveaxis(b.values, hor, (-2, -1))
            assert np.array_equal(av[..., ~dark], bv[..., ~dark]), k
            assert np.all(bv[..., dark] == 0.0) and not np.signbit(bv[..., dark]).any(), k
            assert np.array_equal(again[k].values, a.values), k
    top = d0["downwelling_shortwave_flux_in_air"]      # without the skip the night columns receive the clamped sun
    hor = tuple(top.dims.index(x) for x in state["zenith_angle"].dims)
    assert np.all(np.moveaxis(top.values, hor, (-2, -1))[..., dark].max(axis=0) > 0.0)


def test_component_on_a_device_state_with_instellation():
    """A DeviceState step whose zenith angle comes from the Instellation kernel: night columns zero, day columns the default
    instance's bits, the longwave component's outputs bit-equal either way.  (The kernel clamps the zenith angle to pi/2, whose
    cosine is +6e-17: the component hands the library 0.0 there.)"""
    import climt_amd
    sun = climt_amd.Instellation()
    plain, skip = climt_amd.RRTMGShortwave(), climt_amd.RRTMGShortwave(skip_night_columns=True)
    lw = climt_amd.RRTMGLongwave(allow_synthetic_tables=True)
    state = climt_amd.get_default_state([sun, plain, lw], grid_state=climt_amd.get_grid(nx=256, ny=6, nz=28))
    ds = climt_amd.DeviceState.from_host(state, [sun, plain, lw])
    try:
        ds.update(sun(ds))

        def call(comp):
            _, diag = comp(ds)
            ds.ctx.synchronize()
            return {k: q.buf.download().reshape(q.shape) for k, q in diag.items()}
        s_off, l_off = call(plain), call(lw)
        assert ds.ctx.sw_night_last() == (0, 0)
        s_on, l_on = call(skip), call(lw)
        tiles, cols = ds.ctx.sw_night_last()
        s_off2 = call(plain)
        # Instellation clamps the zenith angle to pi/2: those columns are the night (RRTMGShortwave.night_coszen)
        z = ds.download("zenith_angle").values.ravel()
        dark = z >= 0.5 * np.pi
        day = ~dark
        assert dark.sum() > 256 and day.sum() > 256
        assert (tiles, cols) == night.night_counts(skip.night_coszen(z)) and tiles >= 1, (tiles, cols)
        for k in s_off:
            assert np.array_equal(s_off[k][..., day], s_on[k][..., day]), k
            assert np.all(s_on[k][..., dark] == 0.0) and not np.signbit(s_on[k][..., dark]).any(), k
            assert np.array_equal(s_off[k], s_off2[k]), k
        assert float(s_off["downwelling_shortwave_flux_in_air"][-1][dark].min()) > 0.0
        for k in l_off:
            assert np.array_equal(l_off[k], l_on[k]), k
    finally:
        ds.close()


def test_sharded_radiation_over_a_night_skipping_context(gpu_ctx):
    """climt_amd.distributed.ShardedRadiation (one rank, RCCL collective forced, as the existing sharded GPU tests run it) on a
    context with the skip on: the gathered outputs are those of the plain device call with the skip on."""
    from climt_amd.distributed import RcclComm, ShardedRadiation
    c = grid(NLON, 2, 40, 57, True, 2)
    dark = check_shares(c["coszen"], NLON)
    off, _ = run(gpu_ctx, c, True, False, extras=False)
    want, n = run(gpu_ctx, c, True, True, extras=False)
    lw = gpu_ctx.lw_fluxes(c, mcica=True)
    comm = RcclComm(0, 1, 0)
    try:
        gpu_ctx.set_sw_night_skip(True)
        sr = ShardedRadiation(gpu_ctx, comm, 1024, 40, gather="all", force=True)
        sr.set_inputs(c)
        for i in range(2):
            b = sr.step(mcica=True, sync=(i == 1))
        sr.finish()
        got = sr.gathered_host(b)
        assert gpu_ctx.sw_night_last() == n
        sr.close()
    finally:
        gpu_ctx.set_sw_night_skip(False)
        gpu_ctx.set_deferred(False)
        comm.close()
    assert all(np.array_equal(got[k], want[k]) for k in want) and all(np.array_equal(got[k], lw[k]) for k in lw)
    check_on_against_off(off, {k: got[k] for k in off}, dark, "sharded")
