"""GPU tests of the joint shortwave + longwave host call (rrtmg_hip_radiation_fluxes, Context.radiation_fluxes,
climt_amd.radiation_step; run with -m gpu on an MI355X).

The reference is the library's own separate calls -- rrtmg_hip_sw_fluxes* followed by rrtmg_hip_lw_fluxes* on the same
arguments, on a second context that never sees a joint call -- which the rest of the suite pins to the reference Fortran.
Every comparison is bit for bit (np.array_equal; outputs are pre-filled with NaN, so an element that was not written fails).

Shapes: 130 x 30 (three 64-column tiles, the last ragged; every array is below kScanMin = 131 072 doubles, so inputs take the
plain upload path) and 2240 x 60 (134 400 doubles per layer array >= kScanMin, 35 tiles: the scan / fill / absent paths run, and
the well-mixed gases are uniform)."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

KSCANMIN = 1 << 17
BASE = dict(iaer=0, adjes=1.0, dyofyr=1, scon=1367.0, isolvar=0, inflg=2, iceflg=1, liqflg=1, idrv=0)
SW_COMPONENTS = ("dirdflx", "difdflx", "dirdnuv", "difdnuv", "dirdnir", "difdnir", "dirdflxc", "difdflxc")
SW_BANDS = ("up", "dn", "upc", "dnc", "dndir", "dndirc")
LW_BANDS = ("up", "dn", "upc", "dnc")
# the inputs both argument structs have, by the cloud switch under which both spectra read them
SHARED_ALWAYS = ("play", "plev", "tlay", "h2o", "o3", "co2", "ch4", "n2o", "o2")
SHARED_CLOUDS = ("cldfr", "cicewp", "cliqwp", "reice", "reliq")
SCALE_OF = {"play": ("pressure_scale",), "plev": ("pressure_scale",), "cicewp": ("water_path_scale",), "cliqwp": ("water_path_scale",),
            "h2o": ("h2o_mul", "h2o_div")}


@pytest.fixture(scope="module")
def sep_ctx():
    """A second context for the separate calls: it never sees a joint call."""
    from climt_amd._lib import Context
    from oracle.ref_driver import CONSTANTS, CPDAIR
    ctx = Context(0)
    ctx.set_constants(**CONSTANTS)
    ctx.sw_init(CPDAIR)
    ctx.lw_init(CPDAIR)
    yield ctx
    ctx.close()


_columns = {}


def columns(ncol, nlay, kind, **flags):
    """climt_amd.synthetic inputs, made once per (shape, kind) and never modified: clear | mcica | overcast."""
    from climt_amd.synthetic import make_columns, overcast
    key = (ncol, nlay, kind)
    if key not in _columns:
        c = make_columns(ncol, nlay, cloudy=kind != "clear", seed=20 + ncol % 7)
        c.pop("lat")
        if kind == "overcast":
            c = overcast(c)
            c = {k: (np.ascontiguousarray(v) if isinstance(v, np.ndarray) else v) for k, v in c.items()}
        _columns[key] = c
    c = dict(_columns[key])
    c.update(BASE)
    c.update(icld={"clear": 0, "mcica": 2, "overcast": 1}[kind])
    if kind == "mcica":
        c.update(irng=0, permuteseed=7)
    c.update(flags)
    return c


def aerosols(c, nband, seed):
    nlay, ncol = c["play"].shape
    rng = np.random.default_rng(seed)
    shape = (nband, nlay, ncol)
    if nband == 14:
        return dict(iaer=10, tauaer=0.02 * rng.uniform(0.0, 1.0, shape), ssaaer=rng.uniform(0.8, 0.99, shape), asmaer=rng.uniform(0.5, 0.8, shape))
    return dict(tauaer=0.01 * rng.uniform(0.0, 1.0, shape))


def band_albedo_inputs(c):
    from climt_amd.rrtmg.shortwave import albedo_by_band_rule
    albdir, albdif = albedo_by_band_rule(c["asdir"], c["asdif"], c["aldir"], c["aldif"])
    f = np.linspace(0.7, 1.3, 14)[:, None]
    return {"albdir": np.ascontiguousarray(albdir * f), "albdif": np.ascontiguousarray(albdif * f[::-1])}


def call_args(swc, lwc, sw_mcica, lw_mcica, full=False, surface=None):
    """Fresh, NaN-filled outputs around the inputs -> (sw kwargs, lw kwargs) of Context.sw_fluxes / lw_fluxes / radiation_fluxes."""
    from climt_amd._lib import LW_OUT, SW_OUT
    nlay, ncol = swc["play"].shape
    nan = lambda *shape: np.full(shape, np.nan)
    sw = dict(inp=swc, mcica=sw_mcica, out={k: nan(nlay + lev, ncol) for k, lev in SW_OUT})
    lw = dict(inp=lwc, mcica=lw_mcica, out={k: nan(nlay + lev, ncol) for k, lev in LW_OUT})
    if lwc.get("idrv"):
        lw["out"].update(duflx_dt=nan(nlay + 1, ncol), duflxc_dt=nan(nlay + 1, ncol))
    if full:
        sw.update(components={k: nan(nlay + 1, ncol) for k in SW_COMPONENTS}, bands={k: nan(14, nlay + 1, ncol) for k in SW_BANDS})
        lw.update(bands={k: nan(16, nlay + 1, ncol) for k in LW_BANDS})
    if surface is not None:
        sw.update(surface=surface)
    return sw, lw


def flat(sw, lw):
    out = {"sw." + k: v for k, v in sw["out"].items()}
    out.update({"lw." + k: v for k, v in lw["out"].items()})
    for tag, kw in (("sw", sw), ("lw", lw)):
        for group in ("components", "bands"):
            out.update({"%s.%s.%s" % (tag, group, k): v for k, v in (kw.get(group) or {}).items()})
    return out


def separate(ctx, make):
    sw, lw = make()
    ctx.sw_fluxes(**sw)
    ctx.lw_fluxes(**lw)
    return flat(sw, lw)


def joint(ctx, make):
    sw, lw = make()
    ctx.radiation_fluxes(sw=sw, lw=lw)
    return flat(sw, lw)


def assert_same_bits(got, want, what=""):
    assert set(got) == set(want)
    for k in want:
        assert not np.isnan(want[k]).any(), (what, k, "the separate call left elements unwritten")
        assert np.array_equal(got[k], want[k]), (what, k, float(np.nanmax(np.abs(got[k] - want[k]))))


def expected_sharing(swc, lwc):
    """-> (arrays, bytes): the non-NULL inputs common to both structs, passed as the same array with equal unit factors, and the
    summed sizes of those that have structure (a uniform array of >= kScanMin doubles is filled on the device: no bytes)."""
    names = SHARED_ALWAYS + (SHARED_CLOUDS if swc["icld"] and lwc["icld"] else ())
    n = nbytes = 0
    for k in names:
        a = swc.get(k)
        if a is None or a is not lwc.get(k) or any(swc.get(s, 0.0) != lwc.get(s, 0.0) for s in SCALE_OF.get(k, ())):
            continue
        n += 1
        if a.size < KSCANMIN or not np.all(a.ravel() == a.flat[0]):
            nbytes += a.nbytes
    return n, nbytes


def bits_case(shape, name):
    ncol, nlay = shape
    full, surface = False, None
    if name == "clear":
        swc = lwc = columns(ncol, nlay, "clear")
        mcica = False
    elif name == "overcast_icld1":
        swc = lwc = columns(ncol, nlay, "overcast")
        mcica = False
    elif name == "mcica_kissvec_icld2" and ncol > 2000:      # every optional output, aerosols, albedo by band, idrv
        base = columns(ncol, nlay, "mcica")
        swc = dict(base, **aerosols(base, 14, 5))
        lwc = dict(base, idrv=1, **aerosols(base, 16, 6))
        mcica, full, surface = True, True, band_albedo_inputs(base)
    elif name == "mcica_kissvec_icld2":
        swc = lwc = columns(ncol, nlay, "mcica")
        mcica = True
    elif name == "mcica_twister_shard":
        swc = lwc = columns(ncol, nlay, "mcica", irng=1, permuteseed=12345, shard_col0=70, shard_ncol=400)
        mcica = True
    else:
        raise KeyError(name)
    return lambda: call_args(swc, lwc, mcica, mcica, full=full, surface=surface), swc, lwc


BITS = [((130, 30), n) for n in ("clear", "mcica_kissvec_icld2", "overcast_icld1", "mcica_twister_shard")] + \
       [((2240, 60), n) for n in ("clear", "mcica_kissvec_icld2", "overcast_icld1")]


@pytest.mark.parametrize("shape,name", BITS, ids=["%dx%d-%s" % (s + (n,)) for s, n in BITS])
def test_bits_equal_the_separate_calls(gpu_ctx, sep_ctx, shape, name):
    make, swc, lwc = bits_case(shape, name)
    want = separate(sep_ctx, make)
    got = joint(gpu_ctx, make)
    assert_same_bits(got, want, "joint")
    assert gpu_ctx.radiation_last()[0] == expected_sharing(swc, lwc)[0] > 0
    # the same joint call again (cached fills, work buffers), then a separate call on the context that ran the joint ones
    assert_same_bits(joint(gpu_ctx, make), want, "joint, repeated")
    assert_same_bits(separate(gpu_ctx, make), want, "separate, after joint")
    # the event pairs of rrtmg_hip_kernel_ms are per spectrum, as after separate calls
    assert gpu_ctx.kernel_ms("sw") > 0.0 and gpu_ctx.kernel_ms("lw") > 0.0


def test_bits_with_subcolumns_given(gpu_ctx, sep_ctx):
    """cldfmcl given for both spectra (112 and 140 sub-columns: two arrays of their own, nothing to share between them)."""
    c = columns(130, 30, "mcica")
    swc = dict(c, cldfmcl=sep_ctx.mcica_mask("sw", c["play"], c["cldfr"], 2, 3, 0))
    lwc = dict(c, cldfmcl=sep_ctx.mcica_mask("lw", c["play"], c["cldfr"], 2, 4, 0))
    make = lambda: call_args(swc, lwc, True, True)
    assert_same_bits(joint(gpu_ctx, make), separate(sep_ctx, make))


def test_what_was_shared(gpu_ctx, sep_ctx):
    c = columns(2240, 60, "clear")
    make = lambda: call_args(c, c, False, False)
    want = separate(sep_ctx, make)
    assert_same_bits(joint(gpu_ctx, make), want)
    n, nbytes = expected_sharing(c, c)
    assert n == 9 and nbytes == 8 * (4 * 2240 * 60 + 2240 * 61)      # play, tlay, h2o, o3 and plev have structure; four gases are uniform
    shared, uploaded, saved = gpu_ctx.radiation_last()
    assert (shared, saved) == (n, nbytes)
    # what the call copied: the five structured arrays once, the shortwave's four albedos and coszen, the longwave's tlev, tsfc
    # and emis (its CFCs are uniform: filled)
    assert uploaded == nbytes + 8 * (5 * 2240 + 2240 * 61 + 2240 + 16 * 2240)
    # every shared array passed to the longwave as a copy: nothing matches, everything is uploaded twice, same bits
    lwc = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in c.items()}
    assert_same_bits(joint(gpu_ctx, lambda: call_args(c, lwc, False, False)), want, "copies")
    shared2, uploaded2, saved2 = gpu_ctx.radiation_last()
    assert (shared2, saved2) == (0, 0) == expected_sharing(c, lwc) and uploaded2 == uploaded + nbytes


def test_keys_that_must_not_match(gpu_ctx, sep_ctx):
    c = columns(2240, 60, "mcica")
    # (a) pressures in Pa with pressure_scale = 0.01 for the shortwave; the longwave has pre-scaled arrays of its own
    play_pa, plev_pa = c["play"] * 100.0, c["plev"] * 100.0
    swc = dict(c, play=play_pa, plev=plev_pa, pressure_scale=0.01)
    lwc = dict(c, play=play_pa * 0.01, plev=plev_pa * 0.01)
    make = lambda: call_args(swc, lwc, True, True)
    assert_same_bits(joint(gpu_ctx, make), separate(sep_ctx, make), "pressure_scale")
    assert gpu_ctx.radiation_last()[0] == expected_sharing(swc, lwc)[0] == 12
    # (b) the same pointers under different factors: the pressures (Pa with 0.01 for the shortwave, 0.0099 for the longwave: an
    # atmosphere one per cent thinner, as valid as the other) and the water vapour (two roundings against one)
    swc = dict(c, play=play_pa, plev=plev_pa, pressure_scale=0.01, h2o_mul=28.964, h2o_div=18.02)
    lwc = dict(c, play=play_pa, plev=plev_pa, pressure_scale=0.0099, h2o_mul=28.964 / 18.02)
    make = lambda: call_args(swc, lwc, True, True)
    assert_same_bits(joint(gpu_ctx, make), separate(sep_ctx, make), "same pointer, other factors")
    assert gpu_ctx.radiation_last()[0] == expected_sharing(swc, lwc)[0] == 11
    # (c) one array as cicewp of the shortwave and cliqwp of the longwave: shared, content is what counts
    swc, lwc = dict(c), dict(c, cliqwp=c["cicewp"])
    make = lambda: call_args(swc, lwc, True, True)
    assert_same_bits(joint(gpu_ctx, make), separate(sep_ctx, make), "cicewp as cliqwp")
    shared, _, saved = gpu_ctx.radiation_last()
    assert shared == expected_sharing(swc, lwc)[0] + 1 == 14      # thirteen by name, and the longwave's cliqwp from the shortwave's cicewp
    # (d) a uniform cloud fraction of zeros (filled on the device: no bytes) and a structured one
    o = columns(2240, 60, "overcast")
    z = dict(o, cldfr=np.zeros_like(o["cldfr"]))
    saved_by = {}
    for tag, cc in (("zeros", z), ("structured", o)):
        make = lambda: call_args(cc, cc, False, False)
        assert_same_bits(joint(gpu_ctx, make), separate(sep_ctx, make), tag)
        shared, _, saved_by[tag] = gpu_ctx.radiation_last()
        assert (shared, saved_by[tag]) == expected_sharing(cc, cc)
    assert saved_by["structured"] - saved_by["zeros"] == o["cldfr"].nbytes


def test_status_codes(gpu_ctx, sep_ctx):
    """A liquid radius the longwave refuses (RRTMG_ERR_LIQ_RADIUS, 12: tests/helpers.py STOP_CASES) with valid shortwave inputs,
    the mirrored case with an ice radius the shortwave refuses (11), and both."""
    from climt_amd._lib import RRTMGError
    c = columns(130, 30, "mcica")
    bad_lw = dict(c, reliq=np.full_like(c["reliq"], 1.0))
    bad_sw = dict(c, reice=np.full_like(c["reice"], 500.0))
    clean = lambda: call_args(c, c, True, False)
    want = separate(sep_ctx, clean)
    for swc, lwc, code, who, intact in ((c, bad_lw, 12, "longwave", "sw."), (bad_sw, c, 11, "shortwave", "lw."), (bad_sw, bad_lw, 11, "shortwave", None)):
        sw, lw = call_args(swc, lwc, True, False)
        with pytest.raises(RRTMGError) as e:
            gpu_ctx.radiation_fluxes(sw=sw, lw=lw)
        assert e.value.code == code and who in str(e.value), str(e.value)
        got = flat(sw, lw)
        for k in want:
            if intact and k.startswith(intact):
                assert np.array_equal(got[k], want[k]), (who, k)
        assert_same_bits(joint(gpu_ctx, clean), want, "clean call after a %s failure" % who)
    assert_same_bits(separate(gpu_ctx, clean), want)


def raw_structs(ctx, sw, lw, keep):
    from climt_amd._lib import RadiationCall
    a, sf, c, b, _ = ctx._sw_structs(sw["inp"], sw["mcica"], sw["out"], 0, sw.get("components"), sw.get("bands"), "all", sw.get("surface"), keep)
    la, lb, _ = ctx._lw_structs(lw["inp"], lw["mcica"], lw["out"], 0, lw.get("bands"), "all", keep)
    call = RadiationCall()
    call.struct_size = C.sizeof(RadiationCall)
    call.sw, call.lw = C.pointer(a), C.pointer(la)
    call.sw_surface, call.sw_components, call.sw_bands, call.lw_bands = C.pointer(sf), C.pointer(c), C.pointer(b), C.pointer(lb)
    return call, dict(sw=a, sw_surface=sf, sw_components=c, sw_bands=b, lw=la, lw_bands=lb)


REFUSALS = [("call", "struct_size", 8), ("sw", "struct_size", 0), ("sw_surface", "struct_size", 4), ("sw_components", "struct_size", 1),
            ("sw_bands", "struct_size", 999), ("lw", "struct_size", 12), ("lw_bands", "struct_size", 0),
            ("sw", "memspace", 1), ("lw", "memspace", 1), ("lw", "ncol", 129), ("sw", "nlay", 29), ("lw", "shard_col0", 1)]


def test_refused_before_anything_is_written(gpu_ctx, sep_ctx):
    """RRTMG_ERR_ARG (4) and not one output element written (all outputs stay NaN), then the same arguments untouched: clean."""
    base = columns(130, 30, "mcica")
    surface = band_albedo_inputs(base)
    make = lambda: call_args(base, base, True, True, full=True, surface=surface)
    want = separate(sep_ctx, make)
    for where, field, value in REFUSALS:
        sw, lw = make()
        keep = []
        call, members = raw_structs(gpu_ctx, sw, lw, keep)
        setattr(call if where == "call" else members[where], field, value)
        rc = gpu_ctx.lib.rrtmg_hip_radiation_fluxes(gpu_ctx.h, C.byref(call))
        assert rc == 4, (where, field, rc, gpu_ctx.lib.rrtmg_hip_last_error(gpu_ctx.h))
        for k, v in flat(sw, lw).items():
            assert np.isnan(v).all(), (where, field, k)
    sw, lw = make()
    call, _ = raw_structs(gpu_ctx, sw, lw, [])
    assert gpu_ctx.lib.rrtmg_hip_radiation_fluxes(gpu_ctx.h, C.byref(call)) == 0
    assert_same_bits(flat(sw, lw), want)


def test_pending_deferred_work_is_collected_first(gpu_ctx, sep_ctx):
    """A deferred device-resident shortwave call on a poisoned input is left pending; the host joint call that follows collects
    its flag (as call_own_flag documents for a synchronous call: the pending error is what it returns), and the next is clean."""
    from climt_amd import _hip
    from climt_amd._lib import RRTMGError, SW_OUT
    c = columns(130, 30, "mcica")
    nlay, ncol = c["play"].shape
    bad = dict(c, reice=np.full_like(c["reice"], 500.0))
    make = lambda: call_args(c, c, True, True)
    want = separate(sep_ctx, make)
    dev = {k: _hip.DeviceArray.from_host(v) for k, v in bad.items() if isinstance(v, np.ndarray)}
    args = {k: v.ptr for k, v in dev.items()}
    args.update({k: v for k, v in bad.items() if not isinstance(v, np.ndarray)}); args.update(ncol=ncol, nlay=nlay)
    dout = {k: _hip.DeviceArray((nlay + lev, ncol)) for k, lev in SW_OUT}
    gpu_ctx.set_deferred(True)
    try:
        gpu_ctx.sw_fluxes(args, mcica=True, out={k: v.ptr for k, v in dout.items()}, memspace=1)      # returns once enqueued
        with pytest.raises(RRTMGError) as e:
            joint(gpu_ctx, make)
        assert e.value.code == 11 and "shortwave" in str(e.value)
        assert_same_bits(joint(gpu_ctx, make), want, "joint call after the collection, deferred mode still on")
    finally:
        gpu_ctx.set_deferred(False)
    assert_same_bits(joint(gpu_ctx, make), want)


def test_radiation_last_before_any_joint_call(sep_ctx):
    from climt_amd._lib import RRTMGError
    with pytest.raises(RRTMGError) as e:
        sep_ctx.radiation_last()
    assert e.value.code == 4


def terminator_zenith(shape):
    """Zenith angles on both sides of 90 degrees, a night stretch longer than a 64-column tile (climt_amd.night states the tiles)."""
    return np.deg2rad(np.linspace(20.0, 160.0, int(np.prod(shape)))).reshape(shape)


@pytest.mark.parametrize("case", ["default", "mcica_kissvec_night_skip"])
def test_radiation_step_equals_the_two_component_calls(case):
    import climt_amd
    from climt_amd import night
    kw = dict(mcica=True, random_number_generator="kissvec", cloud_overlap_method="maximum_random") if case != "default" else {}
    sw = climt_amd.RRTMGShortwave(skip_night_columns=case != "default", **kw)
    lw = climt_amd.RRTMGLongwave(allow_synthetic_tables=True, **kw)
    state = climt_amd.get_default_state([sw, lw], grid_state=climt_amd.get_grid(nx=16, ny=10, nz=30))
    if case != "default":
        z = state["zenith_angle"].values
        z[:] = terminator_zenith(z.shape)
        assert night.night_tiles(sw.night_coszen(z).ravel()).any()
        frac = state["cloud_area_fraction_in_atmosphere_layer"].values
        frac[3:9] = 0.5
        state["mass_content_of_cloud_liquid_water_in_atmosphere_layer"].values[3:9] = 0.03
    np.random.seed(5)
    want = (sw(state), lw(state))
    np.random.seed(5)
    got = climt_amd.radiation_step(sw, lw, state)
    assert sw._ctx.radiation_last()[0] > 0
    for (gt, gd), (wt, wd) in zip(got, want):
        for g, w in ((gt, wt), (gd, wd)):
            assert list(g) == list(w)
            for k in w:
                assert type(g[k]) is type(w[k]) and g[k].dims == w[k].dims and g[k].attrs == w[k].attrs, k
                assert np.array_equal(g[k].values, w[k].values), k
    for (t, d), name in zip(got + want, ["shortwave", "longwave"] * 2):
        alias = np.shares_memory(d["air_temperature_tendency_from_" + name].values, t["air_temperature"].values)
        assert alias == (name == "longwave"), name
    if case != "default":
        dark = (state["zenith_angle"].values >= 0.5 * np.pi).ravel()
        down = got[0][1]["downwelling_shortwave_flux_in_air"].values.reshape(31, -1)
        assert dark.any() and np.all(down[:, dark] == 0.0) and np.all(down[-1, ~dark] > 0.0)
