"""Solar variability where a column's position matters (tests/solvar_cases.py), on the GPU: 136 columns x 12 layers -- two
full tiles and a ragged one -- with facular / sunspot amplitudes that the host rescales once per column of the call.  The
per-column multipliers are a positional input; every path that moves columns must hand each column ITS multipliers and leave
the caller's `indsolvar` as one call of the reference over the grid does: against the reference fixtures first, then every
other path bit for bit against the host-pointer call."""
import numpy as np
import pytest

import solvar_cases as S
from helpers import CONSTANTS, CPDAIR, band_rule, maxdiff

pytestmark = pytest.mark.gpu

TIGHT = 5.0e-9       # the project's bound for committed fixtures (tests/test_gpu_parity.py)
L1 = S.NLAY + 1
_BASE = {}


def _plain(gpu_ctx, case):
    """The host-pointer call of the case, once: (inputs, mcica, fixture, outputs -- read-only --, amplitudes as it left them)."""
    if case not in _BASE:
        c, mcica, fx = S.load_case(case)
        call = S.fresh(c)
        out = gpu_ctx.sw_fluxes(call, mcica=mcica)
        for v in out.values():
            v.setflags(write=False)
        _BASE[case] = (c, mcica, fx, out, call["indsolvar"].copy())
    return _BASE[case]


def _same(got, want, what):
    for k in want:
        assert np.array_equal(got[k], want[k]), (what, k, maxdiff(got[k], want[k]))


def _device_call(ctx, c, mcica, ncol=S.NCOL):
    """The call on device pointers (`indsolvar` stays the caller's HOST array under either memspace) -> (outputs downloaded by
    `fetch()`, the amplitudes array of this call)."""
    from climt_amd import _hip
    from climt_amd._lib import SW_OUT
    call = S.fresh(c)
    dev = {k: _hip.DeviceArray.from_host(v) for k, v in call.items() if isinstance(v, np.ndarray) and k != "indsolvar"}
    args = {k: v.ptr for k, v in dev.items()}
    args.update({k: v for k, v in call.items() if k not in dev})
    args.update(ncol=ncol, nlay=S.NLAY)
    out = {k: _hip.DeviceArray((S.NLAY + lev, ncol)) for k, lev in SW_OUT}
    for v in out.values():
        v.upload(np.full(v.shape, -7.0))      # (every element must be written)
    ctx.sw_fluxes(args, mcica=mcica, out={k: v.ptr for k, v in out.items()}, memspace=1)
    return (lambda: {k: v.download() for k, v in out.items()}), call["indsolvar"], dev


@pytest.mark.parametrize("case", list(S.CASES))
def test_host_pointer_call_meets_the_reference(gpu_ctx, case):
    """Every column within TIGHT of ONE reference call over the grid (an excess that grows with the column index would be a
    column reading another column's multipliers), and the amplitudes come back EQUAL to the reference's."""
    c, mcica, fx, out, ind = _plain(gpu_ctx, case)
    for k, v in S.expected(fx).items():
        d = np.abs(out[k] - v).max(axis=0)
        print("%s %s: max |d| = %.3e at column %d" % (case, k, d.max(), int(d.argmax())))
        assert d.max() <= TIGHT, (case, k, float(d.max()), int(d.argmax()))
    assert np.array_equal(ind, fx["indsolvar"]), (case, ind, fx["indsolvar"])


@pytest.mark.parametrize("case", list(S.CASES))
def test_device_pointers_and_deferred_mode_keep_the_bits(gpu_ctx, case):
    c, mcica, _, plain, ind = _plain(gpu_ctx, case)
    fetch, got_ind, keep = _device_call(gpu_ctx, c, mcica)
    _same(fetch(), plain, "memspace 1")
    assert np.array_equal(got_ind, ind)
    gpu_ctx.set_deferred(True)
    try:
        fetch, got_ind, keep = _device_call(gpu_ctx, c, mcica)
        gpu_ctx.synchronize()
        _same(fetch(), plain, "deferred")
        assert np.array_equal(got_ind, ind)
    finally:
        gpu_ctx.set_deferred(False)


def test_column_chunks_keep_the_bits(gpu_ctx, monkeypatch):
    """A second context under RRTMG_HIP_CHUNK_TILES=1: three chunks, the multipliers indexed by the column of the CALL."""
    from climt_amd._lib import Context
    base = {case: _plain(gpu_ctx, case) for case in S.CASES}
    monkeypatch.setenv("RRTMG_HIP_CHUNK_TILES", "1")
    small = Context(0)
    try:
        small.set_constants(**CONSTANTS); small.sw_init(CPDAIR)
        for case, (c, mcica, _, plain, ind) in base.items():
            call = S.fresh(c)
            out = small.sw_fluxes(call, mcica=mcica)
            assert small.kernel_launches("sw", cloudy=False) == 3, case
            _same(out, plain, case)
            assert np.array_equal(call["indsolvar"], ind), case
    finally:
        small.close()


@pytest.mark.parametrize("case", S.NIGHT_CASES)
def test_night_skip_keeps_day_columns_and_the_rescale_steps_of_night_columns(gpu_ctx, case):
    """Night columns are exact zeros, day columns keep their bits -- the night run in the middle of the grid still counts as
    rescale steps, as in the reference (inatm_sw runs before the zenith test) -- and sw_night_last reports the run."""
    c, mcica, _, plain, ind = _plain(gpu_ctx, case)
    night = c["coszen"] <= 0.0
    assert night.sum() == S.NIGHT[1] - S.NIGHT[0]
    gpu_ctx.set_sw_night_skip(True)
    try:
        call = S.fresh(c)
        out = gpu_ctx.sw_fluxes(call, mcica=mcica)
        assert gpu_ctx.sw_night_last() == (0, int(night.sum()))
    finally:
        gpu_ctx.set_sw_night_skip(False)
    for k in plain:
        assert np.array_equal(out[k][:, ~night], plain[k][:, ~night]), (case, k)
        assert not out[k][:, night].any() and not np.signbit(out[k][:, night]).any(), (case, k)
    assert np.array_equal(call["indsolvar"], ind)


@pytest.mark.parametrize("case", list(S.CASES))
def test_tile_aligned_shards_equal_the_whole(gpu_ctx, case):
    from climt_amd.distributed import slice_columns
    c, mcica, _, plain, ind = _plain(gpu_ctx, case)
    for lo, hi in S.SHARDS:
        sub = slice_columns(S.fresh(c), lo, hi)
        sub.update(shard_col0=lo, shard_ncol=S.NCOL)
        out = gpu_ctx.sw_fluxes(sub, mcica=mcica)
        for k in plain:
            assert np.array_equal(out[k], plain[k][:, lo:hi]), (case, (lo, hi), k, maxdiff(out[k], plain[k][:, lo:hi]))
        assert np.array_equal(sub["indsolvar"], ind), (case, (lo, hi))


def test_sharded_radiation_on_device_equals_the_whole(gpu_ctx):
    """ShardedRadiation (device-resident blocks, deferred mode) over the three blocks, one after the other on one GPU:
    `indsolvar` stays a host array of the caller, every block's columns get the whole grid's bits and every block leaves the
    whole grid's amplitudes."""
    from climt_amd.distributed import ShardedRadiation

    class Comm:
        world = 3

        def __init__(self, rank):
            self.rank = rank

        def wait(self):
            pass
    case = "mcica_i2_s0"
    c, mcica, _, plain, ind = _plain(gpu_ctx, case)
    for rank in range(3):
        call = S.fresh(c)
        sr = ShardedRadiation(gpu_ctx, Comm(rank), S.NCOL, S.NLAY, gather="none")
        try:
            assert (sr.lo, sr.hi) == S.SHARDS[rank]
            sr.set_inputs(call)
            got = sr.local_host(sr.step(mcica=mcica))
        finally:
            sr.close()
        for k in plain:
            assert np.array_equal(got[k], plain[k][:, sr.lo:sr.hi]), (rank, k)
        assert np.array_equal(call["indsolvar"], ind), rank


@pytest.mark.parametrize("case", list(S.CASES))
def test_bands_components_and_surface_calls_keep_the_bits(gpu_ctx, case):
    """rrtmg_hip_sw_fluxes_bands, _components and _surface (the albedo by band set to the broadband rule): their standard outputs
    and `indsolvar` equal the plain call's bit for bit; the band rows meet the reference's (the integration kernels of these
    outputs read the multipliers of their own)."""
    c, mcica, fx, plain, ind = _plain(gpu_ctx, case)
    albdir, albdif = band_rule(c)
    band = {"dn": np.zeros((14, 2, S.NCOL))}
    comp = {"dirdflx": np.zeros((L1, S.NCOL)), "difdflx": np.zeros((L1, S.NCOL))}
    band2 = {"dn": np.zeros((14, 2, S.NCOL))}
    for what, kw in (("bands", dict(bands=band, band_levels="boundaries")), ("components", dict(components=comp)),
                     ("surface", dict(surface=dict(albdir=albdir, albdif=albdif), bands=band2, band_levels="boundaries"))):
        call = S.fresh(c)
        out = gpu_ctx.sw_fluxes(call, mcica=mcica, **kw)
        _same(out, plain, (case, what))
        assert np.array_equal(call["indsolvar"], ind), (case, what)
    assert np.array_equal(band["dn"], band2["dn"])
    assert np.array_equal(comp["difdflx"], plain["swdflx"] - comp["dirdflx"])
    assert np.all(np.abs(band["dn"].sum(axis=0) - plain["swdflx"][[0, S.NLAY]]) <= 256 * 2.0 ** -53 * np.abs(plain["swdflx"][[0, S.NLAY]]))
    if case in S.BAND_CASES:
        d = maxdiff(band["dn"], fx["band/dn"])
        print("%s band/dn: max |d| = %.3e" % (case, d))
        assert d <= TIGHT, (case, d)


@pytest.mark.parametrize("case", S.CLOUDY_CASES)
def test_column_sort_on(gpu_ctx, case):
    """rrtmg_hip_set_column_sort with amplitudes != 1: cloudy columns keep the bits of the unsorted call, cloud-free ones stay
    within 1e-10 W m^-2 of it (the two rules of the sort), every column meets the reference, and `indsolvar` comes back as from
    the unsorted call -- rescaled once per column of the CALL, not per slot of the padded internal copy."""
    c, mcica, fx, plain, ind = _plain(gpu_ctx, case)
    cloudy = (c["cldfr"] > 0).any(axis=0)
    try:
        gpu_ctx.set_column_sort(True)
        fetch, got_ind, keep = _device_call(gpu_ctx, c, mcica)
        srt = fetch()
    finally:
        gpu_ctx.set_column_sort(False)
    for k in plain:
        d = np.abs(srt[k] - plain[k]).max(axis=0)
        print("%s %s sorted - unsorted: max |d| = %.3e at column %d" % (case, k, d.max(), int(d.argmax())))
    for k, v in S.expected(fx).items():
        print("%s %s sorted - reference: max |d| = %.3e" % (case, k, maxdiff(srt[k], v)))
    print("%s indsolvar sorted %r unsorted %r" % (case, got_ind, ind))
    for k in plain:
        assert np.array_equal(srt[k][:, cloudy], plain[k][:, cloudy]), (case, k, maxdiff(srt[k][:, cloudy], plain[k][:, cloudy]))
        assert maxdiff(srt[k][:, ~cloudy], plain[k][:, ~cloudy]) <= 1e-10, (case, k, maxdiff(srt[k][:, ~cloudy], plain[k][:, ~cloudy]))
    for k, v in S.expected(fx).items():
        assert maxdiff(srt[k], v) <= TIGHT, (case, k, maxdiff(srt[k], v))
    assert np.array_equal(got_ind, ind), (case, got_ind, ind)


def test_column_sort_on_leaves_the_amplitudes_of_a_call_without_multipliers(gpu_ctx):
    """isolvar 0 with amplitudes != 1: no per-column multipliers exist, but the reference still rescales the IN/OUT array once
    per column of the call; only `indsolvar` is at stake."""
    case = "mcica_i1_s1365"
    c, mcica, _, _, _ = _plain(gpu_ctx, case)
    c = dict(c, isolvar=0)
    call = S.fresh(c)
    want = gpu_ctx.sw_fluxes(call, mcica=mcica)
    want_ind = call["indsolvar"].copy()
    assert not np.array_equal(want_ind, S.amplitudes(0))
    try:
        gpu_ctx.set_column_sort(True)
        fetch, got_ind, keep = _device_call(gpu_ctx, c, mcica)
        srt = fetch()
    finally:
        gpu_ctx.set_column_sort(False)
    print("isolvar 0: indsolvar sorted %r unsorted %r" % (got_ind, want_ind))
    assert np.array_equal(got_ind, want_ind), (got_ind, want_ind)
    cloudy = (c["cldfr"] > 0).any(axis=0)
    for k in want:
        assert np.array_equal(srt[k][:, cloudy], want[k][:, cloudy]) and maxdiff(srt[k], want[k]) <= 1e-10, k
