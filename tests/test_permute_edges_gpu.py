"""GPU tests of the edges of the column-permutation engine (csrc/rrtmg_permute.h; run with -m gpu on an MI355X): the one slot
map that serves the column sort (rrtmg_hip_set_column_sort) and the day-column pack (rrtmg_hip_set_sw_night_pack), where a
block is empty, fills its tiles exactly, or holds one column, on grids of two and three tiles with and without a ragged last
tile.  tools/permute_check.cpp checks the same map on the CPU; the larger grids are tests/test_gpu_parity.py (the sort at 1000
columns) and tests/test_night_pack_gpu.py.

Sort: make_columns at 6 layers with every column made cloudy, then clouds removed (cldfr, cliqwp, cicewp zeroed) by pattern.
The asserts are those of the sort test of tests/test_gpu_parity.py: every element written, a cloudy column has the bits of
the unsorted call, a cloud-free one is within 1e-10 of it and has the bits of the call on the cloud-free columns alone.
Pack: coszen fields at the same sizes with no day column, no night column and exactly 64 day columns; the asserts of
tests/test_night_pack_gpu.py.  Its test_shapes has these three fields at 300 columns of 20 clear-sky layers only, so none of
them is skipped here: these have clouds (McICA, both solve variants), 128 columns (no ragged tile) and a day block of one tile."""
import numpy as np
import pytest

from climt_amd import night
from test_night_pack_gpu import check_night_zero, columns
from test_night_pack_gpu import run as run_sw_night

pytestmark = pytest.mark.gpu

BASE = dict(icld=1, iaer=0, adjes=1.0, dyofyr=1, scon=1367.0, isolvar=0, inflg=2, iceflg=1, liqflg=1)
NLAY = 6
SIZES = (128, 130, 191)
VARIANT_TOL = 1.0e-10      # cloud-free column in the other solve variant: the bound of the column-sort test
CLOUD_KEYS = ("cldfr", "cliqwp", "cicewp")
PATTERNS = ("none_cloudy", "all_cloudy", "64_cloud_free", "one_cloud_free", "one_cloudy")


def all_cloudy(ncol, mcica, seed):
    """make_columns with a cloud in EVERY column: a cloud-free column takes the three cloud arrays of a cloudy one."""
    from climt_amd.synthetic import make_columns, overcast
    c = make_columns(ncol, NLAY, cloudy=True, seed=seed); c.pop("lat")
    if not mcica:
        c = overcast(c)
    has = (c["cldfr"] > 0).any(axis=0)
    donors = np.flatnonzero(has)
    assert donors.size > 0 and (~has).any()
    for i, col in enumerate(np.flatnonzero(~has)):
        for k in CLOUD_KEYS:
            c[k] = c[k].copy()
            c[k][:, col] = c[k][:, donors[i % donors.size]]
    assert (c["cldfr"] > 0).any(axis=0).all()
    c.update(BASE); c.update(irng=0, permuteseed=17, icld=2 if mcica else 1)
    return c


def cloud_free_columns(ncol, pattern):
    """-> bool [ncol]: the columns whose clouds are removed.  The 64 are spread over every tile (no tile of one kind)."""
    free = np.zeros(ncol, dtype=bool)
    if pattern == "none_cloudy":
        free[:] = True
    elif pattern == "64_cloud_free":
        free[ncol - 1] = True      # (one of each kind in a ragged last tile of two columns, too)
        free[np.random.default_rng(ncol).permutation(ncol - 2)[:63]] = True
        assert all(0 < free[t:t + 64].sum() < free[t:t + 64].size for t in range(0, ncol, 64))
    elif pattern == "one_cloud_free":
        free[ncol - 2] = True
    elif pattern == "one_cloudy":
        free[:] = True; free[70] = False
    return free


def with_pattern(c, free):
    c = dict(c)
    for k in CLOUD_KEYS:
        c[k] = c[k].copy(); c[k][:, free] = 0.0
    assert np.array_equal((c["cldfr"] > 0).any(axis=0), ~free)
    return c


def run(ctx, spectrum, inp, mcica, sort):
    """One device-resident call of one spectrum -> {name: array}; every output starts as NaN."""
    from climt_amd import _hip
    from climt_amd._lib import LW_OUT, SW_OUT
    nlay, ncol = inp["play"].shape
    outs = list(SW_OUT if spectrum == "sw" else LW_OUT)
    if spectrum == "lw" and inp.get("idrv"):
        outs += [("duflx_dt", 1), ("duflxc_dt", 1)]
    dev = {k: _hip.DeviceArray.from_host(v) for k, v in inp.items() if isinstance(v, np.ndarray)}
    args = {k: v.ptr for k, v in dev.items()}
    args.update({k: v for k, v in inp.items() if not isinstance(v, np.ndarray)}); args.update(ncol=ncol, nlay=nlay)
    out = {k: _hip.DeviceArray.from_host(np.full((nlay + lev, ncol), np.nan)) for k, lev in outs}
    ctx.set_column_sort(sort)
    try:
        (ctx.sw_fluxes if spectrum == "sw" else ctx.lw_fluxes)(args, mcica=mcica, out={k: v.ptr for k, v in out.items()}, memspace=1)
    finally:
        ctx.set_column_sort(False)
    return {k: v.download() for k, v in out.items()}


def check_sorted(ctx, spectrum, c, free, mcica, what):
    plain = run(ctx, spectrum, c, mcica, False)
    srt = run(ctx, spectrum, c, mcica, True)
    alone = run(ctx, spectrum, columns(c, np.flatnonzero(free)), mcica, True) if free.any() else None
    for k in plain:
        assert not np.isnan(plain[k]).any() and not np.isnan(srt[k]).any(), (what, k, "an element was not written")
        assert np.array_equal(srt[k][:, ~free], plain[k][:, ~free]), (what, k, "cloudy column moved")
        if free.any():
            d = float(np.abs(srt[k][:, free] - plain[k][:, free]).max())
            assert d <= VARIANT_TOL, (what, k, d)
            assert np.array_equal(srt[k][:, free], alone[k]), (what, k, "not the bits of the cloud-free columns alone")
    return plain


@pytest.fixture(scope="module")
def base_columns():
    """The all-cloudy inputs by (ncol, mcica): built once, never changed (with_pattern copies what it edits)."""
    return {(n, m): all_cloudy(n, m, 40 + n) for n in SIZES for m in (True, False)}


@pytest.mark.parametrize("mcica", [False, True], ids=["nomcica", "mcica"])
@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("ncol", SIZES)
def test_sort_edges(gpu_ctx, base_columns, ncol, pattern, mcica):
    free = cloud_free_columns(ncol, pattern)
    c = with_pattern(base_columns[(ncol, mcica)], free)
    for spectrum in ("sw", "lw"):
        check_sorted(gpu_ctx, spectrum, c, free, mcica, (spectrum, ncol, pattern, mcica))


@pytest.mark.parametrize("extra", ["idrv", "tauaer"])
def test_sort_longwave_lists(gpu_ctx, base_columns, extra):
    """What only the longwave's gather and output lists hold: the two idrv = 1 outputs, and tauaer ([16][nlay][ncol])."""
    ncol, mcica = 191, True
    free = cloud_free_columns(ncol, "64_cloud_free")
    c = with_pattern(base_columns[(ncol, mcica)], free)
    ref = run(gpu_ctx, "lw", c, mcica, False)
    if extra == "idrv":
        c["idrv"] = 1
    else:
        c["tauaer"] = 0.05 * np.random.default_rng(3).uniform(0.0, 1.0, (16, NLAY, ncol))
    plain = check_sorted(gpu_ctx, "lw", c, free, mcica, extra)
    if extra == "idrv":
        assert set(plain) - set(ref) == {"duflx_dt", "duflxc_dt"} and np.all(plain["duflx_dt"][0] > 0.0)
    else:
        assert not np.array_equal(plain["uflx"], ref["uflx"])      # the aerosol optical depth is read


def pack_coszen(ncol, pattern):
    """Terminator-like fields: the sign of coszen flips by column, the day values spread over (0, 1]."""
    cz = -0.1 - 0.5 * np.abs(np.cos(np.arange(ncol)))
    if pattern == "no_night":
        cz = 0.05 + 0.9 * np.abs(np.cos(np.arange(ncol)))
    elif pattern == "64_day":
        cz[np.arange(64) * 2 + 1] = np.linspace(0.05, 1.0, 64)      # every tile but a ragged third one is mixed
    return cz


@pytest.mark.parametrize("pattern", ["no_day", "no_night", "64_day"])
@pytest.mark.parametrize("ncol", SIZES)
def test_pack_edges(gpu_ctx, base_columns, ncol, pattern):
    mcica = True
    free = cloud_free_columns(ncol, "64_cloud_free")
    c = with_pattern(base_columns[(ncol, mcica)], free)
    c["coszen"] = pack_coszen(ncol, pattern)
    dark = night.night_columns(c["coszen"])
    nday = int((~dark).sum())
    assert nday == {"no_day": 0, "no_night": ncol, "64_day": 64}[pattern]
    what = (ncol, pattern)
    whole, n0 = run_sw_night(gpu_ctx, c, mcica, "off")
    on, n_on = run_sw_night(gpu_ctx, c, mcica, "pack")
    assert n0 == (0, 0) and n_on == night.packed_counts(c["coszen"]) == ((ncol + 63) // 64 - (nday + 63) // 64, ncol - nday), (what, n_on)
    check_night_zero(on, dark, what)
    if nday:
        alone, _ = run_sw_night(gpu_ctx, columns(c, np.flatnonzero(~dark)), mcica, "off")
        for k in on:
            assert np.array_equal(on[k][..., ~dark], alone[k]), (what, k, "not the bits of the day-only call")
            assert np.array_equal(on[k][..., ~free & ~dark], whole[k][..., ~free & ~dark]), (what, k, "cloudy day column moved")
            if (free & ~dark).any():
                d = float(np.abs(on[k][..., free & ~dark] - whole[k][..., free & ~dark]).max())
                assert d <= VARIANT_TOL, (what, k, d)
