"""Every grid array of a call through the three paths that hand the driver a COPY of the caller's arrays (run with -m gpu on an
MI355X): the column sort and the day pack (csrc/rrtmg_permute.h) and the float32 boundary (csrc/rrtmg_precision.h), which walk
the array lists of csrc/rrtmg_call_arrays.h.  A characterisation test: the optional arrays the other suites never put through
those paths -- shortwave aerosols (iaer 10 and 6), the band-fastest cloud optics of inflag 0, the caller's sub-columns, the
longwave's CFCs, aerosol and interface temperatures, idrv -- on the smallest grid that passes both gates.

130 columns x 6 layers (two full tiles and a ragged one of two columns; the sort wants ncol >= 128, the pack ncol > 64).
Inputs: tests/test_permute_edges_gpu.py's all_cloudy -- the sort is then a pure permutation and no comparison needs a
tolerance -- rounded to float32 and widened again, so that ONE fp64 call is the reference of the sorted, the packed and the
float32 call.  Every array differs by column (uniform ones times 1 + 1e-3 * column): a gather of the wrong column or the wrong
array changes bits.  Before anything is compared, every array under test is shown to matter: zeroed (tlev: left out), the
plain call gives other fluxes."""
import numpy as np
import pytest

from climt_amd import night
from climt_amd._lib import LW_BAND_FLUXES, SW_BAND_FLUXES, SW_COMPONENTS
from test_boundary_f32_gpu import device_call, same_as_rounded, widened
from test_night_pack_gpu import check_night_zero
from test_permute_edges_gpu import NLAY, all_cloudy, pack_coszen

pytestmark = pytest.mark.gpu

NCOL = 130
BAND_FASTEST = ("taucld", "ssacld", "asmcld", "fsfcld", "cldfmcl")      # [nlay][ncol][k]: the column is the middle axis
UNIFORM = ("co2", "ch4", "n2o", "o2", "cfc11", "cfc12", "cfc22", "ccl4", "reliq", "reice")


def base(mcica, seed):
    c = all_cloudy(NCOL, mcica, seed)
    by_column = 1.0 + 1.0e-3 * np.arange(NCOL)
    for k in UNIFORM:
        c[k] = c[k] * by_column
    c["emis"] = 0.8 * c["emis"] * by_column
    return c, np.random.default_rng(seed + 1)


def sw_a():
    """inflag 2, iaer 10, McICA with the caller's sub-columns."""
    c, rng = base(True, 71)
    shape = (14, NLAY, NCOL)
    c.update(iaer=10, tauaer=0.05 * rng.uniform(0.2, 1.0, shape), ssaaer=rng.uniform(0.8, 0.99, shape), asmaer=rng.uniform(0.5, 0.8, shape))
    c["cldfmcl"] = (rng.uniform(0.0, 1.0, (NLAY, NCOL, 112)) < c["cldfr"][:, :, None]).astype(np.float64)
    return c, True, ("tauaer", "ssaaer", "asmaer", "cldfmcl")


def sw_b():
    """inflag 0: the cloud optics given by band; iaer 6; no McICA."""
    c, rng = base(False, 72)
    shape = (NLAY, NCOL, 14)
    cloud = (c["cldfr"] > 0)[:, :, None]
    c.update(inflg=0, iaer=6, taucld=cloud * rng.uniform(1.0, 8.0, shape), ssacld=rng.uniform(0.7, 0.999, shape),
             asmcld=rng.uniform(0.7, 0.9, shape), fsfcld=rng.uniform(0.4, 0.7, shape), ecaer=rng.uniform(0.01, 0.08, (6, NLAY, NCOL)))
    return c, False, ("taucld", "ssacld", "asmcld", "fsfcld", "ecaer")


def lw_a():
    """All four CFCs, the aerosol optical depth, interface temperatures of the caller's, idrv 1, McICA kissvec."""
    c, rng = base(True, 73)
    c["tlev"] = c["tlev"] + 0.5 * np.cos(np.arange(NCOL))[None, :]
    c.update(idrv=1, tauaer=0.05 * rng.uniform(0.2, 1.0, (16, NLAY, NCOL)))
    return c, True, ("cfc11", "cfc12", "cfc22", "ccl4", "tauaer", "tlev")


def lw_b():
    """inflag 0: the cloud optical depth given by band; no interface temperatures; idrv 0."""
    c, rng = base(False, 74)
    c.pop("tlev")
    c.update(inflg=0, idrv=0, taucld=(c["cldfr"] > 0)[:, :, None] * rng.uniform(0.5, 6.0, (NLAY, NCOL, 16)))
    return c, False, ("taucld",)


CASES = {"sw_a": ("sw", sw_a), "sw_b": ("sw", sw_b), "lw_a": ("lw", lw_a), "lw_b": ("lw", lw_b)}


def rounded(c):
    x32 = {k: (v.astype(np.float32) if isinstance(v, np.ndarray) else v) for k, v in c.items()}
    return x32, widened(x32)


def day_columns(c, sel):
    return {k: (np.ascontiguousarray(v[:, sel] if k in BAND_FASTEST else v[..., sel]) if isinstance(v, np.ndarray) else v) for k, v in c.items()}


def equal_bits(got, want, what):
    assert set(got) == set(want), (what, sorted(got), sorted(want))
    for k in want:
        assert not np.isnan(got[k]).any() and not np.isnan(want[k]).any(), (what, k, "an element was not written")
        assert np.array_equal(got[k], want[k]), (what, k)


@pytest.fixture(scope="module")
def plain(gpu_ctx):
    """name -> (which, x32, x64, mcica, arrays under test, the plain fp64 call): built once, never changed."""
    res = {}
    for name, (which, make) in CASES.items():
        c, mcica, under_test = make()
        x32, x64 = rounded(c)
        res[name] = (which, x32, x64, mcica, under_test, device_call(gpu_ctx, which, x64, np.float64, mcica))
    return res


@pytest.mark.parametrize("name", list(CASES))
def test_every_array_under_test_matters(gpu_ctx, plain, name):
    which, _, x64, mcica, under_test, ref = plain[name]
    flux = "swuflx" if which == "sw" else "uflx"
    for k in under_test:
        without = {j: v for j, v in x64.items() if j != k} if k == "tlev" else dict(x64, **{k: np.zeros_like(x64[k])})
        assert not np.array_equal(device_call(gpu_ctx, which, without, np.float64, mcica)[flux], ref[flux]), (name, k, "is not read")
    if name == "lw_a":
        assert set(ref) == {"uflx", "dflx", "hr", "uflxc", "dflxc", "hrc", "duflx_dt", "duflxc_dt"} and np.all(ref["duflx_dt"][0] > 0.0)


@pytest.mark.parametrize("name", list(CASES))
def test_column_sort_keeps_the_bits(gpu_ctx, plain, name):
    which, _, x64, mcica, _, ref = plain[name]
    gpu_ctx.set_column_sort(True)
    try:
        got = device_call(gpu_ctx, which, x64, np.float64, mcica)
    finally:
        gpu_ctx.set_column_sort(False)
    equal_bits(got, ref, name)


def sw_extras(name):
    """Components and band fluxes, every level and the two boundary levels: shortwave A only (none: the standard outputs)."""
    if name != "sw_a":
        return [{}]
    return [dict(components=SW_COMPONENTS, bands=SW_BAND_FLUXES, band_levels=lv) for lv in ("all", "boundaries")]


@pytest.mark.parametrize("name", ["sw_a", "sw_b"])
def test_day_pack_keeps_the_bits(gpu_ctx, plain, name):
    _, _, x64, mcica, _, _ = plain[name]
    c = dict(x64, coszen=pack_coszen(NCOL, "64_day").astype(np.float32).astype(np.float64))
    dark = night.night_columns(c["coszen"])
    assert int((~dark).sum()) == 64
    for kw in sw_extras(name):
        gpu_ctx.set_sw_night_pack(True)
        try:
            on = device_call(gpu_ctx, "sw", c, np.float64, mcica, **kw)
            counts = gpu_ctx.sw_night_last()
        finally:
            gpu_ctx.set_sw_night_pack(False)
        assert counts == night.packed_counts(c["coszen"]) == (2, NCOL - 64), (name, counts)
        assert len(on) == (6 + 8 + 6 if kw else 6)
        check_night_zero(on, dark, name)
        alone = device_call(gpu_ctx, "sw", day_columns(c, np.flatnonzero(~dark)), np.float64, mcica, **kw)
        equal_bits({k: v[..., ~dark] for k, v in on.items()}, alone, (name, kw.get("band_levels")))


@pytest.mark.parametrize("name", list(CASES))
def test_float32_boundary_is_the_fp64_call_rounded_once(gpu_ctx, plain, name):
    which, x32, x64, mcica, _, ref = plain[name]
    same_as_rounded(device_call(gpu_ctx, which, x32, np.float32, mcica), ref, name)
    extras = sw_extras(name) if which == "sw" else [dict(bands=LW_BAND_FLUXES, band_levels="all")] if name == "lw_a" else []
    for kw in extras:
        if not kw:
            continue
        want = device_call(gpu_ctx, which, x64, np.float64, mcica, **kw)
        assert len(want) == len(ref) + len(kw.get("components", ())) + len(kw["bands"])
        same_as_rounded(device_call(gpu_ctx, which, x32, np.float32, mcica, **kw), want, (name, kw["band_levels"]))
