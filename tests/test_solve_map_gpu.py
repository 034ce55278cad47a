"""The partial last block of a large solve chunk, on the GPU: the launch-order rule of the solve kernels (csrc/rrtmg_solve_map.h;
its arithmetic alone: tools/solve_map_check.cpp, tests/test_night_pack.py) as the kernels use it -- the list entry `first`, the
sched position `k`, the tile-list addressing and the launch sizing.

274 tiles (17 536 columns) x 12 layers, cloudy and cloud-free tiles alternating, 137 of each: 128 + 9 tiles for the shortwave's
16-wave workgroups, 17 x 8 + 1 for its 8-wave ones, 34 x 4 + 1 for the longwave's -- every solve kernel has one full block of its
launch order, one partial block and a partly filled last workgroup.  Each call is made twice (the chunk plan enlarges the chunks
only after a call that saw both kinds of tiles); the second must have run each solve variant in ONE launch, and its outputs must
be, bit for bit, those of the same columns computed in tile-aligned blocks of 64 tiles through a fresh context, where every
variant's tiles fit one block of the order."""
import numpy as np
import pytest

from climt_amd._lib import LW_OUT, LW_OUT_CLEAR, SW_OUT, SW_OUT_ALLSKY
from oracle.ref_driver import CONSTANTS, CPDAIR

pytestmark = pytest.mark.gpu

NTILE, NLAY, BLOCK_TILES = 274, 12, 64
NCOL = NTILE * 64
FLAGS = dict(iaer=0, dyofyr=1, scon=1367.0, isolvar=0, adjes=1.0, inflg=2, iceflg=1, liqflg=1, irng=0, permuteseed=684)
LEVELS = dict(SW_OUT + LW_OUT, dirdflx=1)


@pytest.fixture(scope="module")
def columns():
    """mcica -> the grid: McICA with kissvec and random overlap | no McICA, overcast layers, maximum-random overlap (icld 2)."""
    from climt_amd.synthetic import make_columns, overcast
    c = make_columns(NCOL, NLAY, cloudy=True, seed=274)
    c.pop("lat")
    free = (np.arange(NCOL) // 64) % 2 == 1
    for k in ("cldfr", "cliqwp", "cicewp"):
        c[k][:, free] = 0.0
    out = {}
    for mcica in (True, False):
        g = dict(c if mcica else overcast(c), icld=1 if mcica else 2, **FLAGS)
        cloudy = (g["cldfr"] > 0).any(axis=0).reshape(NTILE, 64).any(axis=1)
        assert np.array_equal(cloudy, np.arange(NTILE) % 2 == 0)      # 137 cloudy tiles, 137 cloud-free ones, alternating
        out[mcica] = g
    return out


def _context(which, clear_sky):
    from climt_amd._lib import Context
    ctx = Context(0)
    ctx.set_constants(**CONSTANTS)
    if which == "sw":
        ctx.sw_init(CPDAIR)
        ctx.set_sw_clear_sky(clear_sky)
    else:
        ctx.lw_init(CPDAIR)
        ctx.set_lw_clear_sky(clear_sky)
    return ctx


def _call(ctx, which, c, mcica, keys, direct):
    """One device-resident call into NaN-filled device buffers -> {name: downloaded array}."""
    from climt_amd import _hip
    nlay, ncol = c["play"].shape
    dev = {k: _hip.DeviceArray.from_host(v) for k, v in c.items() if isinstance(v, np.ndarray)}
    args = {k: v.ptr for k, v in dev.items()}
    args.update({k: v for k, v in c.items() if not isinstance(v, np.ndarray)}, ncol=ncol, nlay=nlay)
    dout = {k: _hip.DeviceArray.from_host(np.full((nlay + LEVELS[k], ncol), np.nan)) for k in keys + (("dirdflx",) if direct else ())}
    out = {k: dout[k].ptr for k in keys}
    if which == "sw":
        ctx.sw_fluxes(args, mcica=mcica, out=out, memspace=1, components={"dirdflx": dout["dirdflx"].ptr} if direct else None)
    else:
        ctx.lw_fluxes(args, mcica=mcica, out=out, memspace=1)
    ctx.synchronize()
    return {k: v.download() for k, v in dout.items()}


@pytest.mark.parametrize("mcica", [True, False], ids=["mcica_kissvec", "icld2"])
@pytest.mark.parametrize("which, clear_sky, direct", [("sw", True, False), ("sw", False, False), ("sw", True, True), ("lw", True, False), ("lw", False, False)],
                         ids=["sw", "sw_allsky_only", "sw_direct_component", "lw", "lw_allsky_only"])
def test_partial_last_block_of_a_large_chunk(columns, which, clear_sky, direct, mcica):
    from climt_amd.distributed import slice_columns
    c = columns[mcica]
    std = SW_OUT if which == "sw" else LW_OUT
    keys = tuple(k for k, _ in std if clear_sky or (k in SW_OUT_ALLSKY if which == "sw" else k not in LW_OUT_CLEAR))
    big = _context(which, clear_sky)
    try:
        _call(big, which, c, mcica, keys, direct)
        got = _call(big, which, c, mcica, keys, direct)
        launches = {cloudy: big.kernel_launches(which, cloudy=cloudy) for cloudy in (False, True)}
    finally:
        big.close()
    print("solve launches of the second call (cloud-free, cloudy):", launches)
    assert launches == {False: 1, True: 1}
    ref = _context(which, clear_sky)
    try:
        parts = [_call(ref, which, slice_columns(c, lo, min(lo + BLOCK_TILES * 64, NCOL)), mcica, keys, direct) for lo in range(0, NCOL, BLOCK_TILES * 64)]
    finally:
        ref.close()
    for k in got:
        want = np.concatenate([p[k] for p in parts], axis=1)
        assert np.isfinite(want).all(), k
        assert np.array_equal(got[k], want), (k, float(np.nanmax(np.abs(got[k] - want))))
    if clear_sky:      # the cloudy tiles are cloudy: the two sky streams differ
        up = "swuflx" if which == "sw" else "uflx"
        assert float(np.abs(got[up] - got[up + "c"]).max()) > 1.0
