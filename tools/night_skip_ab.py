"""Cost and gain of the shortwave's night-column skip (rrtmg_hip_set_sw_night_skip): the same library, option off against
option on, interleaved.  Per row: the device-event time of one device-resident shortwave call, and the time of the SW + LW
step in deferred mode (the two spectra on two streams; host clock from the first enqueue to the end of synchronize()), each
the median of the alternations; beside the on / off ratios the share t of night tiles -- a solve time linear in t would give
1 - t for the solve kernels alone.  Beside them, for reading the step: the shortwave solve kernels' own event brackets summed
over the call's chunks (rrtmg_hip_kernel_ms: what the launches took, however few of a launch's workgroups had work) and the
longwave call alone.  --chunk-tiles N: a diagnostic run with the solve chunks fixed at N tiles (RRTMG_HIP_CHUNK_TILES) instead
of the library's plan.  Writes the table to stdout (profiles/night_skip_ab.txt is its output).

    python tools/night_skip_ab.py [--alternations 6] [--rows global512,global1440,small128,allday] [--chunk-tiles N]
"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from climt_amd import _hip, night  # noqa: E402
from climt_amd._lib import LW_OUT, SW_OUT, Context, source_hash  # noqa: E402
from climt_amd.synthetic import make_columns  # noqa: E402
from oracle.ref_driver import CONSTANTS, CPDAIR  # noqa: E402

BASE = dict(icld=1, iaer=0, adjes=1.0, dyofyr=1, scon=1367.0, isolvar=0, inflg=2, iceflg=1, liqflg=1, irng=0, permuteseed=5)
# name -> (longitudes, latitudes, layers, McICA, terminator field?)
ROWS = {
    "global512": (512, 256, 60, True, True),       # BASELINE config 4 whole
    "global1440": (1440, 90, 100, True, True),
    "small128": (128, 64, 60, False, True),        # two tiles per latitude row: the unfavourable case
    "allday": (8192, 1, 60, False, False),         # nothing to skip: the cost of the option
}


def equinox_terminator(nlon, nlat):
    """coszen [nlat * nlon], longitude fastest: cos(lat) cos(lon - lon0) on a regular grid at equinox, the sun a third of a
    tile off the first longitude."""
    lon = 2.0 * np.pi * (np.arange(nlon) + 0.5) / nlon
    lat = np.deg2rad(-90.0 + 180.0 * (np.arange(nlat) + 0.5) / nlat)
    return np.ascontiguousarray((np.cos(lat)[:, None] * np.cos(lon - 2.0 * np.pi * 20.3 / nlon)[None, :]).ravel())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--alternations", type=int, default=6)
    ap.add_argument("--rows", default=",".join(ROWS))
    ap.add_argument("--chunk-tiles", type=int, default=0)
    args = ap.parse_args()
    if args.chunk_tiles:
        os.environ["RRTMG_HIP_CHUNK_TILES"] = str(args.chunk_tiles)      # read when the context is created
    ctx = Context(0)
    ctx.set_constants(**CONSTANTS)
    ctx.sw_init(CPDAIR)
    ctx.lw_init(CPDAIR)
    print("# night-column skip, off against on, %d alternations, medians (ms); sw: HIP events around one device-resident call; step: SW + LW"
          " deferred on two streams, host clock to the end of synchronize() (includes the enqueue); solve: the shortwave solve kernels' event"
          " brackets of that call, summed; lw: the longwave call alone; chunks: %s; library src:%s"
          % (args.alternations, "%d tiles (RRTMG_HIP_CHUNK_TILES)" % args.chunk_tiles if args.chunk_tiles else "the library's plan", source_hash()))
    print("# %-30s %7s %7s %9s %9s %7s %9s %9s %7s %9s %9s %7s %9s" % ("row", "t", "1-t", "sw off", "sw on", "on/off", "step off", "step on", "on/off",
                                                                        "solve off", "solve on", "on/off", "lw"))
    for name in args.rows.split(","):
        nlon, nlat, nlay, mcica, field = ROWS[name]
        n = nlon * nlat
        c = make_columns(n, nlay, cloudy=mcica, seed=9)
        c.pop("lat")
        c.update(BASE)
        c["icld"] = 2 if mcica else 0
        if field:
            c["coszen"] = equinox_terminator(nlon, nlat)
        tiles = night.night_tiles(c["coszen"])
        share = float(tiles.sum()) / tiles.size
        want = night.night_counts(c["coszen"])
        dev = {k: _hip.DeviceArray.from_host(v) for k, v in c.items() if isinstance(v, np.ndarray)}
        inp = {k: v.ptr for k, v in dev.items()}
        inp.update({k: v for k, v in c.items() if not isinstance(v, np.ndarray)})
        inp.update(ncol=n, nlay=nlay)
        lwinp = dict(inp, icld=1 if mcica else 0)
        so = {k: _hip.DeviceArray((nlay + lev, n)) for k, lev in SW_OUT}
        lo = {k: _hip.DeviceArray((nlay + lev, n)) for k, lev in LW_OUT}
        sptr, lptr = {k: v.ptr for k, v in so.items()}, {k: v.ptr for k, v in lo.items()}
        e0, e1 = _hip.Event(), _hip.Event()

        def sw_call(on):
            ctx.set_sw_night_skip(on)
            e0.record(ctx.stream)
            ctx.sw_fluxes(inp, mcica=mcica, out=sptr, memspace=1)
            e1.record(ctx.stream)
            e1.synchronize()
            solve[on].append(sum(ctx.kernel_ms("sw", cloudy=cl) for cl in (False, True) if ctx.kernel_launches("sw", cloudy=cl) > 0))
            return e0.elapsed_ms(e1)

        def lw_call():
            e0.record(ctx.stream)
            ctx.lw_fluxes(lwinp, mcica=mcica, out=lptr, memspace=1)
            e1.record(ctx.stream)
            e1.synchronize()
            return e0.elapsed_ms(e1)

        def step(on):
            ctx.set_sw_night_skip(on)
            ctx.set_deferred(True)
            try:
                ctx.synchronize()
                t0 = time.perf_counter()
                ctx.sw_fluxes(inp, mcica=mcica, out=sptr, memspace=1)
                ctx.lw_fluxes(lwinp, mcica=mcica, out=lptr, memspace=1)
                ctx.synchronize()
                return (time.perf_counter() - t0) * 1.0e3
            finally:
                ctx.set_deferred(False)
        t = {(k, on): [] for k in ("sw", "step") for on in (False, True)}
        solve, lw = {False: [], True: []}, []
        for on in (False, True, False, True):      # warm-up: buffers, code objects, chunk plans
            sw_call(on)
            step(on)
        assert ctx.sw_night_last() == want, (ctx.sw_night_last(), want)
        solve = {False: [], True: []}
        for _ in range(args.alternations):
            for on in (False, True):
                t[("sw", on)].append(sw_call(on))
            lw.append(lw_call())
            for on in (False, True):
                t[("step", on)].append(step(on))
        ctx.set_sw_night_skip(False)
        m = {k: float(np.median(v)) for k, v in t.items()}
        so_, sn_ = float(np.median(solve[False])), float(np.median(solve[True]))
        print("  %-30s %7.3f %7.3f %9.3f %9.3f %7.3f %9.3f %9.3f %7.3f %9.3f %9.3f %7.3f %9.3f   (%s)" % (
            "%s %dx%dx%d %s" % (name, nlon, nlat, nlay, "McICA" if mcica else "clear"), share, 1.0 - share,
            m[("sw", False)], m[("sw", True)], m[("sw", True)] / m[("sw", False)],
            m[("step", False)], m[("step", True)], m[("step", True)] / m[("step", False)], so_, sn_, sn_ / so_, float(np.median(lw)),
            " | ".join("%s %s " % (k, "on" if on else "off") + " ".join("%.3f" % x for x in v) for (k, on), v in t.items())))
        sys.stdout.flush()
        for v in list(dev.values()) + list(so.values()) + list(lo.values()):
            v.free()
    ctx.close()


if __name__ == "__main__":
    main()
