"""Cost and gain of the shortwave's day-column pack (rrtmg_hip_set_sw_night_pack): the same library, three arms interleaved --
skip off, skip on (the night-column skip alone) and pack on.  Per row: the device-event time of one device-resident shortwave
call, the shortwave solve kernels' own event brackets summed over the call's chunks (rrtmg_hip_kernel_ms), and the time of the
SW + LW step in deferred mode (the two spectra on two streams; host clock from the first enqueue to the end of synchronize()),
each the median of the alternations behind two warm-up rounds; the raw lists are kept.  t: the share of night tiles the skip
finds; p: the share of the tiles' solve work the pack does not do (night.packed_counts).  The all-day row has nothing to skip:
pack against skip there is the cost of the map, the gathers and the scatter.  Writes the table to stdout
(profiles/night_pack_ab.txt is its output).

    python tools/night_pack_ab.py [--alternations 6] [--rows small128clear,small128mcica,global512,allday]
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
from tools.night_skip_ab import BASE, equinox_terminator  # noqa: E402

# name -> (longitudes, latitudes, layers, McICA, terminator field?)
ROWS = {
    "small128clear": (128, 64, 60, False, True),     # the headline grid: two tiles per latitude row, all mixed
    "small128mcica": (128, 64, 60, True, True),
    "global512": (512, 256, 60, True, True),
    "allday": (8192, 1, 60, False, False),           # nothing to skip: the cost of packing
}
ARMS = ("off", "skip", "pack")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--alternations", type=int, default=6)
    ap.add_argument("--rows", default=",".join(ROWS))
    args = ap.parse_args()
    ctx = Context(0)
    ctx.set_constants(**CONSTANTS)
    ctx.sw_init(CPDAIR)
    ctx.lw_init(CPDAIR)
    print("# day-column pack: skip off / skip on / pack on, %d alternations behind 2 warm-up rounds, medians (ms); sw: HIP events around one"
          " device-resident call; solve: the shortwave solve kernels' event brackets of that call, summed; step: SW + LW deferred on two"
          " streams, host clock to the end of synchronize() (includes the enqueue); t: share of night tiles (skip); p: share of the tiles'"
          " solve work not done (pack); library src:%s" % (args.alternations, source_hash()))
    print("# %-30s %6s %6s | %8s %8s %8s %9s | %8s %8s %8s %9s | %8s %8s %8s %9s" % (
        "row", "t", "p", "sw off", "sw skip", "sw pack", "pack/skip", "slv off", "slv skip", "slv pack", "pack/skip",
        "step off", "step skp", "step pck", "pack/skip"))
    for name in args.rows.split(","):
        nlon, nlat, nlay, mcica, field = ROWS[name]
        n = nlon * nlat
        c = make_columns(n, nlay, cloudy=mcica, seed=9)
        c.pop("lat")
        c.update(BASE)
        c["icld"] = 2 if mcica else 0
        if field:
            c["coszen"] = equinox_terminator(nlon, nlat)
        ntile = (n + 63) // 64
        want = {"off": (0, 0), "skip": night.night_counts(c["coszen"]), "pack": night.packed_counts(c["coszen"])}
        dev = {k: _hip.DeviceArray.from_host(v) for k, v in c.items() if isinstance(v, np.ndarray)}
        inp = {k: v.ptr for k, v in dev.items()}
        inp.update({k: v for k, v in c.items() if not isinstance(v, np.ndarray)})
        inp.update(ncol=n, nlay=nlay)
        lwinp = dict(inp, icld=1 if mcica else 0)
        so = {k: _hip.DeviceArray((nlay + lev, n)) for k, lev in SW_OUT}
        lo = {k: _hip.DeviceArray((nlay + lev, n)) for k, lev in LW_OUT}
        sptr, lptr = {k: v.ptr for k, v in so.items()}, {k: v.ptr for k, v in lo.items()}
        e0, e1 = _hip.Event(), _hip.Event()
        t = {(k, arm): [] for k in ("sw", "solve", "step") for arm in ARMS}

        def switch(arm):
            ctx.set_sw_night_skip(arm == "skip")
            ctx.set_sw_night_pack(arm == "pack")

        def sw_call(arm, keep):
            switch(arm)
            e0.record(ctx.stream)
            ctx.sw_fluxes(inp, mcica=mcica, out=sptr, memspace=1)
            e1.record(ctx.stream)
            e1.synchronize()
            assert ctx.sw_night_last() == want[arm], (arm, ctx.sw_night_last(), want[arm])
            if keep:
                t[("sw", arm)].append(e0.elapsed_ms(e1))
                t[("solve", arm)].append(sum(ctx.kernel_ms("sw", cloudy=cl) for cl in (False, True) if ctx.kernel_launches("sw", cloudy=cl) > 0))

        def step(arm, keep):
            switch(arm)
            ctx.set_deferred(True)
            try:
                ctx.synchronize()
                t0 = time.perf_counter()
                ctx.sw_fluxes(inp, mcica=mcica, out=sptr, memspace=1)
                ctx.lw_fluxes(lwinp, mcica=mcica, out=lptr, memspace=1)
                ctx.synchronize()
                if keep:
                    t[("step", arm)].append((time.perf_counter() - t0) * 1.0e3)
            finally:
                ctx.set_deferred(False)
        for r in range(2 + args.alternations):      # two warm-up rounds: buffers, code objects, chunk plans
            for arm in ARMS:
                sw_call(arm, r >= 2)
            for arm in ARMS:
                step(arm, r >= 2)
        switch("off")
        m = {k: float(np.median(v)) for k, v in t.items()}
        print("  %-30s %6.3f %6.3f | %8.3f %8.3f %8.3f %9.3f | %8.3f %8.3f %8.3f %9.3f | %8.3f %8.3f %8.3f %9.3f   (%s)" % (
            "%s %dx%dx%d %s" % (name, nlon, nlat, nlay, "McICA" if mcica else "clear"), want["skip"][0] / ntile, want["pack"][0] / ntile,
            m[("sw", "off")], m[("sw", "skip")], m[("sw", "pack")], m[("sw", "pack")] / m[("sw", "skip")],
            m[("solve", "off")], m[("solve", "skip")], m[("solve", "pack")], m[("solve", "pack")] / m[("solve", "skip")],
            m[("step", "off")], m[("step", "skip")], m[("step", "pack")], m[("step", "pack")] / m[("step", "skip")],
            " | ".join("%s %s " % k + " ".join("%.3f" % x for x in v) for k, v in t.items())))
        sys.stdout.flush()
        for v in list(dev.values()) + list(so.values()) + list(lo.values()):
            v.free()
    ctx.close()


if __name__ == "__main__":
    main()
