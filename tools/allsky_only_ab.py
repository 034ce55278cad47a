"""Gain of the shortwave call without the clear-sky outputs (rrtmg_hip_set_sw_clear_sky): the same library, setting 1 (the
default path) against setting 0, interleaved.  Per row: the device-event time of one shortwave call, the shortwave solve
kernels' own event brackets summed over the call's chunks (rrtmg_hip_kernel_ms), and the SW + LW step in deferred mode (two
streams; host clock from the first enqueue to the end of synchronize()), each the median of the alternations after two
warm-up rounds, with the raw lists behind.  The host-pointer row times the whole call on the host clock instead (uploads,
solve, three or six downloads) and has no step.  Writes the table to stdout (profiles/allsky_only_ab.txt is its output).

    python tools/allsky_only_ab.py [--alternations 6] [--rows mcica,mixed,shard,clear,host]
"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from climt_amd import _hip  # noqa: E402
from climt_amd._lib import LIB_PATH, LW_OUT, SW_OUT, SW_OUT_ALLSKY, Context, source_hash  # noqa: E402
from climt_amd.synthetic import make_columns  # noqa: E402
from oracle.ref_driver import CONSTANTS, CPDAIR  # noqa: E402

BASE = dict(icld=1, iaer=0, adjes=1.0, dyofyr=1, scon=1367.0, isolvar=0, inflg=2, iceflg=1, liqflg=1, irng=0, permuteseed=5)
# name -> (columns, layers, McICA, every fourth tile cloud-free, shard of, host pointers)
ROWS = {
    "mcica": (8192, 60, True, False, 0, False),
    "mixed": (8192, 60, True, True, 0, False),
    "shard": (16384, 60, True, False, 131072, False),      # BASELINE config 4: one of eight shards of 512 x 256
    "clear": (8192, 60, False, False, 0, False),           # the integration kernel and the absent outputs only
    "host": (128 * 64, 60, True, False, 0, True),          # the host-pointer call at 128 x 64 x 60
}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--alternations", type=int, default=6)
    ap.add_argument("--rows", default=",".join(ROWS))
    args = ap.parse_args()
    ctx = Context(0)
    ctx.set_constants(**CONSTANTS)
    ctx.sw_init(CPDAIR)
    ctx.lw_init(CPDAIR)
    print("# shortwave clear-sky outputs, setting 1 against 0, %d alternations after 2 warm-up rounds, medians (ms); sw: HIP events around one"
          " device-resident call (host row: host clock around the host-pointer call); solve: the shortwave solve kernels' event brackets of"
          " that call, summed; step: SW + LW deferred on two streams, host clock to the end of synchronize(); library %s src:%s"
          % (args.alternations, os.path.basename(LIB_PATH), source_hash()))
    print("# %-28s %9s %9s %7s %9s %9s %7s %9s %9s %7s" % ("row", "sw 1", "sw 0", "0/1", "solve 1", "solve 0", "0/1", "step 1", "step 0", "0/1"))
    for name in args.rows.split(","):
        n, nlay, mcica, mixed, shard_of, host = ROWS[name]
        c = make_columns(n, nlay, cloudy=mcica, seed=9)
        c.pop("lat")
        c.update(BASE)
        c["icld"] = 2 if mcica else 0
        if mixed:
            for t in range(0, n // 64, 4):
                for k in ("cldfr", "cliqwp", "cicewp"):
                    c[k][:, t * 64:(t + 1) * 64] = 0.0
        if shard_of:
            c.update(shard_col0=0, shard_ncol=shard_of)
        keep = []
        if host:
            inp, lwinp = c, None
            sout = {k: np.zeros((nlay + lev, n)) for k, lev in SW_OUT}
        else:
            dev = {k: _hip.DeviceArray.from_host(v) for k, v in c.items() if isinstance(v, np.ndarray)}
            inp = {k: v.ptr for k, v in dev.items()}
            inp.update({k: v for k, v in c.items() if not isinstance(v, np.ndarray)})
            inp.update(ncol=n, nlay=nlay)
            lwinp = dict(inp, icld=1 if mcica else 0)
            so = {k: _hip.DeviceArray((nlay + lev, n)) for k, lev in SW_OUT}
            lo = {k: _hip.DeviceArray((nlay + lev, n)) for k, lev in LW_OUT}
            keep = list(dev.values()) + list(so.values()) + list(lo.values())
            sout, lptr = {k: v.ptr for k, v in so.items()}, {k: v.ptr for k, v in lo.items()}
        e0, e1 = _hip.Event(), _hip.Event()
        solve = {True: [], False: []}

        def sw_out(on):
            return sout if on else {k: sout[k] for k in SW_OUT_ALLSKY}

        def sw_call(on):
            ctx.set_sw_clear_sky(on)
            if host:
                t0 = time.perf_counter()
                ctx.sw_fluxes(inp, mcica=mcica, out=sw_out(on))
                ms = (time.perf_counter() - t0) * 1.0e3
            else:
                e0.record(ctx.stream)
                ctx.sw_fluxes(inp, mcica=mcica, out=sw_out(on), memspace=1)
                e1.record(ctx.stream)
                e1.synchronize()
                ms = e0.elapsed_ms(e1)
            solve[on].append(sum(ctx.kernel_ms("sw", cloudy=cl) for cl in (False, True) if ctx.kernel_launches("sw", cloudy=cl) > 0))
            return ms

        def step(on):
            ctx.set_sw_clear_sky(on)
            ctx.set_deferred(True)
            try:
                ctx.synchronize()
                t0 = time.perf_counter()
                ctx.sw_fluxes(inp, mcica=mcica, out=sw_out(on), memspace=1)
                ctx.lw_fluxes(lwinp, mcica=mcica, out=lptr, memspace=1)
                ctx.synchronize()
                return (time.perf_counter() - t0) * 1.0e3
            finally:
                ctx.set_deferred(False)
        t = {(k, on): [] for k in ("sw", "step") for on in (True, False)}
        for on in (True, False, True, False):      # warm-up: buffers, code objects, chunk plans
            sw_call(on)
            if not host:
                step(on)
        solve[True], solve[False] = [], []
        for _ in range(args.alternations):
            for on in (True, False):
                t[("sw", on)].append(sw_call(on))
            if not host:
                for on in (True, False):
                    t[("step", on)].append(step(on))
        ctx.set_sw_clear_sky(True)
        med = lambda v: float(np.median(v)) if v else float("nan")
        m = {k: med(v) for k, v in t.items()}
        s1, s0 = med(solve[True]), med(solve[False])
        raw = dict(t)
        raw.update({("solve", on): v for on, v in solve.items()})
        print("  %-28s %9.3f %9.3f %7.3f %9.3f %9.3f %7.3f %9.3f %9.3f %7.3f   (%s)" % (
            "%s %dx%d %s%s" % (name, n, nlay, "McICA" if mcica else "clear", " host pointers" if host else ""),
            m[("sw", True)], m[("sw", False)], m[("sw", False)] / m[("sw", True)], s1, s0, s0 / s1,
            m[("step", True)], m[("step", False)], m[("step", False)] / m[("step", True)],
            " | ".join("%s %d " % (k, on) + " ".join("%.3f" % x for x in v) for (k, on), v in raw.items() if v)))
        sys.stdout.flush()
        for v in keep:
            v.free()
    ctx.close()


if __name__ == "__main__":
    main()
