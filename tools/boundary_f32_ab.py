"""What the float32 boundary costs and gains: (a) the fp64 call -- the parent's path -- against (b) the same call through
rrtmg_hip_*_fluxes_f32 (precision="float32"), on ONE library and the same state, interleaved.  Two warm-up rounds, then
--alternations rounds of (a), (b); medians, with the raw lists beside them.  Every row runs in a child process of its own under
its own time limit; a row that fails or runs out of time ends the run.

Rows: host-pointer calls at 128 x 64 x 60, clear sky and McICA (kissvec), caller-owned pageable arrays, by the host clock --
Context.sw_fluxes, Context.lw_fluxes and Context.radiation_fluxes; device-resident calls at 8192 x 60, by HIP events on the
context's stream -- Context.sw_fluxes and Context.lw_fluxes with memspace=1.  (a) holds float64 arrays, (b) the same values
rounded to float32.  Writes the table to stdout (profiles/boundary_f32_ab.txt is its output).

    python tools/boundary_f32_ab.py [--alternations 6] [--rows host_sw_clear,...] [--limit 240]
"""
import argparse
import os
import subprocess
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

# name -> (pointers, call, columns, layers, McICA)
ROWS = {
    "host_sw_clear": ("host", "sw", 128 * 64, 60, False), "host_sw_mcica": ("host", "sw", 128 * 64, 60, True),
    "host_lw_clear": ("host", "lw", 128 * 64, 60, False), "host_lw_mcica": ("host", "lw", 128 * 64, 60, True),
    "host_joint_clear": ("host", "joint", 128 * 64, 60, False), "host_joint_mcica": ("host", "joint", 128 * 64, 60, True),
    "device_sw": ("device", "sw", 8192, 60, True), "device_lw": ("device", "lw", 8192, 60, True),
}


def run_row(name, alternations):
    from climt_amd._hip import DeviceArray, Event
    from climt_amd._lib import LW_OUT, SW_OUT
    from climt_amd.rrtmg.common import make_context
    from climt_amd.synthetic import make_columns
    pointers, call, ncol, nlay, mcica = ROWS[name]
    ctx = make_context(0)
    ctx.sw_init(1004.64); ctx.lw_init(1004.64)
    c = make_columns(ncol, nlay, cloudy=mcica, seed=9)
    c.pop("lat")
    c.update(icld=2 if mcica else 0, iaer=0, adjes=1.0, dyofyr=1, scon=1367.0, isolvar=0, inflg=2, iceflg=1, liqflg=1, irng=0, permuteseed=5)
    arms = {}
    for arm, dt in (("a", np.float64), ("b", np.float32)):
        x = {k: (np.ascontiguousarray(v, dtype=dt) if isinstance(v, np.ndarray) else v) for k, v in c.items()}
        so = {k: np.zeros((nlay + lev, ncol), dt) for k, lev in SW_OUT}
        lo = {k: np.zeros((nlay + lev, ncol), dt) for k, lev in LW_OUT}
        kw = dict(mcica=mcica, precision=np.dtype(dt).name)
        if pointers == "device":
            hold = [DeviceArray.from_host(v) for v in x.values() if isinstance(v, np.ndarray)]
            names = [k for k, v in x.items() if isinstance(v, np.ndarray)]
            x = dict(x, nlay=nlay, ncol=ncol, **{k: d.ptr for k, d in zip(names, hold)})
            outs = {k: DeviceArray(v.shape, dt) for k, v in (so if call == "sw" else lo).items()}
            out = {k: d.ptr for k, d in outs.items()}
            fn = (lambda x=x, out=out, kw=kw: ctx.sw_fluxes(x, out=out, memspace=1, **kw)) if call == "sw" else \
                 (lambda x=x, out=out, kw=kw: ctx.lw_fluxes(x, out=out, memspace=1, **kw))
            arms[arm] = (fn, hold, outs)
        elif call == "joint":
            arms[arm] = (lambda x=x, so=so, lo=lo, kw=kw: ctx.radiation_fluxes(sw=dict(inp=x, out=so, mcica=mcica), lw=dict(inp=x, out=lo, mcica=mcica), precision=kw["precision"]),)
        elif call == "sw":
            arms[arm] = (lambda x=x, so=so, kw=kw: ctx.sw_fluxes(x, out=so, **kw),)
        else:
            arms[arm] = (lambda x=x, lo=lo, kw=kw: ctx.lw_fluxes(x, out=lo, **kw),)
    t = {"a": [], "b": []}
    e0, e1 = Event(), Event()
    for r in range(2 + alternations):
        for arm in ("a", "b"):
            fn = arms[arm][0]
            if pointers == "device":
                e0.record(ctx.stream); fn(); e1.record(ctx.stream); e1.synchronize()
                dt_ms = e0.elapsed_ms(e1)
            else:
                t0 = time.perf_counter(); fn(); dt_ms = (time.perf_counter() - t0) * 1.0e3
            if r >= 2:
                t[arm].append(dt_ms)
    a, b = float(np.median(t["a"])), float(np.median(t["b"]))
    extra = ""
    if call == "joint":
        shared, up = ctx.radiation_last()[:2]
        extra = "  (b) radiation_last: %d shared, %.1f MB up" % (shared, up / 1.0e6)
    print("  %-34s %9.3f %9.3f %7.3f   (%s)%s" % ("%s %dx%d %s, %s" % (name, ncol, nlay, "McICA" if mcica else "clear", "HIP events" if pointers == "device" else "host clock"),
                                                a, b, b / a, " | ".join("%s " % k + " ".join("%.3f" % v for v in vals) for k, vals in t.items()), extra))
    sys.stdout.flush()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--alternations", type=int, default=6)
    ap.add_argument("--rows", default=",".join(ROWS))
    ap.add_argument("--limit", type=int, default=240, help="seconds per row")
    ap.add_argument("--row", help="(internal) run this one row in this process")
    args = ap.parse_args()
    if args.row:
        return run_row(args.row, args.alternations)
    from climt_amd._lib import source_hash
    print("# float32 boundary: (a) fp64 call against (b) the same call with precision=\"float32\", 2 warm-up rounds + %d alternations, medians (ms);"
          " library src:%s" % (args.alternations, source_hash()))
    print("# %-34s %9s %9s %7s" % ("row", "(a) fp64", "(b) f32", "b/a"))
    sys.stdout.flush()
    for name in args.rows.split(","):
        if name not in ROWS:
            raise SystemExit("unknown row %r (one of %s)" % (name, ", ".join(ROWS)))
        try:      # a fresh child per row, under its own time limit; trouble ends the run
            rc = subprocess.run([sys.executable, os.path.abspath(__file__), "--row", name, "--alternations", str(args.alternations)], timeout=args.limit).returncode
        except subprocess.TimeoutExpired:
            raise SystemExit("row %s did not finish within %d s: stopping" % (name, args.limit))
        if rc:
            raise SystemExit("row %s failed (exit status %d): stopping" % (name, rc))


if __name__ == "__main__":
    main()
