#!/usr/bin/env python3
"""The simple boundary layer (rrtmg_hip_boundary_layer, climt_amd.SimpleBoundaryLayer): what the kernel costs, device resident
and from the host, beside the 1.69 ms device-resident radiation step it joins.

    timeout -k 10 600 python tools/boundary_layer_ab.py [--sizes 8192,131072] [--nlay 60] [--repeats 5] [--batch 20] [--statement-columns 128]

Two profiles per size, both in 'bulk' mode (flux_mode 1) with 251 columns of their own numbers, repeated: "deep" -- the heated case of
tests/boundary_layer_cases.py, a mixed layer of ~500 hPa, so the K-profile (log, pow, divisions) is formed at a third of the
interfaces -- and "no_top" (no Richardson number exceeds Ric: nothing diffuses, the three passes run all the same).  Per profile
and size:
  device   device pointers, deferred mode: `batch` calls enqueued back to back and ONE synchronise behind them (out of place;
           a single launch would measure the enqueue and the wake-up of the host), `repeats` times after a warm-up: median, min, max
  host     Context.boundary_layer on numpy arrays: nine arrays up, the kernel, four profiles and five diagnostics down, per call
Before timing, the device result of the first `statement-columns` columns is compared with the numpy statement on the scales of
boundary_layer_cases.deviations, and the largest is printed.  Fails where there is no GPU: no fall-back."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

STEP_MS = 1.69      # the device-resident SW + LW + Adams-Bashforth + slab step at 8192 x 60 (README), without this component
DIAG = ("stress_north", "stress_east", "height", "sh_out", "lh_out")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="8192,131072")
    ap.add_argument("--nlay", type=int, default=60)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--batch", type=int, default=20)
    ap.add_argument("--statement-columns", type=int, default=128)
    a = ap.parse_args()
    from climt_amd import _hip
    from climt_amd._lib import Context
    from climt_amd.build import source_hash
    import boundary_layer_cases as X
    ctx = Context(0)
    nlay, mode = a.nlay, 1
    print("boundary_layer_ab: source %s; %d repeats; device: %d calls per synchronise, deferred mode; flux mode 1; per call:" % (source_hash(), a.repeats, a.batch))
    worst = 0.0
    for ncol in [int(s) for s in a.sizes.split(",")]:
        for kind, name in (("deep", "heated"), ("no_top", "no_top")):
            base = X._inputs(name, nlay, min(ncol, 251))      # the case's 251 columns, repeated: its numbers are made for a few hundred
            c = {k: np.ascontiguousarray(np.tile(v, -(-ncol // v.shape[-1]))[..., :ncol]) for k, v in base.items()}
            ns = min(a.statement_columns, ncol)
            want = X.statement(*(c[k][..., :ns] for k in X.INPUTS[:9]), mode)
            assert want["margin"] >= X.MIN_MARGIN, want["margin"]
            want = dict({k: c[k][..., :ns] for k in X.INPUTS}, **want)
            dev = {k: _hip.DeviceArray.from_host(c[k]) for k in X.INPUTS[:9]}
            out = [_hip.DeviceArray((nlay, ncol)) for _ in range(4)]
            diag = {n: _hip.DeviceArray((ncol,)) for n in DIAG}
            args = [c[k] for k in X.INPUTS[:9]] + [X.DT, X.CONSTANTS, mode]

            def device():
                ctx.boundary_layer(*(dev[k] for k in X.INPUTS[:9]), X.DT, X.CONSTANTS, mode, t_out=out[0], q_out=out[1], u_out=out[2], v_out=out[3],
                                   diagnostics=diag, memspace=1, ncol=ncol, nlay=nlay)

            def host():
                return ctx.boundary_layer(*args)

            # ---- the results at the timed size, before any timing ----------------------------------------------------------------
            device()
            ctx.synchronize()
            got = dict(zip(X.PROFILES, (o.download() for o in out)))
            got.update({k: diag[n].download() for k, n in zip(X.DIAGNOSTICS, DIAG)})
            err = max(X.deviations({k: v[..., :ns] for k, v in got.items()}, want).values())
            assert err <= X.TOL, err
            worst = max(worst, err)
            h = host()
            assert all(X.same_bits(x, got[k]) for x, k in zip(h[:4], X.PROFILES)), "host and device pointers differ"
            assert all(X.same_bits(h[4][n], got[k]) for k, n in zip(X.DIAGNOSTICS, DIAG)), "host and device pointers differ"

            # ---- timing -------------------------------------------------------------------------------------------------------------
            def timed(fn, batch):
                ctx.synchronize()
                t0 = time.perf_counter()
                for _ in range(batch):
                    fn()
                ctx.synchronize()
                return (time.perf_counter() - t0) * 1e3 / batch
            ctx.set_deferred(True)
            timed(device, a.batch)
            td = [timed(device, a.batch) for _ in range(a.repeats)]
            ctx.set_deferred(False)
            timed(host, 1)
            th = [timed(host, 1) for _ in range(a.repeats)]
            md = float(np.median(td))
            print("  %7d x %d %-7s (top at interface %d..%d, height %.0f..%.0f m; within %.1e of the statement on %d columns)" % (
                ncol, nlay, kind, int(want["count"].min()), int(want["count"].max()), float(got["height"].min()), float(got["height"].max()), err, ns))
            print("      device  median %8.4f ms   min %8.4f ms   max %8.4f ms" % (md, min(td), max(td)))
            print("      host    median %8.4f ms   min %8.4f ms   max %8.4f ms" % (float(np.median(th)), min(th), max(th)))
            if ncol == 8192:
                print("      beside the %.2f ms device-resident step without the component: %.1f %%" % (STEP_MS, 100.0 * md / STEP_MS))
    print("  largest deviation / scale from the statement over all sides: %.3e" % worst)
    ctx.close()


if __name__ == "__main__":
    main()
