#!/usr/bin/env python3
"""The dry convective adjustment (rrtmg_hip_dry_adjustment, climt_amd.DryConvectiveAdjustment): what the kernel costs, device
resident and from the host, beside the numpy statement on the CPU and beside the 1.69 ms device-resident radiation step.

    timeout -k 10 600 python tools/dry_adjust_ab.py [--sizes 8192,131072] [--nlay 60] [--repeats 5] [--batch 20] [--statement-columns 128]

Two profiles per size: "unstable" -- potential temperature falling with height through the lowest third of the column, stable
above, so every column mixes a run of nlay / 3 layers from the surface -- and "stable" (isothermal 290 K: the scan of every k and
no mixing).  Every column has its own numbers.  Per profile and size:
  device   device pointers, deferred mode: `batch` calls enqueued back to back and ONE synchronise behind them (out of place;
           a single launch would measure the enqueue and the wake-up of the host), `repeats` times after a warm-up: median, min, max
  host     Context.dry_adjustment on numpy arrays: four arrays up, the kernel, two arrays and mixed_top down, per call
  numpy    tests/dry_adjust_cases.statement on the first `statement-columns` columns, scaled to the size (a plain Python loop:
           the reference's numpy path without a JIT is of this kind)
Before timing, the device result of the first `statement-columns` columns is compared with the statement: mixed_top exactly, and
the largest relative deviation of T is printed.  Fails where there is no GPU: no fall-back."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

STEP_MS = 1.69      # the device-resident SW + LW + Adams-Bashforth + slab step at 8192 x 60 (README)


def profile(kind, nlay, ncol):
    import dry_adjust_cases as X
    p, p_int = X.pressures(nlay, ncol)
    if kind == "stable":
        return np.full((nlay, ncol), 290.0), np.zeros((nlay, ncol)), p, p_int
    lev = np.arange(nlay)[:, None] * np.ones((1, ncol))
    amp = 1.0 + 0.5 * (np.arange(ncol)[None, :] % 251) / 251.0
    third = nlay // 3
    theta = np.where(lev < third, 310.0 - 0.4 * amp * lev, 310.0 + 3.0 * (lev - third + 1))
    q = 0.015 * (p / p_int[0]) ** 3
    return theta * (p / X.CONSTANTS["pref"]) ** (X.CONSTANTS["rd"] / X.CONSTANTS["cpd"]), q, p, p_int


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
    import dry_adjust_cases as X
    ctx = Context(0)
    nlay = a.nlay
    print("dry_adjust_ab: source %s; %d repeats; device: %d calls per synchronise, deferred mode; per call:" % (source_hash(), a.repeats, a.batch))
    worst = 0.0
    for ncol in [int(s) for s in a.sizes.split(",")]:
        for kind in ("unstable", "stable"):
            t, q, p, p_int = profile(kind, nlay, ncol)
            ns = min(a.statement_columns, ncol)
            t0 = time.perf_counter()
            want_t, want_q, margin, want_top = X.statement(t[:, :ns], q[:, :ns], p[:, :ns], p_int[:, :ns])
            numpy_ms = (time.perf_counter() - t0) * 1e3 * ncol / ns
            assert margin >= X.MIN_MARGIN, margin
            dev = {k: _hip.DeviceArray.from_host(np.ascontiguousarray(v)) for k, v in (("t", t), ("q", q), ("p", p), ("p_int", p_int))}
            t_out, q_out, top = _hip.DeviceArray((nlay, ncol)), _hip.DeviceArray((nlay, ncol)), _hip.DeviceArray((ncol,), np.int32)

            def device():
                ctx.dry_adjustment(dev["t"], dev["q"], dev["p"], dev["p_int"], X.CONSTANTS, t_out=t_out, q_out=q_out, mixed_top=top, memspace=1, ncol=ncol, nlay=nlay)

            def host():
                return ctx.dry_adjustment(t, q, p, p_int, X.CONSTANTS)

            # ---- the results at the timed size, before any timing ----------------------------------------------------------------
            device()
            ctx.synchronize()
            got_t, got_q, got_top = t_out.download(), q_out.download(), top.download()
            assert (got_top[:ns] == want_top).all(), "mixed_top differs from the numpy statement"
            err = X.rel_err(got_t[:, :ns], want_t)
            assert err <= X.TOL and float(np.abs(got_q[:, :ns] - want_q).max()) <= X.TOL * max(float(want_q.max()), 1e-300), err
            worst = max(worst, err)
            ht, hq, htop = host()
            assert X.same_bits(ht, got_t) and X.same_bits(hq, got_q) and (htop == got_top).all(), "host and device pointers differ"
            mixed = int((got_top >= 0).sum())

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
            print("  %7d x %d %-8s (%d columns mix, top layer %d; T within %.1e of the statement on %d columns)" % (ncol, nlay, kind, mixed, int(got_top.max()), err, ns))
            print("      device  median %8.4f ms   min %8.4f ms   max %8.4f ms" % (md, min(td), max(td)))
            print("      host    median %8.4f ms   min %8.4f ms   max %8.4f ms" % (float(np.median(th)), min(th), max(th)))
            print("      numpy   %10.1f ms (statement, %d columns scaled)   = %.0f x the device call" % (numpy_ms, ns, numpy_ms / md))
            if ncol == 8192:
                print("      share of the %.2f ms device-resident step: %.1f %%" % (STEP_MS, 100.0 * md / STEP_MS))
    print("  largest relative deviation of T from the statement over all sides: %.3e" % worst)
    ctx.close()


if __name__ == "__main__":
    main()
