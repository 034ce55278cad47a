#!/usr/bin/env python3
"""The simple physics package (rrtmg_hip_simple_physics, climt_amd.SimplePhysics): what the kernel costs, device resident.

    timeout -k 10 600 python tools/simple_physics_ab.py [--ncol 8192] [--nlays 30,60] [--repeats 5] [--batch 20] [--statement-columns 128]

Two profiles per shape, both with all three processes on: "dry_calm" (nothing saturated, no wind: every branch of the
condensation is the cheap one and the diffusivities are zero, the three passes run all the same) and "raining_wind" (the varied
case of tests/simple_physics_cases.py: supersaturated layers, winds on both sides of 20 m/s), 130 columns of their own numbers,
repeated.  Per profile and shape: device pointers, deferred mode, `batch` calls enqueued back to back and ONE synchronise behind
them (out of place; a single launch would measure the enqueue and the wake-up of the host), `repeats` times after a warm-up:
median, min, max in ms, and the achieved fraction of the bytes the call must move -- each of t, q, u, v, pmid, pint read once,
the four profiles written once, the [ncol] arrays -- against 8 TB/s (the work slabs and the second and third pass over the
outputs are traffic the call does not have to make, so they are not counted).  tools/boundary_layer_ab.py gives the time of
boundary_layer_kernel, the nearest kernel of the same structure, at the same shapes (--sizes 8192 --nlay 30 | 60).
Before timing, the device result of the first `statement-columns` columns is compared with the numpy statement at the stored
tolerances.  Fails where there is no GPU: no fall-back."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

PEAK = 8.0e12      # bytes per second
DIAG = ("precl", "sh_out", "lh_out")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ncol", type=int, default=8192)
    ap.add_argument("--nlays", default="30,60")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--batch", type=int, default=20)
    ap.add_argument("--statement-columns", type=int, default=128)
    a = ap.parse_args()
    from climt_amd import _hip
    from climt_amd._lib import Context
    from climt_amd.build import source_hash
    import simple_physics_cases as X
    ctx = Context(0)
    ncol = a.ncol
    print("simple_physics_ab: source %s; %d repeats; device: %d calls per synchronise, deferred mode; all three processes on; per call:" % (
        source_hash(), a.repeats, a.batch))
    for nlay in [int(s) for s in a.nlays.split(",")]:
        for kind, name in (("dry_calm", "dry_calm"), ("raining_wind", "varied")):
            base, flags = X._inputs(name, nlay, min(ncol, 130))
            c = {k: np.ascontiguousarray(np.tile(v, -(-ncol // v.shape[-1]))[..., :ncol]) for k, v in base.items()}
            switches = dict(zip(X.SWITCH_NAMES + X.FLAGS, X.SWITCHES["all"] + tuple(flags)), clamp_latent_heat_flux=1)
            ns = min(a.statement_columns, ncol)
            want = X.statement(*(c[k][..., :ns] for k in X.INPUTS), X.SWITCHES["all"], flags, clamp=True)
            assert want["margin"] >= X.MIN_MARGIN, want["margins"]
            dev = {k: _hip.DeviceArray.from_host(c[k]) for k in X.INPUTS}
            out = [_hip.DeviceArray((nlay, ncol)) for _ in range(4)]
            diag = {n: _hip.DeviceArray((ncol,)) for n in DIAG}

            def device():
                ctx.simple_physics(*(dev[k] for k in X.INPUTS[:7]), X.DT, X.CONSTANTS, switches, ts=dev["ts"], qsurf=dev["qsurf"], lat=dev["lat"],
                                   t_out=out[0], q_out=out[1], u_out=out[2], v_out=out[3], diagnostics=diag, memspace=1, ncol=ncol, nlay=nlay)

            device()
            ctx.synchronize()
            got = dict(zip(X.PROFILES, (o.download()[..., :ns] for o in out)))
            got.update({k: diag[n].download()[:ns] for k, n in zip(X.DIAGNOSTICS, DIAG)})
            d = X.deviations(got, want)
            assert X.within(d, X.tolerances(name, "all")), d

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
            md = float(np.median(td))
            moved = 8.0 * (10 * nlay * ncol + ncol + 6 * ncol)
            print("  %7d x %d %-12s (%d saturated layers, wind %.1f..%.1f m/s, rain in %d of %d columns; largest deviation from the statement %.1e)" % (
                ncol, nlay, kind, int(want["saturated"].sum()), float(want["wind"].min()), float(want["wind"].max()), int((want["precl"] > 0).sum()), ns, max(d.values())))
            print("      device  median %8.4f ms   min %8.4f ms   max %8.4f ms;  %.1f MB to move: %.1f %% of 8 TB/s" % (
                md, min(td), max(td), moved / 1e6, 100.0 * moved / (md * 1e-3) / PEAK))
    ctx.close()


if __name__ == "__main__":
    main()
