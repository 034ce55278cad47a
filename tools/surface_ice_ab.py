#!/usr/bin/env python3
"""The snow/ice column (rrtmg_hip_surface_ice): what the kernel costs, device resident, and what the host-pointer call costs.

    timeout -k 10 600 python tools/surface_ice_ab.py [--ncol 8192] [--nlay 30] [--repeats 5] [--batch 20] [--statement-columns 128] [--out profiles/surface_ice_ab.txt]

Inputs: sea-ice cases of tests/surface_ice_cases.py, 130 columns of their own numbers, repeated.  Three column mixes: "all cold"
(flux top, one solve), "all melting" (Dirichlet top, melt inside the snow) and "half inactive" (every other column open sea: the
lanes of a wave diverge).  Per mix: device pointers, deferred mode, `batch` calls enqueued back to back and ONE synchronise behind
them (a single launch would measure the enqueue and the wake-up of the host), `repeats` times after a warm-up: median, min, max in
ms per call, and the effective bandwidth over the bytes the call must move, as GB/s and as a fraction of 8 TB/s.  Per column: t read
and t_out, height_out written (3 nlay words of 8 bytes; a column that is not active reads `height` too, nlay more -- an active
one never does), 9 [ncol] inputs and 6 [ncol] outputs of 8 bytes, the area type and the flags of 4 bytes; the two work slabs,
written and read back once, are traffic the call does not have to make and are not counted.  Then the host-pointer call on the same arrays (staging
both ways included, one call per synchronise).  Before timing, the device result of the first `statement-columns` columns is
compared with the numpy statement: the same bits.  The lines go to stdout and to --out.  Fails where there is no GPU: no fall-back."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

PEAK = 8.0e12      # bytes per second


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ncol", type=int, default=8192)
    ap.add_argument("--nlay", type=int, default=30)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--batch", type=int, default=20)
    ap.add_argument("--statement-columns", type=int, default=128)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "surface_ice_ab.txt"))
    a = ap.parse_args()
    from climt_amd import _hip
    from climt_amd._lib import SURFACE_ICE_OUT, Context
    from climt_amd.build import source_hash
    import surface_ice_cases as X
    ctx = Context(0)
    ncol, nlay, lines = a.ncol, a.nlay, []

    def say(text):
        print(text, flush=True)
        lines.append(text)

    say("surface_ice_ab: source %s; %d x %d, kind 0; %d repeats; device pointers: %d calls per synchronise, deferred mode; per call:" % (
        source_hash(), ncol, nlay, a.repeats, a.batch))
    must_move = lambda inactive: (8.0 * ((3.0 + inactive) * nlay + 15) + 8.0) * ncol      # bytes; `inactive`: the fraction of such columns
    tile = lambda v: np.ascontiguousarray(np.tile(v, -(-ncol // v.shape[-1]))[..., :ncol])
    for label, name in (("all cold", "cold"), ("all melting", "melting"), ("half inactive", "cold")):
        case = X.ice_case(0, name, nlay, min(ncol, 130))
        c = {k: tile(case[k]) for k in X.INPUTS}
        if label == "half inactive":
            c["area_type"][::2] = 2
        moved = must_move(0.5 if label == "half inactive" else 0.0)
        ns = min(a.statement_columns, ncol)
        want = X.ice_statement(0, *(c[k][..., :ns] for k in X.INPUTS), case["dt"])
        dev = {k: _hip.DeviceArray.from_host(v) for k, v in c.items()}
        shape = lambda n: (nlay, ncol) if n in ("t_out", "height_out") else (ncol,)
        out = {n: _hip.DeviceArray(shape(n)) for n in SURFACE_ICE_OUT + ("cond_flux", "albedo")}
        out["flags"] = _hip.DeviceArray((ncol,), np.int32)
        outs = {n: out[n] for n in SURFACE_ICE_OUT}
        diag = {n: out[n] for n in ("cond_flux", "albedo", "flags")}

        def device():
            ctx.surface_ice(0, dev["t"], dev["height"], dev["thick"], dev["snow"], dev["base"], {k: dev[k] for k in X.FLUXES}, dev["area_type"], case["dt"],
                            X.constants(0), diagnostics=diag, memspace=1, ncol=ncol, nlay=nlay, **outs)

        def host():
            ctx.surface_ice(0, c["t"], c["height"], c["thick"], c["snow"], c["base"], {k: c[k] for k in X.FLUXES}, c["area_type"], case["dt"], X.constants(0))

        device()
        ctx.synchronize()
        got = {n: out[n].download()[..., :ns] for n in out}
        assert all(X.same_bits(got[f], want[f]) for f in X.FIELDS + ("flags",)), label

        def timed(fn, batch):
            ctx.synchronize()
            t0 = time.perf_counter()
            for _ in range(batch):
                fn()
            ctx.synchronize()
            return (time.perf_counter() - t0) * 1e3 / batch
        ctx.set_deferred(True)
        timed(device, a.batch)
        t = [timed(device, a.batch) for _ in range(a.repeats)]
        ctx.set_deferred(False)
        m = float(np.median(t))
        say("  %-14s kernel  median %8.4f ms   min %8.4f ms   max %8.4f ms;  %6.2f MB to move: %7.1f GB/s, %5.2f %% of 8 TB/s  (%d of %d columns active, the same bits as the statement)" % (
            label, m, min(t), max(t), moved / 1e6, moved / (m * 1e-3) / 1e9, 100.0 * moved / (m * 1e-3) / PEAK, int((want["flags"] & 1).sum()), ns))
        timed(host, 2)
        t = [timed(host, 1) for _ in range(a.repeats)]
        say("  %-14s host-pointer call  median %8.4f ms   min %8.4f ms   max %8.4f ms" % (label, float(np.median(t)), min(t), max(t)))
    ctx.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
