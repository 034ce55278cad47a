#!/usr/bin/env python3
"""The Emanuel convection scheme (rrtmg_hip_emanuel_convection, climt_amd.EmanuelConvection): what the kernel costs, device
resident, beside the 1.69 ms device-resident radiation step it joins.

    timeout -k 10 600 python tools/emanuel_ab.py [--ncol 8192] [--nlays 30,60] [--repeats 5] [--batch 10]

Three states per layer count, on the synthetic sounding T = max(200, 300 (p/1000)^0.19), q = rh q_sat (p/1000)^1.5, ph = 1000
linspace(1, 0.02), a sheared wind, dt = 600 s, qs formed by the kernel: "convecting" (rh 0.95 +- 0.03 by column, cbmf_in 0.02: every
column walks its mixing block), "quiet" (rh 0.3, cbmf_in 0: every column leaves by the DTMAX exit after one lifting) and "mixed"
(the two alternating column by column, so every wave waits for its convecting lanes).  Per state: device pointers, deferred mode,
`batch` calls enqueued back to back and ONE synchronise behind them (a single launch would measure the enqueue and the wake-up of
the host), `repeats` times after a warm-up: median, min, max.  Before timing, iflag of the state is checked (1 / 0 / alternating)
and the host-pointer call is compared bit for bit with the device-pointer one.  Fails where there is no GPU: no fall-back."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

STEP_MS = 1.69      # the device-resident SW + LW + Adams-Bashforth + slab step at 8192 x 60 (README), without this component


def sounding(nlay, rh, cbmf):
    """rh, cbmf: [ncol] -> the inputs [nlay][ncol]."""
    ncol = rh.size
    ph = 1000.0 * np.linspace(1.0, 0.02, nlay + 1)
    p = 0.5 * (ph[:-1] + ph[1:])
    t = np.maximum(200.0, 300.0 * (p / 1000.0) ** 0.19)
    es = 611.2 * np.exp(17.67 * (t - 273.15) / (t - 29.65))
    qs = (287.04 / 461.5) * es / (p * 100.0 - (1 - 287.04 / 461.5) * es)
    col = lambda x: np.ascontiguousarray(np.repeat(x[:, None], ncol, axis=1))
    return dict(t=col(t), q=np.ascontiguousarray((qs * (p / 1000.0) ** 1.5)[:, None] * rh[None, :]), u=col(5.0 + (1000.0 - p) / 100.0),
                v=col(-2.0 + 0.5 * (1000.0 - p) / 100.0), p=col(p), ph=col(ph), cbmf=np.ascontiguousarray(cbmf))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ncol", type=int, default=8192)
    ap.add_argument("--nlays", default="30,60")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--batch", type=int, default=10)
    a = ap.parse_args()
    from climt_amd import _hip
    from climt_amd._lib import Context
    from climt_amd.build import source_hash
    import emanuel_cases as X
    ctx = Context(0)
    ncol = a.ncol
    print("emanuel_ab: source %s; %d columns; %d repeats; %d calls per synchronise, deferred mode; qs formed by the kernel; per call:" % (
        source_hash(), ncol, a.repeats, a.batch))
    wet, odd = 0.95 + 0.03 * np.sin(np.arange(ncol)), np.arange(ncol) % 2 == 1
    states = (("convecting", wet, np.full(ncol, 0.02)), ("quiet", np.full(ncol, 0.3), np.zeros(ncol)),
              ("mixed", np.where(odd, 0.3, wet), np.where(odd, 0.0, 0.02)))
    for nlay in [int(s) for s in a.nlays.split(",")]:
        for kind, rh, cbmf in states:
            c = sounding(nlay, rh, cbmf)
            names = ("t", "q", "u", "v", "p", "ph", "cbmf")
            dev = {k: _hip.DeviceArray.from_host(c[k]) for k in names}
            out = [_hip.DeviceArray((nlay, ncol)) for _ in range(4)]
            cb = _hip.DeviceArray((ncol,))
            diag = dict(precip=_hip.DeviceArray((ncol,)), iflag=_hip.DeviceArray((ncol,), np.int32))

            def device():
                ctx.emanuel_convection(*(dev[k] for k in names), 600.0, X.PARAMETERS, X.CONSTANTS, ft=out[0], fq=out[1], fu=out[2], fv=out[3],
                                       cbmf_out=cb, diagnostics=diag, memspace=1, ncol=ncol, nlay=nlay)

            device()
            ctx.synchronize()
            flag, precip = diag["iflag"].download(), diag["precip"].download()
            want = dict(convecting=np.ones(ncol), quiet=np.zeros(ncol), mixed=np.where(odd, 0, 1))[kind]
            assert np.array_equal(flag, want), (kind, nlay, np.bincount(flag))
            h = ctx.emanuel_convection(*(c[k] for k in names), 600.0, X.PARAMETERS, X.CONSTANTS)
            assert all(X.same_bits(x, o.download()) for x, o in zip(h[:4], out)) and X.same_bits(h[5]["precip"], precip), "host and device pointers differ"

            def timed(batch):
                ctx.synchronize()
                t0 = time.perf_counter()
                for _ in range(batch):
                    device()
                ctx.synchronize()
                return (time.perf_counter() - t0) * 1e3 / batch
            ctx.set_deferred(True)
            timed(a.batch)
            td = [timed(a.batch) for _ in range(a.repeats)]
            ctx.set_deferred(False)
            md = float(np.median(td))
            print("  %6d x %d %-10s (precipitation %.2f..%.2f mm/day)  median %8.4f ms   min %8.4f ms   max %8.4f ms   %5.0f %% of the %.2f ms step" % (
                ncol, nlay, kind, float(precip.min()), float(precip.max()), md, min(td), max(td), 100.0 * md / STEP_MS, STEP_MS))
    print("  work space per column: %d bytes at 30 layers, %d at 60" % tuple(8 * (22 * (n + 1) + 6 * (n - 4) * (n - 3)) for n in (30, 60)))
    ctx.close()


if __name__ == "__main__":
    main()
