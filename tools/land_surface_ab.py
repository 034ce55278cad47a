#!/usr/bin/env python3
"""The land surface (rrtmg_hip_bucket_hydrology, rrtmg_hip_second_best): what the two kernels cost, device resident.

    timeout -k 10 600 python tools/land_surface_ab.py [--ncol 8192] [--repeats 11] [--batch 20] [--statement-columns 130] [--out profiles/land_surface_ab.txt]

Inputs: cases of tests/land_surface_cases.py, 130 columns of their own numbers, repeated.  SecondBEST `mixed_types` (half the
columns land or land ice, both stability branches: the lanes of a wave diverge) and `unstable_day` (every column active) at 4 and
12 soil levels; BucketHydrology `below_beta` (one layer) and `drainage` (two).  Per configuration: device pointers, deferred mode,
`batch` calls enqueued back to back and ONE synchronise behind them (a single launch would measure the enqueue and the wake-up of
the host), `repeats` times after a warm-up: median, min, max in ms per call, and the effective bandwidth over the bytes the call
must move (every input read and every output written once; the two work slabs of SecondBEST are not counted), as GB/s and as a
fraction of 8 TB/s.  Before timing, the device result of the first `statement-columns` columns is compared with the numpy
statement: the Bucket bit for bit, SecondBEST to the fixtures' tolerances with the flags exactly.  The lines go to stdout and to
--out.  Fails where there is no GPU: no fall-back."""
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
    ap.add_argument("--repeats", type=int, default=11)
    ap.add_argument("--batch", type=int, default=20)
    ap.add_argument("--statement-columns", type=int, default=130)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "land_surface_ab.txt"))
    a = ap.parse_args()
    from climt_amd import _hip, _lib
    from climt_amd._lib import Context
    from climt_amd.build import source_hash
    import land_surface_cases as X
    ctx = Context(0)
    ncol, lines = a.ncol, []

    def say(text):
        print(text, flush=True)
        lines.append(text)

    def timed(fn, batch):
        ctx.synchronize()
        t0 = time.perf_counter()
        for _ in range(batch):
            fn()
        ctx.synchronize()
        return (time.perf_counter() - t0) * 1e3 / batch

    def measure(label, fn, moved, note):
        ctx.set_deferred(True)
        timed(fn, a.batch)
        t = [timed(fn, a.batch) for _ in range(a.repeats)]
        ctx.set_deferred(False)
        m = float(np.median(t))
        say("  %-34s median %8.4f ms   min %8.4f ms   max %8.4f ms;  %6.2f MB to move: %7.1f GB/s, %5.2f %% of 8 TB/s  (%s)" % (
            label, m, min(t), max(t), moved / 1e6, moved / (m * 1e-3) / 1e9, 100.0 * moved / (m * 1e-3) / PEAK, note))

    say("land_surface_ab: source %s; %d columns; %d repeats; device pointers: %d calls per synchronise, deferred mode; per call:" % (source_hash(), ncol, a.repeats, a.batch))
    tile = lambda v: np.ascontiguousarray(np.tile(v, -(-ncol // v.shape[-1]))[..., :ncol])
    ns = min(a.statement_columns, ncol, 130)
    for name in ("mixed_types", "unstable_day"):
        for nlay in (4, 12):
            case = X.best_case(name, nlay, 130)
            c = {k: tile(case[k]) for k in X.BEST_INPUTS}
            dev = {k: _hip.DeviceArray.from_host(v) for k, v in c.items()}
            shape = lambda n: (nlay, ncol) if n in ("t_soil_out", "x_w_out", "x_i_out") else (ncol,)
            outs = {n: _hip.DeviceArray(shape(n)) for n in _lib.SECOND_BEST_OUT}
            diag = {n: _hip.DeviceArray((ncol,), np.int32 if n == "flags" else np.float64) for n in _lib.SECOND_BEST_DIAG}
            fn = lambda: ctx.second_best(dev, case["dt"], X.best_constants(name), outs=outs, diagnostics=diag, memspace=1, ncol=ncol, nlay=nlay)
            fn()
            ctx.synchronize()
            got = {n: x.download()[..., :ns] for n, x in list(outs.items()) + list(diag.items())}
            want = {f: case[f][..., :ns] for f in X.BEST_FIELDS + ("flags",)}
            assert X.within(X.deviations(got, want, X.BEST_FIELDS), X.tolerances(name)) and X.same_bits(got["flags"], want["flags"]), (name, nlay)
            moved = (8.0 * (7 * nlay + 12 + 2 + 11) + 8.0) * ncol
            measure("second_best %s, %d levels" % (name, nlay), fn, moved, "%d of %d columns active, within the fixtures' tolerances of the statement" % (int((want["flags"] & 1).sum()), ns))
    for name in ("below_beta", "drainage"):
        case = X.bucket_case(name, 130)
        layers = case["layers"]
        c = {k: tile(case[k]) for k in X.BUCKET_INPUTS if k in case}
        dev = {k: _hip.DeviceArray.from_host(v) for k, v in c.items()}
        outs = {n: _hip.DeviceArray((ncol,)) for n in _lib.BUCKET_HYDROLOGY_OUT[:2 * layers]}
        diag = {n: _hip.DeviceArray((ncol,)) for n in _lib.BUCKET_HYDROLOGY_DIAG[:4 + 2 * (layers - 1)]}
        fn = lambda: ctx.bucket_hydrology(layers, dev, case["dt"], case["scalars"], outs=outs, diagnostics=diag, memspace=1, ncol=ncol)
        fn()
        ctx.synchronize()
        got = {n: x.download()[:ns] for n, x in list(outs.items()) + list(diag.items())}
        assert all(X.same_bits(got[f], case[f][:ns]) for f in X.BUCKET_FIELDS[layers]), name
        measure("bucket_hydrology %s, %d layer%s" % (name, layers, "s" * (layers - 1)), fn, 8.0 * (len(dev) + len(outs) + len(diag)) * ncol, "the same bits as the statement")
    ctx.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
