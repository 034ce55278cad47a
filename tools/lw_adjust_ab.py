#!/usr/bin/env python3
"""The longwave between radiation calls (rrtmg_hip_lw_adjust_surface, climt_amd.IntermittentLongwave): what an in-between step
costs against the full longwave call it stands in for.

    timeout -k 10 300 python tools/lw_adjust_ab.py [--ncol 8192] [--nlay 60] [--rounds 15] [--batch 20]

Device pointers, deferred mode, one GPU.  A side is `batch` calls enqueued back to back and ONE synchronise behind them (a single
launch of a few microseconds would measure the enqueue and the wake-up of the host); the sides -- the adjustment out of place, the
adjustment in place (one thread per column), the full longwave call (clear sky, idrv = 1) -- are alternated `rounds` times after a warm-up
of every side, and the median and the minimum per call are printed with the bytes the adjustment moves (with the clear-sky stream
7 level arrays and 2 column arrays read, 4 written; the halo levels of the blocks of layers, read twice, are not counted) and the
rate that follows.  Before timing, the
out-of-place and the in-place result are compared bit for bit with the numpy statement of tests/lw_adjust_cases.py at the timed
size.  Fails where there is no GPU: no fall-back."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ncol", type=int, default=8192)
    ap.add_argument("--nlay", type=int, default=60)
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--batch", type=int, default=20)
    a = ap.parse_args()
    from climt_amd import _hip
    from climt_amd._lib import Context
    from climt_amd.rrtmg.common import physical_constants
    from climt_amd.synthetic import make_columns
    import lw_adjust_cases as X
    ctx = Context(0)
    k = physical_constants()
    ctx.set_constants(**k)
    ctx.lw_init(1004.64)
    heatfac = k["grav"] * k["secdy"] / (1004.64 * 1.e2)
    c = make_columns(a.ncol, a.nlay, cloudy=False, seed=7)
    c.pop("lat", None)
    c.update(icld=1, inflg=2, iceflg=1, liqflg=1, idrv=1)
    nlay, ncol = c["play"].shape
    lw_names = ("play", "plev", "tlay", "tlev", "tsfc", "h2o", "o3", "co2", "ch4", "n2o", "o2", "cfc11", "cfc12", "cfc22", "ccl4", "emis", "cldfr", "cicewp", "cliqwp", "reice", "reliq")
    dev = {n: _hip.DeviceArray.from_host(c[n]) for n in lw_names}
    args = {n: v for n, v in c.items() if not isinstance(v, np.ndarray)}
    args.update({n: v.ptr for n, v in dev.items()})
    args.update(ncol=ncol, nlay=nlay)
    rows = lambda n: nlay + (0 if n in ("hr", "hrc") else 1)
    kept = {n: _hip.DeviceArray((rows(n), ncol)) for n in ("uflx", "dflx", "hr", "uflxc", "dflxc", "hrc", "duflx_dt", "duflxc_dt")}
    adjusted = {n: _hip.DeviceArray((rows(n), ncol)) for n in ("uflx", "hr", "uflxc", "hrc")}
    scratch = {n: _hip.DeviceArray((rows(n), ncol)) for n in ("uflx", "uflxc")}      # the in-place side works on copies
    rng = np.random.default_rng(3)
    tsfc_now = c["tsfc"] + rng.uniform(-3.0, 3.0, ncol)
    now = _hip.DeviceArray.from_host(tsfc_now)

    def longwave():
        ctx.lw_fluxes(args, mcica=False, out={n: v.ptr for n, v in kept.items()}, memspace=1)

    def adjust():
        ctx.lw_adjust_surface(ncol, nlay, dev["tsfc"], now, dev["plev"], (kept["uflx"], kept["dflx"], kept["duflx_dt"], adjusted["uflx"], adjusted["hr"]),
                              (kept["uflxc"], kept["dflxc"], kept["duflxc_dt"], adjusted["uflxc"], adjusted["hrc"]))

    def adjust_in_place():
        ctx.lw_adjust_surface(ncol, nlay, dev["tsfc"], now, dev["plev"], (scratch["uflx"], kept["dflx"], kept["duflx_dt"], scratch["uflx"], adjusted["hr"]),
                              (scratch["uflxc"], kept["dflxc"], kept["duflxc_dt"], scratch["uflxc"], adjusted["hrc"]))

    # ---- the results at the timed size, before any timing ----------------------------------------------------------------------
    longwave()
    ctx.synchronize()
    host = {n: v.download() for n, v in kept.items()}
    want = X.want(dict(tsfc_call=c["tsfc"], tsfc_now=tsfc_now, plev=c["plev"], **{n: host[n] for n in ("uflx", "dflx", "duflx_dt", "uflxc", "dflxc", "duflxc_dt")}), heatfac=heatfac)
    adjust()
    ctx.synchronize()
    for n, w in want.items():
        assert X.same_bits(adjusted[n].download(), w), "out of place: %s differs from the numpy statement" % n
    for n in scratch:
        scratch[n].upload(host[n])
    adjust_in_place()
    ctx.synchronize()
    for n, w in want.items():
        got = (scratch[n] if n in scratch else adjusted[n]).download()
        assert X.same_bits(got, w), "in place: %s differs from the numpy statement" % n
    print("lw_adjust_ab: %d columns x %d layers: out of place and in place equal the numpy statement bit for bit" % (ncol, nlay))

    # ---- timing -----------------------------------------------------------------------------------------------------------------
    def timed(fn):
        ctx.synchronize()
        t = time.perf_counter()
        for _ in range(a.batch):
            fn()
        ctx.synchronize()
        return (time.perf_counter() - t) * 1e3 / a.batch
    ctx.set_deferred(True)
    sides = (("adjust", adjust), ("adjust_in_place", adjust_in_place), ("longwave", longwave))
    for _ in range(3):
        for _, fn in sides:
            timed(fn)
    t = {n: [] for n, _ in sides}
    for _ in range(a.rounds):
        for n, fn in sides:
            t[n].append(timed(fn))
    ctx.set_deferred(False)
    m = {n: float(np.median(v)) for n, v in t.items()}
    from climt_amd.build import source_hash
    nl1, nl = (nlay + 1) * ncol, nlay * ncol
    needed = (7 * nl1 + 2 * ncol + 2 * nl1 + 2 * nl) * 8      # plev, 2 x (uflx, dflx, duflx_dt) and the surface temperatures read; 2 x (uflx', hr') written
    print("source %s; %d rounds of %d calls per side, alternated, deferred mode, one synchronise per side; per call:" % (source_hash(), a.rounds, a.batch))
    for n, _ in sides:
        print("  %-16s median %8.4f ms   min %8.4f ms   max %8.4f ms" % (n, m[n], min(t[n]), max(t[n])))
    print("  the adjustment moves %.1f MB at the least: %.0f GB/s out of place, %.0f GB/s in place (median)" % (needed / 1e6, needed / m["adjust"] / 1e6, needed / m["adjust_in_place"] / 1e6))
    print("  full longwave call / adjustment: %.1f x (out of place), %.1f x (in place)" % (m["longwave"] / m["adjust"], m["longwave"] / m["adjust_in_place"]))
    ctx.close()


if __name__ == "__main__":
    main()
