#!/usr/bin/env python3
"""The table-driven correlated-k longwave (rrtmg_hip_cork_longwave): what a call costs, device resident, against the bytes it must
move, with RRTMGLongwave's clear-sky call on the same grid beside it as context.

    timeout -k 10 600 python tools/cork_ab.py [--ncol 8192] [--nlays 30,60] [--repeats 5] [--batch 10] [--statement-columns 128]
                                              [--table <k-table .npz>] [--out profiles/cork_ab.txt]

Table: tests/golden/cork_table_earth4.npz (4 bands x 8 g-points, rank 7, continuum, float32) unless --table names another file of
the premixed-background kind, the reference's full earth_low_res_lw.npz (14 bands) say.  Inputs: the atmosphere of the "cloudy" case
of tests/cork_cases.py (130 columns of their own numbers, repeated), emissivity 1 and cloud depth in every third layer for the
table's own bands.
Per shape and arm: device pointers, deferred mode, `batch` calls enqueued back to back and ONE synchronise behind them (a single
call would measure the enqueue and the wake-up of the host; a call is two launches, cork_band_kernel and cork_broadband_kernel, and
nothing else, so this is the kernels' time), `repeats` times after a warm-up: median, min, max in ms per call; the bytes the call
must move (every input read once, every output written once; the per-band fluxes that go to work space where the caller does not
ask for them are traffic the call does not have to make and are not counted) and the time those bytes take at 8 TB/s -- the floor.
  all   every diagnostic written, the cloud depth read
  lean  up, dn and tend only, no cloud depth
  rrtmg rrtmg_hip_lw_fluxes, clear sky (icld 0), same columns and layers: context only -- another scheme, 16 bands x 140 g-points
Before timing, the device result of the first `statement-columns` columns is compared with the numpy statement at the stored
tolerances of the "cloudy" case.  The lines go to stdout and to --out.  Fails where there is no GPU: no fall-back."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

PEAK = 8.0e12      # bytes per second


def must_move(nlay, nband, ngas_arrays):
    """8-byte words per column that each arm must move."""
    lean_in = 2 * nlay + (nlay + 1) + 1 + nband + ngas_arrays * nlay      # t, p, p_int, tsfc, emis, the gases
    lean_out = 2 * (nlay + 1) + nlay                                      # up, dn, tend
    return dict(lean=lean_in + lean_out,
                all=lean_in + nlay * nband + lean_out + nlay + 2 * nband * (nlay + 1) + 3 * nband * nlay)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ncol", type=int, default=8192)
    ap.add_argument("--nlays", default="30,60")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--batch", type=int, default=10)
    ap.add_argument("--statement-columns", type=int, default=128)
    ap.add_argument("--table", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cork_ab.txt"))
    a = ap.parse_args()
    from climt_amd import _hip, cork
    from climt_amd._lib import Context
    from climt_amd.build import source_hash
    from climt_amd.rrtmg.common import physical_constants
    from climt_amd.synthetic import make_columns
    import cork_cases as X
    path = a.table or X.table_path("earth4")
    kt = cork.KTable(path)
    if kt.gas_rule != 1 or not kt.has_co2_axis:
        raise SystemExit("cork_ab: --table must be a premixed-background table with the H2O and the CO2 axis, as earth4 is")
    with np.load(path, allow_pickle=False) as z:
        tab = {k: z[k] for k in z.files}
    tab.update(rule=1, gases=["h2o", "co2"])
    ctx = Context(0)
    ctx.set_constants(**physical_constants())
    ctx.lw_init(1004.64)
    handle = kt.upload(ctx)
    nband, ncol, lines = kt.nband, a.ncol, []
    constants = dict(m_h2o=X.M_H2O, sigma_sb=X.SIGMA_SB, g=X.G, cpd=X.CPD, diffusivity=1.66)

    def say(text):
        print(text, flush=True)
        lines.append(text)

    say("cork_ab: source %s; table %s: %d bands x %d g-points, k %s %s; %d repeats; device pointers, %d calls per synchronise, deferred mode; per call:" % (
        source_hash(), os.path.basename(path), nband, kt.ngpt, kt.k.dtype, "x".join(str(n) for n in kt.k.shape[3:]), a.repeats, a.batch))
    for nlay in [int(s) for s in a.nlays.split(",")]:
        own = min(ncol, 130)
        tile = lambda v, axis=-1: np.ascontiguousarray(np.take(v, np.arange(ncol) % v.shape[axis], axis=axis))
        base = X._inputs("cloudy", nlay, own)
        c = {k: tile(base[k]) for k in ("t", "p", "p_int", "tsfc", "h2o", "co2")}
        c["emis"] = np.ones((nband, ncol))
        lev, col = np.arange(nlay)[:, None, None], np.arange(ncol)[None, :, None]
        c["taucld"] = np.ascontiguousarray(((lev + col) % 3 == 0) * (0.2 + 0.7 * np.arange(nband)[None, None, :] / nband) * np.ones((nlay, ncol, nband)))
        ns = min(a.statement_columns, ncol)
        cs = {k: np.ascontiguousarray(v[:, :ns, :] if k == "taucld" else v[..., :ns]) for k, v in c.items()}
        want = X.statement(tab, cs, 1.66)
        dev = {k: _hip.DeviceArray.from_host(v) for k, v in c.items()}
        shapes = dict(up=(nlay + 1, ncol), dn=(nlay + 1, ncol), tend=(nlay, ncol), hr=(nlay, ncol), up_band=(nband, nlay + 1, ncol), dn_band=(nband, nlay + 1, ncol),
                      tau_band=(nband, nlay, ncol), trans_band=(nband, nlay, ncol), hr_band=(nband, nlay, ncol))
        out = {n: _hip.DeviceArray(s) for n, s in shapes.items()}
        head = (handle, nband, dev["t"], dev["p"], dev["p_int"], dev["tsfc"], dev["emis"], constants, kt.gas_rule)
        kw = dict(gases=[dev["h2o"], dev["co2"]], gas_scale=kt.gas_scale, up=out["up"], dn=out["dn"], tend=out["tend"], memspace=1, ncol=ncol, nlay=nlay)

        def every():
            ctx.cork_longwave(*head, taucld=dev["taucld"], diagnostics={n: out[n] for n in X.FIELDS[3:]}, **kw)

        def lean():
            ctx.cork_longwave(*head, diagnostics=None, **kw)

        r = make_columns(ncol, nlay, cloudy=False, seed=7)
        r.pop("lat", None)
        r.update(icld=0, inflg=2, iceflg=1, liqflg=1, idrv=0)
        lw_names = ("play", "plev", "tlay", "tlev", "tsfc", "h2o", "o3", "co2", "ch4", "n2o", "o2", "cfc11", "cfc12", "cfc22", "ccl4", "emis", "cldfr", "cicewp", "cliqwp", "reice", "reliq")
        rdev = {n: _hip.DeviceArray.from_host(r[n]) for n in lw_names}
        rargs = {n: v for n, v in r.items() if not isinstance(v, np.ndarray)}
        rargs.update({n: v.ptr for n, v in rdev.items()})
        rargs.update(ncol=ncol, nlay=nlay)
        rout = {n: _hip.DeviceArray((nlay + (0 if n in ("hr", "hrc") else 1), ncol)) for n in ("uflx", "dflx", "hr", "uflxc", "dflxc", "hrc")}

        def rrtmg():
            ctx.lw_fluxes(rargs, mcica=False, out={n: v.ptr for n, v in rout.items()}, memspace=1)

        # the numbers first
        every()
        ctx.synchronize()
        got = {n: np.ascontiguousarray(out[n].download().reshape(shapes[n])[..., :ns]) for n in X.FIELDS}
        d = X.deviations(got, want)
        assert X.within(d, X.tolerances("cloudy")), d
        ctx.cork_longwave(*head, taucld=dev["taucld"], diagnostics=None, **kw)      # (the same call without the optional outputs: the same bits)
        ctx.synchronize()
        assert all(X.same_bits(out[n].download().reshape(shapes[n])[..., :ns], got[n]) for n in ("up", "dn", "tend"))
        rrtmg()
        ctx.synchronize()

        def timed(fn):
            ctx.synchronize()
            t0 = time.perf_counter()
            for _ in range(a.batch):
                fn()
            ctx.synchronize()
            return (time.perf_counter() - t0) * 1e3 / a.batch
        words = must_move(nlay, nband, 2)
        say("  %d x %d (largest deviation of the first %d columns from the statement %.1e; up, dn, tend keep their bits without the optional outputs)" % (ncol, nlay, ns, max(d.values())))
        ctx.set_deferred(True)
        for key, label, fn in (("all", "all diagnostics, cloud depth", every), ("lean", "up, dn, tend only", lean), (None, "RRTMGLongwave clear sky", rrtmg)):
            timed(fn)
            t = [timed(fn) for _ in range(a.repeats)]
            m = float(np.median(t))
            if key is None:
                say("      %-30s median %8.4f ms   min %8.4f ms   max %8.4f ms   (context: another scheme)" % (label, m, min(t), max(t)))
                continue
            moved = 8.0 * words[key] * ncol
            say("      %-30s median %8.4f ms   min %8.4f ms   max %8.4f ms;  %7.2f MB to move: floor %7.4f ms at 8 TB/s, %6.1f x the floor;  %.2f ns per column, band and layer" % (
                label, m, min(t), max(t), moved / 1e6, moved / PEAK * 1e3, m * 1e-3 / (moved / PEAK), m * 1e6 / (float(ncol) * nband * nlay)))
        ctx.set_deferred(False)
    ctx.cork_table_destroy(handle)
    ctx.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
