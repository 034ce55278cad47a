#!/usr/bin/env python3
"""The gray radiation path (rrtmg_hip_frierson_optical_depth, rrtmg_hip_gray_longwave, rrtmg_hip_grid_scale_condensation): what the
three kernels cost, device resident, and the fused call against the two separate ones.

    timeout -k 10 600 python tools/gray_ab.py [--ncol 8192] [--nlays 30,60] [--repeats 5] [--batch 20] [--statement-columns 128] [--out profiles/gray_ab.txt]

Inputs: the "varied" gray case and the "alternate" condensation case of tests/gray_cases.py, 130 columns of their own numbers,
repeated.  Per entry and shape: device pointers, deferred mode, `batch` calls enqueued back to back and ONE synchronise behind
them (a single launch would measure the enqueue and the wake-up of the host), `repeats` times after a warm-up: median, min, max
in ms per call, and the effective bandwidth over the bytes the call must move (every input read once, every output
written once; what the sweep's downward pass reads back of its own upward pass is traffic the call does not have to make and is
not counted), as GB/s and as a fraction of 8 TB/s.  "pair" is the optical depth followed by the sweep on it, two launches and the
depth through HBM; "fused" the one launch that forms the depth inside the sweep, with and without writing it out.
Before timing, the device result of the first `statement-columns` columns is compared with the numpy statements at the stored
tolerances.  The lines go to stdout and to --out.  Fails where there is no GPU: no fall-back."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

PEAK = 8.0e12      # bytes per second


def must_move(nlay):
    """8-byte words per column that each call must move."""
    return dict(frierson=2 * nlay + 4, gray=7 * nlay + 5, fused=6 * nlay + 6, fused_tau=7 * nlay + 7, pair=(2 * nlay + 4) + (7 * nlay + 5), gsc=6 * nlay + 2)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ncol", type=int, default=8192)
    ap.add_argument("--nlays", default="30,60")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--batch", type=int, default=20)
    ap.add_argument("--statement-columns", type=int, default=128)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gray_ab.txt"))
    a = ap.parse_args()
    from climt_amd import _hip
    from climt_amd._lib import Context
    from climt_amd.build import source_hash
    import gray_cases as X
    ctx = Context(0)
    ncol, lines = a.ncol, []

    def say(text):
        print(text, flush=True)
        lines.append(text)

    say("gray_ab: source %s; %d repeats; device pointers, %d calls per synchronise, deferred mode; per call:" % (source_hash(), a.repeats, a.batch))
    for nlay in [int(s) for s in a.nlays.split(",")]:
        tile = lambda v: np.ascontiguousarray(np.tile(v, -(-ncol // v.shape[-1]))[..., :ncol])
        c = {k: tile(v) for k, v in X._gray_inputs("varied", nlay, min(ncol, 130)).items()}
        g = {k: tile(v) for k, v in X._gsc_inputs("alternate", nlay, min(ncol, 130)).items()}
        ns = min(a.statement_columns, ncol)
        cut = lambda d, names: {k: d[k][..., :ns] for k in names}
        cs, gs = cut(c, X.GRAY_INPUTS), cut(g, X.GSC_INPUTS)
        want = X.gray_statement(cs["t"], cs["tsfc"], cs["p_int"], cs["tau"])
        want["tau"] = X.frierson_statement(cs["lat"], cs["p_int"], cs["ps"])
        assert X.same_bits(want["tau"], cs["tau"])
        want_g = X.gsc_statement(gs["t"], gs["q"], gs["p"], gs["p_int"])
        assert want_g["margin"] >= X.MIN_MARGIN
        dev = {k: _hip.DeviceArray.from_host(v) for k, v in c.items()}
        dev_g = {k: _hip.DeviceArray.from_host(v) for k, v in g.items()}
        il, ml = (nlay + 1, ncol), (nlay, ncol)
        out = {n: _hip.DeviceArray(il if n in ("up", "dn", "tau", "tau_out") else ml) for n in ("up", "dn", "tend", "hr", "tau", "tau_out")}
        out_g = dict(t=_hip.DeviceArray(ml), q=_hip.DeviceArray(ml), precip=_hip.DeviceArray((ncol,)))
        size = dict(memspace=1, ncol=ncol, nlay=nlay)
        flux = dict(up=out["up"], dn=out["dn"], tend=out["tend"])

        def frierson():
            ctx.frierson_optical_depth(dev["p_int"], dev["ps"], dev["lat"], X.FRIERSON, tau=out["tau"], **size)

        def gray():
            ctx.gray_longwave(dev["t"], dev["tsfc"], dev["p_int"], X.GRAY_CONSTANTS, tau=out["tau"], diagnostics=dict(hr=out["hr"]), **flux, **size)

        def pair():
            frierson()
            gray()

        def fused(tau_out=False):
            d = dict(hr=out["hr"], **(dict(tau_out=out["tau_out"]) if tau_out else {}))
            ctx.gray_longwave(dev["t"], dev["tsfc"], dev["p_int"], X.GRAY_CONSTANTS, ps=dev["ps"], lat=dev["lat"], frierson=X.FRIERSON, diagnostics=d, **flux, **size)

        def gsc():
            ctx.grid_scale_condensation(dev_g["t"], dev_g["q"], dev_g["p"], dev_g["p_int"], X.GSC_CONSTANTS, t_out=out_g["t"], q_out=out_g["q"],
                                        diagnostics=dict(precip=out_g["precip"]), **size)

        # the numbers first
        pair()
        ctx.synchronize()
        two = {n: out[n].download()[..., :ns] for n in ("up", "dn", "tend", "hr", "tau")}
        fused(True)
        ctx.synchronize()
        one = {n: out[n].download()[..., :ns] for n in ("up", "dn", "tend", "hr", "tau_out")}
        assert all(X.same_bits(one[n], two[n]) for n in X.GRAY_FIELDS) and X.same_bits(one["tau_out"], two["tau"])
        d = X.deviations(two, want, X.GRAY_FIELDS + ("tau",))
        assert X.within(d, X.tolerances("gray", "varied")), d
        gsc()
        ctx.synchronize()
        dg = X.deviations(dict(t_new=out_g["t"].download()[..., :ns], q_new=out_g["q"].download()[..., :ns], precip=out_g["precip"].download()[:ns]), want_g, X.GSC_FIELDS)
        assert X.within(dg, X.tolerances("gsc", "alternate")), dg

        def timed(fn):
            ctx.synchronize()
            t0 = time.perf_counter()
            for _ in range(a.batch):
                fn()
            ctx.synchronize()
            return (time.perf_counter() - t0) * 1e3 / a.batch
        words = must_move(nlay)
        say("  %d x %d (fused == pair bit for bit; largest deviation from the statements: gray %.1e, condensation %.1e; %d of %d layers saturated)" % (
            ncol, nlay, max(d.values()), max(dg.values()), int(want_g["saturated"].sum()), want_g["saturated"].size))
        ctx.set_deferred(True)
        medians = {}
        for key, label, fn in (("frierson", "frierson_optical_depth", frierson), ("gray", "gray_longwave (tau read)", gray), ("pair", "pair: depth, then sweep", pair),
                               ("fused", "fused, depth not written", fused), ("fused_tau", "fused, depth written", lambda: fused(True)),
                               ("gsc", "grid_scale_condensation", gsc)):
            timed(fn)
            t = [timed(fn) for _ in range(a.repeats)]
            m = medians[key] = float(np.median(t))
            moved = 8.0 * words[key] * ncol
            say("      %-26s median %8.4f ms   min %8.4f ms   max %8.4f ms;  %6.2f MB to move: %7.1f GB/s, %5.2f %% of 8 TB/s" % (
                label, m, min(t), max(t), moved / 1e6, moved / (m * 1e-3) / 1e9, 100.0 * moved / (m * 1e-3) / PEAK))
        ctx.set_deferred(False)
        say("      fused (depth written) / pair: %.3f of the time, %.2f MB less through HBM and no resident depth needed" % (
            medians["fused_tau"] / medians["pair"], 8.0 * (words["pair"] - words["fused_tau"]) * ncol / 1e6))
    ctx.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
