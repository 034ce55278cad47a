#!/usr/bin/env python3
"""Cost of in-call McICA mask generation under exponential-random overlap (icld 5) against maximum-random overlap (icld 2):
device-resident flux calls of one shape, the two modes interleaved on one GPU, both generators and both spectra.

    python tools/exp_overlap_ab.py [--ncol 8192] [--nlay 60] [--pairs 9]

Prints, per (spectrum, generator), the median wall time of a synchronous device-pointer call in each mode and the difference.
The two modes draw other masks, so the solves see other cloud fields: the difference is the whole call's, of which the mask
step (twice the draws per sub-column, one more [nlay][ncol] input) is the part that this option adds."""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ncol", type=int, default=8192)
    ap.add_argument("--nlay", type=int, default=60)
    ap.add_argument("--pairs", type=int, default=9)
    a = ap.parse_args()
    from climt_amd import _hip
    from climt_amd._lib import Context
    from climt_amd.rrtmg.common import physical_constants
    from climt_amd.synthetic import make_columns
    ctx = Context(0)
    ctx.set_constants(**physical_constants())
    ctx.sw_init(1004.64); ctx.lw_init(1004.64)
    c = make_columns(a.ncol, a.nlay, cloudy=True, seed=7); c.pop("lat")
    c.update(iaer=0, adjes=1.0, dyofyr=1, scon=1367.0, isolvar=0, inflg=2, iceflg=1, liqflg=1)
    nlay, ncol = c["play"].shape
    dev = {k: _hip.DeviceArray.from_host(v) for k, v in c.items() if isinstance(v, np.ndarray)}
    alpha = _hip.DeviceArray((nlay, ncol))
    ctx.overlap_alpha(dev["play"].ptr, dev["tlay"].ptr, 2000.0, 287.0 / 9.80665, out=alpha.ptr, memspace=1, ncol=ncol, nlay=nlay)
    ctx.set_mcica_overlap_alpha("both", alpha.ptr, memspace=1, ncol=ncol, nlay=nlay)
    names = {"sw": ("swuflx", "swdflx", "swhr", "swuflxc", "swdflxc", "swhrc"), "lw": ("uflx", "dflx", "hr", "uflxc", "dflxc", "hrc")}
    print("exp_overlap_ab: %d columns x %d layers, %d interleaved pairs, device pointers, synchronous calls" % (ncol, nlay, a.pairs))
    for which in ("sw", "lw"):
        out = {k: _hip.DeviceArray((nlay + (0 if k.endswith(("hr", "hrc")) else 1), ncol)) for k in names[which]}
        fn = ctx.sw_fluxes if which == "sw" else ctx.lw_fluxes
        for irng, gen in ((0, "kissvec"), (1, "mersenne_twister")):
            args = {k: v for k, v in c.items() if k not in dev}
            args.update({k: v.ptr for k, v in dev.items()}); args.update(ncol=ncol, nlay=nlay, irng=irng, permuteseed=684)

            def run(icld):
                t0 = time.perf_counter()
                fn(dict(args, icld=icld), mcica=True, out={k: v.ptr for k, v in out.items()}, memspace=1)
                ctx.synchronize()
                return (time.perf_counter() - t0) * 1e3
            for _ in range(2):
                run(2); run(5)
            t2, t5 = [], []
            for _ in range(a.pairs):
                t2.append(run(2)); t5.append(run(5))
            m2, m5 = float(np.median(t2)), float(np.median(t5))
            # steady state: one mode call after call, as a model runs it (the twister's jump polynomials stay on the device
            # while the grid and the mode stay the same; interleaving the modes uploads them again on every call)
            s2 = [run(2) for _ in range(a.pairs + 1)][1:]
            s5 = [run(5) for _ in range(a.pairs + 1)][1:]
            print("%s %-16s icld 2: %7.3f ms   icld 5: %7.3f ms   difference %+7.3f ms (%+.1f %%)   [min %.3f / %.3f]"
                  % (which, gen, m2, m5, m5 - m2, 100.0 * (m5 - m2) / m2, min(t2), min(t5)))
            print("%s %-16s steady state, not interleaved: icld 2 %7.3f ms   icld 5 %7.3f ms   difference %+7.3f ms"
                  % (which, gen, float(np.median(s2)), float(np.median(s5)), float(np.median(s5)) - float(np.median(s2))))
    # the host-state route of the components (climt_amd.rrtmg.common.set_overlap_alpha: pressure and temperature up, alpha formed
    # and copied on the device) against the four-transfer route through host arrays (alpha down and up again), per spectrum
    from climt_amd.rrtmg.common import rd_over_g, set_overlap_alpha

    def via_host():
        ctx.set_mcica_overlap_alpha("sw", ctx.overlap_alpha(c["play"], c["tlay"], 2000.0, rd_over_g()))
    for name, fn in (("alpha kept on the device (2 uploads)", lambda: set_overlap_alpha(ctx, "sw", 2000.0, c["play"], c["tlay"])),
                     ("alpha through host arrays (2 uploads, 1 download, 1 upload)", via_host)):
        t = []
        for i in range(a.pairs + 2):
            t0 = time.perf_counter()
            fn()
            ctx.synchronize()
            t.append((time.perf_counter() - t0) * 1e3)
        print("host-state component, alpha step per spectrum and call: %-62s %7.3f ms (median of %d)" % (name, float(np.median(t[2:])), a.pairs))
    ctx.close()


if __name__ == "__main__":
    main()
