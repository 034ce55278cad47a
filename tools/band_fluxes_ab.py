"""Cost of the fluxes by band: device-event time of one device-resident rrtmg_hip_{sw,lw}_fluxes call, plain against a band
call with every member requested -- levels=1 (surface and top) and levels=0 (all interface levels) -- interleaved plain /
levels=1 / levels=0.  Writes the table to stdout (profiles/band_fluxes_ab.txt is its output).

    python tools/band_fluxes_ab.py [--alternations 6] [--cloudy] [--sizes 8192,131072]
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from climt_amd import _hip  # noqa: E402
from climt_amd._lib import LW_BAND_FLUXES, LW_OUT, SW_BAND_FLUXES, SW_OUT, Context, source_hash  # noqa: E402
from climt_amd.synthetic import make_columns  # noqa: E402
from oracle.ref_driver import CONSTANTS, CPDAIR  # noqa: E402

BASE = dict(icld=1, iaer=0, adjes=1.0, dyofyr=1, scon=1367.0, isolvar=0, inflg=2, iceflg=1, liqflg=1, irng=0, permuteseed=5)
MODES = ("plain", "boundaries", "all")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--alternations", type=int, default=6)
    ap.add_argument("--cloudy", action="store_true", help="McICA cloudy columns instead of clear sky")
    ap.add_argument("--sizes", default="8192,131072")
    args = ap.parse_args()
    nlay = 60
    ctx = Context(0)
    ctx.set_constants(**CONSTANTS)
    ctx.sw_init(CPDAIR)
    ctx.lw_init(CPDAIR)
    print("# call time (ms, HIP events around one device-resident call): plain, bands levels=1, bands levels=0 (all members), %d alternations,"
          " %s; library src:%s" % (args.alternations, "McICA cloudy" if args.cloudy else "clear sky", source_hash()))
    print("# %-18s %9s %9s %9s %8s %8s" % ("config", "plain", "levels=1", "levels=0", "l1/plain", "l0/plain"))
    for n in [int(x) for x in args.sizes.split(",")]:
        c = make_columns(n, nlay, cloudy=args.cloudy, seed=9)
        c.pop("lat")
        c.update(BASE)
        dev = {k: _hip.DeviceArray.from_host(v) for k, v in c.items() if isinstance(v, np.ndarray)}
        inp = {k: v.ptr for k, v in dev.items()}
        inp.update({k: v for k, v in c.items() if not isinstance(v, np.ndarray)})
        inp.update(ncol=n, nlay=nlay)
        for which, outs, members, nband in (("sw", SW_OUT, SW_BAND_FLUXES, 14), ("lw", LW_OUT, LW_BAND_FLUXES, 16)):
            inp["icld"] = (2 if which == "sw" else 1) if args.cloudy else 0
            out = {k: _hip.DeviceArray((nlay + lev, n)) for k, lev in outs}
            band = {"all": {m: _hip.DeviceArray((nband, nlay + 1, n)) for m in members},
                    "boundaries": {m: _hip.DeviceArray((nband, 2, n)) for m in members}}
            optr = {k: v.ptr for k, v in out.items()}
            call = ctx.sw_fluxes if which == "sw" else ctx.lw_fluxes
            e0, e1 = _hip.Event(), _hip.Event()
            t = {m: [] for m in MODES}

            def run(mode):
                kw = {} if mode == "plain" else dict(bands={m: v.ptr for m, v in band[mode].items()}, band_levels=mode)
                e0.record(ctx.stream)
                call(inp, mcica=args.cloudy, out=optr, memspace=1, **kw)
                e1.record(ctx.stream)
                e1.synchronize()
                return e0.elapsed_ms(e1)
            for mode in MODES + MODES:    # warm-up: buffers, code objects
                run(mode)
            for _ in range(args.alternations):
                for mode in MODES:
                    t[mode].append(run(mode))
            med = {m: float(np.median(t[m])) for m in MODES}
            print("  %-18s %9.3f %9.3f %9.3f %8.3f %8.3f   (%s)" % (
                "%s %dx%d" % (which, n, nlay), med["plain"], med["boundaries"], med["all"], med["boundaries"] / med["plain"], med["all"] / med["plain"],
                " | ".join(m + " " + " ".join("%.3f" % x for x in t[m]) for m in MODES)))
            for v in list(out.values()) + [x for b in band.values() for x in b.values()]:
                v.free()
        for v in dev.values():
            v.free()
    ctx.close()


if __name__ == "__main__":
    main()
