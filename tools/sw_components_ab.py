"""Cost of the shortwave flux components: device-event time of one device-resident rrtmg_hip_sw_fluxes call with the
components off and on (all eight requested), interleaved off / on, plus the two solve kernels' event times
(rrtmg_hip_kernel_ms).  Writes the table to stdout (profiles/sw_components_ab.txt is its output).

    python tools/sw_components_ab.py [--alternations 8]
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from climt_amd import _hip  # noqa: E402
from climt_amd._lib import SW_COMPONENTS, SW_OUT, Context, source_hash  # noqa: E402
from climt_amd.synthetic import make_columns  # noqa: E402
from oracle.ref_driver import CONSTANTS, CPDAIR  # noqa: E402

BASE = dict(icld=1, iaer=0, adjes=1.0, dyofyr=1, scon=1367.0, isolvar=0, inflg=2, iceflg=1, liqflg=1, irng=0, permuteseed=5)
CONFIGS = (("8192x60 clear", 8192, 60, False), ("8192x60 McICA", 8192, 60, True), ("131072x60 clear", 131072, 60, False))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--alternations", type=int, default=8)
    args = ap.parse_args()
    ctx = Context(0)
    ctx.set_constants(**CONSTANTS)
    ctx.sw_init(CPDAIR)
    print("# SW call time (ms, HIP events around one device-resident call), components off / on, %d alternations; library src:%s"
          % (args.alternations, source_hash()))
    print("# %-16s %10s %10s %8s   %s" % ("config", "off", "on", "on/off", "solve kernels off -> on (ms, clear + cloudy)"))
    for name, n, nlay, mcica in CONFIGS:
        c = make_columns(n, nlay, cloudy=mcica, seed=9)
        c.pop("lat")
        c.update(BASE)
        c.update(icld=2 if mcica else 0)
        dev = {k: _hip.DeviceArray.from_host(v) for k, v in c.items() if isinstance(v, np.ndarray)}
        inp = {k: v.ptr for k, v in dev.items()}
        inp.update({k: v for k, v in c.items() if not isinstance(v, np.ndarray)})
        inp.update(ncol=n, nlay=nlay)
        out = {k: _hip.DeviceArray((nlay + lev, n)) for k, lev in SW_OUT}
        comp = {k: _hip.DeviceArray((nlay + 1, n)) for k in SW_COMPONENTS}
        optr = {k: v.ptr for k, v in out.items()}
        cptr = {k: v.ptr for k, v in comp.items()}
        e0, e1 = _hip.Event(), _hip.Event()
        t = {False: [], True: []}
        kern = {False: [], True: []}

        def run(on):
            e0.record(ctx.stream)
            ctx.sw_fluxes(inp, mcica=mcica, out=optr, memspace=1, components=cptr if on else None)
            e1.record(ctx.stream)
            e1.synchronize()
            return e0.elapsed_ms(e1)
        for on in (False, True, False, True):    # warm-up: buffers, code objects
            run(on)
        for _ in range(args.alternations):
            for on in (False, True):
                t[on].append(run(on))
                k = ctx.kernel_ms("sw")
                if mcica:
                    k += ctx.kernel_ms("sw", cloudy=True)
                kern[on].append(k)
        off, on = np.median(t[False]), np.median(t[True])
        print("  %-16s %10.3f %10.3f %8.3f   %.3f -> %.3f   (off %s | on %s)" % (
            name, off, on, on / off, np.median(kern[False]), np.median(kern[True]),
            " ".join("%.3f" % x for x in t[False]), " ".join("%.3f" % x for x in t[True])))
        for v in list(dev.values()) + list(out.values()) + list(comp.values()):
            v.free()
    ctx.close()


if __name__ == "__main__":
    main()
