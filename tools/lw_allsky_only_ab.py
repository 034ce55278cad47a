"""Gain of the longwave call without the clear-sky outputs (rrtmg_hip_set_lw_clear_sky): the same library, setting 1 (the
default path) against setting 0, interleaved.  Per row: the device-event time of one device-resident longwave call and the
cloudy solve kernel's own event brackets summed over the call's chunks (rrtmg_hip_kernel_ms, which = 3; the cloud-free
variant's, which = 1, beside it where the grid has such tiles), each the median of the alternations after two warm-up rounds,
with the raw lists behind.  Writes the table to stdout (profiles/lw_allsky_only_ab.txt is its output).

    python tools/lw_allsky_only_ab.py [--alternations 6] [--rows cloudy,shard,mixed,rtrnmr]
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from climt_amd import _hip  # noqa: E402
from climt_amd._lib import LIB_PATH, LW_OUT, LW_OUT_CLEAR, Context, source_hash  # noqa: E402
from climt_amd.synthetic import make_columns  # noqa: E402
from oracle.ref_driver import CONSTANTS, CPDAIR  # noqa: E402

BASE = dict(iaer=0, inflg=2, iceflg=1, liqflg=1, irng=0, permuteseed=5)
# name -> (columns, layers, McICA, icld, every fourth tile cloud-free, shard of)
ROWS = {
    "cloudy": (8192, 60, True, 2, False, 0),             # bench.py --cloudy: 8192 x 60, McICA
    "shard": (16384, 60, True, 2, False, 131072),        # BASELINE config 4: one of eight shards of 512 x 256
    "mixed": (8192, 60, True, 2, True, 0),
    "rtrnmr": (8192, 60, False, 2, False, 0),            # non-McICA maximum / random overlap (MR = true)
}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--alternations", type=int, default=6)
    ap.add_argument("--rows", default=",".join(ROWS))
    args = ap.parse_args()
    if args.alternations < 6:
        ap.error("at least 6 alternations")
    ctx = Context(0)
    ctx.set_constants(**CONSTANTS)
    ctx.lw_init(CPDAIR)
    print("# longwave clear-sky outputs, setting 1 against 0, %d alternations after 2 warm-up rounds, medians (ms); lw: HIP events around one"
          " device-resident call; solve: the cloudy solve kernel's event brackets of that call, summed over its chunks (rrtmg_hip_kernel_ms,"
          " which = 3); free: the cloud-free variant's (which = 1); library %s src:%s" % (args.alternations, os.path.basename(LIB_PATH), source_hash()))
    print("# %-28s %9s %9s %7s %9s %9s %7s %9s %9s" % ("row", "lw 1", "lw 0", "0/1", "solve 1", "solve 0", "0/1", "free 1", "free 0"))
    for name in args.rows.split(","):
        n, nlay, mcica, icld, mixed, shard_of = ROWS[name]
        c = make_columns(n, nlay, cloudy=True, seed=9)
        c.pop("lat")
        c.update(BASE)
        c["icld"] = icld
        if mixed:
            for t in range(0, n // 64, 4):
                for k in ("cldfr", "cliqwp", "cicewp"):
                    c[k][:, t * 64:(t + 1) * 64] = 0.0
        if shard_of:
            c.update(shard_col0=0, shard_ncol=shard_of)
        dev = {k: _hip.DeviceArray.from_host(v) for k, v in c.items() if isinstance(v, np.ndarray)}
        inp = {k: v.ptr for k, v in dev.items()}
        inp.update({k: v for k, v in c.items() if not isinstance(v, np.ndarray)})
        inp.update(ncol=n, nlay=nlay)
        lo = {k: _hip.DeviceArray((nlay + lev, n)) for k, lev in LW_OUT}
        keep = list(dev.values()) + list(lo.values())
        lptr = {k: v.ptr for k, v in lo.items()}
        e0, e1 = _hip.Event(), _hip.Event()
        t = {(k, on): [] for k in ("lw", "solve", "free") for on in (True, False)}

        def lw_call(on):
            ctx.set_lw_clear_sky(on)
            out = lptr if on else {k: v for k, v in lptr.items() if k not in LW_OUT_CLEAR}
            e0.record(ctx.stream)
            ctx.lw_fluxes(inp, mcica=mcica, out=out, memspace=1)
            e1.record(ctx.stream)
            e1.synchronize()
            t[("lw", on)].append(e0.elapsed_ms(e1))
            for key, cl in (("solve", True), ("free", False)):
                if ctx.kernel_launches("lw", cloudy=cl) > 0:
                    t[(key, on)].append(ctx.kernel_ms("lw", cloudy=cl))

        for on in (True, False, True, False):      # warm-up: buffers, code objects, chunk plans
            lw_call(on)
        for v in t.values():
            del v[:]
        for _ in range(args.alternations):
            for on in (True, False):
                lw_call(on)
        ctx.set_lw_clear_sky(True)
        med = lambda v: float(np.median(v)) if v else float("nan")
        m = {k: med(v) for k, v in t.items()}
        print("  %-28s %9.3f %9.3f %7.3f %9.3f %9.3f %7.3f %9.3f %9.3f   (%s)" % (
            "%s %dx%d %s icld %d" % (name, n, nlay, "McICA" if mcica else "no McICA", icld),
            m[("lw", True)], m[("lw", False)], m[("lw", False)] / m[("lw", True)], m[("solve", True)], m[("solve", False)],
            m[("solve", False)] / m[("solve", True)], m[("free", True)], m[("free", False)],
            " | ".join("%s %d " % (k, on) + " ".join("%.3f" % x for x in v) for (k, on), v in t.items() if v)))
        sys.stdout.flush()
        for v in keep:
            v.free()
    ctx.close()


if __name__ == "__main__":
    main()
