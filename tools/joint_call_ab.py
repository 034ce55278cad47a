"""What a host caller gains from the joint shortwave + longwave call: (a) the two separate calls against (b) the one joint call,
on the same library and the same state, interleaved.  Host clock around each side; two warm-up rounds, then --alternations
rounds of (a), (b); medians, with the raw lists beside them.

Rows: an unmodified model script on a host state -- sw(state); lw(state) against climt_amd.radiation_step(sw, lw, state) -- at
128 x 64 x 60 clear sky, the same with McICA (kissvec) and 512 x 256 x 60 McICA; and a C-ABI caller with its own pageable
output arrays at 8192 x 60 -- Context.sw_fluxes; lw_fluxes against Context.radiation_fluxes.  Beside each row: radiation_last()
of the joint call (arrays shared, MB uploaded, MB not uploaded) and the solve kernels' event times (rrtmg_hip_kernel_ms, summed
over the variants that ran) on both sides: the kernels are the same, and inside the joint call they share the GPU.
Writes the table to stdout (profiles/joint_call_ab.txt is its output).

    python tools/joint_call_ab.py [--alternations 6] [--rows clear128,mcica128,mcica512,cabi8192]
"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import climt_amd  # noqa: E402
from climt_amd._lib import LW_OUT, SW_OUT, source_hash  # noqa: E402
from climt_amd.rrtmg.common import make_context  # noqa: E402
from climt_amd.synthetic import make_columns  # noqa: E402

# name -> (kind, nx, ny, layers, McICA)
ROWS = {
    "clear128": ("state", 128, 64, 60, False),
    "mcica128": ("state", 128, 64, 60, True),
    "mcica512": ("state", 512, 256, 60, True),
    "cabi8192": ("cabi", 8192, 1, 60, False),
}


def solve_ms(ctx, which):
    return sum(ctx.kernel_ms(which, cloudy=cl) for cl in (False, True) if ctx.kernel_launches(which, cloudy=cl) > 0)


def state_row(nx, ny, nz, mcica):
    kw = dict(mcica=True, random_number_generator="kissvec") if mcica else {}
    sw, lw = climt_amd.RRTMGShortwave(**kw), climt_amd.RRTMGLongwave(allow_synthetic_tables=True, **kw)
    state = climt_amd.get_default_state([sw, lw], grid_state=climt_amd.get_grid(nx=nx, ny=ny, nz=nz))
    if mcica:      # a cloud deck over every third column, so that both solve variants run
        frac = state["cloud_area_fraction_in_atmosphere_layer"].values
        frac[8:20, :, ::3] = 0.5
        state["mass_content_of_cloud_liquid_water_in_atmosphere_layer"].values[8:20, :, ::3] = 0.03
    keep = {}

    def separate():
        keep["a"] = (sw(state), lw(state))

    def joint():
        keep["b"] = climt_amd.radiation_step(sw, lw, state)
    return sw._ctx, separate, joint


def cabi_row(ncol, nlay):
    ctx = make_context(0)
    c = make_columns(ncol, nlay, cloudy=False, seed=9)
    c.pop("lat")
    c.update(icld=0, iaer=0, adjes=1.0, dyofyr=1, scon=1367.0, isolvar=0, inflg=2, iceflg=1, liqflg=1)
    # caller-owned pageable outputs, allocated once and written by every call (as a C host's arrays are)
    so = {k: np.zeros((nlay + lev, ncol)) for k, lev in SW_OUT}
    lo = {k: np.zeros((nlay + lev, ncol)) for k, lev in LW_OUT}

    def separate():
        ctx.sw_fluxes(c, out=so)
        ctx.lw_fluxes(c, out=lo)

    def joint():
        ctx.radiation_fluxes(sw=dict(inp=c, out=so), lw=dict(inp=c, out=lo))
    return ctx, separate, joint


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--alternations", type=int, default=6)
    ap.add_argument("--rows", default=",".join(ROWS))
    args = ap.parse_args()
    print("# joint SW+LW host call: (a) separate calls against (b) one joint call, host clock, 2 warm-up rounds + %d alternations, medians (ms);"
          " shared / MB up / MB saved: radiation_last() of (b); solve: rrtmg_hip_kernel_ms of the solve kernels, sw + lw, after (a) and after (b);"
          " library src:%s" % (args.alternations, source_hash()))
    print("# %-28s %9s %9s %7s %7s %7s %8s %10s %10s" % ("row", "(a) sep", "(b) joint", "b/a", "shared", "MB up", "MB saved", "solve (a)", "solve (b)"))
    for name in args.rows.split(","):
        kind, nx, ny, nz, mcica = ROWS[name]
        ctx, separate, joint = state_row(nx, ny, nz, mcica) if kind == "state" else cabi_row(nx * ny, nz)
        t = {"a": [], "b": []}
        solve = {"a": [], "b": []}
        for r in range(2 + args.alternations):
            for side, fn in (("a", separate), ("b", joint)):
                np.random.seed(11)
                t0 = time.perf_counter()
                fn()
                dt = (time.perf_counter() - t0) * 1.0e3
                if r >= 2:
                    t[side].append(dt)
                    solve[side].append((solve_ms(ctx, "sw"), solve_ms(ctx, "lw")))
        shared, up, saved = ctx.radiation_last()
        a, b = float(np.median(t["a"])), float(np.median(t["b"]))
        sa, sb = np.median(np.array(solve["a"]), axis=0), np.median(np.array(solve["b"]), axis=0)
        print("  %-28s %9.3f %9.3f %7.3f %7d %7.1f %8.1f %10s %10s   (%s)" % (
            "%s %dx%dx%d %s" % (name, nx, ny, nz, "McICA" if mcica else "clear"), a, b, b / a, shared, up / 1.0e6, saved / 1.0e6,
            "%.2f+%.2f" % tuple(sa), "%.2f+%.2f" % tuple(sb),
            " | ".join("%s " % k + " ".join("%.3f" % x for x in v) for k, v in t.items())))
        sys.stdout.flush()


if __name__ == "__main__":
    main()
