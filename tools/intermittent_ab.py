#!/usr/bin/env python3
"""The shortwave between radiation calls (climt_amd.IntermittentShortwave): what a step costs, and what it buys.

    python tools/intermittent_ab.py [--ncol 8192] [--nlay 60] [--pairs 15] [--skip-accuracy]

A/B timing, device pointers, synchronous calls, the two sides alternated on one GPU:
  (a) an in-between step -- rrtmg_hip_mean_coszen of the step plus ONE rrtmg_hip_scale_columns launch over the six default
      outputs -- against a full shortwave call;
  (b) an update step -- mean_coszen of the update interval and of the step, the shortwave call, the scale launch -- against the
      plain shortwave call: the difference is the small kernels.
Accuracy: 24 hours on one latitude circle (the equator, 128 longitudes), model step 30 min, update interval 3 h: the daily-mean
surface downward shortwave of (1) UpdateFrequencyWrapper with the zenith angle of the call's instant, (2) the interval-mean
zenith angle alone, held between calls, (3) IntermittentShortwave (mean zenith and rescale), each against the shortwave called
at every step with the step-mean zenith angle."""
import argparse
import datetime
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def timing(a):
    from climt_amd import _hip
    from climt_amd._lib import Context
    from climt_amd.rrtmg.common import physical_constants
    from climt_amd.synthetic import make_columns
    ctx = Context(0)
    ctx.set_constants(**physical_constants())
    ctx.sw_init(1004.64)
    c = make_columns(a.ncol, a.nlay, cloudy=False, seed=7); c.pop("lat", None)
    c.update(icld=0, iaer=0, adjes=1.0, dyofyr=80, scon=1367.0, isolvar=0, inflg=2, iceflg=1, liqflg=1)
    nlay, ncol = c["play"].shape
    dev = {k: _hip.DeviceArray.from_host(v) for k, v in c.items() if isinstance(v, np.ndarray)}
    lat = _hip.DeviceArray.from_host(np.degrees(np.arcsin(np.linspace(-0.98, 0.98, ncol))))
    lon = _hip.DeviceArray.from_host(np.mod(137.5 * np.arange(ncol), 360.0))
    col = {k: _hip.DeviceArray((ncol,)) for k in ("mu_rad", "f_rad", "zen_rad", "mu_step", "f_step", "ins_step")}
    names = ("swuflx", "swdflx", "swhr", "swuflxc", "swdflxc", "swhrc")
    rows = {k: nlay + (0 if k.endswith(("hr", "hrc")) else 1) for k in names}
    kept = {k: _hip.DeviceArray((rows[k], ncol)) for k in names}
    scaled = {k: _hip.DeviceArray((rows[k], ncol)) for k in names}
    args = {k: v for k, v in c.items() if k not in dev}
    args.update({k: v.ptr for k, v in dev.items()}); args.update(ncol=ncol, nlay=nlay)
    t0 = 0.2 + 4.0 / 24.0 / 36525.0
    t_rad, t_step = t0 + 3.0 / 24.0 / 36525.0, t0 + 0.5 / 24.0 / 36525.0

    def sun(t1, prefix, zenith):
        ctx.mean_coszen(lat.ptr, lon.ptr, t0, t1, out_mean=col["mu_" + prefix].ptr, out_fraction=col["f_" + prefix].ptr, memspace=1, ncol=ncol,
                        out_zenith=col["zen_rad"].ptr if zenith else None, out_insolation=col["ins_step"].ptr if not zenith else None)

    def shortwave():
        ctx.sw_fluxes(args, mcica=False, out={k: v.ptr for k, v in kept.items()}, memspace=1)

    def scale():
        ctx.scale_columns(col["ins_step"], col["mu_rad"], [(kept[k], scaled[k], rows[k]) for k in names])

    def between():
        sun(t_step, "step", False); scale()

    def update():
        sun(t_rad, "rad", True); shortwave(); sun(t_step, "step", False); scale()

    def timed(fn):
        ctx.synchronize()
        t = time.perf_counter()
        fn()
        ctx.synchronize()
        return (time.perf_counter() - t) * 1e3
    ctx.set_deferred(True)      # the calls of a side are enqueued back to back, one synchronise behind them
    for _ in range(3):
        timed(update); timed(shortwave); timed(between)
    t = {"between": [], "shortwave": [], "update": []}
    for _ in range(a.pairs):
        t["between"].append(timed(between)); t["shortwave"].append(timed(shortwave)); t["update"].append(timed(update))
    m = {k: float(np.median(v)) for k, v in t.items()}
    moved = sum(rows.values()) * ncol * 16
    print("intermittent_ab: %d columns x %d layers, clear sky, %d alternated triples, device pointers, deferred mode, one synchronise per side" % (ncol, nlay, a.pairs))
    print("(a) in-between step (mean_coszen + one scale launch, %d arrays, %.1f MB read + written): %7.3f ms   full shortwave call: %7.3f ms   ratio %.1f x   [min %.3f / %.3f]"
          % (len(names), moved / 1e6, m["between"], m["shortwave"], m["shortwave"] / m["between"], min(t["between"]), min(t["shortwave"])))
    print("(b) update step (2 x mean_coszen + shortwave + scale): %7.3f ms   plain shortwave call: %7.3f ms   difference %+7.3f ms (%+.1f %%)   [min %.3f / %.3f]"
          % (m["update"], m["shortwave"], m["update"] - m["shortwave"], 100.0 * (m["update"] - m["shortwave"]) / m["shortwave"], min(t["update"]), min(t["shortwave"])))
    ctx.set_deferred(False)
    ctx.close()


def accuracy():
    import climt_amd
    step, update = datetime.timedelta(minutes=30), datetime.timedelta(hours=3)
    start = datetime.datetime(2000, 3, 20, 0, 0)
    nsteps = 48
    sun = climt_amd.Instellation()

    def run(kind):
        sw = climt_amd.RRTMGShortwave()
        state = climt_amd.get_default_state([sun, sw], grid_state=climt_amd.get_grid(nx=128, ny=1, nz=28))
        wrapped = {"instant": climt_amd.UpdateFrequencyWrapper(sw, update), "intermittent": climt_amd.IntermittentShortwave(sw, sun, update)}.get(kind)
        total, held = 0.0, None
        for i in range(nsteps):
            state["time"] = start + i * step
            if kind == "every_step":
                state["zenith_angle"] = sun.interval_mean(state, step)["zenith_angle"]
                frac = sun.interval_mean(state, step)["sunlit_fraction"].values
                _, d = sw(state)
                down = d["downwelling_shortwave_flux_in_air"].values[0] * frac      # the sunlit mean holds for the sunlit part of the step
            elif kind == "instant":
                state.update(sun(state))
                _, d = wrapped(state)
                down = d["downwelling_shortwave_flux_in_air"].values[0]
            elif kind == "mean_only":
                if i % 6 == 0:
                    m = sun.interval_mean(state, update)
                    _, d = sw(dict(state, zenith_angle=m["zenith_angle"]))
                    held = d["downwelling_shortwave_flux_in_air"].values[0] * m["sunlit_fraction"].values
                down = held
            else:
                _, d = wrapped(state, step)
                down = d["downwelling_shortwave_flux_in_air"].values[0]
            total = total + np.asarray(down, dtype=np.float64)
        return (total / nsteps).ravel()
    ref = run("every_step")
    print("accuracy: equator, 128 longitudes, 24 h from %s, step 30 min, update 3 h; daily-mean surface downward shortwave, W m^-2" % start.isoformat())
    print("  reference (shortwave at every step, step-mean zenith angle): zonal mean %.3f, min %.3f, max %.3f" % (ref.mean(), ref.min(), ref.max()))
    for kind, label in (("instant", "UpdateFrequencyWrapper, zenith angle of the instant"), ("mean_only", "interval-mean zenith angle, held between calls"),
                        ("intermittent", "IntermittentShortwave: mean zenith and rescale")):
        d = run(kind) - ref
        print("  %-52s zonal-mean bias %+8.3f   rms over longitudes %7.3f   max |d| %7.3f" % (label + ":", d.mean(), float(np.sqrt((d * d).mean())), float(np.abs(d).max())))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ncol", type=int, default=8192)
    ap.add_argument("--nlay", type=int, default=60)
    ap.add_argument("--pairs", type=int, default=15)
    ap.add_argument("--skip-accuracy", action="store_true")
    a = ap.parse_args()
    timing(a)
    if not a.skip_accuracy:
        accuracy()


if __name__ == "__main__":
    main()
