"""The longwave between radiation calls, stated in numpy (TEST INFRASTRUCTURE ONLY): the rule of rrtmg_hip_lw_adjust_surface
(include/rrtmg_hip.h, climt_amd/csrc/rrtmg_lw_adjust.h) with the product and the sum as separate numpy operations -- every one
rounded on its own, as the library's statement is -- and seeded inputs for it."""
import numpy as np

CHUNK = 8      # kLwAdjustChunk: the layers of one thread's block (tests/test_lw_adjust.py checks it against the header)


def adjust(tsfc_call, tsfc_now, plev, uflx, dflx, duflx_dt, heatfac, pressure_scale=0.0):
    """One stream: [nlay+1][ncol] arrays -> (uflx' [nlay+1][ncol], hr' [nlay][ncol])."""
    dT = tsfc_now - tsfc_call
    change = duflx_dt * dT[None, :]
    up = uflx + change
    net = up - dflx
    p = plev * pressure_scale if pressure_scale != 0.0 else plev
    dp = p[:-1] - p[1:]
    dnet = net[:-1] - net[1:]
    scaled = heatfac * dnet
    return up, scaled / dp


HEATFAC = 9.80665 * 86400.0 / (1004.64 * 1.e2)      # rrtmg_tables.cpp: grav * secdy / (cpdair * 1.e2) with the tests' constants


def case(ncol, nlay, seed=0, pascal=False):
    """Seeded inputs: fluxes of O(100) W m^-2, derivatives in [0, 6], dT in [-3, 3] with exact zeros in some columns, monotone
    plev (mbar, or Pa for pressure_scale = 0.01) -> dict of float64 arrays, [nlay+1][ncol] and [ncol]."""
    rng = np.random.default_rng(1000 * nlay + ncol + 7919 * seed)
    il = (nlay + 1, ncol)
    c = {}
    c["tsfc_call"] = rng.uniform(250.0, 310.0, ncol)
    dT = rng.uniform(-3.0, 3.0, ncol)
    dT[::3] = 0.0
    c["tsfc_now"] = c["tsfc_call"] + dT
    c["tsfc_now"][::3] = c["tsfc_call"][::3]
    steps = rng.uniform(0.5, 1.5, il)
    steps[0] = 0.0
    p = 1013.0 * (1.0 - 0.999 * np.cumsum(steps, axis=0) / np.sum(steps, axis=0))      # strictly decreasing, 1013 -> ~1 mbar
    c["plev"] = p * 100.0 if pascal else p
    for k, (lo, hi) in (("uflx", (150.0, 450.0)), ("dflx", (0.0, 400.0)), ("uflxc", (150.0, 450.0)), ("dflxc", (0.0, 400.0))):
        c[k] = rng.uniform(lo, hi, il)
    for k in ("duflx_dt", "duflxc_dt"):
        c[k] = rng.uniform(0.0, 6.0, il)
    return c


def want(c, clear=True, heatfac=HEATFAC, pressure_scale=0.0):
    """-> {"uflx", "hr"[, "uflxc", "hrc"]} of the numpy statement."""
    out = {}
    out["uflx"], out["hr"] = adjust(c["tsfc_call"], c["tsfc_now"], c["plev"], c["uflx"], c["dflx"], c["duflx_dt"], heatfac, pressure_scale)
    if clear:
        out["uflxc"], out["hrc"] = adjust(c["tsfc_call"], c["tsfc_now"], c["plev"], c["uflxc"], c["dflxc"], c["duflxc_dt"], heatfac, pressure_scale)
    return out


# ---- real longwave states: the flux call with idrv = 1, then the adjustment -----------------------------------------------------------
NCOL = 136
STATES = {"clear_L60": (False, 60), "clear_L5": (False, 5), "mcica_L60": (True, 60), "mcica_L5": (True, 5)}
STREAMS = (("uflx", "dflx", "duflx_dt", "hr"), ("uflxc", "dflxc", "duflxc_dt", "hrc"))


def flux_state(name):
    """-> (inputs of Context.lw_fluxes with idrv = 1 and an EXPLICIT tlev, mcica flag): 136 columns of climt_amd.synthetic, clear
    sky, or broken cloud decks under McICA (kissvec, a fixed seed: the same mask in every call)."""
    from climt_amd.synthetic import make_columns
    mcica, nlay = STATES[name]
    c = make_columns(NCOL, nlay, cloudy=mcica, seed=31 + nlay)
    c.update(icld=1, inflg=2, iceflg=1, liqflg=1, idrv=1)
    if mcica:
        c.update(irng=0, permuteseed=684)
        assert (c["cldfr"] > 0).any()
    assert c["tlev"] is not None
    return c, mcica


def surface_change(ncol=NCOL):
    """Per-column dT in [-3, 3] K: every fourth column exactly 0, the others at least 0.5 K in size for two in three."""
    rng = np.random.default_rng(2015)
    dT = rng.uniform(-3.0, 3.0, ncol)
    dT[::4] = 0.0
    return dT


def first_order_ratios(base, full, adjusted, dT):
    """The inequality of the first-order test, per quantity: for the columns with |dT| >= 0.5 K, the maximum over levels of
    |adjusted - full(tsfc + dT)| against that of |unadjusted - full(tsfc + dT)| -> {name: (errors [ncol'], references [ncol'])}."""
    big = np.abs(dT) >= 0.5
    out = {}
    for k in ("uflx", "uflxc", "hr", "hrc"):
        if k in adjusted:
            out[k] = (np.abs(adjusted[k] - full[k])[:, big].max(axis=0), np.abs(base[k] - full[k])[:, big].max(axis=0))
    return out


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def same_bits(got, want_):
    got, want_ = np.asarray(got), np.asarray(want_)
    return got.shape == want_.shape and np.array_equal(bits(got), bits(want_))
