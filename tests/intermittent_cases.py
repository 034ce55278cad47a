"""The shortwave between radiation calls: the numpy statement of the definition (include/rrtmg_hip.h, rrtmg_hip_mean_coszen and
rrtmg_hip_scale_columns), the 320 columns and the four intervals the CPU and the GPU tests hold the kernels against, and the
tolerances.  Importing the module asserts, with numpy alone, that the inputs hit every branch of the column function and that
the filter of the separately compared outputs drops few columns -- the inputs cannot silently stop covering a branch."""
import datetime

import numpy as np

from oracle.instellation_oracle import days_from_2000, sun_position

PI = np.pi
TWO_PI = 2.0 * np.pi

# |difference| of the interval-mean insolation factor I / D = coszen_mean * sunlit_fraction.  The integrand vanishes at the
# sunlit boundary, so I is insensitive to the rounding of H; its terms are O(1) with a few ulp each, and the division by
# D >= 4e-3 (60 s) amplifies 2e-16 to at most 1e-13.
TOL_INSOLATION = 1.0e-12
# ... of sunlit_fraction and coszen_mean on their own: first order in the error of H = acos(x), unbounded as |x| -> 1, so they
# are compared only where the numpy statement has |x| <= 1 - 1e-6 (dH <= a few ulp / 1.4e-3) or clamps x outright.
TOL_SEPARATE = 1.0e-11
FILTER_EDGE = 1.0 - 1.0e-6
FILTER_MAX_DROPPED = 0.05


# ---- the definition ----------------------------------------------------------------------------------------------------------
def centuries(time):
    return days_from_2000(time) / 36525.0


def interval_sun(t0, t1):
    """(sin_dec, cos_dec, g0, D) of the interval [t0, t1] in Julian centuries: declination of the midpoint, hour angle of
    Greenwich at t0, its advance to t1 in (0, 2 pi)."""
    _, ra0, gmst0 = sun_position(t0)
    _, ra1, gmst1 = sun_position(t1)
    dec, _, _ = sun_position(0.5 * (t0 + t1))
    g0 = gmst0 - ra0
    d = float(np.fmod((gmst1 - ra1) - g0, TWO_PI))
    if d <= 0:
        d += TWO_PI
    return float(np.sin(dec)), float(np.cos(dec)), float(g0), d


def mean_coszen(lat_deg, lon_deg, sun):
    """The numpy statement: a dict with mean, fraction, insolation (I / D) and what the branch assertions look at."""
    sin_dec, cos_dec, g0, D = sun
    lat_deg, lon_deg = np.asarray(lat_deg, dtype=np.float64), np.asarray(lon_deg, dtype=np.float64)
    lat = lat_deg * (PI / 180.0)
    cos_lat = np.where(np.abs(lat_deg) == 90.0, 0.0, np.cos(lat))
    A, B = np.sin(lat) * sin_dec, cos_lat * cos_dec
    h0 = g0 + lon_deg * (PI / 180.0)
    h0 = h0 - TWO_PI * np.floor((h0 + PI) / TWO_PI)
    h0 = np.where(h0 >= PI, h0 - TWO_PI, np.where(h0 < -PI, h0 + TWO_PI, h0))
    h1 = h0 + D
    with np.errstate(divide="ignore", invalid="ignore"):
        x = np.where(B > 0.0, -A / np.where(B > 0.0, B, 1.0), np.where(A > 0.0, -np.inf, np.inf))
    H = np.where(B > 0.0, np.arccos(np.clip(x, -1.0, 1.0)), np.where(A > 0.0, PI, 0.0))
    S, I, pieces = np.zeros_like(lat), np.zeros_like(lat), np.zeros(lat.shape, dtype=int)
    for k in (-1, 0, 1):
        c = TWO_PI * k
        a, b = np.maximum(h0, c - H), np.minimum(h1, c + H)
        on = b > a
        S = np.where(on, S + (b - a), S)
        I = np.where(on, I + (A * (b - a) + B * (np.sin(b) - np.sin(a))), I)
        pieces += on
    with np.errstate(divide="ignore", invalid="ignore"):
        mean = np.clip(np.where(S > 0.0, I / np.where(S > 0.0, S, 1.0), 0.0), 0.0, 1.0)
    return dict(mean=mean, fraction=S / D, insolation=I / D, A=A, B=B, x=x, H=H, h0=h0, h1=h1, S=S, pieces=pieces, D=D)


def separately_comparable(want):
    """Where sunlit_fraction and coszen_mean are compared on their own: the numpy statement alone decides."""
    ax = np.abs(want["x"])
    return (ax <= FILTER_EDGE) | (ax > 1.0)


def check_mean_coszen(got_mean, got_fraction, want, what=""):
    """The three comparisons of a kernel's (or the host program's) output with the numpy statement -> the measured maxima."""
    d_ins = float(np.abs(got_mean * got_fraction - want["insolation"]).max())
    keep = separately_comparable(want)
    d_frac = float(np.abs(got_fraction - want["fraction"])[keep].max())
    d_mean = float(np.abs(got_mean - want["mean"])[keep].max())
    print("%s max |d insolation| = %.3e   max |d fraction| = %.3e   max |d mean| = %.3e   (%d of %d columns compared separately)"
          % (what, d_ins, d_frac, d_mean, int(keep.sum()), keep.size))
    assert np.all((got_mean >= 0.0) & (got_mean <= 1.0)), what
    assert d_ins <= TOL_INSOLATION, (what, d_ins)
    assert d_frac <= TOL_SEPARATE, (what, d_frac)
    assert d_mean <= TOL_SEPARATE, (what, d_mean)
    return d_ins, d_frac, d_mean


def scale_columns(src, num, den):
    """dst = src * s, s = den > 0 ? num / den : +0.0 by column (the last axis); s = 0 writes +0.0 whatever src holds."""
    with np.errstate(divide="ignore", invalid="ignore"):
        s = np.where(den > 0.0, num / np.where(den > 0.0, den, 1.0), 0.0)
        return np.where(s == 0.0, 0.0, src * s)


def scale_factor(num, den):
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(den > 0.0, num / np.where(den > 0.0, den, 1.0), 0.0)


# ---- the inputs: 320 columns (a 256-thread block and a ragged one), four intervals from one start ------------------------------------
NCOL = 320
T0 = datetime.datetime(2000, 6, 21, 3, 17, 0)
INTERVALS = {"3h": 10800.0, "12h": 43200.0, "30min": 1800.0, "60s": 60.0}


def interval_centuries(name):
    return centuries(T0), centuries(T0 + datetime.timedelta(seconds=INTERVALS[name]))


def _columns():
    """8 latitude circles of 40 longitudes: the poles exactly, polar day and polar night of the June solstice, the latitude of
    a night shorter than three hours, and four ordinary ones; then a few columns set by hand (below)."""
    lats = np.array([90.0, -90.0, 80.0, -80.0, 66.0, 40.0, 0.0, -45.0])
    lons = 4.5 + 9.0 * np.arange(40)
    lat, lon = np.repeat(lats, 40), np.tile(lons, 8)
    sin_dec, cos_dec, g0, _ = interval_sun(*interval_centuries("3h"))
    # h0 within one ulp of -pi (row of latitude 40): the longitude nearest to -pi - g0, then its neighbours in double precision
    target = np.fmod(-PI - g0, TWO_PI) * (180.0 / PI)
    best = None
    cand = target
    for _ in range(64):
        cand = np.nextafter(cand, -np.inf)
    for _ in range(128):
        h0 = mean_coszen(np.array([40.0]), np.array([cand]), (sin_dec, cos_dec, g0, 1.0))["h0"][0]
        err = abs(h0 + PI)
        if best is None or err < best[0]:
            best = (err, cand)
        cand = np.nextafter(cand, np.inf)
    lon[5 * 40 + 0] = best[1]
    # a sunset in the middle of the 60-second interval, on the equator (x = 0: H = pi/2, the best-conditioned acos)
    d60 = interval_sun(*interval_centuries("60s"))[3]
    lon[6 * 40 + 0] = (PI / 2.0 - 0.5 * d60 - g0) * (180.0 / PI)
    # ... and a sunrise there
    lon[6 * 40 + 1] = (-PI / 2.0 - 0.5 * d60 - g0) * (180.0 / PI)
    # two columns just inside the band the filter drops (|x| within 1e-6 of 1, x unclamped), for the 3-hour interval's declination
    tan_dec = sin_dec / cos_dec
    lat[4 * 40 + 0] = np.degrees(np.arctan((1.0 - 1.0e-8) / tan_dec))
    lat[4 * 40 + 1] = -np.degrees(np.arctan((1.0 - 1.0e-7) / tan_dec))
    return lat, lon


LAT, LON = _columns()


def _assert_coverage():
    assert LAT.size == LON.size == NCOL and NCOL > 256 and NCOL % 256 != 0
    w = {name: mean_coszen(LAT, LON, interval_sun(*interval_centuries(name))) for name in INTERVALS}
    every = lambda key: np.concatenate([w[n][key] for n in INTERVALS])
    x, B, H, S, D = every("x"), every("B"), every("H"), every("S"), np.concatenate([np.full(NCOL, w[n]["D"]) for n in INTERVALS])
    h0, h1, pieces, frac = every("h0"), every("h1"), every("pieces"), every("fraction")
    assert np.any((B == 0.0) & (H == PI)) and np.any((B == 0.0) & (H == 0.0))            # the poles exactly, both
    assert np.any((B > 0.0) & (x < -1.0)) and np.any((B > 0.0) & (x > 1.0))              # polar day, polar night
    unclamped = (B > 0.0) & (np.abs(x) < 1.0)
    assert np.any(unclamped & (frac == 1.0) & (pieces == 1))                              # wholly in daylight
    assert np.any(unclamped & (S == 0.0))                                                 # wholly at night
    inside = lambda edge: (edge > h0) & (edge < h1)
    rise = inside(-H) | inside(TWO_PI - H)
    sets = inside(H) | inside(TWO_PI + H)
    assert np.any(unclamped & rise & ~sets) and np.any(unclamped & sets & ~rise)          # sunrise only, sunset only
    assert np.any(unclamped & (pieces == 2) & (H < PI) & sets & rise)                     # a whole short night: two sunlit pieces
    assert np.any(np.abs(h0 + PI) <= 2.0 ** -51)                                          # h0 within one ulp of -pi
    assert np.any(h1 > PI) and np.any((h1 > PI) & (S > 0.0) & (H < PI))                   # h1 wraps past pi, into the next day's window
    assert abs(w["12h"]["D"] - PI) < 0.02 and abs(w["60s"]["D"] - TWO_PI * 60.0 / 86400.0) < 1e-5
    s60 = w["60s"]
    assert np.any((s60["fraction"] > 0.2) & (s60["fraction"] < 0.8))                      # a terminator inside the 60 seconds
    for name in INTERVALS:
        keep = separately_comparable(w[name])
        assert 1.0 - keep.mean() <= FILTER_MAX_DROPPED, (name, keep.mean())
    assert not separately_comparable(w["3h"]).all()                                       # the filter does drop something
    return w


WANT = _assert_coverage()


# ---- arrays for the rescale: 130 x 6, three tiles with a ragged last one -----------------------------------------------------------
def scale_case(ncol=130, nlay=6, seed=5):
    """-> (num, den, [4 arrays [nlay+1][ncol], 2 arrays [nlay][ncol]]): den = 0 and num = 0 columns, a negative zero, a NaN
    and an infinity in src (in columns whose factor is 0 they must come back +0.0)."""
    rng = np.random.default_rng(seed)
    num, den = rng.uniform(0.0, 1.0, ncol), rng.uniform(0.05, 1.0, ncol)
    den[[3, 64, ncol - 1]] = 0.0
    num[[5, 65]] = 0.0
    num[7] = -0.0
    den[9] = -0.5
    arrays = [rng.uniform(-50.0, 900.0, (nlay + 1, ncol)) for _ in range(4)] + [rng.uniform(-2.0, 30.0, (nlay, ncol)) for _ in range(2)]
    arrays[0][2, 11] = -0.0
    arrays[1][0, 3] = np.nan
    arrays[1][1, 64] = -np.inf
    arrays[2][3, 5] = -123.0
    arrays[4][nlay - 1, ncol - 1] = -1.0
    return num, den, arrays
