"""Exponential (icld 4) and exponential-random (icld 5) McICA overlap: the numpy statement of the definition in
include/rrtmg_hip.h (rrtmg_hip_set_mcica_overlap_alpha), from RAW generator draws, and the inputs the tests share.  Nothing here
calls the library: tests/test_exp_overlap.py and tests/test_exp_overlap_gpu.py compare the library with it, bit for bit."""
import numpy as np

CLDMIN = 1.0e-20
NSUB = {"sw": 112, "lw": 140}
# (columns, layers): one mask word, two mask words
SHAPES = ((70, 33), (70, 70))
ALPHA_KINDS = ("zero", "two", "random")


# ---- raw draws ---------------------------------------------------------------------------------------------------------------
def kiss_draws(play, n):
    """The first n real numbers of every column's kissvec stream, [n][ncol]: seeds from the fractional digits of the four lowest
    mid-layer pressures (hPa * 100), the four component generators, kiss * 2.328306e-10 + 0.5."""
    p = np.asarray(play[:4], dtype=np.float64) * 1.0e2
    seeds = ((p - np.trunc(p)) * 1000000000.0).astype(np.int64).astype(np.uint32)
    a, b, c, e = (seeds[i].copy() for i in range(4))
    out = np.empty((n, p.shape[1]))
    u = np.uint32
    for i in range(n):
        a = a * u(69069) + u(1327217885)
        b = b ^ (b << u(13)); b = b ^ (b >> u(17)); b = b ^ (b << u(5))
        c = u(18000) * (c & u(65535)) + (c >> u(16))
        e = u(30903) * (e & u(65535)) + (e >> u(16))
        kiss = (a + b + (c << u(16)) + e).view(np.int32)
        out[i] = kiss.astype(np.float64) * 2.328306e-10 + 0.5
    return out


def mt_words(seed, n):
    """The first n tempered 32-bit words of MT19937 seeded with one integer (init_genrand: numpy's legacy integer seeding)."""
    return np.random.RandomState(int(seed))._bit_generator.random_raw(int(n)).astype(np.uint32)


def mt_real(words):
    """getRandomReal of the reference: a word that is negative as a 32-bit integer goes through single precision."""
    li = np.asarray(words, dtype=np.uint32).view(np.int32)
    neg = (li.astype(np.float32) + np.float32(4294967296.0)).astype(np.float64) / 4294967295.0
    return np.where(li < 0, neg, li.astype(np.float64) / 4294967295.0)


# ---- the definition ----------------------------------------------------------------------------------------------------------
def exp_mask(x, y, cldfr, alpha, icld):
    """x, y [nsub][nlay][ncol]: the draws of every (sub-column, layer, column); -> mask bits, bool [nsub][nlay][ncol]."""
    assert icld in (4, 5)
    cf = np.where(cldfr < CLDMIN, 0.0, cldfr)
    nlay = cf.shape[0]
    bits = np.zeros(x.shape, dtype=bool)
    rank = x[:, 0]
    bits[:, 0] = rank >= 1.0 - cf[0]
    for l in range(1, nlay):
        a = alpha[l] if icld == 4 else np.where(cf[l - 1] == 0.0, 0.0, alpha[l])
        rank = np.where(y[:, l] < a, rank, x[:, l])
        bits[:, l] = rank >= 1.0 - cf[l]
    return bits


def kiss_exp_mask(draws, cldfr, alpha, icld, nsub, seed):
    """draws: kiss_draws(play, >= seed + nsub * 2 * nlay).  Sub-column g starts seed + g * 2 nlay draws into the column's stream."""
    nlay, ncol = cldfr.shape
    d = draws[seed:seed + nsub * 2 * nlay].reshape(nsub, nlay, 2, ncol)
    return exp_mask(d[:, :, 0], d[:, :, 1], cldfr, alpha, icld)


def mt_exp_mask(seed, cldfr, alpha, icld, nsub, col0=0, ncol_total=None):
    """The one Mersenne-twister stream, ordered (sub-column, column, layer, {x, y}); columns col0 .. of a grid of ncol_total."""
    nlay, ncol = cldfr.shape
    total = ncol if ncol_total is None else ncol_total
    r = mt_real(mt_words(seed, nsub * total * nlay * 2)).reshape(nsub, total, nlay, 2)[:, col0:col0 + ncol]
    return exp_mask(r[..., 0].transpose(0, 2, 1), r[..., 1].transpose(0, 2, 1), cldfr, alpha, icld)


def mt_random_mask(seed, cldfr, nsub):
    """icld 1 (random overlap) from the same raw words: pins mt_words / mt_real against the existing generator."""
    nlay, ncol = cldfr.shape
    cf = np.where(cldfr < CLDMIN, 0.0, cldfr)
    r = mt_real(mt_words(seed, nsub * ncol * nlay)).reshape(nsub, ncol, nlay).transpose(0, 2, 1)
    return r >= 1.0 - cf[None]


def as_cldfmcl(bits):
    """bool [nsub][nlay][ncol] -> the library's cldfmcl layout, doubles [nlay][ncol][nsub]."""
    return np.ascontiguousarray(bits.transpose(1, 2, 0)).astype(np.float64)


def unpack_words(words, nlay):
    """uint64 [nsub][nw][ncol] (bit l & 63 of word l >> 6) -> bool [nsub][nlay][ncol]."""
    l = np.arange(nlay)
    return ((words[:, l >> 6, :] >> (l & 63).astype(np.uint64)[None, :, None]) & np.uint64(1)).astype(bool)


# ---- inputs ------------------------------------------------------------------------------------------------------------------
def pressures(ncol, nlay, seed=3):
    from climt_amd.synthetic import make_columns
    c = make_columns(ncol, nlay, seed=seed)
    return np.ascontiguousarray(c["play"]), np.ascontiguousarray(c["tlay"])


def cloud_field(ncol, nlay, seed=11):
    """Cloud fractions in (0, 1) in blocks of layers separated by clear gaps (so that icld 4 and 5 differ), with a few values
    below cldmin (treated as 0), a few overcast cells and one column without any cloud."""
    rng = np.random.default_rng(seed)
    cf = rng.uniform(0.05, 0.95, (nlay, ncol))
    cf[rng.uniform(size=(nlay, ncol)) < 0.3] = 0.0
    cf[nlay // 3:nlay // 3 + 2] = 0.0
    cf[rng.uniform(size=(nlay, ncol)) < 0.03] = 1.0e-25
    cf[rng.uniform(size=(nlay, ncol)) < 0.03] = 1.0
    cf[:, 5] = 0.0
    return cf


def alpha_field(kind, ncol, nlay, seed=17):
    if kind == "zero":
        return np.zeros((nlay, ncol))
    if kind == "two":
        return np.full((nlay, ncol), 2.0)
    rng = np.random.default_rng(seed)
    return rng.uniform(0.02, 0.98, (nlay, ncol))


def overlap_alpha_numpy(play, tlay, length, rd_over_g):
    """rrtmg_hip_overlap_alpha, the same operations in the same order."""
    a = np.ones(play.shape)
    dz = rd_over_g * (0.5 * (tlay[1:] + tlay[:-1])) * np.log(play[:-1] / play[1:])
    a[1:] = np.exp(-dz / length)
    return a
