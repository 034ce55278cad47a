"""What the shortwave's opt-in night-column skip (rrtmg_hip_set_sw_night_skip, RRTMGShortwave(skip_night_columns=True))
treats as night, stated in numpy: for callers who want to know what a grid saves, and for the tests of the kernels.

A night COLUMN has coszen <= 0 as the caller passes it (0.0 and -0.0 are night, NaN is not).  A night TILE is one of the 64
consecutive columns the solve kernels work on -- columns 64 t .. 64 t + 63 of the call, the last tile possibly shorter --
whose columns are all night.  Every night column gets zeros; only night tiles save work."""
import numpy as np

TILE = 64


def night_columns(coszen):
    """-> bool [ncol]: the columns whose outputs the skip sets to zero."""
    c = np.asarray(coszen, dtype=np.float64).ravel()
    with np.errstate(invalid="ignore"):
        return c <= 0.0


def night_tiles(coszen):
    """-> bool [ceil(ncol / 64)]: the tiles for which the skip does no work (every in-range column is night)."""
    n = night_columns(coszen)
    ntile = (n.size + TILE - 1) // TILE
    pad = np.ones(ntile * TILE, dtype=bool)
    pad[:n.size] = n
    return pad.reshape(ntile, TILE).all(axis=1)


def mixed_tiles(coszen):
    """-> bool [tiles]: tiles with night AND day columns: solved whole, their night columns zeroed afterwards."""
    n = night_columns(coszen)
    ntile = (n.size + TILE - 1) // TILE
    pad = np.zeros(ntile * TILE, dtype=bool)
    pad[:n.size] = n
    return pad.reshape(ntile, TILE).any(axis=1) & ~night_tiles(coszen)


def night_counts(coszen):
    """-> (night tiles, night columns): what rrtmg_hip_sw_night_last reports for a call with this coszen."""
    return int(night_tiles(coszen).sum()), int(night_columns(coszen).sum())


# ---- the day-column pack (rrtmg_hip_set_sw_night_pack, RRTMGShortwave(pack_day_columns=True)) ------------------------------
def packed_order(coszen):
    """-> (src, dst), int [64 * (ceil(ncol / 64) + 1)]: the internal copy a packed call runs on, slot by slot.
    src[slot]: the caller's column whose inputs the slot holds.  Slots [0, nday): the day columns in the caller's order;
    [nday, ndpad), ndpad = 64 * ceil(nday / 64): replicas of the last day column; [ndpad, ndpad + nnight): the night columns in
    the caller's order (only their coszen is copied); behind them filler slots, src -1 (coszen 0.0).
    dst[slot]: the caller's column the slot's outputs are scattered to (a night column's as +0.0), -1 for replica and filler
    slots.  Every caller's column appears in dst exactly once, and no 64-slot tile holds both day and night columns."""
    night = night_columns(coszen)
    n = night.size
    day_cols, night_cols = np.flatnonzero(~night), np.flatnonzero(night)
    nday = day_cols.size
    ndpad = (nday + TILE - 1) // TILE * TILE
    npad = ((n + TILE - 1) // TILE + 1) * TILE
    src = np.full(npad, -1, dtype=np.int64)
    dst = np.full(npad, -1, dtype=np.int64)
    src[:nday] = day_cols
    dst[:nday] = day_cols
    if nday:
        src[nday:ndpad] = day_cols[-1]
    src[ndpad:ndpad + night_cols.size] = night_cols
    dst[ndpad:ndpad + night_cols.size] = night_cols
    return src, dst


def packed_counts(coszen):
    """-> (night tiles, night columns): what rrtmg_hip_sw_night_last reports after a PACKED call with this coszen: the tiles'
    worth of solve work not done, ceil(ncol / 64) - ceil(nday / 64), and ncol - nday."""
    night = night_columns(coszen)
    n, nday = night.size, int((~night).sum())
    return (n + TILE - 1) // TILE - (nday + TILE - 1) // TILE, n - nday
