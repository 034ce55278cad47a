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
