"""CPU tests of the numpy statements of the shortwave's day-column pack (climt_amd.night.packed_order / packed_counts:
rrtmg_hip_set_sw_night_pack, RRTMGShortwave(pack_day_columns=True)), checked by hand on tiny fields, and of the component's
constructor check.  The kernels are tested against these statements in tests/test_night_pack_gpu.py; the slot rule they use
(csrc/rrtmg_permute.h) is checked against the same hand-written fields by tools/permute_check.cpp, built and run here."""
import subprocess

import numpy as np
import pytest

from climt_amd import night
from helpers import build_host_program


def check_invariants(cz):
    """What holds for every field: the day columns in order in front, every caller's column exactly once in dst, no tile of
    the copy with both kinds, slots from ndpad on all night or filler."""
    cz = np.asarray(cz, dtype=np.float64)
    n = cz.size
    dark = night.night_columns(cz)
    nday = int((~dark).sum())
    ndpad = (nday + 63) // 64 * 64
    src, dst = night.packed_order(cz)
    assert src.shape == dst.shape == (64 * ((n + 63) // 64 + 1),)
    assert np.array_equal(src[:nday], np.flatnonzero(~dark)) and np.array_equal(dst[:nday], src[:nday])
    assert np.array_equal(np.sort(dst[dst >= 0]), np.arange(n))
    assert np.all(dst[nday:ndpad] == -1)
    if nday:
        assert np.all(src[nday:ndpad] == np.flatnonzero(~dark)[-1])
    tail = src[ndpad:]
    assert np.all((tail == -1) | dark[np.maximum(tail, 0)])
    nn = n - nday
    assert np.array_equal(tail[:nn], np.flatnonzero(dark)) and np.all(tail[nn:] == -1) and np.all(dst[ndpad + nn:] == -1)
    assert np.array_equal(dst[ndpad:ndpad + nn], tail[:nn])
    # no tile holds both kinds: a slot's kind is day in front of ndpad (replicas included), night or filler behind
    kind = np.arange(src.size) < ndpad
    assert np.all(kind.reshape(-1, 64).all(axis=1) | ~kind.reshape(-1, 64).any(axis=1))
    assert night.packed_counts(cz) == ((n + 63) // 64 - ndpad // 64, nn)
    return src, dst


def test_130_columns_with_3_day_columns():
    cz = np.full(130, -0.3)
    cz[[5, 70, 129]] = (0.2, 1.0e-300, 0.9)
    src, dst = check_invariants(cz)
    assert src.size == 256
    assert src[:3].tolist() == [5, 70, 129] and dst[:3].tolist() == [5, 70, 129]
    assert np.all(src[3:64] == 129) and np.all(dst[3:64] == -1)
    nights = [c for c in range(130) if c not in (5, 70, 129)]
    assert src[64:64 + 127].tolist() == nights and dst[64:64 + 127].tolist() == nights
    assert np.all(src[191:] == -1) and np.all(dst[191:] == -1)
    # three tiles of columns, one tile of solve work: two tiles' worth not done; the skip alone finds no night tile here
    assert night.packed_counts(cz) == (2, 127)
    assert night.night_counts(cz) == (0, 127)


def test_day_count_an_exact_multiple_of_64_has_no_replicas():
    cz = np.where(np.arange(200) % 3 == 0, 0.5, -0.5)      # 67 day columns ...
    cz[[0, 3, 6]] = 0.0                                   # ... less three: 64
    src, dst = check_invariants(cz)
    day = np.flatnonzero(cz > 0.0)
    assert day.size == 64
    assert np.array_equal(src[:64], day) and np.array_equal(dst[:64], day)
    assert src[64] == 0 and dst[64] == 0      # the first night column directly behind the day block: no replica slot
    assert not np.any((dst == -1) & (src >= 0))
    assert night.packed_counts(cz) == (4 - 1, 136)


def test_all_night_and_all_day():
    cz = np.linspace(-1.0, 0.0, 100)
    src, dst = check_invariants(cz)
    assert np.array_equal(src[:100], np.arange(100)) and np.array_equal(dst[:100], np.arange(100))
    assert np.all(src[100:] == -1) and src.size == 192
    assert night.packed_counts(cz) == (2, 100)
    cz = np.linspace(0.1, 1.0, 100)
    src, dst = check_invariants(cz)
    assert np.array_equal(src[:100], np.arange(100)) and np.all(src[100:128] == 99) and np.all(dst[100:128] == -1)
    assert np.all(src[128:] == -1) and np.all(dst[128:] == -1)
    assert night.packed_counts(cz) == (0, 0)


def test_negative_zero_is_night_and_nan_is_day():
    cz = np.array([0.3, -0.0, np.nan, 0.0, -1.0, 5.0e-324, np.nan])
    src, dst = check_invariants(cz)
    assert src[:4].tolist() == [0, 2, 5, 6]
    assert np.all(src[4:64] == 6)
    assert src[64:67].tolist() == [1, 3, 4] and dst[64:67].tolist() == [1, 3, 4]
    assert np.all(src[67:] == -1) and src.size == 128
    assert night.packed_counts(cz) == (0, 3)


@pytest.mark.parametrize("n, seed", [(1, 0), (63, 1), (64, 2), (65, 3), (128, 4), (500, 5), (641, 6)])
def test_invariants_on_random_fields(n, seed):
    rng = np.random.default_rng(seed)
    check_invariants(rng.uniform(-1.0, 1.0, n))
    check_invariants(np.where(rng.uniform(size=n) < 0.02, 0.5, -0.5))


def test_component_requires_the_skip():
    """pack_day_columns=True without skip_night_columns=True is refused at construction, before anything touches a device."""
    from climt_amd.rrtmg.shortwave import RRTMGShortwave
    with pytest.raises(ValueError, match="skip_night_columns"):
        RRTMGShortwave(pack_day_columns=True)
    with pytest.raises(ValueError, match="skip_night_columns"):
        RRTMGShortwave(pack_day_columns=True, skip_night_columns=False)


def test_permute_check_program(tmp_path_factory):
    """tools/permute_check.cpp -- the library's own slot rule, head and table builder on the CPU -- compiles and reports ok."""
    exe = build_host_program(tmp_path_factory, "permute_check.cpp")
    assert subprocess.run([exe], capture_output=True, text=True, check=True).stdout.strip() == "ok"


def _solve_map_lines(exe):
    out = subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split("\n")
    assert out[-2:] == ["ok", ""]
    return [tuple(int(x) for x in line.split()) for line in out[:-2]]


# The first 40 workgroups of a longwave launch (4 wavefronts per workgroup, blocks of 8 workgroups, 38 work items) over 21 tiles
# of the variant, (blockIdx.x, first list entry, position in sched), from the formulas lw_solve_all_kernel carried itself before
# csrc/rrtmg_solve_map.h: nblk = 6, per = 304, nfull = 0, so bpg = 6, r = q, grp = 0, k = r / 6, first = (r % 6) * 4.
SOLVE_MAP_FIRST_40 = [
    (0, 0, 0), (1, 4, 0), (2, 8, 0), (3, 12, 0), (4, 16, 0), (5, 20, 0),
    (6, 0, 1), (7, 4, 1), (8, 8, 1), (9, 12, 1), (10, 16, 1), (11, 20, 1),
    (12, 0, 2), (13, 4, 2), (14, 8, 2), (15, 12, 2), (16, 16, 2), (17, 20, 2),
    (18, 0, 3), (19, 4, 3), (20, 8, 3), (21, 12, 3), (22, 16, 3), (23, 20, 3),
    (24, 0, 4), (25, 4, 4), (26, 8, 4), (27, 12, 4), (28, 16, 4), (29, 20, 4),
    (30, 0, 5), (31, 4, 5), (32, 8, 5), (33, 12, 5), (34, 16, 5), (35, 20, 5),
    (36, 0, 6), (37, 4, 6), (38, 8, 6), (39, 12, 6)]
# ... and the workgroups 296 .. 311 over 45 tiles, across the end of the full block: nblk = 12, per = 304, nfull = 1; q < 304:
# bpg = 8, r = q, grp = 0, k = r / 8 = 37, first = (r % 8) * 4; from 304 on: bpg = 4, r = q - 304, grp = 1, k = r / 4,
# first = 32 + (r % 4) * 4.
SOLVE_MAP_BLOCK_END = [
    (296, 0, 37), (297, 4, 37), (298, 8, 37), (299, 12, 37), (300, 16, 37), (301, 20, 37), (302, 24, 37), (303, 28, 37),
    (304, 32, 0), (305, 36, 0), (306, 40, 0), (307, 44, 0), (308, 32, 1), (309, 36, 1), (310, 40, 1), (311, 44, 1)]


@pytest.mark.parametrize("sanitized", [False, True])
def test_solve_map_check_program(tmp_path_factory, sanitized):
    """tools/solve_map_check.cpp -- the solve kernels' one launch-order rule (csrc/rrtmg_solve_map.h) on the CPU, plain and under
    the address and undefined-behaviour sanitizers: it checks exactly-once, dense dispatch, the promised order and the list
    bound itself for every workgroup shape in use, and prints the mappings held against the hand-written list here."""
    exe = build_host_program(tmp_path_factory, "solve_map_check.cpp", sanitized=sanitized)
    assert _solve_map_lines(exe) == SOLVE_MAP_FIRST_40 + SOLVE_MAP_BLOCK_END
