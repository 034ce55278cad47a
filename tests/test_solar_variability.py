"""Solar variability where a column's position matters (tests/solvar_cases.py), on the host emulation of the device functions.

The reference rescales the facular / sunspot amplitudes once per column of a call, so the solar-variability multipliers of a
column depend on where it sits in the call, and the caller's `indsolvar` comes back rescaled.  136 columns x 12 layers, against
fixtures of the reference Fortran (one call each), then: shards of the grid, aligned to the 64-column tile and not, must be the
whole grid bit for bit and leave the same amplitudes; and the drop-in class must carry the amplitudes from call to call."""
import functools
import os

import numpy as np
import pytest

import solvar_cases as S
from helpers import GOLDEN, EmuContext, emu_sw, maxdiff

EMU_TOL = 1.0e-10      # the bound of test_sw_solar_variability_methods_vs_reference (tests/test_device_functions_emulated.py)
BAND_TOL = 1.0e-9      # the bound of tests/test_band_fluxes.py
LARGEST_EXISTING_FIXTURE = 200 * 1024


@functools.lru_cache(maxsize=None)
def _whole(case):
    """The case on the emulation, once: (inputs, mcica, fixture, outputs -- read-only --, amplitudes as the call left them)."""
    c, mcica, fx = S.load_case(case)
    call = S.fresh(c)
    out = EmuContext().sw_fluxes(call, mcica=mcica)
    for v in out.values():
        v.setflags(write=False)
    return c, mcica, fx, out, call["indsolvar"].copy()


@pytest.mark.parametrize("case", list(S.CASES))
def test_fixture_discriminates(case):
    """A fixture whose amplitudes had decayed to 1 could be met by a library that ignores a column's position: the last two sunlit
    columns must differ in swdflx[top] / coszen by more than 1e-6 W m^-2 and the returned amplitudes from 1 by more than 1e-3
    (load_case asserts both, as the generator did).  The night run sits in the reference's fluxes as its clamp leaves it."""
    c, _, fx = S.load_case(case)
    diff, away = S.discriminates(c, fx["sw/swdflx"], fx["indsolvar"])
    assert diff > 1.0e-6 and away > 1.0e-3
    assert os.path.getsize(os.path.join(GOLDEN, "ref_solvar_%s.npz" % case)) <= LARGEST_EXISTING_FIXTURE
    assert ("band/dn" in fx) == (case in S.BAND_CASES)
    if case in S.NIGHT_CASES:
        assert np.all(c["coszen"][S.NIGHT[0]:S.NIGHT[1]] <= 0.0) and np.all(fx["sw/swdflx"][:, S.NIGHT[0]:S.NIGHT[1]] <= 1.0e-6)
    if case in S.CLOUDY_CASES:
        has = (c["cldfr"] > 0).any(axis=0)
        runs = np.diff(np.flatnonzero(np.diff(has.astype(int)) != 0))
        assert 0 < has.sum() < S.NCOL and runs.size >= 6      # cloudy and cloud-free columns alternate: the sort permutes


def test_a_decayed_fixture_is_rejected():
    """solcycfrac 0.2 contracts the amplitudes by about a half per column: they are exactly 1 long before column 136, and
    discriminates() -- what the generator asserts before it writes -- refuses such outputs."""
    c, mcica = S.case_inputs("clear_i1_s0")
    c["solcycfrac"] = 0.2
    out = EmuContext().sw_fluxes(c, mcica=mcica)
    assert np.array_equal(c["indsolvar"], np.ones(2))
    with pytest.raises(AssertionError):
        S.discriminates(c, out["swdflx"], c["indsolvar"])


@pytest.mark.parametrize("case", list(S.CASES))
def test_emulation_meets_the_reference(case):
    """Every output of every column within 1e-10 of ONE reference call over the 136 columns -- the night run counts as rescale
    steps, inatm_sw runs before the zenith test -- and the amplitudes come back EQUAL to the reference's: scalar host
    arithmetic in the reference's order of operations."""
    c, mcica, fx, out, ind = _whole(case)
    for k, v in S.expected(fx).items():
        d = np.abs(out[k] - v).max(axis=0)
        print("%s %s: max |d| = %.3e at column %d" % (case, k, d.max(), int(d.argmax())))
        assert d.max() <= EMU_TOL, (case, k, float(d.max()), int(d.argmax()))
    assert np.array_equal(ind, fx["indsolvar"]), (case, ind, fx["indsolvar"])
    assert not np.array_equal(ind, S.amplitudes(c["isolvar"]))


@pytest.mark.parametrize("case", S.BAND_CASES)
def test_emulated_band_rows_meet_the_reference(case):
    """The downward flux by band at the surface and the top (sw_band_level reads the multipliers of its own): the bound of
    tests/test_band_fluxes.py; the plain outputs keep their bits."""
    c, mcica, fx, whole, ind = _whole(case)
    call = S.fresh(c)
    out, _, band = emu_sw(call, mcica, bands=("dn",), levels="boundaries")
    assert all(np.array_equal(out[k], whole[k]) for k in whole) and np.array_equal(call["indsolvar"], ind)
    d = maxdiff(band["dn"], fx["band/dn"])
    print("%s band/dn: max |d| = %.3e" % (case, d))
    assert d <= BAND_TOL, (case, d)


@pytest.mark.parametrize("cuts", [S.SHARDS, S.UNALIGNED_SHARDS], ids=["tiles", "unaligned"])
@pytest.mark.parametrize("case", list(S.CASES))
def test_shards_equal_the_whole(case, cuts):
    """A shard placed by shard_col0 / shard_ncol performs the rescale steps of the columns in front of it before its first
    column: its columns get the whole grid's bits, and its `indsolvar` comes back as the whole grid's does."""
    from climt_amd.distributed import slice_columns
    c, mcica, _, whole, ind = _whole(case)
    emu = EmuContext()
    for lo, hi in cuts:
        sub = slice_columns(S.fresh(c), lo, hi)
        sub.update(shard_col0=lo, shard_ncol=S.NCOL)
        out = emu.sw_fluxes(sub, mcica=mcica)
        for k in whole:
            assert np.array_equal(out[k], whole[k][:, lo:hi]), (case, (lo, hi), k, maxdiff(out[k], whole[k][:, lo:hi]))
        assert np.array_equal(sub["indsolvar"], ind), (case, (lo, hi), sub["indsolvar"], ind)


def test_a_shard_without_its_position_differs():
    """The defect the placement repairs: a shard that starts the rescale at its own first column gets other multipliers."""
    from climt_amd.distributed import slice_columns
    c, mcica, _, whole, ind = _whole("clear_i1_s0")
    sub = slice_columns(S.fresh(c), 64, 128)
    out = EmuContext().sw_fluxes(sub, mcica=mcica)
    assert maxdiff(out["swdflx"], whole["swdflx"][:, 64:128]) > 1.0e-3 and not np.array_equal(sub["indsolvar"], ind)


def test_class_carries_the_amplitudes_from_call_to_call(monkeypatch):
    """RRTMGShortwave(solar_variability_method=1, facular_sunspot_amplitude=...) twice on the same 136-column state against two
    consecutive reference calls: the amplitudes persist in the object, so the second call starts where the first one ended."""
    from climt_amd.rrtmg import shortwave
    monkeypatch.setattr(shortwave, "make_context", lambda device: EmuContext(device))
    _, _, fx = S.load_case(S.CLASS_CASE)
    comp = S.class_component()
    state = S.class_state(comp)
    for group, ind in (("sw", "indsolvar"), ("call2", "indsolvar2")):
        t, d = comp(state)
        for k, q in S.CLASS_DIAGNOSTICS.items():
            want = fx["%s/%s" % (group, k)]
            dd = maxdiff(np.asarray(d[q].values).reshape(want.shape), want)
            print("%s %s: max |d| = %.3e" % (group, k, dd))
            assert dd <= EMU_TOL, (group, k, dd)
        assert np.array_equal(t["air_temperature"].values, d["air_temperature_tendency_from_shortwave"].values)
        assert np.array_equal(comp._fac_sunspot_coeff, fx[ind]), (group, comp._fac_sunspot_coeff, fx[ind])
    assert maxdiff(fx["sw/swdflx"], fx["call2/swdflx"]) > 1.0e-3      # (the second call is another call)
