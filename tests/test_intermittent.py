"""The shortwave between radiation calls without a GPU: the exported symbols, the header and the ctypes layer; the stand-alone host
program of the per-column functions (tools/mean_coszen_check.cpp on csrc/rrtmg_intermittent.h) against the numpy statement of the
definition (tests/intermittent_cases.py) -- the interval mean to the derived tolerances, the rescale bit for bit -- once more
under the host sanitizers; and what IntermittentShortwave checks before it needs a device."""
import ctypes as C
import datetime
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

import climt_amd
from climt_amd import _lib
from helpers import ROOT, build_host_program

import intermittent_cases as X

SYMBOLS = ("rrtmg_hip_mean_coszen", "rrtmg_hip_mean_coszen_sun", "rrtmg_hip_scale_columns")


def test_symbols_header_and_python_layer():
    syms = subprocess.check_output(["nm", "-D", "--defined-only", _lib.LIB_PATH]).decode()
    for s in SYMBOLS:
        assert re.search(r" T %s\b" % s, syms), s
    hdr = open(os.path.join(ROOT, "include", "rrtmg_hip.h")).read()
    flat = " ".join(hdr.split())
    assert ("int rrtmg_hip_mean_coszen(rrtmg_ctx *ctx, int ncol, int memspace, const double *lat_deg, const double *lon_deg, double t0_centuries, "
            "double t1_centuries, double *coszen_mean, double *sunlit_fraction, double *zenith_mean, double *insolation);") in flat
    assert ("int rrtmg_hip_mean_coszen_sun(rrtmg_ctx *ctx, int ncol, int memspace, const double *lat_deg, const double *lon_deg, double sin_dec, "
            "double cos_dec, double hour_angle0, double hour_angle_advance, double *coszen_mean, double *sunlit_fraction, "
            "double *zenith_mean, double *insolation);") in flat
    assert "int rrtmg_hip_scale_columns(rrtmg_ctx *ctx, int ncol, const double *num, const double *den, int nentries, const rrtmg_scale_entry *entries);" in flat
    assert "typedef struct rrtmg_scale_entry { const double *src; /* [rows][ncol] */ double *dst;" in flat
    assert "#define RRTMG_SCALE_MAX_ENTRIES 16" in hdr and _lib.SCALE_MAX_ENTRIES == 16
    assert "#define RRTMG_HIP_ABI_VERSION 5" in hdr      # probed by symbol: the structs of the flux calls are unchanged
    lib = _lib.load_library()
    assert all(hasattr(lib, s) for s in SYMBOLS) and lib.rrtmg_hip_abi_version() == 5
    # the ctypes signatures, argument for argument against the header
    d, i, p = C.c_double, C.c_int, C.c_void_p
    assert lib.rrtmg_hip_mean_coszen.argtypes == [p, i, i, p, p, d, d, p, p, p, p]
    assert lib.rrtmg_hip_mean_coszen_sun.argtypes == [p, i, i, p, p, d, d, d, d, p, p, p, p]
    assert lib.rrtmg_hip_scale_columns.argtypes == [p, i, p, p, i, C.POINTER(_lib.ScaleEntry)]
    assert [(n, t) for n, t in _lib.ScaleEntry._fields_] == [("src", p), ("dst", p), ("rows", C.c_int32), ("reserved", C.c_int32)]
    assert C.sizeof(_lib.ScaleEntry) == 24
    # a NULL context is an argument error
    a = np.zeros(4)
    assert lib.rrtmg_hip_mean_coszen(None, 4, 0, a.ctypes.data, a.ctypes.data, 0.1, 0.1 + 1e-6, a.ctypes.data, a.ctypes.data, None, None) == 4
    assert lib.rrtmg_hip_mean_coszen_sun(None, 4, 0, a.ctypes.data, a.ctypes.data, 0.4, 0.9, 0.0, 0.5, a.ctypes.data, a.ctypes.data, None, None) == 4
    assert lib.rrtmg_hip_scale_columns(None, 4, a.ctypes.data, a.ctypes.data, 1, (_lib.ScaleEntry * 1)()) == 4
    # the methods of Context
    sig = inspect.signature(_lib.Context.mean_coszen)
    assert list(sig.parameters)[:9] == ["self", "lat_deg", "lon_deg", "t0_centuries", "t1_centuries", "out_mean", "out_fraction", "memspace", "ncol"]
    assert sig.parameters["memspace"].default == 0 and sig.parameters["out_mean"].default is None
    assert list(inspect.signature(_lib.Context.scale_columns).parameters)[:4] == ["self", "num", "den", "entries"]
    assert isinstance(_lib.Context.has_intermittent, property)
    assert "IntermittentShortwave" in climt_amd.__all__ and hasattr(climt_amd.Instellation, "interval_mean")


# ---- the stand-alone host program -----------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def program(tmp_path_factory):
    return build_host_program(tmp_path_factory, "mean_coszen_check.cpp", flags=["-ffp-contract=off"])


@pytest.fixture(scope="module")
def program_sanitized(tmp_path_factory):
    return build_host_program(tmp_path_factory, "mean_coszen_check.cpp", sanitized=True, flags=["-ffp-contract=off"])


def run_mean(exe, tmp_path, lat, lon, t0=0.0, t1=0.0, sun=None, status=0):
    fin, fout = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    head = [0.0, t0, t1, 0.0, 0.0, 0.0, 0.0] if sun is None else [1.0, 0.0, 0.0] + list(sun)
    np.concatenate([head, lat, lon]).astype(np.float64).tofile(fin)
    p = subprocess.run([exe, "mean", str(lat.size), fin, fout], capture_output=True, text=True)
    assert p.returncode == status, (p.returncode, p.stderr)
    if status:
        return None
    assert p.stdout.startswith("ok"), p.stdout
    out = np.fromfile(fout)
    return tuple(out[:4]), out[4:].reshape(4, lat.size)


def run_scale(exe, tmp_path, num, den, arrays, in_place):
    fin, fout = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    np.concatenate([[len(arrays)], [a.shape[0] for a in arrays], in_place, num, den] + [a.ravel() for a in arrays]).astype(np.float64).tofile(fin)
    out = subprocess.check_output([exe, "scale", str(num.size), fin, fout]).decode()
    assert out.startswith("ok"), out
    flat, res, at = np.fromfile(fout), [], 0
    for a in arrays:
        res.append(flat[at:at + a.size].reshape(a.shape))
        at += a.size
    return res


def same_bits(got, want):
    return got.shape == want.shape and np.array_equal(got.view(np.uint64), want.view(np.uint64))


@pytest.mark.parametrize("name", list(X.INTERVALS))
def test_host_program_equals_the_numpy_statement(program, tmp_path, name):
    """mean_coszen_column on the 320 columns, the interval from its two times: the sun as the numpy statement forms it (the last
    bits of libm apart), the insolation factor to 1e-12, fraction and mean on their own to 1e-11 where they are conditioned."""
    t0, t1 = X.interval_centuries(name)
    sun, out = run_mean(program, tmp_path, X.LAT, X.LON, t0, t1)
    want_sun = X.interval_sun(t0, t1)
    assert np.allclose(sun, want_sun, rtol=0.0, atol=1e-14), (sun, want_sun)
    mean, fraction, zenith, insolation = out
    X.check_mean_coszen(mean, fraction, X.WANT[name], "host program, %s:" % name)
    assert same_bits(insolation, mean * fraction)
    assert same_bits(zenith, np.where(mean > 0.0, np.arccos(mean), 0.5 * np.pi)) or np.abs(zenith - np.arccos(mean)).max() <= 1e-15
    assert np.all(zenith[mean == 0.0] == 0.5 * np.pi)
    # ... and with the sun handed over (rrtmg_hip_mean_coszen_sun): the numpy statement's own four numbers
    _, out2 = run_mean(program, tmp_path, X.LAT, X.LON, sun=want_sun)
    X.check_mean_coszen(out2[0], out2[1], X.WANT[name], "host program, %s, sun given:" % name)


def test_intervals_that_are_refused(program, tmp_path):
    t0 = X.centuries(X.T0)
    day = 1.0 / 36525.0
    for t1 in (t0, t0 - 0.1 * day, t0 + 0.5 * day * 1.001, t0 + day, float("nan")):
        run_mean(program, tmp_path, X.LAT[:4], X.LON[:4], t0, t1, status=4)      # RRTMG_ERR_ARG
    run_mean(program, tmp_path, X.LAT[:4], X.LON[:4], t0, X.centuries(X.T0 + datetime.timedelta(hours=12)))
    for advance in (0.0, -0.1, 2.0 * np.pi, 7.0):
        run_mean(program, tmp_path, X.LAT[:4], X.LON[:4], sun=(0.4, 0.9, 1.0, advance), status=4)


def test_additivity_on_the_host(program, tmp_path):
    """Six 30-minute steps against the whole 3 hours, one declination: sum mu_i f_i D_i = mu f D to 1e-12 D (the GPU test's
    statement, here on the host program)."""
    sin_dec, cos_dec, g0, D = X.interval_sun(*X.interval_centuries("3h"))
    _, whole = run_mean(program, tmp_path, X.LAT, X.LON, sun=(sin_dec, cos_dec, g0, D))
    total = np.zeros(X.NCOL)
    for i in range(6):
        _, part = run_mean(program, tmp_path, X.LAT, X.LON, sun=(sin_dec, cos_dec, g0 + i * (D / 6.0), D / 6.0))
        total += part[3] * (D / 6.0)
    assert np.abs(total - whole[3] * D).max() <= 1e-12 * D


@pytest.mark.parametrize("in_place", [0, 1], ids=["out_of_place", "in_place"])
def test_scale_rule_equals_numpy_bit_for_bit(program, tmp_path, in_place):
    num, den, arrays = X.scale_case()
    got = run_scale(program, tmp_path, num, den, arrays, [in_place] * len(arrays))
    s = X.scale_factor(num, den)
    assert (s == 0.0).sum() >= 6 and np.signbit(s[7])      # den = 0, den < 0, num = 0 and num = -0.0 (a factor of -0.0 writes +0.0 too)
    for g, a in zip(got, arrays):
        want = X.scale_columns(a, num, den)
        both_nan = np.isnan(g) & np.isnan(want)
        assert np.array_equal(g.view(np.uint64)[~both_nan], want.view(np.uint64)[~both_nan])
        assert np.all(g[:, s == 0.0] == 0.0) and not np.signbit(g[:, s == 0.0]).any()      # +0.0 under NaN, -inf and -0.0 too
    assert np.signbit(got[0][2, 11]) and got[0][2, 11] == 0.0      # a negative zero of src under a factor that is not 0 stays one
    # a deep array (14 bands x 7 levels: more row groups than one trip) beside a one-row one, mixed in place / out of place
    rng = np.random.default_rng(8)
    deep = [rng.uniform(-1.0, 1.0, (14 * 7 * 6, num.size)), rng.uniform(0.0, 1.0, (1, num.size))]
    for g, a in zip(run_scale(program, tmp_path, num, den, deep, [in_place, 1 - in_place]), deep):
        assert same_bits(g, X.scale_columns(a, num, den))


def test_host_program_under_the_address_and_undefined_behaviour_sanitizers(program_sanitized, tmp_path):
    """The same program built with -fsanitize=address,undefined and run stand-alone: every interval, the refusals, the rescale."""
    for name in X.INTERVALS:
        _, out = run_mean(program_sanitized, tmp_path, X.LAT, X.LON, *X.interval_centuries(name))
        X.check_mean_coszen(out[0], out[1], X.WANT[name], "sanitized host program, %s:" % name)
    run_mean(program_sanitized, tmp_path, X.LAT[:4], X.LON[:4], 0.2, 0.2, status=4)
    num, den, arrays = X.scale_case()
    for in_place in (0, 1):
        for g, a in zip(run_scale(program_sanitized, tmp_path, num, den, arrays, [in_place] * len(arrays)), arrays):
            want = X.scale_columns(a, num, den)
            ok = ~(np.isnan(g) & np.isnan(want))
            assert np.array_equal(g.view(np.uint64)[ok], want.view(np.uint64)[ok])


# ---- the Python layer, as far as it goes without a device -----------------------------------------------------------------------------
class _NoDevice:
    _boundary_dtype = np.float64


def test_wrapper_checks_its_arguments():
    sw, sun = _NoDevice(), object()
    with pytest.raises(TypeError):
        climt_amd.IntermittentShortwave(sw, sun, 3600)
    for bad in (datetime.timedelta(0), datetime.timedelta(hours=13), datetime.timedelta(hours=-1)):
        with pytest.raises(ValueError, match="12 hours"):
            climt_amd.IntermittentShortwave(sw, sun, bad)
    f32 = _NoDevice()
    f32._boundary_dtype = np.float32
    with pytest.raises(ValueError, match="float32"):
        climt_amd.IntermittentShortwave(f32, sun, datetime.timedelta(hours=3))
    w = climt_amd.IntermittentShortwave(sw, sun, datetime.timedelta(hours=3))
    assert w.component is sw and w._boundary_dtype == np.float64      # attribute access falls through, as UpdateFrequencyWrapper's
    with pytest.raises(TypeError):
        w._due(datetime.datetime(2000, 1, 1), 1800)
    with pytest.raises(ValueError, match="timestep"):
        w._due(datetime.datetime(2000, 1, 1), datetime.timedelta(hours=4))
    t = datetime.datetime(2000, 1, 1)
    assert w._due(t, datetime.timedelta(minutes=30))
    w._last_update_time = t
    assert not w._due(t + datetime.timedelta(hours=2, minutes=30), datetime.timedelta(minutes=30))
    assert w._due(t + datetime.timedelta(hours=3), datetime.timedelta(minutes=30))
