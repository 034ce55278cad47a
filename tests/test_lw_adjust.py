"""The longwave between radiation calls without a GPU: the exported symbol, the header and the ctypes layer; the stand-alone host
program of the rule and of the kernel's per-thread walk (tools/lw_adjust_check.cpp on csrc/rrtmg_lw_adjust.h) against the numpy
statement (tests/lw_adjust_cases.py), bit for bit -- once more under the host sanitizers; the argument checks of the C entry and
what IntermittentLongwave refuses before it needs a device."""
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

import lw_adjust_cases as X

SYMBOL = "rrtmg_hip_lw_adjust_surface"
HEADER_STRUCT = ("typedef struct { uint32_t struct_size; int32_t ncol, nlay; const double *tsfc_call, *tsfc_now; /* [ncol] */ "
                 "const double *plev; double pressure_scale; /* [nlay+1][ncol] */ const double *uflx, *dflx, *duflx_dt; /* [nlay+1][ncol] */ "
                 "const double *uflxc, *dflxc, *duflxc_dt; /* all three NULL: no clear-sky stream */ "
                 "double *uflx_out, *hr_out, *uflxc_out, *hrc_out; /* uflx_out may be uflx (in place); hr [nlay][ncol] */ } rrtmg_lw_adjust;")


def test_symbol_header_and_python_layer():
    syms = subprocess.check_output(["nm", "-D", "--defined-only", _lib.LIB_PATH]).decode()
    assert re.search(r" T %s\b" % SYMBOL, syms)
    hdr = open(os.path.join(ROOT, "include", "rrtmg_hip.h")).read()
    flat = " ".join(hdr.split())
    assert HEADER_STRUCT in flat
    assert "int rrtmg_hip_lw_adjust_surface(rrtmg_ctx *ctx, const rrtmg_lw_adjust *a);" in flat
    assert "#define RRTMG_HIP_ABI_VERSION 5" in hdr      # probed by symbol: the structs of the flux calls are unchanged
    lib = _lib.load_library()
    assert hasattr(lib, SYMBOL) and lib.rrtmg_hip_abi_version() == 5
    assert lib.rrtmg_hip_lw_adjust_surface.argtypes == [C.c_void_p, C.POINTER(_lib.LwAdjust)]
    # the ctypes struct, field for field against the header's declaration order
    p, d = C.c_void_p, C.c_double
    want = ([("struct_size", C.c_uint32), ("ncol", C.c_int32), ("nlay", C.c_int32), ("tsfc_call", p), ("tsfc_now", p), ("plev", p), ("pressure_scale", d)]
            + [(n, p) for n in "uflx dflx duflx_dt uflxc dflxc duflxc_dt uflx_out hr_out uflxc_out hrc_out".split()])
    assert [(n, t) for n, t in _lib.LwAdjust._fields_] == want
    declared = re.findall(r"\*?(\w+)\s*[,;]", HEADER_STRUCT.split("{", 1)[1].rsplit("}", 1)[0].replace("/*", ";/*").replace("*/", "*/;"))
    declared = [n for n in declared if n in dict(want)]
    assert declared == [n for n, _ in want]
    assert C.sizeof(_lib.LwAdjust) == 16 + 3 * 8 + 8 + 10 * 8
    assert lib.rrtmg_hip_lw_adjust_surface(None, C.byref(_lib.LwAdjust())) == 4      # a NULL context is an argument error
    sig = inspect.signature(_lib.Context.lw_adjust_surface)
    assert list(sig.parameters) == ["self", "ncol", "nlay", "tsfc_call", "tsfc_now", "plev", "all_sky", "clear_sky", "pressure_scale"]
    assert sig.parameters["clear_sky"].default is None and sig.parameters["pressure_scale"].default == 0.0
    assert isinstance(_lib.Context.has_lw_adjust, property)
    assert "IntermittentLongwave" in climt_amd.__all__
    assert "output_work" in inspect.signature(climt_amd.device_state.longwave_device_call).parameters
    src = open(os.path.join(ROOT, "climt_amd", "csrc", "rrtmg_lw_adjust.h")).read()
    assert "constexpr int kLwAdjustChunk = %d;" % X.CHUNK in src


# ---- the C entry's argument checks (a context made without a GPU reports errors) ------------------------------------------------------
@pytest.fixture()
def bare_context():
    lib = _lib.load_library()
    h = C.c_void_p()
    lib.rrtmg_hip_create(C.byref(h), 0)
    assert h.value
    yield lib, h
    lib.rrtmg_hip_destroy(h)


def _args(ncol=4, nlay=3, clear=True):
    """A well-formed struct over host memory (the checks under test come before anything is dereferenced or enqueued)."""
    a, keep = _lib.LwAdjust(), {}
    a.struct_size, a.ncol, a.nlay = C.sizeof(_lib.LwAdjust), ncol, nlay
    names = ["tsfc_call", "tsfc_now", "plev", "uflx", "dflx", "duflx_dt", "uflx_out", "hr_out"] + (["uflxc", "dflxc", "duflxc_dt", "uflxc_out", "hrc_out"] if clear else [])
    for n in names:
        keep[n] = np.zeros((nlay + 1) * ncol)
        setattr(a, n, keep[n].ctypes.data)
    return a, keep


def test_the_entry_refuses_bad_arguments(bare_context):
    lib, h = bare_context
    call = lambda a: lib.rrtmg_hip_lw_adjust_surface(h, C.byref(a))
    message = lambda: lib.rrtmg_hip_last_error(h).decode()
    a, keep = _args()
    # well formed, but rrtmg_hip_lw_init has not run: the status and the words of the flux call
    assert call(a) == 2 and "rrtmg_hip_lw_init has not been called" in message()
    flux = _lib.LwArgs()
    flux.ncol, flux.nlay, flux.struct_size = 4, 3, C.sizeof(_lib.LwArgs)
    assert lib.rrtmg_hip_lw_fluxes(h, C.byref(flux)) == 2
    assert lib.rrtmg_hip_lw_adjust_surface(h, None) == 4
    for size in (0, C.sizeof(_lib.LwAdjust) - 8, C.sizeof(_lib.LwAdjust) + 8):
        a, keep = _args()
        a.struct_size = size
        assert call(a) == 4 and "struct_size" in message()
    for field, value in (("ncol", 0), ("ncol", -1), ("nlay", 0), ("nlay", -3)):
        a, keep = _args()
        setattr(a, field, value)
        assert call(a) == 4 and "positive" in message()
    for field in ("tsfc_call", "tsfc_now", "plev", "uflx", "dflx", "duflx_dt", "uflx_out", "hr_out"):
        for clear in (True, False):
            a, keep = _args(clear=clear)
            setattr(a, field, None)
            assert call(a) == 4 and "must be given" in message(), field
    # the clear-sky stream in part: any one of the five missing, any one of them alone
    clear_fields = ("uflxc", "dflxc", "duflxc_dt", "uflxc_out", "hrc_out")
    for field in clear_fields:
        a, keep = _args()
        setattr(a, field, None)
        assert call(a) == 4 and "all five, or none" in message(), field
        b, keep_b = _args(clear=False)
        setattr(b, field, keep[field].ctypes.data)
        assert call(b) == 4 and "all five, or none" in message(), field
    # an output over an input
    for out in ("hr_out", "hrc_out", "uflx_out", "uflxc_out"):
        for inp in ("tsfc_call", "tsfc_now", "plev", "uflx", "dflx", "duflx_dt", "uflxc", "dflxc", "duflxc_dt"):
            if (out, inp) in (("uflx_out", "uflx"), ("uflxc_out", "uflxc")):
                continue
            a, keep = _args()
            setattr(a, out, keep[inp].ctypes.data)
            assert call(a) == 4 and "%s aliases an input" % out in message(), (out, inp)
    a, keep = _args()
    a.hr_out = keep["uflx"].ctypes.data + 8 * 5      # inside the array, not at its start
    assert call(a) == 4 and "hr_out aliases an input" in message()
    a, keep = _args()
    a.uflx_out = keep["uflx"].ctypes.data + 8      # in place means exactly in place
    assert call(a) == 4 and "uflx_out aliases an input" in message()
    a, keep = _args()
    a.hrc_out = keep["hr_out"].ctypes.data
    assert call(a) == 4 and "hrc_out overlaps hr_out" in message()
    # in place passes the argument checks (and stops, here, at the missing initialisation)
    a, keep = _args()
    a.uflx_out, a.uflxc_out = a.uflx, a.uflxc
    assert call(a) == 2
    a, keep = _args(clear=False)
    assert call(a) == 2


# ---- the stand-alone host program -----------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def program(tmp_path_factory):
    return build_host_program(tmp_path_factory, "lw_adjust_check.cpp", flags=["-ffp-contract=off"])


@pytest.fixture(scope="module")
def program_sanitized(tmp_path_factory):
    return build_host_program(tmp_path_factory, "lw_adjust_check.cpp", sanitized=True, flags=["-ffp-contract=off"])


def run_program(exe, tmp_path, c, clear, in_place, pressure_scale=0.0):
    fin, fout = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    names = ["tsfc_call", "tsfc_now", "plev", "uflx", "dflx", "duflx_dt"] + (["uflxc", "dflxc", "duflxc_dt"] if clear else [])
    np.concatenate([[float(clear), float(in_place), pressure_scale, X.HEATFAC]] + [c[k].ravel() for k in names]).astype(np.float64).tofile(fin)
    nlev, ncol = c["uflx"].shape
    p = subprocess.run([exe, str(ncol), str(nlev - 1), fin, fout], capture_output=True, text=True)
    assert p.returncode == 0 and p.stdout.startswith("ok"), (p.returncode, p.stdout, p.stderr)
    flat, out, at = np.fromfile(fout), {}, 0
    for k, rows in (("uflx", nlev), ("hr", nlev - 1), ("uflxc", nlev), ("hrc", nlev - 1))[:4 if clear else 2]:
        out[k] = flat[at:at + rows * ncol].reshape(rows, ncol)
        at += rows * ncol
    assert at == flat.size
    return out


def check_program(exe, tmp_path, ncol, nlay, clear, in_place, pressure_scale=0.0):
    c = X.case(ncol, nlay, pascal=pressure_scale != 0.0)
    got, want = run_program(exe, tmp_path, c, clear, in_place, pressure_scale), X.want(c, clear, pressure_scale=pressure_scale)
    assert set(got) == set(want)
    for k in want:
        assert X.same_bits(got[k], want[k]), (ncol, nlay, clear, in_place, k, float(np.abs(got[k] - want[k]).max()))
    still = c["tsfc_now"] == c["tsfc_call"]
    assert still.any() and not still.all() if ncol > 1 else True
    assert X.same_bits(got["uflx"][:, still], c["uflx"][:, still])      # (a) dT = 0: the bits of uflx


@pytest.mark.parametrize("in_place", [0, 1], ids=["out_of_place", "in_place"])
@pytest.mark.parametrize("clear", [1, 0], ids=["both_streams", "all_sky_only"])
@pytest.mark.parametrize("nlay", [1, X.CHUNK - 1, X.CHUNK, X.CHUNK + 1])
@pytest.mark.parametrize("ncol", [1, 65])
def test_host_program_equals_the_numpy_statement_bit_for_bit(program, tmp_path, ncol, nlay, clear, in_place):
    check_program(program, tmp_path, ncol, nlay, clear, in_place)


def test_host_program_with_a_pressure_scale_and_a_deep_column(program, tmp_path):
    """plev in Pa with pressure_scale 0.01 (every element scaled, then the difference), and 60 and 1100 layers: 8 blocks of layers,
    and more blocks than the grid is deep -- several trips per thread."""
    for in_place in (0, 1):
        check_program(program, tmp_path, 65, X.CHUNK + 1, 1, in_place, pressure_scale=0.01)
        check_program(program, tmp_path, 3, 60, 1, in_place)
    check_program(program, tmp_path, 2, 1100, 0, 0)


def test_host_program_under_the_address_and_undefined_behaviour_sanitizers(program_sanitized, tmp_path):
    """The same program built with -fsanitize=address,undefined and run stand-alone, clean."""
    for ncol, nlay in ((1, 1), (65, X.CHUNK - 1), (65, X.CHUNK), (65, X.CHUNK + 1), (5, 60)):
        for clear in (1, 0):
            for in_place in (0, 1):
                check_program(program_sanitized, tmp_path, ncol, nlay, clear, in_place)


# ---- the wrapper, as far as it goes without a device -------------------------------------------------------------------------------
class _NoDevice:
    _boundary_dtype = np.float64
    _calc_dflxdt = 1
    _band_fluxes = False


def test_wrapper_checks_its_arguments():
    hours = datetime.timedelta(hours=3)
    with pytest.raises(TypeError):
        climt_amd.IntermittentLongwave(_NoDevice(), 3600)
    for bad in (datetime.timedelta(0), datetime.timedelta(hours=-1)):
        with pytest.raises(ValueError, match="positive"):
            climt_amd.IntermittentLongwave(_NoDevice(), bad)
    plain = _NoDevice()
    plain._calc_dflxdt = 0
    with pytest.raises(ValueError, match="calculate_change_up_flux=True"):
        climt_amd.IntermittentLongwave(plain, hours)
    bands = _NoDevice()
    bands._band_fluxes = True
    with pytest.raises(ValueError, match="band_fluxes"):
        climt_amd.IntermittentLongwave(bands, hours)
    f32 = _NoDevice()
    f32._boundary_dtype = np.float32
    with pytest.raises(ValueError, match="float32"):
        climt_amd.IntermittentLongwave(f32, hours)
    lw = _NoDevice()
    w = climt_amd.IntermittentLongwave(lw, datetime.timedelta(hours=36))      # no 12-hour cap
    assert w.component is lw and w._boundary_dtype == np.float64      # attribute access falls through, as UpdateFrequencyWrapper's
    w = climt_amd.IntermittentLongwave(lw, hours)
    with pytest.raises(TypeError):
        w._due(datetime.datetime(2000, 1, 1), 1800)
    with pytest.raises(ValueError, match="timestep"):
        w._due(datetime.datetime(2000, 1, 1), datetime.timedelta(hours=4))
    t = datetime.datetime(2000, 1, 1)
    assert w._due(t, datetime.timedelta(minutes=30))
    w._last_update_time = t
    assert not w._due(t + datetime.timedelta(hours=2, minutes=30), datetime.timedelta(minutes=30))
    assert w._due(t + datetime.timedelta(hours=3), datetime.timedelta(minutes=30))


def test_wrapper_refuses_the_real_components_options(monkeypatch):
    """The same refusals on RRTMGLongwave instances (the host emulation stands in for the context)."""
    from climt_amd.rrtmg import longwave
    from helpers import EmuContext
    monkeypatch.setattr(longwave, "make_context", lambda device: EmuContext(device))
    monkeypatch.setenv("RRTMG_HIP_ALLOW_SYNTHETIC_LW", "1")
    hours = datetime.timedelta(hours=3)
    with pytest.raises(ValueError, match="calculate_change_up_flux=True"):
        climt_amd.IntermittentLongwave(climt_amd.RRTMGLongwave(), hours)
    with pytest.raises(ValueError, match="band_fluxes"):
        climt_amd.IntermittentLongwave(climt_amd.RRTMGLongwave(calculate_change_up_flux=True, band_fluxes=True), hours)
    with pytest.raises(ValueError, match="float32"):
        climt_amd.IntermittentLongwave(climt_amd.RRTMGLongwave(calculate_change_up_flux=True, boundary_dtype="float32"), hours)
    w = climt_amd.IntermittentLongwave(climt_amd.RRTMGLongwave(calculate_change_up_flux=True, clear_sky_diagnostics=False), hours)
    assert "upwelling_longwave_flux_in_air_assuming_clear_sky" not in w.diagnostic_properties
