"""Exponential and exponential-random McICA overlap (icld 4, 5) without a GPU: the exported symbols and the header's contract, the
stand-alone host program of the kissvec functions (tools/exp_overlap_check.cpp on csrc/rrtmg_sw_device.h and rrtmg_kiss_host.h)
against the numpy statement of the definition (tests/exp_overlap_cases.py), bit for bit, and the Python layer -- what a component
with cloud_overlap_method="exponential[_random]" hands to its context -- on the host emulation of the device functions."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import climt_amd
from climt_amd import _lib
from climt_amd.rrtmg import common, longwave, shortwave
from helpers import ROOT, EmuContext, build_host_program

import exp_overlap_cases as X

SYMBOLS = ("rrtmg_hip_set_mcica_overlap_alpha", "rrtmg_hip_overlap_alpha")
ROCM = os.environ.get("ROCM_PATH", "/opt/rocm")


def test_symbols_header_and_abi_version():
    syms = subprocess.check_output(["nm", "-D", "--defined-only", _lib.LIB_PATH]).decode()
    for s in SYMBOLS:
        assert re.search(r" T %s\b" % s, syms), s
    hdr = open(os.path.join(ROOT, "include", "rrtmg_hip.h")).read()
    flat = " ".join(hdr.split())
    assert "int rrtmg_hip_set_mcica_overlap_alpha(rrtmg_ctx *ctx, int which, int ncol, int nlay, int memspace, const double *alpha);" in flat
    assert ("int rrtmg_hip_overlap_alpha(rrtmg_ctx *ctx, int ncol, int nlay, int memspace, const double *play, const double *tlay, "
            "double rd_over_g, double decorrelation_m, double *alpha);") in flat
    for phrase in ("x_0, y_0, x_1, y_1", "y_0 is drawn and unused", "c_l = c_{l-1} if y_l < a_l", "no clamp", "COPIED"):
        assert phrase in flat, phrase
    assert "#define RRTMG_HIP_ABI_VERSION 5" in hdr
    lib = _lib.load_library()
    assert lib.rrtmg_hip_abi_version() == 5
    assert all(hasattr(lib, s) for s in SYMBOLS)
    # a NULL context is an argument error
    assert lib.rrtmg_hip_set_mcica_overlap_alpha(None, 2, 4, 4, 0, None) == 4
    a = np.ones((4, 4))
    assert lib.rrtmg_hip_overlap_alpha(None, 4, 4, 0, a.ctypes.data, a.ctypes.data, 29.3, 2000.0, a.ctypes.data) == 4


# ---- the stand-alone host program ---------------------------------------------------------------------------------------------
FLAGS = ["-ffp-contract=off", "-D__HIP_PLATFORM_AMD__", "-I" + os.path.join(ROCM, "include")]


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    return build_host_program(tmp_path_factory, "exp_overlap_check.cpp", flags=FLAGS)


@pytest.fixture(scope="module")
def draws():
    """The raw kissvec draws of the two shapes' columns, once: enough for 140 sub-columns behind changeSeed 684."""
    out = {}
    for ncol, nlay in X.SHAPES:
        play, _ = X.pressures(ncol, nlay)
        out[(ncol, nlay)] = (play, X.kiss_draws(play, 684 + 140 * 2 * nlay))
    return out


def _run(exe, tmp_path, play, cldfr, alpha, nsub, icld, seed):
    nlay, ncol = cldfr.shape
    fin, fout = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    np.concatenate([play.ravel(), cldfr.ravel(), alpha.ravel()]).astype(np.float64).tofile(fin)
    out = subprocess.check_output([exe, str(ncol), str(nlay), str(nsub), str(icld), str(seed), fin, fout]).decode()
    assert out.startswith("ok"), out
    nw = (nlay + 63) // 64
    return X.unpack_words(np.fromfile(fout, dtype=np.uint64).reshape(nsub, nw, ncol), nlay)


@pytest.mark.parametrize("shape", X.SHAPES, ids=lambda s: "%dx%d" % s)
def test_host_program_equals_the_numpy_statement_bit_for_bit(program, draws, tmp_path, shape):
    """kiss_mask_jump_exp (checked by the program itself against the sequential kiss_mask_column_exp) against the definition
    from raw draws: icld 4 and 5, 112 and 140 sub-columns, changeSeed 0 and 684, alpha 0, 2 and random in (0, 1)."""
    ncol, nlay = shape
    play, d = draws[shape]
    cldfr = X.cloud_field(ncol, nlay)
    for kind in X.ALPHA_KINDS:
        alpha = X.alpha_field(kind, ncol, nlay)
        for nsub in (112, 140):
            for seed in (0, 684):
                got = {icld: _run(program, tmp_path, play, cldfr, alpha, nsub, icld, seed) for icld in (4, 5)}
                for icld in (4, 5):
                    want = X.kiss_exp_mask(d, cldfr, alpha, icld, nsub, seed)
                    assert np.array_equal(got[icld], want), (kind, nsub, seed, icld, int((got[icld] != want).sum()))
                # the clear gaps make the two modes differ wherever a rank can be inherited at all
                assert (kind == "zero") == np.array_equal(got[4], got[5]), (kind, nsub, seed)
                assert not got[4][:, :, 5].any()      # the column without cloud
    # alpha = 0 is random overlap on every second draw; alpha = 2 keeps the first rank of a sub-column all the way up (icld 4)
    cf = np.where(cldfr < X.CLDMIN, 0.0, cldfr)
    x0 = d[0:112 * 2 * nlay].reshape(112, nlay, 2, ncol)[:, :, 0]
    assert np.array_equal(_run(program, tmp_path, play, cldfr, X.alpha_field("zero", ncol, nlay), 112, 4, 0), x0 >= 1.0 - cf[None])
    assert np.array_equal(_run(program, tmp_path, play, cldfr, X.alpha_field("two", ncol, nlay), 112, 4, 0), x0[:, :1] >= 1.0 - cf[None])


def test_host_program_under_the_address_and_undefined_behaviour_sanitizers(tmp_path_factory, tmp_path, draws):
    """The same program, built with -fsanitize=address,undefined and run stand-alone: two mask words, both modes."""
    exe = build_host_program(tmp_path_factory, "exp_overlap_check.cpp", sanitized=True, flags=FLAGS)
    ncol, nlay = X.SHAPES[1]
    play, d = draws[(ncol, nlay)]
    cldfr, alpha = X.cloud_field(ncol, nlay), X.alpha_field("random", ncol, nlay)
    for icld in (4, 5):
        assert np.array_equal(_run(exe, tmp_path, play, cldfr, alpha, 140, icld, 684), X.kiss_exp_mask(d, cldfr, alpha, icld, 140, 684))


def test_adjacent_layers_agree_as_often_as_the_definition_says(program, tmp_path):
    """cf = 0.5, alpha = 0.6 everywhere, 64 columns x 33 layers x 140 sub-columns: adjacent layers share their rank with
    probability alpha and are independent otherwise, so their bits are equal with probability alpha + (1 - alpha) * 0.5 = 0.8.
    2.9e5 pairs: the binomial sigma is 7.5e-4, the margin 0.01."""
    ncol, nlay = 64, 33
    play, _ = X.pressures(ncol, nlay, seed=9)
    bits = _run(program, tmp_path, play, np.full((nlay, ncol), 0.5), np.full((nlay, ncol), 0.6), 140, 4, 0)
    equal = float((bits[:, 1:] == bits[:, :-1]).mean())
    print("fraction of adjacent-layer pairs with equal bits: %.5f" % equal)
    assert abs(equal - 0.8) <= 0.01
    assert abs(float(bits.mean()) - 0.5) <= 0.01


# ---- the Python layer -------------------------------------------------------------------------------------------------------
class OverlapEmuContext(EmuContext):
    """The host emulation behind Context's two new methods: records what it is handed.  The emulated device functions know the
    reference's overlap rules only, so the flux call itself runs as the parent library runs icld > 3: as 2."""
    sw_clear_sky = lw_clear_sky = True

    def set_sw_clear_sky(self, on=True):
        self.log.append(("sw_clear", bool(on)))

    def set_lw_clear_sky(self, on=True):
        self.log.append(("lw_clear", bool(on)))

    def __init__(self, device=0):
        super().__init__(device)
        self.log = []
        self.has_mcica_overlap_alpha = True

    def overlap_alpha(self, play, tlay, decorrelation_length, rd_over_g=287.05 / 9.80665, out=None, memspace=0, ncol=None, nlay=None):
        self.log.append(("alpha", play.shape, float(decorrelation_length), float(rd_over_g)))
        return X.overlap_alpha_numpy(play, tlay, decorrelation_length, rd_over_g)

    def set_mcica_overlap_alpha(self, which, alpha, memspace=0, ncol=None, nlay=None):
        self.log.append(("set", which, None if alpha is None else np.array(alpha)))

    def _flux(self, which, inp, mcica, out):
        self.log.append((which, inp["icld"], bool(mcica), inp["play"].shape))
        res = (EmuContext.sw_fluxes if which == "sw" else EmuContext.lw_fluxes)(self, dict(inp, icld=min(inp["icld"], 2) if inp["icld"] > 3 else inp["icld"]), mcica=mcica)
        for k, v in out.items():
            v[...] = res[k]
        return out

    def sw_fluxes(self, inp, mcica=False, out=None, memspace=0):
        return self._flux("sw", inp, mcica, out)

    def lw_fluxes(self, inp, mcica=False, out=None, memspace=0):
        return self._flux("lw", inp, mcica, out)

    def radiation_fluxes(self, sw, lw):
        return self._flux("sw", sw["inp"], sw.get("mcica", False), sw["out"]), self._flux("lw", lw["inp"], lw.get("mcica", False), lw["out"])


@pytest.fixture
def emu(monkeypatch):
    ctx = OverlapEmuContext()
    monkeypatch.setattr(shortwave, "make_context", lambda device: ctx)
    monkeypatch.setattr(longwave, "make_context", lambda device: ctx)
    return ctx


def _state(sw, lw):
    return climt_amd.get_default_state([sw, lw], grid_state=climt_amd.get_grid(nx=4, ny=3, nz=10))


def test_exponential_methods_need_mcica(emu):
    for cls, kw in ((climt_amd.RRTMGShortwave, {}), (climt_amd.RRTMGLongwave, dict(allow_synthetic_tables=True))):
        for method in ("exponential", "exponential_random", "Exponential_Random"):
            with pytest.raises(ValueError, match="mcica"):
                cls(cloud_overlap_method=method, **kw)
        with pytest.raises(ValueError, match="positive"):
            cls(cloud_overlap_method="exponential", mcica=True, cloud_overlap_decorrelation_length=0.0, **kw)
    # the reference's dictionary is the reference's
    assert common.rrtmg_cloud_overlap_method_dict == {"clear_only": 0, "random": 1, "maximum_random": 2, "maximum": 3}
    assert common.rrtmg_exponential_overlap_dict == {"exponential": 4, "exponential_random": 5}


def test_components_hand_alpha_over_before_each_call(emu):
    sw = climt_amd.RRTMGShortwave(cloud_overlap_method="exponential", mcica=True, random_number_generator="kissvec")
    lw = climt_amd.RRTMGLongwave(cloud_overlap_method="exponential_random", mcica=True, random_number_generator="kissvec",
                                 cloud_overlap_decorrelation_length=1500.0, allow_synthetic_tables=True)
    state = _state(sw, lw)
    sw(state); lw(state)
    # (each component also says what it wants of the clear-sky stream before its call, as ever)
    assert [e for e in emu.log if e[0].endswith("_clear")] == [("sw_clear", True), ("lw_clear", True)]
    emu.log[:] = [e for e in emu.log if not e[0].endswith("_clear")]
    kinds = [e[0] for e in emu.log]
    assert kinds == ["alpha", "set", "sw", "alpha", "set", "lw"]
    nlay, ncol = 10, 12
    assert emu.log[0][1] == (nlay, ncol) and emu.log[0][2] == 2000.0 and emu.log[3][2] == 1500.0
    assert abs(emu.log[0][3] - 287.0 / 9.80665) < 1e-12
    assert emu.log[1][1] == "sw" and emu.log[4][1] == "lw"
    for i, length in ((1, 2000.0), (4, 1500.0)):
        a = emu.log[i][2]
        assert a.shape == (nlay, ncol) and a.dtype == np.float64
        assert np.all(a[0] == 1.0) and np.all((a[1:] > 0.0) & (a[1:] < 1.0))
        p, t = np.asarray(state["air_pressure"].values).reshape(nlay, ncol), np.asarray(state["air_temperature"].values).reshape(nlay, ncol)
        assert np.array_equal(a, X.overlap_alpha_numpy(p, t, length, 287.0 / 9.80665))
    assert emu.log[2] == ("sw", 4, True, (nlay, ncol)) and emu.log[5] == ("lw", 5, True, (nlay, ncol))
    # the joint call: one alpha for both spectra where both ask for the same length, else one each
    del emu.log[:]
    lw2 = climt_amd.RRTMGLongwave(cloud_overlap_method="exponential", mcica=True, random_number_generator="kissvec", allow_synthetic_tables=True)
    climt_amd.radiation_step(sw, lw2, state)
    # the joint call hands over both components' clear-sky settings, then alpha once, then runs both spectra
    assert [e[0] for e in emu.log] == ["sw_clear", "lw_clear", "alpha", "set", "sw", "lw"] and emu.log[3][1] == "both"
    del emu.log[:]
    climt_amd.radiation_step(sw, lw, state)
    assert [e[:2] for e in emu.log if e[0] == "set"] == [("set", "sw"), ("set", "lw")]


def test_default_instance_is_unchanged(emu):
    sw, lw = climt_amd.RRTMGShortwave(mcica=True, random_number_generator="kissvec"), climt_amd.RRTMGLongwave(mcica=True, random_number_generator="kissvec", allow_synthetic_tables=True)
    state = _state(sw, lw)
    sw(state); lw(state)
    emu.log[:] = [e for e in emu.log if not e[0].endswith("_clear")]
    assert [e[0] for e in emu.log] == ["sw", "lw"] and emu.log[0][1] == 1 and emu.log[1][1] == 1
    assert sw._exp_overlap is None and lw._exp_overlap is None
    for method, icld in (("maximum_random", 2), ("maximum", 3), ("random", 1)):
        assert climt_amd.RRTMGShortwave(cloud_overlap_method=method)._cloud_overlap == icld
    import inspect
    for cls in (climt_amd.RRTMGShortwave, climt_amd.RRTMGLongwave):
        assert inspect.signature(cls.__init__).parameters["cloud_overlap_decorrelation_length"].default == 2000.0
