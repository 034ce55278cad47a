"""CPU tests of the fluxes by band (rrtmg_hip_sw_fluxes_bands, rrtmg_hip_lw_fluxes_bands, band_fluxes=True of the two
components): the reference driver shims against the reference binder, the committed fixtures against a fresh run of the
reference, the device functions of the band integration (host emulation, tests/emu) against the fixtures, the struct
mirrors and exports, the band limits, the components' properties, and the recorded comparison of the tuned kernels' device
code with the parent commit's."""
import ctypes as C
import json
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import band_cases as B
from helpers import GOLDEN, EmuContext, emu_lw, emu_sw, maxdiff
from climt_amd._lib import LwBandFluxes, SwBandFluxes

ROOT = B.ROOT
TIGHT = 1.0e-9       # as the emulation tests of the plain outputs (test_device_functions_emulated.py)
FC = os.environ.get("FC", "/opt/rocm/lib/llvm/bin/flang")
LARGEST_EXISTING_FIXTURE = 200729   # bytes: tests/golden/ref_swcomp_aer10_overcast.npz


def _reference_present():
    from oracle import ref_driver
    return ref_driver.available("sw") and ref_driver.available("lw") and shutil.which(FC) is not None


needs_reference = pytest.mark.skipif(not _reference_present(), reason="oracle/_ref (the reference Fortran) or flang not present")


@pytest.fixture(scope="module")
def shims():
    subprocess.check_call([os.path.join(ROOT, "tests", "refshim", "build.sh")])
    assert B.shims_available()


@needs_reference
@pytest.mark.parametrize("case", list(B.CASES))
def test_shim_reproduces_the_binder_and_bands_sum_to_it(shims, case):
    """Called over the full band range the shim's sums == the binder's outputs, bit for bit; the per-band rows are
    non-negative and sum to that broadband within the rounding bound."""
    which = case[:2]
    _, binder, out = B.reference(case)
    for i, m in enumerate(B.MEMBERS[which]):
        full = out[0, i]
        if m in B.BROADBAND[which]:
            bb = binder[B.BROADBAND[which][m]]
            assert np.array_equal(full, bb), (case, m, maxdiff(full, bb))
        assert np.all(out[1:, i] >= 0.0), (case, m)
        assert np.all(np.abs(out[1:, i].sum(axis=0) - full) <= B.SUM_BOUND * np.abs(full)), (case, m)


@needs_reference
@pytest.mark.parametrize("case", list(B.CASES))
def test_fixtures_regenerate_bit_for_bit(shims, case):
    fresh = B.fixture_arrays(case)
    z = np.load(os.path.join(GOLDEN, "ref_bands_%s.npz" % case))
    assert sorted(z.files) == sorted(fresh), case
    for k in z.files:
        assert np.array_equal(z[k], fresh[k]), (case, k)


def test_fixtures_are_small_and_whole():
    for case in B.CASES:
        assert os.path.getsize(os.path.join(GOLDEN, "ref_bands_%s.npz" % case)) <= LARGEST_EXISTING_FIXTURE, case
        c, _, _, band = B.load_case(case)
        nlay, ncol = c["play"].shape
        assert set(band) == set(B.MEMBERS[case[:2]])
        for m, v in band.items():      # fewer columns, never fewer bands or levels
            assert v.shape == (B.NBAND[case[:2]], nlay + 1, ncol), (case, m)
    assert {B.load_case(c)[0]["play"].shape[0] for c in B.CASES} == {60, 100}


def emu_bands(which, inp, mcica, levels="all", members=None):
    """The band path of the device functions, run on the host -> (plain outputs, requested band arrays)."""
    members = members or B.MEMBERS[which]
    if which == "lw":
        return emu_lw(inp, mcica, bands=members, levels=levels)
    out, _, band = emu_sw(inp, mcica, bands=members, levels=levels)
    return out, band


@pytest.mark.parametrize("case", list(B.CASES))
def test_emulated_bands_match_reference(case):
    """sw_band_level / lw_band_level on the host against the reference's per-band calls, every member, both `levels`; the
    sum over the bands against the broadband output of the same run."""
    which = case[:2]
    c, mcica, bb, exp = B.load_case(case)
    nlay = c["play"].shape[0]
    out, band = emu_bands(which, c, mcica)
    for m in B.MEMBERS[which]:
        d = maxdiff(band[m], exp[m])
        assert d <= TIGHT, (case, m, d)
    for k, v in bb.items():
        assert maxdiff(out[k], v) <= TIGHT, (case, k)
    for m, k in B.BROADBAND[which].items():
        assert np.all(band[m] >= 0.0)
        assert np.all(np.abs(band[m].sum(axis=0) - out[k]) <= B.SUM_BOUND * np.abs(out[k])), (case, m)
    _, two = emu_bands(which, c, mcica, levels="boundaries")
    for m in B.MEMBERS[which]:
        assert np.array_equal(two[m][:, 0], band[m][:, 0]) and np.array_equal(two[m][:, 1], band[m][:, nlay]), (case, m)


@pytest.mark.parametrize("case", ["sw_mcica_kiss_maxrand", "lw_mcica_kiss_random"])
def test_emulated_bands_with_a_generated_mask(case):
    """McICA with the sub-column mask generated inside the emulation (kissvec, no cldfmcl), which the band path could not do
    while it had a driver of its own.  No fixture: the band sums close on the broadband outputs of the same run."""
    which = case[:2]
    c, mcica, _, _ = B.load_case(case)
    assert mcica and c["irng"] == 0
    c = {k: v for k, v in c.items() if k != "cldfmcl"}
    out, band = emu_bands(which, c, mcica)
    for m, k in B.BROADBAND[which].items():
        assert out[k].max() > 1.0, (case, k)
        assert np.all(np.abs(band[m].sum(axis=0) - out[k]) <= B.SUM_BOUND * np.abs(out[k])), (case, m)


def test_emulated_bands_identities():
    c, mcica, _, _ = B.load_case("sw_lowsun_night")
    out, band = emu_bands("sw", c, mcica)
    assert np.all(band["dndir"] <= band["dn"] + 1e-9) and np.all(band["dndirc"] <= band["dnc"] + 1e-9)
    for m in B.MEMBERS["sw"]:
        assert np.all(np.abs(band[m][:, :, 0]) <= B.NIGHT_ZERO), m      # the night column
    assert band["dn"][:, :, 3].max() > 1.0
    _, some = emu_bands("sw", c, mcica, members=("upc", "dndir"))
    assert np.array_equal(some["upc"], band["upc"]) and np.array_equal(some["dndir"], band["dndir"])
    c, mcica, _, _ = B.load_case("sw_clear_L60")       # cloud-free columns: the clear-sky outputs are the all-sky ones
    _, band = emu_bands("sw", c, mcica)
    assert np.array_equal(band["upc"], band["up"]) and np.array_equal(band["dnc"], band["dn"]) and np.array_equal(band["dndirc"], band["dndir"])
    c, mcica, _, _ = B.load_case("lw_clear_L60")
    _, band = emu_bands("lw", c, mcica)
    assert np.array_equal(band["upc"], band["up"]) and np.array_equal(band["dnc"], band["dn"])
    _, some = emu_bands("lw", c, mcica, members=("dn",))
    assert np.array_equal(some["dn"], band["dn"])


def test_struct_mirrors_match_the_header(tmp_path):
    """ctypes.sizeof of the mirrors == sizeof in a compiled snippet of the header, and the field offsets."""
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("clang") or "/opt/rocm/lib/llvm/bin/clang"
    src = tmp_path / "sizes.c"
    fields_sw = ("struct_size", "levels", "up", "dn", "upc", "dnc", "dndir", "dndirc")
    fields_lw = fields_sw[:6]
    prints = ['printf("%zu\\n", sizeof(rrtmg_sw_band_fluxes));', 'printf("%zu\\n", sizeof(rrtmg_lw_band_fluxes));']
    prints += ['printf("%%zu\\n", offsetof(rrtmg_sw_band_fluxes, %s));' % f for f in fields_sw]
    prints += ['printf("%%zu\\n", offsetof(rrtmg_lw_band_fluxes, %s));' % f for f in fields_lw]
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "rrtmg_hip.h"\nint main(void) { %s return 0; }\n' % " ".join(prints))
    exe = tmp_path / "sizes"
    subprocess.check_call([cc, "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    want = [C.sizeof(SwBandFluxes), C.sizeof(LwBandFluxes)]
    want += [getattr(SwBandFluxes, f).offset for f in fields_sw] + [getattr(LwBandFluxes, f).offset for f in fields_lw]
    assert got == want
    assert [n for n, _ in SwBandFluxes._fields_] == list(fields_sw) and [n for n, _ in LwBandFluxes._fields_] == list(fields_lw)


def test_library_exports_band_entries():
    from climt_amd._lib import LIB_PATH
    assert os.path.exists(LIB_PATH)
    syms = subprocess.run(["nm", "-D", "--defined-only", LIB_PATH], capture_output=True, text=True, check=True).stdout
    for s in ("rrtmg_hip_sw_fluxes_bands", "rrtmg_hip_lw_fluxes_bands", "rrtmg_hip_band_limits"):
        assert " %s\n" % s in syms, s
    hdr = open(os.path.join(ROOT, "include", "rrtmg_hip.h")).read()
    assert "typedef struct rrtmg_sw_band_fluxes" in hdr and "typedef struct rrtmg_lw_band_fluxes" in hdr
    assert re.search(r"#define RRTMG_HIP_ABI_VERSION 5\b", hdr)      # probed by the symbol, not by the version


def test_band_limits():
    from climt_amd._lib import band_limits, load_library
    lo, hi = band_limits("sw")
    assert list(lo) == [2600, 3250, 4000, 4650, 5150, 6150, 7700, 8050, 12850, 16000, 22650, 29000, 38000, 820]
    assert list(hi) == [3250, 4000, 4650, 5150, 6150, 7700, 8050, 12850, 16000, 22650, 29000, 38000, 50000, 2600]
    assert np.array_equal(hi[:12], lo[1:13])       # bands 16..28 are contiguous; band 29 (820-2600) comes last
    lo, hi = band_limits("lw")
    assert lo[0] == 10 and hi[-1] == 3250 and np.array_equal(hi[:-1], lo[1:])
    delwave = EmuContext().get_table("lw/wvn/delwave")      # the table the longwave weights its bands with
    assert delwave.shape == (16,) and np.array_equal(hi - lo, delwave)
    lib = load_library()
    assert lib.rrtmg_hip_band_limits(2, None, None) < 0 and lib.rrtmg_hip_band_limits(0, None, None) == 14
    assert lib.rrtmg_hip_band_limits(1, None, None) == 16


SW_NEW = {
    "upwelling_shortwave_flux_in_air_by_band": "up", "downwelling_shortwave_flux_in_air_by_band": "dn",
    "upwelling_shortwave_flux_in_air_assuming_clear_sky_by_band": "upc", "downwelling_shortwave_flux_in_air_assuming_clear_sky_by_band": "dnc",
    "downwelling_direct_shortwave_flux_in_air_by_band": "dndir", "downwelling_direct_shortwave_flux_in_air_assuming_clear_sky_by_band": "dndirc"}
LW_NEW = {
    "upwelling_longwave_flux_in_air_by_band": "up", "downwelling_longwave_flux_in_air_by_band": "dn",
    "upwelling_longwave_flux_in_air_assuming_clear_sky_by_band": "upc", "downwelling_longwave_flux_in_air_assuming_clear_sky_by_band": "dnc"}


def test_band_flux_properties():
    from climt_amd.rrtmg import longwave, shortwave
    ref = json.load(open(os.path.join(GOLDEN, "reference_interface.json")))
    for mod, cls, new, dim, refname in ((shortwave, shortwave.RRTMGShortwave, SW_NEW, "num_shortwave_bands", "RRTMGShortwave"),
                                        (longwave, longwave.RRTMGLongwave, LW_NEW, "num_longwave_bands", "RRTMGLongwave")):
        assert mod.BAND_FLUX_DIAGNOSTICS == new
        before = cls.diagnostic_properties
        assert cls.diagnostic_properties_for(band_fluxes=False) is before      # the default instance keeps the class dict itself
        assert cls.diagnostic_properties_for() is before
        props = cls.diagnostic_properties_for(band_fluxes=True)
        assert set(props) - set(before) == set(new)
        for k in new:
            assert props[k] == {"dims": [dim, "interface_levels", "*"], "units": "W m^-2"}, k
            broadband = k.replace("_by_band", "")
            assert broadband in before or "direct" in k, k      # the broadband names with _by_band appended
        for k, v in before.items():
            assert props[k] is v
        assert cls.diagnostic_properties is before
        assert json.loads(json.dumps(cls.diagnostic_properties)) == ref[refname]["diagnostic_properties"]      # class untouched
    both = shortwave.RRTMGShortwave.diagnostic_properties_for(flux_components=True, band_fluxes=True)
    assert set(both) == set(shortwave.RRTMGShortwave.diagnostic_properties) | set(shortwave.FLUX_COMPONENT_DIAGNOSTICS) | set(SW_NEW)


def test_python_layer_refuses_unknown_names():
    from climt_amd._lib import LW_BAND_FLUXES, SW_BAND_FLUXES, SW_NBAND, LwBandFluxes as L, SwBandFluxes as S, _band_struct
    with pytest.raises(KeyError):
        _band_struct(S, SW_BAND_FLUXES, SW_NBAND, {"sideways": np.zeros((14, 61, 4))}, "all", 60, 4)
    with pytest.raises(KeyError):
        _band_struct(L, LW_BAND_FLUXES, 16, {"dndir": np.zeros((16, 61, 4))}, "all", 60, 4)
    with pytest.raises(ValueError):
        _band_struct(S, SW_BAND_FLUXES, SW_NBAND, {"up": np.zeros((14, 61, 4))}, "some", 60, 4)
    with pytest.raises(ValueError):
        _band_struct(S, SW_BAND_FLUXES, SW_NBAND, {"up": np.zeros((14, 61, 4))}, "boundaries", 60, 4)      # wants [14][2][4]
    b = _band_struct(S, SW_BAND_FLUXES, SW_NBAND, {"up": np.zeros((14, 2, 4)), "dndir": 4096}, "boundaries", 60, 4)
    assert b.levels == 1 and b.struct_size == C.sizeof(S) and b.dndir == 4096 and not b.dn


ISA_KERNELS = ("sw_solve_all_kernel<", "sw_solve_cloudy_kernel(", "sw_solve_all_dir_kernel<", "sw_solve_cloudy_dir_kernel(",
               "lw_solve_all_kernel<", "sw_fluxheat_kernel(", "lw_fluxheat_kernel(", "sw_components_kernel(")


def test_recorded_isa_comparison_says_identical():
    """profiles/isa_compare_band_fluxes.txt (tools/isa_compare.py, the parent commit's build against this one): the solve
    kernels, the flux / heating kernels and the components kernel disassemble to the same instruction stream."""
    from tools.isa_compare import KERNELS
    assert tuple(k.replace("rrtmg::", "") for k in KERNELS) == ISA_KERNELS
    lines = [l for l in open(os.path.join(ROOT, "profiles", "isa_compare_band_fluxes.txt")).read().splitlines() if l and not l.startswith("#")]
    for k in ISA_KERNELS:
        mine = [l for l in lines if "rrtmg::" + k in l]
        assert mine, k
        for l in mine:
            assert l.startswith("identical "), l
    assert sum("lw_solve_all_kernel<" in l for l in lines) == 3      # rtrn, rtrnmc and rtrnmr (MR = true) variants
    assert not any(l.startswith(("DIFFERENT", "MISSING")) or "MISSING" in l for l in lines)


def test_recorded_call_path_isa_comparison_says_identical():
    """profiles/isa_compare_call_path.txt (tools/isa_compare.py --all, the parent commit's build against the build with the shared
    host call path, csrc/rrtmg_call.h): every device function of the parent's code objects -- the kernels of both spectra, the
    night kernels included -- disassembles to the same instruction stream, and this build has no function of its own."""
    from tools.isa_compare import KERNELS
    night = tuple("rrtmg::sw_%s_night_kernel(" % n for n in ("prep_fused", "cloud", "tile_lists", "kiss_mask", "fluxheat", "components", "bandflux"))
    lines = [l for l in open(os.path.join(ROOT, "profiles", "isa_compare_call_path.txt")).read().splitlines() if l and not l.startswith("#")]
    for k in KERNELS + night:
        assert any(k in l for l in lines), k
    for l in lines:
        assert l.startswith("identical "), l


def test_item_order_is_asserted_at_init():
    """The flush-on-change walk needs band-contiguous items: build_sw_tab / build_lw_tab check it and fail init otherwise."""
    for f in ("rrtmg_sw_host.h", "rrtmg_lw_host.h"):
        src = open(os.path.join(ROOT, "climt_amd", "csrc", f)).read()
        assert 'err = "work items are not band-contiguous in slot order"; return false;' in src, f
        assert 'err = "work items do not cover every band"; return false;' in src, f
