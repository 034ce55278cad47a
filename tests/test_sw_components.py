"""CPU tests of the shortwave flux components (rrtmg_hip_sw_fluxes_components, RRTMGShortwave(flux_components=True)):
the reference driver shim against the reference binder, the committed fixtures against a fresh run of the reference, the
device functions of the components path (host emulation) against the fixtures, the component's properties and the export."""
import ctypes as C
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

import swcomp_cases as S
from helpers import GOLDEN, emu_sw, maxdiff
from climt_amd._lib import SwComponents

ROOT = S.ROOT
FLUX_TOL, TIGHT = 1.0e-2, 1.0e-9       # as the emulation tests of the plain outputs (test_device_functions_emulated.py)
FC = os.environ.get("FC", "/opt/rocm/lib/llvm/bin/flang")


def _reference_present():
    from oracle import ref_driver
    return ref_driver.available("sw") and shutil.which(FC) is not None


needs_reference = pytest.mark.skipif(not _reference_present(), reason="oracle/_ref (the reference Fortran) or flang not present")


@pytest.fixture(scope="module")
def shim():
    subprocess.check_call([os.path.join(ROOT, "tests", "refshim", "build.sh")])
    assert S.shim_available()


@needs_reference
@pytest.mark.parametrize("case", list(S.CASES))
def test_shim_reproduces_the_binder(shim, case):
    """The replicated driver steps are the reference's: the shim's broadband sums == the binder's outputs, bit for bit."""
    _, binder, z = S.reference(case)
    e = S.expected_from_rows(z)
    for k in S.BROADBAND:
        assert np.array_equal(e[k], binder[k]), (k, maxdiff(e[k], binder[k]))


@needs_reference
@pytest.mark.parametrize("case", list(S.CASES))
def test_fixtures_regenerate_bit_for_bit(shim, case):
    fresh = S.fixture_arrays(case)
    z = np.load(os.path.join(GOLDEN, "ref_swcomp_%s.npz" % case))
    assert sorted(z.files) == sorted(fresh), case
    for k in z.files:
        assert np.array_equal(z[k], fresh[k]), (case, k)


def test_fixtures_are_small():
    for case in S.CASES:
        assert os.path.getsize(os.path.join(GOLDEN, "ref_swcomp_%s.npz" % case)) < 256 * 1024, case


@pytest.mark.parametrize("case", list(S.CASES))
def test_emulated_components_match_reference(case):
    """Band split, cloudy / clear choice of the direct beam and the weights of the direct sums, without a GPU."""
    c, mcica, exp = S.load_case(case)
    out, comp, _ = emu_sw(c, mcica, components=S.COMPONENTS)
    for k in S.COMPONENTS:
        d = maxdiff(comp[k], exp[k])
        assert d <= FLUX_TOL and d <= TIGHT, (case, k, d)
    for k in S.BROADBAND:
        assert maxdiff(out[k], exp[k]) <= TIGHT, (case, k)
    assert np.array_equal(comp["difdflx"], out["swdflx"] - comp["dirdflx"])
    assert np.array_equal(comp["difdflxc"], out["swdflxc"] - comp["dirdflxc"])


def test_emulated_components_identities():
    c, mcica, _ = S.load_case("mcica_kiss_maxrand")
    out, comp, _ = emu_sw(c, mcica, components=S.COMPONENTS)
    nlay = c["play"].shape[0]
    assert np.all(comp["difdflx"][nlay] == 0.0) and np.all(comp["difdflxc"][nlay] == 0.0)
    for k in ("difdflx", "difdnuv", "difdnir", "difdflxc"):
        assert comp[k].min() >= -1e-9, k
    np.testing.assert_allclose(comp["dirdnuv"] + comp["dirdnir"], comp["dirdflx"], rtol=1e-10, atol=1e-12)
    np.testing.assert_allclose(comp["difdnuv"] + comp["difdnir"], comp["difdflx"], rtol=1e-10, atol=1e-10)
    _, some, _ = emu_sw(c, mcica, components=("dirdnuv", "difdflxc"))
    assert np.array_equal(some["dirdnuv"], comp["dirdnuv"]) and np.array_equal(some["difdflxc"], comp["difdflxc"])


NEW_DIAGNOSTICS = (
    "downwelling_direct_shortwave_flux_in_air", "downwelling_diffuse_shortwave_flux_in_air",
    "downwelling_direct_shortwave_flux_in_air_assuming_clear_sky", "downwelling_diffuse_shortwave_flux_in_air_assuming_clear_sky",
    "downwelling_direct_ultraviolet_and_visible_flux_in_air", "downwelling_diffuse_ultraviolet_and_visible_flux_in_air",
    "downwelling_direct_near_infrared_flux_in_air", "downwelling_diffuse_near_infrared_flux_in_air")


def test_flux_components_properties():
    from climt_amd.rrtmg.shortwave import FLUX_COMPONENT_DIAGNOSTICS, RRTMGShortwave
    ref = json.load(open(os.path.join(GOLDEN, "reference_interface.json")))["RRTMGShortwave"]
    assert set(FLUX_COMPONENT_DIAGNOSTICS) == set(NEW_DIAGNOSTICS)
    assert sorted(FLUX_COMPONENT_DIAGNOSTICS.values()) == sorted(S.COMPONENTS)
    assert json.loads(json.dumps(RRTMGShortwave.diagnostic_properties)) == ref["diagnostic_properties"]
    props = RRTMGShortwave.diagnostic_properties_for(flux_components=True)     # what __init__ sets on the instance
    assert set(props) - set(RRTMGShortwave.diagnostic_properties) == set(NEW_DIAGNOSTICS)
    for k in NEW_DIAGNOSTICS:
        assert props[k] == {"dims": ["interface_levels", "*"], "units": "W m^-2"}, k
    for k, v in RRTMGShortwave.diagnostic_properties.items():
        assert props[k] == v
    assert json.loads(json.dumps(RRTMGShortwave.diagnostic_properties)) == ref["diagnostic_properties"]    # class untouched
    assert RRTMGShortwave.diagnostic_properties_for(flux_components=False) is RRTMGShortwave.diagnostic_properties
    src = open(os.path.join(ROOT, "climt_amd", "rrtmg", "shortwave.py")).read()
    assert "self.diagnostic_properties = self.diagnostic_properties_for(True)" in src


def _body(src, head):
    """Statements of the function whose definition line starts with `head`, up to its closing brace at column 0."""
    i = src.index(head)
    i = src.index("{\n", i) + 2
    return src[i:src.index("\n}\n", i)].splitlines()


def test_cloudy_dir_body_is_the_cloudy_kernel_body():
    """sw_solve_cloudy_kernel keeps its own body (its ISA must not move); sw_solve_cloudy_body, which the components variant
    runs, is a copy of it: the two must agree but for the sink."""
    src = open(os.path.join(ROOT, "climt_amd", "csrc", "rrtmg_sw.hip")).read()
    a = _body(src, "__global__ void __launch_bounds__(64 * kC4Waves) __attribute__((amdgpu_waves_per_eu(2, 2))) sw_solve_cloudy_kernel(")
    b = _body(src, "__device__ __forceinline__ void sw_solve_cloudy_body(")
    assert len(a) == len(b) > 10
    diff = [(x, y) for x, y in zip(a, b) if x != y]
    assert diff == [("  SwPartSink sink = sw_part_sink(d, slot, col);", "  auto sink = make_sink(slot, col);")], diff


def test_library_exports_components_entry():
    from climt_amd._lib import LIB_PATH
    assert os.path.exists(LIB_PATH)
    syms = subprocess.run(["nm", "-D", "--defined-only", LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert " rrtmg_hip_sw_fluxes_components\n" in syms
    hdr = open(os.path.join(ROOT, "include", "rrtmg_hip.h")).read()
    assert "rrtmg_hip_sw_fluxes_components" in hdr and "typedef struct rrtmg_sw_components" in hdr
    assert C.sizeof(SwComponents) == 8 + 8 * 8
