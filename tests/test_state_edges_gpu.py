"""GPU tests on atmospheric states off the synthetic profile (tests/golden/ref_state_*.npz, make_golden.py states): the index
clamps of setcoef, the ends of the Planck table, the 1e-32 gas substitutions, and -- what only a device run can see -- lanes of
one wavefront that disagree about laytrop, jp, jt and the clamp taken.  24 columns: one 64-column tile, one call per case."""
import numpy as np
import pytest

from helpers import STATE_CASES, load_state_case, maxdiff

pytestmark = pytest.mark.gpu

FLUX_TOL, HR_TOL, TIGHT = 1.0e-2, 1.0e-3, 5.0e-9      # as tests/test_gpu_parity.py


def _run(ctx, spectrum, c, mcica):
    return ctx.sw_fluxes(c, mcica=mcica) if spectrum == "sw" else ctx.lw_fluxes(c, mcica=mcica)


def _columns(c, sel):
    """The columns `sel` (an index array or a slice) of boundary-level inputs: the column axis is the last one, except in the
    direct cloud optics [layer, column, band], which no state case has."""
    ncol = c["play"].shape[1]
    return {k: (np.ascontiguousarray(v[..., sel]) if isinstance(v, np.ndarray) and v.shape[-1] == ncol else v) for k, v in c.items()}


@pytest.mark.parametrize("case", STATE_CASES)
def test_states_vs_reference_fixture(gpu_ctx, case):
    """The device against the reference Fortran's outputs on the inputs stored in the fixture, at the bounds of every other
    committed fixture.  Measured on an MI355X: longwave fluxes <= 3.4e-13 W m-2, heating rates <= 1.1e-10 K day-1; shortwave
    fluxes <= 1.3e-10 (hot_wet McICA), heating rates <= 1.6e-9 (ragged_tropopause McICA, a layer of 0.02 hPa)."""
    spectrum, mcica, c, exp = load_state_case(case)
    out = _run(gpu_ctx, spectrum, c, mcica)
    assert set(exp) <= set(out)
    for k, v in exp.items():
        d = maxdiff(out[k], v)
        print(case, k, "%.2e" % d)
        assert d <= (HR_TOL if k.endswith(("hr", "hrc")) else FLUX_TOL), (k, d)
        assert d <= TIGHT, (k, d)


@pytest.mark.parametrize("case", [c for c in STATE_CASES if "ragged_tropopause" in c or "deep_column" in c])
def test_state_columns_do_not_depend_on_their_neighbours(gpu_ctx, case):
    """Neighbouring lanes differ in laytrop by up to 38 layers and in jp by 5 and more at the same layer: the 24 columns in one
    call, one column per call, and the columns in reversed order must give the same bits (kissvec seeds per column).  A
    wave-uniform assumption about laytrop, jp or the solar-source layer cannot pass this."""
    spectrum, mcica, c, _ = load_state_case(case)
    ncol = c["play"].shape[1]
    whole = _run(gpu_ctx, spectrum, c, mcica)
    for o in whole.values():
        assert np.all(np.isfinite(o))
    assert (c["icld"] == 0) or (c["cldfr"] > 0).any(0).all()     # (every column takes the solve variant its tile takes)
    differ = []
    for i in range(ncol):
        one = _run(gpu_ctx, spectrum, _columns(c, slice(i, i + 1)), mcica)
        differ += [(k, i, maxdiff(whole[k][:, i:i + 1], one[k])) for k in whole if not np.array_equal(whole[k][:, i:i + 1], one[k])]
    assert not differ, differ
    back = _run(gpu_ctx, spectrum, _columns(c, np.arange(ncol)[::-1]), mcica)
    for k in whole:
        assert np.array_equal(whole[k][:, ::-1], back[k]), k


@pytest.mark.parametrize("case", [c for c in STATE_CASES if "cold_dry" in c])
def test_state_edges_host_and_device_pointer_paths_agree(gpu_ctx, case):
    """cold_dry: gases exactly zero in a few layers, water vapour one value down whole columns -- arrays that look all-zero or
    uniform to the probes of the host-input path (rrtmg_host_inputs.h) and are neither.  The host-pointer path (detection, fills,
    unit factors on the device) and the device-pointer path (uploads what it is given) must give the same bits."""
    from climt_amd import _hip
    from climt_amd._lib import LW_OUT, SW_OUT
    spectrum, mcica, c, _ = load_state_case(case)
    nlay, ncol = c["play"].shape
    host = _run(gpu_ctx, spectrum, c, mcica)
    dev = {k: _hip.DeviceArray.from_host(v) for k, v in c.items() if isinstance(v, np.ndarray)}
    inp = {k: v.ptr for k, v in dev.items()}
    inp.update({k: v for k, v in c.items() if not isinstance(v, np.ndarray)}); inp.update(ncol=ncol, nlay=nlay)
    names = [(k, nlay + lev) for k, lev in (SW_OUT if spectrum == "sw" else LW_OUT)]
    if c.get("idrv"):
        names += [("duflx_dt", nlay + 1), ("duflxc_dt", nlay + 1)]
    out = {k: _hip.DeviceArray((rows, ncol)) for k, rows in names}
    fluxes = gpu_ctx.sw_fluxes if spectrum == "sw" else gpu_ctx.lw_fluxes
    fluxes(inp, mcica=mcica, out={k: v.ptr for k, v in out.items()}, memspace=1)
    assert set(host) == set(out)
    for k in host:
        assert np.array_equal(host[k], out[k].download()), k
