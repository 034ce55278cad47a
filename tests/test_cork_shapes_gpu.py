"""The correlated-k longwave kernels over the shape of the table: every instantiation of cork_band_kernel<NG, K> on the shape tables
of tests/cork_cases.py (X.SHAPE_TABLES: 1, 3, 4, 5, 9 and 16 g-points, so every NG filled and padded; rank 5, 6 and 7, with and
without a continuum; eight gases; 32 bands; two-node axes), each resident twice -- as stored (float) and with k cast to double.
Every value of the tables is float32-exact, so the two uploads must agree in every bit of every field: what differs is a stride or a
conversion.  Against the numpy statement under the tolerances the maker measured on the reference (tests/golden/cork_<case>.npz), at 1
and 30 layers x 1, 65 and 130 columns: one lane, one tile and a one-lane tile, three tiles.  The first test prints the largest
deviation per field, case and type."""
import numpy as np
import pytest

import climt_amd
from climt_amd import _hip, cork, initialization

import cork_cases as X
from test_cork_lw_gpu import HOST_NAMES, constants, same, state_of

pytestmark = pytest.mark.gpu
NLAYS, NCOLS, TYPES = (1, 30), (1, 65, 130), ("f32", "f64")


@pytest.fixture(autouse=True)
def band_count():
    before = initialization._num_bands["longwave"]
    yield
    initialization._num_bands["longwave"] = before


@pytest.fixture(scope="module")
def ctx():
    from climt_amd.rrtmg.common import make_context
    return make_context(0)


def upload(ctx, kt, k, typ):
    return ctx.cork_table_create(k.astype(np.float32 if typ == "f32" else np.float64), kt.weights, kt.planck, kt.t_grid, kt.p_grid_log, x_grid_log=kt.x_grid_log,
                                 x_clip=kt.x_clip, c_grid_log=kt.c_grid_log, c_clip=kt.c_clip, log_cont=kt.log_cont)


@pytest.fixture(scope="module")
def uploads(ctx):
    """(table, type) -> (KTable, handle): every shape table resident twice on the module's context; the grids, the weights, the
    Planck fractions and the continuum are the same arrays in both."""
    out = {}
    for name in X.SHAPE_TABLES:
        kt = cork.KTable(X.table_path(name))
        assert kt.k.dtype == np.float32 and X.same_bits(kt.k.astype(np.float64).astype(np.float32), kt.k)
        for typ in TYPES:
            out[name, typ] = (kt, upload(ctx, kt, kt.k, typ))
    return out


def call(ctx, entry, name, c, gases=None, gas_scale=None, **kw):
    kt, handle = entry
    gases = [c[g] for g in X.gas_names(name)] if gases is None else gases
    up, dn, tend, d = ctx.cork_longwave(handle, kt.nband, c["t"], c["p"], c["p_int"], c["tsfc"], c["emis"], constants(name), kt.gas_rule, gases=gases,
                                        gas_scale=kt.gas_scale if gas_scale is None else gas_scale, taucld=c["taucld"], **kw)
    return dict(up=up, dn=dn, tend=tend, **(d or {}))


@pytest.mark.parametrize("name", list(X.SHAPE_CASES))
def test_float_and_double_tables_equal_the_statement_and_each_other(ctx, uploads, name):
    tol, table = X.tolerances(name), X.CASES[name][0]
    worst = {typ: {} for typ in TYPES}
    for nlay in NLAYS:
        for ncol in NCOLS:
            c = X.cork_case(name, nlay, ncol)
            got = {typ: call(ctx, uploads[table, typ], name, c) for typ in TYPES}
            for typ in TYPES:
                g = got[typ]
                dev = X.deviations(g, c)
                assert len(dev) == len(X.FIELDS)
                # exact, for either type: the ascending band sum, the two heating rates, the top of the downward sweep
                up, dn = np.zeros_like(g["up"]), np.zeros_like(g["dn"])
                for b in range(g["up_band"].shape[0]):
                    up += g["up_band"][b]
                    dn += g["dn_band"][b]
                assert X.same_bits(up, g["up"]) and X.same_bits(dn, g["dn"]), (name, typ, nlay, ncol)
                assert X.same_bits(g["hr"], g["tend"] * 86400.0)
                assert X.same_bits(g["hr_band"], np.stack([X.heating(u - d, c["p_int"]) * 86400.0 for u, d in zip(g["up_band"], g["dn_band"])]))
                assert X.same_bits(g["dn_band"][:, -1], np.zeros((g["dn_band"].shape[0], ncol)))
                for k, v in dev.items():
                    worst[typ][k] = max(worst[typ].get(k, 0.0), v)
            for f in X.FIELDS:
                assert X.same_bits(got["f32"][f], got["f64"][f]), (name, nlay, ncol, f)
    ngpt = X.table(table)["k_coefficients"].shape[2]
    for typ in TYPES:
        print("cork_band_kernel<%d, %s>, %s: largest deviation from the statement (tolerance) %s" % (
            X.kernel_ng(ngpt), typ, name, ", ".join("%s %.2e (%.1e)" % (k, v, tol[k]) for k, v in sorted(worst[typ].items()))))
    for typ in TYPES:
        for k, v in worst[typ].items():
            assert v <= tol[k], (name, typ, k, v, tol[k])


@pytest.mark.parametrize("typ", TYPES)
def test_every_gas_slot_reads_its_own_profile(ctx, uploads, typ):
    from climt_amd._lib import RRTMGError
    name, tol = "g4_gases8", X.tolerances("g4_gases8")
    c = X.cork_case(name, 30, 65)
    kt, _ = uploads[name, typ]
    names = X.gas_names(name)
    straight = call(ctx, uploads[name, typ], name, c)
    # the profiles moved on by one slot, and any two slots exchanged: other fluxes
    assert not X.same_bits(call(ctx, uploads[name, typ], name, c, gases=[c[g] for g in names[1:] + names[:1]])["up"], straight["up"])
    for i in range(8):
        swapped = list(names)
        swapped[i], swapped[(i + 1) % 8] = swapped[(i + 1) % 8], swapped[i]
        assert not X.same_bits(call(ctx, uploads[name, typ], name, c, gases=[c[g] for g in swapped])["up"], straight["up"]), (i, swapped)
    # the table's gas axis and the profiles permuted together: the statement of that table (the gas sum in its order)
    perm = [3, 0, 6, 1, 7, 2, 5, 4]
    moved = [names[i] for i in perm]
    tab = dict(X.table(name))
    tab["k_coefficients"], tab["gases"] = tab["k_coefficients"][perm], moved
    want = dict(c, **X.statement(tab, c, X.CASES[name][1]))
    assert not X.same_bits(want["tau_band"], c["tau_band"]) and X.within(X.deviations(want, c), {f: 1e-9 for f in X.FIELDS})      # another order of the sum, the same gases
    handle = upload(ctx, kt, kt.k[perm], typ)
    got = call(ctx, (kt, handle), name, c, gases=[c[g] for g in moved], gas_scale=[kt.gas_scale[i] for i in perm])
    ctx.cork_table_destroy(handle)
    dev = X.deviations(got, want)
    assert len(dev) == len(X.FIELDS) and X.within(dev, tol), (dev, tol)
    with pytest.raises(RRTMGError, match="a gas array is missing"):
        call(ctx, uploads[name, typ], name, c, gases=[None if i == 5 else c[g] for i, g in enumerate(names)])
    assert same(call(ctx, uploads[name, typ], name, c), straight)


@pytest.mark.parametrize("name", ["bands32_cloudy", "g16_cont", "g16_cont_spans"])
def test_a_block_of_columns_alone_equals_the_block_inside_the_whole(ctx, uploads, name):
    lo, hi = 37, 101
    c = X.cork_case(name, 30, 130)
    for typ in TYPES:
        entry = uploads[X.CASES[name][0], typ]
        whole = call(ctx, entry, name, c)
        part = call(ctx, entry, name, {k: np.ascontiguousarray(v[..., lo:hi, :] if k == "taucld" else v[..., lo:hi]) for k, v in c.items() if k not in X.FIELDS})
        assert all(X.same_bits(part[f], whole[f][..., lo:hi]) for f in X.FIELDS), (name, typ)


@pytest.mark.parametrize("typ", TYPES)
def test_host_pointers_equal_device_pointers_with_eight_gases(ctx, uploads, typ):
    name = "g4_gases8"
    kt, handle = uploads[name, typ]
    c = X.cork_case(name, 30, 65)
    host = call(ctx, uploads[name, typ], name, c)
    names = ("t", "p", "p_int", "tsfc", "emis", "taucld") + tuple(X.gas_names(name))
    dev = {k: _hip.DeviceArray.from_host(np.ascontiguousarray(c[k])) for k in names}
    out = {f: _hip.DeviceArray(c[f].shape, np.float64) for f in X.FIELDS}
    ctx.cork_longwave(handle, kt.nband, dev["t"], dev["p"], dev["p_int"], dev["tsfc"], dev["emis"], constants(name), kt.gas_rule, gases=[dev[g] for g in X.gas_names(name)],
                      gas_scale=kt.gas_scale, taucld=dev["taucld"], up=out["up"], dn=out["dn"], tend=out["tend"],
                      diagnostics={f: out[f] for f in X.FIELDS[3:]}, memspace=1, ncol=65, nlay=30)
    ctx.synchronize()
    assert all(X.same_bits(out[f].download().reshape(c[f].shape), host[f]) for f in X.FIELDS)
    assert all(X.same_bits(dev[k].download().reshape(c[k].shape), c[k]) for k in names)      # only read


@pytest.mark.parametrize("name", ["g4_gases8", "bands32_cloudy"])
def test_component_on_a_host_state_and_on_a_device_state(ctx, uploads, name):
    c = X.cork_case(name, 30, 65)
    direct = call(ctx, uploads[X.CASES[name][0], "f32"], name, c)
    comp = climt_amd.CorkLongwaveRadiation(optics="correlated_k", table=X.table_path(X.CASES[name][0]), diffusivity_factor=X.CASES[name][1], context=ctx)
    state = state_of(comp, c)
    assert len(state) == 1 + len(X.INPUTS) + len(X.gas_names(name))
    tend, diag = comp(state)
    assert X.same_bits(tend["air_temperature"].values, direct["tend"]) and set(diag) == set(HOST_NAMES.values())
    for f, n in HOST_NAMES.items():
        v = diag[n].values
        assert X.same_bits(np.moveaxis(v, -1, 0) if f.endswith("_band") else v, direct[f]), (name, f)
    with climt_amd.DeviceState.from_host(state, [comp], context=ctx) as ds:
        t_dev, d_dev = comp(ds)
        ctx.synchronize()
        got = dict(tend=t_dev["air_temperature"].buf.download().reshape(direct["tend"].shape),
                   **{f: d_dev[n].buf.download().reshape(direct[f].shape) for f, n in HOST_NAMES.items()})
        assert same(got, direct), name
