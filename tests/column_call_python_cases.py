"""What the Python layer does with a column component's arrays, recorded without a library: the eleven Context methods of
climt_amd/_lib.py are driven against a stand-in whose rrtmg_hip_<entry> callables keep a copy of the struct they are handed and
return 0.  record() -> one JSON-ready dict per variant: for every call the scalars of the struct, for every pointer member
whether it is NULL, the caller's own array (by name), an array the method returned, or a fresh copy, and the structure, shapes
and dtypes of what came back; for every refusal the exception type and its text (stored compactly: _struct, _describe, _compact).  tests/golden/make_column_call_python_golden.py
writes it, tests/test_column_call_python.py compares.  The shapes below are this file's own statement of the eleven tables: it
reads neither COLUMN_ARRAYS nor the C tables."""
import ctypes as C
import json
import threading

import numpy as np

from climt_amd import _lib

NCOL, NBAND = 3, 2
TABLE = 0x7ab1e000      # stands for a handle of cork_table_create


class RecordingLibrary:
    """Every rrtmg_hip_<name> exists, keeps a copy of the struct behind byref() and succeeds."""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        if not name.startswith("rrtmg_hip_"):
            raise AttributeError(name)

        def entry(handle, ref):
            assert handle is None
            self.calls.append((name, type(ref._obj).from_buffer_copy(ref._obj)))
            return 0
        return entry


def make_context(lib=None):
    ctx = _lib.Context.__new__(_lib.Context)
    ctx.lib, ctx._lock, ctx.h = lib or RecordingLibrary(), threading.RLock(), None
    return ctx


class FakeDeviceArray:
    def __init__(self, ptr, dtype):
        self.ptr, self.dtype = ptr, dtype


def _numbers(names, first):
    return {n: first + 0.25 * i for i, n in enumerate(names)}


# ---- the eleven methods: name-keyed inputs A, outputs O and the diagnostics argument D -> the method's own signature --------------------
def _dry_adjustment(ctx, A, O, D, **kw):
    return ctx.dry_adjustment(A["t"], A["q"], A["pmid"], A["pint"], _numbers(_lib.DRY_ADJUST_CONSTANTS, 1.5), t_out=O.get("t_out"), q_out=O.get("q_out"),
                              mixed_top=D.get("mixed_top") if isinstance(D, dict) else None, **kw)


def _boundary_layer(flux_mode):
    def call(ctx, A, O, D, **kw):
        return ctx.boundary_layer(*(A[n] for n in _lib.BOUNDARY_LAYER_IN[:9]), 600.0, _numbers(_lib.BOUNDARY_LAYER_CONSTANTS, 2.5), flux_mode, sh_in=A.get("sh_in"),
                                  lh_in=A.get("lh_in"), diagnostics=D, pressure_scale=100.0, ps_scale=0.5, **O, **kw)
    return call


def _emanuel(ctx, A, O, D, **kw):
    return ctx.emanuel_convection(*(A[n] for n in _lib.EMANUEL_IN[:7]), 300.0, dict(_numbers(_lib.EMANUEL_PARAMETERS, 3.5), minorig=1), _numbers(_lib.EMANUEL_CONSTANTS, 4.5),
                                  qs=A.get("qs"), diagnostics=D, pressure_scale=0.01, **O, **kw)


def _simple_physics(ctx, A, O, D, **kw):
    return ctx.simple_physics(*(A[n] for n in _lib.SIMPLE_PHYSICS_IN[:7]), 450.0, _numbers(_lib.SIMPLE_PHYSICS_CONSTANTS, 5.5), dict(do_lsc=1, do_pbl=1, do_surf_flux=1, use_ts_ext=1),
                              ts=A.get("ts"), qsurf=A.get("qsurf"), lat=A.get("lat"), diagnostics=D, pressure_scale=2.0, ps_scale=3.0, **O, **kw)


def _frierson(ctx, A, O, D, **kw):
    return ctx.frierson_optical_depth(A["pint"], A["ps"], A["lat"], _numbers(_lib.FRIERSON_SCALARS, 6.5), tau=O.get("tau"), pressure_scale=4.0, ps_scale=5.0, **kw)


def _gray_longwave(fused):
    def call(ctx, A, O, D, **kw):
        return ctx.gray_longwave(A["t"], A["tsfc"], A["pint"], _numbers(_lib.GRAY_LONGWAVE_CONSTANTS, 7.5), tau=A.get("tau"), ps=A.get("ps"), lat=A.get("lat"),
                                 frierson=_numbers(_lib.FRIERSON_SCALARS, 8.5) if fused else None, diagnostics=D, pressure_scale=6.0, ps_scale=7.0, **O, **kw)
    return call


def _grid_scale_condensation(ctx, A, O, D, **kw):
    return ctx.grid_scale_condensation(A["t"], A["q"], A["pmid"], A["pint"], _numbers(_lib.GRID_SCALE_CONDENSATION_CONSTANTS, 9.5), diagnostics=D, pressure_scale=8.0, **O, **kw)


def _cork_longwave(ctx, A, O, D, **kw):
    gases = tuple(A.get(g) for g in _lib.CORK_LONGWAVE_GASES[:3]) if "gas0" in A else ()
    return ctx.cork_longwave(TABLE, NBAND, A["t"], A["pmid"], A["pint"], A["tsfc"], A["emis"], _numbers(_lib.CORK_LONGWAVE_CONSTANTS, 10.5), 1 if gases else 0, gases=gases,
                             gas_scale=(0.625, 1.5) if gases else (), taucld=A.get("taucld"), diagnostics=D, pressure_scale=9.0, **O, **kw)


def _surface_ice(ctx, A, O, D, **kw):
    return ctx.surface_ice(0, A["t"], A["height"], A["thick"], A["snow"], A["base"], {n: A[n] for n in _lib.SURFACE_ICE_FLUXES}, A["area_type"], 1800.0,
                           _numbers(_lib.SURFACE_ICE_CONSTANTS, 11.5), diagnostics=D, **O, **kw)


def _bucket_hydrology(layers):
    def call(ctx, A, O, D, **kw):
        kw.pop("nlay", None)
        return ctx.bucket_hydrology(layers, A, 900.0, dict(_numbers(_lib.BUCKET_HYDROLOGY_SCALARS, 12.5), tau_drain=None if layers == 1 else 86400.0), outs=O, diagnostics=D,
                                    pressure_scale=10.0, **kw)
    return call


def _second_best(ctx, A, O, D, **kw):
    return ctx.second_best(A, 1200.0, _numbers(_lib.SECOND_BEST_CONSTANTS, 13.5), outs=O, diagnostics=D, pressure_scale=11.0, ps_scale=12.0, **kw)


_LAND_COLUMNS = "t_air q_air u v p_air ps ts q_sfc snow sw_down lw_down sw_up lw_up area_type ts_out snow_out".split()
# variant -> (method, call, nlay: the entry's minimum, inputs, outputs, diagnostics, {shape class: names}; a name in no class is [nlay][ncol])
VARIANTS = {
    "dry_adjustment": ("dry_adjustment", _dry_adjustment, 1, _lib.DRY_ADJUST_IN, _lib.DRY_ADJUST_OUT, _lib.DRY_ADJUST_DIAG, dict(lev="pint", col="mixed_top", i32="mixed_top")),
    "boundary_layer": ("boundary_layer", _boundary_layer(1), 2, _lib.BOUNDARY_LAYER_IN[:9], _lib.BOUNDARY_LAYER_OUT, _lib.BOUNDARY_LAYER_DIAG,
                       dict(lev="pint", col="ps ts qs sh_in lh_in stress_north stress_east height sh_out lh_out")),
    "boundary_layer_external": ("boundary_layer", _boundary_layer(2), 2, _lib.BOUNDARY_LAYER_IN, _lib.BOUNDARY_LAYER_OUT, _lib.BOUNDARY_LAYER_DIAG,
                                dict(lev="pint", col="ps ts qs sh_in lh_in stress_north stress_east height sh_out lh_out")),
    "emanuel_convection": ("emanuel_convection", _emanuel, 4, _lib.EMANUEL_IN[:7], _lib.EMANUEL_OUT + ("cbmf_out",), _lib.EMANUEL_DIAG,
                           dict(lev="pint", col="cbmf cbmf_out precip wd tprime qprime cape iflag", i32="iflag")),
    "emanuel_convection_qs": ("emanuel_convection", _emanuel, 4, _lib.EMANUEL_IN, _lib.EMANUEL_OUT + ("cbmf_out",), _lib.EMANUEL_DIAG,
                              dict(lev="pint", col="cbmf cbmf_out precip wd tprime qprime cape iflag", i32="iflag")),
    "simple_physics": ("simple_physics", _simple_physics, 1, _lib.SIMPLE_PHYSICS_IN, _lib.SIMPLE_PHYSICS_OUT, _lib.SIMPLE_PHYSICS_DIAG,
                       dict(lev="pint", col="ps ts qsurf lat precl sh_out lh_out")),
    "simple_physics_bare": ("simple_physics", _simple_physics, 1, _lib.SIMPLE_PHYSICS_IN[:7], _lib.SIMPLE_PHYSICS_OUT, _lib.SIMPLE_PHYSICS_DIAG,
                            dict(lev="pint", col="ps ts qsurf lat precl sh_out lh_out")),
    "frierson_optical_depth": ("frierson_optical_depth", _frierson, 1, _lib.FRIERSON_IN, _lib.FRIERSON_OUT, (), dict(lev="pint tau", col="ps lat")),
    "gray_longwave": ("gray_longwave", _gray_longwave(False), 1, ("t", "tsfc", "pint", "tau"), _lib.GRAY_LONGWAVE_OUT, ("hr",), dict(lev="pint tau up dn tau_out", col="tsfc ps lat")),
    "gray_longwave_fused": ("gray_longwave", _gray_longwave(True), 1, ("t", "tsfc", "pint", "ps", "lat"), _lib.GRAY_LONGWAVE_OUT, _lib.GRAY_LONGWAVE_DIAG,
                            dict(lev="pint tau up dn tau_out", col="tsfc ps lat")),
    "grid_scale_condensation": ("grid_scale_condensation", _grid_scale_condensation, 1, _lib.GRID_SCALE_CONDENSATION_IN, _lib.GRID_SCALE_CONDENSATION_OUT,
                                _lib.GRID_SCALE_CONDENSATION_DIAG, dict(lev="pint", col="precip")),
    "cork_longwave": ("cork_longwave", _cork_longwave, 1, ("t", "pmid", "pint", "tsfc", "emis", "taucld", "gas0", "gas2"), _lib.CORK_LONGWAVE_OUT, _lib.CORK_LONGWAVE_DIAG,
                      dict(lev="pint up dn", col="tsfc", bandcol="emis", bandlev="up_band dn_band", bandlay="tau_band trans_band hr_band", layband="taucld")),
    "cork_longwave_bare": ("cork_longwave", _cork_longwave, 1, ("t", "pmid", "pint", "tsfc", "emis"), _lib.CORK_LONGWAVE_OUT, _lib.CORK_LONGWAVE_DIAG,
                           dict(lev="pint up dn", col="tsfc", bandcol="emis", bandlev="up_band dn_band", bandlay="tau_band trans_band hr_band", layband="taucld")),
    "surface_ice": ("surface_ice", _surface_ice, 3, _lib.SURFACE_ICE_IN, _lib.SURFACE_ICE_OUT, _lib.SURFACE_ICE_DIAG,
                    dict(col=" ".join(n for n in _lib.SURFACE_ICE_IN + _lib.SURFACE_ICE_OUT + _lib.SURFACE_ICE_DIAG if n not in ("t", "height", "t_out", "height_out")),
                         i32="area_type flags")),
    "bucket_hydrology_1": ("bucket_hydrology", _bucket_hydrology(1), 1, _lib.BUCKET_HYDROLOGY_IN[:-2], _lib.BUCKET_HYDROLOGY_OUT[:2], _lib.BUCKET_HYDROLOGY_DIAG[:4],
                           dict(flat=" ".join(_lib.BUCKET_HYDROLOGY_IN + _lib.BUCKET_HYDROLOGY_OUT + _lib.BUCKET_HYDROLOGY_DIAG))),
    "bucket_hydrology_2": ("bucket_hydrology", _bucket_hydrology(2), 1, _lib.BUCKET_HYDROLOGY_IN, _lib.BUCKET_HYDROLOGY_OUT, _lib.BUCKET_HYDROLOGY_DIAG,
                           dict(flat=" ".join(_lib.BUCKET_HYDROLOGY_IN + _lib.BUCKET_HYDROLOGY_OUT + _lib.BUCKET_HYDROLOGY_DIAG))),
    "second_best": ("second_best", _second_best, 2, _lib.SECOND_BEST_IN, _lib.SECOND_BEST_OUT, _lib.SECOND_BEST_DIAG,
                    dict(col=" ".join(_LAND_COLUMNS + list(_lib.SECOND_BEST_DIAG)), i32="area_type flags")),
}
IN_PLACE = {"cbmf_out": "cbmf", "base_flux_out": "base"}      # an output that may be an input of another name; the others: x_out may be x


class Variant:
    def __init__(self, name):
        self.name = name
        self.method, self.call, self.nlay, self.IN, self.OUT, self.DIAG, classes = VARIANTS[name]
        self.classes = {n: k for k, names in classes.items() if k != "i32" for n in names.split()}
        self.i32 = classes.get("i32", "").split()
        self.struct = None

    def shape(self, n, nlay=None, ncol=NCOL):
        nlay = self.nlay if nlay is None else nlay
        return dict(lay=(nlay, ncol), lev=(nlay + 1, ncol), col=(ncol,), flat=(ncol,), bandcol=(NBAND, ncol), bandlev=(NBAND, nlay + 1, ncol), bandlay=(NBAND, nlay, ncol),
                    layband=(nlay, ncol, NBAND))[self.classes.get(n, "lay")]

    def dtype(self, n):
        return np.int32 if n in self.i32 else np.float64

    def array(self, n, shape=None):
        shape = self.shape(n) if shape is None else shape
        return (np.arange(int(np.prod(shape))).reshape(shape) + 1).astype(self.dtype(n))

    def pointers(self, names, first):
        return {n: first + 0x1000 * i for i, n in enumerate(names)}

    def sizes(self):
        return dict(ncol=NCOL, nlay=self.nlay)


def _describe(x, mine):
    """The structure of a returned value: an array as "<dtype>[<shape>]", with " strided" where it is not C-contiguous and
    " =<name>" where it IS the caller's array of that name; a device pointer as "ptr <the caller's name for it>"."""
    if isinstance(x, (tuple, list)):
        return [_describe(v, mine) for v in x]
    if isinstance(x, dict):
        return {k: _describe(v, mine) for k, v in x.items()}
    if isinstance(x, np.ndarray):
        who = [n for n, a in mine.items() if a is x]
        return "%s[%s]%s%s" % (x.dtype.name, ",".join(map(str, x.shape)), "" if x.flags.c_contiguous else " strided", " =" + who[0] if who else "")
    if isinstance(x, (int, np.integer)):
        who = [n for n, a in mine.items() if isinstance(a, (int, np.integer)) and a == x]
        return "ptr " + (who[0] if who else hex(x))
    assert x is None, type(x)
    return None


def _returned_arrays(v, x, found):
    """address -> "returned:<name>" for every array the method returned: a dict names its own, a tuple is the outputs in
    their order and then the diagnostics (a dict, or dry_adjustment's mixed_top), a bare array is the one output."""
    if isinstance(x, np.ndarray):
        x = (x,)
    for i, item in enumerate(x):
        named = x[item] if isinstance(x, dict) else item
        if isinstance(named, dict):
            _returned_arrays(v, named, found)
        elif isinstance(named, np.ndarray):
            found.setdefault(named.ctypes.data, "returned:" + (item if isinstance(x, dict) else (v.OUT + v.DIAG)[i]))


def pointer_members(struct):
    return [n for n, t in struct._fields_ if t is C.c_void_p]


def _struct(a, owners):
    """-> (scalars by name, pointers).  The pointers: one character per pointer member in the struct's order -- "." NULL, "="
    the caller's own array (or device pointer) of the member's name, "r" the array the method returned under that name, "f" a
    fresh copy nobody else holds, "?" anything else, spelled out in the dict behind."""
    scalars, chars, other = {}, "", {}
    for name, ctype in a._fields_:
        x = getattr(a, name)
        if ctype is not C.c_void_p:
            scalars[name] = list(x) if hasattr(x, "__len__") else x
            continue
        label = "NULL" if x is None else owners.get(x, "fresh")
        short = {"NULL": ".", "caller:" + name: "=", "returned:" + name: "r", "fresh": "f"}.get(label, "?")
        chars += short
        if short == "?":
            other[name] = label
    return scalars, [chars, other] if other else chars


def one_call(v, A, O, D, **kw):
    """One call of the variant's method -> its record.  `mine`: every array or pointer the caller handed in, by name."""
    ctx = make_context()
    mine = dict(A)
    mine.update({k: x for k, x in O.items() if x is not None})
    if isinstance(D, dict):
        mine.update(D)
    result = v.call(ctx, dict(A), dict(O), dict(D) if isinstance(D, dict) else D, **kw)
    (symbol, a), = ctx.lib.calls
    assert symbol == "rrtmg_hip_" + v.method
    v.struct = type(a)
    owners = {TABLE: "the table's handle"}
    for n, x in mine.items():
        owners.setdefault(x.ctypes.data if isinstance(x, np.ndarray) else x.ptr if isinstance(x, FakeDeviceArray) else int(x), "caller:" + n)
    if not kw.get("memspace"):
        _returned_arrays(v, result, owners)
    scalars, pointers = _struct(a, owners)
    return dict(scalars=scalars, pointers=pointers, returned=_describe(result, mine))


def _compact(v, calls, refusals):
    """The record as it is stored: the scalars of the first call once and for every call those that differ from them; a call
    whose pointers and return value are those of an earlier call says so ("as"); the refusals by their text."""
    first = next(iter(calls.values()))["scalars"]
    out, seen = {}, {}
    for name, c in calls.items():
        key = json.dumps([c["pointers"], c["returned"]], sort_keys=True)
        rest = {"as": seen[key]} if key in seen else dict(pointers=c["pointers"], returned=c["returned"])
        seen.setdefault(key, name)
        differ = {k: x for k, x in c["scalars"].items() if x != first[k]}
        out[name] = dict(rest, **({"scalars_differ": differ} if differ else {}))
    by_text = {}
    for what, r in refusals.items():
        by_text.setdefault("%s: %s" % (r["type"], r["text"]) if r["type"] else "accepted", []).append(what)
    return dict(pointer_members=" ".join(pointer_members(v.struct)), scalars=first, calls=out, refusals=by_text)


def refusal(v, A, O, D, **kw):
    ctx = make_context()
    try:
        v.call(ctx, dict(A), dict(O), dict(D) if isinstance(D, dict) else D, **kw)
    except Exception as e:      # the exact type and text are the record
        assert not ctx.lib.calls
        return dict(type=type(e).__name__, text=str(e))
    return dict(type=None, text="accepted")


def record_variant(name):
    v = Variant(name)
    calls, refusals = {}, {}
    # ---- device pointers: made-up integers, every one different
    PA, PO, PD = v.pointers(v.IN, 0x10000000), v.pointers(v.OUT, 0x20000000), v.pointers(v.DIAG, 0x30000000)
    calls["device"] = one_call(v, PA, PO, PD, memspace=1, **v.sizes())
    calls["device, no diagnostics"] = one_call(v, PA, PO, None, memspace=1, **v.sizes())
    calls["device, diagnostics True"] = one_call(v, PA, PO, True, memspace=1, **v.sizes())
    calls["device, DeviceArrays"] = one_call(v, {n: FakeDeviceArray(p, v.dtype(n)) for n, p in PA.items()}, PO, None, memspace=1, **v.sizes())
    # ---- host arrays at the smallest legal shape
    HA = {n: v.array(n) for n in v.IN}
    none = {n: None for n in v.OUT}
    calls["host"] = one_call(v, HA, none, True)
    calls["host, no diagnostics"] = one_call(v, HA, none, None)
    calls["host, diagnostics False"] = one_call(v, HA, none, False)
    mine = {n: v.array(n) for n in v.OUT}
    calls["host, the caller's outputs and one diagnostic"] = one_call(v, HA, mine, {n: v.array(n) for n in v.DIAG[:1]})
    in_place = {n: HA[IN_PLACE.get(n, n[:-4])] for n in v.OUT if IN_PLACE.get(n, n[:-4] if n.endswith("_out") else None) in HA}
    if in_place:
        calls["host, in place"] = one_call(v, HA, dict(none, **in_place), None)
    converted = dict(HA)
    converted[v.IN[-1]] = HA[v.IN[-1]].astype(np.float32 if v.dtype(v.IN[-1]) == np.float64 else np.int64)
    converted[v.IN[0]] = np.asfortranarray(np.tile(HA[v.IN[0]], (2,) * HA[v.IN[0]].ndim))[tuple(slice(0, s) for s in HA[v.IN[0]].shape)]
    calls["host, an input of another type and one that is not contiguous"] = one_call(v, converted, none, None)
    if name != v.method and v.method != "bucket_hydrology":      # (the refusals once per method; BucketHydrology under both layer counts)
        return json.loads(json.dumps(_compact(v, calls, {})))
    # ---- what is refused, one fault at a time
    by_class = lambda k: [n for n in v.IN if v.classes.get(n, "lay") in k]
    for what, names, shape in (("a profile", by_class(("lay",)), (v.nlay + 1, NCOL)), ("a column", by_class(("col", "flat")), (NCOL + 1,)), ("pint", by_class(("lev",)), (v.nlay, NCOL)),
                               ("a band array", by_class(("bandcol",)), (NBAND + 1, NCOL)), ("taucld", by_class(("layband",)), (NBAND, v.nlay, NCOL))):
        for n in names[-1:]:
            refusals["%s of the wrong shape (%s)" % (what, n)] = refusal(v, dict(HA, **{n: v.array(n, shape)}), none, None)
    if "t" in v.IN:
        refusals["t with one dimension"] = refusal(v, dict(HA, t=v.array("t", (NCOL,))), none, None)
    out = v.OUT[0]
    shape = v.shape(out)
    strided = np.empty(shape[:-1] + (2 * shape[-1],))[..., ::2]
    for what, x in (("not contiguous", strided), ("of the wrong dtype", np.empty(shape, dtype=np.float32)), ("of the wrong size", np.empty(shape[:-1] + (shape[-1] + 1,))),
                    ("not an array", [0.0] * NCOL)):
        refusals["an output %s (%s)" % (what, out)] = refusal(v, HA, dict(none, **{out: x}), None)
    if v.DIAG and v.method != "dry_adjustment":
        d = v.DIAG[0]
        refusals["a diagnostic of the wrong size (%s)" % d] = refusal(v, HA, none, {d: np.empty(v.shape(d)[:-1] + (NCOL + 1,), dtype=v.dtype(d))})
        refusals["a diagnostic of the wrong dtype (%s)" % d] = refusal(v, HA, none, {d: np.empty(v.shape(d), dtype=np.int64)})
        refusals["an unknown diagnostic, host"] = refusal(v, HA, none, dict(nonsense=np.empty(NCOL)))
        refusals["an unknown diagnostic, device"] = refusal(v, PA, PO, dict(nonsense=0x40000000), memspace=1, **v.sizes())
        refusals["an input named as a diagnostic, host"] = refusal(v, HA, none, {v.IN[0]: np.empty(v.shape(v.IN[0]))})
    refusals["device pointers without an output (%s)" % v.OUT[-1]] = refusal(v, PA, dict(PO, **{v.OUT[-1]: None}), None, memspace=1, **v.sizes())
    refusals["device pointers without ncol"] = refusal(v, PA, PO, None, memspace=1, **dict(v.sizes(), ncol=None))
    if v.method != "bucket_hydrology":
        refusals["device pointers without nlay"] = refusal(v, PA, PO, None, memspace=1, **dict(v.sizes(), nlay=None))
    for n in (v.IN[0], v.IN[-1]):
        wrong = np.float32 if v.dtype(n) == np.float64 else np.float64
        refusals["a DeviceArray of the wrong dtype (%s)" % n] = refusal(v, dict(PA, **{n: FakeDeviceArray(PA[n], wrong)}), PO, None, memspace=1, **v.sizes())
    refusals["a DeviceArray of the wrong dtype (output %s)" % out] = refusal(v, PA, dict(PO, **{out: FakeDeviceArray(PO[out], np.float32)}), None, memspace=1, **v.sizes())
    return json.loads(json.dumps(_compact(v, calls, refusals)))


def record():
    return {name: record_variant(name) for name in VARIANTS}


def dumps(x, depth=0):
    """JSON with one line per call, per refusal text and per variant's scalars."""
    if not isinstance(x, dict) or depth >= 3:
        return json.dumps(x, sort_keys=True)
    pad = " " * (depth + 1)
    items = ["%s%s: %s" % (pad, json.dumps(k), json.dumps(v, sort_keys=True) if k in ("scalars", "pointer_members") else dumps(v, depth + 1)) for k, v in sorted(x.items())]
    return "{\n" + ",\n".join(items) + "\n" + " " * depth + "}"
