"""radiation_step -- RRTMGShortwave and RRTMGLongwave of one host state through ONE library call.

`shortwave(state); longwave(state)` extracts the state twice and makes two library calls: every array the two spectra have
in common -- pressures, temperature, the gases, the cloud fields -- crosses to the device twice, and the two solves run back
to back.  Context.radiation_fluxes (rrtmg_hip_radiation_fluxes) takes both argument sets in one call, uploads an array that
both name as the same host array once, and runs the spectra on two streams.  radiation_step is the drop-in route to it: the
state is extracted ONCE, for the union of the two components' inputs, through the machinery the components' own __call__
uses, so the two argument sets hold the very same arrays; array_call's parts 1 and 3 of both components run around the one
library call; the results are re-wrapped per component.  What it returns is what the two separate calls return."""
import weakref

from .. import _sympl_compat as _sc
from .._util import ensure_contiguous_state
from .longwave import RRTMGLongwave
from .shortwave import RRTMGShortwave

# unit strings of the two components' input_properties that name the same unit (specific humidity: "dimensionless" in the
# shortwave, "g/g" in the longwave)
_PURE_NUMBER = ("dimensionless", "g/g", "kg/kg", "1", "")


def _same_property(a, b):
    ua, ub = a.get("units", ""), b.get("units", "")
    return list(a["dims"]) == list(b["dims"]) and (ua == ub or (ua in _PURE_NUMBER and ub in _PURE_NUMBER))


def _union_properties(shortwave, longwave):
    """The inputs of both components: the shortwave's, then what only the longwave reads."""
    props = dict(shortwave.input_properties)
    for name, prop in longwave.input_properties.items():
        if name in props and not _same_property(props[name], prop):
            raise ValueError("radiation_step: input %r is declared as %r by the shortwave and as %r by the longwave: it cannot be extracted once"
                             % (name, props[name], prop))
        props.setdefault(name, prop)
    return props


@ensure_contiguous_state
def _contiguous(_self, raw):
    return raw


def _raw_view(raw, component):
    """The raw state `component`'s array_call would have received: its own inputs (converted, or handed over unconverted under
    name@raw) out of the joint extraction -- the same array objects in both components' views -- and a `_unit_factors` of its own."""
    from .common import RAW
    view = {"time": raw.get("time")}
    for name in component.input_properties:
        for key in (name, name + RAW):
            if key in raw:
                view[key] = raw[key]
    if "_unit_factors" in raw:
        view["_unit_factors"] = {k: v for k, v in raw["_unit_factors"].items() if k in component.input_properties}
    return view


class _JointExtraction(object if _sc.HAVE_SYMPL else _sc.TendencyComponent):
    """The state -> raw arrays and raw arrays -> DataArrays steps of TendencyComponent.__call__ for the union of two components'
    inputs: sympl's two functions, or the stand-in's _extract / _wrap (a stand-in component that is never called itself)."""
    tendency_properties = {}
    diagnostic_properties = {}

    def __init__(self, shortwave, longwave):
        self.input_properties = _union_properties(shortwave, longwave)
        self._unit_factor_on_device = tuple(n for n in shortwave._unit_factor_on_device if n in longwave._unit_factor_on_device)
        self._input_staging = shortwave._input_staging
        self._boundary_dtype = shortwave._boundary_dtype      # (radiation_step has checked that the longwave's is the same)
        super(_JointExtraction, self).__init__()

    def extract(self, state):
        if _sc.HAVE_SYMPL:   # pragma: no cover - sympl is absent in the build container
            from sympl import get_numpy_arrays_with_properties
            raw = get_numpy_arrays_with_properties(state, self.input_properties)
            raw["time"] = state["time"]
            return raw
        return self._extract(state)

    def wrap(self, component, state, tendencies, diagnostics):
        if _sc.HAVE_SYMPL:   # pragma: no cover
            from sympl import restore_data_arrays_with_properties
            return (restore_data_arrays_with_properties(tendencies, component.tendency_properties, state, component.input_properties),
                    restore_data_arrays_with_properties(diagnostics, component.diagnostic_properties, state, component.input_properties))
        # (the stand-in's _wrap reads the wildcard dims its _extract recorded: those of this extraction)
        component._dim_lengths, component._wild_names, component._wild_shape = self._dim_lengths, self._wild_names, self._wild_shape
        return component._wrap(tendencies, component.tendency_properties), component._wrap(diagnostics, component.diagnostic_properties)


def radiation_step(shortwave, longwave, state):
    """-> (sw_tendencies, sw_diagnostics), (lw_tendencies, lw_diagnostics): exactly what `shortwave(state)` and
    `longwave(state)` return, in that order -- same keys, types, units, aliasing and values, bit for bit -- from one
    Context.radiation_fluxes call: shared inputs uploaded once, the two spectra overlapped on the GPU
    (Context.radiation_last() reports what was shared).  McICA seeds are drawn shortwave first, then longwave, as the two
    separate calls draw them.  Host states only: a DeviceState has its own overlapped path.  Both components must have the same
    `boundary_dtype` (ValueError otherwise); with "float32" the one call is rrtmg_hip_radiation_fluxes_f32."""
    from ..device_state import DeviceState
    if not isinstance(shortwave, RRTMGShortwave) or not isinstance(longwave, RRTMGLongwave):
        raise ValueError("radiation_step(shortwave, longwave, state): an RRTMGShortwave and an RRTMGLongwave, in that order")
    if isinstance(state, DeviceState):
        raise ValueError("radiation_step is for host states: a DeviceState already runs the two spectra overlapped (call the components on it)")
    ctx = shortwave._ctx
    if longwave._ctx is not ctx:
        raise ValueError("radiation_step: the two components are on different contexts or devices (%r, %r): one library call serves one context"
                         % (getattr(ctx, "device", None), getattr(longwave._ctx, "device", None)))
    if shortwave._boundary_dtype != longwave._boundary_dtype:
        raise ValueError("radiation_step: the shortwave has boundary_dtype %s, the longwave %s: one library call has one element type"
                         % (shortwave._boundary_dtype.name, longwave._boundary_dtype.name))
    if _sc.HAVE_SYMPL and (getattr(shortwave, "tendencies_in_diagnostics", False) or getattr(longwave, "tendencies_in_diagnostics", False)):   # pragma: no cover
        raise ValueError("radiation_step: tendencies_in_diagnostics is not supported; call the components separately")
    # (the extraction plan is worked out once per pair of components and state structure, as each component keeps its own)
    cache = shortwave.__dict__.setdefault("_joint_extractions", {})
    entry = cache.get(id(longwave))
    if entry is None or entry[1]() is not longwave:
        entry = cache[id(longwave)] = (_JointExtraction(shortwave, longwave), weakref.ref(longwave))
    joint = entry[0]
    raw = _contiguous(None, joint.extract(state))
    sw_call = shortwave._prepare_call(_raw_view(raw, shortwave))
    lw_call = longwave._prepare_call(_raw_view(raw, longwave))
    shortwave._apply_night_skip(ctx)
    longwave._apply_clear_sky(ctx)
    # exponential overlap: the rank correlations of the one state, set for both spectra at once where both ask for the same length
    se, le = getattr(shortwave, "_exp_overlap", None), getattr(longwave, "_exp_overlap", None)
    if se and le and se[1] == le[1]:
        shortwave._apply_overlap(ctx, sw_call, which="both")
    else:
        shortwave._apply_overlap(ctx, sw_call)
        longwave._apply_overlap(ctx, lw_call)
    sw_kw, lw_kw = dict(sw_call["library"]), dict(lw_call["library"])
    precision = {"precision": sw_kw.pop("precision")} if "precision" in sw_kw else {}      # (float32 boundary: said once, for both)
    lw_kw.pop("precision", None)
    ctx.radiation_fluxes(sw=sw_kw, lw=lw_kw, **precision)
    sw_t, sw_d = shortwave._finish_call(sw_call)
    lw_t, lw_d = longwave._finish_call(lw_call)
    return joint.wrap(shortwave, state, sw_t, sw_d), joint.wrap(longwave, state, lw_t, lw_d)


__all__ = ("radiation_step",)
