"""A model state that lives in HBM, and the radiation step on it.

The reference's model loop (examples/gmd_aquaplanet.py:61-104) hands every component a host state and gets host arrays
back; with the kernels on the GPU that is 0.2-0.5 GB over PCIe per radiation call.  Here the state is uploaded ONCE:

    dstate = DeviceState.from_host(state, [sun, sw, lw, slab])       # component units and [levels][columns] layout
    stepper = DeviceAdamsBashforth(sw, lw, slab)                     # the same component instances as on the host
    for ...:
        dstate.update(sun(dstate))                                   # components recognise a DeviceState
        diagnostics, dstate = stepper(dstate, timestep)              # SW || LW -> tendency sum -> slab -> Adams-Bashforth
        dstate.update(diagnostics)
        dstate["time"] += timestep
    olr = dstate.download("upwelling_longwave_flux_in_air")          # only what is looked at comes back

`component(dstate)` returns (tendencies, diagnostics) -- or diagnostics -- whose values are DeviceQuantity handles; the
host work of `array_call` between the kernels (interface temperatures, q -> volume mixing ratio, cos(zenith), tendency
sums, the Adams-Bashforth update) runs as small kernels on the same streams (rrtmg_hip_interface_values /
_elementwise / _ab_step), shortwave and longwave overlap on the context's two streams, and nothing is copied until
`download`.  One library context (tables of both spectra) is shared by all components of a DeviceState.
"""
import datetime

import numpy as np

from . import _hip
from . import _sympl_compat as _sc
from ._lib import SLAB_IN
from .rrtmg.common import make_context


class DeviceQuantity:
    """A quantity in HBM: float64 (or int32) array in a component's layout -- dims like ['mid_levels', '*'], the wildcard
    being the flattened horizontal grid -- with its units."""

    def __init__(self, buf, shape, dims, units):
        self.buf, self.shape, self.dims, self.units = buf, tuple(int(s) for s in shape), tuple(dims), units

    @property
    def ptr(self):
        return self.buf.ptr

    @property
    def size(self):
        return int(np.prod(self.shape))

    def __repr__(self):
        return "DeviceQuantity(%s, dims=%s, units=%s)" % (self.shape, self.dims, self.units)


def _units_of(da):
    return getattr(da, "attrs", {}).get("units", "")


def _convert(values, src, dst):
    if hasattr(_sc, "convert_units"):
        return _sc.convert_units(values, src, dst)
    return _sc.DataArray(values, attrs={"units": src}).to_units(dst).values      # real sympl / xarray


def _same_units(a, b):
    if hasattr(_sc, "_canon"):
        return _sc._canon(a) == _sc._canon(b)
    return a == b


class DeviceState(dict):
    """name -> DeviceQuantity (plus 'time' -> datetime).  Built once from a host state for a set of components."""

    def __init__(self, ctx, wild_names, wild_shape):
        super().__init__()
        self.ctx = ctx
        self.wild_names, self.wild_shape = list(wild_names), list(wild_shape)
        self.ncol = int(np.prod(wild_shape)) if wild_shape else 1
        self.scalars = {}          # zero-dimensional quantities stay on the host (name -> float)
        self.host_dims = {}        # name -> dims of the host DataArray the quantity came from (download restores them)
        self._work = {}            # derived arrays and component outputs, by key: allocated once, reused every step
        self._tables = set()
        self.step_count = 0
        self._derived_ok = False   # interface temperatures / vmr / cos(zenith) match the resident state

    def __setitem__(self, name, value):
        self._derived_ok = False
        super().__setitem__(name, value)

    def update(self, *args, **kwargs):
        self._derived_ok = False
        super().update(*args, **kwargs)

    # ---- construction --------------------------------------------------------------------------------------------
    @classmethod
    def from_host(cls, state, components, device=0, context=None, deferred=True):
        ctx = context if context is not None else make_context(device)
        props = {}
        for comp in components:
            comp = getattr(comp, "component", comp)          # UpdateFrequencyWrapper
            # (a component whose host layout is not the resident one -- EmanuelConvection is [*][levels] -- names the resident layout)
            for name, prop in getattr(comp, "device_input_properties", comp.input_properties).items():
                props.setdefault(name, prop)
        wild_names = wild_shape = None
        for name, prop in props.items():
            if name in state and "*" in prop["dims"]:
                da = state[name]
                named = [d for d in prop["dims"] if d != "*"]
                wn = [d for d in da.dims if d not in named]
                if wild_names is None or len(wn) > len(wild_names):
                    wild_names, wild_shape = wn, [np.asarray(da.values).shape[da.dims.index(d)] for d in wn]
        self = cls(ctx, wild_names or [], wild_shape or [])
        self["time"] = state.get("time")
        for name, prop in props.items():
            if name not in state:
                continue          # produced by another component during the step (zenith angle, fluxes ...)
            self.put_host(name, state[name], prop)
        if deferred:
            self._prev_deferred = ctx.set_deferred(True)
        return self

    def close(self):
        """Collect the pending work and hand the (shared) context back in the mode it was found in: from_host switches the
        context to deferred mode, which every other memspace=1 caller of the same context would otherwise inherit."""
        prev = getattr(self, "_prev_deferred", None)
        if prev is not None:
            self.ctx.synchronize()
            self.ctx.set_deferred(prev)
            self._prev_deferred = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def put_host(self, name, da, prop):
        """Upload a host DataArray in the layout / units of `prop` (a component's input property)."""
        values, dims = np.asarray(da.values), tuple(da.dims)
        want = list(prop["dims"])
        if name in _SURFACE_ROW:          # always resident as the radiation writes them, whoever asked first
            want = ["interface_levels", "*"]
        self.host_dims[name] = dims
        if values.dtype.kind not in "fiub":      # area_type strings -> codes (slab_surface.py:9)
            from .slab_surface import AREA_MAP
            codes = np.zeros(values.shape, dtype=np.int32)
            s = values.astype(str)
            for k, v in AREA_MAP.items():
                codes[s == k] = v
            self[name] = DeviceQuantity(_hip.DeviceArray.from_host(np.ascontiguousarray(codes.reshape(-1))), (codes.size,), ("*",), prop["units"])
            return
        values = _convert(values.astype(np.float64), _units_of(da), prop["units"])
        if not want:
            self.scalars[name] = float(values)
            return
        named = [d for d in want if d != "*"]
        wild = [d for d in dims if d not in named]
        if wild and sorted(wild) == sorted(self.wild_names):
            wild = self.wild_names
        order = []
        for d in want:
            order.extend([dims.index(w) for w in (wild if d == "*" else [d])])
        shape = [self.ncol if d == "*" else values.shape[dims.index(d)] for d in want]
        arr = np.ascontiguousarray(np.transpose(values, order).reshape(shape))
        self[name] = DeviceQuantity(_hip.DeviceArray.from_host(arr), shape, want, prop["units"])

    # ---- buffers -------------------------------------------------------------------------------------------------
    def work(self, key, shape, dims, units, dtype=np.float64):
        """A device array owned by the state, allocated on first use (component outputs, derived inputs)."""
        q = self._work.get(key)
        if q is None or q.shape != tuple(shape):
            q = self._work[key] = DeviceQuantity(_hip.DeviceArray(shape, dtype), shape, dims, units)
        return q

    def need(self, name, prop):
        q = self.get(name)
        if q is None:
            raise KeyError("device state is missing input quantity %r" % name)
        if tuple(q.dims) != tuple(prop["dims"]):
            raise ValueError("quantity %r is resident as %s, component wants %s" % (name, q.dims, prop["dims"]))
        if q.buf.dtype == np.float64 and not _same_units(q.units, prop["units"]):
            raise ValueError("quantity %r is resident in %r, component wants %r" % (name, q.units, prop["units"]))
        return q

    def init_tables(self, which, cpd):
        (self.ctx.sw_init if which == "sw" else self.ctx.lw_init)(cpd)      # (idempotent per context)

    # ---- back to the host ----------------------------------------------------------------------------------------
    def join_streams(self):
        """Main-stream work enqueued from here on runs after the longwave that is in flight on its own stream.  Called by
        whatever consumes the longwave's outputs or overwrites its inputs on the main stream -- NOT by the shortwave call, so a
        stepper that calls the longwave and then the shortwave gets the two side by side (ordering the main stream behind the
        longwave inside the longwave call, as this did at first, ran them back to back: 1.87 instead of 1.6 ms per step)."""
        if getattr(self, "_lw_inflight", False):
            self.ctx.order_streams(1)
            self._lw_inflight = False

    def download(self, name, synchronize=True):
        """The quantity as a host DataArray: wildcard re-expanded to the horizontal dims it was uploaded with."""
        if synchronize:
            self.ctx.synchronize()
        if name in self.scalars:
            return _sc.DataArray(np.array(self.scalars[name]), dims=(), attrs={"units": ""})
        q = self[name]
        arr = q.buf.download().reshape(q.shape)
        shape, names = [], []
        for d, n in zip(q.dims, q.shape):
            if d == "*":
                shape.extend(self.wild_shape); names.extend(self.wild_names)
            else:
                shape.append(n); names.append(d)
        return _sc.DataArray(arr.reshape(shape), dims=names, attrs={"units": q.units})


# radiation outputs [interface_levels][*] of which the slab reads the surface row in place
_SURFACE_ROW = ("downwelling_shortwave_flux_in_air", "downwelling_longwave_flux_in_air", "upwelling_shortwave_flux_in_air",
                "upwelling_longwave_flux_in_air")


# ---- the components' device paths ---------------------------------------------------------------------------------
def _derived(ds, comp_inputs):
    """Interface temperatures, water-vapour volume mixing ratio and cos(zenith) from the resident state, once per step."""
    if ds._derived_ok:
        return ds._work["derived_vals"]
    ctx = ds.ctx
    ds.join_streams()      # a longwave still in flight reads the buffers rewritten here
    t, p, pi = ds["air_temperature"], ds["air_pressure"], ds["air_pressure_on_interface_levels"]
    nlay, ncol = t.shape
    out = {}
    tint = ds.work("d.tint", (nlay + 1, ncol), ("interface_levels", "*"), "degK")
    ctx.interface_values(ncol, nlay, t.ptr, ds["surface_temperature"].ptr, p.ptr, pi.ptr, tint.ptr)
    out["tint"] = tint
    q = ds.work("d.h2o", (nlay, ncol), ("mid_levels", "*"), "dimensionless")
    ctx.elementwise("muldiv", nlay * ncol, ds["specific_humidity"].ptr, q.ptr, alpha=28.964, beta=18.02)
    out["h2o"] = q
    if "zenith_angle" in ds:
        cz = ds.work("d.coszen", (ncol,), ("*",), "dimensionless")
        ctx.elementwise("cos", ncol, ds["zenith_angle"].ptr, cz.ptr)
        out["coszen"] = cz
    ctx.order_streams(0)          # the longwave stream may start once these (and everything before them) are done
    ds._work["derived_vals"] = out
    ds._derived_ok = True
    return out


def _device_overlap(self, ds, which, inp):
    """cloud_overlap_method "exponential" / "exponential_random" on a DeviceState: the rank correlations from the resident
    pressure and temperature (rrtmg_hip_overlap_alpha with device pointers, on the main stream), copied into the context for
    this spectrum in stream order (rrtmg_hip_set_mcica_overlap_alpha) -- nothing leaves HBM."""
    if not getattr(self, "_exp_overlap", None):
        return
    from .rrtmg.common import rd_over_g
    nlay, ncol = inp["nlay"], inp["ncol"]
    alpha = ds.work(("d.overlap_alpha", which), (nlay, ncol), ("mid_levels", "*"), "dimensionless")
    ds.ctx.overlap_alpha(inp["play"], inp["tlay"], self._exp_overlap[1], rd_over_g(), out=alpha.ptr, memspace=1, ncol=ncol, nlay=nlay)
    ds.ctx.set_mcica_overlap_alpha(which, alpha.ptr, memspace=1, ncol=ncol, nlay=nlay)


def shortwave_device_call(self, ds, output_work=None):
    """RRTMGShortwave on a DeviceState: the body of array_call (sw/component.py:472-668) with device pointers.
    `output_work(key, shape, dims, units)`: the caller's own buffers for the outputs (climt_amd.IntermittentShortwave keeps a
    call's results across model steps); default: two alternating sets of the state's."""
    ds.init_tables("sw", self._Cpd)
    P = self.input_properties
    g = lambda n: ds.need(n, P[n]).ptr
    der = _derived(ds, P)
    nlay, ncol = ds["air_temperature"].shape
    day_of_year = 0 if self._ignore_day_of_year else ds["time"].timetuple().tm_yday
    inp = dict(
        ncol=ncol, nlay=nlay, play=g("air_pressure"), plev=g("air_pressure_on_interface_levels"), tlay=g("air_temperature"), tlev=der["tint"].ptr,
        tsfc=g("surface_temperature"), h2o=der["h2o"].ptr, o3=g("mole_fraction_of_ozone_in_air"), co2=g("mole_fraction_of_carbon_dioxide_in_air"),
        ch4=g("mole_fraction_of_methane_in_air"), n2o=g("mole_fraction_of_nitrous_oxide_in_air"), o2=g("mole_fraction_of_oxygen_in_air"),
        coszen=der["coszen"].ptr, cldfr=g("cloud_area_fraction_in_atmosphere_layer"),
        taucld=g("shortwave_optical_thickness_due_to_cloud"), ssacld=g("single_scattering_albedo_due_to_cloud"),
        asmcld=g("cloud_asymmetry_parameter"), fsfcld=g("cloud_forward_scattering_fraction"),
        cicewp=g("mass_content_of_cloud_ice_in_atmosphere_layer"), cliqwp=g("mass_content_of_cloud_liquid_water_in_atmosphere_layer"),
        reice=g("cloud_ice_particle_size"), reliq=g("cloud_water_droplet_radius"),
        tauaer=g("shortwave_optical_thickness_due_to_aerosol"), ssaaer=g("single_scattering_albedo_due_to_aerosol"),
        asmaer=g("aerosol_asymmetry_parameter"), ecaer=g("aerosol_optical_depth_at_55_micron"),
        bndsolvar=self._solar_var_by_band, indsolvar=self._fac_sunspot_coeff,
        icld=self._cloud_overlap, iaer=self._aerosol_type, inflg=self._cloud_optics, iceflg=self._ice_props, liqflg=self._liq_props,
        dyofyr=day_of_year, isolvar=self._solar_var_flag, scon=float(self._solar_const),
        adjes=ds.scalars["flux_adjustment_for_earth_sun_distance"], solcycfrac=ds.scalars["solar_cycle_fraction"])
    surface = None
    if getattr(self, "_spectral_albedo", False):      # the resident [band][column] arrays, read in place
        from .rrtmg.shortwave import SPECTRAL_ALBEDO_INPUTS
        surface = {m: g(k) for k, m in SPECTRAL_ALBEDO_INPUTS.items()}
    else:
        inp.update(asdir=g("surface_albedo_for_direct_shortwave"), asdif=g("surface_albedo_for_diffuse_shortwave"),
                   aldir=g("surface_albedo_for_direct_near_infrared"), aldif=g("surface_albedo_for_diffuse_near_infrared"))
    if self._mcica:
        if self._random_number_generator == 0:
            self._permute_seed = np.random.randint(0, 1024)
        elif self._random_number_generator == 1:
            self._permute_seed = np.random.randint(0, 2 ** 31 - 1)
        inp.update(irng=self._random_number_generator, permuteseed=self._permute_seed)
    il, ml = (nlay + 1, ncol), (nlay, ncol)
    self._device_calls = getattr(self, "_device_calls", 0) + 1          # outputs alternate between two buffer sets: the
    w = output_work or (lambda key, shape, dims, units: ds.work(("sw", id(self), key, self._device_calls & 1), shape, dims, units))   # state may still hold the last ones
    clear = getattr(self, "_clear_sky", True)      # False: no buffers for the three clear-sky outputs, which the library then leaves out
    fl = {k: w(k, il, ("interface_levels", "*"), "W m^-2") for k in (("swuflx", "swdflx", "swuflxc", "swdflxc") if clear else ("swuflx", "swdflx"))}
    hr = w("swhr", ml, ("mid_levels", "*"), "degK day^-1")
    out = {k: v.ptr for k, v in fl.items()}
    out.update(swhr=hr.ptr)
    if clear:
        hrc = w("swhrc", ml, ("mid_levels", "*"), "degK day^-1")
        out.update(swhrc=hrc.ptr)
    comps = None
    if getattr(self, "_flux_components", False):
        from .rrtmg.shortwave import FLUX_COMPONENT_DIAGNOSTICS
        comps = {c: w(c, il, ("interface_levels", "*"), "W m^-2") for c in FLUX_COMPONENT_DIAGNOSTICS.values()}
    bands = None
    if getattr(self, "_band_fluxes", False):
        from .rrtmg.shortwave import BAND_FLUX_DIAGNOSTICS
        bands = {b: w("band." + b, (14,) + il, ("num_shortwave_bands", "interface_levels", "*"), "W m^-2") for b in BAND_FLUX_DIAGNOSTICS.values()}
    self._apply_night_skip(ds.ctx)
    if getattr(self, "_skip_night", False):      # cos(zenith) with its night columns at 0.0 (RRTMGShortwave.night_coszen), same stream
        cz = ds.work("d.coszen.night", (ncol,), ("*",), "dimensionless")
        ds.ctx.elementwise("cosday", ncol, ds["zenith_angle"].ptr, cz.ptr)
        inp["coszen"] = cz.ptr
    _device_overlap(self, ds, "sw", inp)
    if comps or bands or surface:
        ds.ctx.sw_fluxes(inp, mcica=self._mcica, out=out, memspace=1, components={c: q.ptr for c, q in comps.items()} if comps else None,
                         bands={b: q.ptr for b, q in bands.items()} if bands else None, surface=surface)
    else:
        ds.ctx.sw_fluxes(inp, mcica=self._mcica, out=out, memspace=1)
    diagnostics = {"upwelling_shortwave_flux_in_air": fl["swuflx"], "downwelling_shortwave_flux_in_air": fl["swdflx"],
                   "air_temperature_tendency_from_shortwave": hr}
    if clear:
        diagnostics.update({"upwelling_shortwave_flux_in_air_assuming_clear_sky": fl["swuflxc"], "downwelling_shortwave_flux_in_air_assuming_clear_sky": fl["swdflxc"],
                            "air_temperature_tendency_from_shortwave_assuming_clear_sky": hrc})
    if comps:
        diagnostics.update({k: comps[c] for k, c in FLUX_COMPONENT_DIAGNOSTICS.items()})
    if bands:
        diagnostics.update({k: bands[b] for k, b in BAND_FLUX_DIAGNOSTICS.items()})
    return {"air_temperature": hr}, diagnostics


def longwave_device_call(self, ds, output_work=None):
    """RRTMGLongwave on a DeviceState: the body of array_call (lw/component.py:373-522) with device pointers.
    `output_work(key, shape, dims, units)`: the caller's own buffers for the outputs, the derivatives of idrv = 1 included
    (climt_amd.IntermittentLongwave keeps a call's results across model steps); default: two alternating sets of the state's."""
    ds.init_tables("lw", self._Cpd)
    P = self.input_properties
    g = lambda n: ds.need(n, P[n]).ptr
    der = _derived(ds, P)
    nlay, ncol = ds["air_temperature"].shape
    tlev = der["tint"].ptr if self._calc_Tint else g("air_temperature_on_interface_levels")
    inp = dict(
        ncol=ncol, nlay=nlay, play=g("air_pressure"), plev=g("air_pressure_on_interface_levels"), tlay=g("air_temperature"), tlev=tlev,
        tsfc=g("surface_temperature"), h2o=der["h2o"].ptr, o3=g("mole_fraction_of_ozone_in_air"), co2=g("mole_fraction_of_carbon_dioxide_in_air"),
        ch4=g("mole_fraction_of_methane_in_air"), n2o=g("mole_fraction_of_nitrous_oxide_in_air"), o2=g("mole_fraction_of_oxygen_in_air"),
        cfc11=g("mole_fraction_of_cfc11_in_air"), cfc12=g("mole_fraction_of_cfc12_in_air"), cfc22=g("mole_fraction_of_cfc22_in_air"),
        ccl4=g("mole_fraction_of_carbon_tetrachloride_in_air"), emis=g("surface_longwave_emissivity"),
        cldfr=g("cloud_area_fraction_in_atmosphere_layer"), taucld=g("longwave_optical_thickness_due_to_cloud"),
        cicewp=g("mass_content_of_cloud_ice_in_atmosphere_layer"), cliqwp=g("mass_content_of_cloud_liquid_water_in_atmosphere_layer"),
        reice=g("cloud_ice_particle_size"), reliq=g("cloud_water_droplet_radius"), tauaer=g("longwave_optical_thickness_due_to_aerosol"),
        icld=self._cloud_overlap, idrv=self._calc_dflxdt, inflg=self._cloud_optics, iceflg=self._ice_props, liqflg=self._liq_props)
    if self._mcica:
        if self._random_number_generator == 0:
            self._permute_seed = np.random.randint(0, 1024)
        elif self._random_number_generator == 1:
            self._permute_seed = np.random.randint(0, 2 ** 31 - 1)
        inp.update(irng=self._random_number_generator, permuteseed=self._permute_seed)
    il, ml = (nlay + 1, ncol), (nlay, ncol)
    self._device_calls = getattr(self, "_device_calls", 0) + 1
    w = output_work or (lambda key, shape, dims, units: ds.work(("lw", id(self), key, self._device_calls & 1), shape, dims, units))
    clear = getattr(self, "_clear_sky", True)      # False: no buffers for the clear-sky outputs, which the library then leaves out
    fl = {k: w(k, il, ("interface_levels", "*"), "W m^-2") for k in (("uflx", "dflx", "uflxc", "dflxc") if clear else ("uflx", "dflx"))}
    hr = w("hr", ml, ("mid_levels", "*"), "degK day^-1")
    out = {k: v.ptr for k, v in fl.items()}
    out.update(hr=hr.ptr)
    if clear:
        hrc = w("hrc", ml, ("mid_levels", "*"), "degK day^-1")
        out.update(hrc=hrc.ptr)
    if self._calc_dflxdt:
        du = w("duflx_dt", il, ("interface_levels", "*"), "W m^-2 K^-1")
        duc = w("duflxc_dt", il, ("interface_levels", "*"), "W m^-2 K^-1") if clear else None
        out.update(duflx_dt=du.ptr)
        if clear:
            out.update(duflxc_dt=duc.ptr)
        self.change_in_upward_flux_with_surface_temperature, self.change_in_clear_sky_upward_flux_with_surface_temperature = du, duc
    bands = None
    if getattr(self, "_band_fluxes", False):
        from .rrtmg.longwave import BAND_FLUX_DIAGNOSTICS
        names = getattr(self, "_band_names", tuple(BAND_FLUX_DIAGNOSTICS))
        bands = {BAND_FLUX_DIAGNOSTICS[k]: w("band." + BAND_FLUX_DIAGNOSTICS[k], (16,) + il, ("num_longwave_bands", "interface_levels", "*"), "W m^-2") for k in names}
    self._apply_clear_sky(ds.ctx)
    _device_overlap(self, ds, "lw", inp)
    if bands:
        ds.ctx.lw_fluxes(inp, mcica=self._mcica, out=out, memspace=1, bands={b: q.ptr for b, q in bands.items()})
    else:
        ds.ctx.lw_fluxes(inp, mcica=self._mcica, out=out, memspace=1)
    ds._lw_inflight = True      # consumers on the main stream (tendency sum, slab, the next derived fields) join first: join_streams()
    diagnostics = {"upwelling_longwave_flux_in_air": fl["uflx"], "downwelling_longwave_flux_in_air": fl["dflx"],
                   "air_temperature_tendency_from_longwave": hr}
    if clear:
        diagnostics.update({"upwelling_longwave_flux_in_air_assuming_clear_sky": fl["uflxc"], "downwelling_longwave_flux_in_air_assuming_clear_sky": fl["dflxc"],
                            "air_temperature_tendency_from_longwave_assuming_clear_sky": hrc})
    if bands:
        diagnostics.update({k: bands[b] for k, b in BAND_FLUX_DIAGNOSTICS.items() if b in bands})
    return {"air_temperature": hr}, diagnostics


def instellation_device_call(self, ds):
    """Instellation on a DeviceState: latitude / longitude resident, time arithmetic on the host (component.py:64-82)."""
    from .instellation import days_from_2000
    lat, lon = ds.need("latitude", self.input_properties["latitude"]), ds.need("longitude", self.input_properties["longitude"])
    self._device_calls = getattr(self, "_device_calls", 0) + 1
    zen = ds.work(("sun", id(self), self._device_calls & 1), (ds.ncol,), ("*",), "radians")
    ds.ctx.zenith_angle(lat.ptr, lon.ptr, days_from_2000(ds["time"]) / 36525.0, out=zen.ptr, memspace=1, ncol=ds.ncol)
    return {"zenith_angle": zen}


def instellation_interval_device_call(self, ds, timedelta, work=None):
    """Instellation.interval_mean on a DeviceState (rrtmg_hip_mean_coszen with device pointers, on the main stream) ->
    zenith_angle, sunlit_fraction and, for climt_amd.IntermittentShortwave, coszen_mean and insolation (mean * fraction).
    `work(key, shape, dims, units)`: where the four outputs live; default: two alternating sets of the state's own."""
    from .instellation import interval_centuries
    lat, lon = ds.need("latitude", self.input_properties["latitude"]), ds.need("longitude", self.input_properties["longitude"])
    if work is None:
        self._interval_calls = getattr(self, "_interval_calls", 0) + 1
        work = lambda key, shape, dims, units: ds.work(("sun.interval", id(self), key, self._interval_calls & 1), shape, dims, units)
    out = {k: work(k, (ds.ncol,), ("*",), u) for k, u in (("zenith_angle", "radians"), ("sunlit_fraction", "dimensionless"),
                                                         ("coszen_mean", "dimensionless"), ("insolation", "dimensionless"))}
    ds.ctx.mean_coszen(lat.ptr, lon.ptr, *interval_centuries(ds["time"], timedelta), out_mean=out["coszen_mean"].ptr,
                       out_fraction=out["sunlit_fraction"].ptr, memspace=1, ncol=ds.ncol, out_zenith=out["zenith_angle"].ptr,
                       out_insolation=out["insolation"].ptr)
    return out


def slab_device_call(self, ds):
    """SlabSurface on a DeviceState: rrtmg_hip_slab_surface reads the SURFACE ROW of the [level][column] radiation outputs in place."""
    names = dict(sw_down="downwelling_shortwave_flux_in_air", lw_down="downwelling_longwave_flux_in_air", sw_up="upwelling_shortwave_flux_in_air",
                 lw_up="upwelling_longwave_flux_in_air", lh="surface_upward_latent_heat_flux", sh="surface_upward_sensible_heat_flux",
                 up_heat_soil="upward_heat_flux_at_ground_level_in_soil", heat_flux_sea_ice="heat_flux_into_sea_water_due_to_sea_ice",
                 sea_water_dens="sea_water_density", surf_dens="surface_material_density", heat_cap_soil="heat_capacity_of_soil",
                 surf_therm_cap="surface_thermal_capacity", ocean_mix_thick="ocean_mixed_layer_thickness", soil_layer_thick="soil_layer_thickness",
                 ocean_heat_transport="ocean_heat_transport_convergence")
    ds.join_streams()      # the longwave fluxes in the state may be this step's
    ptrs = {}
    for k in SLAB_IN:
        q = ds[names[k]]
        if names[k] in _SURFACE_ROW:
            if q.dims[0] != "interface_levels":      # uploaded from the host in the slab's own ['*', 'interface_levels'] layout
                raise ValueError("%s must be resident as [interface_levels][*] (a radiation output) for the in-place surface row" % names[k])
        ptrs[k] = q.ptr                               # row 0 = the surface
    self._device_calls = getattr(self, "_device_calls", 0) + 1
    tend = ds.work(("slab", id(self), "tend", self._device_calls & 1), (ds.ncol,), ("*",), "degK s^-1")
    depth = ds.work(("slab", id(self), "depth", self._device_calls & 1), (ds.ncol,), ("*",), "m")
    ds.ctx.slab_surface_device(ds.ncol, ptrs, ds["area_type"].ptr, tend.ptr, depth.ptr)
    return {"surface_temperature": tend}, {"depth_of_slab_surface": depth, "ocean_heat_transport_convergence": ds["ocean_heat_transport_convergence"]}


def _one_pressure_unit(p, pi):
    if not _same_units(p.units, pi.units):
        raise ValueError("air_pressure is resident in %r, air_pressure_on_interface_levels in %r" % (p.units, pi.units))


def _resident_pressures(ds, who, surface=False):
    """air_pressure and air_pressure_on_interface_levels (with `surface`: and surface_air_pressure) for a column component, as
    they are resident -- in the units of whichever component asked for them first: [mid_levels][*] and [interface_levels][*] in
    the same units (and [*]).  (The convection scheme names the quantity that is resident otherwise: it checks the dims itself.)"""
    got = [ds[n] for n in ("air_pressure", "air_pressure_on_interface_levels") + (("surface_air_pressure",) if surface else ())]
    if any(tuple(x.dims) != dims for x, dims in zip(got, (("mid_levels", "*"), ("interface_levels", "*"), ("*",)))):
        raise ValueError("the pressures are resident as %s and %s, %s wants [levels][*]%s" % (
            ", ".join(str(x.dims) for x in got[:-1]), got[-1].dims, who, " and [*]" if surface else ""))
    _one_pressure_unit(got[0], got[1])
    return got


def _step_work(self, ds, prefix, ncol):
    """-> work(key, units, like=None, dtype): a column component's work buffer of this step, [ncol] or of the shape and dims of
    `like`.  The buffers alternate with the step count, so the arrays the state held before the step stay what they were."""
    slot = ds.step_count & 1

    def work(key, units, like=None, dtype=np.float64):
        shape, dims = ((ncol,), ("*",)) if like is None else (like.shape, like.dims)
        return ds.work((prefix, id(self), key, slot), shape, dims, units, dtype)
    return work


def dry_adjustment_device_call(self, ds, timestep=None):
    """DryConvectiveAdjustment on a DeviceState: rrtmg_hip_dry_adjustment with device pointers on the main stream.  The
    pressures are read as they are resident -- in the units of whichever component asked for them first; only ratios and
    differences of pressures enter, so the reference pressure is brought to THEIR units on the host.  The adjusted temperature
    and humidity go to work buffers that alternate with the step count (the state's previous arrays stay what they were), and
    the state is rebound to them: -> ({}, the same state)."""
    P = self.input_properties
    t, q = ds.need("air_temperature", P["air_temperature"]), ds.need("specific_humidity", P["specific_humidity"])
    p, pi = _resident_pressures(ds, "the adjustment")
    nlay, ncol = t.shape
    if p.shape != (nlay, ncol) or pi.shape != (nlay + 1, ncol) or q.shape != (nlay, ncol):
        raise ValueError("temperature %s, humidity %s and pressures %s, %s do not belong to one grid" % (t.shape, q.shape, p.shape, pi.shape))
    ds.join_streams()      # a longwave still in flight belongs to the step this adjustment closes
    work = _step_work(self, ds, "dry", ncol)
    t_new, q_new = work("t", t.units, like=t), work("q", q.units, like=q)
    ds.ctx.dry_adjustment(t.ptr, q.ptr, p.ptr, pi.ptr, self.constants(p.units), t_out=t_new.ptr, q_out=q_new.ptr, memspace=1, ncol=ncol, nlay=nlay)
    ds["air_temperature"], ds["specific_humidity"] = t_new, q_new
    return {}, ds


def boundary_layer_device_call(self, ds, timestep):
    """SimpleBoundaryLayer on a DeviceState: rrtmg_hip_boundary_layer with device pointers on the main stream.  The pressures are
    read as they are resident -- in the units of whichever component asked for them first; the rule needs Pa (densities), so the
    library multiplies every pressure it reads by `pressure_scale` / `ps_scale`, Pa per resident unit: the one rounding the unit
    conversion of the host path makes.  The four new profiles go to work buffers that alternate with the step count (the
    state's previous arrays stay what they were) and the state is rebound to them; the diagnostics go to [ncol] work buffers,
    which SlabSurface's device call can read as its flux inputs: -> (diagnostics as DeviceQuantity, the same state)."""
    P = self.input_properties
    names = ("air_temperature", "specific_humidity", "eastward_wind", "northward_wind")
    t, q, u, v = (ds.need(n, P[n]) for n in names)
    ts, qs = ds.need("surface_temperature", P["surface_temperature"]), ds.need("surface_specific_humidity", P["surface_specific_humidity"])
    p, pi, ps = _resident_pressures(ds, "the boundary layer", surface=True)
    nlay, ncol = t.shape
    if any(x.shape != (nlay, ncol) for x in (q, u, v, p)) or pi.shape != (nlay + 1, ncol) or any(x.shape != (ncol,) for x in (ps, ts, qs)):
        raise ValueError("temperature %s, humidity %s, winds %s, %s, pressures %s, %s and surface values %s, %s, %s do not belong to one grid" % (
            t.shape, q.shape, u.shape, v.shape, p.shape, pi.shape, ps.shape, ts.shape, qs.shape))
    fluxes = {}
    if self._flux_mode == 2:
        sh, lh = (ds.need(n, P[n]) for n in ("surface_upward_sensible_heat_flux", "surface_upward_latent_heat_flux"))
        if sh.shape != (ncol,) or lh.shape != (ncol,):
            raise ValueError("the prescribed surface fluxes %s, %s do not belong to the grid of %d columns" % (sh.shape, lh.shape, ncol))
        fluxes = dict(sh_in=sh.ptr, lh_in=lh.ptr)
    ds.join_streams()      # a longwave still in flight belongs to the step this component closes
    col = _step_work(self, ds, "bl", ncol)
    new = [col(n, x.units, like=x) for n, x in zip(names, (t, q, u, v))]
    d = dict(stress_north=col("stress_north", "Pa"), stress_east=col("stress_east", "Pa"), height=col("height", "m"))
    if self._flux_mode == 1:
        d.update(sh_out=col("sh", "W m^-2"), lh_out=col("lh", "W m^-2"))
    to_pa = lambda units: float(_convert(np.float64(1.0), units, "Pa"))
    ds.ctx.boundary_layer(t.ptr, q.ptr, u.ptr, v.ptr, p.ptr, pi.ptr, ps.ptr, ts.ptr, qs.ptr, timestep.total_seconds(), self.constants(),
                          self._flux_mode, t_out=new[0].ptr, q_out=new[1].ptr, u_out=new[2].ptr, v_out=new[3].ptr,
                          diagnostics={k: x.ptr for k, x in d.items()}, pressure_scale=to_pa(p.units), ps_scale=to_pa(ps.units),
                          memspace=1, ncol=ncol, nlay=nlay, **fluxes)
    ds.update(zip(names, new))
    diagnostics = {"northward_wind_stress": d["stress_north"], "eastward_wind_stress": d["stress_east"], "boundary_layer_height": d["height"]}
    if self._flux_mode == 1:
        diagnostics.update(surface_upward_sensible_heat_flux=d["sh_out"], surface_upward_latent_heat_flux=d["lh_out"])
    return diagnostics, ds


def emanuel_device_call(self, ds, timestep):
    """EmanuelConvection on a DeviceState: rrtmg_hip_emanuel_convection with device pointers on the main stream.  The profiles are
    read as they are resident, [levels][*]; the pressures in the units of whichever component asked for them first -- the rule
    needs hPa, so the library multiplies every pressure it reads by `pressure_scale`, hPa per resident unit: the one rounding the
    unit conversion of the host path makes.  The saturation humidity is formed by the kernel.  Tendencies and diagnostics go to
    work buffers that alternate with the step count and stay in HBM; cloud_base_mass_flux is rebound to the new array, as a
    model script does with state.update(diagnostics): -> (tendencies, diagnostics) as DeviceQuantity."""
    names = ("air_temperature", "specific_humidity", "eastward_wind", "northward_wind")
    P = self.input_properties
    t, q, u, v = (ds[n] for n in names)
    p, pi, cb = ds["air_pressure"], ds["air_pressure_on_interface_levels"], ds.need("cloud_base_mass_flux", P["cloud_base_mass_flux"])
    for n, x in zip(names + ("air_pressure",), (t, q, u, v, p)):
        if tuple(x.dims) != ("mid_levels", "*"):
            raise ValueError("quantity %r is resident as %s, the convection scheme wants [mid_levels][*]" % (n, x.dims))
    for n, x in zip(names, (t, q, u, v)):
        if not _same_units(x.units, P[n]["units"]):
            raise ValueError("quantity %r is resident in %r, component wants %r" % (n, x.units, P[n]["units"]))
    if tuple(pi.dims) != ("interface_levels", "*"):
        raise ValueError("air_pressure_on_interface_levels is resident as %s, the convection scheme wants [interface_levels][*]" % (pi.dims,))
    _one_pressure_unit(p, pi)
    nlay, ncol = t.shape
    if any(x.shape != (nlay, ncol) for x in (q, u, v, p)) or pi.shape != (nlay + 1, ncol) or cb.shape != (ncol,):
        raise ValueError("temperature %s, humidity %s, winds %s, %s, pressures %s, %s and mass flux %s do not belong to one grid" % (
            t.shape, q.shape, u.shape, v.shape, p.shape, pi.shape, cb.shape))
    ds.join_streams()      # a longwave still in flight may be reading the profiles' neighbours on its own stream; the sums follow on the main one
    work = _step_work(self, ds, "emanuel", ncol)
    T = self.tendency_properties
    tend = {n: work(n, T[n]["units"], like=t) for n in names}
    D = self.diagnostic_properties
    col = lambda key, name, dtype=np.float64: work(key, D[name]["units"], dtype=dtype)
    d = dict(precip=col("precip", "convective_precipitation_rate"), wd=col("wd", "convective_downdraft_velocity_scale"),
             tprime=col("tprime", "convective_downdraft_temperature_scale"), qprime=col("qprime", "convective_downdraft_specific_humidity_scale"),
             cape=col("cape", "atmosphere_convective_available_potential_energy"), iflag=col("iflag", "convective_state", np.int32),
             ft_per_day=work("ft_per_day", "degK day^-1", like=t))
    cb_new = col("cbmf", "cloud_base_mass_flux")
    ds.ctx.emanuel_convection(t.ptr, q.ptr, u.ptr, v.ptr, p.ptr, pi.ptr, cb.ptr, timestep.total_seconds(), self.parameters(), self.constants(),
                              ft=tend[names[0]].ptr, fq=tend[names[1]].ptr, fu=tend[names[2]].ptr, fv=tend[names[3]].ptr, cbmf_out=cb_new.ptr,
                              diagnostics={k: x.ptr for k, x in d.items()}, pressure_scale=float(_convert(np.float64(1.0), p.units, "hPa")),
                              memspace=1, ncol=ncol, nlay=nlay)
    ds["cloud_base_mass_flux"] = cb_new
    diagnostics = {"convective_state": d["iflag"], "convective_precipitation_rate": d["precip"], "convective_downdraft_velocity_scale": d["wd"],
                   "convective_downdraft_temperature_scale": d["tprime"], "convective_downdraft_specific_humidity_scale": d["qprime"],
                   "cloud_base_mass_flux": cb_new, "atmosphere_convective_available_potential_energy": d["cape"],
                   "air_temperature_tendency_from_convection": d["ft_per_day"]}
    return tend, diagnostics


def simple_physics_device_call(self, ds, timestep):
    """SimplePhysics on a DeviceState: rrtmg_hip_simple_physics with device pointers on the main stream.  The pressures are read
    as they are resident -- in the units of whichever component asked for them first; the rule needs Pa (saturation, densities,
    the top of the boundary layer), so the library multiplies every pressure it reads by `pressure_scale` / `ps_scale`, Pa per
    resident unit: the one rounding the unit conversion of the host path makes.  The four new profiles go to work buffers that
    alternate with the step count (the state's previous arrays stay what they were) and the state is rebound to them; the three
    diagnostics go to [ncol] work buffers, which SlabSurface's device call can read as its flux inputs:
    -> (diagnostics as DeviceQuantity, the same state)."""
    P = self.input_properties
    names = ("air_temperature", "specific_humidity", "eastward_wind", "northward_wind")
    t, q, u, v = (ds.need(n, P[n]) for n in names)
    ts, qsurf, lat = (ds.need(n, P[n]) for n in ("surface_temperature", "surface_specific_humidity", "latitude"))
    p, pi, ps = _resident_pressures(ds, "the simple physics", surface=True)
    nlay, ncol = t.shape
    if any(x.shape != (nlay, ncol) for x in (q, u, v, p)) or pi.shape != (nlay + 1, ncol) or any(x.shape != (ncol,) for x in (ps, ts, qsurf, lat)):
        raise ValueError("temperature %s, humidity %s, winds %s, %s, pressures %s, %s and surface values %s, %s, %s, %s do not belong to one grid" % (
            t.shape, q.shape, u.shape, v.shape, p.shape, pi.shape, ps.shape, ts.shape, qsurf.shape, lat.shape))
    ds.join_streams()      # a longwave still in flight belongs to the step this component closes
    col = _step_work(self, ds, "sp", ncol)
    new = [col(n, x.units, like=x) for n, x in zip(names, (t, q, u, v))]
    d = dict(precl=col("precl", "m s^-1"), sh_out=col("sh", "W m^-2"), lh_out=col("lh", "W m^-2"))
    to_pa = lambda units: float(_convert(np.float64(1.0), units, "Pa"))
    ds.ctx.simple_physics(t.ptr, q.ptr, u.ptr, v.ptr, p.ptr, pi.ptr, ps.ptr, timestep.total_seconds(), self.constants(), self.switches(),
                          ts=ts.ptr, qsurf=qsurf.ptr, lat=lat.ptr, t_out=new[0].ptr, q_out=new[1].ptr, u_out=new[2].ptr, v_out=new[3].ptr,
                          diagnostics={k: x.ptr for k, x in d.items()}, pressure_scale=to_pa(p.units), ps_scale=to_pa(ps.units),
                          memspace=1, ncol=ncol, nlay=nlay)
    ds.update(zip(names, new))
    return {"stratiform_precipitation_rate": d["precl"], "surface_upward_sensible_heat_flux": d["sh_out"],
            "surface_upward_latent_heat_flux": d["lh_out"]}, ds


def _to_pa(units):
    return float(_convert(np.float64(1.0), units, "Pa"))


def _gray_surface(ds, who, nlev, ncol):
    """-> (air_pressure_on_interface_levels, surface_air_pressure, latitude) as they are resident, for the Frierson optical depth:
    [interface_levels][*] and [*]; the pressures in any pressure unit (the library scales them), the latitude in degrees north
    under either of the names the components use for that unit."""
    pi, ps, lat = (ds.get(n) for n in ("air_pressure_on_interface_levels", "surface_air_pressure", "latitude"))
    for n, x in zip(("air_pressure_on_interface_levels", "surface_air_pressure", "latitude"), (pi, ps, lat)):
        if x is None:
            raise KeyError("device state is missing input quantity %r" % n)
    if tuple(pi.dims) != ("interface_levels", "*") or tuple(ps.dims) != ("*",) or tuple(lat.dims) != ("*",):
        raise ValueError("the interface pressures, the surface pressure and the latitude are resident as %s, %s and %s, %s wants [interface_levels][*], [*] and [*]" % (
            pi.dims, ps.dims, lat.dims, who))
    if float(_convert(np.float64(1.0), lat.units, "degrees_N")) != 1.0:
        raise ValueError("quantity 'latitude' is resident in %r, component wants 'degrees_N'" % lat.units)
    if pi.shape != (nlev, ncol) or ps.shape != (ncol,) or lat.shape != (ncol,):
        raise ValueError("interface pressures %s, surface pressure %s and latitude %s do not belong to one grid of %d interfaces by %d columns" % (
            pi.shape, ps.shape, lat.shape, nlev, ncol))
    return pi, ps, lat


def frierson_device_call(self, ds):
    """Frierson06LongwaveOpticalDepth on a DeviceState: rrtmg_hip_frierson_optical_depth with device pointers on the main stream.
    The pressures are read as they are resident (only the ratio pint / ps enters; the library brings both to Pa).  The depth goes
    to one of two alternating work buffers: -> diagnostics as DeviceQuantity."""
    pi = ds.get("air_pressure_on_interface_levels")
    if pi is None:
        raise KeyError("device state is missing input quantity 'air_pressure_on_interface_levels'")
    nlev, ncol = pi.shape if len(pi.shape) == 2 else (0, 0)
    pi, ps, lat = _gray_surface(ds, "the optical depth", nlev, ncol)
    self._device_calls = getattr(self, "_device_calls", 0) + 1
    tau = ds.work(("frierson", id(self), self._device_calls & 1), (nlev, ncol), ("interface_levels", "*"), "dimensionless")
    ds.ctx.frierson_optical_depth(pi.ptr, ps.ptr, lat.ptr, self.parameters(), tau=tau.ptr, pressure_scale=_to_pa(pi.units), ps_scale=_to_pa(ps.units),
                                  memspace=1, ncol=ncol, nlay=nlev - 1)
    return {"longwave_optical_depth_on_interface_levels": tau}


def gray_longwave_device_call(self, ds):
    """GrayLongwaveRadiation on a DeviceState: rrtmg_hip_gray_longwave with device pointers on the main stream; the fluxes, the
    tendency and the heating rate go to two alternating sets of work buffers and stay in HBM (the fluxes [interface_levels][*], as
    SlabSurface's device call reads them).  With `optical_depth` the fused call: the depth is formed inside the sweep from the
    resident pressures and latitude and is a diagnostic.  The interface pressures are read as they are resident; the library
    brings them to Pa.  -> (tendencies, diagnostics) as DeviceQuantity."""
    P = self.input_properties
    t, ts = ds.need("air_temperature", P["air_temperature"]), ds.need("surface_temperature", P["surface_temperature"])
    nlay, ncol = t.shape
    fused = self._optical_depth is not None
    if fused:
        pi, ps, lat = _gray_surface(ds, "the gray longwave", nlay + 1, ncol)
    else:
        pi = ds.get("air_pressure_on_interface_levels")
        tau = ds.need("longwave_optical_depth_on_interface_levels", P["longwave_optical_depth_on_interface_levels"])
        if pi is None:
            raise KeyError("device state is missing input quantity 'air_pressure_on_interface_levels'")
        if tuple(pi.dims) != ("interface_levels", "*"):
            raise ValueError("air_pressure_on_interface_levels is resident as %s, the gray longwave wants [interface_levels][*]" % (pi.dims,))
        if pi.shape != (nlay + 1, ncol) or tau.shape != (nlay + 1, ncol):
            raise ValueError("temperature %s, interface pressures %s and optical depth %s do not belong to one grid" % (t.shape, pi.shape, tau.shape))
    if ts.shape != (ncol,):
        raise ValueError("temperature %s and surface temperature %s do not belong to one grid" % (t.shape, ts.shape))
    self._device_calls = getattr(self, "_device_calls", 0) + 1
    w = lambda key, shape, dims, units: ds.work(("gray", id(self), key, self._device_calls & 1), shape, dims, units)
    il, ml = (nlay + 1, ncol), (nlay, ncol)
    up, dn = (w(k, il, ("interface_levels", "*"), "W m^-2") for k in ("up", "dn"))
    tend, hr = w("tend", ml, ("mid_levels", "*"), "degK s^-1"), w("hr", ml, ("mid_levels", "*"), "degK day^-1")
    d = dict(hr=hr.ptr)
    kw = dict(up=up.ptr, dn=dn.ptr, tend=tend.ptr, pressure_scale=_to_pa(pi.units), memspace=1, ncol=ncol, nlay=nlay)
    if fused:
        depth = w("tau", il, ("interface_levels", "*"), "dimensionless")
        d.update(tau_out=depth.ptr)
        ds.ctx.gray_longwave(t.ptr, ts.ptr, pi.ptr, self.constants(), ps=ps.ptr, lat=lat.ptr, frierson=self._optical_depth.parameters(), diagnostics=d,
                             ps_scale=_to_pa(ps.units), **kw)
    else:
        ds.ctx.gray_longwave(t.ptr, ts.ptr, pi.ptr, self.constants(), tau=tau.ptr, diagnostics=d, **kw)
    diagnostics = {"upwelling_longwave_flux_in_air": up, "downwelling_longwave_flux_in_air": dn, "air_temperature_tendency_from_longwave": hr}
    if fused:
        diagnostics["longwave_optical_depth_on_interface_levels"] = depth
    return {"air_temperature": tend}, diagnostics


def cork_longwave_device_call(self, ds):
    """CorkLongwaveRadiation on a DeviceState: rrtmg_hip_cork_longwave with device pointers on the main stream and the component's
    table resident on the state's context.  The two pressures are read as they are resident, in one unit (Pa or any other: the
    library brings them to Pa); the gases, the emissivity [num_longwave_bands][*] and the cloud depth [mid_levels][*]
    [num_longwave_bands] as the component's properties state them.  The fluxes, the tendency and the diagnostics go to two
    alternating sets of work buffers and stay in HBM; the per-band ones are [num_longwave_bands][levels][*], the layout of the
    RRTMG per-band fluxes.  -> (tendencies, diagnostics) as DeviceQuantity."""
    P = self.input_properties
    t, ts = ds.need("air_temperature", P["air_temperature"]), ds.need("surface_temperature", P["surface_temperature"])
    nlay, ncol = t.shape
    nband = self.num_longwave_bands
    p, pi = ds.get("air_pressure"), ds.get("air_pressure_on_interface_levels")
    for n, x, dims in (("air_pressure", p, ("mid_levels", "*")), ("air_pressure_on_interface_levels", pi, ("interface_levels", "*"))):
        if x is None:
            raise KeyError("device state is missing input quantity %r" % n)
        if tuple(x.dims) != dims:
            raise ValueError("quantity %r is resident as %s, the correlated-k longwave wants %s" % (n, x.dims, dims))
    if _to_pa(p.units) != _to_pa(pi.units):
        raise ValueError("air_pressure is resident in %r and air_pressure_on_interface_levels in %r: the correlated-k longwave wants one unit" % (p.units, pi.units))
    emis = ds.need("surface_longwave_emissivity", P["surface_longwave_emissivity"])
    cloud = ds.need("longwave_optical_thickness_due_to_cloud", P["longwave_optical_thickness_due_to_cloud"])
    gases = [None if n is None else ds.need(n, P[n]) for n in self.gas_inputs()]
    if (p.shape != (nlay, ncol) or pi.shape != (nlay + 1, ncol) or ts.shape != (ncol,) or emis.shape != (nband, ncol) or cloud.shape != (nlay, ncol, nband)
            or any(g is not None and g.shape != (nlay, ncol) for g in gases)):
        raise ValueError("temperature %s, pressures %s, %s, surface temperature %s, emissivity %s, cloud depth %s and gases %s do not belong to one grid of %d bands" % (
            t.shape, p.shape, pi.shape, ts.shape, emis.shape, cloud.shape, [None if g is None else g.shape for g in gases], nband))
    if ds.ctx is not self._ctx:      # the table lives on the context that runs the call
        if getattr(self, "_handle_ctx", None) is not ds.ctx:
            self._handle_ds, self._handle_ctx = self._ktable.upload(ds.ctx), ds.ctx
        handle = self._handle_ds
    else:
        handle = self.table_handle()
    self._device_calls = getattr(self, "_device_calls", 0) + 1
    w = lambda key, shape, dims, units: ds.work(("cork", id(self), key, self._device_calls & 1), shape, dims, units)
    il, ml = ("interface_levels", "*"), ("mid_levels", "*")
    up, dn = (w(k, (nlay + 1, ncol), il, "W m^-2") for k in ("up", "dn"))
    tend, hr = w("tend", (nlay, ncol), ml, "degK s^-1"), w("hr", (nlay, ncol), ml, "degK day^-1")
    band = ("num_longwave_bands",)
    ub, db = (w(k, (nband, nlay + 1, ncol), band + il, "W m^-2") for k in ("up_band", "dn_band"))
    tb, trb = (w(k, (nband, nlay, ncol), band + ml, "dimensionless") for k in ("tau_band", "trans_band"))
    hb = w("hr_band", (nband, nlay, ncol), band + ml, "degK day^-1")
    ds.ctx.cork_longwave(handle, nband, t.ptr, p.ptr, pi.ptr, ts.ptr, emis.ptr, self.constants(), self._ktable.gas_rule,
                         gases=[None if g is None else g.ptr for g in gases], gas_scale=self._ktable.gas_scale, taucld=cloud.ptr, up=up.ptr, dn=dn.ptr, tend=tend.ptr,
                         diagnostics=dict(hr=hr.ptr, up_band=ub.ptr, dn_band=db.ptr, tau_band=tb.ptr, trans_band=trb.ptr, hr_band=hb.ptr),
                         pressure_scale=_to_pa(p.units), memspace=1, ncol=ncol, nlay=nlay)
    return {"air_temperature": tend}, {
        "upwelling_longwave_flux_in_air": up, "downwelling_longwave_flux_in_air": dn, "upwelling_longwave_flux_in_air_per_band": ub,
        "downwelling_longwave_flux_in_air_per_band": db, "air_temperature_tendency_from_longwave": hr, "longwave_optical_depth_per_band": tb,
        "longwave_transmittance_per_band": trb, "air_temperature_tendency_from_longwave_per_band": hb}


def cork_shortwave_device_call(self, ds):
    """CorkShortwaveRadiation on a DeviceState: rrtmg_hip_cork_shortwave with device pointers on the main stream and the
    component's table resident on the state's context.  The two pressures are read as they are resident, in one unit (Pa or any
    other: the library brings them to Pa); the zenith angle, the albedo and the earth-sun factor [*] (the factor of the first
    column scales every column, formed on the device: nothing comes to the host), the gases and the three cloud arrays
    [mid_levels][*][num_shortwave_bands] as the component's properties state them.  The fluxes, the tendency and the diagnostics
    go to two alternating sets of work buffers and stay in HBM; the per-band ones are [num_shortwave_bands][levels][*].
    A DeviceState keeps a quantity in the units of the FIRST component of from_host's list that asks for it: beside a component
    that takes one unit only (RRTMG's: mbar), list that one before this one -- this call reads the pressures in whatever one unit
    it finds, the other would refuse Pa (examples/radiative_convective.py orders its list so).
    -> (tendencies, diagnostics) as DeviceQuantity."""
    P = self.input_properties
    t = ds.need("air_temperature", P["air_temperature"])
    nlay, ncol = t.shape
    nband = self.num_shortwave_bands
    p, pi = ds.get("air_pressure"), ds.get("air_pressure_on_interface_levels")
    for n, x, dims in (("air_pressure", p, ("mid_levels", "*")), ("air_pressure_on_interface_levels", pi, ("interface_levels", "*"))):
        if x is None:
            raise KeyError("device state is missing input quantity %r" % n)
        if tuple(x.dims) != dims:
            raise ValueError("quantity %r is resident as %s, the correlated-k shortwave wants %s" % (n, x.dims, dims))
    if _to_pa(p.units) != _to_pa(pi.units):
        raise ValueError("air_pressure is resident in %r and air_pressure_on_interface_levels in %r: the correlated-k shortwave wants one unit" % (p.units, pi.units))
    columns = [ds.need(n, P[n]) for n in ("zenith_angle", "surface_albedo_for_direct_shortwave", "flux_adjustment_for_earth_sun_distance")]
    cloud = [ds.need(n, P[n]) for n in ("shortwave_optical_thickness_due_to_cloud", "single_scattering_albedo_due_to_cloud", "cloud_asymmetry_parameter")]
    gases = [None if n is None else ds.need(n, P[n]) for n in self.gas_inputs()]
    if (p.shape != (nlay, ncol) or pi.shape != (nlay + 1, ncol) or any(x.shape != (ncol,) for x in columns) or any(x.shape != (nlay, ncol, nband) for x in cloud)
            or any(g is not None and g.shape != (nlay, ncol) for g in gases)):
        raise ValueError("temperature %s, pressures %s, %s, zenith, albedo and earth-sun factor %s, cloud arrays %s and gases %s do not belong to one grid of %d bands" % (
            t.shape, p.shape, pi.shape, [x.shape for x in columns], [x.shape for x in cloud], [None if g is None else g.shape for g in gases], nband))
    if ds.ctx is not self._ctx:      # the table lives on the context that runs the call
        if getattr(self, "_handle_ctx", None) is not ds.ctx:
            self._handle_ds, self._handle_ctx = self._ktable.upload(ds.ctx), ds.ctx
        handle = self._handle_ds
    else:
        handle = self.table_handle()
    self._device_calls = getattr(self, "_device_calls", 0) + 1
    w = lambda key, shape, dims, units: ds.work(("cork_sw", id(self), key, self._device_calls & 1), shape, dims, units)
    il, ml = ("interface_levels", "*"), ("mid_levels", "*")
    up, dn = (w(k, (nlay + 1, ncol), il, "W m^-2") for k in ("up", "dn"))
    tend, hr = w("tend", (nlay, ncol), ml, "degK s^-1"), w("hr", (nlay, ncol), ml, "degK day^-1")
    band = ("num_shortwave_bands",)
    ub, db = (w(k, (nband, nlay + 1, ncol), band + il, "W m^-2") for k in ("up_band", "dn_band"))
    tb = w("tau_band", (nband, nlay, ncol), band + ml, "dimensionless")
    hb = w("hr_band", (nband, nlay, ncol), band + ml, "degK day^-1")
    ds.ctx.cork_shortwave(handle, nband, t.ptr, p.ptr, pi.ptr, columns[0].ptr, columns[1].ptr, columns[2].ptr, self.constants(), self._ktable.gas_rule,
                          gases=[None if g is None else g.ptr for g in gases], gas_scale=self._ktable.gas_scale, cloud=tuple(x.ptr for x in cloud),
                          up=up.ptr, dn=dn.ptr, tend=tend.ptr, diagnostics=dict(hr=hr.ptr, up_band=ub.ptr, dn_band=db.ptr, tau_band=tb.ptr, hr_band=hb.ptr),
                          pressure_scale=_to_pa(p.units), memspace=1, ncol=ncol, nlay=nlay)
    return {"air_temperature": tend}, {
        "upwelling_shortwave_flux_in_air": up, "downwelling_shortwave_flux_in_air": dn, "upwelling_shortwave_flux_in_air_per_band": ub,
        "downwelling_shortwave_flux_in_air_per_band": db, "air_temperature_tendency_from_shortwave": hr, "shortwave_optical_depth_per_band": tb,
        "air_temperature_tendency_from_shortwave_per_band": hb}


def grid_scale_condensation_device_call(self, ds, timestep=None):
    """GridScaleCondensation on a DeviceState: rrtmg_hip_grid_scale_condensation with device pointers on the main stream.  The
    pressures are read as they are resident -- in the units of whichever component asked for them first; the saturation formula
    needs Pa, so the library multiplies every pressure it reads by `pressure_scale`, Pa per resident unit: the one rounding the
    unit conversion of the host path makes.  The two new profiles go to work buffers that alternate with the step count (the
    state's previous arrays stay what they were) and the state is rebound to them; the precipitation goes to an [ncol] work
    buffer: -> (diagnostics as DeviceQuantity, the same state)."""
    P = self.input_properties
    names = ("air_temperature", "specific_humidity")
    t, q = (ds.need(n, P[n]) for n in names)
    p, pi = _resident_pressures(ds, "the condensation")
    nlay, ncol = t.shape
    if q.shape != (nlay, ncol) or p.shape != (nlay, ncol) or pi.shape != (nlay + 1, ncol):
        raise ValueError("temperature %s, humidity %s and pressures %s, %s do not belong to one grid" % (t.shape, q.shape, p.shape, pi.shape))
    ds.join_streams()      # a longwave still in flight belongs to the step this component closes
    work = _step_work(self, ds, "gsc", ncol)
    new = [work(n, x.units, like=x) for n, x in zip(names, (t, q))]
    precip = work("precip", "kg m^-2")
    ds.ctx.grid_scale_condensation(t.ptr, q.ptr, p.ptr, pi.ptr, self.constants(), t_out=new[0].ptr, q_out=new[1].ptr, diagnostics=dict(precip=precip.ptr),
                                   pressure_scale=_to_pa(p.units), memspace=1, ncol=ncol, nlay=nlay)
    ds.update(zip(names, new))
    return {"precipitation_amount": precip}, ds


def surface_ice_device_call(self, ds, timestep, check_maximum_height=True):
    """SeaIce / LandIce on a DeviceState: rrtmg_hip_surface_ice with device pointers on the main stream; nothing leaves HBM.
    The surface rows of the resident [interface_levels][*] radiative fluxes are bound by pointer (row 0 is the surface); the
    area-type codes are the resident ones, and the kernel decides from them which columns it steps.  The stepped column goes to
    work buffers that alternate with the step count (the state's previous arrays stay what they were) and the state is rebound
    to them; the diagnostics are DeviceQuantity handles SlabSurface and the shortwave can take from the state.
    The reference raises for a column taller than the maximum before it computes anything.  Here the kernel leaves such a
    column as it is and flags it: `check_maximum_height` True downloads the 4 * ncol bytes of the flags (which waits for the
    stream) and raises the reference's ValueError; False downloads nothing and leaves the column flagged in the
    component's `device_flags` (a DeviceQuantity).  -> (diagnostics, the same state)."""
    from .surface_ice import FLAG_TOO_TALL, FLUX_NAMES, too_tall_message
    P = self.input_properties
    ice_names = ("snow_and_ice_temperature", "height_on_ice_interface_levels")
    t, height = (ds.need(n, P[n]) for n in ice_names)
    col_names = (self.thickness_name, "surface_snow_thickness", self.base_name, "surface_upward_latent_heat_flux", "surface_upward_sensible_heat_flux")
    thick, snow, base, lh, sh = (ds.need(n, P[n]) for n in col_names)
    if len(t.shape) != 2:
        raise ValueError("quantity 'snow_and_ice_temperature' is resident as %s, component wants %s" % (t.dims, P["snow_and_ice_temperature"]["dims"]))
    nlay, ncol = t.shape
    area = ds.get("area_type")
    if area is None:
        raise KeyError("device state is missing input quantity 'area_type'")
    fluxes = dict(lh=lh.ptr, sh=sh.ptr)
    for k, name in FLUX_NAMES.items():
        if name not in _SURFACE_ROW:
            continue
        q = ds.get(name)
        if q is None:
            raise KeyError("device state is missing input quantity %r" % name)
        if q.dims[0] != "interface_levels":
            raise ValueError("%s must be resident as [interface_levels][*] (a radiation output) for the in-place surface row" % name)
        if q.shape[1:] != (ncol,):
            raise ValueError("ice temperature %s and %s %s do not belong to one grid" % (t.shape, name, q.shape))
        fluxes[k] = q.ptr                              # row 0 = the surface
    shapes = [height.shape] + [x.shape for x in (thick, snow, base, lh, sh, area)]
    if height.shape != (nlay, ncol) or any(x.shape != (ncol,) for x in (thick, snow, base, lh, sh, area)):
        raise ValueError("ice temperature %s, heights %s and the columns %s do not belong to one grid" % (t.shape, height.shape, shapes[1:]))
    ds.join_streams()      # the longwave fluxes in the state may be this step's
    work = _step_work(self, ds, "ice%d" % self.kind, ncol)
    t_new, h_new = work("t", t.units, like=t), work("height", height.units, like=height)
    thick_new, snow_new, tsfc = work("thick", thick.units), work("snow", snow.units), work("tsfc", "degK")
    base_flux, cond, albedo = work("base_flux", "W m^-2"), work("cond", "W m^-2"), work("albedo", "dimensionless")
    flags = work("flags", "dimensionless", dtype=np.int32)
    ds.ctx.surface_ice(self.kind, t.ptr, height.ptr, thick.ptr, snow.ptr, base.ptr, fluxes, area.ptr, float(timestep.total_seconds()), self.constants(),
                       t_out=t_new.ptr, height_out=h_new.ptr, thick_out=thick_new.ptr, snow_out=snow_new.ptr, tsfc_out=tsfc.ptr, base_flux_out=base_flux.ptr,
                       diagnostics=dict(cond_flux=cond.ptr, albedo=albedo.ptr, flags=flags.ptr), memspace=1, ncol=ncol, nlay=nlay)
    if check_maximum_height:
        ds.ctx.synchronize()
        got = flags.buf.download().reshape(-1)
        if np.any(got & FLAG_TOO_TALL):
            raise ValueError(too_tall_message(self._max_height))
        self.log_negative_energy(got)
    ds.update({"snow_and_ice_temperature": t_new, "height_on_ice_interface_levels": h_new, self.thickness_name: thick_new,
               "surface_snow_thickness": snow_new, "surface_temperature": tsfc})
    self.device_flags = flags      # int32 [*]: bit 0 active, bit 1 negative melt energy clamped, bit 2 taller than the maximum
    diagnostics = {self.base_flux_name: base_flux, "surface_albedo_for_direct_shortwave": albedo, "surface_albedo_for_diffuse_shortwave": albedo}
    if self.kind == 0:
        diagnostics["surface_downward_heat_flux_in_sea_ice"] = cond
    return diagnostics, ds


def sea_ice_device_call(self, ds, timestep, check_maximum_height=True):
    """SeaIce on a DeviceState (surface_ice_device_call)."""
    return surface_ice_device_call(self, ds, timestep, check_maximum_height)


def land_ice_device_call(self, ds, timestep, check_maximum_height=True):
    """LandIce on a DeviceState (surface_ice_device_call)."""
    return surface_ice_device_call(self, ds, timestep, check_maximum_height)


def _land_surface_inputs(self, ds, names, what):
    """The [ncol] inputs of a land-surface call by pointer: row 0 of a resident [mid_levels][*] profile is the lowest model level,
    row 0 of a resident [interface_levels][*] radiative flux the surface.  -> ({library name: pointer}, {library name: quantity}, ncol)"""
    P = self.input_properties
    ncol = ds.need("surface_temperature", P["surface_temperature"]).shape[0]
    ptrs, got = {}, {}
    for k, name in names.items():
        if name in _SURFACE_ROW:
            q = ds.get(name)
            if q is None:
                raise KeyError("device state is missing input quantity %r" % name)
            if q.dims[0] != "interface_levels":
                raise ValueError("%s must be resident as [interface_levels][*] (a radiation output) for the in-place surface row" % name)
        elif name in ("air_pressure", "surface_air_pressure"):
            # as resident -- in the units of whichever component asked first (the radiation asks for mbar): the caller hands the
            # library `pressure_scale` / `ps_scale`, Pa per resident unit.  Only the dims are checked, as in _resident_pressures
            q = ds.get(name)
            if q is None:
                raise KeyError("device state is missing input quantity %r" % name)
            if tuple(q.dims) != tuple(P[name]["dims"]):
                raise ValueError("quantity %r is resident as %s, component wants %s" % (name, q.dims, P[name]["dims"]))
        else:
            q = ds.need(name, P[name])
        if q.shape[-1] != ncol or len(q.shape) > 2:
            raise ValueError("%s %s and the %d columns of the surface temperature do not belong to one grid (%s)" % (name, q.shape, ncol, what))
        ptrs[k], got[k] = q.ptr, q
    return ptrs, got, ncol


def bucket_hydrology_device_call(self, ds, timestep):
    """BucketHydrology on a DeviceState: rrtmg_hip_bucket_hydrology with device pointers on the main stream; nothing leaves HBM.
    The lowest model level of the resident [mid_levels][*] profiles and the surface row of the resident [interface_levels][*]
    radiative fluxes are bound by pointer; the air pressure is read in its resident unit (`pressure_scale`).  The stepped surface
    goes to work buffers that alternate with the step count (the state's previous arrays stay what they were) and the state is
    rebound to them; the diagnostics are DeviceQuantity handles SlabSurface can take from the state.
    -> (diagnostics, the same state)."""
    from .bucket_hydrology import DIAGNOSTIC_NAMES, INPUT_NAMES, OUTPUT_NAMES
    ptrs, got, ncol = _land_surface_inputs(self, ds, self.names(INPUT_NAMES), "the bucket")
    ds.join_streams()      # the longwave fluxes in the state may be this step's
    work = _step_work(self, ds, "bucket%d" % self._num_layers, ncol)
    outs = {k: work(k, self.output_properties[name]["units"]) for k, name in self.names(OUTPUT_NAMES).items()}
    diag = {k: work(k, self.diagnostic_properties[name]["units"]) for k, name in self.names(DIAGNOSTIC_NAMES).items()}
    ds.ctx.bucket_hydrology(self._num_layers, ptrs, float(timestep.total_seconds()), self.scalars(), outs={k: x.ptr for k, x in outs.items()},
                            diagnostics={k: x.ptr for k, x in diag.items()}, pressure_scale=_to_pa(got["p_air"].units), memspace=1, ncol=ncol)
    ds.update({name: outs[k] for k, name in self.names(OUTPUT_NAMES).items()})
    return {name: diag[k] for k, name in self.names(DIAGNOSTIC_NAMES).items()}, ds


def second_best_device_call(self, ds, timestep):
    """SecondBEST on a DeviceState: rrtmg_hip_second_best with device pointers on the main stream; nothing leaves HBM.  The soil
    arrays are resident as [soil_interface_levels][*]; the lowest model level of the [mid_levels][*] profiles and the surface row
    of the [interface_levels][*] radiative fluxes are bound by pointer; the pressures are read in their resident units
    (`pressure_scale`, `ps_scale`); the area-type codes are the resident ones, and the kernel decides from them which columns it
    steps.  The stepped column goes to work buffers that alternate with the step count (the state's previous arrays stay what
    they were) and the state is rebound to them; the diagnostics are DeviceQuantity handles SlabSurface and the shortwave can
    take from the state, and the flags stay on the device in the component's `device_flags`.  -> (diagnostics, the same state)."""
    from .second_best import DIAGNOSTIC_NAMES, INPUT_NAMES, OUTPUT_NAMES
    ptrs, got, ncol = _land_surface_inputs(self, ds, INPUT_NAMES, "SecondBEST")
    t_soil = got["t_soil"]
    if len(t_soil.shape) != 2:
        raise ValueError("quantity 'soil_temperature' is resident as %s, component wants %s" % (t_soil.dims, self.input_properties["soil_temperature"]["dims"]))
    nlay = t_soil.shape[0]
    if any(got[k].shape != (nlay, ncol) for k in ("x_w", "x_i", "height")):
        raise ValueError("soil temperature %s, water %s, ice %s and heights %s do not belong to one grid" % (t_soil.shape, got["x_w"].shape, got["x_i"].shape, got["height"].shape))
    area = ds.get("area_type")
    if area is None:
        raise KeyError("device state is missing input quantity 'area_type'")
    if area.shape != (ncol,):
        raise ValueError("area types %s and the %d columns of the surface temperature do not belong to one grid" % (area.shape, ncol))
    ptrs["area_type"] = area.ptr
    ds.join_streams()      # the longwave fluxes in the state may be this step's
    work = _step_work(self, ds, "best", ncol)
    outs = {k: work(k, self.output_properties[name]["units"], like=got[k[:-4]] if k in ("t_soil_out", "x_w_out", "x_i_out") else None) for k, name in OUTPUT_NAMES.items()}
    diag = {k: work(k, self.diagnostic_properties[name]["units"]) for k, name in DIAGNOSTIC_NAMES.items()}
    flags = work("flags", "dimensionless", dtype=np.int32)
    ds.ctx.second_best(ptrs, float(timestep.total_seconds()), self.constants(), outs={k: x.ptr for k, x in outs.items()},
                       diagnostics=dict({k: x.ptr for k, x in diag.items()}, flags=flags.ptr), pressure_scale=_to_pa(got["p_air"].units),
                       ps_scale=_to_pa(got["ps"].units), memspace=1, ncol=ncol, nlay=nlay)
    ds.update({name: outs[k] for k, name in OUTPUT_NAMES.items()})
    self.device_flags = flags      # int32 [*]: bit 0 active, bit 1 the unstable branch, bit 2 capped at the freezing temperature
    return {name: diag[k] for k, name in DIAGNOSTIC_NAMES.items()}, ds


# ---- time stepping on the device ------------------------------------------------------------------------------------
_AB = {1: (1.0,), 2: (1.5, -0.5), 3: (23.0 / 12.0, -16.0 / 12.0, 5.0 / 12.0), 4: (55.0 / 24.0, -59.0 / 24.0, 37.0 / 24.0, -9.0 / 24.0)}


def _rate(units):
    u = units.strip()
    if u in ("m s^-2", "m/s^2"):      # an acceleration is the rate of a speed
        return 1.0
    for suffix, seconds in ((" s^-1", 1.0), ("/s", 1.0), (" day^-1", 86400.0), ("/day", 86400.0)):
        if u.endswith(suffix):
            return 1.0 / seconds
    raise ValueError("tendency units %r are not a rate" % units)


class DeviceAdamsBashforth:
    """sympl's AdamsBashforth around TendencyComponents (tests/test_components.py:123-160), on a DeviceState: tendencies of
    all components summed in "<state units> per second", order ramping 1 -> 2 -> 3, prognostic quantities replaced in the
    state -- every sum and the update are kernels on the context's main stream.  Returns (diagnostics, the same state).
    wait_every_step=False: the host does not wait for the step (a time loop that reads nothing back keeps the GPU busy while
    the host prepares the next step); the device-side `stop` conditions are sticky and surface at the next download(),
    Context.synchronize() or waiting step."""

    def __init__(self, *components, order=3, wait_every_step=True):
        self._wait = bool(wait_every_step)
        if len(components) == 1 and isinstance(components[0], (list, tuple)):
            components = tuple(components[0])
        if order not in _AB:
            raise ValueError("order must be 1..4")
        self.component_list, self._order = list(components), order
        self._history, self._timestep, self._slot = [], None, 0

    def __call__(self, ds, timestep):
        if not isinstance(timestep, datetime.timedelta):
            raise TypeError("timestep must be a datetime.timedelta")
        if self._timestep is None:
            self._timestep = timestep
        elif timestep != self._timestep:
            raise ValueError("timestep must be constant for Adams-Bashforth time stepping")
        ctx, total, diagnostics = ds.ctx, {}, {}
        slot = self._slot = (self._slot + 1) % (self._order + 1)
        # every component first (the longwave goes to its own stream: the shortwave enqueued behind it on the main stream runs
        # beside it), then the sums in component order
        results = []
        for comp in self.component_list:
            # an ImplicitTendencyComponent (EmanuelConvection) is handed the timestep, as sympl's tendency steppers do
            tend, diag = comp(ds, timestep) if isinstance(comp, _sc.ImplicitTendencyComponent) else comp(ds)
            overlap = set(diag) & set(diagnostics)
            if overlap:
                raise ValueError("two components compute the same diagnostics: %s" % sorted(overlap))
            diagnostics.update(diag)
            results.append(tend)
        ds.join_streams()
        for tend in results:
            for name, q in tend.items():
                acc = ds.work(("ab", id(self), name, slot), q.shape, q.dims, ds[name].units + " s^-1")
                if name in total:
                    ctx.elementwise("axpby", q.size, acc.ptr, acc.ptr, b=q.ptr, alpha=1.0, beta=_rate(q.units))
                else:
                    ctx.elementwise("axpby", q.size, q.ptr, acc.ptr, alpha=_rate(q.units))
                    total[name] = acc
        self._history = [total] + self._history[: self._order - 1]
        dt = timestep.total_seconds()
        for name in total:
            old = ds[name]
            # the contiguous most-recent run of steps that carry a tendency for `name` sets the order for THAT quantity
            # (the coefficients of an order sum to one; a truncated higher-order set would not)
            hist = []
            for h in self._history:
                if name not in h:
                    break
                hist.append(h[name].ptr)
            new = ds.work(("ab", id(self), name, "state", ds.step_count % 2), old.shape, old.dims, old.units)
            ctx.ab_step(old.size, old.ptr, hist, _AB[len(hist)], dt, new.ptr)
            ds[name] = new
        ds.step_count += 1
        if self._wait:
            ctx.synchronize()      # device-side `stop` conditions of this step surface here
        return diagnostics, ds
