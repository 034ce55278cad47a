"""`IntermittentShortwave`: the shortwave every `update_timedelta` of model time, without the diurnal-cycle error of handing
back the last call's output unchanged (`UpdateFrequencyWrapper`).  What every model that runs radiation intermittently does
(Hogan & Hirahara 2016; Manners et al. 2009; Hogan & Bozzo 2015):

  * the radiation call sees the cosine of the zenith angle averaged over the SUNLIT part of the interval it stands for,
    [time, time + update_timedelta] (rrtmg_hip_mean_coszen), not the sun of its instant;
  * every model step rescales the kept fluxes and heating rates by its own insolation: s = mu_step * f_step / mu_rad by column,
    mu and f the sunlit-mean cosine and the sunlit fraction of [time, time + timestep] (one rrtmg_hip_scale_columns launch for
    everything the call returned; all of it is linear in the incoming flux).  A column without sun in the step gets exact zeros.

    sw = IntermittentShortwave(RRTMGShortwave(), Instellation(), timedelta(hours=3))
    tendencies, diagnostics = sw(state, timestep)          # host state, or a climt_amd.DeviceState

When an update is due is UpdateFrequencyWrapper's rule: the first call, then state["time"] >= last update + update_timedelta.
On a host state the kept arrays go up once per update and every step's scaled arrays come down; on a DeviceState nothing
leaves HBM: the kept arrays are a pool of the wrapper's own, the scaled ones a second pool of two alternating sets (the state
may still hold the last step's), and the sequence is enqueued on the shortwave's stream.

`IntermittentLongwave` (below) is the longwave counterpart: the kept upward fluxes and heating rates follow the surface
temperature of every step through the derivative an idrv = 1 call returns (rrtmg_hip_lw_adjust_surface)."""
from datetime import timedelta

import numpy as np

from . import _hip
from ._sympl_compat import DataArray

_MAX_INTERVAL = timedelta(hours=12)


class IntermittentShortwave:
    def __init__(self, shortwave, instellation, update_timedelta):
        if not isinstance(update_timedelta, timedelta):
            raise TypeError("update_timedelta must be a datetime.timedelta, got %r" % (update_timedelta,))
        if not timedelta(0) < update_timedelta <= _MAX_INTERVAL:
            raise ValueError("update_timedelta must be positive and 12 hours at the most (the interval mean is served up to there)")
        if getattr(shortwave, "_boundary_dtype", np.float64) == np.float32:
            raise ValueError('IntermittentShortwave scales float64 arrays: the wrapped shortwave has boundary_dtype="float32"')
        self.component = shortwave
        self._sun = instellation
        self._update_timedelta = update_timedelta
        self._last_update_time = None
        self._calls = 0
        self._pool = {}        # device path: key -> DeviceQuantity (kept arrays, the sun of the two intervals, scaled arrays)
        self._host = {}        # host path: key -> DeviceArray
        self._kept = None

    def __getattr__(self, item):
        return getattr(self.component, item)

    def _due(self, now, timestep):
        if not isinstance(timestep, timedelta):
            raise TypeError("timestep must be a datetime.timedelta")
        if not timedelta(0) < timestep <= self._update_timedelta:
            raise ValueError("timestep must be positive and not longer than update_timedelta")
        return self._last_update_time is None or now >= self._last_update_time + self._update_timedelta

    def __call__(self, state, timestep):
        from .device_state import DeviceState
        self._calls += 1
        if isinstance(state, DeviceState):
            return self._device_call(state, timestep)
        return self._host_call(state, timestep)

    # ---- host state -------------------------------------------------------------------------------------------------------------
    def _host_array(self, key, shape):
        a = self._host.get(key)
        if a is None or a.shape != tuple(shape):
            a = self._host[key] = _hip.DeviceArray(shape)
        return a

    def _host_call(self, state, timestep):
        from .instellation import host_columns, interval_centuries
        now, ctx = state["time"], self.component._ctx
        due = self._due(now, timestep)
        lat, lon = host_columns(state)
        ncol = lat.size
        col = lambda key: self._host_array(key, (ncol,))
        ctx.synchronize()      # (an earlier launch of a deferred context may still read what is uploaded here)
        col("lat").upload(lat); col("lon").upload(lon)

        def sun(prefix, delta, zenith):
            ctx.mean_coszen(col("lat").ptr, col("lon").ptr, *interval_centuries(now, delta), out_mean=col(prefix + "mean").ptr,
                            out_fraction=col(prefix + "fraction").ptr, memspace=1, ncol=ncol, out_zenith=col(prefix + "zenith").ptr if zenith else None,
                            out_insolation=col(prefix + "insolation").ptr)
        if due:
            sun("rad.", self._update_timedelta, True)
            ctx.synchronize()
            horizontal, hshape = tuple(state["latitude"].dims), np.shape(state["latitude"].values)
            call_state = dict(state)      # a shallow copy: the caller's state keeps its zenith angle
            call_state["zenith_angle"] = DataArray(col("rad.zenith").download().reshape(hshape), dims=horizontal, attrs={"units": "radians"})
            tendencies, diagnostics = self.component(call_state)
            kept = []
            for group, arrays in (("tendencies", tendencies), ("diagnostics", diagnostics)):
                for name, da in arrays.items():
                    dims, values = tuple(da.dims), np.asarray(da.values)
                    if not set(horizontal) & set(dims):
                        raise ValueError("%s has no column axis to scale (dims %s)" % (name, dims))
                    if dims[len(dims) - len(horizontal):] != horizontal:
                        raise ValueError("%s: the horizontal dims %s must come last and in the order of the latitude's, got %s" % (name, horizontal, dims))
                    rows = values.size // ncol
                    src = self._host_array(("kept", group, name), (rows, ncol))
                    src.upload(values.reshape(rows, ncol))
                    kept.append((group, name, dims, values.shape, dict(da.attrs), src, self._host_array(("scaled", group, name), (rows, ncol)), rows))
            self._kept, self._last_update_time = kept, now
        sun("step.", timestep, False)
        ctx.scale_columns(col("step.insolation"), col("rad.mean"), [(src, dst, rows) for *_, src, dst, rows in self._kept], ncol=ncol)
        ctx.synchronize()
        out = {"tendencies": {}, "diagnostics": {}}
        for group, name, dims, shape, attrs, _, dst, _ in self._kept:
            out[group][name] = DataArray(dst.download().reshape(shape), dims=dims, attrs=attrs)
        return out["tendencies"], out["diagnostics"]

    # ---- DeviceState ------------------------------------------------------------------------------------------------------------
    def _work(self, *prefix):
        from .device_state import DeviceQuantity

        def work(key, shape, dims, units):
            q = self._pool.get(prefix + (key,))
            if q is None or q.shape != tuple(shape):
                q = self._pool[prefix + (key,)] = DeviceQuantity(_hip.DeviceArray(shape), shape, dims, units)
            return q
        return work

    def _device_call(self, ds, timestep):
        from .device_state import DeviceState, instellation_interval_device_call
        now, ctx = ds["time"], ds.ctx
        if self._due(now, timestep):
            rad = instellation_interval_device_call(self._sun, ds, self._update_timedelta, work=self._work("rad"))
            call_state = DeviceState.__new__(DeviceState)      # a shallow copy: the caller's state keeps its zenith angle
            dict.update(call_state, ds)
            call_state.__dict__.update(ds.__dict__)
            call_state["zenith_angle"] = rad["zenith_angle"]
            tendencies, diagnostics = self.component(call_state, output_work=self._work("kept"))
            # the derived inputs are buffers the two states share: they hold the interval's cosine now
            ds._derived_ok = False
            ds._lw_inflight = getattr(call_state, "_lw_inflight", False)
            self._kept, self._rad, self._last_update_time = (tendencies, diagnostics), rad, now
        step = instellation_interval_device_call(self._sun, ds, timestep, work=self._work("step", self._calls & 1))
        scaled, entries = {}, []
        for arrays in self._kept:
            for q in arrays.values():
                if id(q) in scaled:
                    continue      # (the tendency and its diagnostic are one array)
                if q.dims[-1] != "*":
                    raise ValueError("an output of dims %s has no column axis to scale" % (q.dims,))
                key = len(scaled)
                dst = self._work("scaled", self._calls & 1)(key, q.shape, q.dims, q.units)
                scaled[id(q)] = dst
                entries.append((q.ptr, dst.ptr, q.size // ds.ncol))
        ctx.scale_columns(step["insolation"].ptr, self._rad["coszen_mean"].ptr, entries, ncol=ds.ncol)
        tendencies, diagnostics = ({name: scaled[id(q)] for name, q in arrays.items()} for arrays in self._kept)
        return tendencies, diagnostics


# the outputs of RRTMGLongwave by the stream they belong to: (upward flux, downward flux, heating rate)
_LW_ALL = ("upwelling_longwave_flux_in_air", "downwelling_longwave_flux_in_air", "air_temperature_tendency_from_longwave")
_LW_CLEAR = ("upwelling_longwave_flux_in_air_assuming_clear_sky", "downwelling_longwave_flux_in_air_assuming_clear_sky",
             "air_temperature_tendency_from_longwave_assuming_clear_sky")


class IntermittentLongwave:
    """The longwave every `update_timedelta` of model time, with the upward fluxes and the heating rates of every step in between
    corrected for the surface temperature of that step (the purpose of RRTMG's idrv = 1; Hogan & Bozzo 2015):

        uflx' = uflx + d(uflx)/d(tsfc) * (tsfc_now - tsfc_call)      by column and level, all sky and clear sky
        hr'   = the heating rate of the net flux uflx' - dflx, as the call itself forms it

    in one rrtmg_hip_lw_adjust_surface launch per step.  FIRST ORDER in the temperature change and not clamped; the downward fluxes
    are handed back as kept; air temperatures on the interfaces that the library interpolates itself do not follow the surface
    between updates.

        lw = IntermittentLongwave(RRTMGLongwave(calculate_change_up_flux=True), timedelta(hours=3))
        tendencies, diagnostics = lw(state, timestep)          # host state, or a climt_amd.DeviceState

    An update is due at the first call, then when state["time"] >= last update + update_timedelta.  The update's own call is
    adjusted too (by dT = 0: the call's bits).  A McICA mask belongs to the update and is not drawn again in between.  On a host
    state the kept arrays go up once per update, the surface temperature at every step, and the adjusted arrays come down; on a
    DeviceState nothing leaves HBM: the kept arrays are a pool of the wrapper's own, the adjusted ones a second pool of two
    alternating sets, and the launch is enqueued on the longwave's stream (consumers join it as they join the longwave itself)."""

    def __init__(self, longwave, update_timedelta):
        if not isinstance(update_timedelta, timedelta):
            raise TypeError("update_timedelta must be a datetime.timedelta, got %r" % (update_timedelta,))
        if not update_timedelta > timedelta(0):
            raise ValueError("update_timedelta must be positive")
        if not getattr(longwave, "_calc_dflxdt", 0):
            raise ValueError("IntermittentLongwave needs the derivative of the upward flux with respect to the surface temperature: "
                             "construct the longwave with calculate_change_up_flux=True")
        if getattr(longwave, "_band_fluxes", False):
            raise ValueError("IntermittentLongwave cannot adjust band_fluxes: the surface-temperature derivative has no per-band form")
        if getattr(longwave, "_boundary_dtype", np.float64) == np.float32:
            raise ValueError('IntermittentLongwave adjusts float64 arrays: the wrapped longwave has boundary_dtype="float32"')
        self.component = longwave
        self._update_timedelta = update_timedelta
        self._last_update_time = None
        self._calls = 0
        self._pool = {}        # device path: key -> DeviceQuantity (kept arrays, adjusted arrays)
        self._host = {}        # host path: key -> DeviceArray
        self._kept = None

    def __getattr__(self, item):
        return getattr(self.component, item)

    def _due(self, now, timestep):
        if not isinstance(timestep, timedelta):
            raise TypeError("timestep must be a datetime.timedelta")
        if not timedelta(0) < timestep <= self._update_timedelta:
            raise ValueError("timestep must be positive and not longer than update_timedelta")
        return self._last_update_time is None or now >= self._last_update_time + self._update_timedelta

    def __call__(self, state, timestep):
        from .device_state import DeviceState
        self._calls += 1
        if isinstance(state, DeviceState):
            return self._device_call(state, timestep)
        return self._host_call(state, timestep)

    _host_array = IntermittentShortwave._host_array
    _work = IntermittentShortwave._work

    # ---- host state -------------------------------------------------------------------------------------------------------------
    @staticmethod
    def _surface_temperature(state, horizontal):
        from .device_state import _convert, _units_of
        ts = state["surface_temperature"]
        if tuple(ts.dims) != tuple(horizontal):
            raise ValueError("surface_temperature has dims %s, the longwave's outputs end in %s" % (tuple(ts.dims), tuple(horizontal)))
        return np.ascontiguousarray(_convert(np.asarray(ts.values, dtype=np.float64), _units_of(ts), "degK")).reshape(-1)

    def _host_call(self, state, timestep):
        now, lw = state["time"], self.component
        ctx = lw._ctx
        if self._due(now, timestep):
            tendencies, diagnostics = lw(state)
            up = diagnostics[_LW_ALL[0]]
            dims, shape = tuple(up.dims), np.shape(up.values)
            if dims[0] != "interface_levels":
                raise ValueError("%s: interface_levels must come first, got dims %s" % (_LW_ALL[0], dims))
            nlev, horizontal = shape[0], dims[1:]
            ncol = int(np.prod(shape[1:])) if len(shape) > 1 else 1
            clear = getattr(lw, "_clear_sky", True)
            plev, pressure_scale = lw._interface_pressure_of_call
            streams = []
            for names, derivative in ((_LW_ALL, lw.change_in_upward_flux_with_surface_temperature),) + (
                    ((_LW_CLEAR, lw.change_in_clear_sky_upward_flux_with_surface_temperature),) if clear else ()):
                flux_up, flux_dn, heat = (diagnostics[n] for n in names)
                dev = {}
                for key, values, rows in (("uflx", flux_up.values, nlev), ("dflx", flux_dn.values, nlev), ("duflx_dt", derivative, nlev)):
                    dev[key] = self._host_array(("kept", names[0], key), (rows, ncol))
                    dev[key].upload(np.asarray(values, dtype=np.float64).reshape(rows, ncol))
                dev["uflx_out"] = self._host_array(("adjusted", names[0], "uflx"), (nlev, ncol))
                dev["hr_out"] = self._host_array(("adjusted", names[0], "hr"), (nlev - 1, ncol))
                streams.append((names, (flux_up, flux_dn, heat), dev))
            ctx.synchronize()      # (an earlier launch of a deferred context may still read what is uploaded here)
            self._host_array("plev", (nlev, ncol)).upload(np.asarray(plev, dtype=np.float64).reshape(nlev, ncol))
            self._host_array("tsfc_call", (ncol,)).upload(self._surface_temperature(state, horizontal))      # a copy: the state's own will change
            self._kept = dict(streams=streams, nlev=nlev, ncol=ncol, horizontal=horizontal, pressure_scale=pressure_scale,
                              tendency=tendencies["air_temperature"])
            self._last_update_time = now
        k = self._kept
        nlev, ncol = k["nlev"], k["ncol"]
        ctx.synchronize()
        self._host_array("tsfc_now", (ncol,)).upload(self._surface_temperature(state, k["horizontal"]))
        args = [(d["uflx"], d["dflx"], d["duflx_dt"], d["uflx_out"], d["hr_out"]) for _, _, d in k["streams"]]
        ctx.lw_adjust_surface(ncol, nlev - 1, self._host["tsfc_call"], self._host["tsfc_now"], self._host["plev"], args[0],
                              args[1] if len(args) > 1 else None, pressure_scale=k["pressure_scale"])
        ctx.synchronize()
        diagnostics = {}
        for names, (flux_up, flux_dn, heat), d in k["streams"]:
            diagnostics[names[0]] = DataArray(d["uflx_out"].download().reshape(np.shape(flux_up.values)), dims=tuple(flux_up.dims), attrs=dict(flux_up.attrs))
            diagnostics[names[1]] = DataArray(np.array(flux_dn.values), dims=tuple(flux_dn.dims), attrs=dict(flux_dn.attrs))
            diagnostics[names[2]] = DataArray(d["hr_out"].download().reshape(np.shape(heat.values)), dims=tuple(heat.dims), attrs=dict(heat.attrs))
        # (the tendency and its diagnostic are one array, as in the wrapped component)
        tend = k["tendency"]
        return {"air_temperature": DataArray(diagnostics[_LW_ALL[2]].values, dims=tuple(tend.dims), attrs=dict(tend.attrs))}, diagnostics

    # ---- DeviceState ------------------------------------------------------------------------------------------------------------
    def _device_call(self, ds, timestep):
        now, ctx, lw = ds["time"], ds.ctx, self.component
        nlay, ncol = ds["air_temperature"].shape
        if self._due(now, timestep):
            kept = self._work("kept")
            tendencies, diagnostics = lw(ds, output_work=kept)
            # copies on the main stream, behind whatever wrote the state: the state's own arrays will change
            ts, pl = ds.need("surface_temperature", lw.input_properties["surface_temperature"]), ds.need("air_pressure_on_interface_levels", lw.input_properties["air_pressure_on_interface_levels"])
            tsfc_call, plev = kept("tsfc_call", ts.shape, ts.dims, ts.units), kept("plev", pl.shape, pl.dims, pl.units)
            ctx.elementwise("axpby", ts.size, ts.ptr, tsfc_call.ptr, alpha=1.0)
            ctx.elementwise("axpby", pl.size, pl.ptr, plev.ptr, alpha=1.0)
            self._kept = dict(tendencies=tendencies, diagnostics=diagnostics, tsfc_call=tsfc_call, plev=plev,
                              derivatives=(lw.change_in_upward_flux_with_surface_temperature, lw.change_in_clear_sky_upward_flux_with_surface_temperature))
            self._last_update_time = now
        k = self._kept
        ts = ds.need("surface_temperature", lw.input_properties["surface_temperature"])
        work = self._work("adjusted", self._calls & 1)
        diagnostics, args = dict(k["diagnostics"]), []
        for names, derivative in ((_LW_ALL, k["derivatives"][0]), (_LW_CLEAR, k["derivatives"][1])):
            if derivative is None:
                continue
            flux_up, flux_dn, heat = (k["diagnostics"][n] for n in names)
            up, hr = work(names[0], flux_up.shape, flux_up.dims, flux_up.units), work(names[2], heat.shape, heat.dims, heat.units)
            args.append((flux_up.ptr, flux_dn.ptr, derivative.ptr, up.ptr, hr.ptr))
            diagnostics[names[0]], diagnostics[names[2]] = up, hr
        # the launch goes to the longwave's stream: behind the main stream's work so far (the step that wrote this surface
        # temperature, the copies above, the consumers of the set of adjusted arrays written now)
        ctx.order_streams(0)
        ctx.lw_adjust_surface(ncol, nlay, k["tsfc_call"].ptr, ts.ptr, k["plev"].ptr, args[0], args[1] if len(args) > 1 else None)
        ds._lw_inflight = True      # consumers on the main stream join first: DeviceState.join_streams()
        return {"air_temperature": diagnostics[_LW_ALL[2]]}, diagnostics
