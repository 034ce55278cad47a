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
may still hold the last step's), and the sequence is enqueued on the shortwave's stream."""
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
