"""Instellation -- drop-in for climt.Instellation (climt/_components/instellation/component.py:9-61): zenith angle
from latitude, longitude and model time, the producer of the `zenith_angle` the shortwave consumes.  Same class name,
property dictionaries and output; the per-column kernel (component.py:85-135) runs on the GPU through
rrtmg_hip_zenith_angle (include/rrtmg_hip.h), the time arithmetic (:64-82) stays on the host."""
import datetime

import numpy as np

from ._sympl_compat import DataArray, DiagnosticComponent
from .rrtmg.common import make_context


def total_days(time_diff):
    """Total time in units of days (component.py:69-76)."""
    return time_diff.days + (time_diff.seconds + time_diff.microseconds / 1000000.0) / (24 * 3600.0)


def days_from_2000(model_time):
    """Days since 2000-01-01 12:00 (component.py:64-66)."""
    return total_days(model_time - datetime.datetime(2000, 1, 1, 12, 0))


def interval_centuries(model_time, timedelta):
    """(t0, t1) in Julian centuries of [model_time, model_time + timedelta], as rrtmg_hip_mean_coszen takes them."""
    return days_from_2000(model_time) / 36525.0, days_from_2000(model_time + timedelta) / 36525.0


def host_columns(state):
    """(latitude, longitude) of a host state in degrees, flattened in the order of the latitude's own dims -- the column order
    of every component's "*" axis where the horizontal dims come in one order throughout the state."""
    lat_da, lon_da = state["latitude"], state["longitude"]
    lat, lon = np.asarray(lat_da.values, dtype=np.float64), np.asarray(lon_da.values, dtype=np.float64)
    if tuple(lon_da.dims) != tuple(lat_da.dims):
        if sorted(lon_da.dims) != sorted(lat_da.dims):
            raise ValueError("latitude %s and longitude %s must have the same dims" % (lat_da.dims, lon_da.dims))
        lon = np.transpose(lon, [lon_da.dims.index(d) for d in lat_da.dims])
    return np.ascontiguousarray(lat.reshape(-1)), np.ascontiguousarray(lon.reshape(-1))


class Instellation(DiagnosticComponent):
    """Calculates the zenith angle given orbital parameters (Earth-sun system), on AMD MI355X."""

    input_properties = {
        "latitude": {"dims": ["*"], "units": "degrees_north"},
        "longitude": {"dims": ["*"], "units": "degrees_east"},
    }

    diagnostic_properties = {
        "zenith_angle": {"dims": ["*"], "units": "radians"},
    }

    def __init__(self, device=0, context=None, **kwargs):
        """`context`: share the library context (and its HIP stream) of an RRTMG component; else a new one on `device`."""
        super(Instellation, self).__init__(**kwargs)
        self._ctx = context if context is not None else make_context(device)

    def __call__(self, state, *args, **kwargs):
        """A host state goes through sympl's machinery to array_call; a climt_amd.DeviceState (state resident in HBM) takes
        the device path: same quantities, DeviceQuantity handles instead of arrays (climt_amd/device_state.py)."""
        from .device_state import DeviceState, instellation_device_call
        if isinstance(state, DeviceState):
            return instellation_device_call(self, state)
        return super(Instellation, self).__call__(state, *args, **kwargs)

    def interval_mean(self, state, timedelta):
        """The sun over [state["time"], state["time"] + timedelta] (12 hours at the most; rrtmg_hip_mean_coszen) ->
        {"zenith_angle": arccos of the cosine of the zenith angle averaged over the SUNLIT part of the interval (pi/2 where the
        sun is down throughout), "sunlit_fraction": the part of the interval the sun is up}: what a radiation call that stands
        for the whole interval takes in place of the zenith angle of its instant (climt_amd.IntermittentShortwave).  A host
        state gives DataArrays, a climt_amd.DeviceState DeviceQuantity handles (nothing leaves HBM)."""
        from .device_state import DeviceState, instellation_interval_device_call
        if isinstance(state, DeviceState):
            return instellation_interval_device_call(self, state, timedelta)
        lat, lon = host_columns(state)
        zen = np.empty(lat.shape)
        _, frac = self._ctx.mean_coszen(lat, lon, *interval_centuries(state["time"], timedelta), out_zenith=zen)
        dims, shape = tuple(state["latitude"].dims), np.shape(state["latitude"].values)
        return {"zenith_angle": DataArray(np.reshape(zen, shape), dims=dims, attrs={"units": "radians"}),
                "sunlit_fraction": DataArray(np.reshape(frac, shape), dims=dims, attrs={"units": "dimensionless"})}

    def array_call(self, state):
        lat, lon = state["latitude"], state["longitude"]
        lat_flat = np.ascontiguousarray(np.reshape(lat, (-1,)), dtype=np.float64)
        lon_flat = np.ascontiguousarray(np.reshape(lon, (-1,)), dtype=np.float64)
        julian_centuries = days_from_2000(state["time"]) / 36525.0
        zen = self._ctx.zenith_angle(lat_flat, lon_flat, julian_centuries)
        return {"zenith_angle": np.reshape(zen, np.shape(lat))}
