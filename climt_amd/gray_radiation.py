"""GrayLongwaveRadiation and Frierson06LongwaveOpticalDepth -- drop-ins for climt's (climt/_components/radiation.py): the
two-stream gray longwave sweep and the latitude-dependent optical depth of Frierson et al. 2006 that feeds it.  Same property
dictionaries, aliases, keywords and defaults; the per-column rules run on the GPU through rrtmg_hip_gray_longwave and
rrtmg_hip_frierson_optical_depth (include/rrtmg_hip.h), one thread per column, in the reference's order of operations.

One keyword the reference lacks: GrayLongwaveRadiation(optical_depth=<a Frierson06LongwaveOpticalDepth>) selects the fused call --
the optical depth is formed inside the sweep from the interface pressures, the surface pressure and the latitude, so the
component no longer reads longwave_optical_depth_on_interface_levels; it returns the depth among its diagnostics instead.  The
numbers are those of the two components one after the other, bit for bit."""
import numpy as np

from ._sympl_compat import DiagnosticComponent, TendencyComponent, get_constant
from .rrtmg.common import make_context

TAU = "longwave_optical_depth_on_interface_levels"


class Frierson06LongwaveOpticalDepth(DiagnosticComponent):
    """The longwave optical depth of Frierson, Held and Zurita-Gotor 2006 on the interface levels: 0 at the surface, the
    latitude's tau_0 at the top (the reference's direction; only differences of the depth enter the gray sweep)."""

    input_properties = {
        "air_pressure_on_interface_levels": {
            "dims": ["interface_levels", "*"],
            "units": "Pa",
        },
        "surface_air_pressure": {"dims": ["*"], "units": "Pa"},
        "latitude": {"dims": ["*"], "units": "degrees_N"},
    }

    diagnostic_properties = {
        "longwave_optical_depth_on_interface_levels": {
            "dims": ["interface_levels", "*"],
            "units": "dimensionless",
        }
    }

    def __init__(
        self,
        linear_optical_depth_parameter=0.1,
        longwave_optical_depth_at_equator=6,
        longwave_optical_depth_at_poles=1.5,
        device=0,
        context=None,
        **kwargs
    ):
        """
        Args: the reference's (climt.Frierson06LongwaveOpticalDepth), word for word in names and defaults; plus `device` and
        `context` like the other components of this package.

            linear_optical_depth_parameter (float): the weight of the term linear in sigma = p / ps.  Default 0.1.
            longwave_optical_depth_at_equator (float): Default 6.
            longwave_optical_depth_at_poles (float): Default 1.5.
        """
        self._fl = linear_optical_depth_parameter
        self._tau0e = longwave_optical_depth_at_equator
        self._tau0p = longwave_optical_depth_at_poles
        super(Frierson06LongwaveOpticalDepth, self).__init__(**kwargs)
        self._ctx = context if context is not None else make_context(device)

    def parameters(self):
        """The three parameters as the library takes them."""
        return dict(tau0e=float(self._tau0e), tau0p=float(self._tau0p), fl=float(self._fl))

    def __call__(self, state, *args, **kwargs):
        """A host state goes through sympl's machinery to array_call; a climt_amd.DeviceState (state resident in HBM) takes the
        device path (climt_amd/device_state.py)."""
        from .device_state import DeviceState, frierson_device_call
        if isinstance(state, DeviceState):
            return frierson_device_call(self, state)
        return super(Frierson06LongwaveOpticalDepth, self).__call__(state, *args, **kwargs)

    def array_call(self, state):
        p_int = np.asarray(state["air_pressure_on_interface_levels"], dtype=np.float64)
        tau = self._ctx.frierson_optical_depth(np.reshape(p_int, (p_int.shape[0], -1)), np.reshape(np.asarray(state["surface_air_pressure"], dtype=np.float64), (-1,)),
                                               np.reshape(np.asarray(state["latitude"], dtype=np.float64), (-1,)), self.parameters())
        return {TAU: np.reshape(tau, p_int.shape)}


class GrayLongwaveRadiation(TendencyComponent):
    """The gray two-stream longwave: an upward sweep from the surface's sigma T^4 and a downward one from zero at the top, each
    layer emitting sigma T^4 (1 - exp(-dtau)); the heating from the divergence of the net flux."""

    input_properties = {
        "longwave_optical_depth_on_interface_levels": {
            "dims": ["interface_levels", "*"],
            "units": "dimensionless",
            "alias": "tau",
        },
        "air_temperature": {
            "dims": ["mid_levels", "*"],
            "units": "degK",
            "alias": "sl",
        },
        "surface_temperature": {
            "dims": ["*"],
            "units": "degK",
            "alias": "T_surface",
        },
        "air_pressure": {
            "dims": ["mid_levels", "*"],
            "units": "Pa",
            "alias": "p",
        },
        "air_pressure_on_interface_levels": {
            "dims": ["interface_levels", "*"],
            "units": "Pa",
            "alias": "p_interface",
        },
    }

    diagnostic_properties = {
        "downwelling_longwave_flux_in_air": {
            "dims": ["interface_levels", "*"],
            "units": "W m^-2",
            "alias": "lw_down",
        },
        "upwelling_longwave_flux_in_air": {
            "dims": ["interface_levels", "*"],
            "units": "W m^-2",
            "alias": "lw_up",
        },
        "air_temperature_tendency_from_longwave": {"dims": ["mid_levels", "*"], "units": "degK day^-1"},
    }

    tendency_properties = {
        "air_temperature": {"units": "degK s^-1"},
    }

    def __init__(self, optical_depth=None, device=0, context=None, **kwargs):
        """
        Args: the reference's (climt.GrayLongwaveRadiation takes none of its own), plus

            optical_depth (Frierson06LongwaveOpticalDepth): the fused call.  The component then reads surface_air_pressure and
                latitude instead of longwave_optical_depth_on_interface_levels, forms the optical depth inside the sweep with
                that component's parameters, and returns it among the diagnostics.  Default None: the reference's interface.
            device, context: like the other components of this package.
        """
        if optical_depth is not None:
            if not isinstance(optical_depth, Frierson06LongwaveOpticalDepth):
                raise TypeError("optical_depth must be a Frierson06LongwaveOpticalDepth")
            # (instance attributes: the class keeps the reference's dictionaries)
            self.input_properties = {k: dict(v) for k, v in type(self).input_properties.items() if k != TAU}
            for name in ("surface_air_pressure", "latitude"):
                self.input_properties[name] = dict(Frierson06LongwaveOpticalDepth.input_properties[name])
            self.diagnostic_properties = dict(type(self).diagnostic_properties)
            self.diagnostic_properties[TAU] = dict(Frierson06LongwaveOpticalDepth.diagnostic_properties[TAU])
        self._optical_depth = optical_depth
        super(GrayLongwaveRadiation, self).__init__(**kwargs)
        self._ctx = context if context is not None else make_context(device)

    def constants(self):
        """The three constants of the reference's array_call as the library takes them, asked for at every call under the unit
        strings the reference asks with."""
        return dict(sigma_sb=get_constant("stefan_boltzmann_constant", "W/m^2/K^4"), g=get_constant("gravitational_acceleration", "m/s^2"),
                    cpd=get_constant("heat_capacity_of_dry_air_at_constant_pressure", "J/kg/K"))

    def __call__(self, state, *args, **kwargs):
        """A host state goes through sympl's machinery to array_call; a climt_amd.DeviceState (state resident in HBM) takes the
        device path (climt_amd/device_state.py)."""
        from .device_state import DeviceState, gray_longwave_device_call
        if isinstance(state, DeviceState):
            return gray_longwave_device_call(self, state)
        return super(GrayLongwaveRadiation, self).__call__(state, *args, **kwargs)

    def array_call(self, state):
        def get(name):      # (sympl hands an input with an alias over under it)
            alias = self.input_properties[name].get("alias", name)
            return np.asarray(state[alias] if alias in state else state[name], dtype=np.float64)
        t, p_int = get("air_temperature"), get("air_pressure_on_interface_levels")
        levels = lambda x: np.reshape(x, (x.shape[0], -1))
        columns = lambda x: np.reshape(x, (-1,))
        fused = self._optical_depth is not None
        if fused:
            up, dn, tend, d = self._ctx.gray_longwave(levels(t), columns(get("surface_temperature")), levels(p_int), self.constants(),
                                                      ps=columns(get("surface_air_pressure")), lat=columns(get("latitude")),
                                                      frierson=self._optical_depth.parameters())
        else:
            up, dn, tend, d = self._ctx.gray_longwave(levels(t), columns(get("surface_temperature")), levels(p_int), self.constants(),
                                                      tau=levels(get(TAU)))
        diagnostics = {"downwelling_longwave_flux_in_air": np.reshape(dn, p_int.shape), "upwelling_longwave_flux_in_air": np.reshape(up, p_int.shape),
                       "air_temperature_tendency_from_longwave": np.reshape(d["hr"], t.shape)}
        if fused:
            diagnostics[TAU] = np.reshape(d["tau_out"], p_int.shape)
        return {"air_temperature": np.reshape(tend, t.shape)}, diagnostics
