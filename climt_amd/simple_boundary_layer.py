"""SimpleBoundaryLayer -- drop-in for climt.SimpleBoundaryLayer (climt/_components/simple_boundary_layer/component.py): the
producer of the surface fluxes SlabSurface consumes, and the atmosphere's side of them.  Same constructor, property dictionaries
and outputs; the per-column rule (component.py:89-242 with _core/tridiagonal.py) runs on the GPU through
rrtmg_hip_boundary_layer (include/rrtmg_hip.h), one thread per column, in the reference's order of operations."""
import numpy as np

from ._sympl_compat import Stepper, get_constant
from .rrtmg.common import make_context

_FLUX_MODES = {None: 0, "bulk": 1, "external": 2}
_FLUXES = ("surface_upward_sensible_heat_flux", "surface_upward_latent_heat_flux")


class SimpleBoundaryLayer(Stepper):
    """A simple boundary-layer scheme that exchanges heat, moisture and momentum with the surface and diffuses them through the
    boundary layer (Frierson, Held & Zurita-Gotor 2006; diffusivities from a simplified Monin-Obukhov theory with a K-profile
    capped by a critical Richardson number).  `surface_fluxes`:

    * ``'bulk'`` (default) -- the component computes the bulk fluxes from its own exchange coefficient and applies them
      implicitly; the applied heat and moisture fluxes are the diagnostics ``surface_upward_sensible_heat_flux`` and
      ``surface_upward_latent_heat_flux``.  Momentum uses a no-slip surface value.
    * ``'external'`` -- the two flux quantities are required inputs, applied as prescribed.  Momentum keeps the bulk drag.
    * ``None`` -- no surface exchange: every column integral is conserved.

    ``northward_wind_stress`` and ``eastward_wind_stress`` report the drag on the post-solve layer-0 winds in every mode
    (advisory with ``None``: nothing applies them)."""

    input_properties = {
        "air_temperature": {"dims": ["mid_levels", "*"], "units": "degK"},
        "specific_humidity": {"dims": ["mid_levels", "*"], "units": "kg/kg"},
        "air_pressure": {"dims": ["mid_levels", "*"], "units": "Pa"},
        "air_pressure_on_interface_levels": {"dims": ["interface_levels", "*"], "units": "Pa"},
        "northward_wind": {"dims": ["mid_levels", "*"], "units": "m s^-1"},
        "eastward_wind": {"dims": ["mid_levels", "*"], "units": "m s^-1"},
        "surface_air_pressure": {"dims": ["*"], "units": "Pa"},
        "surface_temperature": {"dims": ["*"], "units": "degK"},
        "surface_specific_humidity": {"dims": ["*"], "units": "kg/kg"},
    }

    output_properties = {
        "air_temperature": {"dims": ["mid_levels", "*"], "units": "degK"},
        "specific_humidity": {"dims": ["mid_levels", "*"], "units": "kg/kg"},
        "northward_wind": {"dims": ["mid_levels", "*"], "units": "m s^-1"},
        "eastward_wind": {"dims": ["mid_levels", "*"], "units": "m s^-1"},
    }

    diagnostic_properties = {
        "northward_wind_stress": {"dims": ["*"], "units": "Pa"},
        "eastward_wind_stress": {"dims": ["*"], "units": "Pa"},
        "boundary_layer_height": {"dims": ["*"], "units": "m"},
    }

    def __init__(self, surface_fluxes="bulk", von_karman_constant=0.4, roughness_length=0.0000321, specific_fraction=0.1,
                 reference_pressure=100000, critical_richardson_number=1, device=0, context=None, **kwargs):
        if surface_fluxes not in _FLUX_MODES:
            raise ValueError("surface_fluxes must be 'bulk', 'external' or None, got %r" % (surface_fluxes,))
        self._surface_fluxes = surface_fluxes
        self._flux_mode = _FLUX_MODES[surface_fluxes]
        self._k = von_karman_constant
        self._z0 = roughness_length
        self._fb = specific_fraction
        self._P0 = reference_pressure
        self._Ric = critical_richardson_number
        flux = {"dims": ["*"], "units": "W m^-2"}
        if surface_fluxes == "bulk":          # per instance: only bulk mode reports the fluxes it applied
            self.diagnostic_properties = dict(self.diagnostic_properties, **{n: dict(flux) for n in _FLUXES})
        elif surface_fluxes == "external":    # per instance: only external mode consumes another component's fluxes
            self.input_properties = dict(self.input_properties, **{n: dict(flux) for n in _FLUXES})
        super(SimpleBoundaryLayer, self).__init__(**kwargs)
        self._ctx = context if context is not None else make_context(device)

    def constants(self):
        """rd, cp, g, lv, karman, z0, fb, p0 and ric as the library takes them: the physical ones through get_constant at every
        call (component.py:385-391), the others the constructor's."""
        return dict(rd=get_constant("gas_constant_of_dry_air", "J kg^-1 K^-1"),
                    cp=get_constant("heat_capacity_of_dry_air_at_constant_pressure", "J kg^-1 K^-1"),
                    g=get_constant("gravitational_acceleration", "m s^-2"), lv=get_constant("latent_heat_of_condensation", "J kg^-1"),
                    karman=float(self._k), z0=float(self._z0), fb=float(self._fb), p0=float(self._P0), ric=float(self._Ric))

    def __call__(self, state, timestep=None, *args, **kwargs):
        """A host state goes through sympl's machinery to array_call; a climt_amd.DeviceState (state resident in HBM) takes
        the device path and comes back rebound to the new profiles (climt_amd/device_state.py)."""
        from .device_state import DeviceState, boundary_layer_device_call
        if isinstance(state, DeviceState):
            return boundary_layer_device_call(self, state, timestep)
        return super(SimpleBoundaryLayer, self).__call__(state, timestep, *args, **kwargs)

    def array_call(self, state, timestep):
        """Diffuse temperature, humidity and wind profiles for each column."""
        t = np.asarray(state["air_temperature"], dtype=np.float64)
        levels = lambda x: np.reshape(np.asarray(x, dtype=np.float64), (np.shape(x)[0], -1))
        columns = lambda x: np.reshape(np.asarray(x, dtype=np.float64), (-1,))
        fluxes = {}
        if self._flux_mode == 2:
            fluxes = dict(sh_in=columns(state[_FLUXES[0]]), lh_in=columns(state[_FLUXES[1]]))
        t_new, q_new, u_new, v_new, d = self._ctx.boundary_layer(
            levels(t), levels(state["specific_humidity"]), levels(state["eastward_wind"]), levels(state["northward_wind"]),
            levels(state["air_pressure"]), levels(state["air_pressure_on_interface_levels"]), columns(state["surface_air_pressure"]),
            columns(state["surface_temperature"]), columns(state["surface_specific_humidity"]), timestep.total_seconds(),
            self.constants(), self._flux_mode, **fluxes)
        wild = np.shape(state["surface_temperature"])
        diagnostics = {"northward_wind_stress": np.reshape(d["stress_north"], wild), "eastward_wind_stress": np.reshape(d["stress_east"], wild),
                       "boundary_layer_height": np.reshape(d["height"], wild)}
        if self._flux_mode == 1:
            diagnostics.update({_FLUXES[0]: np.reshape(d["sh_out"], wild), _FLUXES[1]: np.reshape(d["lh_out"], wild)})
        return diagnostics, {"air_temperature": np.reshape(t_new, t.shape), "specific_humidity": np.reshape(q_new, t.shape),
                             "northward_wind": np.reshape(v_new, t.shape), "eastward_wind": np.reshape(u_new, t.shape)}
