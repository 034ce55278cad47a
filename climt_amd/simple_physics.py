"""SimplePhysics -- drop-in for climt.SimplePhysics (climt/_components/simple_physics/component.py around
climt/_lib/simple_physics/simple_physics_custom.f90): the Reed-Jablonowski package -- large-scale condensation, surface fluxes
and boundary-layer mixing -- and the only place in the reference's model scripts where grid-scale supersaturation is removed.
Same constructor, property dictionaries and outputs; the per-column rule runs on the GPU through rrtmg_hip_simple_physics
(include/rrtmg_hip.h), one thread per column, in the Fortran's order of operations."""
import numpy as np

from ._sympl_compat import Stepper, get_constant
from .rrtmg.common import make_context

_NAMES = ("air_temperature", "specific_humidity", "eastward_wind", "northward_wind")


class SimplePhysics(Stepper):
    """
    Interface to the simple physics package.

    Reed and Jablonowski 2012:
    title = {Idealized tropical cyclone simulations of intermediate complexity: a test case for {AGCMs}}
    journal = {Journal of Advances in Modeling Earth Systems}

    Two behaviours of the reference are kept as they are: `simulate_cyclone=True` selects the moist
    baroclinic wave's latitude-dependent surface temperature and `False` the cyclone's constant 302.15 K (both are read only with
    `use_external_surface_temperature=False`, and `latitude` in degrees_north is taken as radians), and the latent heat flux
    diagnostic is clamped at 0 after the humidity has taken the negative flux.
    """

    input_properties = {
        "air_temperature": {
            "dims": ["mid_levels", "*"],
            "units": "degK",
        },
        "air_pressure": {
            "dims": ["mid_levels", "*"],
            "units": "Pa",
        },
        "air_pressure_on_interface_levels": {
            "dims": ["interface_levels", "*"],
            "units": "Pa",
        },
        "surface_air_pressure": {
            "dims": ["*"],
            "units": "Pa",
        },
        "surface_temperature": {
            "dims": ["*"],
            "units": "degK",
        },
        "specific_humidity": {
            "dims": ["mid_levels", "*"],
            "units": "kg/kg",
        },
        "northward_wind": {
            "dims": ["mid_levels", "*"],
            "units": "m s^-1",
        },
        "eastward_wind": {
            "dims": ["mid_levels", "*"],
            "units": "m s^-1",
        },
        "surface_specific_humidity": {
            "dims": ["*"],
            "units": "kg/kg",
        },
        "latitude": {
            "dims": ["*"],
            "units": "degrees_north",
        },
    }

    diagnostic_properties = {
        "stratiform_precipitation_rate": {
            "dims": ["*"],
            "units": "m s^-1",
        },
        "surface_upward_latent_heat_flux": {
            "dims": ["*"],
            "units": "W m^-2",
        },
        "surface_upward_sensible_heat_flux": {
            "dims": ["*"],
            "units": "W m^-2",
        },
    }

    output_properties = {
        "air_temperature": {"units": "degK"},
        "specific_humidity": {"units": "kg/kg"},
        "northward_wind": {"units": "m s^-1"},
        "eastward_wind": {"units": "m s^-1"},
    }

    def __init__(
        self,
        simulate_cyclone=False,
        large_scale_condensation=True,
        boundary_layer=True,
        surface_fluxes=True,
        use_external_surface_temperature=True,
        use_external_surface_specific_humidity=False,
        top_of_boundary_layer=85000.0,
        boundary_layer_influence_height=20000.0,
        drag_coefficient_heat_fluxes=0.0011,
        base_momentum_drag_coefficient=0.0007,
        wind_dependent_momentum_drag_coefficient=0.000065,
        maximum_momentum_drag_coefficient=0.002,
        device=0,
        context=None,
        **kwargs
    ):
        """
        Args: the reference's (climt.SimplePhysics), word for word in names and defaults; plus `device` and `context` like the
        other components of this package.

            simulate_cyclone (bool): handed to the rule as `test`; see the class docstring.  Default False.
            large_scale_condensation (bool): remove grid-scale supersaturation.  Default True.
            boundary_layer (bool): the implicit boundary-layer mixing.  Needs `surface_fluxes`.  Default True.
            surface_fluxes (bool): the surface fluxes of momentum, heat and moisture on the lowest layer.  Default True.
            use_external_surface_temperature (bool): `surface_temperature` of the state, else an internal one.  Default True.
            use_external_surface_specific_humidity (bool): `surface_specific_humidity` of the state, else the saturation
                value of the surface temperature.  Default False.
            top_of_boundary_layer (float): Pa.  boundary_layer_influence_height (float): Pa.
            drag_coefficient_heat_fluxes, base_momentum_drag_coefficient, wind_dependent_momentum_drag_coefficient,
            maximum_momentum_drag_coefficient (float): Smith and Vogl 2008.
        """
        if boundary_layer and not surface_fluxes:
            raise ValueError("boundary_layer=True needs surface_fluxes=True: the mixing reads the surface diffusivities and the drag coefficient "
                             "that only the surface step sets (the reference reads them unset; there is nothing to reproduce)")
        self._cyclone = simulate_cyclone
        self._lsc = large_scale_condensation
        self._pbl = boundary_layer
        self._surface_flux = surface_fluxes
        self._use_ext_ts = use_external_surface_temperature
        self._use_ext_qsurf = use_external_surface_specific_humidity
        self._Ct = drag_coefficient_heat_fluxes
        self._pbl_top = top_of_boundary_layer
        self._delta_pbl = boundary_layer_influence_height
        self._Cd0 = base_momentum_drag_coefficient
        self._Cd1 = wind_dependent_momentum_drag_coefficient
        self._Cm = maximum_momentum_drag_coefficient
        super(SimplePhysics, self).__init__(**kwargs)
        self._ctx = context if context is not None else make_context(device)

    def constants(self):
        """The fourteen constants of the reference's set_fortran_constants as the library takes them: the physical ones through
        get_constant at every call (component.py:191-201), under the unit strings the reference asks with; the others the constructor's."""
        return dict(g=get_constant("gravitational_acceleration", "m/s^2"),
                    cpair=get_constant("heat_capacity_of_dry_air_at_constant_pressure", "J/kg/degK"),
                    rair=get_constant("gas_constant_of_dry_air", "J/kg/degK"), latvap=get_constant("latent_heat_of_condensation", "J/kg"),
                    rh2o=get_constant("gas_constant_of_vapor_phase", "J/kg/degK"), radius=get_constant("planetary_radius", "m"),
                    omega=get_constant("planetary_rotation_rate", "s^-1"), rhow=get_constant("density_of_liquid_water", "kg/m^3"),
                    pbltop=float(self._pbl_top), pblconst=float(self._delta_pbl), c_heat=float(self._Ct), cd0=float(self._Cd0),
                    cd1=float(self._Cd1), cm=float(self._Cm))

    def switches(self):
        """The rule's switches: the constructor's options as the reference's binder hands them on (simulate_cyclone as `test`), and
        the clamp of the latent heat flux that component.py applies after the call."""
        return dict(do_lsc=int(bool(self._lsc)), do_pbl=int(bool(self._pbl)), do_surf_flux=int(bool(self._surface_flux)),
                    use_ts_ext=int(bool(self._use_ext_ts)), use_qsurf_ext=int(bool(self._use_ext_qsurf)), test=int(bool(self._cyclone)),
                    clamp_latent_heat_flux=1)

    def __call__(self, state, timestep=None, *args, **kwargs):
        """A host state goes through sympl's machinery to array_call; a climt_amd.DeviceState (state resident in HBM) takes
        the device path and comes back rebound to the new profiles (climt_amd/device_state.py)."""
        from .device_state import DeviceState, simple_physics_device_call
        if isinstance(state, DeviceState):
            return simple_physics_device_call(self, state, timestep)
        return super(SimplePhysics, self).__call__(state, timestep, *args, **kwargs)

    def array_call(self, state, timestep):
        """Calculate surface and boundary layer tendencies: -> (diagnostics, the updated profiles)."""
        t = np.asarray(state["air_temperature"], dtype=np.float64)
        levels = lambda x: np.reshape(np.asarray(x, dtype=np.float64), (np.shape(x)[0], -1))
        columns = lambda x: np.reshape(np.asarray(x, dtype=np.float64), (-1,))
        t_new, q_new, u_new, v_new, d = self._ctx.simple_physics(
            levels(t), levels(state["specific_humidity"]), levels(state["eastward_wind"]), levels(state["northward_wind"]),
            levels(state["air_pressure"]), levels(state["air_pressure_on_interface_levels"]), columns(state["surface_air_pressure"]),
            timestep.total_seconds(), self.constants(), self.switches(), ts=columns(state["surface_temperature"]),
            qsurf=columns(state["surface_specific_humidity"]), lat=columns(state["latitude"]))
        wild = np.shape(state["surface_temperature"])
        diagnostics = {"stratiform_precipitation_rate": np.reshape(d["precl"], wild),
                       "surface_upward_sensible_heat_flux": np.reshape(d["sh_out"], wild),
                       "surface_upward_latent_heat_flux": np.reshape(d["lh_out"], wild)}
        return diagnostics, {"air_temperature": np.reshape(t_new, t.shape), "specific_humidity": np.reshape(q_new, t.shape),
                             "northward_wind": np.reshape(v_new, t.shape), "eastward_wind": np.reshape(u_new, t.shape)}
