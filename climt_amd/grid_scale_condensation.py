"""GridScaleCondensation -- drop-in for climt.GridScaleCondensation (climt/_components/grid_scale_condensation.py): grid-scale
supersaturation condensed layer by layer, all of it falling out as precipitation -- the moisture sink of the Frierson set-up.
Same constructor, property dictionaries and outputs; the per-column rule runs on the GPU through
rrtmg_hip_grid_scale_condensation (include/rrtmg_hip.h), one thread per column, in the reference's order of operations."""
import numpy as np

from ._sympl_compat import Stepper, get_constant
from .rrtmg.common import make_context


class GridScaleCondensation(Stepper):
    """
    Calculate condensation due to supersaturation of water.

    Condenses supersaturated water at the grid scale, assuming all
    condensed water falls as precipitation.

    One behaviour of the reference is kept as it is: the layer mass is formed from
    pint[k+1] - pint[k], which is negative where level 0 is the surface, so `precipitation_amount` comes out negative.
    The time step does not enter.
    """

    input_properties = {
        "air_temperature": {
            "dims": ["mid_levels", "*"],
            "units": "degK",
        },
        "specific_humidity": {
            "dims": ["mid_levels", "*"],
            "units": "kg/kg",
        },
        "air_pressure": {"dims": ["mid_levels", "*"], "units": "Pa"},
        "air_pressure_on_interface_levels": {
            "dims": ["interface_levels", "*"],
            "units": "Pa",
        },
    }

    diagnostic_properties = {
        "precipitation_amount": {
            "dims": ["*"],
            "units": "kg m^-2",
        }
    }

    output_properties = {
        "air_temperature": {"units": "degK"},
        "specific_humidity": {"units": "kg/kg"},
    }

    def __init__(self, device=0, context=None, **kwargs):
        """Args: the reference's (none of its own), plus `device` and `context` like the other components of this package."""
        super(GridScaleCondensation, self).__init__(**kwargs)
        self._ctx = context if context is not None else make_context(device)

    def constants(self):
        """The six constants of the reference's _update_constants as the library takes them, under the unit strings the reference
        asks with (asked for at every call)."""
        return dict(cpd=float(get_constant("heat_capacity_of_dry_air_at_constant_pressure", "J/kg/degK")),
                    lv=float(get_constant("latent_heat_of_condensation", "J/kg")), rd=float(get_constant("gas_constant_of_dry_air", "J/kg/degK")),
                    rh2o=float(get_constant("gas_constant_of_vapor_phase", "J/kg/degK")), g=float(get_constant("gravitational_acceleration", "m/s^2")),
                    rhow=float(get_constant("density_of_liquid_phase", "kg/m^3")))

    def __call__(self, state, timestep=None, *args, **kwargs):
        """A host state goes through sympl's machinery to array_call; a climt_amd.DeviceState (state resident in HBM) takes
        the device path and comes back rebound to the new profiles (climt_amd/device_state.py)."""
        from .device_state import DeviceState, grid_scale_condensation_device_call
        if isinstance(state, DeviceState):
            return grid_scale_condensation_device_call(self, state, timestep)
        return super(GridScaleCondensation, self).__call__(state, timestep, *args, **kwargs)

    def array_call(self, state, timestep):
        """-> (diagnostics, the updated profiles)."""
        t = np.asarray(state["air_temperature"], dtype=np.float64)
        levels = lambda x: np.reshape(np.asarray(x, dtype=np.float64), (np.shape(x)[0], -1))
        t_new, q_new, d = self._ctx.grid_scale_condensation(levels(t), levels(state["specific_humidity"]), levels(state["air_pressure"]),
                                                            levels(state["air_pressure_on_interface_levels"]), self.constants())
        return {"precipitation_amount": np.reshape(d["precip"], t.shape[1:])}, {
            "air_temperature": np.reshape(t_new, t.shape), "specific_humidity": np.reshape(q_new, t.shape)}
