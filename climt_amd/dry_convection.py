"""DryConvectiveAdjustment -- drop-in for climt.DryConvectiveAdjustment (climt/_components/dry_convection/component.py): the
step a radiative-convective column model puts behind the radiation and the slab (the reference's
examples/column_code_with_slab.py).  Same property dictionaries and outputs; the per-column sweep (component.py:84-152) runs on
the GPU through rrtmg_hip_dry_adjustment (include/rrtmg_hip.h), one thread per column, in the reference's order of operations."""
import numpy as np

from ._sympl_compat import Stepper, get_constant
from .rrtmg.common import make_context


class DryConvectiveAdjustment(Stepper):
    """
    A conservative scheme to keep the temperature profile close to the
    dry adiabat if it is super-adiabatic.
    """

    input_properties = {
        "air_temperature": {
            "units": "degK",
            "dims": ["mid_levels", "*"],
        },
        "air_pressure": {
            "units": "Pa",
            "dims": ["mid_levels", "*"],
        },
        "air_pressure_on_interface_levels": {
            "units": "Pa",
            "dims": ["interface_levels", "*"],
            "alias": "P_int",
        },
        "specific_humidity": {
            "units": "kg/kg",
            "dims": ["mid_levels", "*"],
        },
    }

    output_properties = {
        "air_temperature": {
            "units": "degK",
        },
        "specific_humidity": {
            "units": "kg/kg",
        },
    }

    diagnostic_properties = {}

    def __init__(self, device=0, context=None, **kwargs):
        super(DryConvectiveAdjustment, self).__init__(**kwargs)
        self._ctx = context if context is not None else make_context(device)

    @staticmethod
    def constants(pressure_units="Pa"):
        """cpd, cvap, rd, rv and pref as the library takes them (component.py:66-74), pref in `pressure_units`."""
        pref = get_constant("reference_air_pressure", "Pa")
        if pressure_units != "Pa":
            from .device_state import _convert
            pref = float(_convert(np.float64(pref), "Pa", pressure_units))
        return dict(cpd=get_constant("heat_capacity_of_dry_air_at_constant_pressure", "J/kg/degK"),
                    cvap=get_constant("heat_capacity_of_vapor_phase", "J/kg/K"),
                    rd=get_constant("gas_constant_of_dry_air", "J/kg/degK"),
                    rv=get_constant("gas_constant_of_vapor_phase", "J/kg/K"), pref=pref)

    def __call__(self, state, timestep=None, *args, **kwargs):
        """A host state goes through sympl's machinery to array_call; a climt_amd.DeviceState (state resident in HBM) takes
        the device path and comes back rebound to the adjusted arrays (climt_amd/device_state.py)."""
        from .device_state import DeviceState, dry_adjustment_device_call
        if isinstance(state, DeviceState):
            return dry_adjustment_device_call(self, state, timestep)
        return super(DryConvectiveAdjustment, self).__call__(state, timestep, *args, **kwargs)

    def array_call(self, state, time_step):
        t = np.asarray(state["air_temperature"], dtype=np.float64)
        p_int = state["P_int"] if "P_int" in state else state["air_pressure_on_interface_levels"]
        flat = lambda x: np.reshape(np.asarray(x, dtype=np.float64), (np.shape(x)[0], -1))
        t_new, q_new, _ = self._ctx.dry_adjustment(flat(t), flat(state["specific_humidity"]), flat(state["air_pressure"]), flat(p_int),
                                                   self.constants())
        return {}, {
            "air_temperature": np.reshape(t_new, t.shape),
            "specific_humidity": np.reshape(q_new, t.shape),
        }
