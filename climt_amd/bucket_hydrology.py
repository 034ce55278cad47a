"""BucketHydrology -- a drop-in for climt.BucketHydrology (climt/_components/bucket_hydrology/component.py): the surface energy
and moisture balance of a land slab with one or two soil-moisture layers.  Bulk sensible and latent heat fluxes from the lowest
model level, beta-limited evaporation, precipitation as an input; with two layers the exchange with a deep store, drainage,
runoff and the deep temperature.  Same constructor, property dictionaries and outputs; the rule runs on the GPU through
rrtmg_hip_bucket_hydrology (include/rrtmg_hip.h), one thread per column, in the reference's order of operations.  Like the
reference it steps every column, whatever its area type."""
import numpy as np

from ._sympl_compat import Stepper, get_constant
from .rrtmg.common import make_context

_FLUX = lambda: {"dims": ["*", "interface_levels"], "units": "W m^-2"}
_MID = lambda units: {"dims": ["mid_levels", "*"], "units": units}
_COL = lambda units: {"dims": ["*"], "units": units}
# the library's names (climt_amd/_lib.py: BUCKET_HYDROLOGY_IN, _OUT, _DIAG) -> the quantities
INPUT_NAMES = dict(t_air="air_temperature", q_air="specific_humidity", u="eastward_wind", v="northward_wind", p_air="air_pressure",
                   ts="surface_temperature", q_sfc="surface_specific_humidity", sw_down="downwelling_shortwave_flux_in_air",
                   lw_down="downwelling_longwave_flux_in_air", sw_up="upwelling_shortwave_flux_in_air", lw_up="upwelling_longwave_flux_in_air",
                   soil_moisture="lwe_thickness_of_soil_moisture_content", precip_conv="convective_precipitation_rate",
                   precip_strat="stratiform_precipitation_rate", density="surface_material_density", thickness="soil_layer_thickness",
                   heat_capacity="heat_capacity_of_soil", deep_moisture="deep_soil_moisture_content", deep_temperature="deep_soil_temperature")
OUTPUT_NAMES = dict(ts_out="surface_temperature", soil_moisture_out="lwe_thickness_of_soil_moisture_content",
                    deep_moisture_out="deep_soil_moisture_content", deep_temperature_out="deep_soil_temperature")
DIAGNOSTIC_NAMES = dict(precip="precipitation_rate", lh="surface_upward_latent_heat_flux", sh="surface_upward_sensible_heat_flux",
                        evaporation="evaporation_rate", runoff="runoff_rate", deep_fraction="deep_soil_moisture_fraction")
DEFAULT_DIFFUSION_TIMESCALE = 5 * 86400.0      # the reference's, where moisture_diffusion_timescale is None


class BucketHydrology(Stepper):
    """
    Manages surface energy and moisture balance.

    The surface is a slab with some heat capacity and moisture holding capacity.  Calculates the sensible and latent heat flux and
    takes precipitation values as input.  With ``num_layers=2`` a deep soil store exchanges moisture and heat with the slab.
    """

    input_properties = {
        "downwelling_longwave_flux_in_air": _FLUX(),
        "downwelling_shortwave_flux_in_air": _FLUX(),
        "upwelling_longwave_flux_in_air": _FLUX(),
        "upwelling_shortwave_flux_in_air": _FLUX(),
        "surface_temperature": _COL("degK"),
        "surface_material_density": _COL("kg m^-3"),
        "soil_layer_thickness": _COL("m"),
        "heat_capacity_of_soil": _COL("J kg^-1 degK^-1"),
        "lwe_thickness_of_soil_moisture_content": _COL("m"),
        "convective_precipitation_rate": _COL("m s^-1"),
        "stratiform_precipitation_rate": _COL("m s^-1"),
        "specific_humidity": _MID("kg/kg"),
        "surface_specific_humidity": _COL("kg/kg"),
        "air_temperature": _MID("degK"),
        "air_pressure": _MID("Pa"),
        "northward_wind": _MID("m s^-1"),
        "eastward_wind": _MID("m s^-1"),
        "area_type": _COL("dimensionless"),
    }

    diagnostic_properties = {
        "precipitation_rate": _COL("m s^-1"),
        "surface_upward_latent_heat_flux": _COL("W m^-2"),
        "surface_upward_sensible_heat_flux": _COL("W m^-2"),
        "evaporation_rate": _COL("m s^-1"),
    }

    output_properties = {
        "surface_temperature": _COL("degK"),
        "lwe_thickness_of_soil_moisture_content": _COL("m"),
    }

    def __init__(self, num_layers=1, soil_moisture_max=0.15, beta_parameter=0.75, specific_latent_heat_of_water=2260000, bulk_coefficient=0.0011,
                 deep_soil_moisture_max=0.50, moisture_diffusion_timescale=None, deep_layer_thickness_ratio=10.0, deep_drainage_timescale=None,
                 device=0, context=None, **kwargs):
        """Args: the reference's -- the number of soil moisture layers (1 or 2), the moisture the slab can hold, the constant of
        the beta factor, the latent heat, the bulk transfer coefficient and, for two layers, the moisture the deep layer can hold,
        the time scale of the exchange between the layers (None: five days), the ratio of the layers' thicknesses and the time
        scale of the drainage out of the deep layer (None: none) -- plus `device` and `context` like the other components of this
        package."""
        if num_layers not in (1, 2):
            raise ValueError("num_layers must be 1 or 2")
        self._num_layers = num_layers
        self._smax = soil_moisture_max
        self._g = beta_parameter
        self._c = bulk_coefficient
        self._l = specific_latent_heat_of_water
        self._deep_smax = deep_soil_moisture_max
        self._tau_m = moisture_diffusion_timescale
        self._deep_ratio = deep_layer_thickness_ratio
        self._tau_drain = deep_drainage_timescale
        if num_layers == 2:      # per instance, as in the reference: a one-layer instance keeps the class's interface
            self.input_properties = dict(self.input_properties, deep_soil_moisture_content=_COL("m"), deep_soil_temperature=_COL("degK"))
            self.output_properties = dict(self.output_properties, deep_soil_moisture_content=_COL("m"), deep_soil_temperature=_COL("degK"))
            self.diagnostic_properties = dict(self.diagnostic_properties, runoff_rate=_COL("m s^-1"), deep_soil_moisture_fraction=_COL("dimensionless"))
        super(BucketHydrology, self).__init__(**kwargs)
        self._ctx = context if context is not None else make_context(device)

    def scalars(self):
        """The three constants under the unit strings the reference asks with (asked for at every call) and the component's own
        parameters, as the library takes them (_lib.BUCKET_HYDROLOGY_SCALARS)."""
        return dict(rd=float(get_constant("gas_constant_of_dry_air", "J kg^-1 K^-1")), rho_water=float(get_constant("density_of_liquid_water", "kg m^-3")),
                    cp=float(get_constant("heat_capacity_of_dry_air_at_constant_pressure", "J kg^-1 K^-1")), lv=float(self._l),
                    bulk_coefficient=float(self._c), beta_parameter=float(self._g), soil_moisture_max=float(self._smax),
                    deep_soil_moisture_max=float(self._deep_smax), tau_m=float(self._tau_m) if self._tau_m is not None else DEFAULT_DIFFUSION_TIMESCALE,
                    deep_ratio=float(self._deep_ratio), tau_drain=None if self._tau_drain is None else float(self._tau_drain))

    def names(self, table):
        """The part of INPUT_NAMES / OUTPUT_NAMES / DIAGNOSTIC_NAMES this instance's layer count has."""
        deep = ("deep_moisture", "deep_temperature", "deep_moisture_out", "deep_temperature_out", "runoff", "deep_fraction")
        return {k: v for k, v in table.items() if self._num_layers == 2 or k not in deep}

    def __call__(self, state, timestep=None, *args, **kwargs):
        """A host state goes through sympl's machinery to array_call; a climt_amd.DeviceState (state resident in HBM) takes
        the device path and comes back rebound to the new surface (climt_amd/device_state.py)."""
        from .device_state import DeviceState, bucket_hydrology_device_call
        if isinstance(state, DeviceState):
            return bucket_hydrology_device_call(self, state, timestep)
        return super(BucketHydrology, self).__call__(state, timestep, *args, **kwargs)

    def array_call(self, raw_state, timestep):
        """-> (diagnostics, outputs), as the reference returns them."""
        wild = np.shape(raw_state["surface_temperature"])
        flat = lambda x: np.ascontiguousarray(np.reshape(np.asarray(x, dtype=np.float64), (-1,)))
        arrays = {}
        for k, name in self.names(INPUT_NAMES).items():
            x = np.asarray(raw_state[name], dtype=np.float64)
            dims = self.input_properties[name]["dims"]
            if dims[0] == "mid_levels":
                x = x[0]                      # the lowest model level
            elif dims[-1] == "interface_levels" and x.ndim > len(wild):
                x = x[..., 0]                 # the surface
            arrays[k] = flat(x)
        o, d = self._ctx.bucket_hydrology(self._num_layers, arrays, float(timestep.total_seconds()), self.scalars())
        col = lambda x: np.reshape(x, wild)
        return ({name: col(d[k]) for k, name in self.names(DIAGNOSTIC_NAMES).items()}, {name: col(o[k]) for k, name in self.names(OUTPUT_NAMES).items()})
