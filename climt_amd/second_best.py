"""SecondBEST -- a drop-in for climt.SecondBEST (climt/_components/second_best/): the intermediate-complexity BEST land surface
over ``area_type in ("land", "land_ice")`` cells.  Surface-layer drag in both stability branches, the wetness-dependent albedo,
bulk sensible heat and beta-limited evaporation, an implicit soil heat column with freeze and melt, and the screen-level
diagnostics.  Same constructor, property dictionaries and outputs.  The reference delegates each calculation to a process
object and loops over the columns in Python; here the BEST default of every process is ONE rule per column, which runs on the
GPU through rrtmg_hip_second_best (include/rrtmg_hip.h), one thread per column, in the reference's order of operations.  The
five ``Best*`` classes are parameter holders: a process argument that is anything else cannot be run by the device rule and
raises NotImplementedError."""
import numpy as np

from ._sympl_compat import Stepper, get_constant
from .rrtmg.common import make_context
from .surface_ice import area_codes

_FLUX = lambda: {"dims": ["*", "interface_levels"], "units": "W m^-2"}
_MID = lambda units: {"dims": ["mid_levels", "*"], "units": units}
_SOIL = lambda units: {"dims": ["soil_interface_levels", "*"], "units": units}
_COL = lambda units: {"dims": ["*"], "units": units}
# the library's names (climt_amd/_lib.py: SECOND_BEST_IN, _OUT, _DIAG) -> the quantities
INPUT_NAMES = dict(t_soil="soil_temperature", x_w="soil_liquid_water_content", x_i="soil_ice_content", height="height_on_soil_interface_levels",
                   t_air="air_temperature", q_air="specific_humidity", u="eastward_wind", v="northward_wind", p_air="air_pressure",
                   ps="surface_air_pressure", ts="surface_temperature", snow="surface_snow_thickness", sw_down="downwelling_shortwave_flux_in_air",
                   lw_down="downwelling_longwave_flux_in_air", sw_up="upwelling_shortwave_flux_in_air", lw_up="upwelling_longwave_flux_in_air")
OUTPUT_NAMES = dict(t_soil_out="soil_temperature", x_w_out="soil_liquid_water_content", x_i_out="soil_ice_content", ts_out="surface_temperature",
                    snow_out="surface_snow_thickness")
DIAGNOSTIC_NAMES = dict(sh="surface_upward_sensible_heat_flux", lh="surface_upward_latent_heat_flux", evaporation="evaporation_rate",
                        albedo_direct="surface_albedo_for_direct_shortwave", albedo_diffuse="surface_albedo_for_diffuse_shortwave",
                        cd_heat="surface_drag_coefficient_for_heat", cd_momentum="surface_drag_coefficient_for_momentum", t2m="air_temperature_at_2m",
                        q2m="specific_humidity_at_2m", u10="eastward_wind_at_10m", v10="northward_wind_at_10m")
FLAG_ACTIVE, FLAG_UNSTABLE, FLAG_CAPPED = 1, 2, 4
# the soil table of BEST by soil type: colour, texture, B, K_H0 (psi_0 is -0.2 for both); over land ice the rule takes texture 0.07
SOIL_TYPES = {"clay": dict(colour=0.2, texture=0.0, B=10.0, K_H0=0.001), "sand": dict(colour=1.0, texture=9.0, B=4.0, K_H0=0.1)}
PSI_0 = -0.2


class BestSoilProperties(object):
    """The BEST soil table (no parameters): selects the device rule's default."""


class BestSurfaceAlbedo(object):
    """The BEST surface albedo (no parameters): selects the device rule's default."""


class BestSurfaceLayer(object):
    """The BEST surface-layer drag (no parameters): selects the device rule's default."""


class BestSurfaceFluxes(object):
    """The BEST bulk surface fluxes (no parameters): selects the device rule's default."""


class BestSubsurfaceTransport(object):
    """The BEST soil heat column; its two parameters are honoured by the device rule."""

    def __init__(self, thermal_conductivity=2.0, volumetric_heat_capacity=2.0e6):
        self._kappa = thermal_conductivity
        self._cv = volumetric_heat_capacity


_PROCESSES = (("soil_properties", BestSoilProperties), ("albedo", BestSurfaceAlbedo), ("surface_layer", BestSurfaceLayer),
              ("fluxes", BestSurfaceFluxes), ("subsurface", BestSubsurfaceTransport))


class SecondBEST(Stepper):
    """Intermediate-complexity BEST land surface model.

    Every process argument is ``None`` (the BEST default) or an instance of the matching ``Best*`` class; the device rule is
    the BEST default, so anything else raises NotImplementedError.
    """

    input_properties = {
        "air_temperature": _MID("degK"),
        "specific_humidity": _MID("kg/kg"),
        "northward_wind": _MID("m s^-1"),
        "eastward_wind": _MID("m s^-1"),
        "air_pressure": _MID("Pa"),
        "downwelling_shortwave_flux_in_air": _FLUX(),
        "downwelling_longwave_flux_in_air": _FLUX(),
        "upwelling_shortwave_flux_in_air": _FLUX(),
        "upwelling_longwave_flux_in_air": _FLUX(),
        "area_type": _COL("dimensionless"),
        "surface_temperature": _COL("degK"),
        "surface_air_pressure": _COL("Pa"),
        "soil_temperature": _SOIL("degK"),
        "soil_liquid_water_content": _SOIL("m^3/m^3"),
        "soil_ice_content": _SOIL("m^3/m^3"),
        "surface_snow_thickness": _COL("m"),
        "height_on_soil_interface_levels": _SOIL("m"),
    }
    output_properties = {
        "surface_temperature": _COL("degK"),
        "soil_temperature": _SOIL("degK"),
        "soil_liquid_water_content": _SOIL("m^3/m^3"),
        "soil_ice_content": _SOIL("m^3/m^3"),
        "surface_snow_thickness": _COL("m"),
    }
    diagnostic_properties = {
        "surface_upward_sensible_heat_flux": _COL("W m^-2"),
        "surface_upward_latent_heat_flux": _COL("W m^-2"),
        "evaporation_rate": _COL("m s^-1"),
        "surface_albedo_for_direct_shortwave": _COL("dimensionless"),
        "surface_albedo_for_diffuse_shortwave": _COL("dimensionless"),
        "surface_drag_coefficient_for_heat": _COL("dimensionless"),
        "surface_drag_coefficient_for_momentum": _COL("dimensionless"),
        "air_temperature_at_2m": _COL("degK"),
        "specific_humidity_at_2m": _COL("kg/kg"),
        "eastward_wind_at_10m": _COL("m s^-1"),
        "northward_wind_at_10m": _COL("m s^-1"),
    }

    def __init__(self, soil_type="clay", num_soil_layers=3, minimum_wind_speed=1.0, soil_properties=None, albedo=None, surface_layer=None,
                 fluxes=None, subsurface=None, device=0, context=None, **kwargs):
        """Args: the reference's -- the soil type ("clay" or "sand"), the number of soil layers (kept; the soil arrays of the
        state decide), the floor of the wind speed, and the five processes (None, or an instance of the matching Best* class) --
        plus `device` and `context` like the other components of this package."""
        given = dict(soil_properties=soil_properties, albedo=albedo, surface_layer=surface_layer, fluxes=fluxes, subsurface=subsurface)
        for name, cls in _PROCESSES:
            if given[name] is not None and not isinstance(given[name], cls):
                raise NotImplementedError("SecondBEST: %s must be None or a %s: the device rule is the BEST default and cannot run another process" % (name, cls.__name__))
        if soil_type not in SOIL_TYPES:
            raise KeyError(soil_type)
        self._soil_type = soil_type
        self._num_soil_layers = num_soil_layers
        self._min_wind = minimum_wind_speed
        self._subsurface = subsurface if subsurface is not None else BestSubsurfaceTransport()
        super(SecondBEST, self).__init__(**kwargs)
        self._ctx = context if context is not None else make_context(device)

    def constants(self):
        """The constants under the unit strings the reference's component and processes ask with (asked for at every call), the
        soil type as numbers and the component's own parameters, as the library takes them (_lib.SECOND_BEST_CONSTANTS)."""
        return dict(rd=float(get_constant("gas_constant_of_dry_air", "J/kg/degK")), g=float(get_constant("gravitational_acceleration", "m/s^2")),
                    cp=float(get_constant("heat_capacity_of_dry_air_at_constant_pressure", "J/kg/degK")), lv=float(get_constant("latent_heat_of_vaporization", "J/kg")),
                    lf=float(get_constant("latent_heat_of_fusion", "J/kg")), rho_water=float(get_constant("density_of_liquid_water", "kg/m^3")),
                    karman=float(get_constant("von_karman_constant", "dimensionless")), t_freeze=float(get_constant("freezing_temperature_of_liquid_phase", "degK")),
                    min_wind=float(self._min_wind), kappa_soil=float(self._subsurface._kappa), cv_soil=float(self._subsurface._cv), psi_0=PSI_0,
                    **SOIL_TYPES[self._soil_type])

    def __call__(self, state, timestep=None, *args, **kwargs):
        """A host state goes through sympl's machinery to array_call; a climt_amd.DeviceState (state resident in HBM) takes
        the device path and comes back rebound to the new soil column (climt_amd/device_state.py)."""
        from .device_state import DeviceState, second_best_device_call
        if isinstance(state, DeviceState):
            return second_best_device_call(self, state, timestep)
        return super(SecondBEST, self).__call__(state, timestep, *args, **kwargs)

    def array_call(self, raw_state, timestep):
        """-> (diagnostics, outputs), as the reference returns them."""
        t_soil = np.asarray(raw_state["soil_temperature"], dtype=np.float64)
        wild = t_soil.shape[1:]
        arrays = {"area_type": area_codes(raw_state["area_type"]).reshape(-1)}
        for k, name in INPUT_NAMES.items():
            x = np.asarray(raw_state[name], dtype=np.float64)
            dims = self.input_properties[name]["dims"]
            if dims[0] == "soil_interface_levels":
                arrays[k] = np.ascontiguousarray(x.reshape(x.shape[0], -1))
                continue
            if dims[0] == "mid_levels":
                x = x[0]                      # the lowest model level
            elif dims[-1] == "interface_levels" and x.ndim > len(wild):
                x = x[..., 0]                 # the surface
            arrays[k] = np.ascontiguousarray(x.reshape(-1))
        o, d = self._ctx.second_best(arrays, float(timestep.total_seconds()), self.constants())
        self.flags = d["flags"].reshape(wild)      # bit 0 active, bit 1 the unstable branch, bit 2 capped at the freezing temperature
        shaped = lambda k, x: np.reshape(x, t_soil.shape if k in ("t_soil_out", "x_w_out", "x_i_out") else wild)
        return ({name: shaped(k, d[k]) for k, name in DIAGNOSTIC_NAMES.items()}, {name: shaped(k, o[k]) for k, name in OUTPUT_NAMES.items()})
