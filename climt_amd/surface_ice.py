"""SeaIce and LandIce -- drop-ins for climt.SeaIce and climt.LandIce (climt/_components/sea_ice/component.py,
land_ice/component.py): one Crank-Nicolson heat-diffusion step of the snow/ice column over sea-ice cells, or over land and
land-ice cells, with surface melt, basal growth (sea ice) or the ground flux (land ice), the surface temperature the next
longwave call needs, the albedo the shortwave needs and the flux the slab needs.  Same constructors, property dictionaries
and outputs; both are thin shells around ONE per-column rule, which runs on the GPU through rrtmg_hip_surface_ice
(include/rrtmg_hip.h), one thread per column, in the reference's order of operations."""
import logging

import numpy as np

from ._sympl_compat import Stepper, get_constant
from .rrtmg.common import make_context
from .slab_surface import AREA_MAP

logger = logging.getLogger(__name__)

_FLUX = {"dims": ["*", "interface_levels"], "units": "W m^-2"}
_ICE = lambda units: {"dims": ["ice_interface_levels", "*"], "units": units}
_COL = lambda units: {"dims": ["*"], "units": units}
# the six parts of the net flux, by the library's names (climt_amd/_lib.py: SURFACE_ICE_FLUXES)
FLUX_NAMES = dict(sw_down="downwelling_shortwave_flux_in_air", lw_down="downwelling_longwave_flux_in_air", sw_up="upwelling_shortwave_flux_in_air",
                  lw_up="upwelling_longwave_flux_in_air", lh="surface_upward_latent_heat_flux", sh="surface_upward_sensible_heat_flux")
FLAG_ACTIVE, FLAG_NEGATIVE_ENERGY, FLAG_TOO_TALL = 1, 2, 4


def area_codes(area_type):
    """The int32 codes of slab_surface.AREA_MAP for an array of area-type strings; a string the map does not know is -1 (no
    component steps it, as in the reference)."""
    s = np.asarray(area_type).astype(str)
    codes = np.full(s.shape, -1, dtype=np.int32)
    for k, v in AREA_MAP.items():
        codes[s == k] = v
    return codes


def too_tall_message(maximum):
    return "Total height exceeds maximum value of {} m.".format(maximum)


class _SnowIceColumn(Stepper):
    """What SeaIce and LandIce share: the constants, the call and the shape of what comes back."""

    kind = None                # 0: sea ice, 1: land ice
    thickness_name = None      # sea_ice_thickness / land_ice_thickness
    base_name = None           # the input behind `base`
    base_flux_name = None      # the diagnostic behind `base_flux_out`

    def __init__(self, maximum_snow_ice_height, albedo_snow, albedo_ice, albedo_melt, device, context, **kwargs):
        self._max_height = maximum_snow_ice_height
        self._albedo_snow = albedo_snow
        self._albedo_ice = albedo_ice
        self._albedo_melt = albedo_melt
        self._epsilon = 1e-5
        super(_SnowIceColumn, self).__init__(**kwargs)
        self._ctx = context if context is not None else make_context(device)

    def constants(self):
        """The eight constants of the reference's _update_constants under the unit strings it asks with (asked for at every
        call), and the component's own scalars, as the library takes them."""
        return dict(k_ice=float(get_constant("thermal_conductivity_of_solid_phase_as_ice", "W/m/degK")),
                    k_snow=float(get_constant("thermal_conductivity_of_solid_phase_as_snow", "W/m/degK")),
                    rho_ice=float(get_constant("density_of_solid_phase_as_ice", "kg/m^3")), c_ice=float(get_constant("heat_capacity_of_solid_phase_as_ice", "J/kg/degK")),
                    rho_snow=float(get_constant("density_of_solid_phase_as_snow", "kg/m^3")), c_snow=float(get_constant("heat_capacity_of_solid_phase_as_snow", "J/kg/degK")),
                    lf=float(get_constant("latent_heat_of_fusion", "J/kg")), t_melt=float(get_constant("freezing_temperature_of_liquid_phase", "degK")),
                    eps=self._epsilon, max_height=float(self._max_height), albedo_snow=float(self._albedo_snow), albedo_ice=float(self._albedo_ice),
                    albedo_melt=float(self._albedo_melt))

    def too_tall(self, codes, thick, snow):
        """The reference's height condition: the columns it raises for."""
        mine = (codes == AREA_MAP["sea_ice"]) & (thick > 0.0) if self.kind == 0 else (codes == AREA_MAP["land_ice"]) | (codes == AREA_MAP["land"])
        return mine & (thick + snow > self._max_height)

    def log_negative_energy(self, flags, net=None, cond=None):
        for col in np.nonzero(np.asarray(flags).reshape(-1) & FLAG_NEGATIVE_ENERGY)[0]:
            logger.debug("Negative melt energy at column %d (net_flux=%s, conducted_flux=%s); clamped to 0.", int(col),
                         None if net is None else net[col], None if cond is None else cond[col])

    def __call__(self, state, timestep=None, *args, **kwargs):
        """A host state goes through sympl's machinery to array_call; a climt_amd.DeviceState (state resident in HBM) takes
        the device path and comes back rebound to the new column (climt_amd/device_state.py).  `check_maximum_height` (device
        path only, default True): download the flags and raise the reference's ValueError for a column taller than the maximum."""
        from .device_state import DeviceState, surface_ice_device_call
        if isinstance(state, DeviceState):
            return surface_ice_device_call(self, state, timestep, check_maximum_height=kwargs.pop("check_maximum_height", True))
        return super(_SnowIceColumn, self).__call__(state, timestep, *args, **kwargs)

    def array_call(self, raw_state, timestep):
        """-> (diagnostics, outputs), as the reference returns them."""
        dt = float(timestep.total_seconds())
        t = np.asarray(raw_state["snow_and_ice_temperature"], dtype=np.float64)
        wild = t.shape[1:]
        nodes = lambda x: np.reshape(np.asarray(x, dtype=np.float64), (np.shape(x)[0], -1))
        flat = lambda x: np.reshape(np.asarray(x, dtype=np.float64), (-1,))

        def surface(x):          # dims ["*", "interface_levels"]: level 0 is the surface
            x = np.asarray(x, dtype=np.float64)
            return np.ascontiguousarray(flat(x[..., 0] if x.ndim > len(wild) else x))

        codes = area_codes(raw_state["area_type"]).reshape(-1)
        thick, snow = flat(raw_state[self.thickness_name]), flat(raw_state["surface_snow_thickness"])
        if np.any(self.too_tall(codes, thick, snow)):
            raise ValueError(too_tall_message(self._max_height))
        fluxes = {k: (surface if "flux_in_air" in name else flat)(raw_state[name]) for k, name in FLUX_NAMES.items()}
        o, d = self._ctx.surface_ice(self.kind, nodes(t), nodes(raw_state["height_on_ice_interface_levels"]), thick, snow, flat(raw_state[self.base_name]),
                                     fluxes, codes, dt, self.constants())
        if np.any(d["flags"] & FLAG_NEGATIVE_ENERGY):
            net = fluxes["sw_down"] + fluxes["lw_down"] - fluxes["sw_up"] - fluxes["lw_up"] - fluxes["sh"] - fluxes["lh"]
            self.log_negative_energy(d["flags"], net, d["cond_flux"] if self.kind == 0 else o["base_flux_out"])
        col = lambda x: np.reshape(x, wild)
        diagnostics = {self.base_flux_name: col(o["base_flux_out"]), "surface_albedo_for_direct_shortwave": col(d["albedo"]),
                       "surface_albedo_for_diffuse_shortwave": col(d["albedo"]).copy()}
        if self.kind == 0:
            diagnostics["surface_downward_heat_flux_in_sea_ice"] = col(d["cond_flux"])
        outputs = {self.thickness_name: col(o["thick_out"]), "surface_snow_thickness": col(o["snow_out"]), "surface_temperature": col(o["tsfc_out"]),
                   "snow_and_ice_temperature": np.reshape(o["t_out"], t.shape), "height_on_ice_interface_levels": np.reshape(o["height_out"], t.shape)}
        return diagnostics, outputs


class SeaIce(_SnowIceColumn):
    """
    1-D thermodynamic sea-ice model over ``area_type == "sea_ice"`` cells.

    The basal boundary is the prescribed ocean heat flux ``heat_flux_into_sea_water_due_to_sea_ice``; the thickness is clamped
    at zero and what would have driven it below goes into that flux.  Behaviours of the reference that are kept as they are
    (INTEGRATION.md): the layer spacing is total / nodes, and on a thin 3-node column the surface temperature may rise above
    melting.
    """

    kind, thickness_name = 0, "sea_ice_thickness"
    base_name = base_flux_name = "heat_flux_into_sea_water_due_to_sea_ice"

    input_properties = {
        "downwelling_longwave_flux_in_air": _FLUX,
        "downwelling_shortwave_flux_in_air": _FLUX,
        "upwelling_longwave_flux_in_air": _FLUX,
        "upwelling_shortwave_flux_in_air": _FLUX,
        "surface_upward_latent_heat_flux": _COL("W m^-2"),
        "surface_upward_sensible_heat_flux": _COL("W m^-2"),
        "sea_ice_thickness": _COL("m"),
        "surface_snow_thickness": _COL("m"),
        "area_type": _COL("dimensionless"),
        "snow_and_ice_temperature": _ICE("degK"),
        "sea_surface_temperature": _COL("degK"),
        "heat_flux_into_sea_water_due_to_sea_ice": _COL("W m^-2"),
        "height_on_ice_interface_levels": _ICE("m"),
    }

    output_properties = {
        "sea_ice_thickness": _COL("m"),
        "surface_snow_thickness": _COL("m"),
        "surface_temperature": _COL("degK"),
        "snow_and_ice_temperature": _ICE("degK"),
        "height_on_ice_interface_levels": _ICE("m"),
    }

    diagnostic_properties = {
        "heat_flux_into_sea_water_due_to_sea_ice": _COL("W m^-2"),
        "surface_downward_heat_flux_in_sea_ice": _COL("W m^-2"),
        "surface_albedo_for_direct_shortwave": _COL("dimensionless"),
        "surface_albedo_for_diffuse_shortwave": _COL("dimensionless"),
    }

    def __init__(self, maximum_snow_ice_height=10, albedo_snow=0.8, albedo_ice=0.5, albedo_melt=0.2, device=0, context=None, **kwargs):
        """Args: the reference's -- the maximum combined height of snow and ice in m and the three albedos (snow on top, bare
        ice, melting surface) -- plus `device` and `context` like the other components of this package."""
        super(SeaIce, self).__init__(maximum_snow_ice_height, albedo_snow, albedo_ice, albedo_melt, device, context, **kwargs)


class LandIce(_SnowIceColumn):
    """
    1-D thermodynamic snow/ice model over ``area_type in ("land_ice", "land")`` cells (snow on land included).

    The base of the column is held at ``soil_surface_temperature``; the exchange with the soil is reported as
    ``upward_heat_flux_at_ground_level_in_soil``.  Thickness and snow are clamped at zero.
    """

    kind, thickness_name = 1, "land_ice_thickness"
    base_name, base_flux_name = "soil_surface_temperature", "upward_heat_flux_at_ground_level_in_soil"

    input_properties = {
        "downwelling_longwave_flux_in_air": _FLUX,
        "downwelling_shortwave_flux_in_air": _FLUX,
        "upwelling_longwave_flux_in_air": _FLUX,
        "upwelling_shortwave_flux_in_air": _FLUX,
        "surface_upward_latent_heat_flux": _COL("W m^-2"),
        "surface_upward_sensible_heat_flux": _COL("W m^-2"),
        "land_ice_thickness": _COL("m"),
        "surface_snow_thickness": _COL("m"),
        "area_type": _COL("dimensionless"),
        "snow_and_ice_temperature": _ICE("degK"),
        "soil_surface_temperature": _COL("degK"),
        "height_on_ice_interface_levels": _ICE("m"),
    }

    output_properties = {
        "land_ice_thickness": _COL("m"),
        "surface_snow_thickness": _COL("m"),
        "surface_temperature": _COL("degK"),
        "snow_and_ice_temperature": _ICE("degK"),
        "height_on_ice_interface_levels": _ICE("m"),
    }

    diagnostic_properties = {
        "upward_heat_flux_at_ground_level_in_soil": _COL("W m^-2"),
        "surface_albedo_for_direct_shortwave": _COL("dimensionless"),
        "surface_albedo_for_diffuse_shortwave": _COL("dimensionless"),
    }

    def __init__(self, maximum_snow_ice_height=10, albedo_snow=0.8, albedo_ice=0.6, albedo_melt=0.2, device=0, context=None, **kwargs):
        """Args: the reference's -- the maximum combined height of snow and ice in m and the three albedos (snow on top, bare
        land ice, melting surface) -- plus `device` and `context` like the other components of this package."""
        super(LandIce, self).__init__(maximum_snow_ice_height, albedo_snow, albedo_ice, albedo_melt, device, context, **kwargs)
