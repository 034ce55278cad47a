"""RRTMGShortwave -- drop-in for climt.RRTMGShortwave (climt/_components/rrtmg/sw/component.py:32-668)
running on librrtmg_hip.so (MI355X).  Same class attributes, keyword options and defaults, property
dictionaries, log messages and (tendencies, diagnostics) contract; the Cython/Fortran calls are replaced
by one rrtmg_hip_sw_fluxes call (include/rrtmg_hip.h)."""
import logging

import numpy as np

from .._sympl_compat import TendencyComponent, get_constant
from .._util import ensure_contiguous_state
from .common import boundary_dtype as _boundary_dtype, cast_inputs
from .common import (UNIT_FACTOR_ON_DEVICE, InputStaging, library_scales, OutputPool, make_context, output_arrays, rrtmg_aerosol_input_dict, rrtmg_cloud_ice_props_dict, rrtmg_cloud_liquid_props_dict,
                     rrtmg_cloud_overlap_method_dict, rrtmg_cloud_props_dict, rrtmg_random_number_dict, exponential_overlap_option, set_overlap_alpha)


def _prop(dims, units):
    return {"dims": list(dims), "units": units}


_ML, _IL, _COL = ["mid_levels", "*"], ["interface_levels", "*"], ["*"]
_CLD = ["mid_levels", "*", "num_shortwave_bands"]
_AER = ["num_shortwave_bands", "mid_levels", "*"]


# the diagnostics of RRTMGShortwave(flux_components=True) -> member of rrtmg_sw_components (include/rrtmg_hip.h)
FLUX_COMPONENT_DIAGNOSTICS = {
    "downwelling_direct_shortwave_flux_in_air": "dirdflx",
    "downwelling_diffuse_shortwave_flux_in_air": "difdflx",
    "downwelling_direct_shortwave_flux_in_air_assuming_clear_sky": "dirdflxc",
    "downwelling_diffuse_shortwave_flux_in_air_assuming_clear_sky": "difdflxc",
    "downwelling_direct_ultraviolet_and_visible_flux_in_air": "dirdnuv",
    "downwelling_diffuse_ultraviolet_and_visible_flux_in_air": "difdnuv",
    "downwelling_direct_near_infrared_flux_in_air": "dirdnir",
    "downwelling_diffuse_near_infrared_flux_in_air": "difdnir",
}


# the diagnostics of RRTMGShortwave(band_fluxes=True) -> member of rrtmg_sw_band_fluxes: the broadband names with _by_band
# appended, plus the direct beam; dims [num_shortwave_bands, interface_levels, *], bands in the order of the reference's
# per-band inputs (RRTMG bands 16..29: the 820-2600 cm^-1 band is last)
BAND_FLUX_DIAGNOSTICS = {
    "upwelling_shortwave_flux_in_air_by_band": "up",
    "downwelling_shortwave_flux_in_air_by_band": "dn",
    "upwelling_shortwave_flux_in_air_assuming_clear_sky_by_band": "upc",
    "downwelling_shortwave_flux_in_air_assuming_clear_sky_by_band": "dnc",
    "downwelling_direct_shortwave_flux_in_air_by_band": "dndir",
    "downwelling_direct_shortwave_flux_in_air_assuming_clear_sky_by_band": "dndirc",
}
_BIL = ["num_shortwave_bands", "interface_levels", "*"]

# the inputs of RRTMGShortwave(spectral_surface_albedo=True) -> member of rrtmg_sw_surface: one albedo per band (bands in the
# order of the band fluxes) in place of the four broadband ones, which the reference's driver spreads over the bands by a
# fixed rule (SPECTRAL_ALBEDO_BAND_RULE: band -> the broadband input it takes; rrtmg_sw_rad.nomcica.f90:648-659)
SPECTRAL_ALBEDO_INPUTS = {
    "surface_albedo_for_direct_shortwave_by_band": "albdir",
    "surface_albedo_for_diffuse_shortwave_by_band": "albdif",
}
BROADBAND_ALBEDO_INPUTS = ("surface_albedo_for_direct_shortwave", "surface_albedo_for_direct_near_infrared",
                           "surface_albedo_for_diffuse_near_infrared", "surface_albedo_for_diffuse_shortwave")
_VISIBLE_BANDS = (9, 10, 11, 12)   # band index 0..13; the others take the near-IR pair
SPECTRAL_ALBEDO_BAND_RULE = {
    "albdir": tuple("surface_albedo_for_direct_shortwave" if b in _VISIBLE_BANDS else "surface_albedo_for_direct_near_infrared" for b in range(14)),
    "albdif": tuple("surface_albedo_for_diffuse_shortwave" if b in _VISIBLE_BANDS else "surface_albedo_for_diffuse_near_infrared" for b in range(14)),
}


def albedo_by_band_rule(asdir, asdif, aldir, aldif):
    """-> (albdir, albdif), [14][ncol]: the four broadband albedos [ncol] spread over the bands as the reference's driver does."""
    vis = np.zeros(14, dtype=bool)
    vis[list(_VISIBLE_BANDS)] = True
    pick = lambda s, l: np.where(vis[:, None], np.asarray(s, dtype=np.float64)[None, :], np.asarray(l, dtype=np.float64)[None, :])
    return np.ascontiguousarray(pick(asdir, aldir)), np.ascontiguousarray(pick(asdif, aldif))


def band_albedo(wavenumber_cm1, albedo):
    """A spectral albedo curve -> the per-band input of `surface_albedo_for_*_shortwave_by_band` / rrtmg_sw_surface.

    `wavenumber_cm1`: [n], increasing; `albedo`: [n] or [n][ncol].  -> [14] or [14][ncol]: for each band (limits and order of
    rrtmg_hip_band_limits: RRTMG bands 16..29, the 820-2600 cm^-1 band last) the mean over the band's wavenumber interval of
    the piecewise-linear curve through the points, held constant beyond its end points.  This is a FLAT average over
    wavenumber, NOT weighted by the solar spectrum: within a wide band (8050-12850 cm^-1, say) a surface whose albedo varies
    strongly is better represented by an average weighted with the incoming flux, which this helper does not attempt."""
    from .._lib import band_limits
    x = np.asarray(wavenumber_cm1, dtype=np.float64)
    a = np.asarray(albedo, dtype=np.float64)
    if x.ndim != 1 or x.size < 1 or a.shape[:1] != x.shape or a.ndim > 2 or np.any(np.diff(x) <= 0.0):
        raise ValueError("band_albedo: wavenumber_cm1 [n] strictly increasing, albedo [n] or [n][ncol]")
    lo, hi = band_limits("sw")
    a2 = a.reshape(x.size, -1)

    def curve(q):   # the curve at the points q, [len(q)][ncol]
        i = np.clip(np.searchsorted(x, q), 1, max(x.size - 1, 1))
        if x.size == 1:
            return np.repeat(a2[:1], len(q), axis=0)
        t = np.clip((q - x[i - 1]) / (x[i] - x[i - 1]), 0.0, 1.0)[:, None]
        return a2[i - 1] * (1.0 - t) + a2[i] * t
    out = np.empty((lo.size, a2.shape[1]))
    for b in range(lo.size):
        q = np.concatenate(([lo[b]], x[(x > lo[b]) & (x < hi[b])], [hi[b]]))
        v = curve(q)
        out[b] = (0.5 * (v[1:] + v[:-1]) * np.diff(q)[:, None]).sum(axis=0) / (hi[b] - lo[b])
    return out[:, 0] if a.ndim == 1 else out


# the diagnostics an instance made with clear_sky_diagnostics=False does not have -> the library's output behind each
CLEAR_SKY_DIAGNOSTICS = {
    "upwelling_shortwave_flux_in_air_assuming_clear_sky": "swuflxc",
    "downwelling_shortwave_flux_in_air_assuming_clear_sky": "swdflxc",
    "air_temperature_tendency_from_shortwave_assuming_clear_sky": "swhrc",
}


class RRTMGShortwave(TendencyComponent):
    """The Rapid Radiative Transfer Model (RRTMG), shortwave, on AMD MI355X."""

    num_shortwave_bands = 14
    _unit_factor_on_device = UNIT_FACTOR_ON_DEVICE   # (see common.library_scales)
    num_ecmwf_aerosols = 6
    num_reduced_g_intervals = 112
    rrtm_iplon = 1

    input_properties = {
        "air_pressure": _prop(_ML, "mbar"),
        "air_pressure_on_interface_levels": _prop(_IL, "mbar"),
        "air_temperature": _prop(_ML, "degK"),
        "specific_humidity": _prop(_ML, "dimensionless"),
        "mole_fraction_of_ozone_in_air": _prop(_ML, "dimensionless"),
        "mole_fraction_of_carbon_dioxide_in_air": _prop(_ML, "dimensionless"),
        "mole_fraction_of_methane_in_air": _prop(_ML, "dimensionless"),
        "mole_fraction_of_nitrous_oxide_in_air": _prop(_ML, "dimensionless"),
        "mole_fraction_of_oxygen_in_air": _prop(_ML, "dimensionless"),
        "mass_content_of_cloud_ice_in_atmosphere_layer": _prop(_ML, "g m^-2"),
        "mass_content_of_cloud_liquid_water_in_atmosphere_layer": _prop(_ML, "g m^-2"),
        "cloud_ice_particle_size": _prop(_ML, "micrometer"),
        "cloud_water_droplet_radius": _prop(_ML, "micrometer"),
        "cloud_area_fraction_in_atmosphere_layer": _prop(_ML, "dimensionless"),
        "surface_temperature": _prop(_COL, "degK"),
        "zenith_angle": _prop(_COL, "radians"),
        "surface_albedo_for_direct_shortwave": _prop(_COL, "dimensionless"),
        "surface_albedo_for_direct_near_infrared": _prop(_COL, "dimensionless"),
        "surface_albedo_for_diffuse_near_infrared": _prop(_COL, "dimensionless"),
        "surface_albedo_for_diffuse_shortwave": _prop(_COL, "dimensionless"),
        "shortwave_optical_thickness_due_to_cloud": _prop(_CLD, "dimensionless"),
        "shortwave_optical_thickness_due_to_aerosol": _prop(_AER, "dimensionless"),
        "single_scattering_albedo_due_to_cloud": _prop(_CLD, "dimensionless"),
        "single_scattering_albedo_due_to_aerosol": _prop(_AER, "dimensionless"),
        "cloud_asymmetry_parameter": _prop(_CLD, "dimensionless"),
        "aerosol_asymmetry_parameter": _prop(_AER, "dimensionless"),
        "cloud_forward_scattering_fraction": _prop(_CLD, "dimensionless"),
        "aerosol_optical_depth_at_55_micron": _prop(["num_ecmwf_aerosols", "mid_levels", "*"], "dimensionless"),
        "solar_cycle_fraction": _prop([], "dimensionless"),
        "flux_adjustment_for_earth_sun_distance": _prop([], "dimensionless"),
    }

    # no "dims" here, exactly as the reference (sw/component.py:148-150)
    tendency_properties = {"air_temperature": {"units": "degK day^-1"}}

    diagnostic_properties = {
        "upwelling_shortwave_flux_in_air": _prop(_IL, "W m^-2"),
        "downwelling_shortwave_flux_in_air": _prop(_IL, "W m^-2"),
        "upwelling_shortwave_flux_in_air_assuming_clear_sky": _prop(_IL, "W m^-2"),
        "downwelling_shortwave_flux_in_air_assuming_clear_sky": _prop(_IL, "W m^-2"),
        "air_temperature_tendency_from_shortwave_assuming_clear_sky": _prop(_ML, "degK day^-1"),
        "air_temperature_tendency_from_shortwave": _prop(_ML, "degK day^-1"),
    }

    @classmethod
    def diagnostic_properties_for(cls, flux_components=False, band_fluxes=False, clear_sky_diagnostics=True):
        """The diagnostic_properties of an instance made with these options: the class dict itself, or a new dict of it plus
        the eight flux components (interface levels, W m^-2) and / or the six band fluxes (bands x interface levels), or
        without the three CLEAR_SKY_DIAGNOSTICS."""
        if not flux_components and not band_fluxes and clear_sky_diagnostics:
            return cls.diagnostic_properties
        props = {k: v for k, v in cls.diagnostic_properties.items() if clear_sky_diagnostics or k not in CLEAR_SKY_DIAGNOSTICS}
        if flux_components:
            props.update({k: _prop(_IL, "W m^-2") for k in FLUX_COMPONENT_DIAGNOSTICS})
        if band_fluxes:
            props.update({k: _prop(_BIL, "W m^-2") for k in BAND_FLUX_DIAGNOSTICS})
        return props

    @classmethod
    def input_properties_for(cls, spectral_surface_albedo=False):
        """The input_properties of an instance made with this option: the class dict itself, or a new dict of it with the two
        albedos by band (bands x columns, dimensionless) in place of the four broadband ones."""
        if not spectral_surface_albedo:
            return cls.input_properties
        props = {k: v for k, v in cls.input_properties.items() if k not in BROADBAND_ALBEDO_INPUTS}
        props.update({k: _prop(["num_shortwave_bands", "*"], "dimensionless") for k in SPECTRAL_ALBEDO_INPUTS})
        return props

    def __init__(self, cloud_overlap_method=None, cloud_optical_properties="liquid_and_ice_clouds",
                 cloud_ice_properties="ebert_curry_two", cloud_liquid_water_properties="radius_dependent_absorption",
                 solar_variability_method=0, use_solar_constant_from_fortran=False, ignore_day_of_year=False,
                 facular_sunspot_amplitude=None, solar_variability_by_band=None, aerosol_type="no_aerosol", mcica=False,
                 random_number_generator="mersenne_twister", device=0, flux_components=False, band_fluxes=False,
                 spectral_surface_albedo=False, skip_night_columns=False, pack_day_columns=False, clear_sky_diagnostics=True,
                 boundary_dtype="float64", cloud_overlap_decorrelation_length=2000.0, **kwargs):
        """Same keyword arguments and defaults as climt.RRTMGShortwave (sw/component.py:179-194); the additions are `device`
        (GPU ordinal) and `flux_components`: True adds the downward flux split into direct and diffuse parts -- all bands,
        UV/visible bands, near-IR bands, and all bands clear sky (FLUX_COMPONENT_DIAGNOSTICS) -- to this instance's
        diagnostics; `band_fluxes`: True adds the up / down fluxes (all sky, clear sky) and the direct beam by spectral
        band (BAND_FLUX_DIAGNOSTICS); `spectral_surface_albedo`: True replaces, in this instance's inputs, the four broadband
        surface albedos by one direct and one diffuse albedo per band (SPECTRAL_ALBEDO_INPUTS; band_albedo() makes them from
        a spectral curve); `skip_night_columns`: True gives every column whose zenith angle is >= pi/2 (a column at exactly pi/2, where
        Instellation clamps the angle and the cosine in double precision is +6e-17, is night) exact zeros in every
        output instead of the reference's fluxes of order 1e-7 W m^-2 (its driver clamps the cosine to 1e-10 and solves), and
        does no work for 64-column tiles that are night throughout (rrtmg_hip_set_sw_night_skip; climt_amd.night.night_tiles
        states which those are); the cosine it hands over is night_coszen(): 0 from a zenith angle of pi/2 on; day columns
        keep their bits; `pack_day_columns`: True (requires skip_night_columns=True, else ValueError) also packs the day
        columns into dense tiles inside the library, so that EVERY night column's solve is saved on any grid, 128 longitudes
        included, where the skip alone finds no night tile (rrtmg_hip_set_sw_night_pack; climt_amd.night.packed_order and
        packed_counts state the layout and what sw_night_last() reports).  Only the device-resident path packs -- a
        climt_amd.DeviceState with kissvec or no McICA and facular_sunspot_amplitude of 1; a host state, radiation_step's
        joint call and every other call run as with skip_night_columns alone.  The night columns' zeros are the same; a day
        column's bits are those of a call on the day columns alone (see the header for when they differ from the whole
        grid's, by at most 1e-10); the class attributes are unchanged; `clear_sky_diagnostics`: False takes the three
        `*_assuming_clear_sky` quantities (CLEAR_SKY_DIAGNOSTICS) out of this instance's diagnostics and has the library form no
        clear-sky stream (rrtmg_hip_set_sw_clear_sky): columns with cloud are solved once, not twice, and three of the six
        outputs are not copied; the other diagnostics and the tendency agree with the default instance's to rounding (<= 5e-8
        W m^-2).  Not together with flux_components or band_fluxes (ValueError): their clear-sky and direct-beam members
        read the stream that is not formed; `boundary_dtype`: "float32" hands the state arrays to the library as 4-byte reals
        (rrtmg_hip_sw_fluxes_f32: an array that already is float32 goes over as it is, the quantities formed here -- the cosine
        of the zenith angle -- are computed as always and then cast) and returns float32 diagnostics and tendencies: the
        fp64 results of those inputs, rounded once.  Half the bytes cross PCIe.  Host states only: a DeviceState stays float64."""
        self._boundary_dtype = _boundary_dtype(boundary_dtype)
        if pack_day_columns and not skip_night_columns:
            raise ValueError("pack_day_columns=True requires skip_night_columns=True")
        if not clear_sky_diagnostics and (flux_components or band_fluxes):
            raise ValueError("clear_sky_diagnostics=False cannot be combined with %s=True" % ("flux_components" if flux_components else "band_fluxes"))
        self._clear_sky = bool(clear_sky_diagnostics)
        if not self._clear_sky:
            self.diagnostic_properties = self.diagnostic_properties_for(clear_sky_diagnostics=False)
        self._skip_night = bool(skip_night_columns)
        self._pack_day = bool(pack_day_columns)
        self._spectral_albedo = bool(spectral_surface_albedo)
        if self._spectral_albedo:
            self.input_properties = self.input_properties_for(True)
        self._flux_components = bool(flux_components)
        self._band_fluxes = bool(band_fluxes)
        if self._flux_components:
            self.diagnostic_properties = self.diagnostic_properties_for(True)
        if self._band_fluxes:
            self.diagnostic_properties = self.diagnostic_properties_for(self._flux_components, band_fluxes=True)
        self._mcica = mcica
        if mcica:
            self._permute_seed = None
            self._random_number_generator = rrtmg_random_number_dict[random_number_generator.lower()]
            # messages asserted by the reference's tests (tests/test_components.py:507-530)
            if type(cloud_overlap_method) is str:
                if cloud_overlap_method.lower() == "clear_only":
                    logging.info("cloud_overlap_method == 'clear_only'."
                                 " This overrides all other properties. "
                                 "There are no clouds.")
            if cloud_optical_properties.lower() == "single_cloud_type":
                logging.warning("cloud_optical_properties must be 'direct_input' or "
                                "'liquid_and_ice_clouds' for radiative calculations with "
                                "clouds using McICA.")
            if cloud_optical_properties.lower() == "liquid_and_ice_clouds":
                if cloud_ice_properties.lower() == "ebert_curry_one":
                    logging.warning("cloud_ice_properties should not be set to "
                                    "'ebert_curry_one' for shortwave calculations with "
                                    "McICA.")
                if cloud_liquid_water_properties.lower() == "radius_independent_absorption":
                    logging.warning("cloud_liquid_water_properties must be set to "
                                    "'radius_dependent_absorption' for use with McICA in "
                                    "the shortwave.")
        if cloud_overlap_method is None:
            cloud_overlap_method = "random"
        # "exponential" / "exponential_random" (McICA only; not in the reference's dict): icld 4 / 5 and the decorrelation length
        self._exp_overlap = exponential_overlap_option(cloud_overlap_method, mcica, cloud_overlap_decorrelation_length)
        self._cloud_overlap = self._exp_overlap[0] if self._exp_overlap else rrtmg_cloud_overlap_method_dict[cloud_overlap_method.lower()]
        self._cloud_optics = rrtmg_cloud_props_dict[cloud_optical_properties.lower()]
        self._ice_props = rrtmg_cloud_ice_props_dict[cloud_ice_properties.lower()]
        self._liq_props = rrtmg_cloud_liquid_props_dict[cloud_liquid_water_properties.lower()]
        self._solar_var_flag = solar_variability_method
        self._ignore_day_of_year = ignore_day_of_year
        self._fac_sunspot_coeff = np.ones(2) if facular_sunspot_amplitude is None else np.asarray(facular_sunspot_amplitude, dtype=float)
        self._solar_var_by_band = np.ones(16) if solar_variability_by_band is None else np.asarray(solar_variability_by_band, dtype=float)
        self._aerosol_type = rrtmg_aerosol_input_dict[aerosol_type.lower()]
        self._solar_const = 0 if use_solar_constant_from_fortran else get_constant("stellar_irradiance", "W/m^2")
        self._Cpd = get_constant("heat_capacity_of_dry_air_at_constant_pressure", "J/kg/K")
        self._ctx = make_context(device)
        self._pool = OutputPool(dtype=self._boundary_dtype)
        self._input_staging = InputStaging()
        # the reference re-runs rrtmg_sw_ini on every McICA call (sw/component.py:547-560); the tables do
        # not depend on the call, so they are built once here
        self._ctx.sw_init(self._Cpd)
        super(RRTMGShortwave, self).__init__(**kwargs)

    @staticmethod
    def night_coszen(zenith_angle):
        """cos(zenith) as an instance with skip_night_columns=True hands it to the library, whose night test is coszen <= 0:
        0.0 where the zenith angle is >= pi/2, cos() elsewhere.  Instellation (like climt's) clamps the zenith angle to pi/2, and
        the cosine of the double nearest pi/2 is +6e-17: without this the sun would never set."""
        z = np.asarray(zenith_angle, dtype=np.float64)
        return np.where(z >= 0.5 * np.pi, 0.0, np.cos(z))

    def _apply_night_skip(self, ctx):
        """This instance's `skip_night_columns` -> the context about to be called (contexts are shared between components, so
        the switch is set before every call).  A context without the switch serves the default only."""
        setter = getattr(ctx, "set_sw_night_skip", None)
        if setter is not None:
            setter(self._skip_night)
        elif self._skip_night:
            raise RuntimeError("skip_night_columns=True: this context has no set_sw_night_skip")
        pack, setter = getattr(self, "_pack_day", False), getattr(ctx, "set_sw_night_pack", None)
        if setter is not None and (pack or getattr(ctx, "has_sw_night_pack", True)):
            setter(pack)
        elif pack:
            raise RuntimeError("pack_day_columns=True: this context has no set_sw_night_pack")
        # `clear_sky_diagnostics`, likewise
        clear, setter = getattr(self, "_clear_sky", True), getattr(ctx, "set_sw_clear_sky", None)
        if setter is not None and (not clear or getattr(ctx, "has_sw_clear_sky", True)):
            setter(clear)
        elif not clear:
            raise RuntimeError("clear_sky_diagnostics=False: this context has no set_sw_clear_sky")

    def _apply_overlap(self, ctx, call, which="sw"):
        """cloud_overlap_method "exponential" / "exponential_random": the rank correlations of this state, computed by the library
        from the call's mid-layer pressure and temperature and set on the context for this spectrum (which="both": for the
        longwave of a joint call too).  Any other method: nothing."""
        if getattr(self, "_exp_overlap", None):
            play, tlay = call["overlap_state"]
            set_overlap_alpha(ctx, which, self._exp_overlap[1], play, tlay)

    def __call__(self, state, *args, **kwargs):
        """A host state goes through sympl's machinery to array_call; a climt_amd.DeviceState (state resident in HBM) takes
        the device path: same quantities, DeviceQuantity handles instead of arrays (climt_amd/device_state.py)."""
        from ..device_state import DeviceState, shortwave_device_call
        if isinstance(state, DeviceState):
            return shortwave_device_call(self, state, **kwargs)      # (output_work: the caller's own output buffers)
        return super(RRTMGShortwave, self).__call__(state, *args, **kwargs)

    @ensure_contiguous_state
    def array_call(self, state):
        """Shortwave heating tendency and up/down fluxes (all-sky and clear-sky)."""
        call = self._prepare_call(state)
        self._apply_night_skip(self._ctx)
        self._apply_overlap(self._ctx, call)
        self._ctx.sw_fluxes(**call["library"])
        return self._finish_call(call)

    def _prepare_call(self, state):
        """array_call, part 1 of 3: the raw state -> {"library": the keyword arguments of Context.sw_fluxes, "tendencies",
        "diagnostics"}.  Part 2 is the library call (after _apply_night_skip), part 3 _finish_call; climt_amd.radiation_step
        runs the parts of this component and of a longwave around ONE Context.radiation_fluxes."""
        # mass_to_volume_mixing_ratio(q, 18.02) = q * 28.964 / 18.02 and the unit factors of the pressures and cloud water paths
        # are applied by the library on the device, after the upload (common.library_scales): no host pass over those arrays
        scales, unit = library_scales(state)
        Q = state["specific_humidity"]
        assert unit["air_pressure"].shape[0] + 1 == unit["air_pressure_on_interface_levels"].shape[0]
        # (the reference also interpolates interface temperatures here, sw/component.py:492-496; RRTMG_SW never reads them)
        Tint = None
        # (recycled when the caller has dropped an earlier call's results: the library overwrites every element)
        diagnostics = output_arrays(self._pool, self.diagnostic_properties, state, self.input_properties)
        tendencies = output_arrays(self._pool, self.tendency_properties, state, self.input_properties)
        day_of_year = 0 if self._ignore_day_of_year else state["time"].timetuple().tm_yday
        inp = dict(
            play=unit["air_pressure"], plev=unit["air_pressure_on_interface_levels"], tlay=state["air_temperature"], tlev=Tint,
            tsfc=state["surface_temperature"], h2o=Q, o3=state["mole_fraction_of_ozone_in_air"],
            co2=state["mole_fraction_of_carbon_dioxide_in_air"], ch4=state["mole_fraction_of_methane_in_air"],
            n2o=state["mole_fraction_of_nitrous_oxide_in_air"], o2=state["mole_fraction_of_oxygen_in_air"],
            coszen=self.night_coszen(state["zenith_angle"]) if self._skip_night else np.cos(state["zenith_angle"]), cldfr=state["cloud_area_fraction_in_atmosphere_layer"],
            taucld=state["shortwave_optical_thickness_due_to_cloud"], ssacld=state["single_scattering_albedo_due_to_cloud"],
            asmcld=state["cloud_asymmetry_parameter"], fsfcld=state["cloud_forward_scattering_fraction"],
            cicewp=unit["mass_content_of_cloud_ice_in_atmosphere_layer"],
            cliqwp=unit["mass_content_of_cloud_liquid_water_in_atmosphere_layer"],
            reice=state["cloud_ice_particle_size"], reliq=state["cloud_water_droplet_radius"],
            tauaer=state["shortwave_optical_thickness_due_to_aerosol"], ssaaer=state["single_scattering_albedo_due_to_aerosol"],
            asmaer=state["aerosol_asymmetry_parameter"], ecaer=state["aerosol_optical_depth_at_55_micron"],
            bndsolvar=self._solar_var_by_band, indsolvar=self._fac_sunspot_coeff,
            icld=self._cloud_overlap, iaer=self._aerosol_type, inflg=self._cloud_optics, iceflg=self._ice_props,
            liqflg=self._liq_props, dyofyr=day_of_year, isolvar=self._solar_var_flag, scon=float(self._solar_const),
            adjes=state["flux_adjustment_for_earth_sun_distance"].item(), solcycfrac=state["solar_cycle_fraction"].item(), **scales
        )
        if self._spectral_albedo:
            surface = {m: state[k] for k, m in SPECTRAL_ALBEDO_INPUTS.items()}
        else:
            surface = None
            inp.update(asdir=state["surface_albedo_for_direct_shortwave"], asdif=state["surface_albedo_for_diffuse_shortwave"],
                       aldir=state["surface_albedo_for_direct_near_infrared"], aldif=state["surface_albedo_for_diffuse_near_infrared"])
        if self._mcica:
            # a fresh seed on every call, drawn exactly as the reference does (sw/component.py:537-545)
            if self._random_number_generator == 0:
                self._permute_seed = np.random.randint(0, 1024)
            elif self._random_number_generator == 1:
                self._permute_seed = np.random.randint(0, 2 ** 31 - 1)
            inp.update(irng=self._random_number_generator, permuteseed=self._permute_seed)
        out = dict(
            swuflx=diagnostics["upwelling_shortwave_flux_in_air"], swdflx=diagnostics["downwelling_shortwave_flux_in_air"],
            swhr=tendencies["air_temperature"])
        if getattr(self, "_clear_sky", True):
            out.update({m: diagnostics[k] for k, m in CLEAR_SKY_DIAGNOSTICS.items()})
        self._input_staging.wait()
        library = dict(inp=inp, mcica=self._mcica, out=out)
        overlap_state = (inp["play"], inp["tlay"])      # (what _apply_overlap reads: the float64 arrays, before any cast)
        if getattr(self, "_boundary_dtype", np.float64) == np.float32:      # (the default passes no keyword: any context serves it)
            cast_inputs(inp, np.float32)
            if surface is not None:
                cast_inputs(surface, np.float32)
            library.update(precision="float32")
        if self._flux_components or self._band_fluxes:
            comps = {c: diagnostics[k] for k, c in FLUX_COMPONENT_DIAGNOSTICS.items()} if self._flux_components else None
            bands = {b: diagnostics[k] for k, b in BAND_FLUX_DIAGNOSTICS.items()} if self._band_fluxes else None
            library.update(components=comps, bands=bands, surface=surface)
        elif surface is not None:
            library.update(surface=surface)
        return dict(library=library, tendencies=tendencies, diagnostics=diagnostics, overlap_state=overlap_state)

    @staticmethod
    def _finish_call(call):
        """array_call, part 3 of 3: what follows the library call."""
        tendencies, diagnostics = call["tendencies"], call["diagnostics"]
        diagnostics["air_temperature_tendency_from_shortwave"][:] = tendencies["air_temperature"]
        return tendencies, diagnostics
