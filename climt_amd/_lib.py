"""ctypes binding of librrtmg_hip.so (include/rrtmg_hip.h) -- replaces climt's Cython shims
_rrtmg_sw.pyx / _rrtmg_lw.pyx (climt/_components/rrtmg/{sw,lw}/).

There is no CPU fallback: importing works anywhere (so property dictionaries can be inspected),
but creating a Context without the built library or without a GPU raises.
"""
import ctypes as C
import functools
import os
import threading

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("RRTMG_HIP_LIB") or os.path.join(HERE, "_lib", "librrtmg_hip.so")
SW_DATA = os.path.join(HERE, "data", "rrtmg_sw_data.bin")
LW_DATA = os.path.join(HERE, "data", "rrtmg_lw_data.bin")

_vp, _i32, _f64 = C.c_void_p, C.c_int32, C.c_double


class RRTMGError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("rrtmg_hip error %d: %s" % (code, msg))
        self.code = code


# unit factors the library applies to host arrays on the device (include/rrtmg_hip.h: rrtmg_sw_args, last four fields)
_SCALES = ("pressure_scale", "water_path_scale", "h2o_mul", "h2o_div")


class SwArgs(C.Structure):
    _fields_ = ([(n, _i32) for n in ("ncol nlay memspace mcica icld iaer inflgsw iceflgsw liqflgsw dyofyr isolvar "
                                     "irng permuteseed shard_col0 shard_ncol struct_size").split()]
                + [(n, _f64) for n in "adjes scon solcycfrac".split()]
                + [(n, _vp) for n in ("bndsolvar indsolvar play plev tlay tlev tsfc h2ovmr o3vmr co2vmr ch4vmr n2ovmr o2vmr "
                                      "asdir asdif aldir aldif coszen cldfr taucld ssacld asmcld fsfcld cicewp cliqwp reice "
                                      "reliq tauaer ssaaer asmaer ecaer cldfmcl swuflx swdflx swhr swuflxc swdflxc swhrc").split()]
                + [(n, _f64) for n in _SCALES])


# members of rrtmg_sw_components (include/rrtmg_hip.h), in order: downward direct / diffuse flux, all bands, UV/visible
# bands, near-IR bands (all sky), and all bands clear sky
SW_COMPONENTS = ("dirdflx", "difdflx", "dirdnuv", "difdnuv", "dirdnir", "difdnir", "dirdflxc", "difdflxc")


class SwComponents(C.Structure):
    """mirrors `rrtmg_sw_components` (include/rrtmg_hip.h), field for field"""
    _fields_ = [("struct_size", _i32), ("reserved", _i32)] + [(n, _vp) for n in SW_COMPONENTS]


# members of rrtmg_sw_band_fluxes / rrtmg_lw_band_fluxes (include/rrtmg_hip.h), in order, and their number of bands
SW_BAND_FLUXES = ("up", "dn", "upc", "dnc", "dndir", "dndirc")
LW_BAND_FLUXES = ("up", "dn", "upc", "dnc")
SW_NBAND, LW_NBAND = 14, 16
BAND_LEVELS = {"all": 0, "boundaries": 1}   # rows of a band array: every interface level, or surface and top


class SwBandFluxes(C.Structure):
    """mirrors `rrtmg_sw_band_fluxes` (include/rrtmg_hip.h), field for field"""
    _fields_ = [("struct_size", _i32), ("levels", _i32)] + [(n, _vp) for n in SW_BAND_FLUXES]


# members of rrtmg_sw_surface (include/rrtmg_hip.h): the surface albedo by band for the direct beam / for diffuse radiation
SW_SURFACE = ("albdir", "albdif")


class SwSurface(C.Structure):
    """mirrors `rrtmg_sw_surface` (include/rrtmg_hip.h), field for field"""
    _fields_ = [("struct_size", _i32), ("reserved", _i32)] + [(n, _vp) for n in SW_SURFACE]


PRECISIONS = {"float64": np.dtype(np.float64), "float32": np.dtype(np.float32)}   # the `precision` of a flux call -> element type of its grid arrays


def _precision(precision):
    if precision not in PRECISIONS:
        raise ValueError("precision %r: one of %s" % (precision, ", ".join(repr(k) for k in PRECISIONS)))
    return PRECISIONS[precision]


def _device_pointer(v, dtype, what):
    """`v` as the integer a struct member takes: a raw device pointer, or a climt_amd._hip.DeviceArray, whose dtype must be the call's."""
    if hasattr(v, "ptr") and hasattr(v, "dtype"):
        if np.dtype(v.dtype) != dtype:
            raise ValueError("%s: a DeviceArray of dtype %s in a %s call" % (what, np.dtype(v.dtype).name, dtype.name))
        return int(v.ptr)
    return int(v)


def _is_pointer(v):
    return isinstance(v, (int, np.integer)) or (hasattr(v, "ptr") and hasattr(v, "dtype") and not isinstance(v, np.ndarray))


def _surface_struct(surface, ncol, keep, dtype=PRECISIONS["float64"]):
    """The filled struct of a `surface=` input (Context.sw_fluxes): arrays [14][ncol] (kept alive in `keep`) or device pointers."""
    s = SwSurface()
    s.struct_size = C.sizeof(SwSurface)
    for k, v in surface.items():
        if k not in SW_SURFACE:
            raise KeyError("unknown surface input %r (one of %s)" % (k, ", ".join(SW_SURFACE)))
        if v is None:
            continue
        if _is_pointer(v):
            setattr(s, k, _device_pointer(v, dtype, "surface input %r" % k))
            continue
        arr = np.ascontiguousarray(v, dtype=dtype)
        if arr.shape != (SW_NBAND, ncol):
            raise ValueError("surface input %r: an array of %d x %d (band, column), not %r" % (k, SW_NBAND, ncol, arr.shape))
        keep.append(arr)
        setattr(s, k, arr.ctypes.data)
    return s


class LwBandFluxes(C.Structure):
    """mirrors `rrtmg_lw_band_fluxes` (include/rrtmg_hip.h), field for field"""
    _fields_ = [("struct_size", _i32), ("levels", _i32)] + [(n, _vp) for n in LW_BAND_FLUXES]


def _band_struct(cls, names, nband, bands, band_levels, nlay, ncol, dtype=PRECISIONS["float64"]):
    """The filled struct of a `bands=` request (Context.sw_fluxes / lw_fluxes)."""
    if band_levels not in BAND_LEVELS:
        raise ValueError("band_levels %r: one of %s" % (band_levels, ", ".join(repr(k) for k in BAND_LEVELS)))
    b = cls()
    b.struct_size, b.levels = C.sizeof(cls), BAND_LEVELS[band_levels]
    nrow = 2 if b.levels else nlay + 1
    for k, v in bands.items():
        if k not in names:
            raise KeyError("unknown band flux %r (one of %s)" % (k, ", ".join(names)))
        if _is_pointer(v):
            setattr(b, k, _device_pointer(v, dtype, "band flux %r" % k))
            continue
        if not (isinstance(v, np.ndarray) and v.dtype == dtype and v.flags.c_contiguous and v.size == nband * nrow * ncol):
            raise ValueError("band flux %r: the library writes it in place: a C-contiguous %s array of %d x %d x %d" % (k, dtype.name, nband, nrow, ncol))
        setattr(b, k, v.ctypes.data)
    return b


class LwArgs(C.Structure):
    _fields_ = ([(n, _i32) for n in ("ncol nlay memspace mcica icld idrv inflglw iceflglw liqflglw irng permuteseed "
                                     "shard_col0 shard_ncol struct_size").split()]
                + [(n, _vp) for n in ("play plev tlay tlev tsfc h2ovmr o3vmr co2vmr ch4vmr n2ovmr o2vmr cfc11vmr cfc12vmr "
                                      "cfc22vmr ccl4vmr emis cldfr taucld cicewp cliqwp reice reliq tauaer cldfmcl "
                                      "uflx dflx hr uflxc dflxc hrc duflx_dt duflxc_dt").split()]
                + [(n, _f64) for n in _SCALES])


class RadiationCall(C.Structure):
    """mirrors `rrtmg_radiation_call` (include/rrtmg_hip.h), field for field"""
    _fields_ = [("struct_size", C.c_int), ("sw", C.POINTER(SwArgs)), ("sw_surface", C.POINTER(SwSurface)),
                ("sw_components", C.POINTER(SwComponents)), ("sw_bands", C.POINTER(SwBandFluxes)),
                ("lw", C.POINTER(LwArgs)), ("lw_bands", C.POINTER(LwBandFluxes))]


SLAB_IN = ("sw_down lw_down sw_up lw_up lh sh up_heat_soil heat_flux_sea_ice sea_water_dens surf_dens heat_cap_soil surf_therm_cap "
           "ocean_mix_thick soil_layer_thick ocean_heat_transport").split()


class SlabArgs(C.Structure):
    """mirrors `rrtmg_slab_args` (include/rrtmg_hip.h), field for field"""
    _fields_ = [(n, _vp) for n in ("sw_down lw_down sw_up lw_up lh sh area_type up_heat_soil heat_flux_sea_ice sea_water_dens surf_dens "
                                   "heat_cap_soil surf_therm_cap ocean_mix_thick soil_layer_thick ocean_heat_transport tend_ts depth").split()]


class ScaleEntry(C.Structure):
    """mirrors `rrtmg_scale_entry` (include/rrtmg_hip.h), field for field"""
    _fields_ = [("src", _vp), ("dst", _vp), ("rows", _i32), ("reserved", _i32)]


SCALE_MAX_ENTRIES = 16      # RRTMG_SCALE_MAX_ENTRIES: the arrays of one rrtmg_hip_scale_columns call


class LwAdjust(C.Structure):
    """mirrors `rrtmg_lw_adjust` (include/rrtmg_hip.h), field for field"""
    _fields_ = ([("struct_size", C.c_uint32), ("ncol", _i32), ("nlay", _i32)]
                + [(n, _vp) for n in ("tsfc_call", "tsfc_now", "plev")] + [("pressure_scale", _f64)]
                + [(n, _vp) for n in "uflx dflx duflx_dt uflxc dflxc duflxc_dt uflx_out hr_out uflxc_out hrc_out".split()])


DRY_ADJUST_CONSTANTS = ("cpd", "cvap", "rd", "rv", "pref")
DRY_ADJUST_IN = ("t", "q", "pmid", "pint")
DRY_ADJUST_OUT = ("t_out", "q_out")
DRY_ADJUST_DIAG = ("mixed_top",)


class DryAdjust(C.Structure):
    """mirrors `rrtmg_dry_adjust` (include/rrtmg_hip.h), field for field"""
    _fields_ = ([("struct_size", C.c_uint32), ("ncol", _i32), ("nlay", _i32), ("memspace", _i32)]
                + [(n, _vp) for n in DRY_ADJUST_IN] + [(n, _f64) for n in DRY_ADJUST_CONSTANTS]
                + [(n, _vp) for n in DRY_ADJUST_OUT + DRY_ADJUST_DIAG])


BOUNDARY_LAYER_CONSTANTS = ("rd", "cp", "g", "lv", "karman", "z0", "fb", "p0", "ric")
BOUNDARY_LAYER_IN = ("t", "q", "u", "v", "pmid", "pint", "ps", "ts", "qs", "sh_in", "lh_in")
BOUNDARY_LAYER_OUT = ("t_out", "q_out", "u_out", "v_out")
BOUNDARY_LAYER_DIAG = ("stress_north", "stress_east", "height", "sh_out", "lh_out")


class BoundaryLayer(C.Structure):
    """mirrors `rrtmg_boundary_layer` (include/rrtmg_hip.h), field for field"""
    _fields_ = ([("struct_size", C.c_uint32), ("ncol", _i32), ("nlay", _i32), ("memspace", _i32), ("flux_mode", _i32)]
                + [(n, _vp) for n in BOUNDARY_LAYER_IN] + [("dt", _f64)] + [(n, _f64) for n in BOUNDARY_LAYER_CONSTANTS]
                + [("pressure_scale", _f64), ("ps_scale", _f64)] + [(n, _vp) for n in BOUNDARY_LAYER_OUT + BOUNDARY_LAYER_DIAG])


EMANUEL_PARAMETERS = ("elcrit", "tlcrit", "entp", "sigd", "sigs", "omtrain", "omtsnow", "coeffr", "coeffs", "cu", "beta", "dtmax", "alpha", "damp", "delt0")
EMANUEL_CONSTANTS = ("cpd", "cpv", "cl", "rv", "rd", "lv0", "g", "rowl")
EMANUEL_IN = ("t", "q", "u", "v", "pmid", "pint", "cbmf", "qs")
EMANUEL_OUT = ("ft", "fq", "fu", "fv")
EMANUEL_DIAG = ("precip", "wd", "tprime", "qprime", "cape", "iflag", "ft_per_day")


class Emanuel(C.Structure):
    """mirrors `rrtmg_emanuel` (include/rrtmg_hip.h), field for field"""
    _fields_ = ([("struct_size", C.c_uint32), ("ncol", _i32), ("nlay", _i32), ("memspace", _i32)] + [(n, _vp) for n in EMANUEL_IN]
                + [("dt", _f64), ("pressure_scale", _f64), ("minorig", _i32), ("reserved", _i32)] + [(n, _f64) for n in EMANUEL_PARAMETERS + EMANUEL_CONSTANTS]
                + [(n, _vp) for n in EMANUEL_OUT + EMANUEL_DIAG + ("cbmf_out",)])


SIMPLE_PHYSICS_SWITCHES = ("do_lsc", "do_pbl", "do_surf_flux", "use_ts_ext", "use_qsurf_ext", "test", "clamp_latent_heat_flux")
SIMPLE_PHYSICS_CONSTANTS = ("g", "cpair", "rair", "latvap", "rh2o", "radius", "omega", "rhow", "pbltop", "pblconst", "c_heat", "cd0", "cd1", "cm")
SIMPLE_PHYSICS_IN = ("t", "q", "u", "v", "pmid", "pint", "ps", "ts", "qsurf", "lat")
SIMPLE_PHYSICS_OUT = ("t_out", "q_out", "u_out", "v_out")
SIMPLE_PHYSICS_DIAG = ("precl", "sh_out", "lh_out")


class SimplePhysics(C.Structure):
    """mirrors `rrtmg_simple_physics` (include/rrtmg_hip.h), field for field"""
    _fields_ = ([("struct_size", C.c_uint32), ("ncol", _i32), ("nlay", _i32), ("memspace", _i32)] + [(n, _i32) for n in SIMPLE_PHYSICS_SWITCHES + ("reserved",)]
                + [(n, _vp) for n in SIMPLE_PHYSICS_IN] + [("dt", _f64)] + [(n, _f64) for n in SIMPLE_PHYSICS_CONSTANTS]
                + [("pressure_scale", _f64), ("ps_scale", _f64)] + [(n, _vp) for n in SIMPLE_PHYSICS_OUT + SIMPLE_PHYSICS_DIAG])


FRIERSON_SCALARS = ("tau0e", "tau0p", "fl")
FRIERSON_IN = ("pint", "ps", "lat")
FRIERSON_OUT = ("tau",)
FRIERSON_DIAG = ()


class FriersonOpticalDepth(C.Structure):
    """mirrors `rrtmg_frierson_optical_depth` (include/rrtmg_hip.h), field for field"""
    _fields_ = ([("struct_size", C.c_uint32), ("ncol", _i32), ("nlay", _i32), ("memspace", _i32)] + [(n, _vp) for n in FRIERSON_IN]
                + [(n, _f64) for n in FRIERSON_SCALARS] + [("pressure_scale", _f64), ("ps_scale", _f64)] + [(n, _vp) for n in FRIERSON_OUT])


GRAY_LONGWAVE_CONSTANTS = ("sigma_sb", "g", "cpd")
GRAY_LONGWAVE_IN = ("t", "tsfc", "pint", "tau", "ps", "lat")
GRAY_LONGWAVE_OUT = ("up", "dn", "tend")
GRAY_LONGWAVE_DIAG = ("hr", "tau_out")


class GrayLongwave(C.Structure):
    """mirrors `rrtmg_gray_longwave` (include/rrtmg_hip.h), field for field"""
    _fields_ = ([("struct_size", C.c_uint32), ("ncol", _i32), ("nlay", _i32), ("memspace", _i32), ("frierson", _i32), ("reserved", _i32)]
                + [(n, _vp) for n in GRAY_LONGWAVE_IN] + [(n, _f64) for n in FRIERSON_SCALARS + GRAY_LONGWAVE_CONSTANTS]
                + [("pressure_scale", _f64), ("ps_scale", _f64)] + [(n, _vp) for n in GRAY_LONGWAVE_OUT + GRAY_LONGWAVE_DIAG])


GRID_SCALE_CONDENSATION_CONSTANTS = ("cpd", "lv", "rd", "rh2o", "g", "rhow")
GRID_SCALE_CONDENSATION_IN = ("t", "q", "pmid", "pint")
GRID_SCALE_CONDENSATION_OUT = ("t_out", "q_out")
GRID_SCALE_CONDENSATION_DIAG = ("precip",)


class GridScaleCondensation(C.Structure):
    """mirrors `rrtmg_grid_scale_condensation` (include/rrtmg_hip.h), field for field"""
    _fields_ = ([("struct_size", C.c_uint32), ("ncol", _i32), ("nlay", _i32), ("memspace", _i32)] + [(n, _vp) for n in GRID_SCALE_CONDENSATION_IN]
                + [(n, _f64) for n in GRID_SCALE_CONDENSATION_CONSTANTS] + [("pressure_scale", _f64)]
                + [(n, _vp) for n in GRID_SCALE_CONDENSATION_OUT + GRID_SCALE_CONDENSATION_DIAG])


CORK_MAX_GAS = 8
CORK_TABLE_SIZES = ("ngas", "nband", "ngpt", "nT", "nP", "nX", "nC")
CORK_LONGWAVE_GASES = tuple("gas%d" % i for i in range(CORK_MAX_GAS))
CORK_LONGWAVE_CONSTANTS = ("m_h2o", "sigma_sb", "g", "cpd", "diffusivity")
CORK_LONGWAVE_IN = ("t", "pmid", "pint", "tsfc", "emis", "taucld") + CORK_LONGWAVE_GASES
CORK_LONGWAVE_OUT = ("up", "dn", "tend")
CORK_LONGWAVE_DIAG = ("hr", "up_band", "dn_band", "tau_band", "trans_band", "hr_band")


class CorkTableDesc(C.Structure):
    """mirrors `rrtmg_cork_table_desc` (include/rrtmg_hip.h), field for field"""
    _fields_ = ([("struct_size", C.c_uint32)] + [(n, _i32) for n in CORK_TABLE_SIZES] + [("k_is_f32", _i32), ("reserved", _i32)]
                + [(n, _vp) for n in ("k", "weights", "planck", "t_grid", "p_grid_log", "x_grid_log", "c_grid_log")]
                + [("x_clip", _f64 * 2), ("c_clip", _f64 * 2), ("log_cont", _vp)])


class CorkLongwave(C.Structure):
    """mirrors `rrtmg_cork_longwave` (include/rrtmg_hip.h), field for field"""
    _fields_ = ([("struct_size", C.c_uint32), ("ncol", _i32), ("nlay", _i32), ("memspace", _i32), ("gas_rule", _i32), ("reserved", _i32), ("table", _vp)]
                + [(n, _vp) for n in CORK_LONGWAVE_IN] + [("gas_scale", _f64 * CORK_MAX_GAS)] + [(n, _f64) for n in CORK_LONGWAVE_CONSTANTS]
                + [("pressure_scale", _f64)] + [(n, _vp) for n in CORK_LONGWAVE_OUT + CORK_LONGWAVE_DIAG])


CORK_SHORTWAVE_CONSTANTS = ("m_h2o", "g", "cpd")
CORK_SHORTWAVE_CLOUD = ("taucld", "ssacld", "asycld")
CORK_SHORTWAVE_IN = ("t", "pmid", "pint", "zenith", "albedo", "earth_sun") + CORK_SHORTWAVE_CLOUD + CORK_LONGWAVE_GASES
CORK_SHORTWAVE_OUT = ("up", "dn", "tend")
CORK_SHORTWAVE_DIAG = ("hr", "up_band", "dn_band", "tau_band", "hr_band")


class CorkSwTableDesc(C.Structure):
    """mirrors `rrtmg_cork_sw_table_desc` (include/rrtmg_hip.h), field for field"""
    _fields_ = ([("struct_size", C.c_uint32)] + [(n, _i32) for n in CORK_TABLE_SIZES] + [("k_is_f32", _i32), ("solar_is_f32", _i32)]
                + [(n, _vp) for n in ("k", "weights", "t_grid", "p_grid_log", "x_grid_log")]
                + [("x_clip", _f64 * 2)] + [(n, _vp) for n in ("log_cont", "solar_source", "rayleigh")])


class CorkShortwave(C.Structure):
    """mirrors `rrtmg_cork_shortwave` (include/rrtmg_hip.h), field for field"""
    _fields_ = ([("struct_size", C.c_uint32), ("ncol", _i32), ("nlay", _i32), ("memspace", _i32), ("gas_rule", _i32), ("max_chunk_cols", _i32), ("table", _vp)]
                + [(n, _vp) for n in CORK_SHORTWAVE_IN] + [("gas_scale", _f64 * CORK_MAX_GAS)] + [(n, _f64) for n in CORK_SHORTWAVE_CONSTANTS]
                + [("pressure_scale", _f64)] + [(n, _vp) for n in CORK_SHORTWAVE_OUT + CORK_SHORTWAVE_DIAG])


SURFACE_ICE_FLUXES = ("sw_down", "lw_down", "sw_up", "lw_up", "lh", "sh")
SURFACE_ICE_CONSTANTS = ("rho_ice", "rho_snow", "c_ice", "c_snow", "k_ice", "k_snow", "lf", "t_melt", "eps", "max_height", "albedo_snow", "albedo_ice", "albedo_melt")
SURFACE_ICE_IN = ("t", "height", "thick", "snow", "base") + SURFACE_ICE_FLUXES + ("area_type",)
SURFACE_ICE_OUT = ("t_out", "height_out", "thick_out", "snow_out", "tsfc_out", "base_flux_out")
SURFACE_ICE_DIAG = ("cond_flux", "albedo", "flags")


class SurfaceIce(C.Structure):
    """mirrors `rrtmg_surface_ice` (include/rrtmg_hip.h), field for field"""
    _fields_ = ([("struct_size", C.c_uint32), ("ncol", _i32), ("nlay", _i32), ("memspace", _i32), ("kind", _i32), ("reserved", _i32)]
                + [(n, _vp) for n in SURFACE_ICE_IN] + [("dt", _f64)] + [(n, _f64) for n in SURFACE_ICE_CONSTANTS]
                + [(n, _vp) for n in SURFACE_ICE_OUT + SURFACE_ICE_DIAG])


LAND_FLUXES = ("sw_down", "lw_down", "sw_up", "lw_up")
BUCKET_HYDROLOGY_SCALARS = ("rd", "cp", "rho_water", "lv", "bulk_coefficient", "beta_parameter", "soil_moisture_max", "deep_soil_moisture_max", "tau_m", "deep_ratio", "tau_drain")
BUCKET_HYDROLOGY_DEEP = ("deep_moisture", "deep_temperature")      # the inputs, outputs (+ "_out") and diagnostics of layers 2 only
BUCKET_HYDROLOGY_IN = (("t_air", "q_air", "u", "v", "p_air", "ts", "q_sfc") + LAND_FLUXES
                       + ("soil_moisture", "precip_conv", "precip_strat", "density", "thickness", "heat_capacity") + BUCKET_HYDROLOGY_DEEP)
BUCKET_HYDROLOGY_OUT = ("ts_out", "soil_moisture_out", "deep_moisture_out", "deep_temperature_out")
BUCKET_HYDROLOGY_DIAG = ("precip", "lh", "sh", "evaporation", "runoff", "deep_fraction")


class BucketHydrology(C.Structure):
    """mirrors `rrtmg_bucket_hydrology` (include/rrtmg_hip.h), field for field"""
    _fields_ = ([("struct_size", C.c_uint32), ("ncol", _i32), ("nlay", _i32), ("memspace", _i32), ("layers", _i32), ("has_drain", _i32), ("reserved", _i32), ("reserved2", _i32)]
                + [(n, _vp) for n in BUCKET_HYDROLOGY_IN] + [("dt", _f64)] + [(n, _f64) for n in BUCKET_HYDROLOGY_SCALARS] + [("pressure_scale", _f64)]
                + [(n, _vp) for n in BUCKET_HYDROLOGY_OUT + BUCKET_HYDROLOGY_DIAG])


SECOND_BEST_CONSTANTS = ("rd", "g", "cp", "lv", "lf", "rho_water", "karman", "t_freeze", "min_wind", "kappa_soil", "cv_soil", "colour", "texture", "B", "K_H0", "psi_0")
SECOND_BEST_SOIL = ("t_soil", "x_w", "x_i", "height")
SECOND_BEST_IN = SECOND_BEST_SOIL + ("t_air", "q_air", "u", "v", "p_air", "ps", "ts", "snow") + LAND_FLUXES + ("area_type",)
SECOND_BEST_OUT = ("t_soil_out", "x_w_out", "x_i_out", "ts_out", "snow_out")
SECOND_BEST_DIAG = ("sh", "lh", "evaporation", "albedo_direct", "albedo_diffuse", "cd_heat", "cd_momentum", "t2m", "q2m", "u10", "v10", "flags")


class SecondBest(C.Structure):
    """mirrors `rrtmg_second_best` (include/rrtmg_hip.h), field for field"""
    _fields_ = ([("struct_size", C.c_uint32), ("ncol", _i32), ("nlay", _i32), ("memspace", _i32)] + [(n, _vp) for n in SECOND_BEST_IN]
                + [("dt", _f64)] + [(n, _f64) for n in SECOND_BEST_CONSTANTS] + [("pressure_scale", _f64), ("ps_scale", _f64), ("reserved", _i32), ("reserved2", _i32)]
                + [(n, _vp) for n in SECOND_BEST_OUT + SECOND_BEST_DIAG])


# The six extents of ColumnExt (csrc/rrtmg_column_call.h), written as the check programs print them -> the shape of the device
# array at (nlay, ncol, nband).
LAY, LEV, COL, BAND_LAY, BAND_LEV, BAND_COL = "[nlay][ncol]", "[nlay+1][ncol]", "[ncol]", "[nband][nlay][ncol]", "[nband][nlay+1][ncol]", "[nband][ncol]"
COLUMN_EXTENTS = {LAY: lambda L, N, B: (L, N), LEV: lambda L, N, B: (L + 1, N), COL: lambda L, N, B: (N,),
                  BAND_LAY: lambda L, N, B: (B, L, N), BAND_LEV: lambda L, N, B: (B, L + 1, N), BAND_COL: lambda L, N, B: (B, N)}
_F64, _I32 = np.dtype(np.float64), np.dtype(np.int32)


def _column_arrays(struct, IN, DIAG, int32=(), optional=(), in_place=(), grid=None, host_axes=None, **names_of):
    """One entry of COLUMN_ARRAYS.  `names_of`: levels=, columns=, band_layers=, band_levels=, band_columns= name the arrays of
    each extent; every other pointer member of `struct` is [nlay][ncol]."""
    members = tuple(n for n, t in struct._fields_ if t is _vp and n != "table")
    extent = dict.fromkeys(members, LAY)
    for key, names in names_of.items():
        assert set(names) <= set(members), (struct, key)
        extent.update(dict.fromkeys(names, dict(levels=LEV, columns=COL, band_layers=BAND_LAY, band_levels=BAND_LEV, band_columns=BAND_COL)[key]))
    return dict(struct=struct, IN=IN, DIAG=DIAG, extent=extent, dtype={n: _I32 if n in int32 else _F64 for n in members}, optional=optional, in_place=in_place,
                grid=grid, host_axes=host_axes or {})


# The single description of a column component's arrays on the Python side, by entry (rrtmg_hip_<entry>): `struct`, whose pointer
# members are the arrays, in the order of the library's table; `IN` and `DIAG` (the outputs are what lies between); `extent` and
# `dtype` by name; `optional`: the inputs that may be absent; `in_place`: (output, input) pairs for which an output that IS the
# caller's input array means that array, not its contiguous copy; `grid`: the input whose shape is the call's -- [nlay][ncol], or
# [ncol] where every array is a column and nlay is 1 (default: t, or pint less one level); `host_axes`: for an array the caller
# holds in another axis order than the device, the device axis of each host axis.  Context._column_call reads nothing else;
# tests/helpers.py (column_rows_agree) holds every key to the rows the library's own tables print.
COLUMN_ARRAYS = {
    "dry_adjustment": _column_arrays(DryAdjust, DRY_ADJUST_IN, DRY_ADJUST_DIAG, int32=("mixed_top",), in_place=(("t_out", "t"), ("q_out", "q")), levels=("pint",), columns=("mixed_top",)),
    "boundary_layer": _column_arrays(BoundaryLayer, BOUNDARY_LAYER_IN, BOUNDARY_LAYER_DIAG, optional=("sh_in", "lh_in"), in_place=tuple((n + "_out", n) for n in "tquv"), levels=("pint",),
                                     columns=("ps", "ts", "qs", "sh_in", "lh_in", "stress_north", "stress_east", "height", "sh_out", "lh_out")),
    "emanuel_convection": _column_arrays(Emanuel, EMANUEL_IN, EMANUEL_DIAG, int32=("iflag",), optional=("qs",), in_place=(("cbmf_out", "cbmf"),), levels=("pint",),
                                         columns=("cbmf", "cbmf_out", "precip", "wd", "tprime", "qprime", "cape", "iflag")),
    "simple_physics": _column_arrays(SimplePhysics, SIMPLE_PHYSICS_IN, SIMPLE_PHYSICS_DIAG, optional=("ts", "qsurf", "lat"), in_place=tuple((n + "_out", n) for n in "tquv"),
                                     levels=("pint",), columns=("ps", "ts", "qsurf", "lat", "precl", "sh_out", "lh_out")),
    # (the gray path: outputs on the interface levels too; the depth has no profile input, its grid is pint's)
    "frierson_optical_depth": _column_arrays(FriersonOpticalDepth, FRIERSON_IN, FRIERSON_DIAG, levels=("pint", "tau"), columns=("ps", "lat")),
    "gray_longwave": _column_arrays(GrayLongwave, GRAY_LONGWAVE_IN, GRAY_LONGWAVE_DIAG, optional=("tau", "ps", "lat"), levels=("pint", "tau", "up", "dn", "tau_out"),
                                    columns=("tsfc", "ps", "lat")),
    "grid_scale_condensation": _column_arrays(GridScaleCondensation, GRID_SCALE_CONDENSATION_IN, GRID_SCALE_CONDENSATION_DIAG, in_place=(("t_out", "t"), ("q_out", "q")),
                                              levels=("pint",), columns=("precip",)),
    # (the correlated-k longwave: extents times the call's nband; the caller holds taucld as [nlay][ncol][nband])
    "cork_longwave": _column_arrays(CorkLongwave, CORK_LONGWAVE_IN, CORK_LONGWAVE_DIAG, optional=("taucld",) + CORK_LONGWAVE_GASES, host_axes=dict(taucld=(1, 2, 0)),
                                    levels=("pint", "up", "dn"), columns=("tsfc",), band_columns=("emis",), band_levels=("up_band", "dn_band"),
                                    band_layers=("taucld", "tau_band", "trans_band", "hr_band")),
    # (the correlated-k shortwave: likewise; the three cloud arrays are the caller's [nlay][ncol][nband])
    "cork_shortwave": _column_arrays(CorkShortwave, CORK_SHORTWAVE_IN, CORK_SHORTWAVE_DIAG, optional=CORK_SHORTWAVE_CLOUD + CORK_LONGWAVE_GASES,
                                     host_axes={n: (1, 2, 0) for n in CORK_SHORTWAVE_CLOUD}, levels=("pint", "up", "dn"), columns=("zenith", "albedo", "earth_sun"),
                                     band_levels=("up_band", "dn_band"), band_layers=CORK_SHORTWAVE_CLOUD + ("tau_band", "hr_band")),
    # (the snow/ice column: nlay counts the ice interface levels, so there are no levels; an int32 input)
    "surface_ice": _column_arrays(SurfaceIce, SURFACE_ICE_IN, SURFACE_ICE_DIAG, int32=("area_type", "flags"),
                                  in_place=(("t_out", "t"), ("height_out", "height"), ("thick_out", "thick"), ("snow_out", "snow"), ("base_flux_out", "base")),
                                  columns=("thick", "snow", "base") + SURFACE_ICE_FLUXES + ("area_type", "thick_out", "snow_out", "tsfc_out", "base_flux_out", "cond_flux", "albedo", "flags")),
    # (the land surface)
    "bucket_hydrology": _column_arrays(BucketHydrology, BUCKET_HYDROLOGY_IN, BUCKET_HYDROLOGY_DIAG, grid="ts", optional=BUCKET_HYDROLOGY_DEEP,
                                       in_place=tuple((n + "_out", n) for n in ("ts", "soil_moisture") + BUCKET_HYDROLOGY_DEEP),
                                       columns=BUCKET_HYDROLOGY_IN + BUCKET_HYDROLOGY_OUT + BUCKET_HYDROLOGY_DIAG),
    "second_best": _column_arrays(SecondBest, SECOND_BEST_IN, SECOND_BEST_DIAG, grid="t_soil", int32=("area_type", "flags"),
                                  in_place=tuple((n + "_out", n) for n in ("t_soil", "x_w", "x_i", "ts", "snow")),
                                  columns=SECOND_BEST_IN[4:] + ("ts_out", "snow_out") + SECOND_BEST_DIAG),
}


_lib = None


def load_library():
    """Load librrtmg_hip.so; raises ImportError (as climt does for its missing Fortran extension,
    lw/component.py:253-257) when it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError("librrtmg_hip.so has not been built (%s); run `python -c 'import __graft_entry__ as g; g.build()'`" % LIB_PATH)
    lib = C.CDLL(LIB_PATH)
    lib.rrtmg_hip_last_error.restype = C.c_char_p
    lib.rrtmg_hip_last_error.argtypes = [_vp]
    lib.rrtmg_hip_version.restype = C.c_char_p
    lib.rrtmg_hip_stream.restype = _vp
    lib.rrtmg_hip_stream.argtypes = [_vp]
    lib.rrtmg_hip_create.argtypes = [C.POINTER(_vp), C.c_int]
    lib.rrtmg_hip_destroy.argtypes = [_vp]
    lib.rrtmg_hip_set_constants.argtypes = [_vp] + [_f64] * 10
    lib.rrtmg_hip_sw_init.argtypes = [_vp, _f64, C.c_char_p]
    lib.rrtmg_hip_lw_init.argtypes = [_vp, _f64, C.c_char_p]
    lib.rrtmg_hip_sw_fluxes.argtypes = [_vp, C.POINTER(SwArgs)]
    lib.rrtmg_hip_lw_fluxes.argtypes = [_vp, C.POINTER(LwArgs)]
    lib.rrtmg_hip_sw_fluxes_components.argtypes = [_vp, C.POINTER(SwArgs), C.POINTER(SwComponents)]
    lib.rrtmg_hip_sw_fluxes_bands.argtypes = [_vp, C.POINTER(SwArgs), C.POINTER(SwComponents), C.POINTER(SwBandFluxes)]
    if hasattr(lib, "rrtmg_hip_sw_fluxes_surface"):      # (a library named by RRTMG_HIP_LIB may predate it: probed by the symbol)
        lib.rrtmg_hip_sw_fluxes_surface.argtypes = [_vp, C.POINTER(SwArgs), C.POINTER(SwSurface), C.POINTER(SwComponents), C.POINTER(SwBandFluxes)]
    lib.rrtmg_hip_lw_fluxes_bands.argtypes = [_vp, C.POINTER(LwArgs), C.POINTER(LwBandFluxes)]
    lib.rrtmg_hip_band_limits.argtypes = [C.c_int, _vp, _vp]
    lib.rrtmg_hip_get_table.restype = C.c_long
    lib.rrtmg_hip_get_table.argtypes = [_vp, C.c_char_p, _vp, C.c_long]
    lib.rrtmg_hip_lw_tables_synthetic.argtypes = [_vp]
    lib.rrtmg_hip_synchronize.argtypes = [_vp]
    lib.rrtmg_hip_set_deferred.argtypes = [_vp, C.c_int]
    lib.rrtmg_hip_stream_wait.argtypes = [_vp, _vp]
    lib.rrtmg_hip_interface_values.argtypes = [_vp, C.c_int, C.c_int, _vp, _vp, _vp, _vp, _vp]
    lib.rrtmg_hip_elementwise.argtypes = [_vp, C.c_int, C.c_long, _vp, _vp, _f64, _f64, _vp]
    lib.rrtmg_hip_ab_step.argtypes = [_vp, C.c_long, C.c_int, _vp, C.POINTER(_vp), C.POINTER(_f64), _f64, _vp]
    lib.rrtmg_hip_order_streams.argtypes = [_vp, C.c_int]
    lib.rrtmg_hip_zenith_angle.argtypes = [_vp, C.c_int, C.c_int, _vp, _vp, _f64, _vp]
    lib.rrtmg_hip_slab_surface.argtypes = [_vp, C.c_int, C.c_int, C.POINTER(SlabArgs)]
    lib.rrtmg_hip_solar_insolation.argtypes = [_vp, C.c_int, C.c_int, _vp, _vp, _f64, _f64, _f64, _f64, _vp, _vp]
    lib.rrtmg_hip_kernel_ms.argtypes = [_vp, C.c_int, C.POINTER(C.c_double)]
    lib.rrtmg_hip_kernel_launches.argtypes = [_vp, C.c_int]
    lib.rrtmg_hip_set_column_sort.argtypes = [_vp, C.c_int]
    if hasattr(lib, "rrtmg_hip_set_sw_night_skip"):      # (RRTMG_HIP_LIB may name a library that predates it, as for the entry above)
        lib.rrtmg_hip_set_sw_night_skip.argtypes = [_vp, C.c_int]
        lib.rrtmg_hip_sw_night_last.argtypes = [_vp, C.POINTER(C.c_int), C.POINTER(C.c_int)]
    if hasattr(lib, "rrtmg_hip_set_sw_night_pack"):      # (likewise)
        lib.rrtmg_hip_set_sw_night_pack.argtypes = [_vp, C.c_int]
    if hasattr(lib, "rrtmg_hip_set_sw_clear_sky"):       # (likewise)
        lib.rrtmg_hip_set_sw_clear_sky.argtypes = [_vp, C.c_int]
    if hasattr(lib, "rrtmg_hip_set_lw_clear_sky"):       # (likewise)
        lib.rrtmg_hip_set_lw_clear_sky.argtypes = [_vp, C.c_int]
    if hasattr(lib, "rrtmg_hip_radiation_fluxes"):       # (likewise)
        lib.rrtmg_hip_radiation_fluxes.argtypes = [_vp, C.POINTER(RadiationCall)]
        lib.rrtmg_hip_radiation_last.argtypes = [_vp, C.POINTER(C.c_int), C.POINTER(C.c_longlong), C.POINTER(C.c_longlong)]
    if hasattr(lib, "rrtmg_hip_sw_fluxes_f32"):          # (likewise: the float32 boundary)
        lib.rrtmg_hip_sw_fluxes_f32.argtypes = [_vp, C.POINTER(SwArgs), C.POINTER(SwSurface), C.POINTER(SwComponents), C.POINTER(SwBandFluxes)]
        lib.rrtmg_hip_lw_fluxes_f32.argtypes = [_vp, C.POINTER(LwArgs), C.POINTER(LwBandFluxes)]
        lib.rrtmg_hip_radiation_fluxes_f32.argtypes = [_vp, C.POINTER(RadiationCall)]
    if hasattr(lib, "rrtmg_hip_set_mcica_overlap_alpha"):   # (likewise: exponential / exponential-random McICA overlap)
        lib.rrtmg_hip_set_mcica_overlap_alpha.argtypes = [_vp, C.c_int, C.c_int, C.c_int, C.c_int, _vp]
        lib.rrtmg_hip_overlap_alpha.argtypes = [_vp, C.c_int, C.c_int, C.c_int, _vp, _vp, _f64, _f64, _vp]
    if hasattr(lib, "rrtmg_hip_mean_coszen"):               # (likewise: the shortwave between radiation calls)
        lib.rrtmg_hip_mean_coszen.argtypes = [_vp, C.c_int, C.c_int, _vp, _vp, _f64, _f64, _vp, _vp, _vp, _vp]
        lib.rrtmg_hip_mean_coszen_sun.argtypes = [_vp, C.c_int, C.c_int, _vp, _vp, _f64, _f64, _f64, _f64, _vp, _vp, _vp, _vp]
        lib.rrtmg_hip_scale_columns.argtypes = [_vp, C.c_int, _vp, _vp, C.c_int, C.POINTER(ScaleEntry)]
    if hasattr(lib, "rrtmg_hip_lw_adjust_surface"):         # (likewise: the longwave between radiation calls)
        lib.rrtmg_hip_lw_adjust_surface.argtypes = [_vp, C.POINTER(LwAdjust)]
    for entry, arrays in COLUMN_ARRAYS.items():             # (likewise, entry by entry: the column components)
        if hasattr(lib, "rrtmg_hip_" + entry):
            getattr(lib, "rrtmg_hip_" + entry).argtypes = [_vp, C.POINTER(arrays["struct"])]
    if hasattr(lib, "rrtmg_hip_cork_table_create"):         # (likewise: the tables of the correlated-k longwave)
        lib.rrtmg_hip_cork_table_create.argtypes = [_vp, C.POINTER(CorkTableDesc), C.POINTER(_vp)]
        lib.rrtmg_hip_cork_table_destroy.argtypes = [_vp, _vp]
    if hasattr(lib, "rrtmg_hip_cork_sw_table_create"):      # (likewise: the tables of the correlated-k shortwave)
        lib.rrtmg_hip_cork_sw_table_create.argtypes = [_vp, C.POINTER(CorkSwTableDesc), C.POINTER(_vp)]
    lib.rrtmg_hip_copy_blocks.argtypes =[_vp, C.c_int, _vp, C.c_long, C.c_long, _vp, _vp, _vp]
    lib.rrtmg_hip_mcica_mask.argtypes = [_vp] + [C.c_int] * 6 + [_vp] * 3
    _lib = lib
    return lib


# the ten constants in the order of rrtmg_sw_set_constants (rrtmg_sw_c_binder.f90:19-46)
CONSTANT_NAMES = ("pi", "grav", "planck", "boltz", "clight", "avogad", "alosmt", "gascon", "sbcnst", "secdy")

# boundary-level names (left) -> SwArgs / LwArgs field (right)
_SW_FIELDS = dict(play="play", plev="plev", tlay="tlay", tlev="tlev", tsfc="tsfc", h2o="h2ovmr", o3="o3vmr", co2="co2vmr",
                  ch4="ch4vmr", n2o="n2ovmr", o2="o2vmr", asdir="asdir", asdif="asdif", aldir="aldir", aldif="aldif",
                  coszen="coszen", cldfr="cldfr", taucld="taucld", ssacld="ssacld", asmcld="asmcld", fsfcld="fsfcld",
                  cicewp="cicewp", cliqwp="cliqwp", reice="reice", reliq="reliq", tauaer="tauaer", ssaaer="ssaaer",
                  asmaer="asmaer", ecaer="ecaer", cldfmcl="cldfmcl", bndsolvar="bndsolvar", indsolvar="indsolvar")
_LW_FIELDS = dict(play="play", plev="plev", tlay="tlay", tlev="tlev", tsfc="tsfc", h2o="h2ovmr", o3="o3vmr", co2="co2vmr",
                  ch4="ch4vmr", n2o="n2ovmr", o2="o2vmr", cfc11="cfc11vmr", cfc12="cfc12vmr", cfc22="cfc22vmr", ccl4="ccl4vmr",
                  emis="emis", cldfr="cldfr", taucld="taucld", cicewp="cicewp", cliqwp="cliqwp", reice="reice", reliq="reliq",
                  tauaer="tauaer", cldfmcl="cldfmcl")
_SW_FLAGS = dict(icld="icld", iaer="iaer", inflg="inflgsw", iceflg="iceflgsw", liqflg="liqflgsw", dyofyr="dyofyr",
                 isolvar="isolvar", irng="irng", permuteseed="permuteseed", shard_col0="shard_col0", shard_ncol="shard_ncol")
_LW_FLAGS = dict(icld="icld", idrv="idrv", inflg="inflglw", iceflg="iceflglw", liqflg="liqflglw", irng="irng",
                 permuteseed="permuteseed", shard_col0="shard_col0", shard_ncol="shard_ncol")
SW_OUT = (("swuflx", 1), ("swdflx", 1), ("swhr", 0), ("swuflxc", 1), ("swdflxc", 1), ("swhrc", 0))
SW_OUT_ALLSKY = ("swuflx", "swdflx", "swhr")      # what a call fills after Context.set_sw_clear_sky(False)
LW_OUT = (("uflx", 1), ("dflx", 1), ("hr", 0), ("uflxc", 1), ("dflxc", 1), ("hrc", 0))
LW_OUT_CLEAR = ("uflxc", "dflxc", "hrc", "duflxc_dt")      # what a call leaves out after Context.set_lw_clear_sky(False)


def source_hash():
    """The hash of the sources the loaded library was built from (rrtmg_hip_version(): "... src:<16 hex digits>")."""
    v = load_library().rrtmg_hip_version().decode()
    return v.split("src:")[1].strip() if "src:" in v else "unknown"


def _locked(fn):
    """Context methods that enter the library hold the context's lock: ctypes releases the GIL for the duration of a
    call, and a context -- its staging buffers, work-buffer map, error string, streams -- is shared by every component of
    the process on that device (climt_amd.rrtmg.common.make_context), so two Python threads must not be inside it at once."""
    @functools.wraps(fn)
    def wrapper(self, *args, **kwargs):
        with self._lock:
            return fn(self, *args, **kwargs)
    return wrapper


def band_limits(spectrum):
    """-> (lo, hi): the band limits in cm^-1 of "sw" (14 bands, RRTMG bands 16..29 in the order of the band arrays: band 29,
    820-2600 cm^-1, is last) or "lw" (16 bands)."""
    lib = load_library()
    n = {"sw": SW_NBAND, "lw": LW_NBAND}[spectrum]
    lo, hi = np.zeros(n), np.zeros(n)
    if lib.rrtmg_hip_band_limits(0 if spectrum == "sw" else 1, lo.ctypes.data, hi.ctypes.data) != n:
        raise RuntimeError("rrtmg_hip_band_limits(%s) failed" % spectrum)
    return lo, hi


class Context:
    """One librrtmg_hip context: constants, device tables, work buffers, HIP streams.  Calls are serialised per context
    (a re-entrant lock), so components sharing it may be driven from several Python threads."""

    def __init__(self, device=0):
        self.lib = load_library()
        self._lock = threading.RLock()
        self.deferred = False
        h = _vp()
        rc = self.lib.rrtmg_hip_create(C.byref(h), int(device))
        self.h = h
        self.device = device
        if rc:
            msg = self.lib.rrtmg_hip_last_error(self.h).decode() if self.h else "context creation failed"
            raise RRTMGError(rc, msg)

    def close(self):
        if getattr(self, "h", None):
            self.lib.rrtmg_hip_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _ck(self, rc):
        if rc:
            raise RRTMGError(rc, self.lib.rrtmg_hip_last_error(self.h).decode())

    @_locked
    def set_constants(self, **k):
        self._ck(self.lib.rrtmg_hip_set_constants(self.h, *[float(k[n]) for n in CONSTANT_NAMES]))

    @_locked
    def sw_init(self, cpdair, blob=None):
        blob = blob or os.environ.get("RRTMG_HIP_SW_DATA") or SW_DATA
        key = ("sw", float(cpdair), blob)
        if getattr(self, "_sw_key", None) != key:       # (components sharing the context initialise the tables once)
            self._ck(self.lib.rrtmg_hip_sw_init(self.h, float(cpdair), blob.encode()))
            self._sw_key = key

    @_locked
    def lw_init(self, cpdair, blob=None):
        blob = blob or os.environ.get("RRTMG_HIP_LW_DATA") or LW_DATA      # (a packed table file elsewhere: tools/ingest_lw_data.sh)
        key = ("lw", float(cpdair), blob)
        if getattr(self, "_lw_key", None) != key:
            self._ck(self.lib.rrtmg_hip_lw_init(self.h, float(cpdair), blob.encode()))
            self._lw_key = key

    def lw_tables_synthetic(self):
        return bool(self.lib.rrtmg_hip_lw_tables_synthetic(self.h))

    @property
    def stream(self):
        return self.lib.rrtmg_hip_stream(self.h)

    @_locked
    def kernel_ms(self, which, cloudy=False):
        """HIP-event duration (ms) of a solve kernel in the last call, summed over the call's column chunks (one launch
        each): which = 'sw' | 'lw'; cloudy selects the kernel that handles the cloudy tiles (sw_solve_cloudy_kernel /
        lw_solve_all_kernel<true,..>) instead of the clear-sky one."""
        ms = C.c_double(0.0)
        self._ck(self.lib.rrtmg_hip_kernel_ms(self.h, (0 if which == "sw" else 1) + (2 if cloudy else 0), C.byref(ms)))
        return ms.value

    @_locked
    def kernel_launches(self, which, cloudy=False):
        """Launches (column chunks) of that solve kernel in the last call; kernel_ms is their sum."""
        return int(self.lib.rrtmg_hip_kernel_launches(self.h, (0 if which == "sw" else 1) + (2 if cloudy else 0)))

    @_locked
    def copy_blocks(self, desc_ptr, nblk, max_rows, max_cols, src, dst, stream=None):
        """rrtmg_hip_copy_blocks: nblk strided 2-d block copies (device pointers; desc = device int64[nblk][6]) on `stream`."""
        self._ck(self.lib.rrtmg_hip_copy_blocks(self.h, int(nblk), _vp(desc_ptr), int(max_rows), int(max_cols), _vp(src), _vp(dst), _vp(stream)))

    @_locked
    def synchronize(self):
        """Wait for all enqueued work; in deferred mode this is where device-side errors are raised."""
        self._ck(self.lib.rrtmg_hip_synchronize(self.h))

    @_locked
    def stream_wait(self, other_stream):
        """`other_stream` (hipStream_t) waits, on the device, for everything enqueued so far on this context's streams."""
        self._ck(self.lib.rrtmg_hip_stream_wait(self.h, _vp(other_stream)))

    # -- glue of the device-resident step (device pointers) ------------------------------------------
    @_locked
    def interface_values(self, ncol, nlay, mid, surf, pmid, pint, out):
        self._ck(self.lib.rrtmg_hip_interface_values(self.h, int(ncol), int(nlay), mid, surf, pmid, pint, out))

    @_locked
    def elementwise(self, op, n, a, out, b=None, alpha=1.0, beta=1.0):
        """op: 'axpby' out = alpha*a (+ beta*b), 'cos' out = cos(a), 'muldiv' out = a*alpha/beta, 'cosday' out = 0 where
        a >= pi/2, else cos(a)"""
        self._ck(self.lib.rrtmg_hip_elementwise(self.h, {"axpby": 0, "cos": 1, "muldiv": 2, "cosday": 3}[op], int(n), a, b, float(alpha), float(beta), out))

    @_locked
    def ab_step(self, n, x, tendencies, weights, dt, out):
        k = len(tendencies)
        f = (_vp * k)(*tendencies)
        w = (_f64 * k)(*weights)
        self._ck(self.lib.rrtmg_hip_ab_step(self.h, int(n), k, x, f, w, float(dt), out))

    @_locked
    def order_streams(self, direction):
        self._ck(self.lib.rrtmg_hip_order_streams(self.h, int(direction)))

    @_locked
    def slab_surface_device(self, ncol, ptrs, area_type, tend_ts, depth):
        """rrtmg_hip_slab_surface on device pointers: `ptrs` maps SLAB_IN names to device addresses."""
        a = SlabArgs()
        for k in SLAB_IN:
            setattr(a, k, int(ptrs[k]))
        a.area_type, a.tend_ts, a.depth = int(area_type), int(tend_ts), int(depth)
        self._ck(self.lib.rrtmg_hip_slab_surface(self.h, int(ncol), 1, C.byref(a)))

    @_locked
    def zenith_angle(self, lat_deg, lon_deg, julian_centuries, out=None, memspace=0, ncol=None):
        """Zenith angle (radians) of every column; host arrays, or device pointers with memspace=1 (then `ncol`)."""
        if memspace:
            self._ck(self.lib.rrtmg_hip_zenith_angle(self.h, int(ncol), 1, int(lat_deg), int(lon_deg), float(julian_centuries), int(out)))
            return out
        lat = np.ascontiguousarray(lat_deg, dtype=np.float64)
        lon = np.ascontiguousarray(lon_deg, dtype=np.float64)
        z = np.empty(lat.shape) if out is None else out
        self._ck(self.lib.rrtmg_hip_zenith_angle(self.h, lat.size, 0, lat.ctypes.data, lon.ctypes.data, float(julian_centuries), z.ctypes.data))
        return z

    @property
    def has_intermittent(self):
        """Whether the library exports the shortwave between radiation calls (rrtmg_hip_mean_coszen, rrtmg_hip_mean_coszen_sun,
        rrtmg_hip_scale_columns; probed by the symbols)."""
        return all(hasattr(self.lib, n) for n in ("rrtmg_hip_mean_coszen", "rrtmg_hip_mean_coszen_sun", "rrtmg_hip_scale_columns"))

    def _intermittent_entry(self, name):
        if not self.has_intermittent:
            raise RRTMGError(4, "this librrtmg_hip.so has no %s (shortwave between radiation calls)" % name)
        return getattr(self.lib, name)

    @_locked
    def mean_coszen(self, lat_deg, lon_deg, t0_centuries, t1_centuries, out_mean=None, out_fraction=None, memspace=0, ncol=None,
                    out_zenith=None, out_insolation=None, sun=None):
        """Cosine of the zenith angle averaged over the sunlit part of [t0, t1] (Julian centuries, 12 hours at the most) and
        the sunlit fraction of the interval, of every column (rrtmg_hip_mean_coszen) -> (mean, fraction).  Host arrays, or
        device pointers with memspace=1 (then `out_mean`, `out_fraction`, `ncol`).  `out_zenith`, `out_insolation`: filled as
        well where given -- acos(mean), pi/2 where the mean is 0, and mean * fraction.  `sun`: (sin_dec, cos_dec, hour angle of
        Greenwich at t0, its advance in (0, 2 pi)) in place of the two times (rrtmg_hip_mean_coszen_sun)."""
        if sun is None:
            entry, head = self._intermittent_entry("rrtmg_hip_mean_coszen"), (float(t0_centuries), float(t1_centuries))
        else:
            entry, head = self._intermittent_entry("rrtmg_hip_mean_coszen_sun"), tuple(float(v) for v in sun)
            if len(head) != 4:
                raise ValueError("sun: (sin_dec, cos_dec, hour_angle0, hour_angle_advance)")
        if memspace:
            opt = [None if p is None else int(p) for p in (out_zenith, out_insolation)]
            self._ck(entry(self.h, int(ncol), 1, int(lat_deg), int(lon_deg), *head, int(out_mean), int(out_fraction), *opt))
            return out_mean, out_fraction
        lat = np.ascontiguousarray(lat_deg, dtype=np.float64)
        lon = np.ascontiguousarray(lon_deg, dtype=np.float64)
        if lat.shape != lon.shape:
            raise ValueError("latitude and longitude must have one shape")
        mean = np.empty(lat.shape) if out_mean is None else out_mean
        frac = np.empty(lat.shape) if out_fraction is None else out_fraction
        for o in (mean, frac, out_zenith, out_insolation):
            if o is not None and not (isinstance(o, np.ndarray) and o.dtype == np.float64 and o.flags.c_contiguous and o.size == lat.size):
                raise ValueError("mean_coszen: an output is written in place: a C-contiguous float64 array of %d elements" % lat.size)
        opt = [None if o is None else o.ctypes.data for o in (out_zenith, out_insolation)]
        self._ck(entry(self.h, lat.size, 0, lat.ctypes.data, lon.ctypes.data, *head, mean.ctypes.data, frac.ctypes.data, *opt))
        return mean, frac

    @_locked
    def scale_columns(self, num, den, entries, ncol=None):
        """dst[r][c] = src[r][c] * s[c], s[c] = den[c] > 0 ? num[c] / den[c] : +0.0, for every (src, dst, rows) of `entries` --
        [rows][ncol] arrays, dst may be src -- in one launch per 16 entries (rrtmg_hip_scale_columns).  Device pointers (or
        DeviceArrays) throughout, on the context's main stream; `ncol` is needed where num is a raw pointer."""
        entry = self._intermittent_entry("rrtmg_hip_scale_columns")
        f64 = PRECISIONS["float64"]
        if ncol is None:
            ncol = int(np.prod(num.shape))
        entries = list(entries)
        if not entries:
            raise ValueError("scale_columns: no entries")
        n, d = _device_pointer(num, f64, "num"), _device_pointer(den, f64, "den")
        for i in range(0, len(entries), SCALE_MAX_ENTRIES):
            part = entries[i:i + SCALE_MAX_ENTRIES]
            table = (ScaleEntry * len(part))()
            for e, (src, dst, rows) in zip(table, part):
                e.src, e.dst, e.rows = _device_pointer(src, f64, "src"), _device_pointer(dst, f64, "dst"), int(rows)
            self._ck(entry(self.h, int(ncol), n, d, len(part), table))

    @property
    def has_lw_adjust(self):
        """Whether the library exports the longwave between radiation calls (rrtmg_hip_lw_adjust_surface; probed by the symbol)."""
        return hasattr(self.lib, "rrtmg_hip_lw_adjust_surface")

    @_locked
    def lw_adjust_surface(self, ncol, nlay, tsfc_call, tsfc_now, plev, all_sky, clear_sky=None, pressure_scale=0.0):
        """uflx' = uflx + duflx_dt * (tsfc_now - tsfc_call) by column and level, and the heating rates of the corrected net
        fluxes (rrtmg_hip_lw_adjust_surface): one launch on the longwave's stream.  `all_sky`, `clear_sky` (None: no clear-sky
        stream): (uflx, dflx, duflx_dt, uflx_out, hr_out), uflx_out may be uflx.  Device pointers (or DeviceArrays) throughout;
        `pressure_scale` as in a flux call (0: plev is in mbar)."""
        if not self.has_lw_adjust:
            raise RRTMGError(4, "this librrtmg_hip.so has no rrtmg_hip_lw_adjust_surface (longwave between radiation calls)")
        f64 = PRECISIONS["float64"]
        a = LwAdjust()
        a.struct_size, a.ncol, a.nlay, a.pressure_scale = C.sizeof(LwAdjust), int(ncol), int(nlay), float(pressure_scale)
        for name, v in (("tsfc_call", tsfc_call), ("tsfc_now", tsfc_now), ("plev", plev)):
            setattr(a, name, _device_pointer(v, f64, name))
        for stream, names in ((all_sky, ("uflx", "dflx", "duflx_dt", "uflx_out", "hr_out")), (clear_sky, ("uflxc", "dflxc", "duflxc_dt", "uflxc_out", "hrc_out"))):
            if stream is None:
                continue
            if len(stream) != 5:
                raise ValueError("lw_adjust_surface: a stream is (uflx, dflx, duflx_dt, uflx_out, hr_out)")
            for name, v in zip(names, stream):
                setattr(a, name, None if v is None else _device_pointer(v, f64, name))
        self._ck(self.lib.rrtmg_hip_lw_adjust_surface(self.h, C.byref(a)))

    def _column_call(self, entry, a, given, outs, diagnostics, memspace, ncol, nlay, nband=None):
        """The array side of a column component's call (rrtmg_hip_<entry>), behind the scalars its method has put into the struct
        `a` -> (outs, diagnostics).  `given`: the inputs the call reads, by name; `outs`: the outputs every call writes, the
        caller's array or None; `diagnostics`: True, a dict, or None; `nband`: the factor of the band-multiplied extents, from
        the entry that has such arrays.  Names, extents and types: COLUMN_ARRAYS[entry]."""
        arrays = COLUMN_ARRAYS[entry]
        IN, DIAG, dtype = arrays["IN"], arrays["DIAG"], arrays["dtype"]
        fn, names = getattr(self.lib, "rrtmg_hip_" + entry), IN + tuple(outs) + DIAG
        if memspace:
            if any(x is None for x in outs.values()) or ncol is None or nlay is None:
                raise ValueError("%s: device pointers need %s, ncol and nlay" % (entry, ", ".join(outs)))
            a.ncol, a.nlay = int(ncol), int(nlay)
            diagnostics = diagnostics if isinstance(diagnostics, dict) else {}
            for name, x in list(given.items()) + list(outs.items()) + list(diagnostics.items()):
                if name not in names:
                    raise ValueError("%s: no diagnostic %r" % (entry, name))
                setattr(a, name, _device_pointer(x, dtype[name], name))
            self._ck(fn(self.h, C.byref(a)))
            return outs, diagnostics
        mine, given = given, {n: np.ascontiguousarray(x, dtype=dtype[n]) for n, x in given.items()}
        grid = arrays["grid"]
        if grid is not None:
            shape = given[grid].shape if given[grid].ndim != 1 else (1,) + given[grid].shape
        else:
            shape = given["t"].shape if "t" in given else (given["pint"].shape[0] - 1,) + given["pint"].shape[1:]      # (no profile: the grid is pint's)
        of, axes = arrays["extent"], arrays["host_axes"]

        def extent(n):      # the caller's shape of the array `n`: the one place a name becomes a shape
            device = COLUMN_EXTENTS[of[n]](shape[0], shape[1], nband)
            return tuple(device[i] for i in axes[n]) if n in axes else device
        wrong = [n for n in given if given[n].shape != extent(n)] if len(shape) == 2 else list(given)
        if wrong and nband is not None:      # the entry with band arrays names the array and what it wants ...
            if len(shape) != 2:
                raise ValueError("%s: t must be [nlay][ncol]" % entry)
            raise ValueError("%s: %s is %s, the grid of t %s and %d bands want %s" % (entry, wrong[0], given[wrong[0]].shape, shape, nband, extent(wrong[0])))
        if wrong:                            # ... the others the group: the profiles and pint, then the columns
            profiles, cols = [n for n in IN if of[n] == LAY], [n for n in IN if of[n] == COL]
            if len(shape) != 2 or any(of[n] != COL for n in wrong):
                raise ValueError("%s: %s%s must be [nlay][ncol] arrays of one shape and pint [nlay+1][ncol]"
                                 % (entry, ", ".join(n for n in profiles if n not in arrays["optional"]), "".join(" (and %s)" % n for n in profiles if n in arrays["optional"])))
            raise ValueError("%s: %s must be %s" % (entry, " and ".join(filter(None, (", ".join(cols[:-1]), cols[-1]))), "[ncol] arrays" if len(cols) > 1 else "an [ncol] array"))
        empty = lambda n: np.empty(extent(n), dtype=dtype[n])
        outs = {n: (empty(n) if x is None else x) for n, x in outs.items()}
        if diagnostics is True:
            diagnostics = {n: empty(n) for n in DIAG}
        elif not isinstance(diagnostics, dict):
            diagnostics = {}
        for name, x in list(outs.items()) + list(diagnostics.items()):
            if name not in tuple(outs) + DIAG:
                raise ValueError("%s: no diagnostic %r" % (entry, name))
            if not (isinstance(x, np.ndarray) and x.dtype == dtype[name] and x.flags.c_contiguous and x.size == int(np.prod(extent(name)))):
                raise ValueError("%s: %s is written in place: a C-contiguous %s array of the right size" % (entry, name, dtype[name].name))
        a.nlay, a.ncol = shape
        for out, inp in arrays["in_place"]:
            if out in outs and outs[out] is mine[inp]:      # (a pair the call does not have: BucketHydrology with one layer)
                given[inp] = outs[out]
        for name, x in list(given.items()) + list(outs.items()) + list(diagnostics.items()):
            setattr(a, name, x.ctypes.data)
        self._ck(fn(self.h, C.byref(a)))
        return outs, diagnostics

    @property
    def has_dry_adjustment(self):
        """Whether the library exports the dry convective adjustment (rrtmg_hip_dry_adjustment; probed by the symbol)."""
        return hasattr(self.lib, "rrtmg_hip_dry_adjustment")

    @_locked
    def dry_adjustment(self, t, q, pmid, pint, constants, t_out=None, q_out=None, mixed_top=None, memspace=0, ncol=None, nlay=None):
        """climt's DryConvectiveAdjustment by column (rrtmg_hip_dry_adjustment) -> (t_out, q_out, mixed_top).  `constants`: cpd,
        cvap, rd, rv and pref, pref in the units of the pressures.  Host arrays t, q, pmid [nlay][ncol] and pint [nlay+1][ncol]
        (outputs are allocated unless given; t_out may be t, q_out may be q), or device pointers (or DeviceArrays) with
        memspace=1 -- then `t_out`, `q_out`, `ncol` and `nlay`, one launch on the main stream; `mixed_top` (int32 [ncol]) is
        written where given, and with host arrays always."""
        if not self.has_dry_adjustment:
            raise RRTMGError(4, "this librrtmg_hip.so has no rrtmg_hip_dry_adjustment (dry convective adjustment)")
        a = DryAdjust()
        a.struct_size, a.memspace = C.sizeof(DryAdjust), 1 if memspace else 0
        for n in DRY_ADJUST_CONSTANTS:
            setattr(a, n, float(constants[n]))
        diagnostics = True if not memspace and mixed_top is None else {} if mixed_top is None else dict(mixed_top=mixed_top)
        outs, diagnostics = self._column_call("dry_adjustment", a, dict(t=t, q=q, pmid=pmid, pint=pint), dict(t_out=t_out, q_out=q_out), diagnostics,
                                              memspace, ncol, nlay)
        return outs["t_out"], outs["q_out"], diagnostics.get("mixed_top")

    @property
    def has_boundary_layer(self):
        """Whether the library exports the simple boundary layer (rrtmg_hip_boundary_layer; probed by the symbol)."""
        return hasattr(self.lib, "rrtmg_hip_boundary_layer")

    @_locked
    def boundary_layer(self, t, q, u, v, pmid, pint, ps, ts, qs, dt, constants, flux_mode, sh_in=None, lh_in=None, t_out=None, q_out=None,
                       u_out=None, v_out=None, diagnostics=True, pressure_scale=1.0, ps_scale=1.0, memspace=0, ncol=None, nlay=None):
        """climt's SimpleBoundaryLayer by column (rrtmg_hip_boundary_layer) -> (t_out, q_out, u_out, v_out, diagnostics).
        `constants`: rd, cp, g, lv, karman, z0, fb, p0, ric; `flux_mode` 0 (no surface exchange), 1 (bulk) or 2 (external: the
        prescribed `sh_in`, `lh_in`); `pressure_scale`, `ps_scale`: Pa per unit of pmid / pint and of ps.  Host arrays t, q, u, v,
        pmid [nlay][ncol], pint [nlay+1][ncol], ps, ts, qs [ncol] (outputs are allocated unless given; each may be its own input),
        `diagnostics` True: a dict of the five [ncol] arrays stress_north, stress_east, height, sh_out, lh_out (False or None:
        none are asked for; a dict: those it names are written).  Or device pointers (or DeviceArrays) with memspace=1 -- then
        the four outputs, `ncol` and `nlay`, and `diagnostics` a dict of device pointers or None; one launch on the main stream."""
        if not self.has_boundary_layer:
            raise RRTMGError(4, "this librrtmg_hip.so has no rrtmg_hip_boundary_layer (simple boundary layer)")
        a = BoundaryLayer()
        a.struct_size, a.memspace, a.flux_mode, a.dt = C.sizeof(BoundaryLayer), 1 if memspace else 0, int(flux_mode), float(dt)
        a.pressure_scale, a.ps_scale = float(pressure_scale), float(ps_scale)
        for n in BOUNDARY_LAYER_CONSTANTS:
            setattr(a, n, float(constants[n]))
        external = int(flux_mode) == 2
        if external and (sh_in is None or lh_in is None):
            raise ValueError("boundary_layer: flux_mode 2 (external) needs sh_in and lh_in")
        given = dict(t=t, q=q, u=u, v=v, pmid=pmid, pint=pint, ps=ps, ts=ts, qs=qs)
        if external:
            given.update(sh_in=sh_in, lh_in=lh_in)
        outs, diagnostics = self._column_call("boundary_layer", a, given, dict(t_out=t_out, q_out=q_out, u_out=u_out, v_out=v_out), diagnostics,
                                              memspace, ncol, nlay)
        return outs["t_out"], outs["q_out"], outs["u_out"], outs["v_out"], diagnostics

    @property
    def has_emanuel_convection(self):
        """Whether the library exports the Emanuel convection scheme (rrtmg_hip_emanuel_convection; probed by the symbol)."""
        return hasattr(self.lib, "rrtmg_hip_emanuel_convection")

    @_locked
    def emanuel_convection(self, t, q, u, v, pmid, pint, cbmf, dt, parameters, constants, qs=None, ft=None, fq=None, fu=None, fv=None, cbmf_out=None,
                           diagnostics=True, pressure_scale=1.0, memspace=0, ncol=None, nlay=None):
        """climt's EmanuelConvection by column (rrtmg_hip_emanuel_convection) -> (ft, fq, fu, fv, cbmf_out, diagnostics).
        `parameters`: minorig and the fifteen scheme parameters (_lib.EMANUEL_PARAMETERS); `constants`: cpd, cpv, cl, rv, rd, lv0, g,
        rowl; `pressure_scale`: hPa per unit of pmid / pint; `qs` None: the kernel forms the reference's bolton_q_sat.  Host arrays
        t, q, u, v, pmid [nlay][ncol], pint [nlay+1][ncol], cbmf [ncol] (outputs are allocated unless given; cbmf_out may be cbmf);
        `diagnostics` True: a dict of precip, wd, tprime, qprime, cape [ncol], iflag (int32) [ncol] and ft_per_day [nlay][ncol]
        (False or None: none are asked for; a dict: those it names are written).  Or device pointers (or DeviceArrays) with
        memspace=1 -- then the four tendencies, cbmf_out, `ncol` and `nlay`, and `diagnostics` a dict of device pointers or None; the
        launches go to the main stream."""
        if not self.has_emanuel_convection:
            raise RRTMGError(4, "this librrtmg_hip.so has no rrtmg_hip_emanuel_convection (Emanuel convection scheme)")
        a = Emanuel()
        a.struct_size, a.memspace, a.dt, a.pressure_scale = C.sizeof(Emanuel), 1 if memspace else 0, float(dt), float(pressure_scale)
        a.minorig = int(parameters["minorig"])
        for n in EMANUEL_PARAMETERS:
            setattr(a, n, float(parameters[n]))
        for n in EMANUEL_CONSTANTS:
            setattr(a, n, float(constants[n]))
        given = dict(t=t, q=q, u=u, v=v, pmid=pmid, pint=pint, cbmf=cbmf)
        if qs is not None:
            given["qs"] = qs
        outs, diagnostics = self._column_call("emanuel_convection", a, given, dict(ft=ft, fq=fq, fu=fu, fv=fv, cbmf_out=cbmf_out), diagnostics,
                                              memspace, ncol, nlay)
        return outs["ft"], outs["fq"], outs["fu"], outs["fv"], outs["cbmf_out"], diagnostics

    @property
    def has_simple_physics(self):
        """Whether the library exports the simple physics package (rrtmg_hip_simple_physics; probed by the symbol)."""
        return hasattr(self.lib, "rrtmg_hip_simple_physics")

    @_locked
    def simple_physics(self, t, q, u, v, pmid, pint, ps, dt, constants, switches, ts=None, qsurf=None, lat=None, t_out=None, q_out=None,
                       u_out=None, v_out=None, diagnostics=True, pressure_scale=1.0, ps_scale=1.0, memspace=0, ncol=None, nlay=None):
        """climt's SimplePhysics by column (rrtmg_hip_simple_physics) -> (t_out, q_out, u_out, v_out, diagnostics).
        `constants`: g, cpair, rair, latvap, rh2o, radius, omega, rhow, pbltop, pblconst, c_heat, cd0, cd1, cm; `switches`: a dict of
        do_lsc, do_pbl, do_surf_flux, use_ts_ext, use_qsurf_ext, test, clamp_latent_heat_flux (a missing one is 0; do_pbl without
        do_surf_flux is refused by the library); `ts`, `qsurf`, `lat` are needed where the switches have them read and ignored
        otherwise; `pressure_scale`, `ps_scale`: Pa per unit of pmid / pint and of ps.  Host arrays t, q, u, v, pmid [nlay][ncol],
        pint [nlay+1][ncol], ps, ts, qsurf, lat [ncol] (outputs are allocated unless given; each may be its own input),
        `diagnostics` True: a dict of the three [ncol] arrays precl, sh_out, lh_out (False or None: none are asked for; a dict:
        those it names are written).  Or device pointers (or DeviceArrays) with memspace=1 -- then the four outputs, `ncol` and
        `nlay`, and `diagnostics` a dict of device pointers or None; one launch on the main stream."""
        if not self.has_simple_physics:
            raise RRTMGError(4, "this librrtmg_hip.so has no rrtmg_hip_simple_physics (simple physics package)")
        a = SimplePhysics()
        a.struct_size, a.memspace, a.dt = C.sizeof(SimplePhysics), 1 if memspace else 0, float(dt)
        a.pressure_scale, a.ps_scale = float(pressure_scale), float(ps_scale)
        for n in SIMPLE_PHYSICS_CONSTANTS:
            setattr(a, n, float(constants[n]))
        for n in switches:
            if n not in SIMPLE_PHYSICS_SWITCHES:
                raise ValueError("simple_physics: no switch %r" % n)
            setattr(a, n, int(switches[n]))
        given = dict(t=t, q=q, u=u, v=v, pmid=pmid, pint=pint, ps=ps)
        given.update({n: x for n, x in (("ts", ts), ("qsurf", qsurf), ("lat", lat)) if x is not None})
        outs, diagnostics = self._column_call("simple_physics", a, given, dict(t_out=t_out, q_out=q_out, u_out=u_out, v_out=v_out), diagnostics,
                                              memspace, ncol, nlay)
        return outs["t_out"], outs["q_out"], outs["u_out"], outs["v_out"], diagnostics

    @property
    def has_gray_radiation(self):
        """Whether the library exports the gray radiation path (rrtmg_hip_frierson_optical_depth, rrtmg_hip_gray_longwave and
        rrtmg_hip_grid_scale_condensation; probed by the symbol)."""
        return all(hasattr(self.lib, "rrtmg_hip_" + n) for n in ("frierson_optical_depth", "gray_longwave", "grid_scale_condensation"))

    def _need_gray_radiation(self, entry):
        if not self.has_gray_radiation:
            raise RRTMGError(4, "this librrtmg_hip.so has no rrtmg_hip_%s (gray radiation path)" % entry)

    @_locked
    def frierson_optical_depth(self, pint, ps, lat, parameters, tau=None, pressure_scale=1.0, ps_scale=1.0, memspace=0, ncol=None, nlay=None):
        """climt's Frierson06LongwaveOpticalDepth by column (rrtmg_hip_frierson_optical_depth) -> tau [nlay+1][ncol].
        `parameters`: tau0e, tau0p, fl; `pressure_scale`, `ps_scale`: Pa per unit of pint and of ps (only their ratio enters).
        Host arrays pint [nlay+1][ncol], ps, lat [ncol] (lat in degrees north; tau is allocated unless given), or device pointers
        (or DeviceArrays) with memspace=1 -- then `tau`, `ncol` and `nlay`; one launch on the main stream."""
        self._need_gray_radiation("frierson_optical_depth")
        a = FriersonOpticalDepth()
        a.struct_size, a.memspace = C.sizeof(FriersonOpticalDepth), 1 if memspace else 0
        a.pressure_scale, a.ps_scale = float(pressure_scale), float(ps_scale)
        for n in FRIERSON_SCALARS:
            setattr(a, n, float(parameters[n]))
        outs, _ = self._column_call("frierson_optical_depth", a, dict(pint=pint, ps=ps, lat=lat), dict(tau=tau), None, memspace, ncol, nlay)
        return outs["tau"]

    @_locked
    def gray_longwave(self, t, tsfc, pint, constants, tau=None, ps=None, lat=None, frierson=None, up=None, dn=None, tend=None, diagnostics=True,
                      pressure_scale=1.0, ps_scale=1.0, memspace=0, ncol=None, nlay=None):
        """climt's GrayLongwaveRadiation by column (rrtmg_hip_gray_longwave) -> (up, dn, tend, diagnostics).  `constants`:
        sigma_sb, g, cpd.  `frierson` None: `tau` [nlay+1][ncol] is read.  `frierson` a dict of tau0e, tau0p, fl: the fused call --
        the optical depth is formed inside the sweep from pint, `ps` and `lat` (degrees north) and `tau` is ignored.
        `pressure_scale`, `ps_scale`: Pa per unit of pint and of ps.  Host arrays t [nlay][ncol], tsfc [ncol], pint [nlay+1][ncol]
        (outputs are allocated unless given), `diagnostics` True: a dict of hr [nlay][ncol] (K/day) and, with `frierson`, tau_out
        [nlay+1][ncol] (False or None: none are asked for; a dict: those it names are written).  Or device pointers (or
        DeviceArrays) with memspace=1 -- then the three outputs, `ncol` and `nlay`, and `diagnostics` a dict of device pointers
        or None; one launch on the main stream."""
        self._need_gray_radiation("gray_longwave")
        a = GrayLongwave()
        a.struct_size, a.memspace, a.frierson = C.sizeof(GrayLongwave), 1 if memspace else 0, 0 if frierson is None else 1
        a.pressure_scale, a.ps_scale = float(pressure_scale), float(ps_scale)
        for n in GRAY_LONGWAVE_CONSTANTS:
            setattr(a, n, float(constants[n]))
        given = dict(t=t, tsfc=tsfc, pint=pint)
        if frierson is None:
            if tau is None:
                raise ValueError("gray_longwave: tau is needed without frierson")
            given["tau"] = tau
        else:
            if ps is None or lat is None:
                raise ValueError("gray_longwave: frierson needs ps and lat")
            for n in FRIERSON_SCALARS:
                setattr(a, n, float(frierson[n]))
            given.update(ps=ps, lat=lat)
        if diagnostics is True and not memspace:      # (the depth is a diagnostic of the fused call only)
            shape = np.shape(t)
            diagnostics = dict(hr=np.empty(shape))
            if frierson is not None:
                diagnostics["tau_out"] = np.empty((shape[0] + 1, shape[1]))
        outs, diagnostics = self._column_call("gray_longwave", a, given, dict(up=up, dn=dn, tend=tend), diagnostics, memspace, ncol, nlay)
        return outs["up"], outs["dn"], outs["tend"], diagnostics

    @_locked
    def grid_scale_condensation(self, t, q, pmid, pint, constants, t_out=None, q_out=None, diagnostics=True, pressure_scale=1.0, memspace=0,
                                ncol=None, nlay=None):
        """climt's GridScaleCondensation by column (rrtmg_hip_grid_scale_condensation) -> (t_out, q_out, diagnostics).
        `constants`: cpd, lv, rd, rh2o, g, rhow; `pressure_scale`: Pa per unit of pmid / pint.  Host arrays t, q, pmid [nlay][ncol],
        pint [nlay+1][ncol] (outputs are allocated unless given; each may be its own input), `diagnostics` True: a dict of the
        [ncol] array precip (False or None: not asked for; a dict: written where named).  Or device pointers (or DeviceArrays)
        with memspace=1 -- then the two outputs, `ncol` and `nlay`, and `diagnostics` a dict of device pointers or None; one
        launch on the main stream."""
        self._need_gray_radiation("grid_scale_condensation")
        a = GridScaleCondensation()
        a.struct_size, a.memspace, a.pressure_scale = C.sizeof(GridScaleCondensation), 1 if memspace else 0, float(pressure_scale)
        for n in GRID_SCALE_CONDENSATION_CONSTANTS:
            setattr(a, n, float(constants[n]))
        outs, diagnostics = self._column_call("grid_scale_condensation", a, dict(t=t, q=q, pmid=pmid, pint=pint), dict(t_out=t_out, q_out=q_out),
                                              diagnostics, memspace, ncol, nlay)
        return outs["t_out"], outs["q_out"], diagnostics

    @property
    def has_cork_longwave(self):
        """Whether the library exports the table-driven correlated-k longwave (rrtmg_hip_cork_longwave; probed by the symbol)."""
        return hasattr(self.lib, "rrtmg_hip_cork_longwave")

    def _need_cork_longwave(self):
        if not self.has_cork_longwave:
            raise RRTMGError(4, "this librrtmg_hip.so has no rrtmg_hip_cork_longwave (correlated-k longwave)")

    @_locked
    def cork_table_create(self, k, weights, planck, t_grid, p_grid_log, x_grid_log=None, x_clip=None, c_grid_log=None, c_clip=None, log_cont=None):
        """Upload a correlated-k table (rrtmg_hip_cork_table_create) -> the handle, owned by this context.  `k` float32 or float64
        in the reference's layout (ngas, nband, ngpt, nT, nP[, nX[, nC]]); the other arrays are taken as float64.  The shapes
        are checked against k's here and the grids by the library, before anything is uploaded."""
        self._need_cork_longwave()
        sized = lambda *axes: lambda n: tuple(n[a] for a in axes)
        return self._cork_table(CorkTableDesc, "rrtmg_hip_cork_table_create", "cork table", {5: "5 (T, p)", 6: "6 (+ H2O)", 7: "7 (+ CO2)"}, k, [
            ("weights", "gpoint_weights", weights, sized("nband", "ngpt"), True), ("planck", "planck_fraction", planck, sized("nband", "ngpt", "nT"), True),
            ("t_grid", "temperature_grid", t_grid, sized("nT"), True), ("p_grid_log", "pressure_grid_log", p_grid_log, sized("nP"), True),
            ("x_grid_log", "h2o_vmr_grid", x_grid_log, sized("nX"), "nX"), ("c_grid_log", "co2_vmr_grid", c_grid_log, sized("nC"), "nC"),
            ("log_cont", "continuum_kappa", log_cont, sized("nband", "nT", "nP", "nX"), False)], dict(x_clip=x_clip, c_clip=c_clip))

    def _cork_table(self, desc_type, entry, label, ranks, k, arrays, clips, keep_type=()):
        """The array side of both table uploads -> the handle.  `ranks`: {rank of k: how the message names it}; `arrays`: (member of
        the description, the table's name for it, the array or None, sizes -> shape, needed: True, False (optional) or the size
        that asks for it); `keep_type`: the members kept float32 where they come so (every other array is taken as float64).
        The shapes are checked against k's here and the grids by the library, before anything is uploaded."""
        k = np.ascontiguousarray(k)
        if k.dtype not in (np.float32, np.float64):
            k = k.astype(np.float64)
        if k.ndim not in ranks:
            names = list(ranks.values())
            raise ValueError("%s: k_coefficients has rank %d, not %s" % (label, k.ndim, " or ".join([", ".join(names[:-1]), names[-1]])))
        n = dict(zip(CORK_TABLE_SIZES, tuple(k.shape) + (0,) * (7 - k.ndim)))
        d = desc_type()
        d.struct_size, d.k_is_f32, d.k = C.sizeof(desc_type), 1 if k.dtype == np.float32 else 0, k.ctypes.data
        for name, v in n.items():
            setattr(d, name, int(v))
        keep = [k]
        for member, name, x, shape, needed in arrays:
            if x is not None:
                x = np.ascontiguousarray(x)
                if not (member in keep_type and x.dtype == np.float32):
                    x = np.ascontiguousarray(x, dtype=np.float64)
            if isinstance(needed, str):
                needed = n[needed] > 0
                x = x if needed else None      # (an axis k does not have: its grid is not read)
            if (x is None and needed) or (x is not None and x.shape != shape(n)):
                raise ValueError("%s: %s is %s, k_coefficients %s wants %s" % (label, name, "missing" if x is None else x.shape, k.shape, shape(n)))
            keep.append(x)
            setattr(d, member, None if x is None else x.ctypes.data)
            if member in keep_type:
                setattr(d, keep_type[member], 1 if x.dtype == np.float32 else 0)
        for name, clip in clips.items():
            if clip is not None:
                getattr(d, name)[0], getattr(d, name)[1] = float(clip[0]), float(clip[1])
        handle = _vp()
        self._ck(getattr(self.lib, entry)(self.h, C.byref(d), C.byref(handle)))
        return handle.value

    @_locked
    def cork_table_destroy(self, handle):
        """Free a table of this context (rrtmg_hip_cork_table_destroy); what is left goes with the context."""
        self._need_cork_longwave()
        self._ck(self.lib.rrtmg_hip_cork_table_destroy(self.h, handle))

    @_locked
    def cork_longwave(self, table, nband, t, pmid, pint, tsfc, emis, constants, gas_rule, gases=(), gas_scale=(), taucld=None, up=None, dn=None, tend=None,
                      diagnostics=True, pressure_scale=1.0, memspace=0, ncol=None, nlay=None):
        """climt's CorkLongwaveRadiation (correlated_k, additive overlap) by column (rrtmg_hip_cork_longwave) -> (up, dn, tend,
        diagnostics).  `table`: a handle of cork_table_create, `nband` its bands; `constants`: m_h2o, sigma_sb, g, cpd, diffusivity;
        `gas_rule` 0 (fully premixed), 1 (premixed background: gases = (specific humidity[, CO2 mole fraction])) or 2 (per gas:
        one array per gas of the table, `gas_scale` its M_gas / M_dry or 1.0); a gas may be None where the library does not read
        it.  Host arrays t, pmid [nlay][ncol], pint [nlay+1][ncol], tsfc [ncol], emis [nband][ncol], taucld [nlay][ncol][nband] or
        None (outputs are allocated unless given); `diagnostics` True: a dict of hr [nlay][ncol], up_band, dn_band
        [nband][nlay+1][ncol], tau_band, trans_band, hr_band [nband][nlay][ncol] (False or None: none; a dict: those it names are
        written).  Or device pointers (or DeviceArrays) with memspace=1 -- then the three outputs, `ncol` and `nlay`, and
        `diagnostics` a dict of device pointers or None; two launches on the main stream."""
        self._need_cork_longwave()
        if len(gases) > CORK_MAX_GAS or len(gas_scale) > CORK_MAX_GAS:
            raise ValueError("cork_longwave: at most %d gases" % CORK_MAX_GAS)
        a = CorkLongwave()
        a.struct_size, a.memspace, a.gas_rule, a.table = C.sizeof(CorkLongwave), 1 if memspace else 0, int(gas_rule), table
        a.pressure_scale = float(pressure_scale)
        for n in CORK_LONGWAVE_CONSTANTS:
            setattr(a, n, float(constants[n]))
        for i in range(CORK_MAX_GAS):
            a.gas_scale[i] = float(gas_scale[i]) if i < len(gas_scale) else 1.0
        given = dict(t=t, pmid=pmid, pint=pint, tsfc=tsfc, emis=emis)
        if taucld is not None:
            given["taucld"] = taucld
        given.update({"gas%d" % i: x for i, x in enumerate(gases) if x is not None})
        outs, diagnostics = self._column_call("cork_longwave", a, given, dict(up=up, dn=dn, tend=tend), diagnostics, memspace, ncol, nlay, nband=int(nband))
        return outs["up"], outs["dn"], outs["tend"], diagnostics

    @property
    def has_cork_shortwave(self):
        """Whether the library exports the table-driven correlated-k shortwave (rrtmg_hip_cork_shortwave; probed by the symbol)."""
        return hasattr(self.lib, "rrtmg_hip_cork_shortwave") and hasattr(self.lib, "rrtmg_hip_cork_sw_table_create")

    def _need_cork_shortwave(self):
        if not self.has_cork_shortwave:
            raise RRTMGError(4, "this librrtmg_hip.so has no rrtmg_hip_cork_shortwave (correlated-k shortwave)")

    @_locked
    def cork_sw_table_create(self, k, weights, solar_source, t_grid, p_grid_log, x_grid_log=None, x_clip=None, log_cont=None, rayleigh=None):
        """Upload a correlated-k shortwave table (rrtmg_hip_cork_sw_table_create) -> the handle, owned by this context and freed
        by cork_table_destroy.  `k` float32 or float64 in the reference's layout (ngas, nband, ngpt, nT, nP[, nX]) -- a rank-7
        table is refused, the reference's shortwave has no CO2 axis; `solar_source` (nband, ngpt) float32 or float64 -- the type
        the earth-sun factor is multiplied in; `rayleigh` (nband,) or None; the other arrays are taken as float64."""
        self._need_cork_shortwave()
        sized = lambda *axes: lambda n: tuple(n[a] for a in axes)
        return self._cork_table(CorkSwTableDesc, "rrtmg_hip_cork_sw_table_create", "cork shortwave table", {5: "5 (T, p)", 6: "6 (+ H2O)"}, k, [
            ("weights", "gpoint_weights", weights, sized("nband", "ngpt"), True), ("solar_source", "solar_source_per_gpoint", solar_source, sized("nband", "ngpt"), True),
            ("t_grid", "temperature_grid", t_grid, sized("nT"), True), ("p_grid_log", "pressure_grid_log", p_grid_log, sized("nP"), True),
            ("x_grid_log", "h2o_vmr_grid", x_grid_log, sized("nX"), "nX"), ("log_cont", "continuum_kappa", log_cont, sized("nband", "nT", "nP", "nX"), False),
            ("rayleigh", "rayleigh_coefficient", rayleigh, sized("nband"), False)], dict(x_clip=x_clip), keep_type={"solar_source": "solar_is_f32"})

    @_locked
    def cork_shortwave(self, table, nband, t, pmid, pint, zenith, albedo, earth_sun, constants, gas_rule, gases=(), gas_scale=(), cloud=None, up=None, dn=None,
                       tend=None, diagnostics=True, pressure_scale=1.0, max_chunk_cols=0, memspace=0, ncol=None, nlay=None):
        """climt's CorkShortwaveRadiation (correlated_k, additive overlap) by column (rrtmg_hip_cork_shortwave) -> (up, dn, tend,
        diagnostics).  `table`: a handle of cork_sw_table_create, `nband` its bands; `constants`: m_h2o, g, cpd; `gas_rule`,
        `gases`, `gas_scale` as in cork_longwave.  Host arrays t, pmid [nlay][ncol], pint [nlay+1][ncol], zenith (radians), albedo,
        earth_sun [ncol] (the FIRST column's factor scales every column, as in the reference), `cloud` None or (taucld, ssacld,
        asycld), each [nlay][ncol][nband] (outputs are allocated unless given); `diagnostics` True: a dict of hr [nlay][ncol],
        up_band, dn_band [nband][nlay+1][ncol], tau_band, hr_band [nband][nlay][ncol] (False or None: none; a dict: those it
        names are written).  `max_chunk_cols`: 0, or the most columns the library runs per chunk of its work space.  Or device
        pointers (or DeviceArrays) with memspace=1 -- then the three outputs, `ncol` and `nlay`, and `diagnostics` a dict of
        device pointers or None; a launch per chunk and the band reduction on the main stream."""
        self._need_cork_shortwave()
        if len(gases) > CORK_MAX_GAS or len(gas_scale) > CORK_MAX_GAS:
            raise ValueError("cork_shortwave: at most %d gases" % CORK_MAX_GAS)
        a = CorkShortwave()
        a.struct_size, a.memspace, a.gas_rule, a.table = C.sizeof(CorkShortwave), 1 if memspace else 0, int(gas_rule), table
        a.pressure_scale, a.max_chunk_cols = float(pressure_scale), int(max_chunk_cols)
        for n in CORK_SHORTWAVE_CONSTANTS:
            setattr(a, n, float(constants[n]))
        for i in range(CORK_MAX_GAS):
            a.gas_scale[i] = float(gas_scale[i]) if i < len(gas_scale) else 1.0
        given = dict(t=t, pmid=pmid, pint=pint, zenith=zenith, albedo=albedo, earth_sun=earth_sun)
        if cloud is not None:
            if len(cloud) != 3:
                raise ValueError("cork_shortwave: cloud is (taucld, ssacld, asycld)")
            given.update({n: x for n, x in zip(CORK_SHORTWAVE_CLOUD, cloud) if x is not None})
        given.update({"gas%d" % i: x for i, x in enumerate(gases) if x is not None})
        outs, diagnostics = self._column_call("cork_shortwave", a, given, dict(up=up, dn=dn, tend=tend), diagnostics, memspace, ncol, nlay, nband=int(nband))
        return outs["up"], outs["dn"], outs["tend"], diagnostics

    @property
    def has_surface_ice(self):
        """Whether the library exports the snow/ice column of SeaIce and LandIce (rrtmg_hip_surface_ice; probed by the symbol)."""
        return hasattr(self.lib, "rrtmg_hip_surface_ice")

    @_locked
    def surface_ice(self, kind, t, height, thick, snow, base, fluxes, area_type, dt, constants, t_out=None, height_out=None, thick_out=None,
                    snow_out=None, tsfc_out=None, base_flux_out=None, diagnostics=True, memspace=0, ncol=None, nlay=None):
        """climt's SeaIce (`kind` 0) and LandIce (`kind` 1) by column (rrtmg_hip_surface_ice) -> (outputs, diagnostics): two
        dicts, by the names of SURFACE_ICE_OUT and SURFACE_ICE_DIAG.  `base`: the ocean heat flux (kind 0) or the soil surface
        temperature (kind 1); `fluxes`: a dict of the six [ncol] parts of the net flux (SURFACE_ICE_FLUXES; the radiative ones are
        the surface row of the flux arrays); `area_type`: int32 codes (slab_surface.AREA_MAP); `constants`:
        SURFACE_ICE_CONSTANTS.  Host arrays t, height [nlay][ncol] (nlay: the ice interface levels, at least 3) and [ncol] arrays
        (outputs are allocated unless given; t_out, height_out, thick_out, snow_out and, for kind 0, base_flux_out may be their own
        inputs), `diagnostics` True: cond_flux, albedo and flags (False or None: none; a dict: those it names).  Or device
        pointers (or DeviceArrays) with memspace=1 -- then the six outputs, `ncol` and `nlay`, and `diagnostics` a dict of
        device pointers or None; one launch on the main stream."""
        if not self.has_surface_ice:
            raise RRTMGError(4, "this librrtmg_hip.so has no rrtmg_hip_surface_ice (sea ice and land ice)")
        a = SurfaceIce()
        a.struct_size, a.memspace, a.kind, a.dt = C.sizeof(SurfaceIce), 1 if memspace else 0, int(kind), float(dt)
        for n in SURFACE_ICE_CONSTANTS:
            setattr(a, n, float(constants[n]))
        given = dict(t=t, height=height, thick=thick, snow=snow, base=base, area_type=area_type)
        given.update({n: fluxes[n] for n in SURFACE_ICE_FLUXES})
        return self._column_call("surface_ice", a, given, dict(t_out=t_out, height_out=height_out, thick_out=thick_out, snow_out=snow_out,
                                                               tsfc_out=tsfc_out, base_flux_out=base_flux_out), diagnostics, memspace, ncol, nlay)

    @property
    def has_bucket_hydrology(self):
        """Whether the library exports the land surface of BucketHydrology (rrtmg_hip_bucket_hydrology; probed by the symbol)."""
        return hasattr(self.lib, "rrtmg_hip_bucket_hydrology")

    @_locked
    def bucket_hydrology(self, layers, arrays, dt, scalars, outs=None, diagnostics=True, pressure_scale=1.0, memspace=0, ncol=None):
        """climt's BucketHydrology by column (rrtmg_hip_bucket_hydrology) -> (outputs, diagnostics): two dicts, by the names of
        BUCKET_HYDROLOGY_OUT and BUCKET_HYDROLOGY_DIAG.  `layers`: 1 or 2; `arrays`: a dict of the [ncol] inputs
        (BUCKET_HYDROLOGY_IN: the lowest model level of the atmosphere, the surface level of the four radiative fluxes, the
        surface and soil columns; the two deep ones with layers 2 only); `scalars`: BUCKET_HYDROLOGY_SCALARS, tau_drain None for
        no drainage; `pressure_scale`: Pa per unit of p_air.  Host arrays (`outs`: a dict of the caller's output arrays, each
        allocated unless given; each may be its own input), `diagnostics` True: precip, lh, sh, evaporation and, with layers 2,
        runoff and deep_fraction (False or None: none; a dict: those it names).  Or device pointers (or DeviceArrays) with
        memspace=1 -- then every output of the layer count, `ncol`, and `diagnostics` a dict of device pointers or None; one
        launch on the main stream."""
        if not self.has_bucket_hydrology:
            raise RRTMGError(4, "this librrtmg_hip.so has no rrtmg_hip_bucket_hydrology (land surface: BucketHydrology)")
        a = BucketHydrology()
        a.struct_size, a.memspace, a.layers, a.dt, a.pressure_scale = C.sizeof(BucketHydrology), 1 if memspace else 0, int(layers), float(dt), float(pressure_scale)
        a.has_drain = 0 if scalars.get("tau_drain") is None else 1
        for n in BUCKET_HYDROLOGY_SCALARS:
            setattr(a, n, 0.0 if scalars.get(n) is None else float(scalars[n]))
        deep = int(layers) == 2
        skip = () if deep else BUCKET_HYDROLOGY_DEEP
        given = {n: arrays[n] for n in BUCKET_HYDROLOGY_IN if n not in skip}
        outs = dict(outs or {})
        outs = {n: outs.get(n) for n in BUCKET_HYDROLOGY_OUT if n[:-4] not in skip}
        if diagnostics is True and not memspace:
            shape = np.shape(arrays["ts"])
            diagnostics = {n: np.empty(shape) for n in BUCKET_HYDROLOGY_DIAG[:6 if deep else 4]}
        return self._column_call("bucket_hydrology", a, given, outs, diagnostics, memspace, ncol, 1)

    @property
    def has_second_best(self):
        """Whether the library exports the land surface of SecondBEST (rrtmg_hip_second_best; probed by the symbol)."""
        return hasattr(self.lib, "rrtmg_hip_second_best")

    @_locked
    def second_best(self, arrays, dt, constants, outs=None, diagnostics=True, pressure_scale=1.0, ps_scale=1.0, memspace=0, ncol=None, nlay=None):
        """climt's SecondBEST with its default processes by column (rrtmg_hip_second_best) -> (outputs, diagnostics): two dicts,
        by the names of SECOND_BEST_OUT and SECOND_BEST_DIAG.  `arrays`: a dict of the inputs (SECOND_BEST_IN): t_soil, x_w, x_i,
        height [nlay][ncol] (nlay: the soil interface levels, at least 2; node 0 is the bottom), the others [ncol] (the lowest model
        level of the atmosphere, the surface level of the four radiative fluxes), area_type int32 codes (slab_surface.AREA_MAP);
        `constants`: SECOND_BEST_CONSTANTS; `pressure_scale`, `ps_scale`: Pa per unit of p_air and of ps.  Host arrays (`outs`: a
        dict of the caller's output arrays, each allocated unless given; each may be its own input), `diagnostics` True: all of
        SECOND_BEST_DIAG (False or None: none; a dict: those it names).  Or device pointers (or DeviceArrays) with memspace=1 --
        then the five outputs, `ncol` and `nlay`, and `diagnostics` a dict of device pointers or None; one launch on the main
        stream."""
        if not self.has_second_best:
            raise RRTMGError(4, "this librrtmg_hip.so has no rrtmg_hip_second_best (land surface: SecondBEST)")
        a = SecondBest()
        a.struct_size, a.memspace, a.dt = C.sizeof(SecondBest), 1 if memspace else 0, float(dt)
        a.pressure_scale, a.ps_scale = float(pressure_scale), float(ps_scale)
        for n in SECOND_BEST_CONSTANTS:
            setattr(a, n, float(constants[n]))
        outs = dict(outs or {})
        return self._column_call("second_best", a, {n: arrays[n] for n in SECOND_BEST_IN}, {n: outs.get(n) for n in SECOND_BEST_OUT}, diagnostics,
                                 memspace, ncol, nlay)

    @_locked
    def solar_insolation(self, lat, lon, sin_delta, cos_delta, fractional_day, irradiance):
        """(zenith angle, insolation) of every column (host arrays): per-column part of BergerSolarInsolation."""
        lat = np.ascontiguousarray(lat, dtype=np.float64)
        lon = np.ascontiguousarray(lon, dtype=np.float64)
        z, s = np.empty(lat.shape), np.empty(lat.shape)
        self._ck(self.lib.rrtmg_hip_solar_insolation(self.h, lat.size, 0, lat.ctypes.data, lon.ctypes.data, float(sin_delta), float(cos_delta),
                                                     float(fractional_day), float(irradiance), z.ctypes.data, s.ctypes.data))
        return z, s

    @_locked
    def slab_surface(self, area_type, **arrays):
        """Kernel of climt SlabSurface on host arrays: -> (surface temperature tendency, slab depth).  `arrays`: SLAB_IN."""
        a = SlabArgs()
        keep = [np.ascontiguousarray(area_type, dtype=np.int32)]
        a.area_type = keep[0].ctypes.data
        n = keep[0].size
        for k in SLAB_IN:
            v = np.ascontiguousarray(arrays[k], dtype=np.float64)
            assert v.size == n, k
            keep.append(v)
            setattr(a, k, v.ctypes.data)
        tend, depth = np.empty(n), np.empty(n)
        a.tend_ts, a.depth = tend.ctypes.data, depth.ctypes.data
        self._ck(self.lib.rrtmg_hip_slab_surface(self.h, n, 0, C.byref(a)))
        return tend, depth

    @_locked
    def set_deferred(self, on=True):
        """Device-resident (memspace=1) calls return after enqueueing; SW and LW overlap on two streams.  Returns the
        previous setting, so that whoever switches it on for the lifetime of an object can restore it (the context is
        shared: a memspace=1 caller that expects per-call synchronisation and error checks must get them back)."""
        prev = self.deferred
        self._ck(self.lib.rrtmg_hip_set_deferred(self.h, 1 if on else 0))
        self.deferred = bool(on)
        return prev

    @_locked
    def set_column_sort(self, on=True):
        """Opt-in internal column order of device-resident calls with clouds: cloud-free columns first (rrtmg_hip_set_column_sort)."""
        self._ck(self.lib.rrtmg_hip_set_column_sort(self.h, 1 if on else 0))

    @_locked
    def set_sw_night_skip(self, on=True):
        """Opt-in night-column skip of the shortwave (rrtmg_hip_set_sw_night_skip): columns with coszen <= 0 get exact zeros in
        every output, and 64-column tiles whose columns are all night are not prepared or solved; day columns keep their bits."""
        self._ck(self.lib.rrtmg_hip_set_sw_night_skip(self.h, 1 if on else 0))

    @property
    def has_sw_night_pack(self):
        return hasattr(self.lib, "rrtmg_hip_set_sw_night_pack")

    @_locked
    def set_sw_night_pack(self, on=True):
        """Opt-in day-column pack of the shortwave (rrtmg_hip_set_sw_night_pack): an eligible device-resident call runs on an
        internal copy with the day columns packed into dense tiles, so that every night column's solve is saved; any other call
        runs as with set_sw_night_skip(True).  Night columns get exact zeros either way."""
        self._ck(self.lib.rrtmg_hip_set_sw_night_pack(self.h, 1 if on else 0))

    @property
    def has_sw_clear_sky(self):
        return hasattr(self.lib, "rrtmg_hip_set_sw_clear_sky")

    @_locked
    def set_sw_clear_sky(self, on=True):
        """Clear-sky outputs of the shortwave (rrtmg_hip_set_sw_clear_sky; on by default).  Off: a shortwave call forms no
        clear-sky stream -- tiles with cloud run a one-stream solve -- and swuflxc, swdflxc and swhrc are neither computed nor
        copied: `out` may leave them out (or hold None), and what it holds for them is not touched.  Calls with components or
        bands are refused while it is off."""
        if not self.has_sw_clear_sky:
            raise RRTMGError(4, "this librrtmg_hip.so has no rrtmg_hip_set_sw_clear_sky (shortwave call without the clear-sky outputs)")
        self._ck(self.lib.rrtmg_hip_set_sw_clear_sky(self.h, 1 if on else 0))
        self.sw_clear_sky = bool(on)

    @property
    def has_lw_clear_sky(self):
        return hasattr(self.lib, "rrtmg_hip_set_lw_clear_sky")

    @_locked
    def set_lw_clear_sky(self, on=True):
        """Clear-sky outputs of the longwave (rrtmg_hip_set_lw_clear_sky; on by default).  Off: a longwave call forms no
        clear-sky stream -- tiles with cloud run a one-stream solve -- and uflxc, dflxc, hrc (and duflxc_dt with idrv) are neither
        computed nor copied: `out` may leave them out (or hold None); an array it does hold for one of them is handed to the
        library, which neither writes nor reads it.  Band calls that request upc or dnc are refused while it is off; up and dn are served."""
        if not self.has_lw_clear_sky:
            raise RRTMGError(4, "this librrtmg_hip.so has no rrtmg_hip_set_lw_clear_sky (longwave call without the clear-sky outputs)")
        self._ck(self.lib.rrtmg_hip_set_lw_clear_sky(self.h, 1 if on else 0))
        self.lw_clear_sky = bool(on)

    @property
    def has_mcica_overlap_alpha(self):
        """Whether the library exports exponential McICA overlap (rrtmg_hip_set_mcica_overlap_alpha, rrtmg_hip_overlap_alpha)."""
        return hasattr(self.lib, "rrtmg_hip_set_mcica_overlap_alpha") and hasattr(self.lib, "rrtmg_hip_overlap_alpha")

    def _overlap_entry(self, name):
        if not self.has_mcica_overlap_alpha:
            raise RRTMGError(4, "this librrtmg_hip.so has no %s (exponential McICA overlap)" % name)
        return getattr(self.lib, name)

    @_locked
    def set_mcica_overlap_alpha(self, which, alpha, memspace=0, ncol=None, nlay=None):
        """Rank correlations of adjacent layers for exponential (icld 4) and exponential-random (icld 5) McICA overlap
        (rrtmg_hip_set_mcica_overlap_alpha).  which: "sw", "lw" or "both" (0, 1, 2).  alpha: [nlay][ncol] host array, or a device
        pointer with memspace=1 (then `ncol`, `nlay`); None clears the setting.  The library copies the array: it may be reused
        at once and is set again when the state changes."""
        w = {"sw": 0, "lw": 1, "both": 2}.get(which, which)
        entry = self._overlap_entry("rrtmg_hip_set_mcica_overlap_alpha")
        if alpha is None:
            self._ck(entry(self.h, int(w), 0, 0, 0, None))
        elif memspace:
            self._ck(entry(self.h, int(w), int(ncol), int(nlay), 1, int(alpha)))
        else:
            a = np.ascontiguousarray(alpha, dtype=np.float64)
            if a.ndim != 2:
                raise ValueError("alpha must be [nlay][ncol], got shape %r" % (a.shape,))
            self._ck(entry(self.h, int(w), a.shape[1], a.shape[0], 0, a.ctypes.data))

    @_locked
    def overlap_alpha(self, play, tlay, decorrelation_length, rd_over_g=287.05 / 9.80665, out=None, memspace=0, ncol=None, nlay=None):
        """alpha [nlay][ncol] = exp(-dz / decorrelation_length) from mid-layer pressure and temperature, row 0 = 1
        (rrtmg_hip_overlap_alpha): dz = rd_over_g * mean temperature of the two layers * ln(p[l-1] / p[l]), metres.  Host arrays
        [nlay][ncol], or device pointers with memspace=1 (then `out`, `ncol`, `nlay`)."""
        entry = self._overlap_entry("rrtmg_hip_overlap_alpha")
        if memspace:
            self._ck(entry(self.h, int(ncol), int(nlay), 1, int(play), int(tlay), float(rd_over_g), float(decorrelation_length), int(out)))
            return out
        p = np.ascontiguousarray(play, dtype=np.float64)
        t = np.ascontiguousarray(tlay, dtype=np.float64)
        if p.ndim != 2 or p.shape != t.shape:
            raise ValueError("play and tlay must be [nlay][ncol] arrays of one shape")
        a = np.empty(p.shape) if out is None else out
        self._ck(entry(self.h, p.shape[1], p.shape[0], 0, p.ctypes.data, t.ctypes.data, float(rd_over_g), float(decorrelation_length), a.ctypes.data))
        return a

    @_locked
    def sw_night_last(self):
        """-> (night tiles, night columns) of the last completed shortwave call (in deferred mode: after synchronize());
        (0, 0) when the skip was off (rrtmg_hip_sw_night_last); after a packed call: night.packed_counts."""
        t, c = C.c_int(0), C.c_int(0)
        self._ck(self.lib.rrtmg_hip_sw_night_last(self.h, C.byref(t), C.byref(c)))
        return t.value, c.value

    @_locked
    def get_table(self, name):
        n = self.lib.rrtmg_hip_get_table(self.h, name.encode(), None, 0)
        if n < 0:
            raise KeyError(name)
        out = np.empty(n)
        self.lib.rrtmg_hip_get_table(self.h, name.encode(), out.ctypes.data, n)
        return out

    # -- host-pointer calls: `inp` maps boundary names to numpy arrays (see _SW_FIELDS) -------
    @property
    def has_f32_boundary(self):
        """Whether the library exports the float32 boundary (rrtmg_hip_{sw,lw,radiation}_fluxes_f32; probed by the symbols)."""
        return all(hasattr(self.lib, n) for n in ("rrtmg_hip_sw_fluxes_f32", "rrtmg_hip_lw_fluxes_f32", "rrtmg_hip_radiation_fluxes_f32"))

    def _f32_entry(self, name):
        if not self.has_f32_boundary:
            raise RRTMGError(4, "this librrtmg_hip.so has no %s (float32 boundary)" % name)
        return getattr(self.lib, name)

    @staticmethod
    def _out_pointer(k, v, shape_size, dtype):
        """An output of a call as the integer its struct member takes.  precision="float32" checks what the library will write into."""
        if _is_pointer(v):
            return _device_pointer(v, dtype, "output %r" % k)
        if dtype != PRECISIONS["float64"] and not (isinstance(v, np.ndarray) and v.dtype == dtype and v.flags.c_contiguous and v.size == shape_size):
            raise ValueError("output %r: the library writes it in place: a C-contiguous %s array of %d elements" % (k, dtype.name, shape_size))
        return v.ctypes.data

    def _fill(self, a, inp, fields, flags, keep, dtype=PRECISIONS["float64"]):
        for k, f in flags.items():
            if k in inp:
                setattr(a, f, int(inp[k]))
        for k in _SCALES:
            if inp.get(k):
                setattr(a, k, float(inp[k]))
        for k, f in fields.items():
            v = inp.get(k)
            if v is None:
                continue
            host64 = k in ("bndsolvar", "indsolvar")      # host arrays of a few doubles, whatever the precision of the grid arrays
            if _is_pointer(v):      # raw device pointer (or a DeviceArray)
                setattr(a, f, _device_pointer(v, PRECISIONS["float64"] if host64 else dtype, "input %r" % k))
            else:
                arr = np.ascontiguousarray(v, dtype=np.float64 if host64 else dtype)
                keep.append(arr)
                setattr(a, f, arr.ctypes.data)

    @_locked
    def sw_fluxes(self, inp, mcica=False, out=None, memspace=0, components=None, bands=None, band_levels="all", surface=None, precision="float64"):
        """`surface`: None, or a dict with "albdir" and / or "albdif": the surface albedo by band for the direct beam / for
        diffuse radiation, [14][ncol] arrays (device pointers with memspace=1), bands in the order of band_limits("sw")
        (rrtmg_hip_sw_fluxes_surface); the one left out follows from asdir / aldir (asdif / aldif) by the reference driver's band
        rule, and with both given those four are not read.  The keys "albdir" / "albdif" of `inp` mean the same.
        `components`: None, or a dict SW_COMPONENTS name -> output (a C-contiguous float64 [nlay+1][ncol] array, or a device
        pointer with memspace=1) that the call fills as well (rrtmg_hip_sw_fluxes_components); the names left out are not
        computed.  `bands`: None, or a dict SW_BAND_FLUXES name -> output [14][nrow][ncol] in the same way
        (rrtmg_hip_sw_fluxes_bands); `band_levels`: "all" (nrow = nlay+1) or "boundaries" (nrow = 2: surface, top).
        `precision`: "float64" (the default: exactly the call without the keyword) or "float32" -- the float32 boundary
        (rrtmg_hip_sw_fluxes_f32): inputs are handed over as C-contiguous float32 (no copy of an array that already is one),
        outputs, components and band arrays must be C-contiguous float32 arrays (device arrays: dtype float32), and the
        results are those of the float64 call on the widened inputs, rounded once."""
        keep = []
        dtype = _precision(precision)
        a, sf, c, b, out = self._sw_structs(inp, mcica, out, memspace, components, bands, band_levels, surface, keep, dtype)
        if dtype == PRECISIONS["float32"]:
            self._ck(self._f32_entry("rrtmg_hip_sw_fluxes_f32")(self.h, C.byref(a), None if sf is None else C.byref(sf), None if c is None else C.byref(c),
                                                               None if b is None else C.byref(b)))
        elif sf is None and c is None and b is None:
            self._ck(self.lib.rrtmg_hip_sw_fluxes(self.h, C.byref(a)))
        elif sf is not None:
            self._ck(self.lib.rrtmg_hip_sw_fluxes_surface(self.h, C.byref(a), C.byref(sf), None if c is None else C.byref(c), None if b is None else C.byref(b)))
        elif b is not None:
            self._ck(self.lib.rrtmg_hip_sw_fluxes_bands(self.h, C.byref(a), None if c is None else C.byref(c), C.byref(b)))
        else:
            self._ck(self.lib.rrtmg_hip_sw_fluxes_components(self.h, C.byref(a), C.byref(c)))
        return out

    def _sw_structs(self, inp, mcica, out, memspace, components, bands, band_levels, surface, keep, dtype=PRECISIONS["float64"]):
        """-> (rrtmg_sw_args, surface struct | None, components struct | None, band struct | None, out) of a shortwave call;
        the arrays the structs point into stay alive in `keep` (and in `out`, `components`, `bands`)."""
        nlay, ncol = (inp["nlay"], inp["ncol"]) if memspace else inp["play"].shape
        a = SwArgs()
        a.struct_size = C.sizeof(SwArgs)
        a.ncol, a.nlay, a.memspace, a.mcica = int(ncol), int(nlay), int(memspace), int(bool(mcica))
        a.icld, a.inflgsw, a.iceflgsw, a.liqflgsw, a.dyofyr = 1, 2, 1, 1, 1
        a.adjes, a.scon, a.solcycfrac = float(inp.get("adjes", 1.0)), float(inp.get("scon", 1367.0)), float(inp.get("solcycfrac", 0.0))
        self._fill(a, inp, _SW_FIELDS, _SW_FLAGS, keep, dtype)
        clear = getattr(self, "sw_clear_sky", True)      # (set_sw_clear_sky(False): the three clear-sky outputs may be absent -> NULL)
        if out is None:
            out = {k: np.zeros((nlay + lev, ncol), dtype=dtype) for k, lev in SW_OUT if clear or k in SW_OUT_ALLSKY}
        for k, lev in SW_OUT:
            v = out[k] if clear or k in SW_OUT_ALLSKY else out.get(k)
            if v is not None:
                setattr(a, k, self._out_pointer(k, v, (nlay + lev) * ncol, dtype))
        if surface is None and (inp.get("albdir") is not None or inp.get("albdif") is not None):
            surface = {k: inp.get(k) for k in SW_SURFACE}
        b = None if bands is None else _band_struct(SwBandFluxes, SW_BAND_FLUXES, SW_NBAND, bands, band_levels, nlay, ncol, dtype)
        sf = None
        if surface is not None:
            if not hasattr(self.lib, "rrtmg_hip_sw_fluxes_surface"):
                raise RRTMGError(4, "this librrtmg_hip.so has no rrtmg_hip_sw_fluxes_surface (surface albedo by band)")
            sf = _surface_struct(surface, ncol, keep, dtype)
        c = None if components is None else self._components_struct(components, nlay, ncol, dtype)
        return a, sf, c, b, out

    @staticmethod
    def _components_struct(components, nlay, ncol, dtype=PRECISIONS["float64"]):
        c = SwComponents()
        c.struct_size = C.sizeof(SwComponents)
        for k, v in components.items():
            if k not in SW_COMPONENTS:
                raise KeyError("unknown shortwave flux component %r (one of %s)" % (k, ", ".join(SW_COMPONENTS)))
            if _is_pointer(v):
                setattr(c, k, _device_pointer(v, dtype, "component %r" % k))
                continue
            if not (isinstance(v, np.ndarray) and v.dtype == dtype and v.flags.c_contiguous and v.size == (nlay + 1) * ncol):
                raise ValueError("component %r: the library writes it in place: a C-contiguous %s array of %d x %d" % (k, dtype.name, nlay + 1, ncol))
            setattr(c, k, v.ctypes.data)
        return c

    @_locked
    def lw_fluxes(self, inp, mcica=False, out=None, memspace=0, bands=None, band_levels="all", precision="float64"):
        """`bands`: None, or a dict LW_BAND_FLUXES name -> output (a C-contiguous float64 [16][nrow][ncol] array, or a device
        pointer with memspace=1) that the call fills as well (rrtmg_hip_lw_fluxes_bands); `band_levels`: "all" (nrow =
        nlay+1) or "boundaries" (nrow = 2: surface, top).  `precision`: as in sw_fluxes (rrtmg_hip_lw_fluxes_f32)."""
        keep = []
        dtype = _precision(precision)
        a, b, out = self._lw_structs(inp, mcica, out, memspace, bands, band_levels, keep, dtype)
        if dtype == PRECISIONS["float32"]:
            self._ck(self._f32_entry("rrtmg_hip_lw_fluxes_f32")(self.h, C.byref(a), None if b is None else C.byref(b)))
        elif b is None:
            self._ck(self.lib.rrtmg_hip_lw_fluxes(self.h, C.byref(a)))
        else:
            self._ck(self.lib.rrtmg_hip_lw_fluxes_bands(self.h, C.byref(a), C.byref(b)))
        return out

    def _lw_structs(self, inp, mcica, out, memspace, bands, band_levels, keep, dtype=PRECISIONS["float64"]):
        """-> (rrtmg_lw_args, band struct | None, out) of a longwave call (see _sw_structs)."""
        nlay, ncol = (inp["nlay"], inp["ncol"]) if memspace else inp["play"].shape
        a = LwArgs()
        a.struct_size = C.sizeof(LwArgs)
        a.ncol, a.nlay, a.memspace, a.mcica = int(ncol), int(nlay), int(memspace), int(bool(mcica))
        a.icld, a.inflglw, a.iceflglw, a.liqflglw = 1, 2, 1, 1
        self._fill(a, inp, _LW_FIELDS, _LW_FLAGS, keep, dtype)
        clear = getattr(self, "lw_clear_sky", True)      # (set_lw_clear_sky(False): the clear-sky outputs may be absent or None -> NULL;
        #                                                    one that `out` does hold is handed over, and the library ignores it)
        if out is None:
            out = {k: np.zeros((nlay + lev, ncol), dtype=dtype) for k, lev in LW_OUT if clear or k not in LW_OUT_CLEAR}
            if a.idrv:
                out["duflx_dt"] = np.zeros((nlay + 1, ncol), dtype=dtype)
                if clear:
                    out["duflxc_dt"] = np.zeros((nlay + 1, ncol), dtype=dtype)
        for k in out:
            v = out[k]
            if v is not None:
                setattr(a, k, self._out_pointer(k, v, (nlay + (0 if k in ("hr", "hrc") else 1)) * ncol, dtype))
        b = None if bands is None else _band_struct(LwBandFluxes, LW_BAND_FLUXES, LW_NBAND, bands, band_levels, nlay, ncol, dtype)
        return a, b, out

    @_locked
    def radiation_fluxes(self, sw, lw, precision="float64"):
        """Both spectra of one host state in one library call (rrtmg_hip_radiation_fluxes): `sw` and `lw` are the keyword sets of
        sw_fluxes and lw_fluxes as dicts -- `inp`, and optionally `mcica`, `out`, `bands`, `band_levels`, and for the shortwave
        `components`, `surface`.  Host arrays only.  -> (sw out, lw out), bit for bit what sw_fluxes(**sw) followed by
        lw_fluxes(**lw) give.  An input that both `inp` hold as the same array (with the same unit factors) is uploaded once,
        and the two spectra overlap on the GPU; radiation_last() says what was shared.  `precision`: as in sw_fluxes, for both
        spectra (rrtmg_hip_radiation_fluxes_f32)."""
        dtype = _precision(precision)
        if not hasattr(self.lib, "rrtmg_hip_radiation_fluxes"):
            raise RRTMGError(4, "this librrtmg_hip.so has no rrtmg_hip_radiation_fluxes (joint shortwave + longwave call)")
        for name, kw, allowed in (("sw", sw, ("inp", "mcica", "out", "components", "bands", "band_levels", "surface")),
                                  ("lw", lw, ("inp", "mcica", "out", "bands", "band_levels"))):
            unknown = [k for k in kw if k not in allowed]
            if unknown or "inp" not in kw:
                raise TypeError("radiation_fluxes: %s takes 'inp' and optionally %s, not %s" % (name, ", ".join(allowed[1:]), ", ".join(map(repr, unknown)) or "nothing"))
        keep = []   # (every array the structs point into, until the call has returned)
        a, sf, c, b, sw_out = self._sw_structs(sw["inp"], sw.get("mcica", False), sw.get("out"), 0, sw.get("components"), sw.get("bands"),
                                               sw.get("band_levels", "all"), sw.get("surface"), keep, dtype)
        la, lb, lw_out = self._lw_structs(lw["inp"], lw.get("mcica", False), lw.get("out"), 0, lw.get("bands"), lw.get("band_levels", "all"), keep, dtype)
        call = RadiationCall()
        call.struct_size = C.sizeof(RadiationCall)
        call.sw, call.lw = C.pointer(a), C.pointer(la)
        if sf is not None:
            call.sw_surface = C.pointer(sf)
        if c is not None:
            call.sw_components = C.pointer(c)
        if b is not None:
            call.sw_bands = C.pointer(b)
        if lb is not None:
            call.lw_bands = C.pointer(lb)
        entry = self._f32_entry("rrtmg_hip_radiation_fluxes_f32") if dtype == PRECISIONS["float32"] else self.lib.rrtmg_hip_radiation_fluxes
        self._ck(entry(self.h, C.byref(call)))
        del keep
        return sw_out, lw_out

    @_locked
    def radiation_last(self):
        """-> (arrays shared, bytes uploaded, bytes shared) of the last radiation_fluxes call on this context
        (rrtmg_hip_radiation_last): inputs taken from what the call had already brought to the device, the host-to-device bytes it
        copied, and the bytes it did not copy because of that."""
        n, up, sh = C.c_int(0), C.c_longlong(0), C.c_longlong(0)
        self._ck(self.lib.rrtmg_hip_radiation_last(self.h, C.byref(n), C.byref(up), C.byref(sh)))
        return n.value, up.value, sh.value

    @_locked
    def mcica_mask(self, which, play, cldfrac, icld, permuteseed, irng):
        """Sub-column cloud mask [nlay][ncol][112 | 140] of 0 / 1 (rrtmg_hip_mcica_mask): icld 1, 2, 3, and -- while
        set_mcica_overlap_alpha holds an array of this shape for the spectrum -- 4 (exponential) and 5 (exponential-random)."""
        nlay, ncol = play.shape
        nsub = 112 if which == "sw" else 140
        out = np.zeros((nlay, ncol, nsub))
        p = np.ascontiguousarray(play, dtype=np.float64)
        c = np.ascontiguousarray(cldfrac, dtype=np.float64)
        self._ck(self.lib.rrtmg_hip_mcica_mask(self.h, 0 if which == "sw" else 1, ncol, nlay, int(icld), int(permuteseed),
                                               int(irng), p.ctypes.data, c.ctypes.data, out.ctypes.data))
        return out
