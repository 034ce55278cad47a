"""CorkLongwaveRadiation -- a drop-in for climt's (climt/_components/cork/lw/component.py) with optics="correlated_k": the
table-driven correlated-k longwave.  Same keywords, defaults and property dictionaries (which depend on the table: its gases,
its CO2 axis); the per-column rules run on the GPU through rrtmg_hip_cork_longwave (include/rrtmg_hip.h), one thread per column
and band, in the reference's order of operations, with the table resident on the device.

Built: additive overlap; tables of rank 5 (T, log p), 6 (+ the H2O axis) and 7 (+ the CO2 axis, interpolated in log k); the
band-grey continuum; the three gas-amount rules; per-band cloud depth and emissivity; diffusivity_factor; the eight diagnostics
of diagnostics_level 0.  Not built, and refused with NotImplementedError: optics="parmentier", ESFT overlap of more than one
gas, diagnostics_level >= 1.

CorkShortwaveRadiation (below) is the shortwave half of the same scheme, on rrtmg_hip_cork_shortwave: the same gas optical depth,
Rayleigh scattering, cloud mixing, delta-Eddington scaling and the two-stream adding method per g-point.

`table` is a path to an .npz, a mapping of arrays, a path to an .nc (where scipy imports), or a bare name, which is looked up in
an importable climt's shipped tables."""
import os

import numpy as np

from ._sympl_compat import TendencyComponent, get_constant
from .initialization import set_num_longwave_bands, set_num_shortwave_bands
from .rrtmg.common import make_context

DIFFUSIVITY_FACTOR = 1.66
# g/mol: H2O comes in as specific humidity, every other gas as a mole fraction times M_gas / M_dry (a gas not listed: 1)
MOLAR_MASS_DRY_AIR = 28.970
MOLAR_MASS = {"h2o": 18.015, "co2": 44.010, "o3": 47.998, "ch4": 16.043, "n2o": 44.013, "o2": 31.998}
_NETCDF_VARS = ("k_coefficients", "gpoint_weights", "temperature_grid", "pressure_grid_log", "h2o_vmr_grid", "co2_vmr_grid", "band_wavenumber_limits",
                "planck_fraction", "solar_source_per_gpoint", "rayleigh_coefficient", "continuum_kappa")
_GAS_CF_NAME = {"h2o": "specific_humidity", "co2": "mole_fraction_of_carbon_dioxide_in_air"}
_GAS_UNITS = {"h2o": "kg/kg"}
MAX_BANDS, MAX_GPOINTS, MAX_GASES = 32, 16, 8


def _decode(x):
    if isinstance(x, bytes):
        return x.decode("utf-8")
    if isinstance(x, np.ndarray) and x.dtype.kind == "S":
        return x.tobytes().decode("utf-8").rstrip("\x00")
    return str(x)


def _load_netcdf(path):
    try:
        from scipy.io import netcdf_file
    except ImportError as exc:
        raise ImportError("Reading .nc k-tables requires scipy; use an .npz table instead") from exc
    with netcdf_file(path, "r", mmap=False) as nc:
        out = {}
        for name in _NETCDF_VARS:
            if name in nc.variables:
                arr = np.asarray(nc.variables[name][:]).copy()
                out[name] = arr.astype(arr.dtype.newbyteorder("=")) if arr.dtype.byteorder not in ("=", "|") else arr
        if "gas_names" in nc.variables:
            out["gas_names"] = np.asarray([_decode(x) for x in np.atleast_1d(nc.variables["gas_names"][:])])
        elif getattr(nc, "gas_names", None) is not None:
            out["gas_names"] = np.asarray([s.strip() for s in _decode(nc.gas_names).split(",") if s.strip()])
        for attr in ("overlap_method", "resolution", "background_is_premixed"):
            if getattr(nc, attr, None) is not None:
                out[attr] = np.asarray(_decode(getattr(nc, attr)))
        return out


def load_k_table(table):
    """-> a dict of arrays: from a mapping, a path to an .npz or .nc, or the name of a table an importable climt ships."""
    if table is None:
        raise ValueError("CorkLongwaveRadiation(optics='correlated_k') needs table=")
    if hasattr(table, "keys"):
        return {k: np.asarray(table[k]) for k in table.keys()}
    table = os.fspath(table)
    if os.path.isfile(table):
        if table.endswith(".nc"):
            return _load_netcdf(table)
        with np.load(table, allow_pickle=False) as npz:
            return {name: npz[name] for name in npz.files}
    try:
        import climt
        folder = os.path.join(os.path.dirname(climt.__file__), "_data", "cork", "correlated_k")
    except ImportError:
        raise FileNotFoundError("no file %r; a bare table name is looked up in climt's shipped tables, and climt does not import here" % table) from None
    for ext, load in ((".npz", load_k_table), (".nc", _load_netcdf)):
        if os.path.isfile(os.path.join(folder, table + ext)):
            return load(os.path.join(folder, table + ext))
    raise FileNotFoundError("No k-table named %r (.npz or .nc)" % table)


class KTable(object):
    """A loaded table, checked and prepared for the device as the reference prepares it at every call: the two mole-fraction
    grids as log(max(grid, 1e-30)) with the grid's own ends as the clip interval, the continuum as log(max(kappa, 1e-40)), every
    grid in float64.  k stays in the file's element type (float32 or float64): the promotion to double is exact."""

    def __init__(self, table, kind="longwave"):
        """kind "longwave": planck_fraction is required.  kind "shortwave": solar_source_per_gpoint is required (kept in the
        file's element type, float32 or float64: the earth-sun factor is multiplied in it), rayleigh_coefficient is optional,
        planck_fraction is not read, and a table of rank 7 is refused."""
        if kind not in ("longwave", "shortwave"):
            raise ValueError("KTable: kind is 'longwave' or 'shortwave', not %r" % (kind,))
        self.kind = kind
        t = self.arrays = load_k_table(table)
        source = "planck_fraction" if kind == "longwave" else "solar_source_per_gpoint"
        for name in ("k_coefficients", "gpoint_weights", "temperature_grid", "pressure_grid_log", source, "gas_names"):
            if name not in t:
                raise ValueError("cork table: %s is missing" % name)
        k = np.asarray(t["k_coefficients"])
        if kind == "shortwave" and k.ndim == 7:
            raise ValueError("cork shortwave table: k_coefficients has rank 7 (a CO2 axis); the reference's shortwave passes no CO2 mole fraction "
                             "and fails on such a table at the first call: ranks 5 (T, p) and 6 (+ H2O) only")
        if k.ndim not in (5, 6, 7):
            raise ValueError("cork table: k_coefficients has rank %d, not 5 (T, p), 6 (+ H2O) or 7 (+ CO2)" % k.ndim)
        self.k = np.ascontiguousarray(k if k.dtype in (np.float32, np.float64) else k.astype(np.float64))
        self.ngas, self.nband, self.ngpt, nT, nP = k.shape[:5]
        nX, nC = (k.shape[5] if k.ndim >= 6 else 0), (k.shape[6] if k.ndim == 7 else 0)
        self.gas_names = [str(g) for g in np.atleast_1d(t["gas_names"])]
        self.overlap = str(t.get("overlap_method", np.array("additive")))
        self.has_h2o_axis, self.has_co2_axis = "h2o_vmr_grid" in t, "co2_vmr_grid" in t
        if len(self.gas_names) != self.ngas:
            raise ValueError("cork table: %d gas names for %d gases in k_coefficients" % (len(self.gas_names), self.ngas))
        if (nX > 0) != self.has_h2o_axis or (nC > 0) != self.has_co2_axis:
            raise ValueError("cork table: k_coefficients of rank %d %s h2o_vmr_grid and %s co2_vmr_grid" % (
                k.ndim, "needs" if nX else "goes without", "needs" if nC else "goes without"))
        if self.nband > MAX_BANDS or self.ngpt > MAX_GPOINTS or self.ngas > MAX_GASES:
            raise ValueError("cork table: %d bands, %d g-points and %d gases; the device path takes at most %d, %d and %d" % (
                self.nband, self.ngpt, self.ngas, MAX_BANDS, MAX_GPOINTS, MAX_GASES))
        f64 = lambda name: np.ascontiguousarray(t[name], dtype=np.float64)
        self.weights, self.t_grid, self.p_grid_log = f64("gpoint_weights"), f64("temperature_grid"), f64("pressure_grid_log")
        shapes = [("gpoint_weights", self.weights, (self.nband, self.ngpt)), ("temperature_grid", self.t_grid, (nT,)), ("pressure_grid_log", self.p_grid_log, (nP,))]
        self.planck = self.solar_source = self.rayleigh = None
        if kind == "longwave":
            self.planck = f64("planck_fraction")
            shapes.append(("planck_fraction", self.planck, (self.nband, self.ngpt, nT)))
        else:
            solar = np.asarray(t["solar_source_per_gpoint"])
            self.solar_source = np.ascontiguousarray(solar if solar.dtype in (np.float32, np.float64) else solar.astype(np.float64))
            shapes.append(("solar_source_per_gpoint", self.solar_source, (self.nband, self.ngpt)))
            if "rayleigh_coefficient" in t:
                self.rayleigh = f64("rayleigh_coefficient")
                shapes.append(("rayleigh_coefficient", self.rayleigh, (self.nband,)))
        self.x_grid_log = self.c_grid_log = self.x_clip = self.c_clip = self.log_cont = None
        if nX:
            x = f64("h2o_vmr_grid")
            self.x_grid_log, self.x_clip = np.log(np.maximum(x, 1e-30)), (float(x[0]), float(x[-1]))
            shapes.append(("h2o_vmr_grid", x, (nX,)))
        if nC:
            c = f64("co2_vmr_grid")
            self.c_grid_log, self.c_clip = np.log(np.maximum(c, 1e-30)), (float(c[0]), float(c[-1]))
            shapes.append(("co2_vmr_grid", c, (nC,)))
        cont = np.asarray(t["continuum_kappa"]) if "continuum_kappa" in t else None
        if cont is not None and cont.ndim == 4:      # (any other rank: the reference applies no continuum)
            if not nX:
                raise ValueError("cork table: continuum_kappa of rank 4 needs the H2O axis")
            # rank 7: the reference casts to float64 and then takes the log; rank 6: it takes the log in the file's own type
            self.log_cont = np.log(np.maximum(np.asarray(cont, dtype=np.float64), 1e-40)) if nC else np.log(np.maximum(cont, 1e-40)).astype(np.float64)
            shapes.append(("continuum_kappa", cont, (self.nband, nT, nP, nX)))
        for name, x, shape in shapes:
            if x.shape != shape:
                raise ValueError("cork table: %s is %s, k_coefficients %s wants %s" % (name, x.shape, k.shape, shape))
        for name, g in (("temperature_grid", self.t_grid), ("pressure_grid_log", self.p_grid_log), ("h2o_vmr_grid", self.x_grid_log), ("co2_vmr_grid", self.c_grid_log)):
            if g is not None and (g.size < 2 or not np.all(np.diff(g) > 0)):
                raise ValueError("cork table: %s must have at least 2 nodes and strictly increase" % name)
        self.fully_premixed = self.gas_names == ["effective"] and not self.has_h2o_axis
        self.premixed_bg = ((self.gas_names == ["effective"] and self.has_h2o_axis)
                            or str(t.get("background_is_premixed", np.array(""))).lower() == "true")
        self.gas_rule = 0 if self.fully_premixed else 1 if self.premixed_bg else 2
        if self.gas_rule != 1 and self.has_h2o_axis:
            raise ValueError("cork table: an H2O axis needs a premixed background (gas_names ['effective'] or background_is_premixed): "
                             "no other gas rule has the H2O mole fraction")
        self.gas_scale = [1.0 if g == "h2o" or self.gas_rule != 2 else MOLAR_MASS.get(g, MOLAR_MASS_DRY_AIR) / MOLAR_MASS_DRY_AIR for g in self.gas_names]

    def upload(self, ctx):
        if self.kind == "shortwave":
            return ctx.cork_sw_table_create(self.k, self.weights, self.solar_source, self.t_grid, self.p_grid_log, x_grid_log=self.x_grid_log, x_clip=self.x_clip,
                                            log_cont=self.log_cont, rayleigh=self.rayleigh)
        return ctx.cork_table_create(self.k, self.weights, self.planck, self.t_grid, self.p_grid_log, x_grid_log=self.x_grid_log, x_clip=self.x_clip,
                                     c_grid_log=self.c_grid_log, c_clip=self.c_clip, log_cont=self.log_cont)


class CorkLongwaveRadiation(TendencyComponent):
    """The correlated-k longwave of climt's cork scheme: k interpolated in (T, log p[, log X_H2O[, log X_CO2]]) from a table,
    summed over the gases, plus the band-grey continuum and the cloud depth; the Planck fraction of every g-point; a
    diffusivity-factor sweep up from the surface and down from the top per g-point; weighted sums by band and over the bands."""

    # Class-level default, as in the reference: an instance pickled before the keyword existed still resolves it
    _diffusivity_factor = DIFFUSIVITY_FACTOR

    def __init__(self, optics="parmentier", table=None, coefficients="solar_composition", rosseland_mean_fit="freedman2014",
                 diffusivity_factor=DIFFUSIVITY_FACTOR, device=0, context=None, **kwargs):
        """
        Args: the reference's, plus `device`, `context` like the other components of this package.  Only optics="correlated_k"
        is built; `coefficients` and `rosseland_mean_fit` belong to the Parmentier optics and are not read.
        """
        self._diffusivity_factor = diffusivity_factor
        self._optics_mode = optics
        if optics == "parmentier":
            raise NotImplementedError("CorkLongwaveRadiation: optics='parmentier' (the picket-fence optics) is not built on the device; use optics='correlated_k'")
        if optics != "correlated_k":
            raise ValueError("Unknown optics mode: %s" % optics)
        self._ktable = KTable(table)
        if self._ktable.overlap == "esft" and self._ktable.ngas > 1:
            raise NotImplementedError("CorkLongwaveRadiation: overlap_method 'esft' with more than one gas (the outer product of g-points) is not built; additive overlap is")
        self._num_bands, self._num_gpts = self._ktable.nband, self._ktable.ngpt
        self._gas_names = list(self._ktable.gas_names)
        self._has_co2_axis = self._ktable.has_co2_axis
        self._fully_premixed, self._premixed_bg = self._ktable.fully_premixed, self._ktable.premixed_bg
        self._diagnostics_level = kwargs.pop("diagnostics_level", 0)
        if self._diagnostics_level >= 1:
            raise NotImplementedError("CorkLongwaveRadiation: diagnostics_level >= 1 (per-g-point fluxes and layer transmittances) is not built: "
                                      "the device path keeps nothing with a g-point axis")
        set_num_longwave_bands(self._num_bands)
        super(CorkLongwaveRadiation, self).__init__(**kwargs)
        self._device = device
        if context is not None:
            self._ctx = context
        self._handle = None

    def __getattr__(self, name):      # (only where the attribute is not there: the context of `device`, made at first use)
        if name == "_ctx" and "_device" in self.__dict__:
            self._ctx = make_context(self._device)
            return self._ctx
        raise AttributeError(name)

    def __getstate__(self):
        """What is pickled: the table and the settings.  The context and the table handles on it belong to the process; a
        copy makes the shared context of its device at first use, where the original may have been given another one."""
        state = {k: v for k, v in self.__dict__.items() if k not in ("_ctx", "_handle_ds", "_handle_ctx")}
        state["_handle"] = None
        return state

    @property
    def input_properties(self):
        props = {
            "air_temperature": {"dims": ["mid_levels", "*"], "units": "degK", "alias": "T"},
            "air_pressure": {"dims": ["mid_levels", "*"], "units": "Pa", "alias": "p"},
            "air_pressure_on_interface_levels": {"dims": ["interface_levels", "*"], "units": "Pa", "alias": "p_int"},
            "surface_temperature": {"dims": ["*"], "units": "degK", "alias": "T_surf"},
            "surface_longwave_emissivity": {"dims": ["num_longwave_bands", "*"], "units": "dimensionless", "alias": "emissivity"},
        }
        if self._premixed_bg:
            props["specific_humidity"] = {"dims": ["mid_levels", "*"], "units": "kg/kg", "alias": "h2o"}
            if self._has_co2_axis:
                props["mole_fraction_of_carbon_dioxide_in_air"] = {"dims": ["mid_levels", "*"], "units": "mole/mole", "alias": "co2"}
        elif not self._fully_premixed:
            for gas in self._gas_names:
                props[_GAS_CF_NAME.get(gas, "mole_fraction_of_%s_in_air" % gas)] = {"dims": ["mid_levels", "*"], "units": _GAS_UNITS.get(gas, "mole/mole"), "alias": gas}
        props["longwave_optical_thickness_due_to_cloud"] = {"dims": ["mid_levels", "*", "num_longwave_bands"], "units": "dimensionless", "alias": "tau_cloud_lw"}
        return props

    @property
    def tendency_properties(self):
        return {"air_temperature": {"units": "degK s^-1"}}

    @property
    def diagnostic_properties(self):
        il, ml = ["interface_levels", "*"], ["mid_levels", "*"]
        band = ["num_longwave_bands"]
        return {
            "upwelling_longwave_flux_in_air": {"dims": il, "units": "W m^-2"},
            "downwelling_longwave_flux_in_air": {"dims": list(il), "units": "W m^-2"},
            "upwelling_longwave_flux_in_air_per_band": {"dims": il + band, "units": "W m^-2"},
            "downwelling_longwave_flux_in_air_per_band": {"dims": il + band, "units": "W m^-2"},
            "air_temperature_tendency_from_longwave": {"dims": ml, "units": "degK day^-1"},
            "longwave_optical_depth_per_band": {"dims": ml + band, "units": "dimensionless"},
            "longwave_transmittance_per_band": {"dims": ml + band, "units": "dimensionless"},
            "air_temperature_tendency_from_longwave_per_band": {"dims": ml + band, "units": "degK day^-1"},
        }

    @property
    def num_longwave_bands(self):
        return self._num_bands

    def constants(self):
        """The constants of the reference's array_call as the library takes them, asked for at every call under the unit strings
        the reference asks with."""
        return dict(m_h2o=MOLAR_MASS["h2o"] / MOLAR_MASS_DRY_AIR, sigma_sb=get_constant("stefan_boltzmann_constant", "W/m^2/K^4"),
                    g=get_constant("gravitational_acceleration", "m/s^2"), cpd=get_constant("heat_capacity_of_dry_air_at_constant_pressure", "J/kg/K"),
                    diffusivity=self._diffusivity_factor)

    def table_handle(self):
        """The table on this component's context, uploaded at the first call."""
        if getattr(self, "_handle", None) is None:
            self._handle = self._ktable.upload(self._ctx)
        return self._handle

    def gas_inputs(self):
        """-> the names of the state quantities that are the library's gas0, gas1, ... (None: not read)."""
        if self._fully_premixed and not self._premixed_bg:
            return []
        if self._premixed_bg:
            return ["specific_humidity" if self._ktable.has_h2o_axis else None] + (["mole_fraction_of_carbon_dioxide_in_air"] if self._has_co2_axis else [])
        return [_GAS_CF_NAME.get(gas, "mole_fraction_of_%s_in_air" % gas) for gas in self._gas_names]

    def __call__(self, state, *args, **kwargs):
        """A host state goes through sympl's machinery to array_call; a climt_amd.DeviceState (state resident in HBM) takes the
        device path (climt_amd/device_state.py)."""
        from .device_state import DeviceState, cork_longwave_device_call
        if isinstance(state, DeviceState):
            return cork_longwave_device_call(self, state)
        return super(CorkLongwaveRadiation, self).__call__(state, *args, **kwargs)

    def array_call(self, state):
        P = self.input_properties

        def get(name):      # (sympl hands an input with an alias over under it)
            alias = P[name].get("alias", name)
            return np.asarray(state[alias] if alias in state else state[name], dtype=np.float64)
        t, p_int = get("air_temperature"), get("air_pressure_on_interface_levels")
        nlay, nband = t.shape[0], self._num_bands
        levels = lambda x: np.reshape(x, (x.shape[0], -1))
        gases = [None if n is None else levels(get(n)) for n in self.gas_inputs()]
        up, dn, tend, d = self._ctx.cork_longwave(
            self.table_handle(), nband, levels(t), levels(get("air_pressure")), levels(p_int), np.reshape(get("surface_temperature"), (-1,)),
            np.reshape(get("surface_longwave_emissivity"), (nband, -1)), self.constants(), self._ktable.gas_rule, gases=gases, gas_scale=self._ktable.gas_scale,
            taucld=np.reshape(get("longwave_optical_thickness_due_to_cloud"), (nlay, -1, nband)))
        last = lambda x, shape: np.moveaxis(x, 0, -1).reshape(tuple(shape) + (nband,))      # [band][k][col] -> (k, *horizontal, band)
        diagnostics = {
            "upwelling_longwave_flux_in_air": up.reshape(p_int.shape), "downwelling_longwave_flux_in_air": dn.reshape(p_int.shape),
            "upwelling_longwave_flux_in_air_per_band": last(d["up_band"], p_int.shape), "downwelling_longwave_flux_in_air_per_band": last(d["dn_band"], p_int.shape),
            "air_temperature_tendency_from_longwave": d["hr"].reshape(t.shape), "longwave_optical_depth_per_band": last(d["tau_band"], t.shape),
            "longwave_transmittance_per_band": last(d["trans_band"], t.shape), "air_temperature_tendency_from_longwave_per_band": last(d["hr_band"], t.shape)}
        return {"air_temperature": tend.reshape(t.shape)}, diagnostics


class CorkShortwaveRadiation(TendencyComponent):
    """The correlated-k two-stream shortwave of climt's cork scheme (climt/_components/cork/sw/component.py with
    optics="correlated_k"): the gas optical depth as in CorkLongwaveRadiation, Rayleigh scattering where the table has a
    coefficient, the cloud mixed in by band, delta-Eddington scaling, the Meador-Weaver / PIFM layer operator and the
    Shonk-Hogan adding method per g-point, on the GPU through rrtmg_hip_cork_shortwave (include/rrtmg_hip.h; the rules:
    climt_amd/csrc/rrtmg_cork_sw.h).  Same keywords, defaults and property dictionaries as the reference's.

    Not built, and refused with NotImplementedError: optics="parmentier", ESFT overlap of more than one gas,
    diagnostics_level >= 1.  A table of rank 7 is refused with ValueError: the reference fails on it at the first call.
    As in the reference, flux_adjustment_for_earth_sun_distance of the FIRST column scales every column, and
    surface_temperature is stated as an input although it is not read."""

    def __init__(self, optics="parmentier", table=None, coefficients="solar_composition", stellar_spectrum="sun", rosseland_mean_fit="freedman2014",
                 device=0, context=None, **kwargs):
        """
        Args: the reference's, plus `device`, `context` like the other components of this package.  Only optics="correlated_k"
        is built; `coefficients`, `stellar_spectrum` and `rosseland_mean_fit` belong to the Parmentier optics and are not read;
        `bond_albedo_feedback` (a keyword of **kwargs, as in the reference) likewise.
        """
        self._optics_mode = optics
        if optics == "parmentier":
            raise NotImplementedError("CorkShortwaveRadiation: optics='parmentier' (the picket-fence optics) is not built on the device; use optics='correlated_k'")
        if optics != "correlated_k":
            raise ValueError("Unknown optics mode: %s" % optics)
        if table is None:
            raise ValueError("CorkShortwaveRadiation(optics='correlated_k') needs table=")
        self._ktable = KTable(table, kind="shortwave")
        if self._ktable.overlap == "esft" and self._ktable.ngas > 1:
            raise NotImplementedError("CorkShortwaveRadiation: overlap_method 'esft' with more than one gas (the outer product of g-points) is not built; additive overlap is")
        self._num_bands, self._num_gpts = self._ktable.nband, self._ktable.ngpt
        self._gas_names = list(self._ktable.gas_names)
        self._has_co2_axis = False
        self._fully_premixed, self._premixed_bg = self._ktable.fully_premixed, self._ktable.premixed_bg
        self._bond_albedo_feedback = kwargs.pop("bond_albedo_feedback", False)
        self._diagnostics_level = kwargs.pop("diagnostics_level", 0)
        if self._diagnostics_level >= 1:
            raise NotImplementedError("CorkShortwaveRadiation: diagnostics_level >= 1 (layer operators and beam profiles by g-point) is not built: "
                                      "the device path keeps nothing with a g-point axis")
        set_num_shortwave_bands(self._num_bands)
        super(CorkShortwaveRadiation, self).__init__(**kwargs)
        self._device = device
        if context is not None:
            self._ctx = context
        self._handle = None

    # the context made at first use, what is pickled, the resident table and the gas inputs: the longwave component's
    __getattr__ = CorkLongwaveRadiation.__getattr__
    __getstate__ = CorkLongwaveRadiation.__getstate__
    table_handle = CorkLongwaveRadiation.table_handle
    gas_inputs = CorkLongwaveRadiation.gas_inputs

    @property
    def input_properties(self):
        props = {
            "air_temperature": {"dims": ["mid_levels", "*"], "units": "degK", "alias": "T"},
            "air_pressure": {"dims": ["mid_levels", "*"], "units": "Pa", "alias": "p"},
            "air_pressure_on_interface_levels": {"dims": ["interface_levels", "*"], "units": "Pa", "alias": "p_int"},
            "surface_temperature": {"dims": ["*"], "units": "degK", "alias": "T_surf"},
            "zenith_angle": {"dims": ["*"], "units": "radians", "alias": "zenith"},
            "surface_albedo_for_direct_shortwave": {"dims": ["*"], "units": "dimensionless", "alias": "albedo"},
            "flux_adjustment_for_earth_sun_distance": {"dims": ["*"], "units": "dimensionless", "alias": "earth_sun_factor"},
        }
        if self._premixed_bg:
            props["specific_humidity"] = {"dims": ["mid_levels", "*"], "units": "kg/kg", "alias": "h2o"}
        elif not self._fully_premixed:
            for gas in self._gas_names:
                props[_GAS_CF_NAME.get(gas, "mole_fraction_of_%s_in_air" % gas)] = {"dims": ["mid_levels", "*"], "units": _GAS_UNITS.get(gas, "mole/mole"), "alias": gas}
        band = {"dims": ["mid_levels", "*", "num_shortwave_bands"], "units": "dimensionless"}
        props["shortwave_optical_thickness_due_to_cloud"] = dict(band, alias="tau_cloud_sw")
        props["single_scattering_albedo_due_to_cloud"] = dict(band, alias="ssa_cloud")
        props["cloud_asymmetry_parameter"] = dict(band, alias="g_cloud")
        return props

    @property
    def tendency_properties(self):
        return {"air_temperature": {"units": "degK s^-1"}}

    @property
    def diagnostic_properties(self):
        il, ml = ["interface_levels", "*"], ["mid_levels", "*"]
        band = ["num_shortwave_bands"]
        return {
            "upwelling_shortwave_flux_in_air": {"dims": il, "units": "W m^-2"},
            "downwelling_shortwave_flux_in_air": {"dims": list(il), "units": "W m^-2"},
            "upwelling_shortwave_flux_in_air_per_band": {"dims": il + band, "units": "W m^-2"},
            "downwelling_shortwave_flux_in_air_per_band": {"dims": il + band, "units": "W m^-2"},
            "air_temperature_tendency_from_shortwave": {"dims": ml, "units": "degK day^-1"},
            "shortwave_optical_depth_per_band": {"dims": ml + band, "units": "dimensionless"},
            "air_temperature_tendency_from_shortwave_per_band": {"dims": ml + band, "units": "degK day^-1"},
        }

    @property
    def num_shortwave_bands(self):
        return self._num_bands

    def constants(self):
        """The constants of the reference's array_call as the library takes them."""
        return dict(m_h2o=MOLAR_MASS["h2o"] / MOLAR_MASS_DRY_AIR, g=get_constant("gravitational_acceleration", "m/s^2"),
                    cpd=get_constant("heat_capacity_of_dry_air_at_constant_pressure", "J/kg/K"))

    def __call__(self, state, *args, **kwargs):
        """A host state goes through sympl's machinery to array_call; a climt_amd.DeviceState (state resident in HBM) takes the
        device path (climt_amd/device_state.py)."""
        from .device_state import DeviceState, cork_shortwave_device_call
        if isinstance(state, DeviceState):
            return cork_shortwave_device_call(self, state)
        return super(CorkShortwaveRadiation, self).__call__(state, *args, **kwargs)

    def array_call(self, state):
        P = self.input_properties

        def get(name):      # (sympl hands an input with an alias over under it)
            alias = P[name].get("alias", name)
            return np.asarray(state[alias] if alias in state else state[name], dtype=np.float64)
        t, p_int = get("air_temperature"), get("air_pressure_on_interface_levels")
        nlay, nband = t.shape[0], self._num_bands
        levels = lambda x: np.reshape(x, (x.shape[0], -1))
        column = lambda name: np.reshape(get(name), (-1,))
        gases = [None if n is None else levels(get(n)) for n in self.gas_inputs()]
        cloud = tuple(np.reshape(get(n), (nlay, -1, nband)) for n in
                      ("shortwave_optical_thickness_due_to_cloud", "single_scattering_albedo_due_to_cloud", "cloud_asymmetry_parameter"))
        up, dn, tend, d = self._ctx.cork_shortwave(
            self.table_handle(), nband, levels(t), levels(get("air_pressure")), levels(p_int), column("zenith_angle"), column("surface_albedo_for_direct_shortwave"),
            column("flux_adjustment_for_earth_sun_distance"), self.constants(), self._ktable.gas_rule, gases=gases, gas_scale=self._ktable.gas_scale, cloud=cloud)
        last = lambda x, shape: np.moveaxis(x, 0, -1).reshape(tuple(shape) + (nband,))      # [band][k][col] -> (k, *horizontal, band)
        diagnostics = {
            "upwelling_shortwave_flux_in_air": up.reshape(p_int.shape), "downwelling_shortwave_flux_in_air": dn.reshape(p_int.shape),
            "upwelling_shortwave_flux_in_air_per_band": last(d["up_band"], p_int.shape), "downwelling_shortwave_flux_in_air_per_band": last(d["dn_band"], p_int.shape),
            "air_temperature_tendency_from_shortwave": d["hr"].reshape(t.shape), "shortwave_optical_depth_per_band": last(d["tau_band"], t.shape),
            "air_temperature_tendency_from_shortwave_per_band": last(d["hr_band"], t.shape)}
        return {"air_temperature": tend.reshape(t.shape)}, diagnostics
