"""Cases of the fluxes by band (rrtmg_hip_sw_fluxes_bands, rrtmg_hip_lw_fluxes_bands) and their reference values.

The expected values come from our drivers of the reference's own procedures (tests/refshim/sw_shim.f90 and
lw_bands_shim.f90, built by tests/refshim/build.sh against oracle/_ref): the reference's transfer routines take a
band range and restart the g-point counter per band (istart = iend = iout = band), but its driver pins them to all bands.
tests/golden/make_band_fluxes.py writes one fixture per case, tests/golden/ref_bands_<case>.npz: gen/ (climt_amd.synthetic.
make_columns), flag/ (options), in/ (inputs given directly), pin (input hash), bb/ (the binder's broadband fluxes) and band/
(expected [nband][nlay+1][ncol] arrays).  The longwave runs on the synthetic tables of this build's blob
(fill_reference_from_blob), as the other longwave fixtures.  The GPU tests read the fixtures only."""
import ctypes as C
import os

import numpy as np

from helpers import GOLDEN, LW_DATA, SW_SHIM, band_rule, input_hash, sw_shim

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHIM = {"sw": SW_SHIM, "lw": os.path.join(ROOT, "tests", "_refshim", "liblw_bands_shim.so")}
MEMBERS = {"sw": ("up", "dn", "upc", "dnc", "dndir", "dndirc"), "lw": ("up", "dn", "upc", "dnc")}
NBAND = {"sw": 14, "lw": 16}
# the broadband output each band member sums to (dndir / dndirc: none among the plain outputs)
BROADBAND = {"sw": dict(up="swuflx", dn="swdflx", upc="swuflxc", dnc="swdflxc"), "lw": dict(up="uflx", dn="dflx", upc="uflxc", dnc="dflxc")}
EPS = 2.0 ** -53
SUM_BOUND = 256 * EPS   # |sum of bands - broadband| <= SUM_BOUND * F: non-negative terms, at most 140 of them, reassociated

_COMMON = dict(icld=1, iaer=0, adjes=1.0, dyofyr=1, scon=1367.0, isolvar=0, inflg=2, iceflg=1, liqflg=1, irng=0, permuteseed=1,
               idrv=0, _mcica=0, _overcast=0)
# fewer columns than the broadband fixtures (a band array is 14 or 16 times a broadband one), never fewer bands or levels
CASES = {
    "sw_clear_L60": (dict(ncol=4, nlay=60, cloudy=False, seed=201), dict(icld=0)),
    "sw_overcast_L60": (dict(ncol=4, nlay=60, cloudy=True, seed=202), dict(_overcast=1)),
    "sw_mcica_kiss_maxrand": (dict(ncol=4, nlay=60, cloudy=True, seed=203), dict(icld=2, irng=0, permuteseed=77, _mcica=1)),
    "sw_aer10_overcast": (dict(ncol=3, nlay=60, cloudy=True, seed=204), dict(iaer=10, _overcast=1)),
    "sw_overcast_L100": (dict(ncol=2, nlay=100, cloudy=True, seed=205), dict(_overcast=1)),
    "sw_lowsun_night": (dict(ncol=4, nlay=60, cloudy=True, seed=206), dict(_overcast=1)),
    "lw_clear_L60": (dict(ncol=4, nlay=60, cloudy=False, seed=211), dict(icld=0)),
    "lw_mcica_kiss_random": (dict(ncol=4, nlay=60, cloudy=True, seed=212), dict(icld=1, irng=0, permuteseed=31, _mcica=1)),
    "lw_maxrand": (dict(ncol=4, nlay=60, cloudy=True, seed=213), dict(icld=2)),
    "lw_cloudy_L100": (dict(ncol=2, nlay=100, cloudy=True, seed=214), dict(icld=1)),
}
SW_CASES = tuple(k for k in CASES if k.startswith("sw_"))
LW_CASES = tuple(k for k in CASES if k.startswith("lw_"))
# "Zero" of a night column: the reference clamps cos(zenith) at 1e-10 (zepzen, rrtmg_sw_rad.nomcica.f90:533-642) instead of
# skipping the column, so every shortwave flux of a night column is at most scon * (Earth-Sun factor <= 1.035) * 1e-10
NIGHT_ZERO = 1367.0 * 1.035 * 1.0e-10
LOW_SUN = (0.0, 1.0e-3, 0.02)   # coszen of columns 0, 1, 2 in sw_lowsun_night: night, and two low suns


def case_inputs(name):
    """-> (boundary-level input dict, mcica, flags with the _keys) of a case, everything but the McICA sub-columns."""
    from climt_amd.synthetic import make_columns, overcast
    gen, fl = CASES[name]
    flags = dict(_COMMON, **fl)
    c = make_columns(**gen)
    if flags["_overcast"]:
        c = overcast(c)
    if flags["iaer"] == 10:
        rng = np.random.default_rng(gen["seed"])
        shape = (14, gen["nlay"], gen["ncol"])
        c.update(tauaer=0.02 * rng.uniform(0.0, 1.0, shape), ssaaer=rng.uniform(0.8, 0.99, shape), asmaer=rng.uniform(0.5, 0.8, shape))
    if name == "sw_lowsun_night":
        cz = c["coszen"].copy()
        cz[:len(LOW_SUN)] = LOW_SUN
        c["coszen"] = cz
    c.update({k: v for k, v in flags.items() if not k.startswith("_")})
    return c, bool(flags["_mcica"]), flags


def shims_available():
    from oracle import ref_driver
    return all(ref_driver.available(w) and os.path.exists(SHIM[w]) for w in ("sw", "lw"))


def _reference_sw(c, mcica):
    from oracle import ref_driver
    ref = ref_driver.RefSW()
    ref.init()
    subcol = ref.subcol(c) if mcica else None
    if mcica:
        c["cldfmcl"] = np.ascontiguousarray(subcol["cldfmcl"])
    binder = ref.fluxes(c, mcica=mcica, subcol=subcol)
    albedo = band_rule(c)
    # the first six rows are the six members; slot 0 = the full band range, slots 1..14 = one call per band
    return binder, np.stack([sw_shim(c, mcica, *albedo, subcol=subcol, band=kb)[0][:len(MEMBERS["sw"])] for kb in range(1 + NBAND["sw"])])


def _reference_lw(c, mcica):
    from oracle import ref_driver
    from oracle.ref_driver import _cd, _d, _ri
    from tools.pack_tables import read_blob
    from tools.synth_lw_tables import fill_reference_from_blob
    blob = read_blob(LW_DATA)
    ref = ref_driver.RefLW()
    ref.init(fill_tables=lambda r: fill_reference_from_blob(r, blob))
    subcol = ref.subcol(c) if mcica else None
    if mcica:
        c["cldfmcl"] = np.ascontiguousarray(subcol["cldfmcl"])
    binder = ref.fluxes(c, mcica=mcica, subcol=subcol)
    nlay, ncol = c["play"].shape
    g = lambda k: _cd(c[k])
    l2 = lambda k, v: _cd(c[k]) if k in c else np.full((nlay, ncol), v)
    emis = _cd(c["emis"]) if "emis" in c else np.ones((16, ncol))
    tauaer = _cd(c["tauaer"]) if "tauaer" in c and np.shape(c["tauaer"])[0] == 16 else np.zeros((16, nlay, ncol))
    taucld = _cd(c["taucld"]) if "taucld" in c and np.shape(c["taucld"])[-1] == 16 else np.zeros((nlay, ncol, 16))
    out = np.zeros((17, 4, nlay + 1, ncol))
    head = [_ri(ncol), _ri(nlay), _ri(c["icld"]), _ri(c.get("idrv", 0)),
            _d(g("play")), _d(g("plev")), _d(g("tlay")), _d(g("tlev")), _d(g("tsfc")),
            _d(g("h2o")), _d(g("o3")), _d(g("co2")), _d(g("ch4")), _d(g("n2o")), _d(g("o2")),
            _d(l2("cfc11", 0.0)), _d(l2("cfc12", 0.0)), _d(l2("cfc22", 0.0)), _d(l2("ccl4", 0.0)),
            _d(emis), _ri(c["inflg"]), _ri(c["iceflg"]), _ri(c["liqflg"])]
    lib = C.CDLL(SHIM["lw"], mode=C.RTLD_LOCAL)
    if mcica:
        s = {k: _cd(v) for k, v in subcol.items()}
        lib.lw_bands_mcica(*(head + [_d(s["cldfmcl"]), _d(s["taucmcl"]), _d(s["ciwpmcl"]), _d(s["clwpmcl"]), _d(s["reicmcl"]), _d(s["relqmcl"]),
                                     _d(tauaer), _d(out)]))
    else:
        cld = [l2("cldfr", 0.0), taucld, l2("cicewp", 0.0), l2("cliqwp", 0.0), l2("reice", 20.0), l2("reliq", 10.0)]
        lib.lw_bands_nomcica(*(head + [_d(x) for x in cld] + [_d(tauaer), _d(out)]))
    return binder, out


def reference(name):
    """Run a case through the reference: the binder's broadband outputs and the shim's sums (needs oracle/_ref and the shims).
    -> (inputs incl. the McICA sub-column mask, binder outputs, shim output [1 + nband][member][nlay+1][ncol]: slot 0 = the
    full band range in one call, slots 1.. = one call per band)"""
    c, mcica, _ = case_inputs(name)
    binder, out = (_reference_sw if name.startswith("sw_") else _reference_lw)(c, mcica)
    return c, binder, out


def fixture_arrays(name):
    """Everything ref_bands_<name>.npz holds, computed now from the reference."""
    which = name[:2]
    c, binder, out = reference(name)
    gen, _ = CASES[name]
    _, mcica, flags = case_inputs(name)
    arr = {"gen/" + k: np.asarray(v) for k, v in gen.items()}
    arr.update({"flag/" + k: np.asarray(v) for k, v in flags.items()})
    if flags["iaer"] == 10:
        for k in ("tauaer", "ssaaer", "asmaer"):
            arr["in/" + k] = c[k]
    if name == "sw_lowsun_night":
        arr["in/coszen"] = c["coszen"]
    if mcica:
        arr["in/cldfmcl_bits"] = np.packbits(c["cldfmcl"].astype(bool).ravel())
        arr["in/cldfmcl_shape"] = np.asarray(c["cldfmcl"].shape)
    arr["pin"] = np.asarray(input_hash(c))
    arr.update({"bb/" + k: binder[k] for k in BROADBAND[which].values()})
    arr.update({"band/" + m: np.ascontiguousarray(out[1:, i]) for i, m in enumerate(MEMBERS[which])})
    return arr


def load_case(name):
    """Fixture -> (inputs at the C-ABI boundary, mcica flag, broadband {name: array}, band {member: [nband][nlay+1][ncol]});
    the inputs are checked against the pin."""
    from climt_amd.synthetic import make_columns, overcast
    z = np.load(os.path.join(GOLDEN, "ref_bands_%s.npz" % name))
    gen = {k[4:]: z[k].item() for k in z.files if k.startswith("gen/")}
    gen["cloudy"] = bool(gen["cloudy"])
    c = make_columns(**gen)
    flags = {k[5:]: z[k].item() for k in z.files if k.startswith("flag/")}
    if flags.pop("_overcast"):
        c = overcast(c)
    mcica = bool(flags.pop("_mcica"))
    c.update(flags)
    for k in z.files:
        if k.startswith("in/") and not k.startswith("in/cldfmcl"):
            c[k[3:]] = np.ascontiguousarray(z[k])
    if "in/cldfmcl_bits" in z.files:
        shape = tuple(int(x) for x in z["in/cldfmcl_shape"])
        c["cldfmcl"] = np.unpackbits(z["in/cldfmcl_bits"])[:int(np.prod(shape))].reshape(shape).astype(np.float64)
    got = input_hash(c)
    assert got == str(z["pin"]), "inputs of fixture ref_bands_%s changed: %s != %s" % (name, got, str(z["pin"]))
    return c, mcica, {k[3:]: z[k] for k in z.files if k.startswith("bb/")}, {k[5:]: z[k] for k in z.files if k.startswith("band/")}


def band_arrays(which, nlay, ncol, levels="all", members=None):
    """Zeroed output arrays of a `bands=` request."""
    nrow = 2 if levels == "boundaries" else nlay + 1
    return {m: np.zeros((NBAND[which], nrow, ncol)) for m in (members or MEMBERS[which])}
