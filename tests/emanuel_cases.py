"""What the Emanuel convection tests share: the names and layout of the fixtures tests/golden/emanuel_<case>_<nlay>.npz (made by
tests/golden/make_emanuel_golden.py from the reference's own numpy statement, pure_python.py::_convect), the scheme's parameters
and constants as the library takes them, tiling of a fixture's few columns to a launch, the deviation measure the fixtures'
tolerances are stated in, and the binary layout of tools/emanuel_check.cpp.

The measure: per column and field, the largest |got - want| relative to the column's largest |want| of that field, absolute where
the field is all zero in that column.  A fixture stores, per field, tol_<field> = max(16 x the largest such deviation that 16
reference runs under +-1 ulp perturbations of the inputs and of exp, log and sqrt showed, 1e-13); iflag is compared exactly."""
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden")

# the required situations (ISSUE: by the reference's own outputs) -> what the maker asserted of every column of the fixture
CASES = {
    "no_origin": "iflag 0 by the first exit: cbmf_in > 0 comes back 0",
    "too_cold": "iflag 0 by the DTMAX exit: cbmf_in = 0 = cbmf_out, and the same column with cbmf_in > 0 convects",
    "lcl_range": "iflag 2: PLCL outside [200, 2000) hPa",
    "base_at_top": "iflag 3: cloud base at the top",
    "deep": "iflag 1 with precip > 0 and wd > 0",
    "flag_only": "iflag 1 with all-zero tendencies: cbmf_in = 0 and the relaxed CBMF clipped to 0",
    "cfl": "iflag 4: a long dt",
    "freezing": "iflag 1, the convecting layers on both sides of 273 K",
    "sheared": "iflag 1 from cbmf_in = 0 in a sheared wind: fu and fv nonzero",
}
NLAYS = (8, 10, 30, 61)
NCOLS = (1, 63, 64, 65, 130)
MIN_NLAY = 4      # the smallest the entry accepts

PARAMETER_NAMES = ("minorig", "elcrit", "tlcrit", "entp", "sigd", "sigs", "omtrain", "omtsnow", "coeffr", "coeffs", "cu", "beta", "dtmax", "alpha", "damp", "delt0")
CONSTANT_NAMES = ("cpd", "cpv", "cl", "rv", "rd", "lv0", "g", "rowl")
# pure_python.py's attribute of each
REFERENCE_ATTRIBUTE = dict(minorig="MINORIG", elcrit="ELCRIT", tlcrit="TLCRIT", entp="ENTP", sigd="SIGD", sigs="SIGS", omtrain="OMTRAIN", omtsnow="OMTSNOW",
                           coeffr="COEFFR", coeffs="COEFFS", cu="CU", beta="BETA", dtmax="DTMAX", alpha="ALPHA", damp="DAMP", delt0="DELT0",
                           cpd="CPD", cpv="CPV", cl="CL", rv="RV", rd="RD", lv0="LV0", g="G", rowl="ROWL")
# the reference constructor's defaults (component.py) and the constants of the reference's statement (pure_python.py)
PARAMETERS = dict(minorig=1, elcrit=0.0011, tlcrit=-55.0, entp=1.5, sigd=0.05, sigs=0.12, omtrain=50.0, omtsnow=5.5, coeffr=1.0, coeffs=0.8, cu=0.7,
                  beta=10.0, dtmax=0.9, alpha=0.1, damp=0.1, delt0=300.0)
CONSTANTS = dict(cpd=1005.7, cpv=1870.0, cl=2500.0, rv=461.5, rd=287.04, lv0=2.501e6, g=9.8, rowl=1000.0)

INPUTS = ("t", "q", "u", "v", "p", "ph", "cbmf", "qs")             # t, q, u, v, p, qs [nlay][ncol]; ph [nlay+1][ncol]; cbmf [ncol]
PROFILES = ("ft", "fq", "fu", "fv")
SCALARS = ("precip", "wd", "tprime", "qprime", "cbmf_out", "cape")   # with iflag: the eleven outputs of _convect
FIELDS = PROFILES + SCALARS


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and bool((a.view(np.int64) == b.view(np.int64)).all())


def bolton_q_sat(t, p_pa, rd, rv):
    """The reference's (_core/util.py)."""
    es = 611.2 * np.exp(17.67 * (t - 273.15) / (t - 29.65))
    epsilon = rd / rv
    return epsilon * es / (p_pa - (1 - epsilon) * es)


_loaded = {}


def load(case, nlay):
    """-> dict of the fixture: the inputs, ref_<field>, ref_iflag, tol_<field>, dt, the parameters and constants."""
    key = (case, nlay)
    if key not in _loaded:
        z = np.load(os.path.join(GOLDEN, "emanuel_%s_%d.npz" % (case, nlay)))
        f = {k: z[k] for k in z.files}
        for k in f:
            f[k].setflags(write=False)
        _loaded[key] = f
    return _loaded[key]


def parameters(f):
    return {n: (int(f[n]) if n == "minorig" else float(f[n])) for n in PARAMETER_NAMES}


def constants(f):
    return {n: float(f[n]) for n in CONSTANT_NAMES}


def tile(f, ncol, keys=INPUTS):
    """The fixture's K columns repeated to ncol: column c is the fixture's column c % K."""
    k = f["t"].shape[1]
    idx = np.arange(ncol) % k
    return {n: np.ascontiguousarray(f[n][..., idx]) for n in keys}


def reference(f, ncol):
    out = tile(f, ncol, tuple("ref_" + n for n in FIELDS) + ("ref_iflag",))
    return {n[4:]: v for n, v in out.items()}


def deviations(got, want):
    """-> {field: the largest deviation over the columns, in the measure of the fixtures' tolerances}."""
    dev = {}
    for n in FIELDS:
        g, w = np.asarray(got[n], dtype=np.float64), np.asarray(want[n], dtype=np.float64)
        assert g.shape == w.shape, (n, g.shape, w.shape)
        g2, w2 = np.atleast_2d(g), np.atleast_2d(w)
        scale = np.abs(w2).max(axis=0)
        d = np.abs(g2 - w2).max(axis=0) / np.where(scale > 0, scale, 1.0)
        assert np.isfinite(g).all(), n
        dev[n] = float(d.max())
    return dev


def check(got, f, ncol, what=""):
    """got against the fixture tiled to ncol, every field within its stored tolerance and iflag exact -> the worst deviation / tolerance."""
    want = reference(f, ncol)
    assert np.array_equal(np.asarray(got["iflag"]).astype(np.int64), want["iflag"].astype(np.int64)), (what, got["iflag"], want["iflag"])
    worst = 0.0
    for n, d in deviations(got, want).items():
        tol = float(f["tol_" + n])
        assert d <= tol, (what, n, d, tol)
        worst = max(worst, d / tol)
    return worst


# ---- tools/emanuel_check.cpp ------------------------------------------------------------------------------------------------------------
def run_program(exe, tmp_path, arrays, dt, params=PARAMETERS, consts=CONSTANTS, use_qs=True, in_place=False, pressure_scale=1.0):
    """arrays: dict of INPUTS (qs may be None with use_qs False) -> dict of FIELDS, iflag and ft_per_day."""
    fin, fout = os.path.join(str(tmp_path), "in.bin"), os.path.join(str(tmp_path), "out.bin")
    nlay, ncol = arrays["t"].shape
    head = [float(use_qs), float(in_place), float(dt), float(pressure_scale)] + [float(params[n]) for n in PARAMETER_NAMES] + [float(consts[n]) for n in CONSTANT_NAMES]
    qs = arrays.get("qs") if use_qs else None
    body = [arrays[n] for n in INPUTS[:-1]] + [np.zeros((nlay, ncol)) if qs is None else qs]
    np.concatenate([head] + [np.asarray(v, dtype=np.float64).ravel() for v in body]).tofile(fin)
    r = subprocess.run([exe, str(ncol), str(nlay), fin, fout], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.startswith("ok"), (r.returncode, r.stdout, r.stderr)
    flat, nl = np.fromfile(fout), nlay * ncol
    assert flat.size == 5 * nl + 7 * ncol
    got = {n: flat[i * nl:(i + 1) * nl].reshape(nlay, ncol) for i, n in enumerate(PROFILES)}
    got.update({n: flat[4 * nl + i * ncol:4 * nl + (i + 1) * ncol] for i, n in enumerate(SCALARS + ("iflag",))})
    got["iflag"] = got["iflag"].astype(np.int32)
    got["ft_per_day"] = flat[4 * nl + 7 * ncol:].reshape(nlay, ncol)
    return got
