"""The dry convective adjustment (rrtmg_hip_dry_adjustment, climt_amd.DryConvectiveAdjustment): the numpy statement of the rule
and the cases the tests run.

`statement` is the rule as include/rrtmg_hip.h states it, a plain loop per column on Python floats (`**` is libm's pow).  It
forms theta_q of a layer once and again after a mixing has rewritten the layer -- the same expression on the same operands as
forming all of them again for every k, which is what the reference does (tests/golden/make_dry_adjust_golden.py runs the
reference's own loop; tests/test_dry_adjustment.py compares).  Besides the new T and q it returns the smallest relative margin
|theta_avg - theta_q[m]| / theta_q[m] over every comparison it made, and mixed_top by column.

Every case used for a comparison of values has a margin >= MIN_MARGIN = 1e-9 (`case` asserts it): a pow that differs from libm's
in its last bits moves theta_q by ~1e-16 relative and cannot flip a decision, so the values agree to rounding: TOL."""
import functools

import numpy as np

# sympl's default constants, as DryConvectiveAdjustment asks for them (pref in Pa)
CONSTANTS = dict(cpd=1004.64, cvap=1846.0, rd=287.0, rv=461.5, pref=1.0132e5)
MIN_MARGIN = 1.0e-9
# against the statement and the goldens, relative: per layer three pow at ~1 ulp and at most 2 nlay rounded additions,
# ~3e-14 at 61 layers
TOL = 1.0e-12
CASES = ("stable", "heated_surface", "whole_column", "two_runs", "cascade", "moist")
NLAYS = (1, 2, 3, 30, 61)
NCOLS = (1, 63, 64, 65, 130)


def statement(T, q, p, p_int, k=CONSTANTS):
    """-> (T_new, q_new, margin, mixed_top): arrays [nlay][ncol] (p_int [nlay+1][ncol]), level 0 at the surface."""
    cpd, cvap, rd, rv, pref = (float(k[n]) for n in ("cpd", "cvap", "rd", "rv", "pref"))
    nlev, ncol = T.shape
    T_new, q_new = np.array(T, dtype=np.float64), np.array(q, dtype=np.float64)
    mixed_top = np.full(ncol, -1, dtype=np.int32)
    margin = np.inf
    eps = rv / rd

    def theta_of(Tm, qm, pm):
        rd_cp = (rd * (1.0 - qm) + rv * qm) / (cpd * (1.0 - qm) + cvap * qm)
        return Tm * (pref / pm) ** rd_cp * (1.0 + qm * eps - qm)

    for i in range(ncol):
        Tc, qc = [float(x) for x in T[:, i]], [float(x) for x in q[:, i]]
        pc, pi = [float(x) for x in p[:, i]], [float(x) for x in p_int[:, i]]
        dp = [pi[m] - pi[m + 1] for m in range(nlev)]
        theta = [theta_of(Tc[m], qc[m], pc[m]) for m in range(nlev)]
        for kk in range(nlev - 1, -1, -1):
            total, top = 0.0, -1
            for m in range(kk, nlev):
                total += theta[m]
                theta_avg = total / (m - kk + 1)
                if m > kk:
                    margin = min(margin, abs(theta_avg - theta[m]) / theta[m])
                    if theta_avg > theta[m]:
                        top = m
            if top == -1:
                continue
            sum_enthalpy, sum_q_dp = 0.0, 0.0
            for m in range(kk, top + 1):
                cp_m = cpd * (1.0 - qc[m]) + cvap * qc[m]
                sum_enthalpy += cp_m * Tc[m] * dp[m]
                sum_q_dp += qc[m] * dp[m]
            mean_q = sum_q_dp / (pi[kk] - pi[top + 1])
            cp_mixed = cpd * (1.0 - mean_q) + cvap * mean_q
            rdcp_mixed = (rd * (1.0 - mean_q) + rv * mean_q) / cp_mixed
            sum_theta_den = 0.0
            for m in range(kk, top + 1):
                sum_theta_den += cp_mixed * (pc[m] / pref) ** rdcp_mixed * dp[m]
            mean_theta = sum_enthalpy / sum_theta_den
            for m in range(kk, top + 1):
                qc[m] = mean_q
                Tc[m] = mean_theta * (pc[m] / pref) ** rdcp_mixed
                theta[m] = theta_of(Tc[m], qc[m], pc[m])
            mixed_top[i] = max(mixed_top[i], top)
        T_new[:, i], q_new[:, i] = Tc, qc
    return T_new, q_new, float(margin), mixed_top


def pressures(nlay, ncol):
    """-> (p [nlay][ncol], p_int [nlay+1][ncol]) in Pa: layers thinner towards the top, the surface pressure varying by column."""
    ps = 1.0e5 + 37.0 * np.arange(ncol)
    sigma = (1.0 - np.arange(nlay + 1) / float(nlay)) ** 1.5
    p_int = 2000.0 + sigma[:, None] * (ps[None, :] - 2000.0)
    return 0.5 * (p_int[:-1] + p_int[1:]), p_int


def _inputs(name, nlay, ncol):
    p, p_int = pressures(nlay, ncol)
    kappa = CONSTANTS["rd"] / CONSTANTS["cpd"]
    to_T = lambda theta: theta * (p / CONSTANTS["pref"]) ** kappa      # (dry air: theta_q is this theta, to rounding)
    lev = np.arange(nlay)[:, None] * np.ones((1, ncol))
    amp = 1.0 + 0.01 * np.arange(ncol)[None, :]                       # every column its own numbers
    stable = 300.0 + 4.0 * lev                                        # +4 K of potential temperature per layer
    q = np.zeros((nlay, ncol))
    if name == "stable":
        T = np.full((nlay, ncol), 290.0)                              # isothermal
    elif name == "heated_surface":
        T = np.full((nlay, ncol), 290.0)
        if nlay > 1:                                                  # layer 0 alone: 2 % (and more by column) above the theta of layer 1
            T[0] = 290.0 * (p[0] / p[1]) ** kappa * (1.0 + 0.02 * amp[0])
    elif name == "whole_column":
        T = to_T(330.0 - (25.0 * amp) * lev / nlay)
    elif name == "two_runs":
        theta = stable.copy()
        for base in (0, nlay // 2 + 2):                               # two reversed stretches of three layers, stable air between
            for j in range(3):
                if base + j < nlay:
                    theta[base + j] = stable[base] + 2.0 - (2.5 * amp[0]) * j
        T = to_T(theta)
    elif name == "cascade":
        # k = 2 mixes with k + 1; k = 1 and then k = 0 are each warmer than the run above them, which the mixing before has
        # just rewritten: their scans read theta_q formed again from the new T and q
        theta = stable + 30.0
        for m, v in enumerate((312.0, 309.0, 307.0, 296.0)):
            if m < nlay:
                theta[m] = v + (m % 2) * 0.3 * amp[0]
        T = to_T(theta)
    elif name == "moist":
        # weakly stable for dry air, top-heavy in theta_q once the vapour counts
        s = 1.0 - p / p_int[0]
        T = to_T(295.0 + (2.0 * amp) * s + 80.0 * s ** 3)
        q = 0.03 * (p / p_int[0]) ** 3
    else:
        raise KeyError(name)
    return dict(t=np.ascontiguousarray(T), q=np.ascontiguousarray(q), p=p, p_int=p_int)


@functools.lru_cache(maxsize=None)
def case(name, nlay, ncol):
    """-> dict(t, q, p, p_int: the inputs; t_new, q_new, margin, mixed_top: the statement's).  Shared and read-only."""
    c = _inputs(name, nlay, ncol)
    c["t_new"], c["q_new"], c["margin"], c["mixed_top"] = statement(c["t"], c["q"], c["p"], c["p_int"])
    assert c["margin"] >= MIN_MARGIN, (name, nlay, ncol, c["margin"])
    acts_from = 30 if name == "moist" else 2      # layers from which the case has something to mix (never: "stable")
    if name == "stable":
        assert (c["mixed_top"] == -1).all()
    elif nlay >= acts_from:
        assert (c["mixed_top"] >= 0).all(), (name, nlay, ncol)
    if name == "moist" and nlay >= acts_from:
        dry = statement(c["t"], np.zeros_like(c["q"]), c["p"], c["p_int"])
        assert (dry[3] == -1).all() and (c["mixed_top"] >= 0).all(), "the vapour decides which layers mix"
    if name == "two_runs" and nlay >= 30:
        changed = np.abs(c["t_new"][:, 0] - c["t"][:, 0]) > 0
        runs = np.count_nonzero(np.diff(np.concatenate([[0], changed.astype(int), [0]])) == 1)
        assert runs == 2, runs
    for v in c.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return c


def rel_err(got, want):
    return float(np.max(np.abs(np.asarray(got) - want) / np.abs(want)))


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def column_sums(T, q, p_int, k=CONSTANTS):
    """-> (sum cp T dp, sum q dp) by column: what a mixing conserves."""
    dp = p_int[:-1] - p_int[1:]
    cp = k["cpd"] * (1.0 - q) + k["cvap"] * q
    return (cp * T * dp).sum(axis=0), (q * dp).sum(axis=0)
