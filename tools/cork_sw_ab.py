#!/usr/bin/env python3
"""The table-driven correlated-k shortwave (rrtmg_hip_cork_shortwave): what a call costs, device resident, at the shape of the
longwave's A/B (tools/cork_ab.py: 8192 columns x 30 and 60 layers).

    timeout -k 10 300 python tools/cork_sw_ab.py [--ncol 8192] [--nlays 30,60] [--repeats 5] [--batch 10] [--out profiles/cork_sw_ab.txt]

Tables: tests/golden/cork_sw_table_sw_earth.npz (3 bands x 2 g-points, rank 6, float32, Rayleigh: cork_sw_band_kernel<2, float>) and
cork_sw_table_sw_g16.npz (1 band x 16 g-points: the 256-VGPR instantiation).  Inputs: the sunlit atmosphere of tests/cork_sw_cases.py
(130 columns of their own numbers, repeated), cloud in every third layer.  Per shape and arm: device pointers, deferred mode,
`batch` calls enqueued back to back and ONE synchronise behind them, `repeats` times after a warm-up: median, min, max in ms per
call, and ns per (column, band, g-point, layer).
  all   every diagnostic written, the cloud arrays read
  lean  up, dn and tend only, no cloud arrays
Before timing, the device result of the first 128 columns is compared with the numpy statement at 1e-11 (the tolerance scale of
the `cloudy` case).  The lines go to stdout and to --out.  Fails where there is no GPU: no fall-back."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ncol", type=int, default=8192)
    ap.add_argument("--nlays", default="30,60")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--batch", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cork_sw_ab.txt"))
    a = ap.parse_args()
    from climt_amd import _hip, cork
    from climt_amd._lib import Context
    from climt_amd.build import source_hash
    import cork_cases as L
    import cork_sw_cases as S
    lines = []

    def say(text):
        print(text, flush=True)
        lines.append(text)
    ctx = Context(0)
    say("# tools/cork_sw_ab.py: rrtmg_hip_cork_shortwave, device resident, library src:%s" % source_hash())
    ncol = a.ncol
    for case, table in (("night", "sw_earth"), ("g16", "sw_g16")):
        kt = cork.KTable(S.table_path(table), kind="shortwave")
        tab, handle, nband = S.table(table), None, kt.nband
        handle = kt.upload(ctx)
        say("%s: %d bands x %d g-points, rank %d, %s" % (table, nband, kt.ngpt, kt.k.ndim, kt.k.dtype))
        for nlay in (int(x) for x in a.nlays.split(",")):
            base = {k: v for k, v in S._inputs(case, 30, 130).items()}
            if nlay != 30:      # (the pressures of the cases at another depth; the profiles interpolated in the layer index)
                p_int = L.pressures(nlay, 130)
                at = np.linspace(0.0, 29.0, nlay)
                lay = lambda x: np.stack([np.interp(at, np.arange(30.0), x[:, i]) for i in range(130)], axis=1)
                base.update(p_int=p_int, p=0.5 * (p_int[:-1] + p_int[1:]), t=lay(base["t"]), **{g: lay(base[g]) for g in S.gas_names(case)})
            reps = -(-ncol // 130)
            tile = lambda x: np.ascontiguousarray(np.tile(x, reps)[..., :ncol])
            c = {k: tile(base[k]) for k in ("t", "p", "p_int", "albedo", "earth_sun") + tuple(S.gas_names(case))}
            col = np.arange(ncol)
            c["zenith"] = 0.1 + 1.2 * np.mod(0.6180339887498949 * (col % 130 + 1), 1.0)
            lev = np.arange(nlay)[:, None, None]
            on = ((lev + col[None, :, None]) % 3 == 0) * np.ones((nlay, ncol, nband))
            c.update(taucld=on * 2.0, ssacld=on * 0.95, asycld=on * 0.85)
            ns = min(128, ncol)
            cs = {k: np.ascontiguousarray(v[:, :ns, :] if k in S.CLOUD else v[..., :ns]) for k, v in c.items()}
            want = S.statement(tab, cs)
            dev = {k: _hip.DeviceArray.from_host(np.ascontiguousarray(v)) for k, v in c.items()}
            shapes = dict(up=(nlay + 1, ncol), dn=(nlay + 1, ncol), tend=(nlay, ncol), hr=(nlay, ncol), up_band=(nband, nlay + 1, ncol), dn_band=(nband, nlay + 1, ncol),
                          tau_band=(nband, nlay, ncol), hr_band=(nband, nlay, ncol))
            out = {n: _hip.DeviceArray(s) for n, s in shapes.items()}
            head = (handle, nband, dev["t"], dev["p"], dev["p_int"], dev["zenith"], dev["albedo"], dev["earth_sun"], dict(m_h2o=S.M_H2O, g=S.G, cpd=S.CPD), kt.gas_rule)
            kw = dict(gases=[dev[g] for g in S.gas_names(case)], gas_scale=kt.gas_scale, up=out["up"], dn=out["dn"], tend=out["tend"], memspace=1, ncol=ncol, nlay=nlay)

            def every():
                ctx.cork_shortwave(*head, cloud=tuple(dev[n] for n in S.CLOUD), diagnostics={n: out[n] for n in S.FIELDS[3:]}, **kw)

            def lean():
                ctx.cork_shortwave(*head, diagnostics=None, **kw)
            every()
            ctx.synchronize()
            got = {n: np.ascontiguousarray(out[n].download().reshape(shapes[n])[..., :ns]) for n in S.FIELDS}
            d = S.deviations(got, want, S.FIELDS)
            assert max(d.values()) <= 1e-11, d

            def timed(fn):
                ctx.synchronize()
                t0 = time.perf_counter()
                for _ in range(a.batch):
                    fn()
                ctx.synchronize()
                return (time.perf_counter() - t0) * 1e3 / a.batch
            work_mb = 8.0 * nband * kt.ngpt * 3 * (nlay + 1) * ncol / 1e6
            say("  %d x %d (largest deviation of the first %d columns from the statement %.1e; work space %.1f MB, one chunk)" % (ncol, nlay, ns, max(d.values()), work_mb))
            ctx.set_deferred(True)
            for label, fn in (("all diagnostics, cloud arrays", every), ("up, dn, tend only", lean)):
                timed(fn)
                t = [timed(fn) for _ in range(a.repeats)]
                m = float(np.median(t))
                say("      %-30s median %8.4f ms   min %8.4f ms   max %8.4f ms;  %.2f ns per column, band, g-point and layer" % (
                    label, m, min(t), max(t), m * 1e6 / (float(ncol) * nband * kt.ngpt * nlay)))
            ctx.set_deferred(False)
        ctx.cork_table_destroy(handle)
    ctx.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
