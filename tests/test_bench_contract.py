"""bench.py's launch contract, as far as it can be checked without a GPU: `--gpus N` with N > 1 and no launcher must start
N ranks itself -- or refuse.  It must never print a line that says n_gpus: 1 when more GPUs were asked for."""
import os
import subprocess
import sys

from helpers import ROOT


def _run(args, env=None):
    e = dict(os.environ)
    for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT"):
        e.pop(k, None)
    e.update(env or {})
    return subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args, capture_output=True, text=True, timeout=300, env=e)


def test_more_gpus_than_the_box_has_is_refused():
    from climt_amd import _hip
    have = _hip.device_count()
    p = _run(["--gpus", str(have + 2), "--steps", "2"])
    assert p.returncode == 2, (p.returncode, p.stderr[-500:])
    assert "refusing" in p.stderr and not any(l.startswith("{") for l in p.stdout.splitlines())


def test_help_names_the_multi_gpu_knobs():
    p = _run(["--help"])
    assert p.returncode == 0
    for flag in ("--gpus", "--gather", "--no-unpack", "--rccl-channels", "--min-seconds", "--config", "--full", "--dump-outputs"):
        assert flag in p.stdout, flag


def _bench_module():
    import importlib.util
    spec = importlib.util.spec_from_file_location("_bench", os.path.join(ROOT, "bench.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_dump_outputs_writes_float64_and_samples_columns_past_the_limit(tmp_path):
    """--dump-outputs: every array as <name>.npy in float64; past the size limit the same seeded columns for every array,
    the same from call to call, and the files stay under the limit."""
    import numpy as np
    bench = _bench_module()
    rng = np.random.default_rng(3)
    arrays = {"a": rng.standard_normal((61, 1000)), "b": rng.standard_normal((60, 1000))}
    assert bench.dump_outputs(str(tmp_path / "whole"), arrays) is None
    for k, v in arrays.items():
        got = np.load(str(tmp_path / "whole" / (k + ".npy")))
        assert got.dtype == np.float64 and np.array_equal(got, v)
    limit = 200000
    cols = bench.dump_outputs(str(tmp_path / "s1"), arrays, limit=limit)
    again = bench.dump_outputs(str(tmp_path / "s2"), arrays, limit=limit)
    assert cols is not None and np.array_equal(cols, again) and np.all(np.diff(cols) > 0)
    assert sum(os.path.getsize(str(tmp_path / "s1" / (k + ".npy"))) for k in arrays) <= limit
    for k, v in arrays.items():
        got = np.load(str(tmp_path / "s1" / (k + ".npy")))
        assert np.array_equal(got, v[:, cols]) and np.array_equal(got, np.load(str(tmp_path / "s2" / (k + ".npy"))))


def test_spawned_ranks_fail_fast_and_print_no_line_without_a_gpu():
    """`--gpus 2 --share-device` starts two ranks of this script; on a box without a GPU both die at once and the parent
    must come back promptly with their exit code and no JSON line (never a made-up n_gpus)."""
    from climt_amd import _hip
    if _hip.device_count() > 0:
        import pytest
        pytest.skip("a GPU is present: the ranks would run")
    p = _run(["--gpus", "2", "--share-device", "--dist-backend", "gloo", "--comm", "torch", "--steps", "2"])
    assert p.returncode != 0
    assert not any(l.startswith("{") for l in p.stdout.splitlines())


def _line(p):
    import json
    lines = [l for l in p.stdout.splitlines() if l.startswith("{")]
    assert p.returncode == 0 and lines, (p.returncode, p.stderr[-800:])
    return json.loads(lines[-1])


def test_valu_issue_json_follows_the_committed_sq_pass():
    """profiles/valu_issue.json (what roofline.issue_frac is computed from): issue_cycles = 4 x (VALU - TRANS_F64) + 16 x TRANS_F64
    wave instructions, and it agrees with the hardware's own SQ_ACTIVE_INST_VALU (quad-cycles) of the same pass within 2 %."""
    import json
    j = json.load(open(os.path.join(ROOT, "profiles", "valu_issue.json")))
    kernels = {k: v for k, v in j.items() if isinstance(v, dict)}
    assert len(kernels) == 4 and j["source_hash"] == json.load(open(os.path.join(ROOT, "profiles", "hbm_traffic.json")))["source_hash"]
    for k, v in kernels.items():
        assert v["issue_cycles"] == 4.0 * (v["valu"] - v["trans_f64"]) + 16.0 * v["trans_f64"], k
        assert abs(4.0 * v["active_inst_valu_quad_cycles"] / v["issue_cycles"] - 1.0) < 0.02, k


import pytest  # noqa: E402


@pytest.mark.gpu
def test_plain_run_times_exactly_its_steps_and_dumps_the_last_one(tmp_path, gpu_ctx):
    """A plain run: one bracket of exactly --steps steps, the headline fields and nothing measured beyond them (those need
    --full); --dump-outputs writes the 12 arrays of the last timed step, and they are what a direct call computes on the
    same seeded columns."""
    import numpy as np
    from climt_amd._lib import LW_OUT, SW_OUT
    from climt_amd.synthetic import make_columns
    j = _line(_run(["--gpus", "1", "--steps", "5", "--warmup", "1", "--dump-outputs", str(tmp_path / "out")]))
    assert j["steps"] == 5 and j["warmup"] == 1 and j["config"]["brackets"] == 1
    assert abs(j["config"]["timed_region_s"] - 5 * j["ms_per_step"] * 1e-3) < 1e-9
    assert j["unit"] == "columns/s" and j["higher_is_better"] is True and j["dtype"] == "f64" and j["metric"]
    assert abs(j["value"] - 8192 / (j["ms_per_step"] * 1e-3)) < 1e-6 * j["value"]
    assert not {"roofline", "mcica", "roofline_mcica", "cpu_baseline", "extra"} & set(j)
    bench = _bench_module()
    c = make_columns(8192, 60, cloudy=False, seed=bench.SEED)
    c.update(bench.FLAGS)
    c.pop("lat")
    want = dict(gpu_ctx.sw_fluxes(c, mcica=False), **gpu_ctx.lw_fluxes(c, mcica=False))
    assert sorted(f[:-4] for f in os.listdir(str(tmp_path / "out"))) == sorted(k for k, _ in SW_OUT + LW_OUT)
    for k, lev in SW_OUT + LW_OUT:
        got = np.load(str(tmp_path / "out" / (k + ".npy")))
        assert got.dtype == np.float64 and got.shape == (60 + lev, 8192), k
        assert np.abs(got - want[k]).max() <= 1e-9 * max(1.0, np.abs(want[k]).max()), k


@pytest.mark.gpu
def test_line_carries_issue_fraction_bound_and_the_mcica_co_headline():
    """VERDICT r4 #2a / #5: `roofline.bound` stays the contract's roofline (hbm: what achieved / peak / frac are quoted against),
    `limiter` says what actually holds the kernel, every solve kernel has its VALU issue fraction, and configs[2] (McICA) is measured with the headline's
    own bracket discipline and has a top-level roofline object."""
    j = _line(_run(["--full", "--steps", "6", "--warmup", "1", "--min-seconds", "0.3", "--no-cpu-baseline", "--no-extra"]))
    r = j["roofline"]
    assert j["n_gpus"] == 1 and j["steps"] == 6 and j["dtype"] == "f64" and j["config"]["workload"] == "rrtmg_lw+sw_clear_sky_8192col_x_60lev_per_gpu"
    assert r["bound"] == "hbm" and "valu" in r["limiter"].lower() and r["unit"] == "GB/s" and abs(r["frac"] - r["achieved"] / r["peak"]) < 1e-12
    assert {"issue_frac", "issue_frac_serial", "traffic", "kernel_ms"} <= set(r)
    assert len(r["kernels"]) == 2 and all({"issue_frac_alone", "valu_issue_ms_per_simd", "limiter", "spectrum"} <= set(k) for k in r["kernels"])
    if r["counters_note"] is None:      # the committed counters belong to the library that ran
        assert 0.2 < r["issue_frac_serial"] < 1.0 and all(0.1 < k["issue_frac_alone"] < 1.0 for k in r["kernels"])
    # round 6: the line says which bytes it counts -- the contract's figure beside the arrays really handed over
    assert r["step_algorithmic_bytes_per_column"] == 43464 and r["algorithmic_bytes_shipped_per_column"] == 21864
    assert abs(r["step_frac_on_shipped_bytes"] / r["step_frac"] - 21864 / 43464) < 1e-12 and "step_issue_frac" in r
    assert r["hbm_rates_measured"]["write_read_mix_of_the_step"] < r["hbm_rates_measured"]["read_streaming"]
    m, rm = j["mcica"], j["roofline_mcica"]
    assert m["workload"] == "rrtmg_lw+sw_mcica_cloudy_8192col_x_60lev_per_gpu" and m["steps"] == j["steps"] and m["brackets"] >= 1
    assert m["timed_region_s"] >= 0.3 and 1.2 < m["ratio_to_clear_sky"] < 3.0 and abs(m["value"] - 8192 / (m["ms_per_step"] * 1e-3)) < 1e-6 * m["value"]
    assert "cloudy" in rm["kernel"] or "<true" in rm["kernel"]
    assert rm["bound"] == "hbm" and rm["limiter"] and len(rm["kernels"]) == 2


@pytest.mark.gpu
def test_one_run_measures_every_gather_mode():
    """VERDICT r4 #3b: the N>1 code path (forced with one rank on a one-GPU box) prints, from ONE run, columns/s per gather
    mode -- ncclAllGather, the direct grouped send/recv exchange, gather to root, none -- with the bytes a GPU receives per step,
    the rate achieved and the rate the compute alone would need."""
    j = _line(_run(["--full", "--force-dist", "--steps", "6", "--warmup", "1", "--min-seconds", "0.3", "--no-cpu-baseline", "--no-extra"]))
    g = j["gather_modes"]
    assert {"all", "direct", "root", "none"} <= set(g)
    for m in ("all", "direct", "root", "none"):
        assert {"value", "ms_per_step", "brackets", "ingress_bytes_per_gpu_per_step", "ingress_GBps_per_gpu_achieved",
                "ingress_GBps_per_gpu_needed_at_compute_rate", "slowdown_vs_none", "gather_ran"} <= set(g[m]), m
        assert g[m]["gather_ran"] == (m != "none") and g[m]["error"] is None
    assert j["config"]["gather_mode"] == "all" and j["config"]["communicator"].endswith("rccl")      # a FIXED headline mode
    assert j["comm_selftest"] == {"all": "OK", "direct": "OK", "root": "OK", "ranks": 1}      # every mode checked on a 1 KB pattern before the brackets
    assert abs(j["value"] - g[j["config"]["gather_mode"]]["value"]) < 1e-6 * j["value"]


@pytest.mark.gpu
def test_two_self_spawned_ranks_share_the_gpu_and_print_one_line():
    """`--gpus 2` without a launcher: bench.py starts its two ranks itself (here both on GPU 0, over torch/gloo with the testing
    communicator, because RCCL refuses two ranks on one device): ONE JSON line, n_gpus 2, value = columns of both ranks / the
    slowest rank's time, every gather mode measured with the bytes a rank receives per step (one peer's block)."""
    p = _run(["--full", "--gpus", "2", "--share-device", "--dist-backend", "gloo", "--comm", "torch", "--steps", "4", "--warmup", "1", "--min-seconds", "0.2",
              "--no-cpu-baseline", "--no-extra"])
    lines = [l for l in p.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, (p.returncode, p.stderr[-600:])
    j = _line(p)
    assert j["n_gpus"] == 2 and j["scaling"] == "weak" and j["config"]["communicator"].startswith("torch.")
    n = j["config"]["columns_per_gpu"]
    assert abs(j["value"] - 2 * n / (j["ms_per_step"] * 1e-3)) < 1e-6 * j["value"]
    g = j["gather_modes"]
    block = 8 * sum((60 + lev) * n for lev in (1, 1, 0, 1, 1, 0) * 2)
    for m in ("all", "direct", "root"):
        assert g[m]["gather_ran"] and g[m]["error"] is None and g[m]["ingress_bytes_per_gpu_per_step"] == block, m
    assert g["none"]["ingress_bytes_per_gpu_per_step"] == 0 and g["none"]["value"] > g["all"]["value"]
