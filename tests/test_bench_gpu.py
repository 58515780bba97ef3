"""The measurement contract of bench.py as the driver parses it: ONE JSON line, the contract's keys, and a `roofline` object that STARTS with
scalars (the driver's record keeps its first ~23 keys and drops unknown top-level keys: VERDICT r05 weak #4).  A plain run carries the
headline alone; `--full` adds the legs that take runs of their own."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

gpu = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

HEADLINE = ["metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline", "dtype", "data",
            "config"]
FULL_ONLY = ["roofline", "roofline_stage1", "cpu_baseline", "exact_mode", "exact_value", "latency", "train_step", "pnp", "operand_range",
             "dead_layer1_computed", "phases_ms", "sharded_leg"]
CONTRACT = ["metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline", "dtype", "data",
            "config", "roofline", "cpu_baseline"]
ROOFLINE_HEAD = ["bound", "achieved", "peak", "unit", "frac", "traffic"]
ROOFLINE_SCALARS = ["frac_algorithmic", "dominant_ms", "dominant_frac_algorithmic", "dominant_frac_executed", "stage1_hbm_frac", "stage1_kernel_ms",
                    "exact_value", "exact_direct_value", "latency_ms_per_image", "train_step_ms", "kernel_ms_per_step", "share_of_step",
                    "launches_per_step", "value_with_dead_layer1_computed", "useful_tflops", "step_direct_conv_equiv_tflops"]


@gpu
def test_bench_line_contract_on_a_small_workload(tmp_path):
    """`python bench.py --workload full_b8_n42_vits --steps 2 --warmup 1 --full --no-latency-leg --dump-outputs DIR` (a child process): the
    line a driver reads, and the last timed step's outputs as DIR/<name>.npy."""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--workload", "full_b8_n42_vits", "--steps", "2", "--warmup", "1",
                        "--full", "--no-latency-leg", "--dump-outputs", str(tmp_path)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600,
                       cwd=ROOT)
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    lines = [ln for ln in r.stdout.decode().splitlines() if ln.strip()]
    assert len(lines) == 1, lines
    d = json.loads(lines[0])
    for k in CONTRACT:
        assert k in d, k
    assert d["unit"] == "crops/s" and d["n_gpus"] == 1 and d["steps"] == 2 and d["warmup"] == 1 and d["higher_is_better"] is True
    assert d["vs_baseline"] is None and d["data"] == "synthetic" and d["value"] > 0 and abs(d["value"] - 8 / (d["ms_per_step"] * 1e-3)) < 1e-6 * d["value"]
    assert d["config"]["workload"].startswith("full_b8_n42_vits") and d["config"]["input_batches"] == 2 and d["config"]["prefetch_query"] is True
    roof = d["roofline"]
    keys = list(roof)
    assert keys[:6] == ROOFLINE_HEAD, keys[:6]
    assert roof["bound"] == "mfma" and roof["unit"] == "TFLOP/s" and abs(roof["frac"] - roof["achieved"] / roof["peak"]) < 1e-9
    head = keys[:23]
    for k in ROOFLINE_SCALARS:
        assert k in head, (k, head)
    for k in head[1:]:
        assert k in ("unit",) or roof[k] is None or isinstance(roof[k], (int, float)), (k, roof[k])       # scalars first, strings after
    for k in keys[23:]:
        if isinstance(roof[k], str):
            assert len(roof[k]) <= 100, (k, len(roof[k]))
    assert roof["exact_value"] == d["exact_value"] and roof["stage1_hbm_frac"] == d["roofline_stage1"]["frac"]
    assert roof["value_with_dead_layer1_computed"] == d["dead_layer1_computed"]["value"] and d["config"]["dpt_layer1_branch"].startswith("not computed")
    cb = d["cpu_baseline"]
    assert cb["kind"] == "port" and cb["value"] > 0 and cb["cores"] >= 1 and cb["unit"] == "crops/s" and isinstance(cb["sample"], str)
    x = d["exact_mode"]["f16x3_vs_exact"]
    assert x["pairs_with_same_template"] > 0 and x["flow_max_abs_px"] < 1e-2 and x["keypoint_slots_equal"] > 0.999
    # --dump-outputs: the hypotheses' Net.forward outputs and the batched PnP/RANSAC results of the last timed step (hyp 5, batch 8)
    dumped = {n: np.load(os.path.join(str(tmp_path), n + ".npy")) for n in d["dump_outputs"]["arrays"]}
    assert dumped["pred_poses"].shape == (5, 8, 4, 4) and dumped["tem_pose"].shape == (5, 8, 4, 4) and dumped["pnp_rot"].shape == (5, 8, 3, 3)
    assert dumped["pnp_tvec"].shape == (5, 8, 3, 1) and dumped["pnp_success"].shape == (5, 8) and dumped["pred_tar_pts"].shape[:2] == (5, 8)
    assert all(v.dtype in (np.float32, np.float64) and np.isfinite(v).all() for v in dumped.values())
    ok = dumped["pnp_success"] > 0
    assert ok.any() and np.abs(np.linalg.det(dumped["pnp_rot"][ok]) - 1).max() < 1e-5      # the PnP poses of the step, not zeros


@gpu
def test_bench_plain_run_carries_the_headline_alone(tmp_path):
    """`python bench.py --workload full_b8_n42_vits --steps 2 --warmup 1 --dump-outputs DIR` without --full: the headline's keys, the
    whole-step FLOP rate, the last timed step's outputs — and none of the legs that run steps of their own after the timed region."""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--workload", "full_b8_n42_vits", "--steps", "2", "--warmup", "1",
                        "--dump-outputs", str(tmp_path)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    lines = [ln for ln in r.stdout.decode().splitlines() if ln.strip()]
    assert len(lines) == 1, lines
    d = json.loads(lines[0])
    for k in HEADLINE:
        assert k in d, k
    for k in FULL_ONLY:
        assert k not in d, k
    assert d["unit"] == "crops/s" and d["n_gpus"] == 1 and d["steps"] == 2 and d["warmup"] == 1 and d["higher_is_better"] is True
    assert d["value"] > 0 and abs(d["value"] - 8 / (d["ms_per_step"] * 1e-3)) < 1e-6 * d["value"] and d["config"]["full"] is False
    assert d["metric"].startswith("image-crops/sec") and d["dtype"].startswith("f32 tensors") and d["mfma"]["useful_tflops"] > 0
    dumped = {n: np.load(os.path.join(str(tmp_path), n + ".npy")) for n in d["dump_outputs"]["arrays"]}
    assert dumped["pred_poses"].shape == (5, 8, 4, 4) and dumped["pnp_rot"].shape == (5, 8, 3, 3) and dumped["pnp_success"].shape == (5, 8)
    assert all(v.dtype in (np.float32, np.float64) and np.isfinite(v).all() for v in dumped.values())
    ok = dumped["pnp_success"] > 0
    assert ok.any() and np.abs(np.linalg.det(dumped["pnp_rot"][ok]) - 1).max() < 1e-5


@gpu
def test_bench_steps_and_dumped_outputs_repeat(tmp_path):
    """--steps sets the number of timed steps, and two runs with the same arguments compute the same outputs (seeded inputs): the
    stage-1 workload of BASELINE configs[1], run twice."""
    lines = []
    for run in ("a", "b"):
        r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--workload", "stage1_b8_n42_c384", "--steps", "3", "--warmup", "1",
                            "--no-cpu-baseline", "--dump-outputs", str(tmp_path / run)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300, cwd=ROOT)
        assert r.returncode == 0, r.stderr.decode()[-2000:]
        lines.append(json.loads(r.stdout.decode().strip().splitlines()[-1]))
    for d in lines:
        assert d["steps"] == 3 and d["ms_per_step"] > 0 and abs(d["value"] - 8 / (d["ms_per_step"] * 1e-3)) < 1e-6 * d["value"]
    a = {n: np.load(str(tmp_path / "a" / (n + ".npy"))) for n in ("score", "index")}
    b = {n: np.load(str(tmp_path / "b" / (n + ".npy"))) for n in ("score", "index")}
    assert a["score"].shape == (8, 5) and a["index"].shape == (8, 5) and a["index"].dtype == np.float32
    assert np.array_equal(a["index"], b["index"]) and np.abs(a["score"] - b["score"]).max() <= 1e-6
