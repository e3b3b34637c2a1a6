"""The N > 1 machinery on a one-GPU box (VERDICT r2 "Next" #1):

  * RCCL really executes: a world-size-1 `nccl` group (legal) is formed on the GPU and hudiff_amd.dist.gather_rows /
    bench.py's gather + all-reduce run through it -- communicator init with device_id, device tensors, torch's HIP runtime
    next to the library's own streams and graphs.
  * `python bench.py --gpus 2 ...` with NO launcher around it (the driver's command shape) starts two ranks by itself and
    the line reports the world size the process group formed.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu

NCCL_WORKER = r'''
import os, sys
import numpy as np
sys.path.insert(0, os.environ["HD_ROOT"]); sys.path.insert(0, os.path.join(os.environ["HD_ROOT"], "tests"))
import hudiff_amd
from hudiff_amd import dist as D
from hudiff_amd.sampler import Job, sample_jobs
from conftest import load_cfg, load_weights, load_golden, chain_or_none
import torch, torch.distributed as tdist
pg = D.init_process_group(force=True)                    # world size 1, backend nccl (= RCCL)
assert pg is not None and tdist.is_initialized() and tdist.get_backend() == "nccl" and tdist.get_world_size() == 1
cfg, sd = load_cfg("ab"), load_weights("ab")
model = hudiff_amd.AntiTFNet(**cfg, device=0)
model.load_state_dict(sd)
z = load_golden("micro_ab_sample_finetune.npz")
B, loc = z["tokens"].shape[0], z["loc"]
ch = chain_or_none(z)
jobs = [Job(tokens=z["tokens"][b], region=z["region"][b], loc=loc, chain=(int(ch[b]), int(ch[B + b]))) for b in range(B)]
# the library's streams / graphs run while torch's HIP runtime holds an RCCL communicator on the same device
res = sample_jobs(model, jobs, replicas=3, seed=5, device_batch=4)               # gather (dst = 0) through RCCL
res_all = sample_jobs(model, jobs, replicas=3, seed=5, device_batch=4, all_ranks=True)   # all_gather through RCCL
assert res.shape == (B, 1, 3, model.max_len) and np.array_equal(res, res_all)
D.shutdown()
assert not tdist.is_initialized()
plain = sample_jobs(model, jobs, replicas=3, seed=5, device_batch=4)             # no group: local reshape
assert np.array_equal(res, plain)
t = torch.ones(4, device="cuda") * 3                     # torch's runtime still healthy beside the library
assert float(t.sum()) == 12.0
model.close()
print("RCCL_OK", res.shape)
'''


def _clean_env(**extra):
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0", HD_ROOT=ROOT, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT", "HUDIFF_DIST_BACKEND"):
        env.pop(k, None)
    env.update(extra)
    return env


def _last_json(stdout):
    return json.loads([ln for ln in stdout.splitlines() if ln.startswith("{")][-1])


def test_rccl_world_size_1_gather(tmp_path):
    script = tmp_path / "nccl_worker.py"
    script.write_text(NCCL_WORKER)
    r = subprocess.run([sys.executable, str(script)], env=_clean_env(), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "RCCL_OK" in r.stdout, r.stdout[-2000:] + r.stderr[-3000:]


def test_bench_gather_and_allreduce_through_rccl(tmp_path):
    """bench.py with HUDIFF_BENCH_FORCE_PG=1: the exact collective code of an N > 1 run (nccl init with device_id, barrier,
    dist.gather of the device token tensor, MAX all-reduce of the timings) on one rank."""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "1", "--warmup", "0", "--batch", "24",
                        "--max-t", "2", "--no-cpu-baseline", "--traffic", "off"],
                       env=_clean_env(HUDIFF_BENCH_FORCE_PG="1"), cwd=str(tmp_path), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    line = _last_json(r.stdout)
    assert line["n_gpus"] == 1 and line["config"]["process_group"] == {"world_size": 1, "backend": "nccl"}
    assert line["all_tokens_valid"] and line["config"]["global_rows"] == 24


def test_bench_gpus_2_without_a_launcher(tmp_path):
    """The driver's command shape, `python bench.py --gpus 2 ...`: bench.py starts the two ranks itself (both on device 0
    here: HUDIFF_BENCH_SHARE_GPU=1 selects the gloo gather because RCCL refuses two ranks on one device)."""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "1", "--warmup", "0", "--batch", "24",
                        "--max-t", "2", "--no-cpu-baseline", "--traffic", "off"],
                       env=_clean_env(HUDIFF_BENCH_SHARE_GPU="1"), cwd=str(tmp_path), capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    line = _last_json(r.stdout)
    assert line["n_gpus"] == 2 and line["config"]["process_group"]["world_size"] == 2 and line["config"]["global_rows"] == 48
    assert line["all_tokens_valid"] and line["scaling"] == "weak"
    pr = line["per_rank_ms_per_step"]                    # a straggler rank is visible (VERDICT r3 "Next" #7)
    assert len(pr["ranks"]) == 2 and pr["min"] <= pr["max"] and abs(pr["max"] - line["ms_per_step"]) < 0.05 * line["ms_per_step"] + 50


def test_bench_gpus_2_reports_rank_0_counters(tmp_path):
    """N > 1 lines carry HBM traffic / GB/s / MFMA-busy too (north_star: "rocprof-reported HBM GB/s and MFMA utilisation ... at
    1/2/4/8 GPUs"): rank 0 profiles a single-rank run of the per-GPU workload while the other rank waits at the final barrier."""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "1", "--warmup", "0", "--batch", "24",
                        "--no-cpu-baseline", "--full"], env=_clean_env(HUDIFF_BENCH_SHARE_GPU="1"), cwd=str(tmp_path), capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    line = _last_json(r.stdout)
    roof = line["roofline"]
    assert line["n_gpus"] == 2 and line["config"]["global_rows"] == 48 and line["all_tokens_valid"]
    assert roof["traffic"] and roof["traffic"] > 1e8 and roof["hbm_gbps"] > 10 and 0.0 < roof["mfma_busy"] < 1.0
    assert "rank 0" in roof["pmc_note"] and "N = 2" in roof["pmc_note"]
    assert "split_precision" not in line and "cpu_baseline" not in line          # N > 1: the metric's own leg only


def test_default_bench_line_carries_the_measurement_contract(tmp_path):
    """One `python bench.py --full` run (smaller batch, bounded CPU leg): the single JSON line must hold everything the
    measurement contract names -- metric / value / unit / n_gpus / steps / warmup / ms_per_step / dtype / config.workload; `roofline`
    with bound, achieved, peak, frac, traffic (live PMC), hbm_gbps and mfma_busy; `cpu_baseline` with value / cores / kind / sample.
    Round 4 (VERDICT r3 "Next" #2): the top level is the split route and says so (`dtype`, `precision_route`, peak 2500 / 3); the
    all-fp32 line is sampled as long as the top level and has its own PMC passes; `precision_evidence` compares both routes with a
    float64 CPU evaluation at three points of the sample and counts token agreement over all timed samples."""
    env = _clean_env()
    for k in ("HUDIFF_X3", "HUDIFF_ATTN_X3", "HUDIFF_PRECISION"):       # the DEFAULT line is what is checked, also inside the nested f32_all re-run
        env.pop(k, None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--batch", "64", "--steps", "2", "--warmup", "0",
                        "--cpu-rows", "2", "--cpu-steps", "2", "--evidence-rows", "2", "--full"], env=env, cwd=str(tmp_path), capture_output=True, text=True, timeout=1500)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1                                      # ONE JSON line
    d = json.loads(lines[0])
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline", "dtype", "data", "config"):
        assert k in d, k
    assert d["n_gpus"] == 1 and d["unit"] == "sequences/s" and d["vs_baseline"] is None and d["higher_is_better"] is True
    assert d["precision_route"] == "split" and "fp16 hi+lo split, 3 MFMA / product" in d["dtype"] and "pruned tail + static branch f32" in d["dtype"]
    assert "HuAb348" in d["metric"] and "workload" in d["config"] and d["config"]["rows_per_gpu"] == 64
    roof = d["roofline"]
    assert roof["bound"] == "mfma" and roof["unit"].startswith("TFLOP/s") and abs(roof["frac"] - roof["achieved"] / roof["peak"]) < 1e-3
    assert roof["traffic"] and roof["traffic"] > 1e9 and roof["hbm_gbps"] > 100 and 0.05 < roof["mfma_busy"] < 1.0
    assert roof["route"] == "split" and abs(roof["peak"] - 2500 / 3) < 0.01
    pi = d["precision_info"]
    assert (pi["precision"], pi["split_built"], pi["split_in_use"], pi["range_fallbacks"], pi["lnsync_fallbacks"]) == ("split", 3, True, 0, 0)
    cpu = d["cpu_baseline"]
    assert cpu["kind"] == "port" and cpu["value"] > 0 and cpu["cores"] >= 1 and cpu["unit"] == "sequences/s" and cpu["sample"]
    a = d["all_fp32_kernels"]
    assert a["steps"] == d["steps"] == 2                       # sampled as long as the top level
    assert a["roofline"]["peak"] == 157.3 and a["precision_info"]["split_built"] == 0 and a["precision_info"]["precision"] == "f32_all"
    assert a["roofline"]["traffic"] and a["roofline"]["hbm_gbps"] > 100 and 0.05 < a["roofline"]["mfma_busy"] < 1.0      # its own PMC passes
    assert a["roofline"].get("clock_power") is None or a["roofline"]["clock_power"]["sclk_mhz_median"] > 500
    assert a["token_agreement_with_top_level"] == {"rows_identical": 128, "rows_compared": 128, "samples_compared": 2}
    g = d["f32_gemm_route"]
    assert g["precision_info"]["precision"] == "f32_gemm" and 157.3 < g["roofline"]["peak"] < 175
    ev = d["precision_evidence"]
    assert len(ev["steps_along_the_sample"]) == 3 and ev["steps_along_the_sample"][0] == 0 and ev["bound"] == 1e-4
    for route in ("split", "f32_all"):
        e = ev["max_abs_dlogit_vs_float64"][route]
        assert len(e["per_step"]) == 3 and 0.0 < e["max"] < 1e-4, (route, e)
    assert ev["token_agreement"]["split vs f32_all"]["rows_identical"] == 128
    nb = d["secondary"]["hudiff_nb_configs3"]
    assert nb["split"]["value"] > 0 and nb["f32_all"]["value"] > 0 and "configs[3]" in nb["config"]["workload"]
    assert d["all_tokens_valid"]
