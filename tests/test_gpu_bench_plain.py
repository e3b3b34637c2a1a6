"""A plain `python bench.py` run is the metric's own leg only, and --dump-outputs writes what its last timed sample returned.

The legs that take runs of their own (other routes, precision evidence, the HuDiff-Nb line, live PMC passes, CPU baseline) are
behind --full (tests/test_gpu_dist.py checks that line).  Two plain runs with the same arguments must dump the same tokens: inputs,
weights and noise keys depend only on the arguments, so builds can be compared output for output.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu


def _env():
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0", PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT", "HUDIFF_DIST_BACKEND", "HUDIFF_BENCH_FORCE_PG",
              "HUDIFF_BENCH_SHARE_GPU"):
        env.pop(k, None)
    return env


def test_plain_bench_line_is_the_metric_alone_and_dumps_its_tokens(tmp_path):
    lines, dumps = [], []
    for n in range(2):
        out = tmp_path / f"dump{n}"
        r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--batch", "24", "--steps", "2", "--warmup", "1",
                            "--dump-outputs", str(out)], env=_env(), cwd=str(tmp_path), capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
        js = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
        assert len(js) == 1
        lines.append(json.loads(js[0]))
        dumps.append(np.load(out / "tokens.npy"))
    for d in lines:
        for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
            assert k in d, k
        assert d["steps"] == 2 and d["warmup"] == 1 and d["n_gpus"] == 1 and d["unit"] == "sequences/s" and d["higher_is_better"] is True
        assert d["ms_per_step"] > 0 and abs(d["value"] - 24 * 1e3 / d["ms_per_step"]) < 1e-3 * d["value"] + 1e-3
        for k in ("all_fp32_kernels", "f32_gemm_route", "precision_evidence", "secondary", "cpu_baseline"):
            assert k not in d, k
        assert d["roofline"]["traffic"] is None and d["all_tokens_valid"]
    for t in dumps:
        assert t.dtype == np.float32 and t.shape == (24, 291)
        assert (t == np.round(t)).all() and t.min() >= 0 and t.max() <= 21       # a full sample: every masked slot filled
    assert np.array_equal(dumps[0], dumps[1])
