#!/usr/bin/env python
"""bench.py -- humanized sequences / second (full T-step sample), the BASELINE.json metric.

    python bench.py --gpus N --steps K --warmup W
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 \
        --master-port P bench.py --gpus N --steps K --warmup W

A "step" is one complete T-step humanization sample of one batch of B = 256 independent rows per GPU
(BASELINE.json configs[1]: HuDiff-Ab on HuAb348, batch 256, 1 x MI355X): up to 154 denoiser forwards of the
39.8 M-parameter AntiTFNet over 291 slots + the exponential-race resampling, with inference-time dropout as
the reference runs it.  Rows are the 348 HuAb348 mouse pairs (pre-slotted integer fixture hudiff_amd/data/real_rows.npz,
scripts/make_real_rows.py; global row g = pair g % 348, replica g // 348, ragged T = 141..154) -- `--data synthetic`
gives the HuAb348-shaped random rows of round 1 instead.  Weights are seeded random weights of the exact production
architecture (no released checkpoint offline).  Rows shard across GPUs with no data-path collective; one RCCL gather
of the final int32 tokens ends the job (weak scaling: 256 rows per GPU).

Precision routes (include/hudiff_hip.h): the top level is the library's DEFAULT route -- split precision since round 4: every
fp32 product of the large GEMMs and of the attention core as three fp16 MFMAs on fp16 (hi, lo) operand splits with fp32
accumulation (`dtype` says so, `roofline.peak` = 2500 / 3 TFLOP/s fp32-equivalent).

A plain run times the metric's own leg only: set up, warm up, time --steps samples, print the line.  `--full` adds everything
else the line can carry, each a run of its own after the timed region: `all_fp32_kernels` (the same workload with every
product on the fp32 MFMA pipe, sampled as long as the top level, with its own PMC passes and clock / power record),
`f32_gemm_route`, `precision_evidence` (for this very run's rows and weights, each route's max |dlogit| against a float64 CPU
evaluation at three points along the sample and the token agreement between the routes over ALL timed samples), the HuDiff-Nb
`secondary` line, the live PMC figures of `roofline` (traffic, hbm_gbps, mfma_busy) and `cpu_baseline`.

`--dump-outputs DIR` writes what the timed path returned for its last sample -- the final tokens of every row, gathered over
the ranks -- as DIR/tokens.npy (float32 [rows, L]).  Inputs, weights and noise keys depend only on the arguments, so two
builds run with the same arguments can be compared output for output.

Timed region: inputs already resident in HBM (hd_sample_begin uploaded them); K x [restore tokens
device-side, re-key noise, run all T steps]; bracketed by barrier + device synchronise on both sides,
max over ranks.  One JSON line is printed by rank 0.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)
os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")   # RCCL needs dmabuf IPC on this driver stack

PEAK_F32_MATRIX_TFLOPS = 157.3     # /opt/skills/guides/MI355X_MICROARCH.md "Peak FP32 (matrix)"


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=2)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--batch", type=int, default=256, help="rows per GPU")
    ap.add_argument("--kind", choices=["ab", "nb"], default="ab")
    ap.add_argument("--mode", default=None, help="ab: finetune|pretrain, nb: plain|inpaint")
    ap.add_argument("--dropout", choices=["faithful", "off"], default="faithful")
    ap.add_argument("--max-t", type=int, default=0, help="truncate every row to this many denoiser steps "
                    "(profiling aid; the JSON line is then marked truncated and is NOT the metric)")
    ap.add_argument("--data", choices=["auto", "real", "synthetic"], default="auto",
                    help="real = rows of the reference's evaluation set (HuAb348 / VHH, hudiff_amd/data/real_rows.npz); "
                         "auto = real when the fixture is present")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--cpu-rows", type=int, default=16, help="rows of the 'best batch' CPU leg (B = 1 is always timed too)")
    ap.add_argument("--cpu-steps", type=int, default=16)
    ap.add_argument("--pmc", "--traffic", dest="pmc", choices=["auto", "live", "off"], default="auto",
                    help="roofline.traffic / hbm_gbps / mfma_busy: live = two rocprofv3 --pmc passes (FETCH_SIZE | WRITE_SIZE + "
                         "SQ_VALU_MFMA_BUSY_CYCLES + GRBM_GUI_ACTIVE) over a 4-step run of this script in a subprocess after the timed region")
    ap.add_argument("--cpu-impl", choices=["auto", "torch", "numpy"], default="auto",
                    help="CPU baseline on the oracle's PyTorch-CPU variant (auto: when torch is importable) or on numpy")
    ap.add_argument("--precision", choices=["default", "split", "f32_gemm", "f32_all"], default="default",
                    help="precision route of the TOP-LEVEL line (hd_set_precision); default = the library default (split)")
    ap.add_argument("--no-split-line", action="store_true", help=argparse.SUPPRESS)      # round-3 flag (the split route is the top level now): accepted, ignored
    ap.add_argument("--no-f32-gemm-line", action="store_true",
                    help="skip the short `f32_gemm_route` leg (fp32 MFMA GEMMs + split attention core: the round-3 default route)")
    ap.add_argument("--no-secondary", action="store_true", help="skip the HuDiff-Nb line (BASELINE configs[3]) printed beside the metric")
    ap.add_argument("--no-all-fp32-line", action="store_true", help="skip the `all_fp32_kernels` leg (every product on the fp32 MFMA pipe, same --steps)")
    ap.add_argument("--no-evidence", action="store_true", help="skip `precision_evidence` (float64 CPU evaluations: ~1 min)")
    ap.add_argument("--evidence-rows", type=int, default=8, help="rows evaluated in float64 per point of `precision_evidence`")
    ap.add_argument("--only-main", action="store_true", help="the metric's own leg only (what the PMC passes profile)")
    ap.add_argument("--no-graph", action="store_true")
    ap.add_argument("--loop-graph", action="store_true", help="the whole T-step loop of a lane as ONE hipGraph (HD_LOOP_GRAPH) "
                    "instead of T replays of the step graph")
    ap.add_argument("--lanes", type=int, default=2, choices=[1, 2],
                    help="2 = the batch runs as two concurrent half-batches on two streams (library default)")
    ap.add_argument("--full", action="store_true",
                    help="also run the other routes' legs, precision_evidence, the HuDiff-Nb secondary line, the live PMC passes and the "
                         "CPU baseline after the timed region (the --no-* switches above pick among them); off: the metric's own leg only")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write the final tokens of the last timed sample (all ranks' rows) to DIR/tokens.npy as float32")
    return ap.parse_args()


def physical_cores():
    """Physical cores of the host ((physical id, core id) pairs of /proc/cpuinfo), logical CPUs."""
    logical = os.cpu_count() or 1
    try:
        seen, phys, core = set(), None, None
        for line in open("/proc/cpuinfo"):
            if line.startswith("physical id"):
                phys = line.split(":")[1].strip()
            elif line.startswith("core id"):
                core = line.split(":")[1].strip()
            elif not line.strip():
                if phys is not None and core is not None:
                    seen.add((phys, core))
                phys = core = None
        return (len(seen) or logical), logical
    except OSError:
        return logical, logical


class ClockPowerSampler:
    """Shader clock and package power of the GPU this rank runs on, read from the amdgpu hwmon files (freq1_input in Hz,
    power1_input in uW) every 100 ms by a thread while the timed region runs.  Both paths sit on the package power limit
    (DESIGN.md section 9), so the sustained clock -- not the 2.4 GHz of the peak figure -- is what the matrix pipe ran at."""

    def __init__(self, device):
        import threading
        self.dir, self.f, self.p, self._stop, self._t = None, [], [], threading.Event(), None
        try:
            import ctypes, glob
            hip = ctypes.CDLL("libamdhip64.so")
            buf = ctypes.create_string_buffer(64)
            if hip.hipDeviceGetPCIBusId(buf, 64, int(device)) == 0:
                d = glob.glob(f"/sys/bus/pci/devices/{buf.value.decode().lower()}/hwmon/hwmon*")
                if d and os.path.exists(os.path.join(d[0], "freq1_input")) and os.path.exists(os.path.join(d[0], "power1_input")):
                    self.dir = d[0]
        except (OSError, AttributeError):
            pass
        if self.dir:
            self._t = threading.Thread(target=self._run, daemon=True)

    def _read(self, name):
        with open(os.path.join(self.dir, name)) as fh:
            return float(fh.read().strip())

    def _run(self):
        while not self._stop.wait(0.1):
            try:
                self.f.append(self._read("freq1_input") * 1e-6)
                self.p.append(self._read("power1_input") * 1e-6)
            except (OSError, ValueError):
                return

    def start(self):
        if self._t:
            self._t.start()
        return self

    def stop(self):
        if not self._t:
            return None
        self._stop.set()
        self._t.join()
        busy = [(f, p) for f, p in zip(self.f, self.p) if p > 500.0] or list(zip(self.f, self.p))
        if not busy:
            return None
        med = lambda v: float(sorted(v)[len(v) // 2])
        out = {"sclk_mhz_median": round(med([f for f, _ in busy]), 1), "power_w_median": round(med([p for _, p in busy]), 1),
               "samples": len(busy)}
        try:
            out["power_cap_w"] = round(self._read("power1_cap") * 1e-6, 1)
        except (OSError, ValueError):
            pass
        return out


def make_batch(kind, B, mode, row0, data):
    from hudiff_amd import evalsets as E
    from hudiff_amd import synthetic as S
    if data == "real" or (data == "auto" and E.available()):
        return E.eval_batch("huab348" if kind == "ab" else "vhh", B, mode=mode, row0=row0, seed=2023), True
    return S.synthetic_batch(kind, B, seed=2023, mode=mode, row0=row0), False


def core_groups(per_group):
    """Disjoint groups of `per_group` logical CPUs, one hardware thread per physical core, neighbours in (package, core id) order --
    i.e. inside one NUMA node as far as the group size allows.  From /sys/devices/system/cpu/cpu*/topology; None if unreadable."""
    try:
        allowed = sorted(os.sched_getaffinity(0))
        first = {}
        for c in allowed:
            base = f"/sys/devices/system/cpu/cpu{c}/topology/"
            key = (int(open(base + "physical_package_id").read()), int(open(base + "core_id").read()))
            first.setdefault(key, c)                       # the first hardware thread of every physical core
        cpus = [first[k] for k in sorted(first)]
        return [cpus[i:i + per_group] for i in range(0, len(cpus) - per_group + 1, per_group)]
    except (OSError, ValueError, AttributeError):
        return None


def _cpu_worker(kind, cfg, wseed, mode, data, rows, row0, steps, threads, cpus, ready, go, out, idx):
    """One process of the all-cores CPU leg: `threads` PyTorch threads pinned to `cpus`, its own rows of the workload."""
    try:
        if cpus:
            os.sched_setaffinity(0, cpus)
        os.environ["OMP_NUM_THREADS"] = str(threads)
        sys.path.insert(0, os.path.join(ROOT, "oracle"))
        import torch
        torch.set_num_threads(threads)
        import hudiff_oracle as ho
        import hudiff_oracle_torch as hot
        from hudiff_amd import synthetic as S
        sd = S.random_state_dict(kind, cfg, seed=wseed)
        net = hot.TorchOracleNet(kind, cfg, sd)
        batch, _ = make_batch(kind, rows, mode, row0, data)

        def run(n_steps):
            t0 = time.perf_counter()
            ho.sample(net, batch["tokens"], batch["region"], batch["chain"], batch["order"], np.minimum(batch["T"], n_steps), seed=1,
                      row0=row0, dropout_mode="philox")
            return time.perf_counter() - t0
        run(1)
        ready.release()
        go.wait()
        t0 = time.time()
        dt = run(steps)
        out.put((idx, t0, t0 + dt, dt))
    except Exception as e:                               # never leave the parent waiting
        ready.release()
        out.put((idx, 0.0, 0.0, repr(e)))


def cpu_all_cores(kind, cfg, wseed, mode, rows, steps, mean_T, data, threads_per_proc=16, budget_s=150.0):
    """The host's best: P = physical cores / 16 processes x 16 threads, each pinned to its own cores, over disjoint rows of the same
    workload (rows are independent; VERDICT r5 "Next" #8).  -> dict or None (no torch, no topology, fewer than two groups)."""
    import multiprocessing as mp
    groups = core_groups(threads_per_proc)
    if not groups or len(groups) < 2:
        return None
    ctx = mp.get_context("spawn")
    ready, go, out = ctx.Semaphore(0), ctx.Event(), ctx.Queue()
    procs = [ctx.Process(target=_cpu_worker, args=(kind, cfg, wseed, mode, data, rows, 4096 + i * rows, steps, threads_per_proc, g, ready, go, out, i),
                         daemon=True) for i, g in enumerate(groups)]
    t_start = time.time()
    for pr in procs:
        pr.start()
    for _ in procs:
        if not ready.acquire(timeout=max(1.0, budget_s - (time.time() - t_start))):
            for pr in procs:
                pr.kill()
            return None
    go.set()
    res = []
    try:
        for _ in procs:
            res.append(out.get(timeout=budget_s))
    except Exception:
        for pr in procs:
            pr.kill()
        return None
    for pr in procs:
        pr.join(timeout=10)
    if any(isinstance(r[3], str) for r in res):
        return {"error": next(r[3] for r in res if isinstance(r[3], str))}
    wall = max(r[2] for r in res) - min(r[1] for r in res)
    total_rows = rows * len(procs)
    return {"value": total_rows / (wall / steps * mean_T), "processes": len(procs), "threads_per_process": threads_per_proc,
            "cores": len(procs) * threads_per_proc, "rows": total_rows, "steps": steps, "wall_s": round(wall, 2),
            "slowest_process_s": round(max(r[3] for r in res), 2), "fastest_process_s": round(min(r[3] for r in res), 2)}


def cpu_baseline(kind, cfg, sd, mode, rows, steps, mean_T, impl="auto", data="auto", wseed=0, all_cores=True):
    """The oracle (CPU port of the reference algorithm) on the host cores, bounded sample.  SURVEY.md §8d: the build's
    CPU restatement, on PyTorch-CPU kernels where torch is present (oracle/hudiff_oracle_torch.py), else on numpy.  Three figures:
    one process at B = 1 (the reference CLI's default --batch_size), one process at `rows` rows on its fastest thread count, and -- the
    host's best, `value_all_cores` -- physical_cores / 16 processes x 16 pinned threads over disjoint rows.  `value` is the best of the three,
    `cores` the threads that one used."""
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import hudiff_oracle as ho
    batch, _ = make_batch(kind, rows, mode, 0, data)
    net, name, threads = None, "numpy+OpenBLAS", None
    if impl in ("auto", "torch"):
        try:
            import torch
            import hudiff_oracle_torch as hot
            net, name, threads = hot.TorchOracleNet(kind, cfg, sd), "PyTorch-CPU kernels", torch.get_num_threads()
        except ImportError:
            if impl == "torch":
                raise
    if net is None:
        net = ho.OracleNet(kind, cfg, sd)
    phys, logical = physical_cores()

    def run(n_rows, n_steps):
        ch = None if batch["chain"] is None else np.concatenate([batch["chain"][:n_rows], batch["chain"][rows:rows + n_rows]])
        t0 = time.perf_counter()
        ho.sample(net, batch["tokens"][:n_rows], batch["region"][:n_rows], ch, batch["order"][:n_rows],
                  np.minimum(batch["T"][:n_rows], n_steps), seed=1, dropout_mode="philox")
        return time.perf_counter() - t0

    run(rows, 1)                                                               # warm-up (threads, caches)
    if threads is not None:
        # many-core hosts oversubscribe these matrix sizes (256 logical CPUs: 0.035 sequences/s on 128 threads, 0.145 on 16): two steps
        # per candidate thread count, ascending up to ALL physical cores; the sweep stops only after TWO consecutive counts were 1.5 x
        # slower than the best so far (one noisy probe must not end it), and the winner is re-timed against its neighbours
        import torch
        cands = sorted({c for c in (8, 16, 32, min(64, phys), phys) if c <= max(phys, 8)})
        timed, slow, stopped = {}, 0, False
        for n in cands:
            torch.set_num_threads(n)
            timed[n] = min(run(rows, 1), run(rows, 1))
            best_t = min(timed.values())
            slow = slow + 1 if timed[n] > 1.5 * best_t else 0
            if slow >= 2:
                stopped = True
                break
        order_ = sorted(timed, key=timed.get)
        for n in order_[:2]:                                                   # winner and runner-up once more, back to back
            torch.set_num_threads(n)
            timed[n] = min(timed[n], run(rows, 1))
        threads = min(timed, key=timed.get)
        torch.set_num_threads(threads)
        name += f" (one process: fastest of {'/'.join(map(str, sorted(timed)))} threads" + \
                ("; the sweep stopped after two consecutive counts were more than 1.5 x slower)" if stopped else ")")
    dt_b = run(rows, steps)
    steps1 = max(2, steps // 2)
    run(1, 1)
    dt_1 = run(1, steps1)
    if threads is None:
        try:
            from threadpoolctl import threadpool_info
            threads = max([p.get("num_threads", 1) for p in threadpool_info()] or [1])
        except Exception:
            threads = os.cpu_count() or 1
    v_b = rows / (dt_b / steps * mean_T)
    v_1 = 1.0 / (dt_1 / steps1 * mean_T)
    out = {"value": max(v_b, v_1), "unit": "sequences/s", "cores": int(threads), "kind": "port",
           "physical_cores": phys, "logical_cpus": logical, "value_batch_1": v_1, f"value_batch_{rows}": v_b}
    sample = (f"oracle restatement of the reference loop on {name}; host has {phys} physical cores / {logical} logical "
              f"CPUs; one process, {threads} threads: {rows} rows x {steps} denoiser steps in {dt_b:.1f} s and 1 row x {steps1} "
              f"steps in {dt_1:.1f} s (B = 1 is the reference CLI's default), philox dropout, extrapolated to the "
              f"mean T = {mean_T:.1f} steps per sequence")
    if all_cores and net is not None and name.startswith("PyTorch"):
        ac = cpu_all_cores(kind, cfg, wseed, mode, rows, max(2, steps // 2), mean_T, data)
        if ac and "value" in ac:
            out["value_all_cores"] = ac["value"]
            out["all_cores"] = ac
            sample += (f"; ALL CORES: {ac['processes']} processes x {ac['threads_per_process']} pinned threads, {ac['rows']} rows x {ac['steps']} "
                       f"steps in {ac['wall_s']} s")
            if ac["value"] > out["value"]:
                out["value"], out["cores"] = ac["value"], ac["cores"]
        elif ac:
            out["all_cores"] = ac
    out["sample"] = sample
    return out


PEAK_F16_MATRIX_TFLOPS = 2500.0    # same guide, dense fp16 MFMA; three fp16 MFMAs per fp32 product -> 833.3 fp32-equivalent


GUARD_INVALIDATED = []          # (route, sample) whose tokens a guard of the split kernels invalidated (reported in precision_evidence)


def tokens_of_sample(model, shape, tag):
    """Tokens of the sample just timed (hd_sample_tokens).  A range / ln_sync guard that fired during that sample makes the library refuse
    them (HD_ERR_STATE: only hd_sample_end repeats a sample); the handle has already switched to the safe kernels (hd_sync looked at the
    flags), so the benchmark goes on: the sample is marked invalid (-1 everywhere) and listed, instead of aborting the run."""
    from hudiff_amd._lib import HD_ERR_STATE, HudiffError
    try:
        return model.sample_tokens()
    except HudiffError as e:
        if e.status != HD_ERR_STATE:
            raise
        GUARD_INVALIDATED.append(tag)
        sys.stderr.write(f"[bench] {tag}: a guard of the split kernels fired during this sample; its tokens are not used ({e})\n")
        return np.full(shape, -1, dtype=np.int32)


def timed_leg(args, kind, cfg, sd, batch, T, rank, local_rank, precision, steps, warmup, first_key=0, keep_tokens=True):
    """One timed leg of a workload beside the top-level line: a model on route `precision` (hd_set_precision), the same protocol
    as the main line (inputs resident, restart + all T steps per sample, device sync on both sides, HIP-event time of the
    replays).  -> (tokens of every timed sample [steps, B, L], model (still open, session ended), dict of raw numbers)."""
    import hudiff_amd
    B = batch["tokens"].shape[0]
    Tmax = int(T.max())
    model = (hudiff_amd.AntiTFNet if kind == "ab" else hudiff_amd.NanoAntiTFNet)(**cfg, device=local_rank, precision=precision)
    model.load_state_dict(sd)
    model.sample_begin(batch["tokens"], batch["region"], batch["chain"], batch["order"], T, seed=2023,
                       row0=rank * B, dropout=args.dropout, graph=(False if args.no_graph else "loop" if args.loop_graph else True), lanes=args.lanes)
    gpu_ms, watch, t0, toks = 0.0, None, 0.0, []
    for i in range(-warmup, steps):
        model.sample_restart(2023 + 7919 * (first_key + i))
        if i == 0:
            model.sync()
            watch = ClockPowerSampler(local_rank).start()
            t0 = time.perf_counter()
        model.sample_run(0, Tmax)
        if i >= 0:
            model.sync()
            gpu_ms += model.last_run_ms()[0]
            if keep_tokens:
                toks.append(tokens_of_sample(model, batch["tokens"].shape, f"{kind}/{precision}/sample {i}"))
    elapsed = time.perf_counter() - t0
    clock_power = watch.stop() if watch else None
    last = model.sample_end()
    if not keep_tokens:
        toks = [last]
    return np.stack(toks), model, {"elapsed": elapsed, "gpu_ms": gpu_ms, "steps": steps, "clock_power": clock_power, "Tmax": Tmax, "B": B,
                                   "precision": model.precision_info()}


DTYPE_OF_ROUTE = {
    "split": "f32-equivalent: fp16 hi+lo split, 3 MFMA / product, f32 accumulate; pruned tail + static branch f32",
    "f32_gemm": "f32 MFMA GEMMs; attention core f32-equivalent (fp16 hi+lo split, 3 MFMA / product, f32 accumulate)",
    "f32_all": "f32 (every product on the fp32 MFMA pipe)",
}
DTYPE_DETAIL = {
    "split": "every large GEMM (Q|K|V, out-projection, FF, ByteNet projections and taps) and the attention core (QK^T, PV): each fp32 operand "
             "as fp16 hi + fp16 lo (22 significand bits), a w ~= a_hi w_hi + a_hi w_lo + a_lo w_hi as three v_mfma_f32_32x32x16_f16 / "
             "16x16x32_f16 with fp32 accumulation; softmax, LayerNorm, residuals, dropout, decoder in fp32; the pruned tail's compact GEMMs and the static branch on fp32 MFMA; range guard (|x| >= 65504) and ln_sync "
             "guard repeat the call on fp32 / ln_apply_k kernels (precision_info)",
    "f32_gemm": "GEMMs (90.5 % of the FLOPs): fp32 MFMA v_mfma_f32_32x32x2_f32; attention core (9.5 %): three fp16 MFMAs per product on "
                "fp16 (hi, lo) splits of the fp32 Q / K / V / P, fp32 accumulation and softmax",
    "f32_all": "every kernel fp32 MFMA (v_mfma_f32_32x32x2_f32 / 16x16x4_f32)",
}


def route_of(info):
    """bench-internal route name of a handle's hd_precision_report: split | f32_gemm | f32_all."""
    return info["precision"]


def attention_core_share(cfg):
    """Share of the algorithmic FLOPs of a forward that is the attention core (QK^T and PV): 2 n_blk x 4 L A of the per-slot sum."""
    L, d, D, A, Fd = cfg["max_len"], cfg["d_model"], cfg["sum_d_model"], cfg["att_model"], cfg["dim_feedforward"]
    dh, Dh, k = d // 2, D // 2, cfg["aa_kernel_size"]
    per_slot = (cfg["n_encoder_layers"] * (4 * d * dh + 2 * k * dh * dh) + cfg["dual_layers"] * (4 * D * Dh + 2 * k * Dh * Dh) +
                2.0 * cfg["cs_layers"] * (8 * D * A + 4 * L * A) + cfg["cs_layers"] * 4 * D * Fd + 2 * D * cfg["n_tokens"])
    return 2.0 * cfg["cs_layers"] * 4 * L * A / per_slot


def route_peak(cfg, route):
    """Matrix-pipe peak a route is priced against, in fp32-equivalent TFLOP/s (guide: 157.3 fp32 MFMA, 2500 dense fp16 MFMA).
    all_fp32: every product on the fp32 pipe.  split: every product as three fp16 MFMAs -> 2500 / 3.  default: the GEMMs on the
    fp32 pipe, the attention core (share a of the FLOPs) as three fp16 MFMAs: the time-weighted harmonic mean
    1 / ((1 - a) / 157.3 + a / 833.3) -- slightly above 157.3, so that moving the attention core to the faster pipe does not
    inflate the fraction."""
    if route in ("all_fp32", "f32_all"):
        return PEAK_F32_MATRIX_TFLOPS
    if route == "split":
        return PEAK_F16_MATRIX_TFLOPS / 3.0
    a = attention_core_share(cfg)
    return 1.0 / ((1.0 - a) / PEAK_F32_MATRIX_TFLOPS + a / (PEAK_F16_MATRIX_TFLOPS / 3.0))


def roofline_object(raw, T, flops_row, flops_row_exec, peak, unit, split):
    """roofline of one leg: algorithmic FLOPs over the HIP-event time of the replays; executed beside it."""
    tf = float(T.sum()) * flops_row * raw["steps"] / (raw["gpu_ms"] * 1e-3) / 1e12
    tf_exec = float(raw["B"] * raw["Tmax"]) * flops_row_exec * raw["steps"] / (raw["gpu_ms"] * 1e-3) / 1e12
    out = {"bound": "mfma", "achieved": round(tf, 3), "peak": round(peak, 2), "unit": unit, "frac": round(tf / peak, 4), "traffic": None,
           "flops_per_launch": raw["B"] * flops_row, "avg_launch_ms": round(raw["gpu_ms"] / (raw["steps"] * raw["Tmax"]), 4),
           "executed_tflops": round(tf_exec, 3), "executed_frac": round(tf_exec / peak, 4),
           "executed_over_algorithmic": round(flops_row_exec / flops_row, 4)}
    cp = raw.get("clock_power")
    if cp:
        pk = peak * cp["sclk_mhz_median"] / 2400.0
        cp = dict(cp, peak_at_sustained_clock=round(pk, 2), frac_at_sustained_clock=round(tf / pk, 4),
                  source="amdgpu hwmon freq1_input / power1_input of this GPU, 10 Hz over the timed region")
        out["clock_power"] = cp
    if split in ("split", True):
        out["peak_note"] = ("fp32-equivalent peak of the split route: dense fp16 MFMA peak of the guide (2500 TFLOP/s at 2.4 GHz) / 3 "
                            "MFMAs per product")
    elif split in ("default", "f32_gemm"):
        out["frac_vs_fp32_matrix_peak_157.3"] = round(tf / PEAK_F32_MATRIX_TFLOPS, 4)
        out["peak_note"] = ("GEMMs priced at the fp32 MFMA peak (157.3), the attention core (its share of the algorithmic FLOPs) at the "
                            "fp32-equivalent fp16 peak 2500 / 3: time-weighted harmonic mean; against 157.3 alone the fraction would be "
                            f"{tf / PEAK_F32_MATRIX_TFLOPS:.4f}")
    return out


def live_pmc(args, kind, mode, precision, n_steps=4):
    """HBM-side bytes per denoiser step and the MFMA pipe's busy fraction from rocprofv3 PMC passes of THIS script on route
    `precision` (a 4-step one-lane run in a subprocess, --kernel-trace only).  Two passes: `FETCH_SIZE` alone (3 of the 4 TCC slots),
    then `WRITE_SIZE` with `SQ_VALU_MFMA_BUSY_CYCLES` and `GRBM_GUI_ACTIVE` (SQ and GRBM slots are independent of the TCC's;
    MI355X_MICROARCH.md "HBM" / "rocprofv3 PMC slots").  FETCH_SIZE doubled (gfx950 tallies 128-B requests at 64 B); unit KB.  Counted
    from the first token gather on (the once-per-batch static branch is excluded).  mfma_busy = MFMA-busy cycles / (GRBM_GUI_ACTIVE / 8
    XCDs x 1024 SIMDs): the fraction of all SIMD cycles, launch gaps included, in which the matrix pipe was executing."""
    import csv
    import glob
    import shutil
    import subprocess
    import tempfile
    if shutil.which("rocprofv3") is None:
        return None
    tot = {}
    tmp = tempfile.mkdtemp(prefix="hudiff_pmc_", dir="/tmp")
    env = dict(os.environ, TMPDIR="/tmp")
    # the profiled run is a single-rank job on this rank's GPU, also when this process is one rank of N (launcher variables scrubbed);
    # its route is given on the command line (an explicit hd_set_precision: the environment cannot override it)
    for k in list(env):
        if k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "LOCAL_WORLD_SIZE", "GROUP_RANK", "ROLE_RANK", "ROLE_WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT",
                 "HUDIFF_BENCH_FORCE_PG", "HUDIFF_BENCH_SHARE_GPU", "HUDIFF_DIST_FORCE") or k.startswith("TORCHELASTIC_"):
            env.pop(k)
    try:
        for n, counters in enumerate((["FETCH_SIZE"], ["WRITE_SIZE", "SQ_VALU_MFMA_BUSY_CYCLES", "GRBM_GUI_ACTIVE"])):
            out = os.path.join(tmp, f"pass{n}")
            cmd = ["rocprofv3", "--pmc", *counters, "--kernel-trace", "--output-format", "csv", "-d", out, "-o", "p", "--",
                   sys.executable, os.path.abspath(__file__), "--kind", kind, "--mode", mode, "--batch", str(args.batch),
                   "--dropout", args.dropout, "--data", args.data, "--steps", "1", "--warmup", "0", "--max-t", str(n_steps),
                   "--no-cpu-baseline", "--lanes", "1", "--pmc", "off", "--only-main", "--precision", precision]
            subprocess.run(cmd, cwd="/tmp", env=env, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, timeout=300, check=True)
            files = glob.glob(os.path.join(out, "**", "*counter_collection.csv"), recursive=True)
            rows = [r for f in files for r in csv.DictReader(open(f))]
            rows.sort(key=lambda r: int(r["Dispatch_Id"]))
            started = False
            for r in rows:
                started = started or "embed_tokens_k" in r["Kernel_Name"]
                if started and r["Counter_Name"] in counters:
                    tot[r["Counter_Name"]] = tot.get(r["Counter_Name"], 0.0) + float(r["Counter_Value"])
    except Exception as e:                 # profiler absent / refused: the bench line must still appear
        sys.stderr.write(f"[bench] live PMC pass failed: {e!r}\n")
        return None
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    if "FETCH_SIZE" not in tot or "WRITE_SIZE" not in tot:
        return None
    rd = 2.0 * tot["FETCH_SIZE"] * 1024.0 / n_steps
    wr = tot["WRITE_SIZE"] * 1024.0 / n_steps
    busy = None
    if tot.get("GRBM_GUI_ACTIVE"):
        busy = tot.get("SQ_VALU_MFMA_BUSY_CYCLES", 0.0) / (tot["GRBM_GUI_ACTIVE"] / 8.0 * 1024.0)
    return {"traffic": rd + wr, "read_bytes": rd, "write_bytes": wr, "mfma_busy": busy,
            "note": f"per denoiser step, live: rocprofv3 --pmc FETCH_SIZE | --pmc WRITE_SIZE SQ_VALU_MFMA_BUSY_CYCLES GRBM_GUI_ACTIVE (two "
                    f"passes) over a {n_steps}-step one-lane run of this command; FETCH_SIZE x 2 (gfx950), KB -> bytes; L2<->fabric side, "
                    "Infinity-Cache hits included; mfma_busy = MFMA-busy cycles / all SIMD cycles of that profiled run"}


def attach_pmc(roof, pmc):
    if pmc is None:
        return
    roof["traffic"] = pmc["traffic"]
    roof["traffic_read_bytes"], roof["traffic_write_bytes"] = pmc["read_bytes"], pmc["write_bytes"]
    # bytes per launch / measured launch time of the timed region = HBM-side GB/s the path sustains (peak ~8 TB/s: not the limiter)
    roof["hbm_gbps"] = round(pmc["traffic"] / (roof["avg_launch_ms"] * 1e-3) / 1e9, 1)
    roof["hbm_frac_of_8TBps"] = round(roof["hbm_gbps"] / 8000.0, 4)
    if pmc["mfma_busy"] is not None:
        roof["mfma_busy"] = round(pmc["mfma_busy"], 4)
    roof["pmc_note"] = pmc["note"]


DUMP_LIMIT_BYTES = 64 << 20


def dump_outputs(out_dir, tokens):
    """--dump-outputs: the final tokens of the last timed sample as DIR/tokens.npy, float32 (token ids are exact in it).  Beyond 64 MB
    a fixed seeded sample of the rows is written, in row order, with their indices in DIR/tokens_rows.npy."""
    os.makedirs(out_dir, exist_ok=True)
    out = np.asarray(tokens, dtype=np.float32)
    max_rows = max(1, DUMP_LIMIT_BYTES // (out.shape[1] * out.itemsize + 8))
    if out.shape[0] > max_rows:
        rows = np.sort(np.random.default_rng(0).choice(out.shape[0], size=max_rows, replace=False))
        out = out[rows]
        np.save(os.path.join(out_dir, "tokens_rows.npy"), rows.astype(np.float64))
    np.save(os.path.join(out_dir, "tokens.npy"), out)


def relaunch_one_rank_per_gpu(args):
    """`python bench.py --gpus N` without a launcher around it (the driver's single-node command shape): start N ranks of
    this very command under torch.distributed.run -- one process per GPU, rendezvous on 127.0.0.1 -- and hand back its exit
    code.  Rank 0 of that job prints the JSON line on the inherited stdout."""
    import socket
    import subprocess
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={args.gpus}",
           "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
    return subprocess.call(cmd, env=dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0"))


def main():
    args = parse()
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        sys.exit(relaunch_one_rank_per_gpu(args))
    rank = int(os.environ.get("RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if world != args.gpus:
        # never print a line whose n_gpus is not what was asked for
        sys.exit(f"bench.py: --gpus {args.gpus} but the launcher started WORLD_SIZE={world} ranks")
    dist = None
    # Debug aid for single-GPU boxes: HUDIFF_BENCH_SHARE_GPU=1 runs every rank on device 0 with a gloo (CPU)
    # gather, so that the N > 1 control flow can be exercised without N GPUs.  Never set by the driver.
    share_gpu = os.environ.get("HUDIFF_BENCH_SHARE_GPU") == "1"
    if share_gpu:
        local_rank = 0
    # HUDIFF_BENCH_FORCE_PG=1: form the RCCL process group even for one rank (a world-size-1 nccl group is legal), so that
    # the communicator init, the device-tensor gather and the all-reduce below run on a one-GPU box (tests/test_gpu_dist.py)
    force_pg = os.environ.get("HUDIFF_BENCH_FORCE_PG") == "1"
    if world > 1 or force_pg:
        import torch
        import torch.distributed as dist
        torch.cuda.set_device(local_rank)
        if force_pg and world == 1:
            os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
            if "MASTER_PORT" not in os.environ:
                import socket
                with socket.socket() as s:
                    s.bind(("127.0.0.1", 0))
                    os.environ["MASTER_PORT"] = str(s.getsockname()[1])
            os.environ.setdefault("RANK", "0")
            os.environ.setdefault("WORLD_SIZE", "1")
        if share_gpu:
            dist.init_process_group("gloo")
        else:
            dist.init_process_group("nccl", device_id=torch.device("cuda", local_rank))   # nccl == RCCL on ROCm
    n_gpus = world
    coll_dev = "cpu" if share_gpu else "cuda"
    formed = {"world_size": 1, "backend": None}
    if dist is not None:
        # what the process group actually formed (not what the environment asked for)
        formed = {"world_size": int(dist.get_world_size()), "backend": str(dist.get_backend())}
        assert formed["world_size"] == world, (formed, world)

    import hudiff_amd
    from hudiff_amd import synthetic as S

    kind = args.kind
    cfg = dict(S.AB_CONFIG if kind == "ab" else S.NB_CONFIG)
    mode = args.mode or ("finetune" if kind == "ab" else "plain")
    sd = S.random_state_dict(kind, cfg, seed=0)
    B = args.batch
    batch, real = make_batch(kind, B, mode, rank * B, args.data)
    T = batch["T"].copy()
    if args.max_t > 0:
        T = np.minimum(T, args.max_t)
    Tmax = int(T.max())

    model = (hudiff_amd.AntiTFNet if kind == "ab" else hudiff_amd.NanoAntiTFNet)(
        **cfg, device=local_rank, precision=None if args.precision == "default" else args.precision)
    model.load_state_dict(sd)
    flops_row = model.flops_per_row_forward()            # canonical / algorithmic
    flops_row_exec = model.flops_per_row_sample_step()   # executed: last attention block pruned to the visited row

    def barrier():
        model.sync()
        if dist is not None:
            import torch
            torch.cuda.synchronize()
            dist.barrier()

    t_up0 = time.perf_counter()
    model.sample_begin(batch["tokens"], batch["region"], batch["chain"], batch["order"], T, seed=2023,
                       row0=rank * B, dropout=args.dropout, graph=(False if args.no_graph else "loop" if args.loop_graph else True), lanes=args.lanes)
    upload_s = time.perf_counter() - t_up0
    gpu_ms = 0.0
    main_tokens = []                                     # every timed sample's tokens (precision_evidence: agreement between routes)

    def one_sample(i, timed):
        nonlocal gpu_ms
        model.sample_restart(2023 + 7919 * i)
        model.sample_run(0, Tmax)
        if timed:
            model.sync()
            gpu_ms += model.last_run_ms()[0]
            main_tokens.append(tokens_of_sample(model, batch["tokens"].shape, f"main/sample {i}"))    # 300 KB device-to-host after the sync: < 0.01 % of a sample

    for i in range(args.warmup):
        one_sample(-1 - i, False)
    barrier()
    watch = ClockPowerSampler(local_rank).start() if rank == 0 else None
    t0 = time.perf_counter()
    for i in range(args.steps):
        one_sample(i, True)
    barrier()
    elapsed = time.perf_counter() - t0
    clock_power = watch.stop() if watch else None
    my_elapsed = elapsed
    tokens = model.sample_end()
    prec_main = model.precision_info()
    route_main = route_of(prec_main)
    only_main = not args.full or args.only_main or args.max_t > 0 or world > 1 or force_pg
    f32_gemm = secondary = None
    t_phase = time.perf_counter()

    def phase(name):
        nonlocal t_phase
        now = time.perf_counter()
        sys.stderr.write(f"[bench] {name}: {now - t_phase:.1f} s\n")
        t_phase = now

    def agreement(a, b):
        """rows with identical final tokens, over every timed sample both legs ran with the same noise keys"""
        n = min(len(a), len(b))
        a, b = np.asarray(a[-n:]), np.asarray(b[-n:])
        ok = (a >= 0).all((1, 2)) & (b >= 0).all((1, 2))          # samples a guard invalidated (tokens_of_sample) are left out
        same = int((a[ok] == b[ok]).all(-1).sum())
        return {"rows_identical": same, "rows_compared": int(ok.sum() * B), "samples_compared": int(ok.sum())}

    all_fp32, fp32_tokens = None, None
    if rank == 0 and not only_main and not args.no_all_fp32_line and route_main != "f32_all":
        # ---- every product on the fp32 MFMA pipe: the SAME number of samples as the top level, own clock / power, own PMC passes ----
        fp32_tokens, mf, rawf = timed_leg(args, kind, cfg, sd, batch, T, rank, local_rank, "f32_all", args.steps, min(args.warmup, 1))
        all_fp32 = {"value": round(B * rawf["steps"] / rawf["elapsed"], 4), "unit": "sequences/s", "steps": rawf["steps"],
                    "ms_per_step": round(1e3 * rawf["elapsed"] / rawf["steps"], 3), "dtype": DTYPE_OF_ROUTE["f32_all"],
                    "roofline": roofline_object(rawf, T, flops_row, flops_row_exec, PEAK_F32_MATRIX_TFLOPS, "TFLOP/s", split=False),
                    "token_agreement_with_top_level": agreement(main_tokens, fp32_tokens),
                    "precision_info": rawf["precision"],
                    "note": "precision route f32_all (hd_set_precision): the reference's own arithmetic -- every product fp32 -- on the same rows, "
                            "weights, noise keys and number of samples as the top level"}
        phase("all-fp32-kernels leg")
    if rank == 0 and not only_main and not args.no_f32_gemm_line and route_main == "split":
        # ---- the round-3 default route (fp32 MFMA GEMMs + split attention core), short: kept for continuity with BENCH_r03 ----
        n_g = min(args.steps, 2)
        g_tokens, mg, rawg = timed_leg(args, kind, cfg, sd, batch, T, rank, local_rank, "f32_gemm", n_g, min(args.warmup, 1), first_key=args.steps - n_g)
        mg.close()
        f32_gemm = {"value": round(B * rawg["steps"] / rawg["elapsed"], 4), "unit": "sequences/s", "steps": rawg["steps"],
                    "ms_per_step": round(1e3 * rawg["elapsed"] / rawg["steps"], 3), "dtype": DTYPE_OF_ROUTE["f32_gemm"],
                    "roofline": roofline_object(rawg, T, flops_row, flops_row_exec, route_peak(cfg, "f32_gemm"), "TFLOP/s (fp32-equivalent)", split="f32_gemm"),
                    "token_agreement_with_top_level": agreement(main_tokens, g_tokens), "precision_info": rawg["precision"],
                    "note": "precision route f32_gemm: BENCH_r03's top-level route"}
        phase("f32-gemm-route leg")

    evidence = None
    if rank == 0 and not only_main and not args.no_evidence and args.max_t == 0:
        # ---- precision_evidence: this run's rows and weights, each route against a float64 CPU evaluation at three points of the sample ----
        sys.path.insert(0, os.path.join(ROOT, "oracle"))
        import hudiff_oracle as ho
        n64 = max(1, min(args.evidence_rows, B))
        n_dev = min(B, 64)             # rows per device forward: enough activation rows (>= 8192) for the big-launch kernels on both models
        last = main_tokens[-1]
        t_mid = int(Tmax // 2)
        pts = [0, t_mid, max(Tmax - 1, 0)]
        ch_dev = None if batch["chain"] is None else np.concatenate([batch["chain"][:n_dev], batch["chain"][B:B + n_dev]])
        ch64 = None if batch["chain"] is None else np.concatenate([batch["chain"][:n64], batch["chain"][B:B + n64]])
        net64 = ho.OracleNet(kind, cfg if args.dropout == "faithful" else dict(cfg, dropout=0.0), sd, dtype=np.float64)
        seed_last = 2023 + 7919 * (args.steps - 1)
        routes = {route_main: model}
        if all_fp32 is not None:
            routes["f32_all"] = mf
        per_route = {r: [] for r in routes}
        for t in pts:
            # token state of the LAST timed sample at step t: the slots visited before t hold their final tokens
            st = batch["tokens"][:n_dev].copy()
            for b in range(n_dev):
                vis = batch["order"][b, :min(t, int(T[b]))]
                st[b, vis] = last[b, vis]
            dr = ho.Dropout("philox", seed=seed_last, rows=np.arange(n64) + rank * B, step=t) if (args.dropout == "faithful" and cfg.get("dropout", 0) > 0) else None
            want = net64(st[:n64], batch["region"][:n64], ch64, dropout=dr)
            for r, mdl in routes.items():
                got = mdl(st, batch["region"][:n_dev], ch_dev, dropout=args.dropout, seed=seed_last, row0=rank * B, step=t)
                per_route[r].append(float(np.abs(got[:n64].astype(np.float64) - want).max()))
        evidence = {"float64_reference": f"oracle/hudiff_oracle.py in float64 (numpy), {n64} rows of this run's batch, its weights, "
                                         f"dropout {args.dropout} (the device's own Philox keep-masks), token state of the last timed sample "
                                         f"at denoiser steps {pts} of {Tmax}; device forwards of {n_dev} rows (big-launch kernels)",
                    "steps_along_the_sample": pts,
                    "max_abs_dlogit_vs_float64": {r: {"per_step": [float(f"{e:.3e}") for e in v], "max": float(f"{max(v):.3e}")} for r, v in per_route.items()},
                    "bound": 1e-4,
                    "token_agreement": {}}
        if all_fp32 is not None:
            evidence["token_agreement"][f"{route_main} vs f32_all"] = agreement(main_tokens, fp32_tokens)
        if f32_gemm is not None:
            evidence["token_agreement"][f"{route_main} vs f32_gemm"] = f32_gemm["token_agreement_with_top_level"]
        # ---- rows identical to the REFERENCE: tests/golden/fliprate_{kind}.npz holds 64 complete production-width samples drawn by the
        # reference's own AntiTFNet / NanoAntiTFNet on the CPU (same seed-0 weights as this run; oracle/make_golden_fliprate.py), with the
        # torch.multinomial noise it used and its near-tie margin of every draw; replayed here on the open models (dropout off, as recorded)
        try:
            import hashlib
            fz = np.load(os.path.join(ROOT, "tests", "golden", f"fliprate_{kind}.npz"))
            h = hashlib.sha256()
            for k in sorted(sd):
                h.update(k.encode())
                h.update(np.ascontiguousarray(sd[k], dtype=np.float32).tobytes())
            if h.hexdigest() == str(fz["weight_sha256"]):
                ftok, freg, fT = fz["tokens"].astype(np.int64), fz["region"].astype(np.int64), fz["T"].astype(np.int64)
                fch = fz["chain"].astype(np.int64) if fz["chain"].size else None
                rep = {"source": f"tests/golden/fliprate_{kind}.npz: {ftok.shape[0]} rows sampled by the reference (PyTorch CPU, float32), recorded noise", "routes": {}}
                for r, mdl in routes.items():
                    got = np.asarray(mdl.sample(ftok, freg, fch, fz["order"].astype(np.int64), fT, q_noise=fz["q"], dropout="off"))
                    diff = []
                    for b in range(ftok.shape[0]):
                        slots = fz["order"][b, :int(fT[b])]
                        bad = np.nonzero(got[b, slots] != fz["final"][b, slots])[0]
                        if bad.size:
                            diff.append({"row": int(b), "first_differing_step": int(bad[0]), "reference_margin_of_that_draw": float(f"{float(fz['margin'][b, bad[0]]):.3e}")})
                    rep["routes"][r] = {"rows_identical_to_the_reference": f"{ftok.shape[0] - len(diff)} of {ftok.shape[0]}", "differing": diff}
                evidence["reference_rows"] = rep
        except (OSError, KeyError) as e:
            evidence["reference_rows"] = {"skipped": repr(e)}
        evidence["precision_info_after"] = {r: mdl.precision_info() for r, mdl in routes.items()}
        phase("precision evidence (float64 oracle, reference rows)")
    if all_fp32 is not None:
        mf.close()

    if rank == 0 and not only_main and not args.no_secondary and kind == "ab":
        # ---- BASELINE configs[3]: HuDiff-Nb on abnativ_select_vhh, plain mask, 256 rows, same protocol -- a secondary object ----
        ncfg = dict(S.NB_CONFIG)
        nsd = S.random_state_dict("nb", ncfg, seed=0)
        nbatch, nreal = make_batch("nb", B, "plain", rank * B, args.data)
        nT = nbatch["T"].copy()
        secondary = {}
        for route in ("split", "f32_all"):
            ntok, mn, rawn = timed_leg(args, "nb", ncfg, nsd, nbatch, nT, rank, local_rank, route, 2, 1, keep_tokens=False)
            f_alg, f_exec = mn.flops_per_row_forward(), mn.flops_per_row_sample_step()
            mn.close()
            pk = route_peak(ncfg, route)
            secondary[route] = {"value": round(B * rawn["steps"] / rawn["elapsed"], 4), "unit": "sequences/s", "steps": rawn["steps"],
                                "ms_per_step": round(1e3 * rawn["elapsed"] / rawn["steps"], 3), "dtype": DTYPE_OF_ROUTE[route],
                                "roofline": roofline_object(rawn, nT, f_alg, f_exec, pk, "TFLOP/s" + ("" if route == "f32_all" else " (fp32-equivalent)"),
                                                            split=route if route != "f32_all" else False),
                                "precision_info": rawn["precision"],
                                "all_tokens_valid": bool(((ntok >= 0) & (ntok <= 21)).all())}
        secondary = {"metric": "humanized sequences/sec (full T-step sample)" + (" on abnativ_select_vhh" if nreal else ""),
                     "config": {"workload": f"BASELINE configs[3]: HuDiff-Nb NanoAntiTFNet (17.5M params, L=152), plain mask, batch {B}/GPU, full "
                                            f"T-step sample (T {int(nT.min())}..{int(nT.max())}, mean {float(nT.mean()):.1f}), dropout {args.dropout}"},
                     **secondary}
        phase("HuDiff-Nb secondary line")

    # ---- the single collective of the job: gather the final tokens on rank 0 (RCCL over xGMI) ----------
    gathered = [tokens]
    per_rank = None
    if dist is not None:
        import torch
        t = torch.from_numpy(tokens).to(coll_dev)
        outs = [torch.empty_like(t) for _ in range(world)] if rank == 0 else None
        dist.gather(t, outs, dst=0)
        if rank == 0:
            gathered = [o.cpu().numpy() for o in outs]
        # every rank's own wall time of the timed region (a straggler GPU shows here; the metric uses the maximum)
        mine = torch.tensor([my_elapsed, gpu_ms], dtype=torch.float64, device=coll_dev)
        alls = [torch.empty_like(mine) for _ in range(world)]
        dist.all_gather(alls, mine)
        per_rank = [[float(a[0]), float(a[1])] for a in alls]
        el = torch.tensor([elapsed, gpu_ms], dtype=torch.float64, device=coll_dev)
        dist.all_reduce(el, op=dist.ReduceOp.MAX)
        elapsed, gpu_ms = float(el[0]), float(el[1])

    if rank == 0:
        all_tokens = np.concatenate(gathered)
        filled = bool(((all_tokens >= 0) & (all_tokens <= 22)).all())
        if args.max_t == 0:
            assert not (all_tokens == 22).any(), "masked slots left after a full sample"
        if args.dump_outputs:
            dump_outputs(args.dump_outputs, all_tokens)
        seqs = n_gpus * B * args.steps
        value = seqs / elapsed
        raw_main = {"gpu_ms": gpu_ms, "steps": args.steps, "B": B, "Tmax": Tmax, "clock_power": clock_power}
        roof = roofline_object(raw_main, T, flops_row, flops_row_exec, route_peak(cfg, route_main), "TFLOP/s" if route_main == "f32_all" else
                               "TFLOP/s (fp32-equivalent)", split=route_main if route_main != "f32_all" else False)
        roof["route"] = route_main
        roof["launch"] = ("one denoiser step = one replay of the captured hipGraph (all kernels of a forward + sampling), HIP events on the "
                          "library's stream")
        out = {
            "metric": "humanized sequences/sec (full T-step sample)" + (" on HuAb348" if (real and kind == "ab") else ""),
            "value": round(value, 4), "unit": "sequences/s", "n_gpus": n_gpus, "steps": args.steps,
            "warmup": args.warmup, "ms_per_step": round(1e3 * elapsed / args.steps, 3), "higher_is_better": True,
            "scaling": "weak", "vs_baseline": None,
            "dtype": DTYPE_OF_ROUTE[route_main],
            "dtype_detail": DTYPE_DETAIL[route_main],
            "precision_route": route_main,
            "data": (("HuAb348 mouse pairs" if kind == "ab" else "abnativ_select_vhh VHH") +
                     f" ({batch['n_sequences']} sequences of the reference's evaluation CSV, IMGT-slotted by hudiff_amd.numbering into "
                     "hudiff_amd/data/real_rows.npz, cycled with distinct replica noise); random-init weights of the production architecture")
            if real else "synthetic",
            "config": {"workload": (("HuDiff-Ab AntiTFNet (39.8M params, L=291) on HuAb348, " if real else
                                     "HuDiff-Ab AntiTFNet (39.8M params, L=291), HuAb348-shaped synthetic rows, ")
                                    if kind == "ab" else
                                    ("HuDiff-Nb NanoAntiTFNet (17.5M params, L=152) on abnativ_select_vhh, " if real else
                                     "HuDiff-Nb NanoAntiTFNet (17.5M params, L=152), VHH-shaped synthetic rows, "))
                       + f"{mode} mask, batch {B}/GPU, full T-step sample (T {int(batch['T'].min())}..{int(batch['T'].max())}, "
                         f"mean {float(batch['T'].mean()):.1f}), dropout {args.dropout}",
                       "rows_per_gpu": B, "global_rows": n_gpus * B, "denoiser_steps_per_sample": Tmax,
                       "parallelism": f"rows sharded x{n_gpus}, one RCCL gather of int32 tokens",
                       "process_group": formed},
            "roofline": roof,
            "gpu_event_ms": round(gpu_ms, 2), "upload_ms": round(1e3 * upload_s, 2), "all_tokens_valid": filled,
            "precision_info": prec_main,
        }
        if per_rank is not None:
            ms = [1e3 * e / args.steps for e, _ in per_rank]
            out["per_rank_ms_per_step"] = {"min": round(min(ms), 3), "max": round(max(ms), 3), "ranks": [round(v, 3) for v in ms],
                                           "gpu_event_ms": [round(g, 2) for _, g in per_rank],
                                           "note": "each rank's own wall time of the timed region / steps; the metric divides by the slowest"}
        # HBM-side traffic, HBM GB/s and MFMA-busy per launch: live PMC passes of this very command (subprocess, after the timed region)
        # (N > 1: rank 0 profiles a single-rank run of the same per-GPU workload on its own GPU while the other ranks wait at the
        #  final barrier -- the ranks are independent, so its counters are every rank's)
        pmc_wanted = args.full and args.pmc in ("auto", "live") and not args.only_main and args.max_t <= 0 and (not force_pg or world > 1)
        if pmc_wanted and (not only_main or world > 1):
            attach_pmc(out["roofline"], live_pmc(args, kind, mode, route_main))
            if world > 1 and "pmc_note" in out["roofline"]:
                out["roofline"]["pmc_note"] += f"; taken on rank 0's GPU (single-rank run of the per-GPU workload), N = {world}"
            phase(f"PMC passes ({route_main})")
            if all_fp32 is not None:
                attach_pmc(all_fp32["roofline"], live_pmc(args, kind, mode, "f32_all"))
                phase("PMC passes (f32_all)")
        if all_fp32 is not None:
            out["all_fp32_kernels"] = all_fp32
        if f32_gemm is not None:
            out["f32_gemm_route"] = f32_gemm
        if evidence is not None:
            if GUARD_INVALIDATED:
                evidence["samples_invalidated_by_a_guard"] = list(GUARD_INVALIDATED)
            out["precision_evidence"] = evidence
        if secondary is not None:
            out["secondary"] = {"hudiff_nb_configs3": secondary}
        if args.max_t > 0:
            out["truncated"] = f"--max-t {args.max_t}: NOT the metric (profiling run)"
        if args.full and not args.no_cpu_baseline and n_gpus == 1 and not args.only_main:
            out["cpu_baseline"] = cpu_baseline(kind, cfg, sd, mode, args.cpu_rows, args.cpu_steps, float(batch["T"].mean()),
                                               args.cpu_impl, args.data)
            phase("CPU baseline")
        print(json.dumps(out), flush=True)
    model.close()
    if dist is not None:
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
