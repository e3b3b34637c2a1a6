"""Block decoding (slots_per_step = K) on the workload bench.py times: throughput and sample quality per K.

    python scripts/block_decode_sweep.py --ks 1,2,4,8,16 --steps 2 --warmup 1 --out profiles/block/sweep.json

The workload is bench.py's (HuAb348 pairs, 256 rows, the library's default route, inference-time dropout as in the reference, seeded
N(0, 0.02) weights); the protocol is bench.py's too: inputs resident (sample_begin), per sample a restart + every order position, a
device sync on both sides, wall time over the timed samples.  bench.py itself is the yardstick and has no K; this script drives the
same session calls with one.

Per K one JSON line:
  seqs_per_s          rows * samples / wall seconds of the timed samples          gpu_ms_per_sample   HIP-event time of one sample
  forwards_per_row    mean over rows of ceil(T / K)
  logp_per_residue    mean over rows of the per-residue log-likelihood of the FIRST timed sample's sequences, scored with K = 1
                      (one slot per forward, dropout off) along --orders random visiting orders
  parent_k1_bench_seqs_per_s   with --parent_bench_json: what bench.py measured on the parent commit's tree (same box, same session)
  differs_from_k1     share of sampled positions whose residue is not the one the K = 1 sample with the same seed drew
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ks", default="1,2,4,8,16")
    ap.add_argument("--steps", type=int, default=2, help="timed samples per K")
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--kind", choices=["ab", "nb"], default="ab")
    ap.add_argument("--orders", type=int, default=8, help="visiting orders of the quality score; 0 = no quality columns")
    ap.add_argument("--dropout", choices=["faithful", "off"], default="faithful")
    ap.add_argument("--parent_bench_json", default=None,
                    help="file holding the JSON line `bench.py --gpus 1` printed on the PARENT commit's tree in the same session on the "
                         "same box; its value is copied into every line as parent_k1_bench_seqs_per_s")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import hudiff_amd
    from hudiff_amd import evalsets as E, scoring, synthetic as S
    from hudiff_amd.sampler import Job
    kind, B = args.kind, args.batch
    cfg = dict(S.AB_CONFIG if kind == "ab" else S.NB_CONFIG)
    sd = S.random_state_dict(kind, cfg, seed=0)
    batch = E.eval_batch("huab348" if kind == "ab" else "vhh", B, mode="finetune" if kind == "ab" else "plain", row0=0, seed=2023)
    T, order = batch["T"], batch["order"]
    model = (hudiff_amd.AntiTFNet if kind == "ab" else hudiff_amd.NanoAntiTFNet)(**cfg, device=0)
    model.load_state_dict(sd)
    visited = np.zeros(batch["tokens"].shape, bool)
    for b in range(B):
        visited[b, order[b, :T[b]]] = True
    parent = None
    if args.parent_bench_json:
        with open(args.parent_bench_json) as f:
            parent = float(json.loads(f.read().strip().splitlines()[-1])["value"])
    results, first = [], {}
    for K in [int(k) for k in args.ks.split(",")]:
        t1 = min(-(-int(T.max()) // K) * K, order.shape[1])
        model.sample_begin(batch["tokens"], batch["region"], batch["chain"], order, T, seed=2023, row0=0, dropout=args.dropout,
                           slots_per_step=K)
        gpu_ms, t0 = 0.0, 0.0
        for i in range(-args.warmup, args.steps):
            if i == 0:
                model.sync()
                t0 = time.perf_counter()
            model.sample_restart(2023 + 7919 * i)
            model.sample_run(0, t1)
            if i >= 0:
                model.sync()
                gpu_ms += model.last_run_ms()[0]
        elapsed = time.perf_counter() - t0
        # outside the timed window: the sample of the first timed seed once more, for the quality columns
        model.sample_restart(2023)
        model.sample_run(0, t1)
        first[K] = model.sample_end()
        r = {"slots_per_step": K, "kind": kind, "rows": B, "samples": args.steps, "dropout": args.dropout,
             "seqs_per_s": B * args.steps / elapsed, "gpu_ms_per_sample": gpu_ms / args.steps,
             "forwards_per_row": float(np.mean(-(-T // K))), "mean_T": float(T.mean()), "route": model.precision_info()["precision"]}
        if parent is not None:
            r["parent_k1_bench_seqs_per_s"] = parent
        if 1 in first:
            r["differs_from_k1"] = float((first[K] != first[1])[visited].mean())
        results.append(r)
    if args.orders > 0:
        for r in results:
            tok = first[r["slots_per_step"]]
            jobs = [Job(tokens=tok[b], region=batch["region"][b], loc=order[b, :T[b]],
                        chain=None if kind == "nb" else (int(batch["chain"][b]), int(batch["chain"][B + b])), name=str(b)) for b in range(B)]
            res = scoring.score_jobs(model, jobs, orders=args.orders, seed=11, dropout="off", parallel=False, device_batch=B)
            r["logp_per_residue"] = float(res["per_residue"].mean())
            r["logp_per_residue_std_over_rows"] = float(res["per_residue"].std())
            r["score_orders"] = args.orders
    model.close()
    for r in results:
        print(json.dumps(r), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(results, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
