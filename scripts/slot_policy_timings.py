"""Slot policy: what the selection stage costs per denoiser forward, and what the samples' own log-likelihood is.

    python scripts/slot_policy_timings.py --ks 1,4,16 --repeats 3 --out profiles/slot_policy/timings.json

One process, one handle, one resident batch (bench.py's workload: HuAb348 pairs, 256 rows, the library's default route, seeded
N(0, 0.02) weights).  Per K the two sessions -- slot_policy "given" and "confident", both recording -- are opened in turn and ALTERNATE
`--repeats` times after one warm-up each, so that clock and thermal drift fall on both alike; every repeat is a restart plus all order
positions, timed by the library's own HIP events (hd_last_run_ms).

Per (K, policy) one JSON line:
  forwards            denoiser forwards of one sample = ceil(max T / K)
  gpu_ms_per_forward  median over the repeats of hd_last_run_ms / forwards          gpu_ms_all   every repeat's value
  logp_per_residue    mean over rows of sum_t logp[b, t] / T[b] of the last repeat: the exact per-residue log-likelihood of the sample
                      under the sampler that drew it (not comparable across K as a quality measure: score at K = 1 for that)
  moved_rows          rows whose realised order differs from the list (confident only)
and per K one line `"policy": "delta"` with confident - given in ms per forward and in percent.
At K = 1 the given-order session prunes its last attention block to the visited row and the confident one cannot, so that delta
holds the unpruned block as well as the selection; `--given_unpruned` times the given-order session with prune=False instead.
"""
from __future__ import annotations

import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ks", default="1,4,16")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--kind", choices=["ab", "nb"], default="ab")
    ap.add_argument("--dropout", choices=["faithful", "off"], default="faithful")
    ap.add_argument("--given_unpruned", action="store_true", help="time the given-order session with prune=False (matters at K = 1 only)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import hudiff_amd
    from hudiff_amd import evalsets as E, synthetic as S
    kind, B = args.kind, args.batch
    cfg = dict(S.AB_CONFIG if kind == "ab" else S.NB_CONFIG)
    sd = S.random_state_dict(kind, cfg, seed=0)
    batch = E.eval_batch("huab348" if kind == "ab" else "vhh", B, mode="finetune" if kind == "ab" else "plain", row0=0, seed=2023)
    T, order = batch["T"], batch["order"]
    model = (hudiff_amd.AntiTFNet if kind == "ab" else hudiff_amd.NanoAntiTFNet)(**cfg, device=0)
    model.load_state_dict(sd)
    lines = []
    try:
        for K in [int(k) for k in args.ks.split(",")]:
            t1 = min(-(-int(T.max()) // K) * K, order.shape[1])
            forwards = -(-t1 // K)
            ms = {"given": [], "confident": []}
            last = {}
            for rep in range(-1, args.repeats):
                for policy in ("given", "confident"):
                    model.sample_begin(batch["tokens"], batch["region"], batch["chain"], order, T, seed=2023 + 7919 * max(rep, 0), row0=0,
                                       dropout=args.dropout, slots_per_step=K, slot_policy=policy, record_logp=True,
                                       prune=not (args.given_unpruned and policy == "given"))
                    model.sample_run(0, t1)
                    model.sync()
                    if rep >= 0:
                        ms[policy].append(model.last_run_ms()[0] / forwards)
                    last[policy] = (model.sample_logp(), model.sample_order())
                    model.sample_end()
            for policy in ("given", "confident"):
                lp, R = last[policy]
                per = lp.astype(np.float64).sum(axis=1) / np.maximum(T, 1)
                line = {"kind": kind, "rows": B, "K": K, "policy": policy, "dropout": args.dropout, "forwards": forwards,
                        "gpu_ms_per_forward": float(np.median(ms[policy])), "gpu_ms_all": [round(float(v), 4) for v in ms[policy]],
                        "logp_per_residue": float(per[T > 0].mean())}
                if policy == "confident":
                    line["moved_rows"] = int(sum(not np.array_equal(R[b], order[b]) for b in range(B)))
                if policy == "given" and args.given_unpruned:
                    line["unpruned"] = True
                lines.append(line)
                print(json.dumps(line), flush=True)
            g, c = float(np.median(ms["given"])), float(np.median(ms["confident"]))
            line = {"kind": kind, "rows": B, "K": K, "policy": "delta", "ms_per_forward": c - g, "percent": 100.0 * (c - g) / g}
            lines.append(line)
            print(json.dumps(line), flush=True)
    finally:
        model.close()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
