"""Refinement rounds against the host-chained form (profiles/refine/README.md): wall time of one sample of a resident 256-row
production-width HuAb348 batch under the confident policy at K slots per step, followed by `--rounds` refinement rounds of `--slots`
slots, in two legs:

  refined   ONE session with refine=dict(rounds, slots): sample_restart, every order position up to its Tmax, synchronise.
  chained   what a caller had to write before: the same first pass (recording), then per round -- read logp and order back, pick every
            row's `slots` least likely positions in numpy, end the session, begin a new one on the re-masked tokens whose list is the
            chosen slots, run it, read its record back.  It uses nothing this feature added (the selection is spelled out below), so
            `--legs chained` runs unchanged on the parent commit.

The clock of a leg starts before its restart / first begin and stops behind its last synchronise; one warm-up sample per leg (graph
capture), then `--reps` timed ones, one leg after the other.  The chained leg's later rounds draw with other noise keys than the refined
session's (its positions start at 0 again), so the two legs' samples differ; both are samples of the same procedure.

`--orders N` > 0 adds the quality columns by the method of profiles/block/README.md: the first timed sample of each leg, and the
unrefined first pass, scored with one slot per forward (dropout off) along N random visiting orders; mean per-residue log-likelihood
over the rows.  With the seeded N(0, 0.02) weights these columns show the method only.  Prints one JSON object.

    python scripts/refine_timing.py [--rows 256] [--k 8] [--rounds 2] [--slots 8] [--reps 3] [--orders 8] [--legs refined,chained]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def least_likely(slot_lp, listed, slots):
    """Per row: the `slots` listed slots with the smallest log-probability of their last draw, among those with logp < 0."""
    out = []
    for b in range(len(slot_lp)):
        s = np.flatnonzero(listed[b] & (slot_lp[b] < 0))
        out.append(s[np.argsort(slot_lp[b, s], kind="stable")][:slots])
    return out


def note(slot_lp, logp, order, T):
    """The record of a session, by slot: the last draw of a slot is the one that counts."""
    for b in range(len(T)):
        slot_lp[b, order[b, :T[b]]] = logp[b, :T[b]]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=256)
    ap.add_argument("--k", type=int, default=8)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--slots", type=int, default=8)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--orders", type=int, default=8)
    ap.add_argument("--legs", default="refined,chained")
    ap.add_argument("--dropout", default="faithful")
    args = ap.parse_args()
    import hudiff_amd
    from hudiff_amd import evalsets as E, scoring, synthetic as S
    from hudiff_amd.sampler import Job
    B, K, R = args.rows, args.k, args.slots
    cfg = dict(S.AB_CONFIG)
    model = hudiff_amd.AntiTFNet(**cfg, device=0)
    model.load_state_dict(S.random_state_dict("ab", cfg, seed=0))
    batch = E.eval_batch("huab348", B, mode="finetune", row0=0, seed=2023)
    T, order = batch["T"], batch["order"]
    base = (batch["tokens"], batch["region"], batch["chain"])
    ckw = dict(row0=0, dropout=args.dropout, slots_per_step=K, slot_policy="confident")
    t_first = min(-(-int(T.max()) // K) * K, order.shape[1])
    legs = [x for x in args.legs.split(",") if x]
    res = {"device": hudiff_amd.device_info(0)["name"], "precision": model.precision_info()["precision"], "rows": B, "slots_per_step": K,
           "rounds": args.rounds, "slots": R, "reps": args.reps, "dropout": args.dropout, "mean_T": float(T.mean())}
    samples = {}
    listed = np.zeros(batch["tokens"].shape, bool)
    for b in range(B):
        listed[b, order[b, :T[b]]] = True

    def refined(seed):
        model.sample_restart(seed)
        model.sample_run(0, model._session_Tmax)
        model.sync()

    def chained(seed, keep=None):
        model.sample_begin(*base, order, T, seed=seed, record_logp=True, **ckw)
        model.sample_run(0, t_first)
        lp, od = model.sample_logp(), model.sample_order()
        tok = model.sample_end()
        if keep is not None:
            keep["first_pass"] = tok.copy()
        slot_lp = np.zeros(tok.shape, np.float32)
        note(slot_lp, lp, od, T)
        for r in range(args.rounds):
            pick = least_likely(slot_lp, listed, R)
            tok = tok.copy()
            order2, T2 = np.zeros((B, R), np.int32), np.zeros(B, np.int32)
            for b, s in enumerate(pick):
                tok[b, s] = 22
                order2[b, :len(s)] = s
                T2[b] = len(s)
            model.sample_begin(tok, base[1], base[2], order2, T2, seed=seed + 1 + r, record_logp=True, **ckw)
            model.sample_run(0, R)
            lp, od = model.sample_logp(), model.sample_order()
            tok = model.sample_end()
            note(slot_lp, lp, od, T2)
        return tok

    times = {leg: [] for leg in legs}
    if "refined" in legs:
        model.sample_begin(*base, order, T, seed=2023, refine=dict(rounds=args.rounds, slots=R), **ckw)
        res["refined_Tmax"] = model._session_Tmax
        for i in range(-1, args.reps):
            t0 = time.perf_counter()
            refined(2023 + 7919 * max(i, 0))
            if i >= 0:
                times["refined"].append(time.perf_counter() - t0)
            if i == 0:
                samples["refined"] = model.sample_tokens()
                res["redrawn_per_row_mean"] = float(model.refine_state()[2].sum(axis=1).mean())
        model.sample_end()
    if "chained" in legs:
        for i in range(-1, args.reps):
            keep = {} if i == 0 else None
            t0 = time.perf_counter()
            tok = chained(2023 + 7919 * max(i, 0), keep)
            if i >= 0:
                times["chained"].append(time.perf_counter() - t0)
            if i == 0:
                samples["chained"], samples["first_pass"] = tok, keep["first_pass"]
    for leg in legs:
        res[leg] = {"wall_s_median": float(np.median(times[leg])), "wall_s_min": float(min(times[leg])), "wall_s_max": float(max(times[leg])),
                    "seqs_per_s": float(B / np.median(times[leg])), "runs_s": [round(x, 4) for x in times[leg]]}
    if args.orders > 0:
        for name, tok in samples.items():
            jobs = [Job(tokens=tok[b], region=batch["region"][b], loc=order[b, :T[b]], chain=(int(batch["chain"][b]), int(batch["chain"][B + b])),
                        name=str(b)) for b in range(B)]
            sc = scoring.score_jobs(model, jobs, orders=args.orders, seed=11, dropout="off", parallel=False, device_batch=B)
            res[f"logp_per_residue_{name}"] = float(sc["per_residue"].mean())
            res[f"logp_per_residue_{name}_std_over_rows"] = float(sc["per_residue"].std())
        res["score_orders"] = args.orders
    res["precision_report"] = model.precision_info()
    model.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
