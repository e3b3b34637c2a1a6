"""Device time of a guided sampling step beside an unguided one (profiles/guide/README.md): hd_last_run_ms of 20 steps of ONE resident
256-row production-width session on the HuAb348 rows (hudiff_amd/data/real_rows.npz), unguided and guided (C and M forbidden
everywhere, temperature 0.7).

Random production-width weights and dropout off, as scripts/logp_timings.py.  Each leg keeps its session open: one warm-up run of the
20 steps (graph capture, code objects), then `--reps` timed runs, each behind a restart and a synchronise; the two legs alternate
`--rounds` times so that drift of the shared machine shows in both.  On a tree without hudiff_amd.guide (the parent commit) only the
unguided leg runs.  Prints one JSON object.

    python scripts/guide_timings.py [--rows 256] [--steps 20] [--reps 5] [--rounds 3]
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def timed(model, steps, reps):
    """[ms] of `reps` runs of steps [0, steps) of the open session after one warm-up; every run restarts the session."""
    out = []
    for i in range(-1, reps):
        model.sample_restart(2023 + i)
        model.sync()
        model.sample_run(0, steps)
        model.sync()
        if i >= 0:
            out.append(model.last_run_ms()[0])
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=256)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--precision", default="default")
    args = ap.parse_args()
    import hudiff_amd
    from hudiff_amd import evalsets as E
    from hudiff_amd import synthetic as S
    try:
        from hudiff_amd.guide import ALL_TOKENS, Guide, letters_mask
        guide = Guide(np.full(S.AB_CONFIG["max_len"], ALL_TOKENS & ~letters_mask("CM"), np.uint32), None, 0.7)
    except ImportError:
        guide = None
    cfg = dict(S.AB_CONFIG, dropout=0.0)
    model = hudiff_amd.AntiTFNet(**cfg, precision=args.precision)
    model.load_state_dict(S.random_state_dict("ab", cfg, seed=0))
    b = E.eval_batch("huab348", args.rows, mode="finetune")
    a = (b["tokens"], b["region"], b["chain"], b["order"], b["T"])
    assert int(b["T"].min()) >= args.steps
    legs = {"unguided": []} if guide is None else {"unguided": [], "guided": []}
    for _ in range(args.rounds):
        for name in legs:
            model.sample_begin(*a, seed=2023, dropout="off", **({"guide": guide} if name == "guided" else {}))
            legs[name] += timed(model, args.steps, args.reps)
            model.sample_end()
    res = {"device": hudiff_amd.device_info(0)["name"], "precision": model.precision_info()["precision"], "rows": args.rows,
           "steps": args.steps, "reps": args.reps, "rounds": args.rounds}
    for name, ms in legs.items():
        per = np.array(ms) / args.steps
        res[name] = {"ms_per_step_median": float(np.median(per)), "ms_per_step_min": float(per.min()), "ms_per_step_max": float(per.max()),
                     "runs_ms": [round(float(x), 3) for x in ms]}
    res["precision_report"] = model.precision_info()
    model.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
