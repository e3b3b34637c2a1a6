"""Device time of a truncated sampling step beside an untruncated one (profiles/truncate/README.md): hd_last_run_ms of 20 steps of ONE
resident 256-row production-width session on the HuAb348 rows (hudiff_amd/data/real_rows.npz), in three legs: untruncated, top_p 0.9,
and all three cuts at once (top_k 8, top_p 0.8, min_p 0.05).

Random production-width weights and dropout off, as scripts/guide_timings.py.  Each leg keeps its session open: one warm-up run of the
20 steps (graph capture, code objects), then `--reps` timed runs, each behind a restart and a synchronise; the legs alternate `--rounds`
times so that drift of the shared machine shows in all of them.  On a tree without hudiff_amd.guide.Truncation (the parent commit) only
the untruncated leg runs.  Prints one JSON object.

    python scripts/truncate_timings.py [--rows 256] [--steps 20] [--reps 5] [--rounds 3]
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
    legs = {"untruncated": None}
    try:
        from hudiff_amd.guide import Truncation
        legs["top_p_0.9"] = Truncation(top_p=0.9)
        legs["top_k_8_top_p_0.8_min_p_0.05"] = Truncation(8, 0.8, 0.05)
    except ImportError:
        pass
    cfg = dict(S.AB_CONFIG, dropout=0.0)
    model = hudiff_amd.AntiTFNet(**cfg, precision=args.precision)
    model.load_state_dict(S.random_state_dict("ab", cfg, seed=0))
    b = E.eval_batch("huab348", args.rows, mode="finetune")
    a = (b["tokens"], b["region"], b["chain"], b["order"], b["T"])
    assert int(b["T"].min()) >= args.steps
    runs = {name: [] for name in legs}
    for _ in range(args.rounds):
        for name, tr in legs.items():
            model.sample_begin(*a, seed=2023, dropout="off", **({} if tr is None else {"truncation": tr}))
            runs[name] += timed(model, args.steps, args.reps)
            model.sample_end()
    res = {"device": hudiff_amd.device_info(0)["name"], "precision": model.precision_info()["precision"], "rows": args.rows,
           "steps": args.steps, "reps": args.reps, "rounds": args.rounds}
    for name, ms in runs.items():
        per = np.array(ms) / args.steps
        res[name] = {"ms_per_step_median": float(np.median(per)), "ms_per_step_min": float(per.min()), "ms_per_step_max": float(per.max()),
                     "runs_ms": [round(float(x), 3) for x in ms]}
    res["precision_report"] = model.precision_info()
    model.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
