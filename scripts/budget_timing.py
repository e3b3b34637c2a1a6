"""Device time of a recording step with and without a mutation budget (profiles/budget/README.md): hd_last_run_ms of 16 order positions
of ONE resident 256-row production-width recording session on the HuAb348 rows (hudiff_amd/data/real_rows.npz), in three legs: the
plain recording session (the plain draw kernel), the same session under the neutral guide (the guided draw kernel a budgeted session
runs on), and the budgeted session (max_mutations = 2 against the rows' own residues: with random weights every row is exhausted
after two positions, so most draws take the forced path).  The denoiser forward is the same work in all three; the legs differ in the
draw launch only.

Random production-width weights and dropout off, as scripts/beam_timing.py.  Each leg keeps its session open: one warm-up run of the
positions (graph capture, code objects), then `--reps` timed runs, each behind a restart and a synchronise; the legs alternate
`--rounds` times so that drift of the shared machine shows in all of them.  Prints one JSON object.

    python scripts/budget_timing.py [--rows 256] [--steps 16] [--reps 5] [--rounds 3] [--max_mutations 2]
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def timed(model, steps, reps):
    """[ms] of `reps` runs of positions [0, steps) of the open session after one warm-up; every run restarts the session."""
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
    ap.add_argument("--steps", type=int, default=16)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--max_mutations", type=int, default=2)
    ap.add_argument("--precision", default="default")
    args = ap.parse_args()
    import hudiff_amd
    from hudiff_amd import evalsets as E
    from hudiff_amd import synthetic as S
    from hudiff_amd.guide import FREE, Budget, Guide
    B = args.rows
    cfg = dict(S.AB_CONFIG, dropout=0.0)
    model = hudiff_amd.AntiTFNet(**cfg, precision=args.precision)
    model.load_state_dict(S.random_state_dict("ab", cfg, seed=0))
    b = E.eval_batch("huab348", B, mode="finetune")
    assert int(b["T"].min()) >= args.steps
    order = np.ascontiguousarray(b["order"][:, :args.steps])
    T = np.full(B, args.steps, np.int32)
    budget = Budget(np.where(b["truth"] <= 21, b["truth"], FREE), np.full(B, args.max_mutations, np.int32))

    def begin(**kw):
        model.sample_begin(b["tokens"], b["region"], b["chain"], order, T, seed=2023, dropout="off", record_logp=True, **kw)
    legs = {"record_plain": lambda: begin(), "record_neutral_guide": lambda: begin(guide=Guide()),
            f"record_budget_m{args.max_mutations}": lambda: begin(budget=budget)}
    runs = {name: [] for name in legs}
    counts = None
    for _ in range(args.rounds):
        for name, start in legs.items():
            start()
            runs[name] += timed(model, args.steps, args.reps)
            if "budget" in name:
                counts = model.mutation_count()
            model.sample_end()
    res = {"device": hudiff_amd.device_info(0)["name"], "precision": model.precision_info()["precision"], "rows": B,
           "steps": args.steps, "reps": args.reps, "rounds": args.rounds,
           "rows_exhausted": int((counts >= args.max_mutations).sum()), "mutations_max": int(counts.max())}
    for name, ms in runs.items():
        per = np.array(ms) / args.steps
        res[name] = {"ms_per_step_median": float(np.median(per)), "ms_per_step_min": float(per.min()), "ms_per_step_max": float(per.max()),
                     "runs_ms": [round(float(x), 3) for x in ms]}
    res["precision_report"] = model.precision_info()
    model.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
