"""Device time of a beam step beside a greedy recording step (profiles/beam/README.md): hd_last_run_ms of 16 order positions of ONE
resident 256-row production-width session on the HuAb348 rows (hudiff_amd/data/real_rows.npz), in two legs: the greedy decode
(temperature 0, HD_RECORD_LOGP) of 256 rows, and a beam session of G = 32 groups of width W = 8.  The denoiser forward is the same work
in both; the beam step issues beam_cand_k + beam_select_k where the greedy step issues one draw.

Random production-width weights and dropout off, as scripts/truncate_timings.py.  Each leg keeps its session open: one warm-up run of
the positions (graph capture, code objects), then `--reps` timed runs, each behind a restart and a synchronise; the legs alternate
`--rounds` times so that drift of the shared machine shows in both.  On a tree without beam search (the parent commit) only the greedy
leg runs.  Prints one JSON object.

    python scripts/beam_timing.py [--groups 32] [--width 8] [--steps 16] [--reps 5] [--rounds 3]
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
    ap.add_argument("--groups", type=int, default=32)
    ap.add_argument("--width", type=int, default=8)
    ap.add_argument("--steps", type=int, default=16)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--precision", default="default")
    args = ap.parse_args()
    import hudiff_amd
    from hudiff_amd import evalsets as E
    from hudiff_amd import synthetic as S
    from hudiff_amd.guide import Guide
    G, W = args.groups, args.width
    cfg = dict(S.AB_CONFIG, dropout=0.0)
    model = hudiff_amd.AntiTFNet(**cfg, precision=args.precision)
    model.load_state_dict(S.random_state_dict("ab", cfg, seed=0))
    b = E.eval_batch("huab348", G * W, mode="finetune")
    assert int(b["T"].min()) >= args.steps
    order = np.ascontiguousarray(b["order"][:, :args.steps])
    T = np.full(G * W, args.steps, np.int32)
    rep = np.repeat(np.arange(G), W)                         # the beam's rows: every group W copies of its first row
    legs = {"greedy_record": lambda: model.sample_begin(b["tokens"], b["region"], b["chain"], order, T, seed=2023, dropout="off",
                                                        record_logp=True, guide=Guide(temperature=0.0))}
    if hasattr(model, "beam_begin"):
        chain = np.concatenate([b["chain"][:G * W][rep * W], b["chain"][G * W:][rep * W]])
        legs[f"beam_w{W}_g{G}"] = lambda: model.beam_begin(b["tokens"][rep * W], b["region"][rep * W], chain, order[rep * W], T, W)
    runs = {name: [] for name in legs}
    for _ in range(args.rounds):
        for name, begin in legs.items():
            begin()
            runs[name] += timed(model, args.steps, args.reps)
            model.sample_end()
    res = {"device": hudiff_amd.device_info(0)["name"], "precision": model.precision_info()["precision"], "rows": G * W,
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
