"""Device time of a denoiser forward with and without a confidence threshold (profiles/threshold/README.md): hd_last_run_ms of
`--forwards` forwards of ONE resident 256-row production-width session on the HuAb348 rows (hudiff_amd/data/real_rows.npz), in three
legs at the same cap K: the confident K-session (the plain kernels), the same session under the neutral guide (the guided kernels a
threshold session runs on), and the threshold session.  The forward, the key launch, the selection launch and the draw launch are the
same grids in all three; the legs differ in what the selection counts and in how many of the K draw workgroups of a row are active.

Random production-width weights and dropout off, as scripts/budget_timing.py: their distributions are flat (no top probability above
0.26), so with the default tau no key qualifies and every forward of the threshold leg fills one slot per row; `--tau 0.15` sits near
their median key (rows take different counts) and `--tau 0.04` makes every key qualify (K per row).
Each leg keeps its session open: one warm-up run (graph capture, code objects), then `--reps` timed runs, each behind a restart and a
synchronise; the legs alternate `--rounds` times so that drift of the shared machine shows in all of them.  Prints one JSON object.

    python scripts/threshold_timing.py [--rows 256] [--forwards 4] [--cap 4] [--tau 0.5] [--reps 5] [--rounds 3]
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def timed(model, run, reps):
    """[ms] of `reps` runs of the open session after one warm-up; every run restarts the session."""
    out = []
    for i in range(-1, reps):
        model.sample_restart(2023 + i)
        model.sync()
        run()
        model.sync()
        if i >= 0:
            out.append(model.last_run_ms()[0])
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=256)
    ap.add_argument("--forwards", type=int, default=4)
    ap.add_argument("--cap", type=int, default=4)
    ap.add_argument("--tau", type=float, default=0.5)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--precision", default="default")
    args = ap.parse_args()
    import hudiff_amd
    from hudiff_amd import evalsets as E
    from hudiff_amd import synthetic as S
    from hudiff_amd.guide import Guide
    B, F, K = args.rows, args.forwards, args.cap
    cfg = dict(S.AB_CONFIG, dropout=0.0)
    model = hudiff_amd.AntiTFNet(**cfg, precision=args.precision)
    model.load_state_dict(S.random_state_dict("ab", cfg, seed=0))
    b = E.eval_batch("huab348", B, mode="finetune")
    Tn = F * K                                            # every leg has slots left in every one of its forwards
    assert int(b["T"].min()) >= Tn
    order = np.ascontiguousarray(b["order"][:, :Tn])
    T = np.full(B, Tn, np.int32)

    def begin(**kw):
        model.sample_begin(b["tokens"], b["region"], b["chain"], order, T, seed=2023, dropout="off", slots_per_step=K, slot_policy="confident", **kw)
    legs = {"confident": (lambda: begin(), lambda: model.sample_run(0, F * K)),
            "confident_neutral_guide": (lambda: begin(guide=Guide()), lambda: model.sample_run(0, F * K)),
            "threshold": (lambda: begin(confidence=args.tau), lambda: model.sample_run(0, F))}
    runs = {name: [] for name in legs}
    filled = None
    for _ in range(args.rounds):
        for name, (start, run) in legs.items():
            start()
            runs[name] += timed(model, run, args.reps)
            if name == "threshold":
                filled = model.sample_progress()
            model.sample_end()
    res = {"device": hudiff_amd.device_info(0)["name"], "precision": model.precision_info()["precision"], "rows": B, "forwards": F, "cap": K,
           "tau": args.tau, "reps": args.reps, "rounds": args.rounds,
           "threshold_slots_per_forward_mean": float(filled.mean() / F), "threshold_slots_per_forward_max_row": float(filled.max() / F)}
    for name, ms in runs.items():
        per = np.array(ms) / F
        res[name] = {"ms_per_forward_median": float(np.median(per)), "ms_per_forward_min": float(per.min()), "ms_per_forward_max": float(per.max()),
                     "runs_ms": [round(float(x), 3) for x in ms]}
    res["precision_report"] = model.precision_info()
    model.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
