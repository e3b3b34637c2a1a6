"""Device time of a recording step with and without the distribution record (profiles/slot_dist/README.md): hd_last_run_ms of 16 order
positions of ONE resident 256-row production-width recording session on the HuAb348 rows (hudiff_amd/data/real_rows.npz), in two legs:
the recording session (HD_RECORD_LOGP) and the same session with HD_RECORD_DIST.  The denoiser forward and the draw launch are the same
in both; the second leg's draw stores 88 more bytes per row.

Random production-width weights and dropout off, as scripts/budget_timing.py.  Each leg keeps its session open: one warm-up run of the
positions (graph capture, code objects), then `--reps` timed runs, each behind a restart and a synchronise; the legs alternate
`--rounds` times so that drift of the shared machine shows in both.  `--scan N` adds the wall time of a mutational scan
(scoring.scan_jobs, context "given") of the first N HuAb348 pairs on the same handle.  Prints one JSON object.

    python scripts/dist_timing.py [--rows 256] [--steps 16] [--reps 5] [--rounds 3] [--scan 348]
"""
import argparse
import json
import os
import sys
import time

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
    ap.add_argument("--scan", type=int, default=0, help="also time a context='given' scan of this many HuAb348 pairs (0 = none)")
    ap.add_argument("--precision", default="default")
    args = ap.parse_args()
    import hudiff_amd
    from hudiff_amd import evalsets as E
    from hudiff_amd import synthetic as S
    B = args.rows
    cfg = dict(S.AB_CONFIG, dropout=0.0)
    model = hudiff_amd.AntiTFNet(**cfg, precision=args.precision)
    model.load_state_dict(S.random_state_dict("ab", cfg, seed=0))
    b = E.eval_batch("huab348", B, mode="finetune")
    assert int(b["T"].min()) >= args.steps
    order = np.ascontiguousarray(b["order"][:, :args.steps])
    T = np.full(B, args.steps, np.int32)

    def begin(**kw):
        model.sample_begin(b["tokens"], b["region"], b["chain"], order, T, seed=2023, dropout="off", **kw)
    legs = {"record_logp": lambda: begin(record_logp=True), "record_dist": lambda: begin(record_dist=True)}
    runs = {name: [] for name in legs}
    logp = {}
    for _ in range(args.rounds):
        for name, start in legs.items():
            start()
            runs[name] += timed(model, args.steps, args.reps)
            logp[name] = model.sample_logp()
            model.sample_end()
    res = {"device": hudiff_amd.device_info(0)["name"], "precision": model.precision_info()["precision"], "rows": B,
           "steps": args.steps, "reps": args.reps, "rounds": args.rounds,
           "logp_bit_equal": bool(logp["record_logp"].tobytes() == logp["record_dist"].tobytes())}
    for name, ms in runs.items():
        per = np.array(ms) / args.steps
        res[name] = {"ms_per_step_median": float(np.median(per)), "ms_per_step_min": float(per.min()), "ms_per_step_max": float(per.max()),
                     "runs_ms": [round(float(x), 3) for x in ms]}
    if args.scan:
        from hudiff_amd.sampler import Job
        from hudiff_amd.scoring import scan_jobs
        s = E.eval_batch("huab348", args.scan, mode="finetune")
        jobs = [Job(tokens=s["truth"][r].astype(np.int32), region=s["region"][r].astype(np.int32), loc=np.sort(s["order"][r, :s["T"][r]]),
                    chain=(int(s["chain"][r]), int(s["chain"][args.scan + r])), name=str(r)) for r in range(args.scan)]
        t0 = time.perf_counter()
        out = scan_jobs(model, jobs, context="given", device_batch=B)
        res["scan"] = {"pairs": args.scan, "rows": int(out["T"].sum()), "wall_s": round(time.perf_counter() - t0, 3),
                       "pseudo_ll_mean": float(out["pseudo_ll"].mean())}
    res["precision_report"] = model.precision_info()
    model.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
