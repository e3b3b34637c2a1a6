"""Device time of likelihood scoring beside sampling (profiles/logp/README.md): hd_last_run_ms of

  1. ONE HuAb348 antibody (B = 1, T ~ 150): the sequential teacher-forced loop against the step-parallel form (every step a
     row of one device batch, chunks of --device-batch rows);
  2. 256 rows: sampling, sampling with HD_RECORD_LOGP, sequential scoring of the sampled tokens.

Production-width random weights and real HuAb348 rows, as bench.py; dropout off (step-parallel scoring needs it), one warm-up
before `--reps` timed repetitions of every leg; prints one JSON object.

    python scripts/logp_timings.py [--rows 256] [--reps 3] [--device-batch 256]
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
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--device-batch", type=int, default=256)
    ap.add_argument("--precision", default="default")
    args = ap.parse_args()
    import hudiff_amd
    from hudiff_amd import evalsets as E
    from hudiff_amd import scoring
    from hudiff_amd import synthetic as S
    cfg = dict(S.AB_CONFIG, dropout=0.0)
    model = hudiff_amd.AntiTFNet(**cfg, precision=args.precision)
    model.load_state_dict(S.random_state_dict("ab", cfg, seed=0))
    res = {"device": hudiff_amd.device_info(0)["name"], "precision": model.precision_info()["precision"], "reps": args.reps}

    # ---- 1. one antibody --------------------------------------------------------------------------------------------------------
    one = E.eval_batch("huab348", 1, mode="finetune")
    T1 = int(one["T"][0])
    a1 = (one["truth"], one["region"], one["chain"], one["order"], one["T"])
    model.score_begin(*a1)
    seq_ms = timed(model, lambda: model.sample_run(0, T1), args.reps)
    model.sample_end()
    seq_lp = model.sample_logp()
    x = scoring.expand_steps(*a1)
    n = x.tokens.shape[0]
    x.tokens[np.arange(n), x.order[:, 0]] = one["truth"][x.rows, x.order[:, 0]]        # hd_score takes its targets from the tokens
    par_ms, par_lp = np.zeros(args.reps), np.zeros(n, np.float32)
    for s in range(0, n, args.device_batch):
        e = min(n, s + args.device_batch)
        ch = np.concatenate([x.chain[s:e], x.chain[n + s:n + e]])
        model.score_begin(x.tokens[s:e], x.region[s:e], ch, x.order[s:e], x.T[s:e])
        par_ms += np.array(timed(model, lambda: model.sample_run(0, 1), args.reps))
        model.sample_end()
        par_lp[s:e] = model.sample_logp()[:, 0]
    res["one_antibody"] = {"T": T1, "sequential_ms": seq_ms, "step_parallel_ms": par_ms.tolist(),
                           "sequential_seq_per_s": 1e3 / float(np.mean(seq_ms)), "step_parallel_seq_per_s": 1e3 / float(np.mean(par_ms)),
                           "forwards_per_s_parallel": T1 * 1e3 / float(np.mean(par_ms)),
                           "max_abs_diff_logp": float(np.abs(x.fold(par_lp, seq_lp.shape[1]) - seq_lp).max()),
                           "total_logp": float(seq_lp.sum())}

    # ---- 2. a device batch ------------------------------------------------------------------------------------------------------
    B = args.rows
    b = E.eval_batch("huab348", B, mode="finetune")
    Tmax = int(b["T"].max())
    a = (b["region"], b["chain"], b["order"], b["T"])
    legs = {}
    model.sample_begin(b["tokens"], *a, seed=2023, dropout="off")
    legs["sample_ms"] = timed(model, lambda: model.sample_run(0, Tmax), args.reps)
    tok = model.sample_end()
    model.sample_begin(b["tokens"], *a, seed=2023, dropout="off", record_logp=True)
    legs["sample_record_logp_ms"] = timed(model, lambda: model.sample_run(0, Tmax), args.reps)
    tok_r = model.sample_end()
    rec = model.sample_logp()
    model.score_begin(tok_r, *a)
    legs["score_sequential_ms"] = timed(model, lambda: model.sample_run(0, Tmax), args.reps)
    model.sample_end()
    sc = model.sample_logp()
    legs.update(rows=B, Tmax=Tmax, tokens_equal_with_and_without_recording=bool(np.array_equal(tok, tok_r)),
                max_abs_diff_recorded_vs_scored=float(np.abs(rec - sc).max()))
    for k in ("sample", "sample_record_logp", "score_sequential"):
        legs[k + "_seq_per_s"] = B * 1e3 / float(np.mean(legs[k + "_ms"]))
    res["batch"] = legs
    res["precision_report"] = model.precision_info()
    model.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
