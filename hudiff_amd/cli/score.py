"""Log-likelihood of given sequences under a HuDiff checkpoint (no counterpart in the reference, which only samples).

    python -m hudiff_amd.cli.score --kind ab --ckpt checkpoints/antibody/hudiffab.pt --data_fpath pairs.csv --orders 8
    python -m hudiff_amd.cli.score --kind nb --ckpt hudiffnb.pt --data_fpath sample_humanization_result.csv --mask inpaint

Every row of ``--data_fpath`` is scored: a pairs CSV (columns ``h_seq``, ``l_seq``, optional ``name`` / ``type``), a VHH CSV (column
``vhhseq``) or a ``sample_humanization_result.csv`` written by the samplers (columns ``name``, ``hseq``[, ``lseq``]).  ``--mask``
chooses WHICH slots are scored, with the samplers' own mask modes -- the score is the log-probability of the residues in those
slots given everything outside them: antibody ``finetune`` (framework outside the Kabat CDRs and the Vernier zone; empty slots are
context) or ``pretrain`` (framework outside the CDR-IMGT; empty slots are scored as gaps), nanobody ``plain`` / ``inpaint``
(``--inpaint_sample False`` / ``True`` of the nanobody sampler).  The slots are visited in ``--orders`` random orders
(a function of --seed, the row and the order's index); each order gives one estimate ``sum_t log p(x_t | x_<t)``.

Output ``--out_fpath`` (default: ``score_result.csv`` beside the data file): ``name,T,logp_mean,logp_std,logp_per_residue`` --
T scored slots, mean and standard deviation of the per-order totals, mean / T.
"""
from __future__ import annotations

import argparse
import os

import numpy as np

from .. import dist as D
from .. import inputs as I
from ..checkpoint import antibody_model_from_checkpoint, load_checkpoint, nanobody_model_from_checkpoint
from ..model import NanoAntiTFNet, model_selected
from ..sampler import Job
from ..scoring import score_jobs
from .common import add_block_args, add_runtime_args, apply_block_args, check_confidence_args, load_numbered, relaunch_if_asked

MASKS = {"ab": ("finetune", "pretrain"), "nb": ("plain", "inpaint")}


def build_parser():
    p = argparse.ArgumentParser()
    p.add_argument("--ckpt", type=str, required=True)
    p.add_argument("--kind", choices=["ab", "nb"], required=True)
    p.add_argument("--data_fpath", type=str, required=True,
                   help="pairs CSV (h_seq, l_seq[, name, type]), VHH CSV (vhhseq) or a sample_humanization_result.csv")
    p.add_argument("--numbered_fpath", type=str, default=None,
                   help="JSON-lines file with pre-numbered IMGT residues, one object per row of --data_fpath")
    p.add_argument("--numbering", choices=["auto", "anarci", "builtin"], default="auto")
    p.add_argument("--orders", type=int, default=1, help="visiting orders per sequence (each is one estimate of the log-likelihood)")
    p.add_argument("--seed", type=int, default=2023)
    p.add_argument("--mask", type=str, default=None,
                   help="which slots are scored, the samplers' mask modes: ab finetune (default) | pretrain, nb plain (default) | inpaint")
    p.add_argument("--dropout", choices=["off", "faithful"], default="off",
                   help="off = the deterministic network, step-parallel scoring; faithful = the reference's inference-time dropout "
                        "(generated masks keyed by row and step), which needs the sequential loop")
    p.add_argument("--device_batch", type=int, default=256, help="rows per device launch")
    p.add_argument("--device", type=int, default=None)
    p.add_argument("--out_fpath", type=str, default=None)
    add_block_args(p)
    add_runtime_args(p)
    return p


def read_rows(fpath, kind):
    """-> [(name, heavy sequence, light sequence or None)] for every row of the file."""
    import pandas as pd
    df = pd.read_csv(fpath, index_col=False)
    cols = set(df.columns)
    rows = []
    if kind == "ab":
        hc, lc = ("h_seq", "l_seq") if "h_seq" in cols else ("hseq", "lseq")
        if hc not in cols or lc not in cols:
            raise ValueError(f"{fpath}: an antibody input needs the columns h_seq, l_seq (pairs CSV) or hseq, lseq (sampler output)")
        for i, line in enumerate(df.itertuples()):
            rows.append((str(getattr(line, "name", i)), getattr(line, hc), getattr(line, lc)))
    else:
        hc = "vhhseq" if "vhhseq" in cols else "hseq"
        if hc not in cols:
            raise ValueError(f"{fpath}: a nanobody input needs the column vhhseq (VHH CSV) or hseq (sampler output)")
        for i, line in enumerate(df.itertuples()):
            rows.append((str(getattr(line, "name", i)), getattr(line, hc), None))
    return rows


def build_jobs(rows, kind, mask, numbered, numbering, pad_region=0):
    """Complete tokens + the slots the chosen mask mode would sample."""
    jobs = []
    for idx, (name, h_seq, l_seq) in enumerate(rows):
        if kind == "ab":
            if numbered is not None:
                h_dict, l_dict, l_type = numbered[idx]["h"], numbered[idx]["l"], numbered[idx].get("l_chain", "K")
            else:
                h_dict, _ = I.number_sequence(h_seq, numbering)
                l_dict, l_type = I.number_sequence(l_seq, numbering)
            full = np.array(I._TK.seq2idx(I.slot_residues(h_dict, "H") + I.slot_residues(l_dict, "L")), np.int32)
            _, reg, chain, loc = I.antibody_row_from_tokens(full, I._TK.chain_type_idx(l_type), finetune=mask == "finetune",
                                                            pad_region=pad_region)
            jobs.append(Job(tokens=full, region=reg, loc=loc, chain=chain, name=name))
        else:
            h_dict = numbered[idx]["h"] if numbered is not None else I.number_sequence(h_seq, numbering)[0]
            full = np.array(I._TK.seq2idx(I.slot_residues(h_dict, "H")), np.int32)
            _, reg, loc = I.nanobody_row_from_tokens(full, inpaint_sample=mask == "inpaint")
            jobs.append(Job(tokens=full, region=reg, loc=loc, name=name))
    return jobs


def write_scores(path, jobs, res):
    with open(path, "w", encoding="UTF-8") as f:
        f.write("name,T,logp_mean,logp_std,logp_per_residue\n")
        for j, job in enumerate(jobs):
            f.write(f"{job.name},{int(res['T'][j])},{res['mean'][j]:.6f},{res['std'][j]:.6f},{res['per_residue'][j]:.6f}\n")
    return path


def main(argv=None):
    parser = build_parser()
    args = check_confidence_args(parser, parser.parse_args(argv))
    if args.slot_policy == "confident" and args.orders > 1:
        parser.error("--slot_policy confident takes --orders 1: the visiting order is the model's own (only ties ever see the list)")
    rc = relaunch_if_asked(args, "hudiff_amd.cli.score", argv)
    if rc is not None:
        return rc
    mask = args.mask or MASKS[args.kind][0]
    if mask not in MASKS[args.kind]:
        raise SystemExit(f"--mask {mask}: --kind {args.kind} takes one of {', '.join(MASKS[args.kind])}")
    rank, world, local_rank = D.env_rank_world()
    D.init_process_group()
    device = args.device if args.device is not None else local_rank
    ckpt = load_checkpoint(args.ckpt)
    pad_region = 0
    if args.kind == "ab":
        # (the envelope says which training stage wrote the checkpoint; --mask alone chooses the slots)
        config, state, _ = antibody_model_from_checkpoint(ckpt, "finetune" if "pretrain_config" in ckpt else "pretrain")
        model = model_selected(config, device=device, precision=args.precision)
        n_region = config["model"]["n_region"] if "model" in config else config.model.n_region
        pad_region = 7 if n_region > 7 else 0
    else:
        _, params, state = nanobody_model_from_checkpoint(ckpt, "finetune_vh" if "infilling_params" in ckpt else "pretrain")
        model = NanoAntiTFNet(**params, device=device, precision=args.precision)
    model.load_state_dict(state)
    model.eval()
    rows = read_rows(args.data_fpath, args.kind)
    numbered = load_numbered(args.numbered_fpath) if args.numbered_fpath else None
    if numbered is not None and len(numbered) != len(rows):
        raise ValueError(f"{args.numbered_fpath}: {len(numbered)} rows for {len(rows)} input rows")
    jobs = build_jobs(rows, args.kind, mask, numbered, args.numbering, pad_region)
    res = score_jobs(model, jobs, orders=args.orders, seed=args.seed, dropout=args.dropout, device_batch=args.device_batch,
                     **apply_block_args(args, jobs))
    if rank != 0 or res is None:
        return None
    out = args.out_fpath or os.path.join(os.path.dirname(os.path.abspath(args.data_fpath)), "score_result.csv")
    return write_scores(out, jobs, res)


if __name__ == "__main__":
    _r = main()
    raise SystemExit(_r if isinstance(_r, int) else 0)      # an int is the exit code of a --gpus N relaunch
