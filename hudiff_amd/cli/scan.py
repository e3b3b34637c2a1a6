"""Mutational scan under a HuDiff checkpoint: the model's 22-token distribution at every scanned position of every sequence.

    python -m hudiff_amd.cli.scan --kind ab --ckpt checkpoints/antibody/hudiffab.pt --data_fpath pairs.csv
    python -m hudiff_amd.cli.scan --kind nb --ckpt hudiffnb.pt --data_fpath vhh.csv --mask inpaint --context masked

The inputs are those of ``hudiff_amd.cli.score``: every row of ``--data_fpath`` is scanned, ``--mask`` chooses WHICH slots with the
samplers' own mask modes.  ``--context given`` (default) asks, slot by slot, what the model accepts there with every other residue
known -- the pseudo-likelihood form, one forward per (sequence, slot); ``--context masked`` asks what the sampler meets at its first
step, with all scanned slots masked -- one forward per 64 slots.  The values are read from the device's distribution record
(include/hudiff_hip.h "distribution record"): one forward gives all 22, where scoring each substitution takes 22.

Output ``--out_fpath`` (default: ``scan_result.csv`` beside the data file), one row per (sequence, scanned position):
``name,chain,imgt,slot,wt,logp_wt,entropy`` and 22 columns ``lp_<letter>`` in ``guide.LETTERS`` order (``lp_gap`` for '-') -- the
log-probability of every residue there; the log-odds of a point mutation is its column minus ``logp_wt``.  -inf is written as ``-inf``.
"""
from __future__ import annotations

import argparse
import os

import numpy as np

from .. import dist as D
from .. import tables as TB
from ..checkpoint import antibody_model_from_checkpoint, load_checkpoint, nanobody_model_from_checkpoint
from ..guide import LETTERS
from ..model import NanoAntiTFNet, model_selected
from ..scoring import SCAN_CONTEXTS, scan_jobs
from .common import add_runtime_args, load_numbered, relaunch_if_asked
from .score import MASKS, build_jobs, read_rows

COLUMNS = ["name", "chain", "imgt", "slot", "wt", "logp_wt", "entropy"] + ["lp_" + ("gap" if c == "-" else c) for c in LETTERS]


def build_parser():
    p = argparse.ArgumentParser()
    p.add_argument("--ckpt", type=str, required=True)
    p.add_argument("--kind", choices=["ab", "nb"], required=True)
    p.add_argument("--data_fpath", type=str, required=True,
                   help="pairs CSV (h_seq, l_seq[, name, type]), VHH CSV (vhhseq) or a sample_humanization_result.csv")
    p.add_argument("--numbered_fpath", type=str, default=None,
                   help="JSON-lines file with pre-numbered IMGT residues, one object per row of --data_fpath")
    p.add_argument("--numbering", choices=["auto", "anarci", "builtin"], default="auto")
    p.add_argument("--mask", type=str, default=None,
                   help="which slots are scanned, the samplers' mask modes: ab finetune (default) | pretrain, nb plain (default) | inpaint")
    p.add_argument("--context", choices=list(SCAN_CONTEXTS), default="given",
                   help="given = every other residue is known (one forward per slot); masked = all scanned slots are masked, the "
                        "distribution the sampler meets at its first step (one forward per 64 slots)")
    p.add_argument("--device_batch", type=int, default=256, help="rows per device launch")
    p.add_argument("--device", type=int, default=None)
    p.add_argument("--out_fpath", type=str, default=None)
    add_runtime_args(p)
    return p


def slot_label(slot):
    """Slot of a row -> (chain letter, IMGT position): the heavy chain's 152 slots come first, then the light chain's."""
    slot = int(slot)
    return ("H", TB.HEAVY_POSITIONS[slot]) if slot < TB.H_LEN else ("L", TB.LIGHT_POSITIONS[slot - TB.H_LEN])


def _num(v):
    v = float(v)
    return "-inf" if v == -np.inf else "inf" if v == np.inf else repr(v)


def write_scan(path, jobs, res):
    """One CSV row per (sequence, scanned position).  float32 values are written by their shortest round-trip form, so the file parses
    back to the arrays bit for bit."""
    with open(path, "w", encoding="UTF-8") as f:
        f.write(",".join(COLUMNS) + "\n")
        for j, job in enumerate(jobs):
            for t in range(int(res["T"][j])):
                slot = int(res["slot"][j, t])
                chain, imgt = slot_label(slot)
                vals = [_f32(v) for v in res["dist"][j, t]]
                f.write(",".join([str(job.name), chain, str(imgt), str(slot), LETTERS[int(res["wt"][j, t])], _f32(res["logp_wt"][j, t]),
                                  _num(res["entropy"][j, t])] + vals) + "\n")
    return path


def _f32(v):
    v = np.float32(v)
    return "-inf" if v == -np.inf else "inf" if v == np.inf else str(v)


def main(argv=None):
    parser = build_parser()
    args = parser.parse_args(argv)
    rc = relaunch_if_asked(args, "hudiff_amd.cli.scan", argv)
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
    res = scan_jobs(model, jobs, context=args.context, device_batch=args.device_batch)
    if rank != 0 or res is None:
        return None
    out = args.out_fpath or os.path.join(os.path.dirname(os.path.abspath(args.data_fpath)), "scan_result.csv")
    return write_scan(out, jobs, res)


if __name__ == "__main__":
    _r = main()
    raise SystemExit(_r if isinstance(_r, int) else 0)      # an int is the exit code of a --gpus N relaunch
