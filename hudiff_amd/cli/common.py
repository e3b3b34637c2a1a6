"""Pieces shared by the two drop-in samplers: log-dir naming, logger, numbered-input readers, FASTA."""
from __future__ import annotations

import json
import logging
import os
import time


def get_new_log_dir(root="./logs", prefix="", tag=""):
    """utils/misc.py:10-24 -- {prefix}_{YYYY_mm_dd__HH_MM_SS}[_{tag}] under root."""
    fn = time.strftime("%Y_%m_%d__%H_%M_%S", time.localtime())
    if prefix != "":
        fn = prefix + "_" + fn
    if tag != "":
        fn = fn + "_" + tag
    log_dir = os.path.join(root, fn)
    os.makedirs(log_dir, exist_ok=True)
    return log_dir


def get_logger(name, log_dir=None):
    """utils/misc.py:34-53 -- same format string, stream + log.txt handlers."""
    logger = logging.getLogger(name)
    logger.setLevel(logging.DEBUG)
    logger.handlers.clear()
    fmt = logging.Formatter("[%(asctime)s::%(name)s::%(levelname)s] %(message)s")
    sh = logging.StreamHandler()
    sh.setLevel(logging.DEBUG)
    sh.setFormatter(fmt)
    logger.addHandler(sh)
    if log_dir is not None:
        fh = logging.FileHandler(os.path.join(log_dir, "log.txt"))
        fh.setLevel(logging.DEBUG)
        fh.setFormatter(fmt)
        logger.addHandler(fh)
    return logger


def add_runtime_args(p):
    """Flags every drop-in CLI adds beside the reference's own: the precision route of the device library and a self-launching
    multi-GPU mode (rows shard across GPUs, one RCCL gather)."""
    p.add_argument("--precision", choices=["default", "split", "f32_gemm", "f32_all"], default="default",
                   help="precision route of libhudiff_hip (include/hudiff_hip.h): default = split (fp32 products as three fp16 MFMAs "
                        "on (hi, lo) operand splits, fp32 accumulation; logits within 1e-4, the reference's traces bit for bit), "
                        "f32_gemm = fp32 MFMA GEMMs + split attention core, f32_all = every product on the fp32 MFMA pipe")
    p.add_argument("--gpus", type=int, default=None,
                   help="N > 1 without a launcher: start N ranks of this command under torch.distributed.run (one process per GPU, "
                        "127.0.0.1 rendezvous); under torchrun it must equal WORLD_SIZE")
    return p


def add_guide_args(p):
    """Flags of the four samplers that steer the draw (hudiff_amd/guide.py); with none of them given the run is the unguided one."""
    p.add_argument("--temperature", type=float, default=1.0,
                   help="temperature of the draw: logits are divided by it; 0 = the greedy decode (no noise)")
    p.add_argument("--forbid", type=str, default="",
                   help="residue letters (of ACDEFGHIKLMNPQRSTVWYX) never drawn at any sampled slot, e.g. CM")
    p.add_argument("--constraints_fpath", type=str, default=None,
                   help="text file, one 'chain,position,residues' per line: chain H|L, position an IMGT label or *, residues tokenizer "
                        "letters ('-' included; a leading ! = all but these); lines intersect, # starts a comment")
    p.add_argument("--bias_fpath", type=str, default=None,
                   help=".npz whose array 'bias' [max_len, 22] is added to the logits of every input")
    return p


def add_truncation_args(p):
    """--top_k / --top_p / --min_p of the four samplers and the scorer (truncated sampling, hudiff_amd/guide.py Truncation); with none
    of them given the run is the untruncated one."""
    p.add_argument("--top_k", type=int, default=0,
                   help="draw only among the k most probable residues of a slot; 0 (default) or 22 = off")
    p.add_argument("--top_p", type=float, default=1.0,
                   help="nucleus sampling: draw only among the smallest set of most probable residues whose probability reaches "
                        "top_p, in (0, 1]; 1 (default) = off")
    p.add_argument("--min_p", type=float, default=0.0,
                   help="draw only among residues at least min_p times as probable as the most probable one, in [0, 1]; 0 (default) = off")
    return p


def apply_truncation_args(args, logger=None):
    """-> {"truncation": Truncation} for sample_jobs[_with_retry] / score_jobs, or {} when the flags cut nothing (the calls are then
    exactly the untruncated ones).  A value outside its range is a ValueError."""
    from ..guide import Truncation
    tr = Truncation(getattr(args, "top_k", 0), getattr(args, "top_p", 1.0), getattr(args, "min_p", 0.0))
    if tr.neutral:
        return {}
    if logger is not None:
        logger.info("Truncation: top_k {}, top_p {}, min_p {}".format(tr.top_k, tr.top_p, tr.min_p))
    return {"truncation": tr}


def slots_per_step_arg(v):
    k = int(v)
    if not 1 <= k <= 64:
        import argparse
        raise argparse.ArgumentTypeError(f"{v}: an integer in [1, 64]")
    return k


def add_block_args(p):
    """--slots_per_step and --slot_policy of the four samplers and the scorer (block decoding, include/hudiff_hip.h); without them, or
    with 1, the run is the one-slot one.  The truncation flags (add_truncation_args) ride along: the same five commands take them."""
    p.add_argument("--slots_per_step", type=slots_per_step_arg, default=1,
                   help="block decoding: K in [1, 64] slots of a row's visiting order are drawn per denoiser forward, independently "
                        "from that forward's conditionals -- ceil(T / K) forwards per row instead of T; 1 = one slot per forward")
    p.add_argument("--slot_policy", choices=("given", "confident"), default="given",
                   help="which slots a forward fills: 'given' follows each row's visiting order; 'confident' lets the device pick, in "
                        "every forward, the --slots_per_step remaining slots whose distribution is most peaked (the order is then only "
                        "the list of slots to fill, and the tie-break)")
    p.add_argument("--confidence", type=confidence_arg, default=None, metavar="TAU",
                   help="confidence threshold in (0, 1], with --slot_policy confident: every forward fills, per row, all remaining "
                        "slots whose top probability is at least TAU -- at least one, at most --slots_per_step -- so the number of "
                        "forwards follows the model's certainty")
    return add_truncation_args(p)


def confidence_arg(v):
    import argparse
    try:
        t = float(v)
    except ValueError:
        raise argparse.ArgumentTypeError(f"{v}: a number in (0, 1]") from None
    if not (t > 0.0 and t <= 1.0):                   # (NaN fails both)
        raise argparse.ArgumentTypeError(f"{v}: a number in (0, 1]")
    return t


def check_confidence_args(p, args):
    """The combinations --confidence does not take are argparse errors."""
    if getattr(args, "confidence", None) is None:
        return args
    if args.slot_policy != "confident":
        p.error("--confidence compares the confident policy's keys: it needs --slot_policy confident")
    if getattr(args, "beam", 0):
        p.error("--confidence is a sampling option: not together with --beam")
    if getattr(args, "max_mutations", None) is not None:
        p.error("--confidence may fill several slots per forward: not together with --max_mutations")
    return args


def log_forward_stats(stats, logger):
    """What a --confidence run needed: mean and maximum forwards per row (this rank's rows)."""
    if logger is not None and stats and stats.get("rows"):
        logger.info("Forwards per row: mean {:.2f}, max {} ({} rows)".format(stats["forwards"] / stats["rows"], stats["max"], stats["rows"]))


def apply_block_args(args, jobs, logger=None, forward_stats=None):
    """-> the keywords for sample_jobs[_with_retry] / score_jobs: {} at K = 1 in the given order (the calls are then exactly the
    one-slot ones); with truncation flags, plus what apply_truncation_args returns.  ``forward_stats`` (samplers only): the dict a
    --confidence run counts its forwards into (log_forward_stats)."""
    k = int(args.slots_per_step)
    more = apply_truncation_args(args, logger)
    more.update(apply_refine_args(args, logger))
    if getattr(args, "slot_policy", "given") != "given":
        more["slot_policy"] = args.slot_policy
        if logger is not None:
            logger.info("Slot policy: {}".format(args.slot_policy))
    if getattr(args, "confidence", None) is not None:
        more["confidence"] = float(args.confidence)
        if forward_stats is not None:
            more["forward_stats"] = forward_stats
        if logger is not None:
            logger.info("Confidence threshold: {} (at most {} slots per forward)".format(args.confidence, k))
        if k != 1:
            more["slots_per_step"] = k
        return more
    if k == 1:
        return more
    if logger is not None:
        steps = sorted({len(j.loc) for j in jobs})
        logger.info("Slots per step: {}; forwards per row: {}".format(
            k, ", ".join("{} (T = {})".format(-(-t // k), t) for t in steps[:8]) + (" ..." if len(steps) > 8 else "")))
    more["slots_per_step"] = k
    return more


def beam_arg(v):
    w = int(v)
    if not 1 <= w <= 64:
        import argparse
        raise argparse.ArgumentTypeError(f"{v}: an integer in [1, 64]")
    return w


def add_beam_args(p):
    """--beam of the four samplers (beam search, include/hudiff_hip.h); without it the run is the sampling one."""
    p.add_argument("--beam", type=beam_arg, default=0,
                   help="beam search instead of sampling: W in [1, 64]; every input gets its W most likely, pairwise different "
                        "humanizations under the guide and truncation flags, best first, where the replicas of a sampling run stand "
                        "(--batch_size and --sample_number are not used; dropout is off; --logp_fpath records the scores)")
    return p


def max_mutations_arg(v):
    n = int(v)
    if n < 0:
        import argparse
        raise argparse.ArgumentTypeError(f"{v}: an integer >= 0")
    return n


def refine_rounds_arg(v):
    n = int(v)
    if not 0 <= n <= 16:
        import argparse
        raise argparse.ArgumentTypeError(f"{v}: an integer in [0, 16]")
    return n


def refine_slots_arg(v):
    n = int(v)
    if not 1 <= n <= 64:
        import argparse
        raise argparse.ArgumentTypeError(f"{v}: an integer in [1, 64]")
    return n


def refine_below_arg(v):
    import argparse
    try:
        x = float(v)
    except ValueError:
        raise argparse.ArgumentTypeError(f"{v}: a finite number <= 0") from None
    if not (x <= 0.0 and x > float("-inf")):          # (NaN fails both)
        raise argparse.ArgumentTypeError(f"{v}: a finite number <= 0")
    return x


def add_refine_args(p):
    """--refine_rounds / --refine_slots / --refine_below of the four samplers (refinement rounds, include/hudiff_hip.h); without
    --refine_rounds the run is today's."""
    p.add_argument("--refine_rounds", type=refine_rounds_arg, default=0,
                   help="refinement rounds: after a row has drawn all its positions, its least likely ones are masked again and redrawn "
                        "with everything else as context, this many times, in [0, 16]; 0 (default) = none")
    p.add_argument("--refine_slots", type=refine_slots_arg, default=None, metavar="R",
                   help="positions redrawn per round, in [1, 64] (default 8); needs --refine_rounds")
    p.add_argument("--refine_below", type=refine_below_arg, default=None, metavar="LOGP",
                   help="only positions whose recorded log-probability is below LOGP (finite, <= 0; default 0: every position drawn "
                        "with probability < 1) are redrawn; needs --refine_rounds")
    return p


def apply_refine_args(args, logger=None):
    """-> {"refine": dict(rounds=, slots=, below=)} for sample_jobs[_with_retry], or {} without --refine_rounds (the calls are then
    exactly today's)."""
    n = int(getattr(args, "refine_rounds", 0) or 0)
    if n == 0:
        return {}
    slots = getattr(args, "refine_slots", None)
    below = getattr(args, "refine_below", None)
    refine = dict(rounds=n, slots=8 if slots is None else int(slots), below=0.0 if below is None else float(below))
    if logger is not None:
        logger.info("Refinement: {rounds} round(s) of {slots} slot(s), log-probability below {below}".format(**refine))
    return {"refine": refine}


def add_budget_args(p):
    """--max_mutations of the four samplers (mutation budget, include/hudiff_hip.h); without it the run is today's.  The refinement
    flags (add_refine_args) ride along: the same four commands take them."""
    add_refine_args(p)
    p.add_argument("--max_mutations", type=max_mutations_arg, default=None,
                   help="mutation budget: every written sequence differs from its input in at most N of the sampled positions -- a row "
                        "that has changed N of them keeps the input's residue from then on; composes with --beam (the W most likely "
                        "humanizations with at most N mutations), the guide flags, --slot_policy confident and --temperature 0")
    return p


def apply_budget_args(args, jobs, logger=None):
    """-> {"max_mutations": N} for sample_jobs[_with_retry] / beam_jobs, or {} without the flag (the calls are then exactly today's).
    The origin a job's changes are counted from is its ``origin`` field: the input's own residue at every sampled slot."""
    n = getattr(args, "max_mutations", None)
    if n is None:
        return {}
    missing = [j.name for j in jobs if j.origin is None]
    if missing:
        raise ValueError(f"--max_mutations: input {missing[0]!r} carries no origin tokens")
    if logger is not None:
        logger.info("Mutation budget: at most {} of the sampled positions change".format(n))
    return {"max_mutations": int(n)}


def parse_with_beam(p, argv):
    """parse_args, and the combinations --beam and --max_mutations do not take are argparse errors."""
    args = check_confidence_args(p, p.parse_args(argv))
    if not getattr(args, "refine_rounds", 0):
        if getattr(args, "refine_slots", None) is not None or getattr(args, "refine_below", None) is not None:
            p.error("--refine_slots / --refine_below describe refinement rounds: they need --refine_rounds")
    else:
        if args.beam:
            p.error("--refine_rounds redraws sampled positions: not together with --beam")
        if getattr(args, "confidence", None) is not None:
            p.error("--refine_rounds opens its rounds by the step: not together with --confidence")
        if getattr(args, "max_mutations", None) is not None:
            p.error("--refine_rounds would count a redrawn position twice: not together with --max_mutations")
    if getattr(args, "max_mutations", None) is not None:
        if int(args.slots_per_step) > 1:
            p.error("--max_mutations counts one slot per forward: not together with --slots_per_step > 1")
        if args.beam and not (args.top_k in (0, 22) and args.top_p >= 1.0 and args.min_p == 0.0):
            p.error("--max_mutations with --beam takes no truncation (--top_k / --top_p / --min_p): the cut may remove the only "
                    "residue the budget still allows")
    if args.beam:
        if int(args.slots_per_step) > 1:
            p.error("--beam searches one slot per forward: not together with --slots_per_step > 1")
        if args.slot_policy != "given":
            p.error("--beam follows the given order: not together with --slot_policy confident")
        if float(args.temperature) == 0.0:
            p.error("--beam ranks under a distribution: not together with --temperature 0 (the greedy decode)")
        if getattr(args, "q_noise_fpath", None):
            p.error("--beam reads no noise: not together with --q_noise_fpath")
    return args


def run_beam(model, jobs, args, kind, logger=None):
    """The --beam run of a sampler: the guide and truncation flags applied, then sampler.beam_jobs.  -> (tokens [J, W, L], score [J, W],
    live [J, W]) on rank 0, None elsewhere."""
    from ..sampler import beam_jobs
    temperature = apply_guide_args(args, kind, jobs, logger)
    if logger is not None:
        logger.info("Beam search: width {} (dropout off, no noise)".format(args.beam))
    res = beam_jobs(model, jobs, args.beam, device_batch=getattr(args, "device_batch", 256), temperature=temperature,
                    **apply_truncation_args(args, logger), **apply_budget_args(args, jobs, logger))
    if res is None:
        return None
    tokens, score, _, live = res
    return tokens, score, live


def apply_guide_args(args, kind, jobs, logger=None):
    """Gives every job the guide the flags of add_guide_args describe and returns the temperature for sample_jobs[_with_retry].  No
    flag given: the jobs stay unguided.  A constraint of --constraints_fpath on a slot an input does not sample is ignored (their
    number is logged once); a sampled slot left without an allowed residue is an error."""
    import numpy as np
    from ..guide import ALL_TOKENS, Guide, LETTERS, N_DRAW, letters_mask, parse_constraints
    temperature = float(args.temperature)
    if not (temperature == 0.0 or 0.01 <= temperature <= 100.0):
        raise ValueError(f"--temperature {args.temperature}: 0 (greedy) or a value in [0.01, 100]")
    if not (args.forbid or args.constraints_fpath or args.bias_fpath) or not jobs:
        return temperature
    if "-" in args.forbid:
        raise ValueError("--forbid: '-' (the gap) cannot be forbidden this way; use --constraints_fpath")
    forbid = letters_mask(args.forbid)
    L = len(jobs[0].tokens) if np.ndim(jobs[0].tokens) == 1 else np.shape(jobs[0].tokens)[-1]
    allow = np.full(L, ALL_TOKENS, np.uint32)
    if args.constraints_fpath:
        with open(args.constraints_fpath) as f:
            allow = parse_constraints(f, kind)
        if allow.shape != (L,):
            raise ValueError(f"{args.constraints_fpath}: constraints describe {allow.shape[0]} slots, the inputs have {L}")
    constrained = allow != ALL_TOKENS
    allow = allow & np.uint32(ALL_TOKENS & ~forbid)
    bias = None
    if args.bias_fpath:
        bias = np.asarray(np.load(args.bias_fpath)["bias"], np.float32)
        if bias.shape != (L, N_DRAW):
            raise ValueError(f"{args.bias_fpath}: bias must be [{L}, {N_DRAW}], got {bias.shape}")
        if not np.isfinite(bias).all():
            raise ValueError(f"{args.bias_fpath}: bias must be finite (forbid a residue with --forbid / --constraints_fpath)")
    ignored = 0
    for job in jobs:
        loc = np.asarray(job.loc, np.int64)
        empty = loc[allow[loc] == 0]
        if len(empty):
            raise ValueError(f"input {job.name!r}: no residue of {LETTERS} is left at sampled slot {int(empty[0])} "
                             "(--forbid and --constraints_fpath together exclude everything)")
        sampled = np.zeros(L, bool)
        sampled[loc] = True
        ignored += int((constrained & ~sampled).sum())
        job.guide = Guide(allow, bias)
    if logger is not None and args.constraints_fpath:
        logger.info("Constraints on slots an input does not sample (ignored): {}".format(ignored))
    return temperature


def relaunch_if_asked(args, module, argv):
    """`python -m hudiff_amd.cli.X --gpus N` without a launcher around it: re-execute as N ranks under torch.distributed.run (the
    same shape bench.py uses) and return that job's exit code; None when this process should carry on (single rank, or already a
    rank of a launched job).  A mismatch between --gpus and the world size a launcher formed is an error, never a silent run."""
    import subprocess
    import sys
    if not args.gpus or args.gpus < 1:
        return None
    world = os.environ.get("WORLD_SIZE")
    if world is not None:
        if int(world) != args.gpus:
            raise SystemExit(f"{module}: --gpus {args.gpus} but the launcher started WORLD_SIZE={world} ranks")
        return None
    if args.gpus == 1:
        return None
    cmd = relaunch_command(module, args.gpus, list(sys.argv[1:] if argv is None else argv))
    return subprocess.call(cmd, env=dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0"))


def relaunch_command(module, gpus, argv):
    import socket
    import sys
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    return [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={gpus}", "--master-addr", "127.0.0.1",
            "--master-port", str(port), "-m", module] + argv


def str2bool_like_reference(v):
    """argparse ``type=bool`` of the reference: any non-empty string is True (sample.py:402, 411-414)."""
    return bool(v)


def load_numbered(path):
    """Pre-numbered sequences for machines without ANARCI: JSON lines, one object per input row, e.g.
    {"name": "ab1", "h": {"1": "E", "2": "V", ..., "111A": "G"}, "l": {...}, "l_chain": "K"}   (antibody)
    {"h": {...}}                                                                               (nanobody)
    keys are IMGT position strings as ``get_pad_seq`` builds them (sample.py:84-88)."""
    rows = []
    with open(path) as f:
        for line in f:
            line = line.strip()
            if line:
                rows.append(json.loads(line))
    return rows


def write_logp_csv(path, rows, sweep=False, redrawn=False):
    """Sidecar of a sampling run (``--logp_fpath``): one line per SAMPLED row, 'name,pass,replica,T,logp,chosen' (with ``sweep``:
    'name,sweep,pass,replica,T,logp,chosen').  T = slots the row sampled, logp = their total log-probability under the distributions
    they were drawn from, chosen = 1 when the row was written to sample_humanization_result.csv.  ``redrawn`` (a run with
    --refine_rounds): a last column 'redrawn', the number of positions the row redrew; logp is then the total over the LIVE positions
    -- every position under the distribution its final residue was drawn from."""
    width = (7 if sweep else 6) + (1 if redrawn else 0)
    with open(path, "w", encoding="UTF-8") as f:
        f.write(("name,sweep,pass,replica,T,logp,chosen" if sweep else "name,pass,replica,T,logp,chosen") + (",redrawn\n" if redrawn else "\n"))
        for row in rows:
            if len(row) != width:
                raise ValueError(f"a row of the log-probability sidecar has {width} fields, got {row!r}")
            *head, T, logp, chosen = row[:-1] if redrawn else row
            f.write(",".join(str(x) for x in head) + f",{int(T)},{float(logp):.6f},{int(chosen)}" + (f",{int(row[-1])}\n" if redrawn else "\n"))
    return path


def write_fasta_2line(records, path):
    """[(id, description, sequence)] -> '>id description\\nSEQ' (the 'fasta-2line' flavour)."""
    with open(path, "w") as f:
        for rid, desc, seq in records:
            f.write(f">{rid} {desc}\n{seq}\n" if desc else f">{rid}\n{seq}\n")


def write_fasta_wrapped(records, path, width=60):
    """Bio.SeqIO 'fasta' flavour: header '>id description', sequence wrapped at 60 columns."""
    with open(path, "w") as f:
        for rid, desc, seq in records:
            f.write(f">{rid} {desc}\n")
            for i in range(0, len(seq), width):
                f.write(seq[i:i + width] + "\n")


def read_fasta(path):
    """-> [(description line without '>', sequence)], multi-line records joined (stand-in for Bio.SeqIO.parse)."""
    records, desc, chunks = [], None, []
    with open(path) as f:
        for line in f:
            line = line.strip()
            if not line:
                continue
            if line.startswith(">"):
                if desc is not None:
                    records.append((desc, "".join(chunks)))
                desc, chunks = line[1:], []
            elif desc is not None:
                chunks.append(line)
    if desc is not None:
        records.append((desc, "".join(chunks)))
    return records


def split_fasta_for_save(csv_path, human_seqs):
    """One '{idx}_human.fasta' per humanized sample under sample_human_fa/ next to the CSV, plus the empty
    sample_human_pdb/ the structure predictor fills.  Nanobody (nanosample.py:163-182): record '{idx}_human_H', wrapped;
    antibody (sample.py:326-349, items are (VH, VL) pairs): '>{idx}_human_H VH' and '>{idx}_human_L VL', two-line records
    as ``Chain.to_fasta`` writes them."""
    base = os.path.dirname(csv_path)
    fa_dir, pdb_dir = os.path.join(base, "sample_human_fa"), os.path.join(base, "sample_human_pdb")
    os.makedirs(fa_dir, exist_ok=True)
    os.makedirs(pdb_dir, exist_ok=True)
    for idx, seq in enumerate(human_seqs):
        path = os.path.join(fa_dir, f"{idx}_human.fasta")
        if isinstance(seq, str):
            write_fasta_wrapped([(f"{idx}_human_H", "<unknown description>", seq)], path)
        else:
            write_fasta_2line([(f"{idx}_human_H", "VH", seq[0]), (f"{idx}_human_L", "VL", seq[1])], path)
    return fa_dir
