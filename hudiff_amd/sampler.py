"""Batched driver of the device-side sampling loop for many independent sequences.

The reference humanizes one antibody at a time with ``batch_size`` replicas sharing one visiting order
(antibody_scripts/sample.py:475-538).  Here every (antibody, replica) is one independent row of a large
device batch: rows carry their own order and length, noise is keyed by the global row id, and rows are
sharded over ranks (hudiff_amd/dist.py).  Visiting orders are produced exactly as the reference does --
one ``np.random.shuffle(loc)`` per sequence in file order from the globally seeded numpy RNG
(sample.py:497-498, utils/misc.py:27-31).
"""
from __future__ import annotations

import random
from dataclasses import dataclass, field
from typing import List, Optional, Sequence

import numpy as np

from . import dist as D


def seed_all(seed: int):
    """utils/misc.py:27-31 (torch's generator is not used by this implementation)."""
    np.random.seed(seed)
    random.seed(seed)


@dataclass
class Job:
    """One sequence to humanize: masked tokens, region ids, chain ids (antibody) and its visiting order."""
    tokens: np.ndarray                   # [L], or [replicas, L] when replicas continue from different states
    region: np.ndarray
    loc: np.ndarray                      # already shuffled (or not) by the caller; the candidate list (and tie-break) under slot_policy="confident"
    chain: Optional[tuple] = None        # (heavy id, light id) for antibodies
    name: str = ""
    parent: dict = field(default_factory=dict)
    guide: Optional[object] = None       # hudiff_amd.guide.Guide of this sequence: allow [L] / bias [L, 22] (its temperature is not used)
    origin: Optional[np.ndarray] = None  # [L] tokens a mutation budget (max_mutations=) counts changes from; 22 = the slot is free; None = all free


def _stack_budget(jb, L, max_mutations):
    """The jobs' origins under one ``max_mutations`` -> hudiff_amd.guide.Budget [len(jb), L]; a job without an origin is free everywhere."""
    from .guide import Budget
    return Budget.stack([None if j.origin is None else Budget(j.origin, int(max_mutations)) for j in jb], L)


def _id_runs(gids: np.ndarray, max_rows: int):
    """Split positions 0..len(gids) into chunks of <= max_rows whose global row ids are consecutive (one device
    launch keys its rows as row0 + b)."""
    s = 0
    while s < len(gids):
        e = s + 1
        while e < len(gids) and e - s < max_rows and gids[e] == gids[e - 1] + 1:
            e += 1
        yield s, e
        s = e


def sample_jobs(model, jobs: Sequence[Job], replicas: int, seed: int, *, passes: int = 1,
                device_batch: int = 256, dropout: str = "faithful", q_noise=None, all_ranks: bool = False,
                job_ids: Optional[Sequence[int]] = None, return_logp: bool = False, temperature: float = 1.0, slots_per_step: int = 1,
                slot_policy: str = "given", return_order: bool = False, truncation=None, max_mutations: Optional[int] = None,
                confidence: Optional[float] = None, forward_stats: Optional[dict] = None, refine: Optional[dict] = None,
                return_redrawn: bool = False):
    """Sample ``replicas`` rows per job; returns int32 [len(jobs), passes, replicas, L] on rank 0 (every rank
    when single-process or ``all_ranks``).  ``passes`` > 1 re-runs the loop over the already filled tokens, which is what the
    reference's ``while sample_number > 0`` loop does (sample.py:499, nanosample.py:316).

    ``job_ids``: the id each job's noise is keyed by (default: its position in ``jobs``).  Row (job, replica) draws
    its noise as global row ``job_ids[job] * replicas + replica``, whatever else is in the batch.

    ``return_logp``: also returns float32 [len(jobs), passes, replicas, Tmax], the log-probability of the token each row drew at
    each step of each pass under the distribution it was drawn from (0 beyond a row's steps); gathered like the tokens.

    ``temperature`` and the jobs' ``guide`` fields steer the draw (hudiff_amd.guide); with no guide on any job and temperature 1 the
    calls into the library are exactly the unguided ones.

    ``slots_per_step`` = K > 1: block decoding (model.sample) -- K slots of a row's order per denoiser forward; at 1 the calls into the
    library are exactly the one-slot ones.

    ``slot_policy`` = "confident": every row's ``loc`` is its candidate list and the device picks, forward by forward, the K slots
    it is surest about (model.sample); with "given" nothing is passed on and the calls into the library are exactly today's.

    ``truncation``: a hudiff_amd.guide.Truncation (top_k, top_p, min_p) for every draw of every row (model.sample); None or a neutral
    one passes nothing on and the calls into the library are exactly today's.

    ``max_mutations``: a mutation budget (model.sample ``budget=``): every row may differ from its job's ``origin`` in at most that many
    of the slots it samples, counted anew in every pass; None passes nothing on and the calls into the library are exactly today's.

    ``confidence``: a threshold tau in (0, 1] under ``slot_policy="confident"`` (model.sample): a forward fills every remaining slot
    of a row whose top probability is at least tau -- at least one, at most ``slots_per_step``; None or 0 passes nothing on and the
    calls into the library are exactly today's.  ``forward_stats``: a dict that then receives, summed over this rank's rows with
    slots to fill, ``rows``, ``forwards`` (their total) and ``max`` (the most any row needed).

    ``refine``: ``dict(rounds=, slots=, below=0.0)``, refinement rounds (model.sample): after a row has drawn its whole ``loc``, its
    least likely slots are masked again and redrawn with everything else as context, anew in every pass; None passes nothing on and
    the calls into the library are exactly today's.  Tmax of the returned arrays is then ``guide.refine_tcap`` of the longest
    ``loc``, and the returned log-probabilities are those of the LIVE positions only (the draw that is the row's final token at its
    slot; 0 elsewhere), so a row's sum is the log-probability of what it ended with, each slot under the context it was last drawn
    in.  ``return_redrawn``: also returns (last) int32 [len(jobs), passes, replicas], the number of slots each row redrew.

    ``return_order``: also returns int32 [len(jobs), passes, replicas, Tmax], the order each row took (model.sample_order;
    under "given" the order it was handed), gathered like the log-probabilities."""
    from .guide import refine_args, refine_live, refine_tcap
    ra = refine_args(refine)
    if return_redrawn and ra is None:
        raise ValueError("return_redrawn needs refine")
    if slot_policy not in ("given", "confident"):
        raise ValueError(f"slot_policy must be 'given' or 'confident', got {slot_policy!r}")
    guided = float(temperature) != 1.0 or any(j.guide is not None for j in jobs)
    L = model.max_len
    n_rows = len(jobs) * replicas
    rank, world, _ = D.env_rank_world()
    lo, hi = D.shard_bounds(n_rows, rank, world)
    is_ab = model.kind == "ab"
    Tmax = max([len(j.loc) for j in jobs] + [1])
    if ra is not None:                                           # the positions the rounds can come to use
        Tmax = refine_tcap([len(j.loc) for j in jobs] + [1], ra[0], ra[1], int(slots_per_step))
    out = np.zeros((passes, hi - lo, L), np.int32)
    lp = np.zeros((passes, hi - lo, Tmax), np.float32) if return_logp else None
    redrawn = np.zeros((passes, hi - lo, 1), np.int32) if return_redrawn else None
    more = {"return_logp": True} if return_logp else {}
    if ra is not None:
        more["refine"] = dict(rounds=ra[0], slots=ra[1], below=ra[2])
    if int(slots_per_step) != 1:
        more["slots_per_step"] = int(slots_per_step)
    if slot_policy != "given":
        more["slot_policy"] = slot_policy
    if truncation is not None and not truncation.neutral:
        more["truncation"] = truncation
    thresh = confidence is not None and float(confidence) != 0.0
    if thresh:
        more["confidence"] = float(confidence)
    od = np.zeros((passes, hi - lo, Tmax), np.int32) if return_order else None
    jid = np.arange(len(jobs), dtype=np.int64) if job_ids is None else np.asarray(job_ids, dtype=np.int64)
    pos = np.arange(lo, hi)                                      # positions in the packed (job-major) row list
    gids = jid[pos // replicas] * replicas + pos % replicas      # the ids the noise is keyed by
    for cs, ce in _id_runs(gids, device_batch):
        ids = pos[cs:ce]
        s, e = int(ids[0]), int(ids[-1]) + 1
        jb = [jobs[i // replicas] for i in ids]
        tok = np.stack([j.tokens if np.ndim(j.tokens) == 1 else j.tokens[i % replicas]
                        for i, j in zip(ids, jb)]).astype(np.int32)
        reg = np.stack([j.region for j in jb]).astype(np.int32)
        order = np.zeros((len(jb), Tmax), np.int32)
        T = np.zeros(len(jb), np.int32)
        for r, j in enumerate(jb):
            order[r, :len(j.loc)] = j.loc
            T[r] = len(j.loc)
        chain = np.array([j.chain[0] for j in jb] + [j.chain[1] for j in jb], np.int32) if is_ab else None
        if guided:
            from .guide import Guide
            more = dict(more, guide=Guide.stack([j.guide for j in jb], L, temperature))
        if max_mutations is not None:
            more = dict(more, budget=_stack_budget(jb, L, max_mutations))
        for p in range(passes):
            tok = model.sample(tok, reg, chain, order, T, seed=seed + 1000003 * p, row0=int(gids[cs]), dropout=dropout,
                               q_noise=None if q_noise is None else np.ascontiguousarray(q_noise[p][:Tmax, gids[cs:ce]]), **more)
            if return_logp:
                tok, lp[p, s - lo:e - lo] = tok
            out[p, s - lo:e - lo] = tok
            if ra is not None and (return_logp or return_redrawn):
                T_now, _, count = model.refine_state(len(jb), ra[0])
                live = refine_live(model.sample_order(len(jb), Tmax), T_now)
                if return_logp:
                    lp[p, s - lo:e - lo] = np.where(live, lp[p, s - lo:e - lo], 0.0)
                if return_redrawn:                                   # (a redrawn slot's live position is an appended one)
                    redrawn[p, s - lo:e - lo, 0] = (live & (np.arange(Tmax)[None, :] >= T[:, None])).sum(axis=1)
            if return_order:
                od[p, s - lo:e - lo] = model.sample_order(len(jb), Tmax)
            if thresh and forward_stats is not None:
                need = model.sample_forwards(len(jb), Tmax).max(axis=1)[T > 0] + 1        # (the last forward that drew in the row)
                forward_stats["rows"] = forward_stats.get("rows", 0) + int(need.size)
                forward_stats["forwards"] = forward_stats.get("forwards", 0) + int(need.sum())
                forward_stats["max"] = max(forward_stats.get("max", 0), int(need.max()) if need.size else 0)
    gathered = [D.gather_rows(out[p], n_rows, L, all_ranks) for p in range(passes)]
    # (the float32 bits of the log-probabilities travel as int32 through the same gather)
    gathered_lp = [D.gather_rows(lp[p].view(np.int32), n_rows, Tmax, all_ranks) for p in range(passes)] if return_logp else None
    gathered_od = [D.gather_rows(od[p], n_rows, Tmax, all_ranks) for p in range(passes)] if return_order else None
    gathered_rd = [D.gather_rows(redrawn[p], n_rows, 1, all_ranks) for p in range(passes)] if return_redrawn else None
    if gathered[0] is None:
        res = (None,) + ((None,) if return_logp else ()) + ((None,) if return_order else ()) + ((None,) if return_redrawn else ())
        return res if len(res) > 1 else None
    tokens = np.stack(gathered, axis=0).reshape(passes, len(jobs), replicas, L).transpose(1, 0, 2, 3)
    res = (tokens,)
    if return_logp:
        logp = np.ascontiguousarray(np.stack(gathered_lp, axis=0), dtype=np.int32).view(np.float32)
        res += (logp.reshape(passes, len(jobs), replicas, Tmax).transpose(1, 0, 2, 3),)
    if return_order:
        res += (np.stack(gathered_od, axis=0).astype(np.int32).reshape(passes, len(jobs), replicas, Tmax).transpose(1, 0, 2, 3),)
    if return_redrawn:
        res += (np.stack(gathered_rd, axis=0).astype(np.int32).reshape(passes, len(jobs), replicas).transpose(1, 0, 2),)
    return res if len(res) > 1 else tokens


def beam_jobs(model, jobs: Sequence[Job], width: int, *, device_batch: int = 256, all_ranks: bool = False, temperature: float = 1.0,
              truncation=None, max_mutations: Optional[int] = None):
    """Beam search (model.beam_search) of width W over every job: the W most likely, pairwise different completions of each along its
    ``loc``, ranked.  A launch takes floor(device_batch / W) jobs (at least one); jobs are sharded over ranks and gathered like tokens.
    Returns, on rank 0 (every rank when single-process or ``all_ranks``; None elsewhere),
        tokens int32 [len(jobs), W, L], score float32 [len(jobs), W], logp float32 [len(jobs), W, Tmax], live bool [len(jobs), W]
    as model.beam_search returns them.  ``temperature`` and the jobs' ``guide`` fields, and ``truncation``, shape the distribution the
    beam ranks under, as in ``sample_jobs``; temperature 0 has no distribution and is an error.  A job with replica states
    (tokens [replicas, L]) is not a beam input.  ``max_mutations``: as in ``sample_jobs`` -- the W most likely completions that differ
    from the job's ``origin`` in at most that many sampled slots; it does not combine with a truncation."""
    W = int(width)
    if float(temperature) == 0.0:
        raise ValueError("beam search ranks under a distribution: temperature 0 (the greedy decode) has none")
    if any(np.ndim(j.tokens) != 1 for j in jobs):
        raise ValueError("beam search takes one state per job (tokens [L])")
    guided = float(temperature) != 1.0 or any(j.guide is not None for j in jobs)
    L = model.max_len
    rank, world, _ = D.env_rank_world()
    lo, hi = D.shard_bounds(len(jobs), rank, world)
    is_ab = model.kind == "ab"
    Tmax = max([len(j.loc) for j in jobs] + [1])
    tok = np.zeros((hi - lo, W, L), np.int32)
    score = np.full((hi - lo, W), -np.inf, np.float32)
    lp = np.zeros((hi - lo, W, Tmax), np.float32)
    per = max(1, int(device_batch) // max(W, 1))
    for s in range(lo, hi, per):
        jb = list(jobs[s:min(hi, s + per)])
        order = np.zeros((len(jb), Tmax), np.int32)
        T = np.zeros(len(jb), np.int32)
        for r, j in enumerate(jb):
            order[r, :len(j.loc)] = j.loc
            T[r] = len(j.loc)
        chain = np.array([j.chain[0] for j in jb] + [j.chain[1] for j in jb], np.int32) if is_ab else None
        more = {}
        if guided:
            from .guide import Guide
            more["guide"] = Guide.stack([j.guide for j in jb], L, temperature)
        if truncation is not None and not truncation.neutral:
            more["truncation"] = truncation
        if max_mutations is not None:
            more["budget"] = _stack_budget(jb, L, max_mutations)
        e = s - lo + len(jb)
        tok[s - lo:e], score[s - lo:e], lp[s - lo:e], _ = model.beam_search(
            np.stack([j.tokens for j in jb]).astype(np.int32), np.stack([j.region for j in jb]).astype(np.int32), chain, order, T, W, **more)
    # one row per job through the gather of the tokens (the float32 bits travel as int32)
    n = len(jobs)
    g_tok = D.gather_rows(tok.reshape(hi - lo, W * L), n, W * L, all_ranks)
    g_score = D.gather_rows(score.view(np.int32), n, W, all_ranks)
    g_lp = D.gather_rows(lp.reshape(hi - lo, W * Tmax).view(np.int32), n, W * Tmax, all_ranks)
    if g_tok is None:
        return None
    score = np.ascontiguousarray(g_score, dtype=np.int32).view(np.float32).reshape(n, W)
    logp = np.ascontiguousarray(g_lp, dtype=np.int32).view(np.float32).reshape(n, W, Tmax)
    return g_tok.reshape(n, W, L), score, logp, np.isfinite(score)


def beam_walk(rows, want: int, tries: int, accept, log=None):
    """One accept / tries walk of sample_jobs_with_retry over the rows of a beam, best first (a re-sweep would return the same rows):
    stop when nothing is wanted; an accepted row is written and counted; a rejected row is written only when ``tries == 1``;
    ``tries`` drops by one per row looked at.  Returns the rows written, in order."""
    out, left = [], want
    for row in rows:
        if left == 0:
            break
        if accept(row):
            out.append(row)
            left -= 1
        else:
            if tries == 1:
                out.append(row)
            if log is not None:
                log(row)
        tries -= 1
    return out


def noise_in_reference_order(q_flat, jobs: Sequence[Job], replicas: int) -> np.ndarray:
    """Recorded ``torch.multinomial`` noise of a REFERENCE run -> the ``q_noise`` argument of ``sample_jobs``.

    The reference draws input row by input row, step by step, one ``[batch_size, 22]`` Exp(1) tensor per step
    (sample.py:499-513, nanosample.py:316-329): ``q_flat`` is that sequence, ``[sum_j T_j, replicas, 22]`` for ONE sweep over
    every input row.  Here row (job j, replica r) is global row ``j * replicas + r`` -> ``[1, Tmax, len(jobs) * replicas, 22]``."""
    q_flat = np.asarray(q_flat, np.float32)
    Ts = [len(j.loc) for j in jobs]
    if q_flat.shape != (sum(Ts), replicas, 22):
        raise ValueError(f"recorded noise has shape {q_flat.shape}; this input needs {(sum(Ts), replicas, 22)} "
                         "(one [batch_size, 22] draw per visited slot of every input row)")
    out = np.ones((1, max(Ts + [1]), len(jobs) * replicas, 22), np.float32)
    at = 0
    for j, T in enumerate(Ts):
        out[0, :T, j * replicas:(j + 1) * replicas] = q_flat[at:at + T]
        at += T
    return out


def sample_jobs_with_retry(model, jobs: Sequence[Job], replicas: int, seed: int, *, want: int, tries: int, accept,
                           device_batch: int = 256, dropout: str = "faithful", log=None, q_noise=None,
                           logp_records: Optional[list] = None, temperature: float = 1.0, slots_per_step: int = 1,
                           slot_policy: str = "given", truncation=None, max_mutations: Optional[int] = None,
                           confidence: Optional[float] = None, forward_stats: Optional[dict] = None,
                           refine: Optional[dict] = None) -> List[List[np.ndarray]]:
    """The nanobody sampler's accept / re-sweep loop (nanobody_scripts/nanosample.py:316-353), batched.

    Per input sequence the reference keeps ``sample_number`` (rows still wanted) and ``try_num``: while both are
    positive it sweeps all ``batch_size`` replicas once more (from their current, already filled tokens), then
    walks the replicas in order: stop when nothing is wanted; an accepted row is written and counted; a rejected
    row is written only when ``try_num == 1``; ``try_num`` drops by one per row looked at.  Here every sweep runs
    all still-active sequences as one device batch; the decisions are taken on every rank from all-gathered
    tokens.  Returns, per job, the rows written, in order.

    ``logp_records``: a list that receives one ``(job index, sweep, replica, T, logp, chosen)`` per sampled row -- logp = the
    row's total log-probability under the distributions this sweep drew from (a re-sweep's value is that sweep's draws given the
    already filled tokens), chosen = the row was written.

    ``slot_policy``: as in ``sample_jobs`` (every sweep starts from the job's ``loc`` as the candidate list).

    ``truncation``: as in ``sample_jobs``, for every sweep.

    ``max_mutations``: as in ``sample_jobs``; every sweep redraws every sampled slot and counts from 0, so every row written differs from
    its job's ``origin`` in at most that many of them.

    ``confidence``, ``forward_stats``: as in ``sample_jobs``, for every sweep.

    ``refine``: as in ``sample_jobs``, for every sweep; a record of ``logp_records`` then has a seventh field, the number of slots the
    row redrew, and its logp is that of the live positions."""
    from .guide import refine_args
    refined = refine_args(refine) is not None
    state = [{"left": want, "tries": tries, "tokens": None, "out": []} for _ in jobs]
    active = [j for j in range(len(jobs)) if want > 0 and tries > 0]
    sweep = 0
    while active:
        sub = [Job(tokens=jobs[j].tokens if state[j]["tokens"] is None else state[j]["tokens"], region=jobs[j].region,
                   loc=jobs[j].loc, chain=jobs[j].chain, name=jobs[j].name, guide=jobs[j].guide, origin=jobs[j].origin) for j in active]
        # noise is keyed by the ORIGINAL job index: a sequence's samples do not depend on which other inputs were
        # accepted earlier (or are in the file at all)
        # (q_noise: injected noise of sweep 0 only, [1, Tmax, len(jobs) * replicas, 22] keyed like the generated noise: parity runs)
        more = {} if logp_records is None else {"return_logp": True}
        if float(temperature) != 1.0:
            more["temperature"] = temperature
        if int(slots_per_step) != 1:
            more["slots_per_step"] = int(slots_per_step)
        if slot_policy != "given":
            more["slot_policy"] = slot_policy
        if truncation is not None and not truncation.neutral:
            more["truncation"] = truncation
        if max_mutations is not None:
            more["max_mutations"] = max_mutations
        if confidence is not None and float(confidence) != 0.0:
            more["confidence"] = confidence
            more["forward_stats"] = forward_stats
        if refined:
            more["refine"] = refine
            more["return_redrawn"] = logp_records is not None
        res = sample_jobs(model, sub, replicas, seed + 1000003 * sweep, device_batch=device_batch, dropout=dropout,
                          all_ranks=True, job_ids=active, q_noise=q_noise if sweep == 0 else None, **more)
        if logp_records is not None:
            res_rd = res[2] if refined else None
            res, res_lp = res[0], res[1]
        still = []
        for a, j in enumerate(active):
            st = state[j]
            st["tokens"] = res[a, 0]
            chosen = set()
            for r, row in enumerate(res[a, 0]):
                if st["left"] == 0:
                    break
                ok = bool(accept(row))
                if ok:
                    st["out"].append(row)
                    st["left"] -= 1
                    chosen.add(r)
                else:
                    if st["tries"] == 1:
                        st["out"].append(row)
                        chosen.add(r)
                    if log is not None:
                        log(jobs[j], row)
                st["tries"] -= 1
            if logp_records is not None:
                for r in range(res.shape[2]):
                    logp_records.append((j, sweep, r, len(jobs[j].loc), float(res_lp[a, 0, r].astype(np.float64).sum()), int(r in chosen))
                                        + ((int(res_rd[a, 0, r]),) if refined else ()))
            if st["left"] > 0 and st["tries"] > 0:
                still.append(j)
        active = still
        sweep += 1
    return [st["out"] for st in state]
