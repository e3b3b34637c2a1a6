"""Likelihood of given sequences under the denoiser (host side; the device side is hd_score, include/hudiff_hip.h).

The network is an order-agnostic autoregressive model: for a visiting order sigma of the scored slots,
``sum_t log p(x_sigma(t) | x_sigma(<t), everything outside the scored slots)`` is a one-order estimate of the log-likelihood of
those slots, and the training objective is its mean over orders.  The tokens are given, so step t of a row does not depend on
step t - 1: the T steps of one sequence are T independent forwards (``expand_steps``) that fill one device batch instead of T
latency-bound launches of a single row.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Optional, Sequence

import numpy as np

from . import dist as D

MASK_TOKEN = 22


@dataclass
class Expanded:
    """Rows of ``expand_steps``: row i is (source row ``rows[i]``, step ``steps[i]``).  With ``slots_per_step`` = K > 1 row i is the
    group of K order positions of its source row that starts at ``steps[i]`` (a multiple of K)."""
    tokens: np.ndarray                   # [N, L] int32
    region: np.ndarray                   # [N, L] int32
    chain: Optional[np.ndarray]          # [2N] int32 (heavy ids, then light ids) or None
    order: np.ndarray                    # [N, K] int32: the slot(s) the row scores (0 beyond T)
    T: np.ndarray                        # [N] int32: slots the row scores (all 1 at K = 1; < K in a row's last group)
    rows: np.ndarray                     # [N] source row b
    steps: np.ndarray                    # [N] (first) step t of the source row
    B: int                               # source rows
    slots_per_step: int = 1              # K

    def fold(self, flat, Tmax: int) -> np.ndarray:
        """Per-row values [N] ([N, K] with K slots per step) -> [B, Tmax] float32, 0 where t >= T[b]: the value of row i at
        position j < T[i] goes to ``[rows[i], steps[i] + j]``."""
        out = np.zeros((self.B, Tmax), np.float32)
        if self.slots_per_step == 1:
            out[self.rows, self.steps] = np.asarray(flat, np.float32).reshape(-1)
            return out
        N, K = self.rows.shape[0], self.slots_per_step
        flat = np.asarray(flat, np.float32).reshape(N, K)
        j = np.arange(K)[None, :]
        live = j < np.asarray(self.T)[:, None]
        out[np.broadcast_to(self.rows[:, None], (N, K))[live], (self.steps[:, None] + j)[live]] = flat[live]
        return out

    def fold_dist(self, flat, Tmax: int) -> np.ndarray:
        """The distribution records of the rows, [N, K, 22] (a session's ``sample_dist``), -> [B, Tmax, 22] float32, 0 where
        t >= T[b]: as ``fold``, 22 values per position."""
        N, K = self.rows.shape[0], self.slots_per_step
        flat = np.asarray(flat, np.float32).reshape(N, K, 22)
        out = np.zeros((self.B, Tmax, 22), np.float32)
        j = np.arange(K)[None, :]
        live = j < np.asarray(self.T)[:, None]
        out[np.broadcast_to(self.rows[:, None], (N, K))[live], (self.steps[:, None] + j)[live]] = flat[live]
        return out


def expand_steps(tokens, region, chain, order, T, slots_per_step: int = 1) -> Expanded:
    """Every (b, t < T[b]) becomes one row: the complete tokens of row b with ``order[b, t:T[b]]`` masked, row b's region and
    chain ids, order ``[order[b, t]]`` and T = 1.  Rows are b-major, t ascending.

    ``slots_per_step`` = K > 1 (block decoding): every (b, f) with f * K < T[b] becomes one row -- ``order[b, f*K:T[b]]`` masked,
    order = the group ``order[b, f*K : min(f*K + K, T[b])]`` (0-padded to K), T = its length -- to be scored in sessions of block
    size K with Tmax = K."""
    K = int(slots_per_step)
    if not 1 <= K <= 64:
        raise ValueError(f"slots_per_step must be in [1, 64], got {slots_per_step}")
    if K > 1:
        return _expand_groups(tokens, region, chain, order, T, K)
    tokens = np.asarray(tokens, np.int32)
    region = np.asarray(region, np.int32)
    T = np.asarray(T, np.int64).reshape(-1)
    B, L = tokens.shape
    order = np.asarray(order, np.int32)
    # not reshape(B, -1): an empty batch (B = 0) leaves -1 undetermined
    order = order.reshape(B, order.shape[1] if order.ndim == 2 else (order.size // B if B else 0))
    if T.shape[0] != B or (T < 0).any() or (T > order.shape[1]).any():
        raise ValueError(f"T must be [{B}] with 0 <= T[b] <= {order.shape[1]}")
    rows = np.repeat(np.arange(B), T)
    steps = np.concatenate([np.arange(t) for t in T] + [np.zeros(0, np.int64)]).astype(np.int64)
    N = rows.shape[0]
    tok = tokens[rows].copy()
    slot = order[rows, steps] if N else np.zeros(0, np.int32)
    # row (b, t) masks order[b, u] for t <= u < T[b]
    at = 0
    for b in range(B):
        n = int(T[b])
        for t in range(n):
            tok[at + t, order[b, t:n]] = MASK_TOKEN
        at += n
    ch = None
    if chain is not None:
        chain = np.asarray(chain, np.int32).reshape(-1)
        if chain.shape[0] != 2 * B:
            raise ValueError(f"chain must be [{2 * B}] (heavy ids, then light ids)")
        ch = np.concatenate([chain[:B][rows], chain[B:][rows]]).astype(np.int32)
    return Expanded(tokens=tok, region=region[rows].copy(), chain=ch, order=slot.reshape(N, 1).astype(np.int32),
                    T=np.ones(N, np.int32), rows=rows, steps=steps, B=B)


def _expand_groups(tokens, region, chain, order, T, K: int) -> Expanded:
    tokens = np.asarray(tokens, np.int32)
    region = np.asarray(region, np.int32)
    T = np.asarray(T, np.int64).reshape(-1)
    B, L = tokens.shape
    order = np.asarray(order, np.int32)
    order = order.reshape(B, order.shape[1] if order.ndim == 2 else (order.size // B if B else 0))
    if T.shape[0] != B or (T < 0).any() or (T > order.shape[1]).any():
        raise ValueError(f"T must be [{B}] with 0 <= T[b] <= {order.shape[1]}")
    groups = (T + K - 1) // K
    rows = np.repeat(np.arange(B), groups)
    steps = np.concatenate([np.arange(0, t, K) for t in T] + [np.zeros(0, np.int64)]).astype(np.int64)
    N = rows.shape[0]
    tok = tokens[rows].copy()
    grp = np.zeros((N, K), np.int32)
    Tg = np.zeros(N, np.int32)
    for i in range(N):
        b, t0, n = int(rows[i]), int(steps[i]), int(T[rows[i]])
        tok[i, order[b, t0:n]] = MASK_TOKEN
        Tg[i] = min(K, n - t0)
        grp[i, :Tg[i]] = order[b, t0:t0 + Tg[i]]
    ch = None
    if chain is not None:
        chain = np.asarray(chain, np.int32).reshape(-1)
        if chain.shape[0] != 2 * B:
            raise ValueError(f"chain must be [{2 * B}] (heavy ids, then light ids)")
        ch = np.concatenate([chain[:B][rows], chain[B:][rows]]).astype(np.int32)
    return Expanded(tokens=tok, region=region[rows].copy(), chain=ch, order=grp, T=Tg, rows=rows, steps=steps, B=B, slots_per_step=K)


def draw_orders(loc, orders: int, seed: int, job_id: int) -> np.ndarray:
    """``orders`` visiting orders of the slots ``loc`` -> [orders, len(loc)]; a function of (seed, job_id, k) alone, so the orders
    of a job do not depend on what else is scored or on how rows are sharded."""
    loc = np.asarray(loc, np.int32)
    out = np.empty((orders, len(loc)), np.int32)
    for k in range(orders):
        out[k] = np.random.default_rng([int(seed), int(job_id), k]).permutation(loc)
    return out


def score_jobs(model, jobs: Sequence, orders: int = 1, seed: int = 0, *, dropout: str = "off", parallel=None,
               device_batch: int = 256, all_ranks: bool = False, job_ids: Optional[Sequence[int]] = None, slots_per_step: int = 1,
               slot_policy: str = "given", truncation=None, confidence: Optional[float] = None):
    """Score every job along ``orders`` random visiting orders of its ``loc``.

    ``truncation``: a hudiff_amd.guide.Truncation -- the scores are under the truncated sampler (model.score); a token its step's cut
    removes scores -inf, and so do the sums it enters.  None or a neutral one passes nothing on.

    ``slot_policy`` = "confident" scores under the confident sampler (model.score): the order is the model's own, found teacher-forced
    from the candidate list ``loc`` as it stands (only ties ever see the list), so ``orders`` must be 1, the sequential loop runs
    (``parallel=True`` is a ValueError) and ``order`` in the result is the order taken.  With "given" nothing is passed on.

    ``confidence``: a threshold tau in (0, 1] under ``slot_policy="confident"``: the scores are under the threshold sampler
    (model.score), ``slots_per_step`` being its cap; None or 0 passes nothing on.

    ``slots_per_step`` = K > 1 scores under the block sampler (model.score); at 1 the calls into the library are the one-slot ones.

    ``Job.tokens`` are COMPLETE sequences here (sampler.Job; ``loc`` = the slots to score, ``region`` / ``chain`` as for sampling).
    Row (job j, order k) is global row ``job_ids[j] * orders + k`` (dropout masks are keyed by it); rows shard over ranks and are
    gathered once.  Returns on rank 0 (every rank when single-process or ``all_ranks``; None elsewhere) a dict:
      total [J, orders] float64   sum_t logp of each order        T [J]                scored slots
      mean, std [J]               over the orders (std 0 for one)  per_residue [J]      mean / T (0 when T = 0)
      logp [J, orders, Tmax] float32 per step, order [J, orders, Tmax] int32 the slot of each step (0-padded)."""
    if orders < 1:
        raise ValueError("orders must be >= 1")
    if slot_policy not in ("given", "confident"):
        raise ValueError(f"slot_policy must be 'given' or 'confident', got {slot_policy!r}")
    confident = slot_policy == "confident"
    if confident and orders != 1:
        raise ValueError("slot_policy='confident' takes orders=1: the visiting order is the model's own")
    J = len(jobs)
    n_rows = J * orders
    rank, world, _ = D.env_rank_world()
    lo, hi = D.shard_bounds(n_rows, rank, world)
    is_ab = model.kind == "ab"
    Tmax = max([len(j.loc) for j in jobs] + [1])
    jid = np.arange(J, dtype=np.int64) if job_ids is None else np.asarray(job_ids, dtype=np.int64)
    all_order = np.zeros((J, orders, Tmax), np.int32)
    for j, job in enumerate(jobs):
        all_order[j, :, :len(job.loc)] = np.asarray(job.loc, np.int32) if confident else draw_orders(job.loc, orders, seed, int(jid[j]))
    out = np.zeros((hi - lo, Tmax), np.float32)
    taken = np.zeros((hi - lo, Tmax), np.int32) if confident else None
    more = {} if int(slots_per_step) == 1 else {"slots_per_step": int(slots_per_step)}
    if confident:
        more["slot_policy"] = slot_policy
    if truncation is not None and not truncation.neutral:
        more["truncation"] = truncation
    if confidence is not None and float(confidence) != 0.0:
        more["confidence"] = float(confidence)
    from .sampler import _id_runs
    pos = np.arange(lo, hi)
    gids = jid[pos // orders] * orders + pos % orders
    for cs, ce in _id_runs(gids, device_batch):
        ids = pos[cs:ce]
        jb = [jobs[i // orders] for i in ids]
        tok = np.stack([np.asarray(j.tokens) for j in jb]).astype(np.int32)
        reg = np.stack([j.region for j in jb]).astype(np.int32)
        order = np.stack([all_order[i // orders, i % orders] for i in ids])
        T = np.array([len(j.loc) for j in jb], np.int32)
        chain = np.array([j.chain[0] for j in jb] + [j.chain[1] for j in jb], np.int32) if is_ab else None
        out[cs:ce] = model.score(tok, reg, chain, order, T, dropout=dropout, parallel=parallel, device_batch=device_batch,
                                 seed=seed, row0=int(gids[cs]), **more)
        if confident:
            taken[cs:ce] = model.sample_order(len(jb), Tmax)
    # one gather, as for the tokens: the float32 bits travel as int32
    got = D.gather_rows(out.view(np.int32), n_rows, Tmax, all_ranks)
    got_order = D.gather_rows(taken, n_rows, Tmax, all_ranks) if confident else None
    if got is None:
        return None
    if confident:
        all_order = np.ascontiguousarray(got_order, dtype=np.int32).reshape(J, orders, Tmax)
    logp = np.ascontiguousarray(got, dtype=np.int32).view(np.float32).reshape(J, orders, Tmax)
    T = np.array([len(j.loc) for j in jobs], np.int64)
    total = logp.astype(np.float64).sum(axis=2)
    mean = total.mean(axis=1)
    with np.errstate(invalid="ignore"):              # (a -inf total -- a token the truncation removes -- has no spread: nan)
        std = total.std(axis=1)
    return {"total": total, "mean": mean, "std": std, "per_residue": np.where(T > 0, mean / np.maximum(T, 1), 0.0),
            "T": T, "logp": logp, "order": all_order}


SCAN_GROUP = 64                          # slots one row of a context="masked" scan scores: the largest block size (hd_set_slots_per_step)
SCAN_CONTEXTS = ("given", "masked")


def expand_scan(tokens, region, chain, loc, T, context: str = "given") -> Expanded:
    """The rows of a mutational scan of the slots ``loc[b, :T[b]]`` of complete sequences ``tokens`` [B, L].

    ``context="given"`` (the pseudo-likelihood form): every (b, s in loc[b]) becomes one row -- the complete row with slot s alone
    masked, order ``[s]``, T = 1.  Rows are b-major, in the order of ``loc``.

    ``context="masked"`` (the distribution the sampler meets at its first step): every job becomes ceil(T / 64) rows, each with ALL of
    ``loc[b]`` masked and a group of at most 64 of the slots as its order (0-padded to 64), to be scored in sessions of block size 64
    with Tmax = 64.  A row holds one group only, so no group sees another's targets."""
    if context not in SCAN_CONTEXTS:
        raise ValueError(f"context must be one of {SCAN_CONTEXTS}, got {context!r}")
    tokens = np.asarray(tokens, np.int32)
    region = np.asarray(region, np.int32)
    T = np.asarray(T, np.int64).reshape(-1)
    B, L = tokens.shape
    loc = np.asarray(loc, np.int32)
    loc = loc.reshape(B, loc.shape[1] if loc.ndim == 2 else (loc.size // B if B else 0))
    if T.shape[0] != B or (T < 0).any() or (T > loc.shape[1]).any():
        raise ValueError(f"T must be [{B}] with 0 <= T[b] <= {loc.shape[1]}")
    K = 1 if context == "given" else SCAN_GROUP
    rows = np.repeat(np.arange(B), (T + K - 1) // K)
    steps = np.concatenate([np.arange(0, t, K) for t in T] + [np.zeros(0, np.int64)]).astype(np.int64)
    N = rows.shape[0]
    tok = tokens[rows].copy()
    grp = np.zeros((N, K), np.int32)
    Tg = np.zeros(N, np.int32)
    for i in range(N):
        b, t0, n = int(rows[i]), int(steps[i]), int(T[rows[i]])
        Tg[i] = min(K, n - t0)
        grp[i, :Tg[i]] = loc[b, t0:t0 + Tg[i]]
        tok[i, grp[i, :Tg[i]] if K == 1 else loc[b, :n]] = MASK_TOKEN
    ch = None
    if chain is not None:
        chain = np.asarray(chain, np.int32).reshape(-1)
        if chain.shape[0] != 2 * B:
            raise ValueError(f"chain must be [{2 * B}] (heavy ids, then light ids)")
        ch = np.concatenate([chain[:B][rows], chain[B:][rows]]).astype(np.int32)
    return Expanded(tokens=tok, region=region[rows].copy(), chain=ch, order=grp, T=Tg, rows=rows, steps=steps, B=B, slots_per_step=K)


def scan_jobs(model, jobs: Sequence, *, context: str = "given", device_batch: int = 256, all_ranks: bool = False,
              temperature: float = 1.0, truncation=None):
    """Mutational scan: the model's whole 22-token distribution at every slot of every job's ``loc``, read from the device's
    distribution record (include/hudiff_hip.h "distribution record") -- one forward per row of ``expand_scan``, not one per token.

    ``Job.tokens`` are COMPLETE sequences, as for ``score_jobs``; the jobs' ``guide`` fields, ``temperature`` and ``truncation`` shape
    the distribution as they shape a draw.  ``context``: "given" = every other residue is known (pseudo-likelihood), "masked" = all of
    ``loc`` is masked.  Dropout is off; the expanded rows carry no (row, step) key, as in step-parallel scoring.  Rows shard over ranks
    and are gathered once.  Returns on rank 0 (every rank when single-process or ``all_ranks``; None elsewhere) a dict:
      dist [J, Tmax, 22] float32  log p of every token (guide.LETTERS order) at position t of ``loc``; -inf = removed; 0 where t >= T
      slot [J, Tmax] int32        the slot of position t         wt [J, Tmax] int32      the residue the sequence has there
      logp_wt [J, Tmax] float32   dist at the wild type          entropy [J, Tmax] float64 (nats, guide.dist_entropy)
      T [J]                       scanned slots                  pseudo_ll [J] float64   sum_t logp_wt."""
    from .guide import Guide, dist_entropy
    J = len(jobs)
    is_ab = model.kind == "ab"
    Lm = model.max_len
    Tmax = max([len(j.loc) for j in jobs] + [1])
    T = np.array([len(j.loc) for j in jobs], np.int64)
    slot = np.zeros((J, Tmax), np.int32)
    for j, job in enumerate(jobs):
        slot[j, :T[j]] = np.asarray(job.loc, np.int32)
    tok = np.stack([np.asarray(j.tokens) for j in jobs]).astype(np.int32) if J else np.zeros((0, Lm), np.int32)
    reg = np.stack([j.region for j in jobs]).astype(np.int32) if J else np.zeros((0, Lm), np.int32)
    chain = np.array([j.chain[0] for j in jobs] + [j.chain[1] for j in jobs], np.int32) if is_ab else None
    x = expand_scan(tok, reg, chain, slot, T, context)
    N, K = x.rows.shape[0], x.slots_per_step
    # a scoring session takes its targets from the tokens it is given (and masks the scored slots itself): the wild type goes back
    live = np.arange(K)[None, :] < x.T[:, None]
    rr = np.broadcast_to(np.arange(N)[:, None], (N, K))[live]
    x.tokens[rr, x.order[live]] = tok[x.rows[rr], x.order[live]]
    guided = float(temperature) != 1.0 or any(j.guide is not None for j in jobs)
    more = {}
    if truncation is not None and not truncation.neutral:
        more["truncation"] = truncation
    rank, world, _ = D.env_rank_world()
    lo, hi = D.shard_bounds(N, rank, world)
    flat = np.zeros((hi - lo, K, 22), np.float32)
    for s in range(lo, hi, int(device_batch)):
        e = min(hi, s + int(device_batch))
        ch = None if x.chain is None else np.ascontiguousarray(np.concatenate([x.chain[s:e], x.chain[N + s:N + e]]))
        if guided:
            more["guide"] = Guide.stack([jobs[b].guide for b in x.rows[s:e]], Lm, temperature)
        _, flat[s - lo:e - lo] = model.score(np.ascontiguousarray(x.tokens[s:e]), np.ascontiguousarray(x.region[s:e]), ch,
                                             np.ascontiguousarray(x.order[s:e]), np.ascontiguousarray(x.T[s:e]), dropout="off",
                                             parallel=False, slots_per_step=K, return_dist=True, **more)
    # one gather, as for the tokens: the float32 bits travel as int32
    got = D.gather_rows(flat.reshape(hi - lo, K * 22).view(np.int32), N, K * 22, all_ranks)
    if got is None:
        return None
    dist = x.fold_dist(np.ascontiguousarray(got, dtype=np.int32).view(np.float32).reshape(N, K, 22), Tmax)
    wt = np.take_along_axis(tok, slot, axis=1).astype(np.int32) if J else np.zeros((0, Tmax), np.int32)
    valid = np.arange(Tmax)[None, :] < T[:, None]
    wt = np.where(valid, wt, 0).astype(np.int32)
    logp_wt = np.where(valid, np.take_along_axis(dist, wt[..., None].astype(np.int64), axis=2)[..., 0], np.float32(0)).astype(np.float32)
    return {"dist": dist, "slot": slot, "wt": wt, "logp_wt": logp_wt, "entropy": np.where(valid, dist_entropy(dist), 0.0), "T": T,
            "pseudo_ll": logp_wt.astype(np.float64).sum(axis=1)}
