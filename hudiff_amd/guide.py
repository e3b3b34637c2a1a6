"""Guided sampling: per-slot residue constraints, temperature and logit bias (include/hudiff_hip.h "guided sampling").

For row b visiting slot s with raw logits z[0:22] the draw stage of a guided session uses

    g_j   = (z_j + bias[b, s, j]) / temperature    for the tokens j allowed at (b, s), -inf for the others
    p     = softmax(g);  token = argmax_j p_j / q_j  (q = the noise of the unguided draw);  logp = log p_token

``allow[b, s]`` is a uint32 whose bit j (0..21, the tokenizer's ids: 'ACDEFGHIKLMNPQRSTVWY', 'X' = 20, '-' = 21) allows token j.
temperature == 0 is the greedy decode: argmax_j (z_j + bias_j) over the allowed j, no noise; its recorded log-probability is the
token's under the temperature-1 guided distribution.

A ``Guide`` is what ``model.sample(..., guide=)`` / ``model.score(..., guide=)`` and ``sampler.Job.guide`` take; ``guided_log_probs`` is
the same definition in numpy float64 for host-side users; ``parse_constraints`` reads the text form of the CLIs' ``--constraints_fpath``.

A ``Truncation`` (top_k, top_p, min_p; include/hudiff_hip.h "truncated sampling") cuts the tail of that distribution in front of the
draw; ``truncation_keep`` is its keep-set in float64, and ``guided_log_probs`` / ``confidence_keys`` take it as ``truncation=``.

A ``Budget`` (origin, max_mutations; include/hudiff_hip.h "mutation budget") caps the slots in which a row may differ from its origin;
``budget_walk`` is its rules 1 and 3 in numpy.

Refinement rounds (include/hudiff_hip.h "refinement rounds"): ``refine_args`` checks a ``refine=dict(rounds=, slots=, below=)``,
``refine_tcap`` is the order capacity such a session needs, ``refine_select`` the rule of a round in numpy, ``refine_live`` /
``refine_fold`` read a record that is keyed by order position slot by slot.
"""
from __future__ import annotations

import numpy as np

from . import tables as T
from .tokenizer import Tokenizer

N_DRAW = 22                              # tokens the draw stage ranges over (sample.py:510)
ALL_TOKENS = (1 << N_DRAW) - 1
_TK = Tokenizer()
LETTERS = "".join(_TK.toks[:N_DRAW])     # 'ACDEFGHIKLMNPQRSTVWYX-'


def letters_mask(letters: str) -> int:
    """Bits of the tokens named by ``letters`` (tokenizer letters, '-' included); an unknown letter raises ValueError."""
    m = 0
    for c in letters:
        i = LETTERS.find(c)
        if i < 0:
            raise ValueError(f"unknown residue letter {c!r} (known: {LETTERS})")
        m |= 1 << i
    return m


class Guide:
    """allow: uint32 [L] or [B, L] (None = everything allowed); bias: float32 [L, 22] or [B, L, 22] (None = none); temperature:
    0 = greedy, else in [0.01, 100].  The [L] forms describe every row of whatever batch consumes the guide."""

    def __init__(self, allow=None, bias=None, temperature=1.0):
        self.allow = None if allow is None else np.ascontiguousarray(np.asarray(allow), dtype=np.uint32)
        self.bias = None if bias is None else np.ascontiguousarray(np.asarray(bias), dtype=np.float32)
        self.temperature = float(temperature)
        if self.allow is not None and self.allow.ndim not in (1, 2):
            raise ValueError(f"allow must be [L] or [B, L], got {self.allow.shape}")
        if self.bias is not None and (self.bias.ndim not in (2, 3) or self.bias.shape[-1] != N_DRAW):
            raise ValueError(f"bias must be [L, {N_DRAW}] or [B, L, {N_DRAW}], got {self.bias.shape}")

    def batch(self, B, L):
        """-> (allow uint32 [B, L] or None, bias float32 [B, L, 22] or None), the [L] forms broadcast to B rows."""
        allow, bias = self.allow, self.bias
        if allow is not None:
            if allow.shape not in ((L,), (B, L)):
                raise ValueError(f"allow must be [{L}] or [{B}, {L}], got {allow.shape}")
            allow = np.ascontiguousarray(np.broadcast_to(allow, (B, L)))
        if bias is not None:
            if bias.shape not in ((L, N_DRAW), (B, L, N_DRAW)):
                raise ValueError(f"bias must be [{L}, {N_DRAW}] or [{B}, {L}, {N_DRAW}], got {bias.shape}")
            bias = np.ascontiguousarray(np.broadcast_to(bias, (B, L, N_DRAW)))
        return allow, bias

    def take(self, rows):
        """The guide of the rows ``rows`` of the batch this one describes (step-parallel scoring: an expanded row takes the guide of
        the row it came from)."""
        rows = np.asarray(rows)
        allow = self.allow if self.allow is None or self.allow.ndim == 1 else self.allow[rows]
        bias = self.bias if self.bias is None or self.bias.ndim == 2 else self.bias[rows]
        return Guide(allow, bias, self.temperature)

    @staticmethod
    def stack(guides, L, temperature=1.0):
        """Per-row guides ([L] forms or None) -> one [B, L] guide; rows without a guide allow everything with zero bias."""
        allow = np.full((len(guides), L), ALL_TOKENS, np.uint32)
        bias = np.zeros((len(guides), L, N_DRAW), np.float32) if any(g is not None and g.bias is not None for g in guides) else None
        for r, g in enumerate(guides):
            if g is None:
                continue
            a, b = g.batch(1, L)
            if a is not None:
                allow[r] = a[0]
            if b is not None:
                bias[r] = b[0]
        return Guide(allow, bias, temperature)


class Truncation:
    """top_k: keep the k best tokens (0 or >= 22 = off); top_p: keep the smallest head whose probability mass reaches top_p (in
    (0, 1], 1 = off); min_p: keep the tokens with p >= min_p * p_max (in [0, 1], 0 = off).  The best token always stays.  Validates
    as hd_set_truncation does; ``neutral`` = nothing is cut (such a truncation is never handed to the library)."""

    def __init__(self, top_k=0, top_p=1.0, min_p=0.0):
        if isinstance(top_k, (bool, float)) or int(top_k) != top_k or not 0 <= int(top_k) <= N_DRAW:
            raise ValueError(f"top_k must be an integer in [0, {N_DRAW}], got {top_k!r}")
        top_p, min_p = float(top_p), float(min_p)
        if not 0.0 < top_p <= 1.0:                   # (NaN fails every comparison)
            raise ValueError(f"top_p must be in (0, 1], got {top_p!r}")
        if not 0.0 <= min_p <= 1.0:
            raise ValueError(f"min_p must be in [0, 1], got {min_p!r}")
        self.top_k, self.top_p, self.min_p = int(top_k), top_p, min_p

    @property
    def neutral(self):
        return self.top_k in (0, N_DRAW) and self.top_p >= 1.0 and self.min_p == 0.0

    def __eq__(self, other):
        return isinstance(other, Truncation) and (self.top_k, self.top_p, self.min_p) == (other.top_k, other.top_p, other.min_p)

    def __hash__(self):
        return hash((self.top_k, self.top_p, self.min_p))

    def __repr__(self):
        return f"Truncation(top_k={self.top_k}, top_p={self.top_p}, min_p={self.min_p})"


FREE = N_DRAW                            # origin of a slot that has none: never forced, never counted


class Budget:
    """origin: int32 [L] or [B, L], token 0..21 = the residue a draw at that slot is compared with, 22 (``FREE``) = the slot has no
    origin; max_mutations: an int or int32 [B], >= 0.  A row that has written max_mutations tokens different from their origin draws
    its origin at every origin-bearing slot from then on.  The [L] / scalar forms describe every row of whatever batch consumes it."""

    def __init__(self, origin, max_mutations):
        self.origin = np.ascontiguousarray(np.asarray(origin), dtype=np.int32)
        self.max_mutations = np.asarray(max_mutations).astype(np.int32)      # (0-d stays 0-d: the scalar form)
        if self.origin.ndim not in (1, 2):
            raise ValueError(f"origin must be [L] or [B, L], got {self.origin.shape}")
        if self.max_mutations.ndim not in (0, 1):
            raise ValueError(f"max_mutations must be an integer or [B], got {self.max_mutations.shape}")
        if np.asarray(max_mutations).dtype.kind not in "iu" or (self.max_mutations < 0).any():
            raise ValueError(f"max_mutations must be integers >= 0, got {max_mutations!r}")

    def batch(self, B, L):
        """-> (origin int32 [B, L], max_mutations int32 [B]), the [L] / scalar forms broadcast to B rows."""
        if self.origin.shape not in ((L,), (B, L)):
            raise ValueError(f"origin must be [{L}] or [{B}, {L}], got {self.origin.shape}")
        if self.max_mutations.shape not in ((), (B,)):
            raise ValueError(f"max_mutations must be an integer or [{B}], got {self.max_mutations.shape}")
        return (np.ascontiguousarray(np.broadcast_to(self.origin, (B, L))),
                np.ascontiguousarray(np.broadcast_to(self.max_mutations, (B,))))

    def take(self, rows):
        """The budget of the rows ``rows`` of the batch this one describes (beam search: a replica takes the budget of its group)."""
        rows = np.asarray(rows)
        return Budget(self.origin if self.origin.ndim == 1 else self.origin[rows],
                      self.max_mutations if self.max_mutations.ndim == 0 else self.max_mutations[rows])

    @staticmethod
    def stack(budgets, L):
        """Per-row budgets ([L] / scalar forms, or None) -> one [B, L] budget; a row without one is free everywhere."""
        origin = np.full((len(budgets), L), FREE, np.int32)
        max_mut = np.zeros(len(budgets), np.int32)
        for r, b in enumerate(budgets):
            if b is None:
                continue
            o, m = b.batch(1, L)
            origin[r], max_mut[r] = o[0], m[0]
        return Budget(origin, max_mut)


def budget_walk(tokens_written, origin, order, T, max_mutations):
    """Rules 1 and 3 of include/hudiff_hip.h "mutation budget" in numpy.  tokens_written int [B, Tmax]: the token row b wrote at order
    position t (of a finished session without a repeated slot: ``tokens[b, order[b, t]]``); origin int [B, L]; order int [B, Tmax];
    T int [B]; max_mutations int [B] (or an int).  Returns ``(exhausted, n)``: bool [B, Tmax], position t met the row with its budget
    spent at an origin-bearing slot (entries at t >= T[b] are False); int32 [B], the mutations counted over the whole row -- targets of
    a scoring session are counted too, so n may pass max_mutations."""
    w, origin, order = np.asarray(tokens_written), np.asarray(origin), np.asarray(order)
    if origin.ndim != 2 or order.ndim != 2 or order.shape[0] != origin.shape[0] or w.shape != order.shape:
        raise ValueError(f"origin must be [B, L], order and tokens_written [B, Tmax]; got {origin.shape}, {order.shape}, {w.shape}")
    B, Tmax = order.shape
    T = np.asarray(T).reshape(-1)
    M = np.broadcast_to(np.asarray(max_mutations), (B,))
    if T.shape != (B,):
        raise ValueError(f"T must be [{B}], got {T.shape}")
    exhausted = np.zeros((B, Tmax), bool)
    n = np.zeros(B, np.int32)
    for b in range(B):
        for t in range(int(T[b])):
            o = int(origin[b, order[b, t]])
            exhausted[b, t] = o <= 21 and n[b] >= M[b]
            if o <= 21 and int(w[b, t]) != o:
                n[b] += 1
    return exhausted, n


def truncation_keep(g22, truncation):
    """The keep-set of include/hudiff_hip.h "truncated sampling" in numpy float64: g22 [..., 22] are the values the draw forms (-inf =
    not allowed) -> bool [..., 22].  Tokens are ranked on g, the lower index first among equals; token j is kept when it is allowed,
    its rank is below top_k, the mass of the tokens ranked ahead of it is below top_p of the whole and exp(g_j - max g) >= min_p; the
    best token is always kept.  ``truncation`` None or neutral keeps every allowed token."""
    g = np.asarray(g22, np.float64)
    if g.shape[-1] != N_DRAW:
        raise ValueError(f"g22 must end in {N_DRAW} tokens, got {g.shape}")
    allowed = g > -np.inf
    if truncation is None or truncation.neutral:
        return allowed
    with np.errstate(invalid="ignore"):
        e = np.where(allowed, np.exp(g - g.max(axis=-1, keepdims=True)), 0.0)
    idx = np.arange(N_DRAW)
    # ahead[..., j, i]: token i is ranked ahead of token j
    gj, gi = g[..., :, None], g[..., None, :]
    ahead = allowed[..., None, :] & ((gi > gj) | ((gi == gj) & (idx[None, :] < idx[:, None])))
    rank = ahead.sum(axis=-1)
    before = np.where(ahead, e[..., None, :], 0.0).sum(axis=-1)
    keep = allowed.copy()
    if 0 < truncation.top_k < N_DRAW:
        keep &= rank < truncation.top_k
    if truncation.top_p < 1.0:
        keep &= before < truncation.top_p * e.sum(axis=-1, keepdims=True)
    if truncation.min_p > 0.0:
        keep &= e >= truncation.min_p
    return keep | (allowed & (rank == 0))


def guided_log_probs(logits22, allow, bias=None, temperature=1.0, truncation=None):
    """The definition in numpy float64: logits22 [..., 22], allow [...] (uint32 bits), bias [..., 22] or None -> log p [..., 22],
    -inf where a token is not allowed.  temperature == 0 (greedy) gives the temperature-1 distribution, the one a greedy session
    records its log-probabilities under; the greedy token is the argmax of the result.  ``truncation`` (a Truncation): the
    distribution is renormalised over ``truncation_keep`` and -inf for the tokens that are not kept, too."""
    z = np.asarray(logits22, np.float64)
    if z.shape[-1] != N_DRAW:
        raise ValueError(f"logits22 must end in {N_DRAW} tokens, got {z.shape}")
    if bias is not None:
        z = z + np.asarray(bias, np.float64)
    tp = float(temperature)
    if tp != 0.0:
        z = z / tp
    ok = ((np.asarray(allow, np.int64)[..., None] >> np.arange(N_DRAW)) & 1).astype(bool)
    g = np.where(ok, z, -np.inf)
    if truncation is not None and not truncation.neutral:
        g = np.where(truncation_keep(g, truncation), g, -np.inf)
    mx = g.max(axis=-1, keepdims=True)
    with np.errstate(divide="ignore"):
        return (g - mx) - np.log(np.exp(g - mx).sum(axis=-1, keepdims=True))


def dist_entropy(dist):
    """Entropy in nats, float64 [...], of a distribution record ``dist`` [..., 22] (log-probabilities, -inf = removed; the device's
    record, model.sample_dist, or ``guided_log_probs``): -sum_j p_j log p_j over the finite entries."""
    lp = np.asarray(dist, np.float64)
    if lp.shape[-1] != N_DRAW:
        raise ValueError(f"dist must end in {N_DRAW} tokens, got {lp.shape}")
    fin = np.isfinite(lp)
    lp = np.where(fin, lp, 0.0)
    return -np.where(fin, np.exp(lp) * lp, 0.0).sum(axis=-1)


def dist_log_odds(dist, wt):
    """Log-odds of every token against the wild type: ``dist - dist[..., wt]``, float64 [..., 22]; ``wt`` int [...] (the residue that
    is there).  A removed token gives -inf; where the wild type itself is removed every finite entry gives +inf (and -inf - -inf is nan)."""
    lp = np.asarray(dist, np.float64)
    if lp.shape[-1] != N_DRAW:
        raise ValueError(f"dist must end in {N_DRAW} tokens, got {lp.shape}")
    w = np.asarray(wt, np.int64)
    if w.shape != lp.shape[:-1] or (w < 0).any() or (w >= N_DRAW).any():
        raise ValueError(f"wt must be {lp.shape[:-1]} with values in [0, {N_DRAW}), got {w.shape}")
    with np.errstate(invalid="ignore"):
        return lp - np.take_along_axis(lp, w[..., None], axis=-1)


def confidence_keys(logits, allow=None, bias=None, temperature=1.0, truncation=None):
    """The key of slot_policy="confident" (include/hudiff_hip.h "slot policy") in numpy float64: logits [..., >= 22] (the first 22
    tokens are the draw's), allow [...] uint32 bits or None (everything allowed), bias [..., 22] or None -> log c [...], with
        c = sum_j exp(g_j - max_j g_j) = 1 / max_j p_j,   g_j = (z_j + bias_j) / temperature over the allowed tokens, -inf elsewhere
    (divisor 1 at temperature 0, as the draw).  Smaller is more confident.  A slot whose c is not a finite positive number -- a NaN
    or +inf logit, nothing allowed -- gets +inf: it ranks behind every finite key.  ``truncation`` (a Truncation): the sum runs over
    ``truncation_keep`` only, c = 1 / max_j p'_j of the truncated distribution."""
    z = np.asarray(logits, np.float64)[..., :N_DRAW]
    if z.shape[-1] != N_DRAW:
        raise ValueError(f"logits must end in at least {N_DRAW} tokens, got {z.shape}")
    if bias is not None:
        z = z + np.asarray(bias, np.float64)
    tp = float(temperature)
    if tp != 0.0:
        z = z / tp
    if allow is not None:
        ok = ((np.asarray(allow, np.int64)[..., None] >> np.arange(N_DRAW)) & 1).astype(bool)
        z = np.where(ok, z, -np.inf)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        if truncation is not None and not truncation.neutral:
            z = np.where(truncation_keep(z, truncation), z, -np.inf)
        c = np.exp(z - z.max(axis=-1, keepdims=True)).sum(axis=-1)
        good = np.isfinite(c) & (c > 0)
        return np.where(good, np.log(np.where(good, c, 1.0)), np.inf)


def confidence_tau(tau):
    """A confidence threshold as the library takes it: a finite float in [0, 1] (0 = none); anything else is a ValueError."""
    if isinstance(tau, (bool, str, bytes)) or tau is None:
        raise ValueError(f"confidence must be a number in [0, 1], got {tau!r}")
    try:
        t = float(tau)
    except (TypeError, ValueError):
        raise ValueError(f"confidence must be a number in [0, 1], got {tau!r}") from None
    if not (np.isfinite(t) and 0.0 <= t <= 1.0):
        raise ValueError(f"confidence must be finite and in [0, 1], got {tau!r}")
    return t


def confidence_cmax(tau):
    """The kernel argument of a confidence threshold (include/hudiff_hip.h "confidence threshold"): cmax = 1.0f / tau, one float32
    division of the float32 tau -- a key c = 1 / p_max qualifies iff c <= cmax.  tau in (0, 1]."""
    t = confidence_tau(tau)
    if t == 0.0:
        raise ValueError("confidence 0 means no threshold: there is no cmax")
    with np.errstate(over="ignore"):
        return np.float32(1.0) / np.float32(t)


def threshold_select(c32, K, cmax):
    """Steps 2 to 4 of include/hudiff_hip.h "confidence threshold" in numpy float32: c32 float32 [N] are the keys of the N >= 1
    remaining positions of one row, in list order; K the cap; cmax float32.  A key that is not a finite positive number becomes +inf;
    q = the keys with c <= cmax (an infinite one never qualifies); cnt = min(K, N, max(1, q)); the cnt smallest (c, i), compared
    lexicographically, are chosen.  Returns ``(chosen, cnt, perm)``: int64 [cnt], the chosen positions in rank order; the count; int64
    [N], the whole permutation -- new position r holds old position perm[r]: the chosen ones, then the others in their previous
    relative order."""
    c = np.array(c32, dtype=np.float32).reshape(-1)
    N, K = c.size, int(K)
    if N < 1 or K < 1:
        raise ValueError(f"threshold_select needs at least one key and K >= 1, got N = {N}, K = {K}")
    cmax = np.float32(cmax)
    with np.errstate(invalid="ignore"):
        c = np.where((c > 0) & (c < np.inf), c, np.float32(np.inf)).astype(np.float32)      # (NaN compares false)
        q = int(np.count_nonzero((c < np.inf) & (c <= cmax)))
    cnt = min(K, N, max(1, q))
    rank = np.argsort(c, kind="stable")              # a stable sort keeps list order among equal keys
    chosen = rank[:cnt].astype(np.int64)
    rest = np.setdiff1d(np.arange(N), chosen)        # (sorted: the previous relative order)
    return chosen, cnt, np.concatenate([chosen, rest]).astype(np.int64)


REFINE_MAX_ROUNDS, REFINE_MAX_SLOTS = 16, 64


def refine_args(refine):
    """A refinement as the library takes it (include/hudiff_hip.h "refinement rounds"): ``refine`` is None, or a mapping with ``rounds``
    in [1, 16], ``slots`` in [1, 64] and optionally ``below``, a finite float <= 0 (default 0).  Returns None when there is nothing to
    arm (None, or rounds == 0), else ``(rounds, slots, below)``; anything else is a ValueError."""
    if refine is None:
        return None
    try:
        unknown = set(refine) - {"rounds", "slots", "below"}
        rounds, slots, below = refine["rounds"], refine.get("slots", 1), refine.get("below", 0.0)
    except (TypeError, KeyError, AttributeError):
        raise ValueError(f"refine must be a mapping with rounds, slots and optionally below, got {refine!r}") from None
    if unknown:
        raise ValueError(f"refine has unknown keys {sorted(unknown)}")
    for name, v in (("rounds", rounds), ("slots", slots)):
        if isinstance(v, (bool, float, str, bytes)) or v is None or int(v) != v:
            raise ValueError(f"refine {name} must be an integer, got {v!r}")
    rounds, slots = int(rounds), int(slots)
    if rounds == 0:
        return None
    if not 1 <= rounds <= REFINE_MAX_ROUNDS:
        raise ValueError(f"refine rounds must be in [0, {REFINE_MAX_ROUNDS}], got {rounds}")
    if not 1 <= slots <= REFINE_MAX_SLOTS:
        raise ValueError(f"refine slots must be in [1, {REFINE_MAX_SLOTS}], got {slots}")
    if isinstance(below, (bool, str, bytes)) or below is None:
        raise ValueError(f"refine below must be a finite number <= 0, got {below!r}")
    below = float(below)
    if not (np.isfinite(below) and below <= 0.0):
        raise ValueError(f"refine below must be a finite number <= 0, got {below!r}")
    return rounds, slots, float(np.float32(below))


def refine_tcap(T, rounds, slots, K=1):
    """Order positions a session with refinement rounds can come to use: with e = T, ``rounds`` times e = ceil(e / K) * K + slots; the
    largest e over the rows of ``T`` (a number or an array).  The ``Tmax`` of such a session must be at least this."""
    rounds, slots, K = int(rounds), int(slots), int(K)
    if rounds < 0 or slots < 0 or K < 1:
        raise ValueError(f"refine_tcap needs rounds >= 0, slots >= 0 and K >= 1, got {rounds}, {slots}, {K}")
    e = np.asarray(T, dtype=np.int64).reshape(-1)
    for _ in range(rounds):
        e = (e + K - 1) // K * K + slots
    return int(e.max()) if e.size else 0


def refine_live(order, T_now):
    """bool, the shape of ``order`` ([Tmax] or [B, Tmax]): position t is LIVE iff t < T_now, order[t] is not a hole (-1) and no later
    position below T_now holds the same slot -- the position whose draw is the row's final token at that slot."""
    order = np.asarray(order)
    one = order.ndim == 1
    o2 = order.reshape(1, -1) if one else order
    Tn = np.asarray(T_now, dtype=np.int64).reshape(-1)
    if o2.ndim != 2 or Tn.shape != (o2.shape[0],):
        raise ValueError(f"order must be [Tmax] or [B, Tmax] and T_now one entry per row, got {order.shape}, {Tn.shape}")
    live = np.zeros(o2.shape, dtype=bool)
    for b in range(o2.shape[0]):
        seen = set()
        for t in range(int(Tn[b]) - 1, -1, -1):
            s = int(o2[b, t])
            if s >= 0 and s not in seen:
                seen.add(s)
                live[b, t] = True
    return live[0] if one else live


def refine_select(logp, order, T_now, slots, below=0.0):
    """The rule of a refinement round for ONE row, in numpy (include/hudiff_hip.h "refinement rounds", 1 and 2): ``logp`` float32
    [Tmax] and ``order`` int [Tmax] are the row's record and order as they stand, ``T_now`` its positions in use.  The live positions
    with logp < below (a float32 compare; NaN never qualifies) are ranked by (logp, position) ascending and the first
    min(slots, candidates) are chosen.  Returns ``(slot, position)``: int64 [R_b] each, in rank order -- the round appends ``slot`` to
    the order at base, base + 1, ... and takes the guide's entries from ``position``."""
    lp = np.asarray(logp, dtype=np.float32).reshape(-1)
    od = np.asarray(order).reshape(-1)
    if lp.shape != od.shape:
        raise ValueError(f"logp and order must have one shape, got {lp.shape}, {od.shape}")
    T_now, slots = int(T_now), int(slots)
    if not 0 <= T_now <= od.size or slots < 1:
        raise ValueError(f"refine_select needs 0 <= T_now <= {od.size} and slots >= 1, got {T_now}, {slots}")
    u = np.flatnonzero(refine_live(od, [T_now]))
    with np.errstate(invalid="ignore"):
        u = u[lp[u] < np.float32(below)]
    u = u[np.argsort(lp[u], kind="stable")][:slots]  # (u ascends, and a stable sort keeps that among equal logp)
    return od[u].astype(np.int64), u.astype(np.int64)


def refine_fold(order, T_now, values, L=None):
    """Per-slot values of a refined session: ``values`` [B, Tmax, ...] is keyed by order position (``sample_logp()``,
    ``sample_dist()``, ...); out[b, s, ...] = values[b, u, ...] at the live position u of slot s, 0 for a slot that is not in the
    row's list.  ``L``: slots per row (default: the largest slot in ``order`` + 1)."""
    order, values = np.asarray(order), np.asarray(values)
    if order.ndim != 2 or values.shape[:2] != order.shape:
        raise ValueError(f"order must be [B, Tmax] and values [B, Tmax, ...], got {order.shape}, {values.shape}")
    live = refine_live(order, T_now)
    L = (int(order.max()) + 1 if order.size else 0) if L is None else int(L)
    out = np.zeros((order.shape[0], max(L, 0)) + values.shape[2:], dtype=values.dtype)
    b, t = np.nonzero(live)
    out[b, order[b, t]] = values[b, t]
    return out


def beam_select(cand, width):
    """Step 3 of include/hudiff_hip.h "beam search" in numpy: cand float32 [W, 22] is the candidate table of one group,
    cand[w, j] = score[w] + lp[w, j].  The candidates (w, j) are ranked by cand descending, ties to the smaller (w, j) compared
    lexicographically; a candidate that is -inf or NaN ranks behind every finite one, in (w, j) order among its like.  Returns
    ``(w, j, value)``: int64 [width], int64 [width], float32 [width] -- row r of the group becomes candidate (w[r], j[r]) and takes
    value[r] = cand[w[r], j[r]] (as it stands in the table) for its score."""
    cand = np.asarray(cand, np.float32)
    if cand.ndim != 2 or cand.shape[1] != N_DRAW:
        raise ValueError(f"cand must be [W, {N_DRAW}], got {cand.shape}")
    width = int(width)
    if not 1 <= width <= cand.size:
        raise ValueError(f"width must be in [1, {cand.size}], got {width}")
    flat = cand.reshape(-1)
    key = np.where(flat > -np.inf, flat, -np.inf)    # (NaN compares false)
    order = np.argsort(-key, kind="stable")[:width]  # a stable sort keeps (w, j) order among equal keys
    return order // N_DRAW, order % N_DRAW, flat[order]


def beam_backtrack(tokens, score, parent, logp, T, width):
    """Host side of a finished beam session: tokens [G*W, L], score [G*W], parent [G*W, Tmax] (index inside the group of the row that
    row b continued at position t), the raw step values logp [G*W, Tmax] and T [G] (positions of each group) -> (tokens [G, W, L], score [G, W], logp [G, W, Tmax],
    live [G, W]).  Final row (g, r) reads its history by following parent backwards from position T[g] - 1 (positions t >= T[g] were never run: their
    history is 0); live = finite score."""
    tokens, score = np.asarray(tokens), np.asarray(score, np.float32)
    parent, logp = np.asarray(parent), np.asarray(logp, np.float32)
    W = int(width)
    B = tokens.shape[0]
    if W < 1 or B % W != 0:
        raise ValueError(f"{B} rows are not whole groups of width {W}")
    G, Tmax = B // W, parent.shape[1]
    if score.shape != (B,) or parent.shape != (B, Tmax) or logp.shape != (B, Tmax):
        raise ValueError(f"score / parent / logp must be [{B}], [{B}, Tmax], [{B}, Tmax]; got {score.shape}, {parent.shape}, {logp.shape}")
    if parent.size and (parent.min() < 0 or parent.max() >= W):
        raise ValueError(f"parent indices must be in [0, {W})")
    T = np.asarray(T).reshape(-1)
    if T.shape != (G,):
        raise ValueError(f"T must be [{G}] (one entry per group), got {T.shape}")
    hist = np.zeros((G, W, Tmax), np.float32)
    base = (np.arange(G) * W)[:, None]
    cur = np.broadcast_to(np.arange(W), (G, W)).copy()           # the row (inside its group) whose step value position t reads
    for t in range(Tmax - 1, -1, -1):
        rows, run = base + cur, (t < T)[:, None]
        hist[:, :, t] = np.where(run, logp[rows, t], 0.0)
        cur = np.where(run, parent[rows, t], cur)
    return tokens.reshape(G, W, -1), score.reshape(G, W), hist, np.isfinite(score).reshape(G, W)


def parse_constraints(lines, kind):
    """Text constraints -> allow uint32 [L] (L = 291 for kind 'ab', 152 for 'nb').

    One constraint per line, ``chain,position,residues``: chain 'H' or 'L' ('H' only for nanobodies); position an IMGT label of
    tables.HEAVY_POSITIONS / LIGHT_POSITIONS or '*' (every position of the chain); residues a string of tokenizer letters ('-'
    included), a leading '!' meaning "all but these".  Lines intersect; '#' starts a comment; an unknown chain, position or letter
    is a ValueError that names the line."""
    if kind not in ("ab", "nb"):
        raise ValueError(f"kind must be 'ab' or 'nb', got {kind!r}")
    L = T.AB_LEN if kind == "ab" else T.H_LEN
    allow = np.full(L, ALL_TOKENS, np.uint32)
    for no, raw in enumerate(lines, 1):
        line = raw.split("#", 1)[0].strip()
        if not line:
            continue

        def bad(why):
            return ValueError(f"constraints line {no} ({raw.strip()!r}): {why}")
        parts = [x.strip() for x in line.split(",")]
        if len(parts) != 3:
            raise bad("expected chain,position,residues")
        chain, pos, res = parts
        if chain == "H":
            table, base = T.HEAVY_POSITIONS_dict, 0
        elif chain == "L" and kind == "ab":
            table, base = T.LIGHT_POSITIONS_dict, T.H_LEN
        else:
            raise bad(f"unknown chain {chain!r} (" + ("'H' or 'L'" if kind == "ab" else "a nanobody has 'H' only") + ")")
        if pos == "*":
            slots = np.arange(base, base + len(table))
        elif pos in table:
            slots = np.array([base + table[pos]])
        else:
            raise bad(f"unknown IMGT position {pos!r} of chain {chain}")
        negate = res.startswith("!")
        try:
            mask = letters_mask(res[1:] if negate else res)
        except ValueError as e:
            raise bad(str(e)) from None
        if negate:
            mask = ALL_TOKENS & ~mask
        allow[slots] &= np.uint32(mask)
    return allow
