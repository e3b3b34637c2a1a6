"""Case table and builders for the pruned tail's whole 22-token distribution (hudiff_amd/csrc/hd_api.hip pruned_tail, both forms).  A
plain helper module: tests/test_tail_cases_host.py proves the construction on the CPU, tests/test_gpu_tail_dist.py runs it on the device.

The probe.  A scoring session returns logp[b, 0] = log p(tokens[b, order[b, 0]] | tokens[b] with order[b, 0:T[b]] masked), through the
pruned tail.  Take one sequence, a masked set M that holds the probe slot s, and 22 copies of the row that differ only in
tokens[b, s] = j: with order[b] = [s, M \\ {s} ...] and T[b] = |M| one forward yields the device's whole log-softmax at (sequence, s).
All probes of a sequence share M -- the probe slots of its kind plus the slots the evaluation row still has masked when half of its
own masked slots are filled -- so they share one denoiser input, and ONE float64 oracle forward per sequence is the reference of all of
them: a forward of the full row with M masked, log-softmax over the 22 drawable tokens at s (`oracle_scoring`).

Groups: "prod" = production width (synthetic.AB_CONFIG / NB_CONFIG, weights seed 3, evaluation rows from row0 = 17), "micro" = the
micro models of tests/golden on their trace rows (D = 48 / 32, two heads: other trip counts in head_proj_k and row_value_k).

Bounds.  No constant: the yard-stick of a (group, kind, dropout) is max |log_softmax(oracle float32) - log_softmax(oracle float64)|
over all its probes, pooled; a device value is held to MARGIN x that, two device values to PAIR x MARGIN x that, and MARGIN x
yard-stick must stay below CAP (tests/test_tail_cases_host.py).
"""
from types import SimpleNamespace

import numpy as np

import hudiff_oracle as ho
from conftest import load_cfg, load_weights
from draw_cases import GOLDEN, TRACE
from test_gpu_logp import log_softmax64
from test_gpu_variants import _rows, _weights

N_DRAW, MASK = 22, 22
N_SEQ = 2
# first and last slot, both sides of the chain boundary (antibody: h_len = 152), of every 64-key stride and of the last 16-key tile
SLOTS = {"ab": (0, 15, 16, 63, 64, 151, 152, 255, 256, 287, 288, 290), "nb": (0, 15, 16, 63, 64, 127, 128, 143, 144, 151)}
LENGTH = {"ab": 291, "nb": 152}
H_LEN = 152
MARGIN, PAIR, CAP = 3.0, 2.0, 2e-5
# dropout on: two slots per kind (antibody: one in each chain), six tokens each, a fixed key
DROP_SLOTS = {"ab": (63, 255), "nb": (16, 143)}
DROP_TOKENS = (0, 5, 10, 15, 20, 21)
DROP_KW = dict(dropout="faithful", seed=0x7A11D157, row0=40)
# a later step: order = [a, b, s, ...] with a, b the sequence's first two own masked slots, read at step 2
LATER = {"ab": dict(seq=1, slot=152), "nb": dict(seq=1, slot=64)}
# the small batches of the edge / graph / recorded-path cases: sequence 0, two slots (antibody: both sides of the chain boundary)
EDGE_SLOTS = {"ab": (151, 152), "nb": (63, 64)}

# forms of the tail: (options, session keywords, must witness, must not reach); "default" leaves the choice to the library
FORMS = {
    "sliced": ({"tail_form": 2, "tail_max_rows": 4096}, {}, ("tail_sliced", "value_via_rows"), ("tail_launches", "value_via_projection")),
    "launches_rows": ({"tail_form": 0}, {}, ("tail_launches", "value_via_rows"), ("tail_sliced", "value_via_projection")),
    "launches_proj": ({"prune_value_via_rows": 0}, {}, ("tail_launches", "value_via_projection"), ("tail_sliced", "value_via_rows")),
    "noprune": ({}, {"prune": False}, (), ("tail_sliced", "tail_launches", "value_via_rows", "value_via_projection")),
}
TAIL_FORMS = ("sliced", "launches_rows", "launches_proj")


def forms_of(group):
    """The micro widths are not the sliced kernels' (hd_api.hip tail_form): every micro session takes the launches."""
    return tuple(f for f in FORMS if group == "prod" or f != "sliced")


def main_matrix(group):
    """(form, route) of the all-slots batch: three routes for the form the library picks for that batch size (above 64 sequences per
    lane: the launches, value through rows) and for the sliced form, the library's choice up to 64 sequences per lane (forced here;
    `edge_routes` runs it as selected); split and f32_all for the other forced forms and the unpruned control."""
    three = ("split", "f32_all", "f32_gemm")
    return [("default", r) for r in three] + [(f, r) for f in forms_of(group) for r in (three if f == "sliced" else three[:2])]


def edge_routes(name):
    """The batches at the 64 / 65 switch run with default options: the default form of their size, on all three routes."""
    return ("split", "f32_all", "f32_gemm") if name.startswith(("one_lane", "two_lanes")) else ("split",)


# (id, rows in the session, options, session keywords, must witness, must not reach, groups).  44 probe rows, the rest fillers.
EDGES = [
    # the switch between the forms, selected and not forced: 64 / 65 sequences per lane with default options
    ("one_lane_64", 64, {}, {"lanes": 1}, ("tail_sliced", "value_via_rows", "sample_lanes_1"), ("tail_launches", "sample_lanes_2"), ("prod",)),
    ("one_lane_65", 65, {}, {"lanes": 1}, ("tail_launches", "value_via_rows", "sample_lanes_1"), ("tail_sliced", "sample_lanes_2"), ("prod",)),
    ("two_lanes_128", 128, {}, {"lanes": 2}, ("tail_sliced", "value_via_rows", "sample_lanes_2"), ("tail_launches", "sample_lanes_1"), ("prod",)),
    ("two_lanes_130", 130, {}, {"lanes": 2}, ("tail_launches", "value_via_rows", "sample_lanes_2"), ("tail_sliced", "sample_lanes_1"), ("prod",)),
    # four sequences per workgroup with a ragged last group: rows per lane = 1, 2, 3 mod 4 (45; 46; 47 and 23 + 23)
    ("launches_45", 45, {"tail_form": 0}, {"lanes": 1}, ("tail_launches", "value_via_rows", "sample_lanes_1"), ("tail_sliced",), ("prod", "micro")),
    ("launches_46", 46, {"tail_form": 0}, {"lanes": 1}, ("tail_launches", "value_via_rows", "sample_lanes_1"), ("tail_sliced",), ("prod", "micro")),
    ("launches_47", 47, {"tail_form": 0}, {"lanes": 1}, ("tail_launches", "value_via_rows", "sample_lanes_1"), ("tail_sliced",), ("prod", "micro")),
    ("launches_23_23", 46, {"tail_form": 0, "lane_min_rows": 2}, {"lanes": 2}, ("tail_launches", "value_via_rows", "sample_lanes_2"), ("tail_sliced", "sample_lanes_1"), ("prod", "micro")),
    ("projection_47", 47, {"prune_value_via_rows": 0}, {"lanes": 1}, ("tail_launches", "value_via_projection", "sample_lanes_1"), ("tail_sliced", "value_via_rows"), ("prod", "micro")),
    ("projection_24_23", 47, {"prune_value_via_rows": 0, "lane_min_rows": 2}, {"lanes": 2}, ("tail_launches", "value_via_projection", "sample_lanes_2"), ("tail_sliced", "sample_lanes_1"), ("prod",)),
    ("sliced_23_22", 45, {"lane_min_rows": 2}, {"lanes": 2}, ("tail_sliced", "value_via_rows", "sample_lanes_2"), ("tail_launches", "sample_lanes_1"), ("prod",)),
]


# ---- weights and sequences ---------------------------------------------------------------------------------------------------------------
def weights(group, kind, dropout=False):
    """(config, state dict): dropout 0 in the config unless asked for (then the production p)."""
    if group == "micro":
        assert not dropout
        return load_cfg(kind), load_weights(kind)
    cfg, sd = _weights(kind)
    return (cfg if dropout else dict(cfg, dropout=0.0)), sd


_seqs = {}


def sequences(group, kind):
    """N_SEQ sequences: full [L] complete tokens, region [L], chain (heavy id, light id) or None, own = the slots the row itself still
    has masked, M = own + the probe slots (sorted), masked [L] = full with M masked: the one denoiser input of all its probes."""
    if (group, kind) in _seqs:
        return _seqs[group, kind]
    out = []
    if group == "prod":
        b, half = _rows(kind, N_SEQ)
        for r in range(N_SEQ):
            out.append(SimpleNamespace(full=b["truth"][r].astype(np.int32), region=b["region"][r].astype(np.int32), own=np.flatnonzero(half[r] == MASK),
                                       chain=None if kind == "nb" else (int(b["chain"][r]), int(b["chain"][N_SEQ + r]))))
    else:
        z = np.load(f"{GOLDEN}/{TRACE[kind]}")
        n, loc = z["tokens"].shape[0], z["loc"]
        for r in range(N_SEQ):
            out.append(SimpleNamespace(full=z["final"][r % n].astype(np.int32), region=z["region"][r % n].astype(np.int32), own=np.sort(loc[len(loc) // 2:]),
                                       chain=None if kind == "nb" else (int(z["chain"][r % n]), int(z["chain"][n + r % n]))))
    for q in out:
        q.M = np.union1d(q.own, SLOTS[kind]).astype(np.int32)
        q.masked = q.full.copy()
        q.masked[q.M] = MASK
    _seqs[group, kind] = out
    return out


# ---- sessions ----------------------------------------------------------------------------------------------------------------------------
def all_picks(kind, seqs=range(N_SEQ), slots=None):
    return [(q, s, j) for q in seqs for s in (SLOTS[kind] if slots is None else slots) for j in range(N_DRAW)]


def filler_positions(B, n_fill):
    """Fillers stand BETWEEN probe rows, spread over the batch: the middle of each of n_fill equal parts."""
    pos = [int((k + 0.5) * B / n_fill) for k in range(n_fill)]
    assert len(set(pos)) == n_fill and all(0 <= p < B for p in pos)
    return pos


def session(group, kind, picks, B=None, later=False, sampling=False):
    """The arrays of one session.  A probe row (sequence q, slot s, token j) is q's full row with tokens[s] = j, order = [s, M \\ {s} ...]
    (later: [a, b, s, ...], a and b the first two own masked slots) and T = |M|; a filler is a masked row with T = 0.  sampling: the
    rows as a sampling session takes them (M masked; the copies of a probe are then the same row)."""
    seqs = sequences(group, kind)
    n = len(picks)
    B = n if B is None else B
    fill = filler_positions(B, B - n) if B > n else []
    probe_rows = [r for r in range(B) if r not in set(fill)]
    L = LENGTH[kind]
    Tmax = max(len(q.M) for q in seqs)
    tokens, region = np.zeros((B, L), np.int32), np.zeros((B, L), np.int32)
    order, T = np.zeros((B, Tmax), np.int32), np.zeros(B, np.int32)
    chain = None if kind == "nb" else np.zeros(2 * B, np.int32)
    src = np.zeros(B, np.int32)

    def put(r, q):
        src[r] = q
        region[r] = seqs[q].region
        if chain is not None:
            chain[r], chain[B + r] = seqs[q].chain

    for r, (q, s, j) in zip(probe_rows, picks):
        Q = seqs[q]
        put(r, q)
        tokens[r] = Q.masked if sampling else Q.full
        if not sampling:
            tokens[r, s] = j
        head = [int(Q.own[0]), int(Q.own[1]), s] if later else [s]
        assert s in Q.M and len(set(head)) == len(head)
        order[r, :len(Q.M)] = head + [int(x) for x in Q.M if x not in head]
        T[r] = len(Q.M)
    for k, r in enumerate(fill):
        put(r, k % len(seqs))
        tokens[r] = seqs[k % len(seqs)].masked
    return SimpleNamespace(tokens=tokens, region=region, chain=chain, order=order, T=T, Tmax=Tmax, B=B, picks=list(picks),
                           probe_rows=np.array(probe_rows, np.int64), fill=np.array(fill, np.int64), src=src, read=2 if later else 0)


def denoiser_input(s, r):
    """What the denoiser sees of row r in the forward that is read: the row with order[read : T] masked."""
    x = s.tokens[r].copy()
    x[s.order[r, s.read:s.T[r]]] = MASK
    return x


def later_context(group, kind):
    """The denoiser input of the later-step probe: M masked except the two slots visited before."""
    Q = sequences(group, kind)[LATER[kind]["seq"]]
    x = Q.masked.copy()
    x[Q.own[:2]] = Q.full[Q.own[:2]]
    return x


# ---- the oracle --------------------------------------------------------------------------------------------------------------------------
def oracle_scoring(net, tokens, region, chain, dropout=None):
    """The scoring definition: a forward of the masked rows, log-softmax over the 22 drawable tokens -> float64 [n, L, 22]."""
    return log_softmax64(net(tokens, region, chain, dropout=dropout)[:, :, :N_DRAW])


def _chain_of(seqs, idx):
    return None if seqs[0].chain is None else np.array([seqs[q].chain[0] for q in idx] + [seqs[q].chain[1] for q in idx], np.int32)


_refs = {}


def reference(group, kind):
    """Built once per (group, kind): want [N_SEQ, L, 22] = the float64 oracle's log-softmax of every sequence's masked row, later [22]
    = that of the later-step context at its slot, yard = the yard-stick (module docstring) pooled over all probes of both."""
    if (group, kind) in _refs:
        return _refs[group, kind]
    cfg, sd = weights(group, kind)
    seqs = sequences(group, kind)
    idx = list(range(N_SEQ)) + [LATER[kind]["seq"]]
    x = np.stack([q.masked for q in seqs] + [later_context(group, kind)])
    reg = np.stack([seqs[q].region for q in idx])
    lsm = {dt: oracle_scoring(ho.OracleNet(kind, cfg, sd, dtype=dt), x, reg, _chain_of(seqs, idx)) for dt in (np.float64, np.float32)}
    slots = list(SLOTS[kind])
    diff = np.abs(lsm[np.float32] - lsm[np.float64])
    yard = max(float(diff[:N_SEQ][:, slots].max()), float(diff[N_SEQ, LATER[kind]["slot"]].max()))
    ref = SimpleNamespace(want=lsm[np.float64][:N_SEQ], later=lsm[np.float64][N_SEQ, LATER[kind]["slot"]], yard=yard,
                          bound=MARGIN * yard, pair=PAIR * MARGIN * yard)
    _refs[group, kind] = ref
    return ref


def drop_picks(kind):
    return all_picks(kind, seqs=(0,), slots=DROP_SLOTS[kind])


def drop_session(kind):
    """Dropout on: the 22 copies of two slots of sequence 0 and three fillers; every row has its own global id, hence its own masks."""
    return session("prod", kind, drop_picks(kind), B=len(drop_picks(kind)) + 3)


def reference_dropout(kind):
    """want [n] = the float64 oracle under the generated masks of row row0 + r for the probe rows of `drop_session` that carry a token
    of DROP_TOKENS (rows [n], in session order); yard = the yard-stick over exactly those values."""
    if ("drop", kind) in _refs:
        return _refs["drop", kind]
    cfg, sd = weights("prod", kind, dropout=True)
    seqs = sequences("prod", kind)
    s = drop_session(kind)
    sel = [(int(r), slot, j) for r, (q, slot, j) in zip(s.probe_rows, s.picks) if j in DROP_TOKENS]
    rows = np.array([r for r, _, _ in sel])
    x = np.stack([seqs[0].masked] * len(sel))
    reg = np.stack([seqs[0].region] * len(sel))
    drop = ho.Dropout("philox", seed=DROP_KW["seed"], rows=rows + DROP_KW["row0"], step=0)
    val = {}
    for dt in (np.float64, np.float32):
        lsm = oracle_scoring(ho.OracleNet(kind, cfg, sd, dtype=dt), x, reg, _chain_of(seqs, [0] * len(sel)), dropout=drop)
        val[dt] = np.array([lsm[i, slot, j] for i, (_, slot, j) in enumerate(sel)])
    yard = float(np.abs(val[np.float32] - val[np.float64]).max())
    ref = SimpleNamespace(rows=rows, want=val[np.float64], yard=yard, bound=MARGIN * yard, pair=PAIR * MARGIN * yard)
    _refs["drop", kind] = ref
    return ref


def expected(ref, s):
    """float64 [n probe rows]: the reference of what a session's probe rows score (in the order of s.picks)."""
    if s.read:
        return np.array([ref.later[j] for _, _, j in s.picks])
    return np.array([ref.want[q, slot, j] for q, slot, j in s.picks])
