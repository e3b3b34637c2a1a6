"""What the key of a captured step graph is for (hd_api.hip StepKey): a session replays the graph of an earlier session on the same
handle only when every launch in it would be the same.

ONE handle per model kind runs a chain of sessions through the captured-graph path.  Each session differs from its predecessor in
exactly one thing the captured step depends on -- draw mode, slots per step, slot policy, guide buffers, temperature, truncation, beam
width, noise source, noise array, pruning, dropout, lane count, rows, Tmax -- so a key that misses that thing replays the predecessor's
graph.  After each session the same session runs again on the same handle with graph=False (launches issued one by one, nothing
replayed) and tokens, log-probabilities and order must be bit-equal between the two runs.  So that a comparison of nothing fails too,
at least one step of every group must also CHANGE the results against its predecessor.  The rows of a session are independent, so its
tokens do not depend on how the batch is split over lanes; what the lanes step changes is the split itself, and the number of lanes a
session ran on (from the launch tally) is therefore carried among its results.

The batch is the golden micro trace's (2 rows), every row twice -- a beam session wants whole groups of equal rows -- with the first
TMAX positions of its order; row pair 1 stops 3 positions early.  Steps marked None lead back (confident -> given, K 3 -> 1, W 2 -> 0,
score -> record) to where the next group can start; they are checked like the others and belong to no group."""
import numpy as np
import pytest

from conftest import chain_or_none, load_cfg, load_golden, load_weights
from test_gpu_guide import ROW0, SEED, _random_guide
from test_gpu_logp import _mk

pytestmark = pytest.mark.gpu

TRACE = {"ab": "micro_ab_sample_finetune.npz", "nb": "micro_nb_sample_plain.npz"}
TMAX = 12
BASE = dict(mode="sample", K=1, policy="given", guide=None, temp=1.0, trunc=None, W=0, noise=None, prune=True, dropout="off", lanes=1,
            rows=4, tmax=TMAX)
STEPS = [
    ("mode", dict(mode="record")), ("mode", dict(mode="score")), (None, dict(mode="record")),
    ("K", dict(K=3)),
    ("policy", dict(policy="confident")),
    ("guide", dict(guide="allow")), ("guide", dict(guide="allow+bias")),
    ("temperature", dict(temp=0.7)),
    ("truncation", dict(trunc=(2, 1.0, 0.0))), ("truncation", dict(trunc=(3, 1.0, 0.0))), ("truncation", dict(trunc=(0, 0.8, 0.0))),
    ("truncation", dict(trunc=(0, 1.0, 0.1))),
    (None, dict(policy="given")), (None, dict(K=1)),
    ("W", dict(W=2)), (None, dict(W=0)),
    ("noise", dict(noise="a")), ("noise", dict(noise="b")),
    ("prune", dict(prune=False)),
    ("dropout", dict(dropout="faithful")),
    ("lanes", dict(lanes=2)),
    ("rows", dict(rows=2)),
    ("Tmax", dict(tmax=TMAX - 5)),
]


@pytest.fixture(scope="module")
def hip():
    import hudiff_amd
    if hudiff_amd.device_count() < 1:
        pytest.fail("no MI355X visible: GPU tests must run on the GPU box (there is no CPU fallback)")
    return hudiff_amd


@pytest.fixture(scope="module", params=["ab", "nb"])
def micro(request, hip):
    kind = request.param
    z = load_golden(TRACE[kind])
    rep = np.repeat(np.arange(z["tokens"].shape[0]), 2)
    chain = chain_or_none(z)
    if chain is not None:
        n = len(chain) // 2
        chain = (chain[:n][rep], chain[n:][rep])
    allow, bias = _random_guide(len(rep) // 2, z["tokens"].shape[1])
    rng = np.random.default_rng(11)
    data = {"tokens": z["tokens"][rep], "final": z["final"][rep], "region": z["region"][rep], "chain": chain,
            "order": np.repeat(z["loc"][None, :TMAX], len(rep), 0).astype(np.int32), "T": np.array([TMAX, TMAX, TMAX - 3, TMAX - 3]),
            "allow": allow[rep], "bias": bias[rep],
            "q": {"a": np.ascontiguousarray(z["q"][:TMAX][:, rep]), "b": rng.exponential(1.0, (TMAX, len(rep), 22)).astype(np.float32)}}
    # a handle that can do everything in the chain: dropout in the weights' config, two lanes from 2 rows on (asked for per session)
    m = _mk(hip, kind, dict(load_cfg(kind), dropout=0.2 if kind == "ab" else 0.5), load_weights(kind), options={"lane_min_rows": 2})
    yield m, data
    m.close()


def _run(m, data, s, graph):
    """The session `s`, whole: {"tokens", "logp", "order", ...} as far as it has them, and the number of lanes it ran on."""
    from hudiff_amd import Guide, Truncation
    rows, tmax = s["rows"], s["tmax"]
    tok = np.ascontiguousarray(data["final" if s["mode"] == "score" else "tokens"][:rows])
    reg = np.ascontiguousarray(data["region"][:rows])
    chn = None if data["chain"] is None else np.concatenate([data["chain"][0][:rows], data["chain"][1][:rows]])
    order = np.ascontiguousarray(data["order"][:rows, :tmax])
    T = np.minimum(data["T"][:rows], tmax)
    guide = None if s["guide"] is None else Guide(data["allow"][:rows], data["bias"][:rows] if s["guide"] == "allow+bias" else None, s["temp"])
    trunc = None if s["trunc"] is None else Truncation(*s["trunc"])
    kw = dict(seed=SEED, row0=ROW0, dropout=s["dropout"], graph=graph, prune=s["prune"], lanes=s["lanes"], guide=guide, truncation=trunc)
    m.debug_launch_tally()                               # (cleared by the call)
    if s["W"]:
        m.beam_begin(tok, reg, chn, order, T, s["W"], **kw)
        try:
            m.sample_run(0, tmax)
        finally:
            out = {"tokens": m.sample_end()}
        out["logp"] = m.sample_logp()
        out["score"], out["parent"], out["cand"] = m.beam_state()
    elif s["mode"] == "score":
        out = {"logp": m.score(tok, reg, chn, order, T, parallel=False, slots_per_step=s["K"], slot_policy=s["policy"], **kw)}
    else:
        q = None if s["noise"] is None else np.ascontiguousarray(data["q"][s["noise"]][:tmax, :rows])
        res = m.sample(tok, reg, chn, order, T, q_noise=q, return_logp=s["mode"] == "record", slots_per_step=s["K"],
                       slot_policy=s["policy"], **kw)
        out = {"tokens": res[0], "logp": res[1]} if s["mode"] == "record" else {"tokens": res}
    out["order"] = m.sample_order(rows, tmax)
    tally = m.debug_launch_tally()
    out["lanes"] = np.array([n for n in (1, 2, 3, 4) if tally[f"sample_lanes_{n}"] > 0])
    return out


def _bit_equal(a, b):
    return a.keys() == b.keys() and all(a[k].shape == b[k].shape and a[k].tobytes() == b[k].tobytes() for k in a)


def _changed(a, b):
    """Something both sessions have differs."""
    return any(a[k].shape != b[k].shape or a[k].tobytes() != b[k].tobytes() for k in a.keys() & b.keys())


def test_every_key_field_recaptures_the_step(micro):
    m, data = micro
    s = dict(BASE)
    prev = _run(m, data, s, True)
    assert _bit_equal(prev, _run(m, data, s, False)), ("base", s)
    changed = {}
    for group, delta in STEPS:
        assert len(delta) == 1 and all(s[k] != v for k, v in delta.items()), (group, delta)       # (the chain itself: one thing per step)
        s.update(delta)
        got = _run(m, data, s, True)                                 # whatever graph the predecessor left is still there
        eager = _run(m, data, s, False)
        ch = _changed(prev, got)
        print(f"[session_key] {group or '(back)':12s} {delta}  changed vs predecessor: {ch}")
        for k in got:
            assert k in eager and got[k].shape == eager[k].shape and got[k].tobytes() == eager[k].tobytes(), \
                (group, delta, k, "the graph run differs from the eager run of the same session")
        if group is not None:
            changed[group] = changed.get(group, False) or ch
        prev = got
    assert all(changed.values()), ("no step of these groups changed the results, so comparing them proved nothing",
                                   [g for g, c in changed.items() if not c])
