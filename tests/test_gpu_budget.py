"""The mutation budget on the GPU (hd_set_budget; include/hudiff_hip.h "mutation budget"): the device caps each row's changes from its
origin, inside the captured step.

The numbering follows the definition's checks: 1 neutrality, 2 M = 0, 3 exactly known logits (tests/budget_cases.py; decided on the CPU
by tests/test_budget_host.py, so no near-tie exemption), 4 replay against an unbudgeted guided session, 5 the beam, 6 launch forms,
7 stale graphs, 8 statuses, 9 production width, 10 the CLIs.  Micro models, B <= 8, T <= 8, W <= 9, lane_min_rows = 2 so that two lanes
really split the batch.  Tolerances are the siblings': draw_cases.logp_bound against the float64 definition, REF_TOL / PAIR_TOL of
tests/test_gpu_logp.py; everything else is compared bit for bit."""
import ctypes as C

import numpy as np
import pytest

import budget_cases as BC
import draw_cases as DC
from conftest import load_cfg, load_weights, prec
from hudiff_amd.guide import FREE
from test_gpu_beam import _check_selection, _groups, _replicate
from test_gpu_guide import ALL, _random_guide
from test_gpu_logp import PAIR_TOL, _ab_checkpoint, _load_prod, _mk, _nb_checkpoint, _ragged

pytestmark = pytest.mark.gpu

B8, TCAP = 8, 6


@pytest.fixture(scope="module")
def hip():
    import hudiff_amd
    if hudiff_amd.device_count() < 1:
        pytest.fail("no MI355X visible: GPU tests must run on the GPU box (there is no CPU fallback)")
    return hudiff_amd


@pytest.fixture(scope="module", params=["ab", "nb"])
def micro(request, hip):
    kind = request.param
    cfg, sd = load_cfg(kind), load_weights(kind)
    models = {"kind": kind, "m0": _mk(hip, kind, cfg, sd, options={"lane_min_rows": 2}),
              "m1": _mk(hip, kind, dict(cfg, dropout=0.2 if kind == "ab" else 0.5), sd, options={"lane_min_rows": 2})}
    yield models
    models["m0"].close(); models["m1"].close()


@pytest.fixture(scope="module")
def exact(hip):
    cache = {}

    def get(kind):
        if kind not in cache:
            cache[kind] = _mk(hip, kind, load_cfg(kind), DC.decoder_state(load_weights(kind), "main"), options={"lane_min_rows": 2})
        return cache[kind]
    yield get
    for m in cache.values():
        m.close()


# ---- helpers ---------------------------------------------------------------------------------------------------------------------------
_data = {}


def _rows(kind):
    """Eight ragged rows (T = 0 and T = 3 among them), a random guide that allows every origin, the origin = the rows' own residues
    with every fifth visited slot free."""
    if kind not in _data:
        batch, order, T = _ragged(kind, B8, 33, TCAP)
        T = T.copy()
        T[5], T[3] = 0, 3
        L = batch["tokens"].shape[1]
        origin = np.where(batch["truth"] <= 21, batch["truth"], FREE).astype(np.int32)
        for b in range(B8):
            assert len(set(order[b, :T[b]].tolist())) == T[b]
            origin[b, order[b, 4::5]] = FREE
        allow, bias = _random_guide(B8, L)
        allow = (allow | np.where(origin <= 21, np.uint32(1) << origin.astype(np.uint32), 0)).astype(np.uint32)
        _data[kind] = dict(args=(batch["tokens"], batch["region"], batch["chain"], order, T), order=order, T=T, L=L, origin=origin,
                           allow=allow, bias=bias, live=np.arange(TCAP)[None, :] < T[:, None])
    return _data[kind]


def _bits(x):
    return np.ascontiguousarray(x, np.float32).view(np.int32)


def _same(a, b):
    if isinstance(a, (tuple, list)):
        return len(a) == len(b) and all(_same(x, y) for x, y in zip(a, b))
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and (np.array_equal(_bits(a), _bits(b)) if a.dtype == np.float32 else np.array_equal(a, b))


def _written(tok, order):
    return np.take_along_axis(tok, order, axis=1)


def _budget(d, M):
    from hudiff_amd import Budget
    return Budget(d["origin"], np.broadcast_to(np.asarray(M, np.int32), (B8,)).copy())


def _record(m, d, budget=None, guide=None, **kw):
    """One recording session -> (tokens, logp, order, mutation_count | None)."""
    kw = dict(dict(seed=11, row0=3, dropout="off"), **kw)
    tok, lp = m.sample(*d["args"], return_logp=True, guide=guide, budget=budget, **kw)
    return tok, lp, m.sample_order(), (m.mutation_count() if budget is not None else None)


# ---- 1. neutral ------------------------------------------------------------------------------------------------------------------------
FAMILIES = ["sample", "record", "score", "greedy", "guided_bias", "truncated", "confident", "beam", "dropout"]


@pytest.mark.parametrize("family", FAMILIES)
def test_neutral(micro, family):
    """max_mutations = T[b]: no row can become exhausted, and every family is the same call without a budget, float bits included."""
    from hudiff_amd import Guide, Truncation
    d = _rows(micro["kind"])
    m = micro["m1"] if family == "dropout" else micro["m0"]
    bud = _budget(d, d["T"])
    kw = dict(seed=11, row0=3, dropout="faithful" if family == "dropout" else "off")

    def run(budget):
        if family == "sample":
            return (m.sample(*d["args"], budget=budget, **kw),)
        if family in ("record", "dropout"):
            return m.sample(*d["args"], return_logp=True, budget=budget, **kw)
        if family == "score":
            full = np.where(d["args"][0] == 22, d["origin"] % 20, d["args"][0]).astype(np.int32)
            return (m.score(full, *d["args"][1:], parallel=False, budget=budget),)
        if family == "greedy":
            return m.sample(*d["args"], return_logp=True, guide=Guide(d["allow"], None, 0.0), budget=budget, **kw)
        if family == "guided_bias":
            return m.sample(*d["args"], return_logp=True, guide=Guide(d["allow"], d["bias"], 0.7), budget=budget, **kw)
        if family == "truncated":
            return m.sample(*d["args"], return_logp=True, truncation=Truncation(top_k=5, top_p=0.9), budget=budget, **kw)
        if family == "confident":
            res = m.sample(*d["args"], return_logp=True, slot_policy="confident", guide=Guide(d["allow"], d["bias"]), budget=budget, **kw)
            return res + (m.sample_order(),)
        g = _groups(micro["kind"])
        from hudiff_amd import Budget
        b3 = None if budget is None else Budget(np.where(g[0] == 22, 3, g[0]), g[4])
        return m.beam_search(*g, 3, budget=b3)
    with_budget = run(bud)
    if family != "beam":
        assert (m.mutation_count() <= d["T"]).all()
    assert _same(with_budget, run(None)), family


# ---- 2. M = 0 --------------------------------------------------------------------------------------------------------------------------
def test_budget_zero(micro):
    m, d = micro["m0"], _rows(micro["kind"])
    tok, lp, _, n = _record(m, d, _budget(d, 0))
    order, T, origin, live = d["order"], d["T"], d["origin"], d["live"]
    o = np.take_along_axis(origin, order, axis=1)
    w = _written(tok, order)
    bearing, free = live & (o <= 21), live & (o == FREE)
    assert bearing.sum() > 20 and free.sum() >= 5
    assert np.array_equal(w[bearing], o[bearing]) and (n == 0).all()
    assert (_bits(lp)[bearing] == 0).all()                                   # +0.0, bit for bit
    assert (w[free] <= 21).all() and (lp[free] < 0).all() and np.isfinite(lp[free]).all()      # free slots still draw
    base = m.sample(*d["args"], seed=11, row0=3, dropout="off")
    assert not np.array_equal(base, tok)                                     # (the unbudgeted session is far from its origin)
    # scoring the origin gives 0 there; any other target gives -inf there and is counted
    full = tok.copy()
    sc = m.score(full, *d["args"][1:], parallel=False, budget=_budget(d, 0))
    assert (m.mutation_count() == 0).all() and (_bits(sc)[bearing] == 0).all() and _same(sc, lp)
    other = full.copy()
    rows = np.flatnonzero(bearing.any(1))
    hit = np.zeros_like(bearing)
    for b in rows:
        t = int(np.flatnonzero(bearing[b])[-1])
        other[b, order[b, t]] = (o[b, t] + 1) % 20
        hit[b, t] = True
    sc2 = m.score(other, *d["args"][1:], parallel=False, budget=_budget(d, 0))
    assert np.isneginf(sc2[hit]).all() and (_bits(sc2)[bearing & ~hit] == 0).all() and not np.isnan(sc2).any()
    assert np.array_equal(m.mutation_count(), hit.sum(1))


# ---- 3. exactly known logits -----------------------------------------------------------------------------------------------------------
def _exact_session(m, bc, b, mode, lanes=2, graph=True, budget=True):
    from hudiff_amd import Budget, Guide
    case = bc.case
    kw = dict(dropout="off", guide=Guide(b.allow, b.bias, case.temperature), truncation=case.truncation, slot_policy=case.policy,
              prune=case.prune, lanes=lanes, graph=graph, budget=Budget(b.origin, b.M) if budget else None)
    args = (b.region, b.chain, b.order, b.T)
    if mode == "score":
        tok, lp = None, m.score(b.full, *args, parallel=False, **kw)
    elif mode == "record":
        tok, lp = m.sample(b.tokens, *args, q_noise=b.q, return_logp=True, **kw)
    else:
        tok, lp = m.sample(b.tokens, *args, q_noise=b.q, **kw), None
    return tok, lp, m.sample_order(), (m.mutation_count() if budget else None)


def _check_exact(bc, b, mode, got, x, perms):
    tok, lp, order, n = got
    want_order, want_tok = b.order.copy(), (b.full if mode == "score" else b.tokens).copy()
    ref = np.zeros((b.B, b.Tmax))
    for r in range(b.B):
        for t, (e, (j, v)) in enumerate(zip(perms[r], x.draws[r])):
            want_order[r, t] = b.order[r, e]
            want_tok[r, want_order[r, t]] = j
            ref[r, t] = v
    assert np.array_equal(order, want_order), (bc.name, mode, order, want_order)
    if tok is not None:
        assert np.array_equal(tok, want_tok), (bc.name, mode, np.argwhere(tok != want_tok))
    assert n.tolist() == x.n, (bc.name, mode, n, x.n)
    if lp is not None:
        live = np.arange(b.Tmax)[None, :] < b.T[:, None]
        assert (lp[~live] == 0).all() and not np.isnan(lp).any() and not np.isposinf(lp).any()
        assert np.array_equal(np.isneginf(lp), np.isneginf(ref)), (bc.name, mode, lp, ref)
        for r in range(b.B):
            for t, ex in enumerate(x.exhausted[r]):
                if ex and np.isfinite(ref[r, t]):
                    assert _bits(lp)[r, t] == 0, (bc.name, mode, r, t, lp[r, t])         # +0.0 exactly
        fin = live & np.isfinite(ref)
        err, bound = np.abs(lp[fin].astype(np.float64) - ref[fin]), DC.logp_bound(ref[fin])
        print(f"{bc.name} {mode}: worst |logp - float64| {err.max():.2e}, worst error / bound {(err / bound).max():.3f}")
        assert (err <= bound).all(), (bc.name, mode, float(err.max()))


@pytest.mark.parametrize("name", [c.name for c in BC.cases()])
def test_exact_logits(exact, name):
    bc = BC.case(name)
    m, b = exact("ab"), BC.batch(bc, "ab")
    for mode in bc.case.modes:
        if bc.case.family == "confident":
            x = BC.expect_confident(bc, mode)
            perms = x.perms
        else:
            x, perms = BC.expect_draws(bc, mode), [list(range(len(r))) for r in bc.case.rows]
        _check_exact(bc, b, mode, _exact_session(m, bc, b, mode), x, perms)
    # the same sessions without the budget do something else: the case can fail
    mode = "record"
    plain = _exact_session(m, bc, b, mode, budget=False)
    with_b = _exact_session(m, bc, b, mode)
    assert not np.array_equal(plain[0], with_b[0])
    if bc.case.family == "confident":
        assert not np.array_equal(plain[2], with_b[2])                       # the exhausted row's origin-bearing slots came first


def test_exact_logits_nanobody(exact):
    for name in ("budget_draw", "budget_confident"):
        bc = BC.case(name)
        m, b = exact("nb"), BC.batch(bc, "nb")
        for mode in bc.case.modes:
            if bc.case.family == "confident":
                x = BC.expect_confident(bc, mode)
                perms = x.perms
            else:
                x, perms = BC.expect_draws(bc, mode), [list(range(len(r))) for r in bc.case.rows]
            _check_exact(bc, b, mode, _exact_session(m, bc, b, mode), x, perms)


# ---- 4. replay -------------------------------------------------------------------------------------------------------------------------
def _replay(m, d, M, dropout, **kw):
    """A budgeted recording session, budget_walk on its tokens, then the unbudgeted guided session whose allowed word at every exhausted
    position is 1 << o, and hd_score of the tokens under the budget: all bit for bit."""
    from hudiff_amd import Guide, budget_walk
    order, T, origin = d["order"], d["T"], d["origin"]
    bud = _budget(d, M)
    kw = dict(kw, dropout=dropout)
    tok, lp, _, n = _record(m, d, bud, Guide(d["allow"], d["bias"]), **kw)
    ex, n_walk = budget_walk(_written(tok, order), origin, order, T, bud.max_mutations)
    assert np.array_equal(n, n_walk) and (n <= bud.max_mutations).all()
    allow2 = d["allow"].copy()
    for b, t in zip(*np.nonzero(ex)):
        allow2[b, order[b, t]] = np.uint32(1) << np.uint32(origin[b, order[b, t]])
    tok2, lp2, _, _ = _record(m, d, None, Guide(allow2, d["bias"]), **kw)
    assert np.array_equal(tok2, tok) and _same(lp2, lp)
    o = np.take_along_axis(origin, order, axis=1)
    assert np.array_equal(_written(tok, order)[ex], o[ex]) and (_bits(lp)[ex] == 0).all()
    sc = m.score(tok, *d["args"][1:], parallel=False, guide=Guide(d["allow"], d["bias"]), budget=bud, dropout=dropout,
                 seed=kw.get("seed", 11), row0=kw.get("row0", 3))
    assert _same(sc, lp) and np.array_equal(m.mutation_count(), n)
    return tok, ex, n


def test_replay(micro):
    d = _rows(micro["kind"])
    q = np.random.default_rng(4).exponential(1.0, (TCAP, B8, 22)).astype(np.float32)
    tok, ex, n = _replay(micro["m0"], d, 2, "off", q_noise=q)
    assert ex.sum() >= 8 and (n == 2).sum() >= 4                             # rows really run out of budget
    free = _record(micro["m0"], d, None, None, q_noise=q)[0]
    assert not np.array_equal(free, tok)
    tok, ex, n = _replay(micro["m1"], d, np.array([2, 1, 0, 3, 2, 1, 2, 6]), "faithful", seed=21, row0=40)
    assert ex.sum() >= 8


# ---- 5. the beam -----------------------------------------------------------------------------------------------------------------------
def _snap(m):
    score, parent, cand = m.beam_state()
    return {"tok": m.sample_tokens(), "score": score, "parent": parent, "lp": m.sample_logp(), "cand": cand, "n": m.mutation_count()}


def _drive(m, groups, W, origin, M, guide=None, **kw):
    from hudiff_amd import Budget
    tokens, region, chain, order, T = groups
    rep = np.repeat(np.arange(tokens.shape[0]), W)
    m.beam_begin(*_replicate(tokens, region, chain, order, T, W), W, guide=None if guide is None else guide.take(rep),
                 budget=Budget(origin[rep], np.asarray(M, np.int32)[rep]), **kw)
    steps, before = [], _snap(m)
    for t in range(order.shape[1]):
        m.sample_run(t, t + 1)
        after = _snap(m)
        steps.append((before, after))
        before = after
    return steps, m.sample_end()


@pytest.mark.parametrize("lanes", [1, 2])
@pytest.mark.parametrize("W", [3, 9])
def test_beam_position_by_position(micro, W, lanes):
    from hudiff_amd.guide import beam_select
    m, groups = micro["m0"], _groups(micro["kind"])
    tokens, region, chain, order, T = groups
    G = tokens.shape[0]
    rng = np.random.default_rng(2)
    origin = rng.integers(0, 20, tokens.shape).astype(np.int32)
    origin[0, order[0, 2]] = FREE
    M = [1, 0, 2]
    steps, final = _drive(m, groups, W, origin, M, lanes=lanes)
    assert _check_selection(groups, W, steps, final) == 6                     # selection, gather, score, parent: beam_select, bit for bit
    assert not steps[0][0]["n"].any()
    masked = 0
    for t, (b, a) in enumerate(steps):
        for g in range(G):
            r = np.arange(g * W, (g + 1) * W)
            if t >= T[g]:
                assert np.array_equal(a["n"][r], b["n"][r])
                continue
            o = int(origin[g, order[g, t]])
            livew = np.isfinite(b["score"][r])
            exh = livew & (b["n"][r] >= M[g]) & (o <= 21)
            gone = np.isneginf(a["cand"][r])
            want = np.zeros((W, 22), bool)
            want[~livew] = True
            want[exh] = True
            if o <= 21:
                want[exh, o] = False
            assert np.array_equal(gone, want) and not np.isnan(a["cand"][r]).any(), (t, g)
            masked += int(exh.sum())
            w, j, _ = beam_select(a["cand"][r], W)
            assert np.array_equal(a["n"][r], b["n"][r][w] + ((j != o) & (o <= 21))), (t, g)
            assert (a["n"][r][np.isfinite(a["score"][r])] <= M[g]).all()
    assert masked >= 4
    # the final rows differ from the origin in at most M visited slots
    for g in range(G):
        for r in range(g * W, (g + 1) * W):
            if np.isfinite(steps[-1][1]["score"][r]):
                s = order[g, :T[g]]
                s = s[origin[g, s] <= 21]
                assert (final[r, s] != origin[g, s]).sum() == steps[-1][1]["n"][r] <= M[g]


def test_beam_enumeration(micro):
    """3 positions x 3 allowed residues that include the origin, M = 1, W = 9: exactly the 7 sequences with at most one mutation are
    live, in score order; rows 8 and 9 are dead; every live score is the unbudgeted model.score of its row.  A second group has another
    M and T = 0."""
    from hudiff_amd import Budget, Guide
    kind, m = micro["kind"], micro["m0"]
    tokens, region, chain, order, _ = _groups(kind)
    tokens, region, order = tokens[:2], region[:2], np.ascontiguousarray(order[:2, :3])
    chain = None if chain is None else np.array([chain[0], chain[1], chain[3], chain[4]], np.int32)
    T = np.array([3, 0], np.int32)
    L = tokens.shape[1]
    sets = ([2, 7, 19], [0, 7, 11], [4, 9, 16])
    org = [7, 0, 16]
    allow = np.full((2, L), ALL, np.uint32)
    origin = np.full((2, L), FREE, np.int32)
    for s, ok, o in zip(order[0], sets, org):
        allow[0, s] = sum(1 << j for j in ok)
        origin[0, s] = o
    guide, bud = Guide(allow), Budget(origin, [1, 2])
    tok, score, logp, live = m.beam_search(tokens, region, chain, order, T, 9, guide=guide, budget=bud)
    assert live[0].tolist() == [True] * 7 + [False] * 2 and live[1].tolist() == [True] + [False] * 8
    assert (np.diff(score[0, :7]) <= 0).all() and np.isneginf(score[0, 7:]).all() and score[1, 0] == 0
    got = {tuple(int(r[s]) for s in order[0]) for r in tok[0, :7]}
    want = {(a, b, c) for a in sets[0] for b in sets[1] for c in sets[2] if (a != org[0]) + (b != org[1]) + (c != org[2]) <= 1}
    assert len(want) == 7 and got == want
    assert np.array_equal(tok[1, 0], tokens[1])
    ch7 = None if chain is None else np.array([chain[0]] * 7 + [chain[2]] * 7, np.int32)
    ref = m.score(tok[0, :7], np.repeat(region[:1], 7, 0), ch7, np.repeat(order[:1], 7, 0), np.full(7, 3), guide=Guide(allow[0]), parallel=False)
    err = float(np.abs(ref.astype(np.float64).sum(1) - score[0, :7]).max())
    print(f"{kind}: |budgeted beam score - unbudgeted model.score| over the 7 sequences {err:.2e}")
    assert err < 2 * PAIR_TOL                                                # lp[b, o] is not renormalised
    # without the budget all nine rows are live
    assert m.beam_search(tokens, region, chain, order, T, 9, guide=guide)[3][0].all()


# ---- 6. launch forms -------------------------------------------------------------------------------------------------------------------
def test_forms_are_bit_identical(micro):
    from hudiff_amd import Guide
    m, d = micro["m0"], _rows(micro["kind"])
    guide, bud = Guide(d["allow"], d["bias"]), _budget(d, 2)
    base = _record(m, d, bud, guide, lanes=1)
    assert (base[3] == 2).sum() >= 4
    for kw in (dict(lanes=2), dict(lanes=1, graph=False), dict(lanes=2, graph=False), dict(lanes=2, graph="loop")):
        assert _same(_record(m, d, bud, guide, **kw), base), kw
    # the session interface: the count as it goes, a restart starts from 0 again, ranges of positions in pieces
    m.sample_begin(*d["args"], seed=5, row0=3, dropout="off", record_logp=True, guide=guide, budget=bud)
    assert not m.mutation_count().any()
    m.sample_run(0, 3)
    mid = m.mutation_count()
    assert mid.any() and (mid <= 2).all()
    m.sample_restart(11)
    assert not m.mutation_count().any()
    m.sample_run(0, 1); m.sample_run(1, TCAP)
    n, lp, order = m.mutation_count(), m.sample_logp(), m.sample_order()
    assert _same((m.sample_end(), lp, order, n), base)
    assert np.array_equal(m.mutation_count(), base[3])                        # legal after the end, like sample_logp


def test_lnsync_guard_repeats_a_budgeted_session(hip):
    """Production width (the micro models' launches hold no ln_sync meeting).  The repeat is a budgeted session from n = 0 on the kernels
    the handle keeps from then on: it is bit for bit the session the handle runs next, mutation_count included."""
    from hudiff_amd import Budget, evalsets as E, synthetic as S
    cfg = dict(S.AB_CONFIG, dropout=0.0)
    mx = _mk(hip, "ab", cfg, S.random_state_dict("ab", cfg, seed=0), precision="split", options={"lane_min_rows": 2})
    try:
        big = E.eval_batch("huab348", B8, row0=0)
        T = np.minimum(big["T"], 4)
        args = (big["tokens"], big["region"], big["chain"], np.ascontiguousarray(big["order"][:, :4]), T)
        bud = Budget(np.where(big["truth"] <= 21, big["truth"], FREE), np.full(B8, 2))
        kw = dict(seed=13, row0=0, return_logp=True, budget=bud)

        def run():
            tok, lp = mx.sample(*args, **kw)
            return tok, lp, mx.mutation_count()
        want = run()
        prec(mx, lnsync_in_use=True, lnsync_fallbacks=0, last_call_repeated=False)
        mx.debug_fail_next_lnsync()
        with pytest.warns(RuntimeWarning, match="ln_sync"):
            again = run()
        prec(mx, lnsync_in_use=False, lnsync_fallbacks=1, last_call_repeated=True)
        after = run()
        prec(mx, lnsync_fallbacks=1, last_call_repeated=False)
        assert _same(again, after) and (again[2] <= 2).all() and (again[2] == 2).any()
        agree = (again[0] == want[0]).all(axis=1)
        print(f"ln_sync guard in a budgeted session: {int(agree.sum())} of {B8} rows draw the undisturbed tokens")
    finally:
        mx.close()


# ---- 7. stale graphs -------------------------------------------------------------------------------------------------------------------
def test_no_stale_graph(micro):
    """One handle, three sessions of one shape: budgeted, unbudgeted (the same guide), budgeted with another origin buffer and budget.
    Each equals its own eager run."""
    from hudiff_amd import Budget, Guide
    m, d = micro["m0"], _rows(micro["kind"])
    guide = Guide(d["allow"], d["bias"])
    other = np.where(d["origin"] <= 21, (d["origin"] + 1) % 20, FREE).astype(np.int32)
    other = np.where(((d["allow"] >> other.clip(0, 21).astype(np.uint32)) & 1).astype(bool), other, FREE).astype(np.int32)
    buds = [_budget(d, 2), None, Budget(other, np.full(B8, 1))]
    graphs = [_record(m, d, b, guide) for b in buds]
    eager = [_record(m, d, b, guide, graph=False) for b in buds]
    for g, e in zip(graphs, eager):
        assert _same(g[:3], e[:3]) and (g[3] is None or np.array_equal(g[3], e[3]))
    assert not np.array_equal(graphs[0][0], graphs[1][0]) and not np.array_equal(graphs[0][0], graphs[2][0])
    assert (graphs[2][3] <= 1).all()


# ---- 8. statuses -----------------------------------------------------------------------------------------------------------------------
def test_lifetime_and_errors(micro):
    from hudiff_amd import Budget, Guide, Truncation
    from hudiff_amd import _lib as L
    from hudiff_amd._lib import HD_ERR_INVALID, HD_ERR_STATE, HD_ERR_UNSUPPORTED, HudiffError
    kind, m, d = micro["kind"], micro["m0"], _rows(micro["kind"])
    args, origin, order, T = d["args"], d["origin"], d["order"], d["T"]
    kw = dict(seed=11, row0=3, dropout="off")

    def raises(status, fn, *a, **k):
        with pytest.raises(HudiffError) as e:
            fn(*a, **k)
        assert e.value.status == status, (e.value.status, status, str(e.value))
    plain = m.sample(*args, **kw)
    want = m.sample(*args, budget=_budget(d, 1), **kw)
    n1 = m.mutation_count()
    assert (n1 <= 1).all() and not np.array_equal(plain, want)

    def ordinary():
        assert np.array_equal(m.sample(*args, **kw), plain)
        raises(HD_ERR_STATE, m.mutation_count)                               # a session without a budget
    ordinary()                                                               # one-shot
    # hd_set_budget's own refusals
    o32, m32 = np.ascontiguousarray(origin), np.full(B8, 1, np.int32)
    for bad in (L.HdBudget(0, L.ptr(o32, C.c_int32), L.ptr(m32, C.c_int32)), L.HdBudget(-1, L.ptr(o32, C.c_int32), L.ptr(m32, C.c_int32)),
                L.HdBudget(B8, None, L.ptr(m32, C.c_int32)), L.HdBudget(B8, L.ptr(o32, C.c_int32), None)):
        assert m._lib.hd_set_budget(m._h, C.byref(bad)) == HD_ERR_INVALID
    ordinary()
    # inside an open session
    m.sample_begin(*args, budget=_budget(d, 1), **kw)
    raises(HD_ERR_STATE, m.set_budget, _budget(d, 1))
    raises(HD_ERR_STATE, m.set_budget, None)
    m.sample_run(0, TCAP)
    assert np.array_equal(m.mutation_count(), n1)                            # inside the session: it synchronises
    assert np.array_equal(m.sample_end(), want) and np.array_equal(m.mutation_count(), n1)
    # NULL clears; hd_forward neither uses nor clears, but ends the read-out
    m.set_budget(_budget(d, 1)); m.set_budget(None)
    ordinary()
    m.set_budget(_budget(d, 1))
    one = (args[0][:1], args[1][:1], None if args[2] is None else np.array([args[2][0], args[2][B8]]))
    m(*one)
    assert np.array_equal(m.sample(*args, **kw), want) and np.array_equal(m.mutation_count(), n1)
    m(*one)
    raises(HD_ERR_STATE, m.mutation_count)
    # the begin's refusals, each consuming the budget
    m.set_budget(Budget(origin[:4], np.ones(4, np.int32)))                   # B differs
    raises(HD_ERR_INVALID, m.sample, *args, **kw)
    ordinary()
    b, t = int(np.flatnonzero(T > 1)[0]), 1
    for v in (23, -1):                                                       # a visited origin outside [0, 22]
        bad = origin.copy()
        bad[b, order[b, t]] = v
        raises(HD_ERR_INVALID, m.sample, *args, budget=Budget(bad, 1), **kw)
        ordinary()
    ok = origin.copy()                                                       # a slot that is not visited is neither checked nor read
    unvisited = np.ones(origin.shape, bool)
    for r in range(B8):
        unvisited[r, order[r, :T[r]]] = False
    ok[unvisited] = 99
    assert np.array_equal(m.sample(*args, budget=Budget(ok, 1), **kw), want)
    neg = _budget(d, 1)
    neg.max_mutations = np.array([1, 1, -1, 1, 1, 1, 1, 1], np.int32)        # (past the Python check)
    raises(HD_ERR_INVALID, m.sample, *args, budget=neg, **kw)
    ordinary()
    allow = d["allow"].copy()                                                # guided: the origin of a visited slot is not allowed there
    s = order[b, t]
    assert origin[b, s] <= 21
    allow[b, s] &= ~(np.uint32(1) << np.uint32(origin[b, s]))
    raises(HD_ERR_INVALID, m.sample, *args, guide=Guide(allow), budget=_budget(d, 1), **kw)
    ordinary()
    free = origin.copy()
    free[b, s] = FREE                                                        # ... a free slot needs no allowed origin
    m.sample(*args, guide=Guide(allow), budget=Budget(free, 1), **kw)
    raises(HD_ERR_UNSUPPORTED, m.sample, *args, budget=_budget(d, 1), slots_per_step=2, **kw)
    ordinary()
    full = np.where(args[0] == 22, origin % 20, args[0]).astype(np.int32)
    raises(HD_ERR_UNSUPPORTED, m.score, full, *args[1:], parallel=False, budget=_budget(d, 1), slots_per_step=2)
    with pytest.raises(ValueError):
        m.score(full, *args[1:], parallel=True, budget=_budget(d, 1))
    # beam
    g = _groups(kind)
    W = 2
    rows = _replicate(*g, W)
    rep = np.repeat(np.arange(3), W)
    gorg = np.where(g[0] == 22, 5, g[0]).astype(np.int32)[rep]
    gM = np.array([1, 1, 2, 2, 0, 0], np.int32)
    m.beam_begin(*rows, W, budget=Budget(gorg, gM))
    m.sample_run(0, 4)
    m.sample_end()
    alive = np.isfinite(m.beam_state()[0])
    assert alive.any() and (m.mutation_count()[alive] <= gM[alive]).all()        # (a dead row's count means nothing)
    badM = gM.copy()
    badM[1] = 2
    raises(HD_ERR_INVALID, m.beam_begin, *rows, W, budget=Budget(gorg, badM))                    # max_mutations differs inside a group
    ordinary()
    bado = gorg.copy()
    bado[1, g[3][0, 1]] = (bado[1, g[3][0, 1]] + 1) % 20
    raises(HD_ERR_INVALID, m.beam_begin, *rows, W, budget=Budget(bado, gM))                      # a visited origin differs
    ordinary()
    oko = gorg.copy()
    oko[5, :] = 7                                                            # (group 2 has T = 0: nothing of it is visited)
    m.beam_begin(*rows, W, budget=Budget(oko, gM))
    m.sample_end()
    raises(HD_ERR_UNSUPPORTED, m.beam_begin, *rows, W, budget=Budget(gorg, gM), truncation=Truncation(top_k=5))
    ordinary()
    assert np.array_equal(m.sample(*args, budget=_budget(d, 1), **kw), want)


# ---- 9. production width ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("route", ["split", "f32_all"])
def test_production_width(hip, route):
    from hudiff_amd import Budget, Guide, budget_walk
    z, cfg, sd = _load_prod("ab")
    m = _mk(hip, "ab", cfg, sd, precision=route, options={"lane_min_rows": 2})
    try:
        n_all, Tn, M = z["tokens"].shape[0], 6, 2
        idx = np.arange(B8) % n_all                      # the fixture's rows, cycled; every row visits another stretch of its order
        assert (z["T"] >= B8 * Tn).all()
        chain = np.concatenate([z["chain"][:n_all][idx], z["chain"][n_all:][idx]])
        order = np.ascontiguousarray(np.stack([z["order"][i, b * Tn:(b + 1) * Tn] for b, i in enumerate(idx)]), np.int32)
        T = np.full(B8, Tn, np.int32)
        args = (z["tokens"][idx], z["region"][idx], chain, order, T)
        origin = np.where(z["final"][idx] <= 21, z["final"][idx], FREE).astype(np.int32)
        origin[np.arange(B8), order[:, 3]] = (origin[np.arange(B8), order[:, 3]] + 1) % 20
        bud = Budget(origin, np.full(B8, M))
        kw = dict(seed=9, row0=0, dropout="off", return_logp=True)
        tok, lp = m.sample(*args, budget=bud, **kw)
        n = m.mutation_count()
        ex, n_walk = budget_walk(_written(tok, order), origin, order, T, bud.max_mutations)
        assert np.array_equal(n, n_walk) and (n <= M).all()
        allow = np.full(origin.shape, ALL, np.uint32)
        for b, t in zip(*np.nonzero(ex)):
            allow[b, order[b, t]] = np.uint32(1) << np.uint32(origin[b, order[b, t]])
        tok2, lp2 = m.sample(*args, guide=Guide(allow), **kw)
        assert np.array_equal(tok2, tok) and _same(lp2, lp) and (_bits(lp)[ex] == 0).all()
        sc = m.score(tok, *args[1:], parallel=False, budget=bud, seed=9, row0=0)
        assert _same(sc, lp)
        free, _ = m.sample(*args, **kw)
        print(f"ab production width, route {route}: {int(ex.sum())} exhausted positions, counts {n.tolist()}; "
              f"{int((free != tok).any(1).sum())} of {B8} rows differ from the unbudgeted session")
        assert ex.sum() >= 1
    finally:
        m.close()


# ---- 10. CLIs --------------------------------------------------------------------------------------------------------------------------
def _cli_args(cli, tmp_path, tag):
    """The command line of one run of a sampler (its checkpoint under a directory of its own: the log-dir name has one-second
    resolution)."""
    from test_gpu_cli import _pdb_fasta, _write_inputs
    root = tmp_path / tag
    root.mkdir()
    if cli == "sample":
        csv, nb = _write_inputs(root, "ab", 2)
        ck = root / "run" / "checkpoints" / "hudiffab.pt"
        _ab_checkpoint(ck)
        return ["--ckpt", str(ck), "--data_fpath", str(csv), "--numbered_fpath", str(nb), "--batch_size", "3", "--seed", "5"]
    if cli == "nanosample":
        csv, nb = _write_inputs(root, "nb", 2)
        ck = root / "run" / "checkpoints" / "hudiffnb.pt"
        _nb_checkpoint(ck)
        return ["--ckpt", str(ck), "--data_fpath", str(csv), "--numbered_fpath", str(nb), "--model", "finetune_vh", "--try_number", "2",
                "--seed", "5"]
    fa = root / "7zzz.fasta"
    _pdb_fasta(fa)
    if cli == "sample_for_anti_cdr":
        ck = root / "hudiffab.pt"
        _ab_checkpoint(ck)
        return ["--ckpt", str(ck), "--anti_complex_fasta", str(fa), "--log_dirpath", str(root / "logs"), "--batch_size", "3",
                "--sample_number", "3", "--numbering", "builtin"]
    ck = root / "hudiffnb.pt"
    _nb_checkpoint(ck)
    return ["--ckpt", str(ck), "--nano_complex_fasta", str(fa), "--batch_size", "3", "--sample_number", "3", "--numbering", "builtin"]


@pytest.mark.parametrize("cli", ["sample", "nanosample", "sample_for_anti_cdr", "sample_for_nano_cdr"])
def test_cli_max_mutations(hip, tmp_path, monkeypatch, cli):
    """--max_mutations 3, also with --beam 4: every row the sampler returns differs from its input in at most 3 sampled positions (so
    does every sequence written); --max_mutations 999 writes the CSV of the run without the flag, byte for byte."""
    import importlib
    from hudiff_amd import sampler
    mod = importlib.import_module("hudiff_amd.cli." + cli)
    worst = []

    def count(job, rows):
        loc = np.asarray(job.loc, np.int64)
        assert job.origin is not None and (job.origin[loc] <= 21).all()
        worst.append(max(int((np.asarray(r)[loc] != job.origin[loc]).sum()) for r in rows))
    real_s, real_b = sampler.sample_jobs, sampler.beam_jobs

    def rec_s(model, jobs, *a, **kw):
        res = real_s(model, jobs, *a, **kw)
        tok = res[0] if isinstance(res, tuple) else res
        for j, job in enumerate(jobs):
            count(job, tok[j].reshape(-1, tok.shape[-1]))
        return res

    def rec_b(model, jobs, *a, **kw):
        res = real_b(model, jobs, *a, **kw)
        for j, job in enumerate(jobs):
            assert res[3][j].any()
            count(job, res[0][j][res[3][j]])
        return res
    monkeypatch.setattr(sampler, "sample_jobs", rec_s)
    monkeypatch.setattr(sampler, "beam_jobs", rec_b)
    if hasattr(mod, "sample_jobs"):
        monkeypatch.setattr(mod, "sample_jobs", rec_s)
    outs = {}
    for tag, extra in (("none", []), ("m3", ["--max_mutations", "3"]), ("beam", ["--max_mutations", "3", "--beam", "4"]),
                       ("m999", ["--max_mutations", "999"])):
        worst.clear()
        out = mod.main(_cli_args(cli, tmp_path, tag) + extra)
        outs[tag] = open(out, "rb").read()
        assert worst, tag
        if tag in ("m3", "beam"):
            assert max(worst) <= 3, (cli, tag, worst)
        else:
            assert max(worst) > 3, (cli, tag, worst)                         # the inputs' own runs are far from them
    assert outs["m999"] == outs["none"] and outs["m3"] != outs["none"]
    if cli != "sample_for_nano_cdr":                                         # (which writes only rows that number as a heavy domain)
        assert outs["m3"].count(b"humanization,") >= 1 and outs["beam"].count(b"humanization,") >= 1
