"""Beam search on the GPU (hd_set_beam): the device keeps the W best rows of every group, position by position.

The definition replayed here is include/hudiff_hip.h "beam search".  Two checks carry every case: (a) selection, gather, score and
parent are `guide.beam_select` applied to the DEVICE's own candidate table, bit for bit; (b) that table, minus the parent's score, is
the float64 oracle's log-softmax at the tokens the row held before the step.  Because (a) uses the device's table and (b) bounds the
table, no near-tie exemption is needed.  Tolerances are the siblings' (tests/test_gpu_logp.py): REF_TOL device against the float64
oracle (divided by min(temperature, 1) when guided), PAIR_TOL device against device."""
import os

import numpy as np
import pytest

import hudiff_oracle as ho
from conftest import chain_or_none, load_cfg, load_golden, load_weights, prec
from test_gpu_block import TRACE, _batch
from test_gpu_guide import ALL, _random_guide
from test_gpu_logp import PAIR_TOL, REF_TOL, _ab_checkpoint, _load_prod, _mk, _nb_checkpoint, _ragged, log_softmax64

pytestmark = pytest.mark.gpu

WIDTHS = [1, 3, 9, 64]


@pytest.fixture(scope="module")
def hip():
    import hudiff_amd
    if hudiff_amd.device_count() < 1:
        pytest.fail("no MI355X visible: GPU tests must run on the GPU box (there is no CPU fallback)")
    return hudiff_amd


@pytest.fixture(scope="module", params=["ab", "nb"])
def micro(request, hip):
    """m0: the micro model; lane_min_rows = 2, so that `lanes=2` really splits the small batches used here (at group boundaries)."""
    kind = request.param
    cfg, sd = load_cfg(kind), load_weights(kind)
    models = {"kind": kind, "m0": _mk(hip, kind, cfg, sd, options={"lane_min_rows": 2}),
              "m1": _mk(hip, kind, dict(cfg, dropout=0.2 if kind == "ab" else 0.5), sd),
              "o0": ho.OracleNet(kind, cfg, sd, dtype=np.float64)}
    yield models
    models["m0"].close(); models["m1"].close()


# ---- helpers ------------------------------------------------------------------------------------------------------------------------
_groups_cache, _row_logits = {}, {}


def _groups(kind):
    """G = 3 groups with T = [4, 2, 0] (the last one is never touched): tokens [3, L], region, chain [6] | None, order [3, 4], T."""
    if kind not in _groups_cache:
        batch, order, T = _ragged(kind, 3, 71, 4)
        assert (T == 4).all()
        _groups_cache[kind] = (batch["tokens"], batch["region"], batch["chain"], order, np.array([4, 2, 0], np.int32))
    return _groups_cache[kind]


def _replicate(tokens, region, chain, order, T, W):
    G = tokens.shape[0]
    rep = np.repeat(np.arange(G), W)
    ch = None if chain is None else np.concatenate([np.asarray(chain)[:G][rep], np.asarray(chain)[G:][rep]])
    return tokens[rep], region[rep], ch, order[rep], np.asarray(T)[rep]


def _bitsame(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.int32), b.view(np.int32))


def _snap(m):
    score, parent, cand = m.beam_state()
    return {"tok": m.sample_tokens(), "score": score, "parent": parent, "lp": m.sample_logp(), "cand": cand}


def _drive(m, groups, W, guide=None, truncation=None, **kw):
    """A beam session position by position: [(state before position t, state after it)], and the final tokens."""
    tokens, region, chain, order, T = groups
    G = tokens.shape[0]
    gd = None if guide is None else guide.take(np.repeat(np.arange(G), W))
    m.beam_begin(*_replicate(tokens, region, chain, order, T, W), W, guide=gd, truncation=truncation, **kw)
    steps, before = [], _snap(m)
    for t in range(order.shape[1]):
        m.sample_run(t, t + 1)
        after = _snap(m)
        steps.append((before, after))
        before = after
    return steps, m.sample_end()


def _check_selection(groups, W, steps, final):
    """(a): what position t did to every group is beam_select of the device's own table, bit for bit."""
    from hudiff_amd.guide import beam_select
    tokens, region, chain, order, T = groups
    G = tokens.shape[0]
    s0 = steps[0][0]
    assert np.array_equal(s0["tok"], np.repeat(tokens, W, 0)) and not s0["parent"].any() and not s0["lp"].any()
    first = np.arange(G * W) % W == 0
    assert (s0["score"][first] == 0).all() and np.isneginf(s0["score"][~first]).all()
    cases = 0
    for t, (b, a) in enumerate(steps):
        for g in range(G):
            r = slice(g * W, (g + 1) * W)
            if t >= T[g]:                                   # untouched
                for k in ("tok", "parent", "lp"):
                    assert np.array_equal(a[k][r], b[k][r]), (t, g, k)
                assert _bitsame(a["score"][r], b["score"][r]) and _bitsame(a["cand"][r], b["cand"][r])
                continue
            slot = order[g, t]
            w, j, v = beam_select(a["cand"][r], W)
            assert _bitsame(a["score"][r], v), (t, g)
            assert np.array_equal(a["parent"][r, t], w), (t, g)
            assert _bitsame((b["score"][r][w] + a["lp"][r, t]).astype(np.float32), v), (t, g)
            want = b["tok"][r][w].copy()
            want[:, slot] = j
            assert np.array_equal(a["tok"][r], want), (t, g)
            assert np.array_equal(np.delete(a["parent"][r], t, 1), np.delete(b["parent"][r], t, 1))       # the other positions stay
            assert np.array_equal(np.delete(a["lp"][r], t, 1), np.delete(b["lp"][r], t, 1))
            # rows stand in score order; the live rows are pairwise different
            live = np.isfinite(a["score"][r])
            n = int(live.sum())
            assert live[:n].all() and (np.diff(a["score"][r][:n]) <= 0).all()
            assert len({row.tobytes() for row in a["tok"][r][:n]}) == n
            cases += 1
    assert np.array_equal(final, steps[-1][1]["tok"])
    return cases


def _oracle_rows(micro, rows, region, chain2):
    """float64 logits [n, L, 22] of the oracle at token rows [n, L] that share region [L] and chain (heavy id, light id) | None; one
    oracle row per distinct state, shared by every width, lane split and test that reaches it."""
    kind = micro["kind"]
    keys = [(kind, region.tobytes(), chain2, row.tobytes()) for row in rows]
    todo = sorted({k for k in keys if k not in _row_logits})
    if todo:
        st = np.stack([np.frombuffer(k[3], np.int32) for k in todo])
        ch = None if chain2 is None else np.array([chain2[0]] * len(todo) + [chain2[1]] * len(todo), np.int32)
        z = np.asarray(micro["o0"](st, np.repeat(region[None], len(todo), 0), ch)[:, :, :22], np.float64)
        for k, zz in zip(todo, z):
            _row_logits[k] = zz
    return np.stack([_row_logits[k] for k in keys])


def _check_table(micro, groups, W, steps, allow=None, bias=None, temperature=1.0, truncation=None):
    """(b): for every live row, cand - score_prev is the oracle's (guided, truncated) log-softmax at the row's pre-step tokens for all
    22 tokens, and exactly -inf where the guide or the cut removes a token."""
    from hudiff_amd.guide import guided_log_probs
    tokens, region, chain, order, T = groups
    G = tokens.shape[0]
    tol = REF_TOL / min(temperature, 1.0)
    worst, rows = 0.0, 0
    for t, (b, a) in enumerate(steps):
        for g in range(G):
            if t >= T[g]:
                continue
            r = np.arange(g * W, (g + 1) * W)
            live = r[np.isfinite(b["score"][r])]
            assert len(live) >= 1
            slot = order[g, t]
            z = _oracle_rows(micro, b["tok"][live], region[g], None if chain is None else (int(chain[g]), int(chain[G + g])))[:, slot]
            al = ALL if allow is None else allow[g, slot]
            want = guided_log_probs(z, np.full(len(live), al), None if bias is None else bias[g, slot][None], temperature, truncation)
            got = a["cand"][live].astype(np.float64) - b["score"][live].astype(np.float64)[:, None]
            gone = np.isneginf(want)
            assert np.array_equal(np.isneginf(a["cand"][live]), gone), (t, g)
            worst = max(worst, float(np.abs(got[~gone] - want[~gone]).max()))
            rows += len(live)
            # a dead row's candidates are all dead
            dead = r[~np.isfinite(b["score"][r])]
            assert np.isneginf(a["cand"][dead]).all()
    print(f"{micro['kind']} W {W}: {rows} live (row, position) pairs, |cand - score - oracle| {worst:.2e} (bound {tol:.1e})")
    assert worst < tol
    return rows


# ---- 1. the definition, position by position ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("lanes", [1, 2])
@pytest.mark.parametrize("W", WIDTHS)
def test_definition_position_by_position(micro, W, lanes):
    m, groups = micro["m0"], _groups(micro["kind"])
    m.debug_launch_tally()
    steps, final = _drive(m, groups, W, lanes=lanes)
    tally = m.debug_launch_tally()
    assert tally[f"sample_lanes_{lanes}"] > 0 and tally["tail_sliced"] + tally["tail_launches"] > 0, tally       # the pruned tail applies
    assert _check_selection(groups, W, steps, final) == 6
    rows = _check_table(micro, groups, W, steps)
    assert rows == sum(min(W, 22 ** t) for t in range(4)) + sum(min(W, 22 ** t) for t in range(2))


# ---- 2. enumeration --------------------------------------------------------------------------------------------------------------------
def test_enumeration(micro):
    """Three allowed residues at each of two slots: W = 9 returns exactly the nine sequences, ranked; their scores are model.score's."""
    from hudiff_amd import Guide
    kind, m = micro["kind"], micro["m0"]
    tokens, region, chain, order, _ = _groups(kind)
    tokens, region, order = tokens[:1], region[:1], np.ascontiguousarray(order[:1, :2])
    chain = None if chain is None else np.array([chain[0], chain[3]], np.int32)
    T = np.array([2], np.int32)
    allow = np.full((1, tokens.shape[1]), ALL, np.uint32)
    sets = ([2, 7, 19], [0, 7, 11])
    for s, ok in zip(order[0], sets):
        allow[0, s] = sum(1 << j for j in ok)
    guide = Guide(allow[0])
    steps, _ = _drive(m, (tokens, region, chain, order, T), 9, guide=guide)
    assert np.isfinite(steps[0][1]["score"]).sum() == 3 and np.isfinite(steps[1][1]["score"]).sum() == 9      # 8, then 6 dead rows went in
    tok, score, logp, live = m.beam_search(tokens, region, chain, order, T, 9, guide=guide)
    assert tok.shape == (1, 9, tokens.shape[1]) and live.all() and (np.diff(score[0]) <= 0).all()
    got = {(int(r[order[0, 0]]), int(r[order[0, 1]])) for r in tok[0]}
    assert got == {(a, b) for a in sets[0] for b in sets[1]}
    rest = np.ones(tokens.shape[1], bool)
    rest[order[0]] = False
    assert (tok[0][:, rest] == tokens[0][rest]).all()
    ch9 = None if chain is None else np.array([chain[0]] * 9 + [chain[1]] * 9, np.int32)
    want = m.score(tok[0], np.repeat(region, 9, 0), ch9, np.repeat(order, 9, 0), np.full(9, 2), guide=guide, parallel=False)
    err = float(np.abs(want.astype(np.float64).sum(1) - score[0]).max())
    print(f"{kind}: |beam score - model.score| over the 9 sequences {err:.2e}; history against score {np.abs(logp[0] - want).max():.2e}")
    assert err < 2 * PAIR_TOL and np.abs(logp[0] - want).max() < PAIR_TOL
    assert np.abs(logp[0].astype(np.float64).sum(1) - score[0]).max() < 1e-5
    # W = 4: the four best of them
    tok4, score4, _, live4 = m.beam_search(tokens, region, chain, order, T, 4, guide=guide)
    assert live4.all() and (np.diff(score4[0]) <= 0).all() and len({r.tobytes() for r in tok4[0]}) == 4
    assert np.abs(score4[0] - score[0, :4]).max() < 2 * PAIR_TOL


# ---- 3. W = 1 against the greedy recording session ------------------------------------------------------------------------------------
def test_width_one_is_the_greedy_decode(micro):
    from hudiff_amd import Guide
    kind, m = micro["kind"], micro["m0"]
    batch, order, T, allow, bias = _batch(kind)
    B, tcap = order.shape
    greedy, glp = m.sample(batch["tokens"], batch["region"], batch["chain"], order, T, dropout="off", return_logp=True,
                           guide=Guide(allow, bias, 0.0))
    steps, final = _drive(m, (batch["tokens"], batch["region"], batch["chain"], order, T), 1, guide=Guide(allow, bias, 1.0))
    same = np.ones(B, bool)                                  # rows whose beam has met no exact tie at the top so far
    ties = compared = 0
    worst = 0.0
    for t, (b, a) in enumerate(steps):
        for r in np.flatnonzero(same & (t < T)):
            top = np.sort(a["cand"][r])[::-1]
            if top[0] == top[1]:
                same[r] = False
                ties += 1
                continue
            assert a["tok"][r, order[r, t]] == greedy[r, order[r, t]], (r, t)
            worst = max(worst, abs(float(a["lp"][r, t]) - float(glp[r, t])))
            compared += 1
    print(f"{kind}: W = 1 against the greedy session: {compared} positions equal, {ties} rows left at an exact tie, |logp| {worst:.2e}")
    assert np.array_equal(final[same], greedy[same]) and compared >= int(T.sum()) - 6 * ties and ties <= 2
    assert worst < PAIR_TOL
    live = np.arange(tcap)[None, :] < T[:, None]
    assert (steps[-1][1]["lp"][~live] == 0).all() and not steps[-1][1]["parent"].any()


# ---- 4. composition -------------------------------------------------------------------------------------------------------------------
def test_guide_and_truncation_compose(micro):
    from hudiff_amd import Guide, Truncation
    kind, m = micro["kind"], micro["m0"]
    groups = _groups(kind)
    allow, bias = _random_guide(3, groups[0].shape[1], seed=9)
    tr = Truncation(top_k=5)
    steps, final = _drive(m, groups, 3, guide=Guide(allow, bias, 0.5), truncation=tr, lanes=2)
    assert _check_selection(groups, 3, steps, final) == 6
    _check_table(micro, groups, 3, steps, allow, bias, 0.5, tr)
    for _, a in steps[:2]:
        assert (np.isfinite(a["cand"][:3]).sum(1) <= 5).all()


# ---- 5. forms and guards ----------------------------------------------------------------------------------------------------------------
def _result(m, groups, W, **kw):
    tokens, region, chain, order, T = groups
    m.beam_begin(*_replicate(tokens, region, chain, order, T, W), W, **kw)
    m.sample_run(0, order.shape[1])
    final = m.sample_end()                                   # (a guard's repeat happens here: the state is read behind it)
    score, parent, _ = m.beam_state()
    return final, score, parent


def _same_result(a, b):
    return np.array_equal(a[0], b[0]) and _bitsame(a[1], b[1]) and np.array_equal(a[2], b[2])


def test_forms_are_bit_identical(micro):
    m, groups = micro["m0"], _groups(micro["kind"])
    W = 9
    base = _result(m, groups, W, lanes=1)
    assert np.isfinite(base[1][:2 * W]).all() and base[2].any()
    for kw in (dict(lanes=2), dict(lanes=1, graph=False), dict(lanes=2, graph=False), dict(lanes=2, graph="loop")):
        assert _same_result(_result(m, groups, W, **kw), base), kw
    # a restart starts from the initial state again; ranges of positions in pieces
    tokens, region, chain, order, T = groups
    m.beam_begin(*_replicate(tokens, region, chain, order, T, W), W)
    m.sample_run(0, 3)
    m.sample_restart(5)
    s0 = _snap(m)
    assert np.array_equal(s0["tok"], np.repeat(tokens, W, 0)) and not s0["parent"].any() and not s0["lp"].any()
    assert (s0["score"][::W] == 0).all() and np.isneginf(np.delete(s0["score"], np.arange(0, 3 * W, W))).all()
    m.sample_run(0, 1); m.sample_run(1, 4)
    score, parent, _ = m.beam_state()
    assert _same_result((m.sample_end(), score, parent), base)


@pytest.mark.parametrize("kind", ["ab", "nb"])
def test_lnsync_guard_repeats_a_beam_session(hip, kind):
    """Production width (the micro models' launches hold no ln_sync meeting), the batch of the siblings' guard tests as 16 (20) groups
    of W = 8.  The repeat is a beam session from its initial state on the kernels the handle keeps from then on: it is bit for bit the
    session the handle runs next.  Against the undisturbed session (whose GEMMs normalise their own rows) the ranked scores agree
    within PAIR_TOL per position."""
    from hudiff_amd import evalsets as E, synthetic as S
    cfg = dict(S.AB_CONFIG if kind == "ab" else S.NB_CONFIG, dropout=0.0)
    mx = _mk(hip, kind, cfg, S.random_state_dict(kind, cfg, seed=0), precision="split")
    try:
        G, W, Tn = (16 if kind == "ab" else 20), 8, 2
        big = E.eval_batch("huab348" if kind == "ab" else "vhh", G, row0=0)
        groups = (big["tokens"], big["region"], big["chain"], np.ascontiguousarray(big["order"][:, :Tn]), np.minimum(big["T"], Tn).astype(np.int32))
        want = _result(mx, groups, W)
        prec(mx, lnsync_in_use=True, lnsync_fallbacks=0, last_call_repeated=False)
        mx.debug_fail_next_lnsync()
        with pytest.warns(RuntimeWarning, match="ln_sync"):
            again = _result(mx, groups, W)
        prec(mx, lnsync_in_use=False, lnsync_fallbacks=1, last_call_repeated=True)
        after = _result(mx, groups, W)
        prec(mx, lnsync_fallbacks=1, last_call_repeated=False)
        assert _same_result(again, after)
        err = float(np.abs(again[1] - want[1]).max())
        agree = (again[0] == want[0]).all(axis=1)
        print(f"{kind}: ln_sync guard in a beam session: |repeat - undisturbed| ranked scores {err:.2e}, {int(agree.sum())} of {G * W} rows equal")
        assert np.isfinite(again[1]).all() and err < Tn * PAIR_TOL
    finally:
        mx.close()


# ---- 6. production width -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("route", ["split", "f32_all"])
def test_production_width(hip, route):
    z, cfg, sd = _load_prod("ab")
    m = _mk(hip, "ab", cfg, sd, precision=route)
    try:
        G, W, Tn = 2, 8, 4
        chain = np.concatenate([z["chain"][:G], z["chain"][z["tokens"].shape[0]:z["tokens"].shape[0] + G]])
        groups = (z["tokens"][:G], z["region"][:G], chain, np.ascontiguousarray(z["order"][:G, :Tn]), np.full(G, Tn, np.int32))
        assert (z["T"][:G] >= Tn).all()
        steps, final = _drive(m, groups, W)
        assert _check_selection(groups, W, steps, final) == G * Tn
        assert np.isfinite(steps[-1][1]["score"]).all()
        worst = 0.0
        rep = np.repeat(np.arange(G), W)
        ch = np.concatenate([chain[:G][rep], chain[G:][rep]])
        for t, (b, a) in enumerate(steps):
            lsm = log_softmax64(m(b["tok"], groups[1][rep], ch, dropout="off")[np.arange(G * W), groups[3][rep, t], :22])
            live = np.isfinite(b["score"])
            got = a["cand"][live].astype(np.float64) - b["score"][live].astype(np.float64)[:, None]
            worst = max(worst, float(np.abs(got - lsm[live]).max()))
        print(f"ab production width, route {route}: |cand - score - log_softmax(hd_forward)| {worst:.2e}")
        assert worst < PAIR_TOL
    finally:
        m.close()


# ---- 7. lifetime and errors -----------------------------------------------------------------------------------------------------------
def test_lifetime_and_errors(micro):
    from hudiff_amd import Guide
    from hudiff_amd._lib import HD_ERR_INVALID, HD_ERR_STATE, HD_ERR_UNSUPPORTED, HudiffError
    kind, m = micro["kind"], micro["m0"]
    z = load_golden(TRACE[kind])
    tokens, region, chain, loc, q, golden = z["tokens"], z["region"], chain_or_none(z), z["loc"], z["q"], z["final"]
    B = tokens.shape[0]
    order, T = np.repeat(loc[None], B, 0), np.full(B, len(loc))

    def raises(status, fn, *a, **kw):
        with pytest.raises(HudiffError) as e:
            fn(*a, **kw)
        assert e.value.status == status, (e.value.status, status)

    def ordinary():
        """An ordinary sampling session on the same handle draws the golden trace's tokens."""
        assert np.array_equal(m.sample(tokens, region, chain, order, T, q_noise=q), golden)
    W = 2
    g = _groups(kind)
    rows = _replicate(g[0], g[1], g[2], g[3], g[4], W)
    base = _result(m, g, W)
    ordinary()                                               # one-shot: the session after a beam session is not one
    raises(HD_ERR_STATE, m.beam_state)                       # ... and it is not a beam session
    # the width's own range; inside an open session
    raises(HD_ERR_INVALID, m.set_beam, -1)
    raises(HD_ERR_INVALID, m.set_beam, 65)
    m.sample_begin(tokens, region, chain, order, T, q_noise=q)
    raises(HD_ERR_STATE, m.set_beam, 2)
    raises(HD_ERR_STATE, m.set_beam, 0)
    raises(HD_ERR_STATE, m.beam_state)
    m.sample_run(0, len(loc))
    assert np.array_equal(m.sample_end(), golden)
    # width 0 clears; hd_forward neither uses nor clears
    m.set_beam(W); m.set_beam(0)
    ordinary()
    m.set_beam(W)
    m(tokens[:1], region[:1], None if chain is None else np.array([chain[0], chain[B]]))
    m.sample_begin(*rows, dropout="off")
    m.sample_run(0, 4)
    score, parent, _ = m.beam_state()
    lp = m.sample_logp()                                      # it records without HD_RECORD_LOGP
    assert _same_result((m.sample_end(), score, parent), base) and (lp[:W] < 0).all()
    assert _bitsame(m.beam_state()[0], base[1])               # legal after the end, like sample_logp
    m(tokens[:1], region[:1], None if chain is None else np.array([chain[0], chain[B]]))
    raises(HD_ERR_STATE, m.beam_state)
    # consumed by a begin that fails -- each of the begin's refusals, and the ordinary session behind it
    bad = [r.copy() if r is not None else None for r in rows]
    bad[0][1, 7] = (bad[0][1, 7] + 1) % 20
    raises(HD_ERR_INVALID, m.beam_begin, *bad, W)             # a row that differs from the first of its group: tokens
    ordinary()
    bad = [r.copy() if r is not None else None for r in rows]
    bad[3][1, 1] = bad[3][1, 0]
    raises(HD_ERR_INVALID, m.beam_begin, *bad, W)             # ... its order
    bad = [r.copy() if r is not None else None for r in rows]
    bad[4][1] = 3
    raises(HD_ERR_INVALID, m.beam_begin, *bad, W)             # ... its T
    bad = [r.copy() if r is not None else None for r in rows]
    bad[1][3, 0] = (bad[1][3, 0] + 1) % 4
    raises(HD_ERR_INVALID, m.beam_begin, *bad, W)             # ... its region
    if chain is not None:
        bad = [r.copy() for r in rows]
        bad[2][len(rows[4]) + 1] = 3 - bad[2][len(rows[4]) + 1]
        raises(HD_ERR_INVALID, m.beam_begin, *bad, W)         # ... its light chain type
    ordinary()
    # an entry of the order beyond T may differ
    ok = [r.copy() if r is not None else None for r in rows]
    ok[3][3, 3] = (ok[3][3, 3] + 1) % 100
    m.beam_begin(*ok, W)
    m.sample_run(0, 4)
    assert np.array_equal(m.sample_end(), base[0])
    five = [rows[0][:5], rows[1][:5], None if chain is None else np.concatenate([rows[2][:5], rows[2][6:11]]), rows[3][:5], rows[4][:5]]
    raises(HD_ERR_INVALID, m.beam_begin, *five, W)            # B % W != 0
    ordinary()
    m.set_beam(W)
    raises(HD_ERR_INVALID, m.sample, *rows, dropout="off", q_noise=np.ones((4, 6, 22), np.float32))       # noise
    ordinary()
    raises(HD_ERR_INVALID, m.beam_begin, *rows, W, guide=Guide(temperature=0.0))                          # greedy guide
    ordinary()
    m.set_beam(W)
    raises(HD_ERR_UNSUPPORTED, m.sample, *rows, dropout="off", slots_per_step=2)
    ordinary()
    m.set_beam(W)
    raises(HD_ERR_UNSUPPORTED, m.sample, *rows, dropout="off", slot_policy="confident")
    ordinary()
    m.set_beam(W)
    raises(HD_ERR_UNSUPPORTED, m.score, golden, region, chain, order, T, parallel=False)                  # scoring consumes it
    assert (m.score(golden, region, chain, order, T, parallel=False) < 0).all()
    ordinary()
    # dropout on: a model whose config has dropout, asked to run it
    m1 = micro["m1"]
    raises(HD_ERR_UNSUPPORTED, m1.beam_begin, *rows, W, dropout="faithful")
    m1.beam_begin(*rows, W, dropout="off")
    m1.sample_run(0, 4)
    assert np.array_equal(m1.sample_end(), base[0])
    # hd_sample with a width set is the whole session; sample_run takes any range
    m.set_beam(W)
    assert np.array_equal(m.sample(*rows, dropout="off"), base[0])
    assert _bitsame(m.beam_state()[0], base[1])
    ordinary()
    assert _same_result(_result(m, g, W), base)


# ---- 8. CLI ------------------------------------------------------------------------------------------------------------------------------
def test_cli_beam(hip, tmp_path):
    """--beam 4 on the synthetic CSV: four rows per input, best first and pairwise different; the sidecar holds their scores; a second
    run writes the same bytes."""
    from hudiff_amd.cli import sample as cli
    from test_gpu_cli import _write_inputs
    csv, nb = _write_inputs(tmp_path, "ab", 3)
    outs = []
    for i in range(2):
        ck = tmp_path / f"beam{i}" / "checkpoints" / "hudiffab.pt"
        _ab_checkpoint(ck)
        sidecar = tmp_path / f"score{i}.csv"
        out = cli.main(["--ckpt", str(ck), "--data_fpath", str(csv), "--numbered_fpath", str(nb), "--beam", "4", "--gpus", "1",
                        "--forbid", "CM", "--top_k", "6", "--logp_fpath", str(sidecar), "--seed", "5"] + (["--device_batch", "5"] if i else []))
        outs.append([open(out, "rb").read(), open(os.path.join(os.path.dirname(out), "sample_identity.fa"), "rb").read(),
                     open(sidecar, "rb").read()])
    assert outs[0] == outs[1]
    lines = outs[0][0].decode().splitlines()
    assert lines[0] == "Specific,name,hseq,lseq," and len(lines) == 1 + 3 * 5
    side = [l.split(",") for l in outs[0][2].decode().splitlines()[1:]]
    assert len(side) == 12
    for i in range(3):
        blk = lines[1 + 5 * i:6 + 5 * i]
        assert blk[0].startswith(f"mouse,m{i},") and all(l.startswith(f"humanization,m{i}human_sample,") for l in blk[1:])
        assert len(set(blk[1:])) == 4
        sc = [float(f[-2]) for f in side[4 * i:4 * i + 4]]
        assert all(f[0] == f"m{i}" and f[-1] == "1" for f in side[4 * i:4 * i + 4]) and [int(f[2]) for f in side[4 * i:4 * i + 4]] == [0, 1, 2, 3]
        assert all(np.isfinite(sc)) and sc == sorted(sc, reverse=True) and sc[0] < 0


def test_cli_beam_nanobody(hip, tmp_path):
    from hudiff_amd.cli import nanosample as cli
    from test_gpu_cli import _write_inputs
    csv, nb = _write_inputs(tmp_path, "nb", 2)
    ck = tmp_path / "beam" / "checkpoints" / "hudiffnb.pt"
    _nb_checkpoint(ck)
    sidecar = tmp_path / "score.csv"
    out = cli.main(["--ckpt", str(ck), "--data_fpath", str(csv), "--numbered_fpath", str(nb), "--model", "finetune_vh", "--beam", "3",
                    "--try_number", "3", "--logp_fpath", str(sidecar), "--seed", "4"])
    lines = open(out).read().splitlines()
    side = [l.split(",") for l in open(sidecar).read().splitlines()[1:]]
    assert len(side) == 6 and all(f[1] == "0" for f in side)
    for i in range(2):
        sc = [float(f[-2]) for f in side[3 * i:3 * i + 3]]
        assert sc == sorted(sc, reverse=True) and all(np.isfinite(sc))
        wrote = [l for l in lines if l.startswith(f"humanization,{i}human_sample,")]
        assert len(wrote) == sum(int(f[-1]) for f in side[3 * i:3 * i + 3]) and len(set(wrote)) == len(wrote) and 1 <= len(wrote) <= 3
