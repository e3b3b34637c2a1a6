"""Confidence-ordered decoding on the GPU (hd_set_slot_policy, HD_SLOTS_CONFIDENT): the device picks each forward's slots.

The definition replayed here (include/hudiff_hip.h "slot policy"): forward f of row b ranks the remaining positions of the row's order
by the key c = sum_j exp(g_j - max g) of THIS forward's distribution at their slots (smaller = surer), moves the min(K, remaining)
smallest (c, position) to the front in ascending order -- a stable partition -- and the block draw then fills them with the noise, guide
and logp entry of their positions.

`_check` is that definition in float64, forward by forward from the device's own tokens (as `_replay` of tests/test_gpu_block.py), with
guide.confidence_keys on the oracle's logits.  Tolerances are the siblings': REF_TOL = 2e-4 (device log-probability against the float64
oracle), PAIR_TOL = 4e-4 (two device results), GAP_TOL = 4e-4 (a draw the oracle cannot call), divided by min(temperature, 1) when
guided.  The device's log key is -log p_max, a log-probability like those REF_TOL bounds, so two keys can swap only when the oracle's are
within 2 REF_TOL of each other: every chosen position's oracle key is at most 2 REF_TOL above every not-chosen one's, and consecutive
chosen keys ascend within the same slack.  The check is kept from being vacuous by a cap of 2 % on the share of compared (chosen,
not-chosen) pairs that lie inside the slack.  Measured with the float64 oracle's OWN draws on the CPU before the first GPU run (the
whole loop end to end; ab / nb):
    batch A  K = 1: 0 of 573 / 0 of 573    K = 2: 0 of 458 / 2 of 458    K = 4: 0 of 304 / 0 of 304
    batch L  K = 64: 0 of 33600 / 1 of 7232
    batch A, K = 3, random guide: temperature 0.5: 1 of 342 / 0 of 342    temperature 0: 0 of 342 / 0 of 342
i.e. at most 0.44 % (nb, batch A, K = 2); the realised order differed from the list in 39 (ab) and 38 (nb) of the 39 live rows.

There is no launch-tally id for the two selection kernels (the table is pinned by tests/test_host_logic.py); the witnesses are the
pruned tail -- a confident session issues none, at K = 1 too -- and hd_sample_order."""
import os

import numpy as np
import pytest

import hudiff_oracle as ho
from conftest import load_cfg, load_golden, load_weights, chain_or_none, prec
from hudiff_amd.guide import confidence_keys
from test_gpu_block import TRACE, _batch, _block_sample, _logits64, _pruned_tail
from test_gpu_guide import ALL, GAP_TOL, ROW0, SEED, _bits, _live, _visited
from test_gpu_logp import PAIR_TOL, REF_TOL, _ab_checkpoint, _mk, _nb_checkpoint

pytestmark = pytest.mark.gpu

CLOSE_CAP = 0.02                                         # largest share of (chosen, not-chosen) pairs inside the slack


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
    p = 0.2 if kind == "ab" else 0.5
    models = {"kind": kind, "p": p, "m0": _mk(hip, kind, cfg, sd), "m1": _mk(hip, kind, dict(cfg, dropout=p), sd),
              "o0": ho.OracleNet(kind, cfg, sd, dtype=np.float64), "o1": ho.OracleNet(kind, dict(cfg, dropout=p), sd, dtype=np.float64)}
    yield models
    models["m0"].close(); models["m1"].close()


_data_cache, _run_cache = {}, {}


def _data(kind, name):
    """Batch A: the siblings' oracle batch (40 rows, tcap 6, T[5] = 0, T[17] = 3, 231 draws).  Batch L: three rows with every slot
    masked, a seeded permutation of all L slots as the list, T = [L, 65, 1]: at K = 64 the rank crosses 64, 128 and (ab) 256
    candidates, one row has fewer candidates left than K and one ends after one position."""
    if (kind, name) not in _data_cache:
        if name == "A":
            batch, order, T, _, _ = _batch(kind)
        else:
            from hudiff_amd import synthetic as S
            batch = S.synthetic_batch(kind, 3, seed=33)
            L = batch["tokens"].shape[1]
            batch = dict(batch, tokens=np.full_like(batch["tokens"], 22))
            rng = np.random.default_rng(7)
            order = np.stack([rng.permutation(L) for _ in range(3)]).astype(np.int32)
            T = np.array([L, 65, 1], np.int32)
        _data_cache[(kind, name)] = (batch, order, T)
    return _data_cache[(kind, name)]


def _args(data):
    batch, order, T = data
    return (batch["tokens"], batch["region"], batch["chain"], order, T)


KW = dict(seed=SEED, row0=ROW0, dropout="off")


def _confident(micro, name, K, lanes=2):
    """(tokens, logp, realised order) of the recording confident session of a batch at dropout off; once per (kind, batch, K, lanes)."""
    key = (micro["kind"], name, K, lanes)
    if key not in _run_cache:
        m = micro["m0"]
        tok, lp = m.sample(*_args(_data(micro["kind"], name)), lanes=lanes, return_logp=True, slots_per_step=K, slot_policy="confident", **KW)
        _run_cache[key] = (tok, lp, m.sample_order())
    return _run_cache[key]


def _check(micro, data, K, tok, lp, R, allow=None, bias=None, temperature=1.0, logits_fn=None, forwards=None, seed=SEED, label=""):
    """The definition in float64 (module docstring).  `logits_fn(state)` -> float64 [B, L, 22] (default: the dropout-off oracle);
    `forwards`: stop after that many (the permutation check at the end then covers the prefix only)."""
    kind = micro["kind"]
    batch, order, T = data
    B, tcap = order.shape
    scale = min(temperature, 1.0) if temperature > 0 else 1.0
    slack = 2 * REF_TOL / scale
    if logits_fn is None:
        logits_fn = lambda state: _logits64(micro, state, batch["region"], batch["chain"])
    state, cur = batch["tokens"].copy(), order.copy()
    pairs = close = cases = left_out = done = 0
    worst_lp, worst_key, smallest_gap = 0.0, -np.inf, np.inf
    noise = {}
    for f, t0 in enumerate(range(0, tcap, K)):
        if not (T > t0).any() or (forwards is not None and f >= forwards):
            break
        z = logits_fn(state)
        nxt = state.copy()
        for b in range(B):
            n = min(t0, int(T[b]))
            k = min(K, int(T[b]) - n)
            if k <= 0:
                continue
            rem = cur[b, n:T[b]]
            key = confidence_keys(z[b, rem], None if allow is None else allow[b, rem], None if bias is None else bias[b, rem], temperature)
            chosen = R[b, n:n + k]
            where = {int(s): i for i, s in enumerate(rem)}
            ci = np.array([where[int(s)] for s in chosen])              # (KeyError: a slot that was not left)
            assert len(set(ci.tolist())) == k
            rest = np.ones(len(rem), bool)
            rest[ci] = False
            kc, kn = key[ci], key[rest]
            assert np.isfinite(key).all()
            if kn.size:
                d = kc[:, None] - kn[None, :]
                worst_key = max(worst_key, float(d.max()))
                assert d.max() <= slack, (label, f, b, float(d.max()))
                pairs += d.size
                close += int((np.abs(d) < slack).sum())
            assert (np.diff(kc) >= -slack).all(), (label, f, b, kc)
            cur[b, n:T[b]] = np.concatenate([chosen, rem[rest]])       # the stable partition, given what was chosen
            for j in range(k):                                          # the draws, as _replay of tests/test_gpu_block.py
                t, s = n + j, int(chosen[j])
                if t not in noise:
                    noise[t] = ho.philox_exp_noise(seed, ROW0 + np.arange(B), t).astype(np.float64)
                ok = np.ones(22, bool) if allow is None else _bits(allow[b, s], np.arange(22))
                g1 = np.where(ok, z[b, s] + (0.0 if bias is None else bias[b, s].astype(np.float64)), -np.inf)
                g = g1 if temperature == 0 else g1 / temperature
                lsm = g - g.max()
                lsm = lsm - np.log(np.exp(lsm).sum())
                score = g if temperature == 0 else np.where(ok, g - np.log(noise[t][b]), -np.inf)
                got = int(tok[b, s])
                worst_lp = max(worst_lp, abs(float(lp[b, t]) - lsm[got]))
                top = np.sort(score[ok])[::-1]
                gap = top[0] - top[1] if len(top) > 1 else np.inf
                smallest_gap = min(smallest_gap, gap)
                cases += 1
                if gap < GAP_TOL / scale:
                    left_out += 1
                else:
                    assert got == int(np.argmax(score)), (label, b, t, got, int(np.argmax(score)), gap)
                nxt[b, s] = got
        state = nxt
        done = min(t0 + K, tcap)
    share = close / max(pairs, 1)
    print(f"{kind} {label} K {K} temperature {temperature}: {cases} draws, {left_out} left out, smallest oracle gap {smallest_gap:.2e}, "
          f"|logp - oracle| {worst_lp:.2e} (bound {REF_TOL / scale:.1e}); keys: {close} of {pairs} pairs inside the slack {slack:.1e} "
          f"({100 * share:.3f} %), largest chosen - not chosen {worst_key:.2e}")
    assert pairs > 0 and share <= CLOSE_CAP
    # (the siblings leave out at most 2 of 231 draws: 1 %)
    assert left_out <= max(2, cases // 100)
    assert worst_lp < REF_TOL / scale
    for b in range(B):
        v = min(done, int(T[b]))
        assert np.array_equal(cur[b, :v], R[b, :v])
        if forwards is None:
            assert np.array_equal(cur[b], R[b])
    return state, cases


def _structure(data, tok, R):
    batch, order, T = data
    B, tcap = order.shape
    L = tok.shape[1]
    for b in range(B):
        assert sorted(R[b, :T[b]].tolist()) == sorted(order[b, :T[b]].tolist()), b
        assert np.array_equal(R[b, T[b]:], order[b, T[b]:]), b
    vis = _visited(order, T, L)
    assert np.array_equal(tok[~vis], batch["tokens"][~vis]) and not (tok[vis] == 22).any()


# ---- 1. the default is untouched -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["ab", "nb"])
def test_given_is_todays_session(hip, kind):
    z = load_golden(TRACE[kind])
    tokens, region, chain, loc, q, final = z["tokens"], z["region"], chain_or_none(z), z["loc"], z["q"], z["final"]
    B = tokens.shape[0]
    order, T = np.repeat(loc[None], B, 0), np.full(B, len(loc))
    m = _mk(hip, kind, load_cfg(kind), load_weights(kind))
    try:
        m.debug_launch_tally()
        tok1, lp1 = m.sample(tokens, region, chain, order, T, q_noise=q, return_logp=True, slot_policy="given")
        tally1 = m.debug_launch_tally()
        assert np.array_equal(m.sample_order(), order)
        m2 = _mk(hip, kind, load_cfg(kind), load_weights(kind))
        try:
            m2.debug_launch_tally()
            tok0, lp0 = m2.sample(tokens, region, chain, order, T, q_noise=q, return_logp=True)
            tally0 = m2.debug_launch_tally()
        finally:
            m2.close()
        assert np.array_equal(tok1, final) and np.array_equal(tok0, final) and np.array_equal(lp1, lp0)
        assert _pruned_tail(tally1) > 0 and _pruned_tail(tally0) > 0, (tally1, tally0)
        assert np.array_equal(m.sample(tokens, region, chain, order, T, q_noise=q, slot_policy="given"), final)
    finally:
        m.close()


def test_given_block_session_is_todays(micro):
    want = _block_sample(micro, 3)
    got = micro["m0"].sample(*_args(_data(micro["kind"], "A")), return_logp=True, slots_per_step=3, slot_policy="given", **KW)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])


# ---- 2. the selection against the float64 oracle ----------------------------------------------------------------------------------------
CASES = [("A", 1, 1), ("A", 1, 2), ("A", 2, 1), ("A", 2, 2), ("A", 4, 1), ("A", 4, 2), ("L", 64, 2)]


@pytest.mark.parametrize("name,K,lanes", CASES)
def test_selection_against_an_oracle_loop(micro, name, K, lanes):
    kind, m = micro["kind"], micro["m0"]
    data = _data(kind, name)
    batch, order, T = data
    tcap = order.shape[1]
    m.debug_launch_tally()
    tok, lp, R = _confident(micro, name, K, lanes)
    tally = m.debug_launch_tally()
    # (a cached result issues nothing: the witnesses are looked at where the session ran)
    if sum(tally.values()) > 0:
        assert _pruned_tail(tally) == 0 and tally[f"sample_lanes_{lanes if name == 'A' else 1}"] > 0, tally
    _structure(data, tok, R)
    live = _live(T, tcap)
    assert (lp[~live] == 0).all() and (lp[live] < 0).all()
    final, cases = _check(micro, data, K, tok, lp, R, label=f"batch {name} lanes {lanes}")
    assert np.array_equal(final, tok) and cases == int(T.sum())
    if name == "A":
        assert cases == 231 and np.array_equal(tok[5], batch["tokens"][5]) and np.array_equal(R[5], order[5])
        moved = sum(not np.array_equal(R[b], order[b]) for b in range(len(T)))
        print(f"{kind} K {K}: the realised order differs from the list in {moved} of 39 live rows")
        assert moved >= 30
    # the plain (not recording) session draws the same tokens
    plain = m.sample(*_args(data), lanes=lanes, slots_per_step=K, slot_policy="confident", **KW)
    assert np.array_equal(plain, tok) and np.array_equal(m.sample_order(), R)


# ---- 3. the replay invariant ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,K,lanes", CASES)
def test_replay_invariant(micro, name, K, lanes):
    """A given-order session at the realised order is the same session bit for bit.  At K = 1 a given-order session prunes its last
    attention block to the visited row (other kernels, so another device result); with prune=False it evaluates the hidden rows the
    confident session did, and that is the one compared bit for bit -- the pruned one within PAIR_TOL."""
    m = micro["m0"]
    batch, order, T = _data(micro["kind"], name)
    tok, lp, R = _confident(micro, name, K, lanes)
    got = m.sample(batch["tokens"], batch["region"], batch["chain"], R, T, lanes=lanes, return_logp=True, slots_per_step=K, prune=K > 1, **KW)
    assert np.array_equal(got[0], tok) and np.array_equal(got[1], lp)
    assert np.array_equal(m.sample_order(), R)
    if K == 1:
        pruned = m.sample(batch["tokens"], batch["region"], batch["chain"], R, T, lanes=lanes, return_logp=True, **KW)
        assert np.array_equal(pruned[0], tok) and np.abs(pruned[1] - lp).max() < PAIR_TOL
    sc = m.score(tok, batch["region"], batch["chain"], R, T, slots_per_step=K)
    err = float(np.abs(sc - lp).max())
    print(f"{micro['kind']} batch {name} K {K}: |score at the realised order - recorded| {err:.2e}")
    assert err < PAIR_TOL


# ---- 4. launch forms ---------------------------------------------------------------------------------------------------------------------------
def test_launch_forms_agree_bit_for_bit(hip, micro):
    kind, K, m = micro["kind"], 2, micro["m0"]
    data = _data(kind, "A")
    batch, order, T = data
    B, tcap = order.shape
    args = _args(data)
    want = _confident(micro, "A", K)
    ckw = dict(KW, slots_per_step=K, slot_policy="confident")

    def run(mm, **kw):
        tok, lp = mm.sample(*args, return_logp=True, **dict(ckw, **kw))
        return tok, lp, mm.sample_order()
    got = {"graph": run(m), "eager": run(m, graph=False), "loop": run(m, graph="loop")}
    m2 = _mk(hip, kind, load_cfg(kind), load_weights(kind), options={"lane_min_rows": 2})
    try:
        got["lanes2"] = run(m2, lanes=2)
    finally:
        m2.close()
    m.sample_begin(*args, record_logp=True, **ckw)
    for t0 in (0, 2, 4):
        m.sample_run(t0, t0 + 2)
        part = m.sample_order()
        for b in range(B):
            v = min(t0 + 2, int(T[b]))
            assert np.array_equal(part[b, :v], want[2][b, :v]), (t0, b)           # the visited prefix is final
            assert sorted(part[b, v:T[b]].tolist()) == sorted(want[2][b, v:T[b]].tolist())
            assert np.array_equal(part[b, T[b]:], order[b, T[b]:])
    lp = m.sample_logp()
    R = m.sample_order()
    got["split_call"] = (m.sample_end(), lp, R)
    assert np.array_equal(m.sample_order(), R)                                     # still legal after the end
    q = np.stack([ho.philox_exp_noise(SEED, ROW0 + np.arange(B), t) for t in range(tcap)])
    got["q_noise"] = run(m, q_noise=q, seed=1)
    for name, res in got.items():
        for a, b in zip(res, want):
            assert np.array_equal(a, b), name
    assert np.array_equal(m.sample(*args, **ckw), want[0])


# ---- 5. scoring under the policy -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [1, 2, 4])
def test_scoring_under_the_policy(micro, K):
    m = micro["m0"]
    batch, order, T = _data(micro["kind"], "A")
    tok, lp, R = _confident(micro, "A", K)
    args = (tok, batch["region"], batch["chain"], order, T)
    sc = m.score(*args, slots_per_step=K, slot_policy="confident", parallel=False)
    assert np.array_equal(m.sample_order(), R)
    err = float(np.abs(sc - lp).max())
    print(f"{micro['kind']} K {K}: |score under the policy - recorded| {err:.2e}")
    assert err < PAIR_TOL and (sc[~_live(T, order.shape[1])] == 0).all()
    with pytest.raises(ValueError):
        m.score(*args, slots_per_step=K, slot_policy="confident", parallel=True)
    auto = m.score(*args, slots_per_step=K, slot_policy="confident")
    assert np.array_equal(auto, sc) and np.array_equal(m.sample_order(), R)
    # the split form
    m.score_begin(*args, slots_per_step=K, slot_policy="confident")
    m.sample_run(0, order.shape[1])
    assert np.array_equal(m.sample_logp(), sc) and np.array_equal(m.sample_order(), R)
    assert np.array_equal(m.sample_end(), tok)


# ---- 6. guide and policy together ----------------------------------------------------------------------------------------------------------
def test_guide_and_policy_together(micro):
    from hudiff_amd import Guide
    kind, m, K = micro["kind"], micro["m0"], 3
    data = _data(kind, "A")
    batch, order, T = data
    _, _, _, allow, bias = _batch(kind)
    B, L = batch["tokens"].shape
    args = _args(data)
    kw = dict(KW, return_logp=True, slots_per_step=K, slot_policy="confident")
    want = _confident(micro, "A", K)
    neutral = Guide(np.full((B, L), ALL, np.uint32), np.zeros((B, L, 22), np.float32), 1.0)
    tok, lp = m.sample(*args, guide=neutral, **kw)
    assert np.array_equal(tok, want[0]) and np.array_equal(lp, want[1]) and np.array_equal(m.sample_order(), want[2])
    vis = _visited(order, T, L)
    for temperature in (0.5, 0.0):
        g = Guide(allow, bias, temperature)
        tok, lp = m.sample(*args, guide=g, **kw)
        R = m.sample_order()
        _structure(data, tok, R)
        assert _bits(allow[vis], tok[vis]).all(), "a drawn token is not allowed at its slot"
        final, cases = _check(micro, data, K, tok, lp, R, allow, bias, temperature, label="guided")
        assert np.array_equal(final, tok) and cases == 231
        # the replay invariant, under the same guide (which is keyed by slot on this side of the ABI)
        again = m.sample(batch["tokens"], batch["region"], batch["chain"], R, T, guide=g, **dict(kw, slot_policy="given"))
        assert np.array_equal(again[0], tok) and np.array_equal(again[1], lp)
        if temperature > 0:
            sc = m.score(tok, *args[1:], guide=g, slots_per_step=K, slot_policy="confident")
            assert np.array_equal(m.sample_order(), R) and np.abs(sc - lp).max() < PAIR_TOL / temperature
    # allowed bits without a bias: the third instantiation's host path (gallow moves, there is no gbias)
    g = Guide(allow, None, 1.0)
    tok, lp = m.sample(*args, guide=g, **kw)
    R = m.sample_order()
    assert _bits(allow[vis], tok[vis]).all()
    again = m.sample(batch["tokens"], batch["region"], batch["chain"], R, T, guide=g, **dict(kw, slot_policy="given"))
    assert np.array_equal(again[0], tok) and np.array_equal(again[1], lp)


# ---- 7. generated dropout --------------------------------------------------------------------------------------------------------------------
def test_generated_dropout(micro):
    kind, m, K = micro["kind"], micro["m1"], 2
    data = _data(kind, "A")
    batch, order, T = data
    B = order.shape[0]
    seed = 0xFEEDFACE1234
    args = _args(data)
    kw = dict(seed=seed, row0=ROW0, dropout="faithful", return_logp=True, slots_per_step=K)
    tok, lp = m.sample(*args, slot_policy="confident", **kw)
    R = m.sample_order()
    tok2, lp2 = m.sample(*args, slot_policy="confident", **kw)
    assert np.array_equal(tok, tok2) and np.array_equal(lp, lp2) and np.array_equal(m.sample_order(), R)
    _structure(data, tok, R)
    again = m.sample(batch["tokens"], batch["region"], batch["chain"], R, T, **kw)
    assert np.array_equal(again[0], tok) and np.array_equal(again[1], lp)
    _, lp_off = m.sample(*args, slot_policy="confident", **dict(kw, dropout="off"))
    assert np.abs(lp_off - lp).max() > 1e-2
    drop = ho.Dropout("philox", seed=seed, rows=np.arange(B) + ROW0, step=0)
    first = lambda state: np.asarray(micro["o1"](state, batch["region"], batch["chain"], dropout=drop)[:, :, :22], np.float64)
    _, cases = _check(micro, data, K, tok, lp, R, logits_fn=first, forwards=1, seed=seed, label="generated dropout, forward 0")
    assert cases == int(np.minimum(T, K).sum())


# ---- 8. lifetime and errors ------------------------------------------------------------------------------------------------------------------
def test_lifetime_and_errors(hip, micro):
    from hudiff_amd._lib import HD_ERR_INVALID, HD_ERR_STATE, HD_ERR_UNSUPPORTED, HudiffError
    kind, m, K = micro["kind"], micro["m0"], 2
    data = _data(kind, "A")
    batch, order, T = data
    B, tcap = order.shape
    args = _args(data)
    rkw = dict(KW, return_logp=True)
    conf = _confident(micro, "A", K)
    plain = m.sample(*args, **rkw)
    assert not np.array_equal(conf[1], plain[1])

    def same(a, b):
        return all(np.array_equal(x, y) for x, y in zip(a, b))

    def run(**kw):
        tok, lp = m.sample(*args, **dict(rkw, **kw))
        return tok, lp, m.sample_order()

    def raises(status, fn, *a, **k):
        with pytest.raises(HudiffError) as e:
            fn(*a, **k)
        assert e.value.status == status, e.value

    # one shot
    assert same(run(slots_per_step=K, slot_policy="confident"), conf)
    assert same(run(), plain + (order,))
    m.set_slot_policy("confident")
    m.set_slots_per_step(K)
    assert same(run(), conf) and same(run(), plain + (order,))
    # hd_forward neither uses nor clears it
    m.set_slot_policy("confident")
    m.set_slots_per_step(K)
    m(batch["tokens"][:2], batch["region"][:2], None if batch["chain"] is None else np.concatenate([batch["chain"][:2], batch["chain"][B:B + 2]]))
    raises(HD_ERR_STATE, m.sample_order, B, tcap)                # (hd_forward ended the last session's claim on the buffers)
    assert same(run(), conf)
    # inside a session; a restart puts the candidate list back and keeps the policy
    m.sample_begin(*args, slots_per_step=K, slot_policy="confident", record_logp=True, **KW)
    raises(HD_ERR_STATE, m.set_slot_policy, "given")
    assert np.array_equal(m.sample_order(), order)
    m.sample_run(0, tcap)
    assert same((m.sample_tokens(), m.sample_logp(), m.sample_order()), conf)
    m.sample_restart(SEED + 1)
    assert np.array_equal(m.sample_order(), order)
    m.sample_run(0, 4); m.sample_run(4, tcap)
    other, R1 = m.sample_tokens(), m.sample_order()
    assert not np.array_equal(other, conf[0])
    _structure(data, other, R1)
    m.sample_restart(SEED)
    m.sample_run(0, tcap)
    lp, R = m.sample_logp(), m.sample_order()
    assert same((m.sample_end(), lp, R), conf)
    assert same(run(), plain + (order,))
    # values
    raises(HD_ERR_INVALID, m.set_slot_policy, 2)
    raises(HD_ERR_INVALID, m.set_slot_policy, -1)
    with pytest.raises(ValueError):
        m.set_slot_policy("surest")
    assert same(run(), plain + (order,))
    # a slot repeated anywhere in a row's list (here: in two different groups)
    rep = order.copy()
    rep[21, 4] = rep[21, 1]
    bad = (batch["tokens"], batch["region"], batch["chain"], rep, T)
    raises(HD_ERR_INVALID, m.sample, *bad, slots_per_step=K, slot_policy="confident", **KW)
    assert same(run(), plain + (order,))                          # the failed begin left the handle on `given`
    m.sample(*bad, slots_per_step=K, **KW)                        # legal without the policy
    raises(HD_ERR_INVALID, m.sample, *bad, slot_policy="confident", **KW)
    m.sample(*bad, **KW)
    raises(HD_ERR_INVALID, m.score, conf[0], *bad[1:], slot_policy="confident")
    rep = order.copy()
    rep[17, 4] = rep[17, 1]                                       # (row 17 stops after three steps: position 4 is beyond its list)
    tok = m.sample(batch["tokens"], batch["region"], batch["chain"], rep, T, slots_per_step=K, slot_policy="confident", **KW)
    assert np.array_equal(tok, conf[0]) and np.array_equal(m.sample_order()[17], np.concatenate([conf[2][17, :3], rep[17, 3:]]))
    # injected masks
    raises(HD_ERR_UNSUPPORTED, m.sample, *args, slot_policy="confident", **dict(KW, dropout="inject"))
    assert same(run(), plain + (order,))
    raises(HD_ERR_UNSUPPORTED, m.score, conf[0], *args[1:], parallel=False, slot_policy="confident", dropout="inject")
    # hd_sample_order on a fresh handle
    fresh = _mk(hip, kind, load_cfg(kind), load_weights(kind))
    try:
        raises(HD_ERR_STATE, fresh.sample_order, B, tcap)
        fresh.sample(*args, **KW)
        assert np.array_equal(fresh.sample_order(), order)
    finally:
        fresh.close()


# ---- 9. guard repeat -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["ab", "nb"])
def test_lnsync_guard_repeats_a_confident_session(hip, kind):
    """Production width, the batch of the siblings' guard tests.  The repeat normalises in separate passes, so near-tied keys may
    legitimately swap against the undisturbed session: what is asserted is that the repeat started from the caller's list again (its
    order is a permutation of it) and that the replay invariant holds for the repeat's own order on the same handle, now off ln_sync."""
    from hudiff_amd import evalsets as E, synthetic as S
    cfg = dict(S.AB_CONFIG if kind == "ab" else S.NB_CONFIG, dropout=0.0)
    mx = _mk(hip, kind, cfg, S.random_state_dict(kind, cfg, seed=0), precision="split")
    try:
        big = E.eval_batch("huab348" if kind == "ab" else "vhh", 128 if kind == "ab" else 160, row0=0)
        T = np.minimum(big["T"], 4)
        args = (big["tokens"], big["region"], big["chain"], big["order"], T)
        kw = dict(seed=13, row0=0, return_logp=True)
        one = mx.sample(*args, **kw)
        prec(mx, lnsync_in_use=True, lnsync_fallbacks=0, last_call_repeated=False)
        mx.debug_fail_next_lnsync()
        with pytest.warns(RuntimeWarning, match="ln_sync"):
            tok, lp = mx.sample(*args, slots_per_step=2, slot_policy="confident", **kw)
        R = mx.sample_order()
        prec(mx, lnsync_in_use=False, lnsync_fallbacks=1, last_call_repeated=True)
        for b in range(len(T)):
            assert sorted(R[b, :T[b]].tolist()) == sorted(big["order"][b, :T[b]].tolist())
            assert np.array_equal(R[b, T[b]:], big["order"][b, T[b]:])
        again = mx.sample(big["tokens"], big["region"], big["chain"], R, T, slots_per_step=2, **kw)
        err = float(np.abs(again[1] - lp).max())
        print(f"{kind}: ln_sync guard in a confident session: |given at the repeat's order - repeat| {err:.2e}")
        assert np.array_equal(again[0], tok) and err < PAIR_TOL
        assert np.array_equal(mx.sample(*args, **kw)[0], one[0])          # the session after it is a plain one-slot session
        assert np.array_equal(mx.sample_order(), big["order"])
    finally:
        mx.close()


# ---- 10. CLIs --------------------------------------------------------------------------------------------------------------------------------
def _cli(kind):
    if kind == "ab":
        from hudiff_amd.cli import sample as cli
        return cli, _ab_checkpoint, "hudiffab.pt", ["--batch_size", "3", "--seed", "5"]
    from hudiff_amd.cli import nanosample as cli
    return cli, _nb_checkpoint, "hudiffnb.pt", ["--model", "finetune_vh", "--batch_size", "2", "--try_number", "3", "--seed", "4"]


def _outputs(out):
    return [open(out, "rb").read(), open(os.path.join(os.path.dirname(out), "sample_identity.fa"), "rb").read()]


@pytest.mark.parametrize("kind", ["ab", "nb"])
def test_cli_flag(hip, tmp_path, monkeypatch, kind):
    """--slot_policy given is the run without the flag, byte for byte.  With confident at K = 4 (dropout off) the sidecar totals are
    the recorded sums, and scoring the sampled tokens under the policy from each job's own list reproduces them (sweep 0 only for
    the nanobody sampler: a re-sweep redraws over filled tokens).  The score CLI with the flag writes one row per job."""
    from hudiff_amd import sampler
    from hudiff_amd.cli import score as score_cli
    from test_gpu_cli import _write_inputs
    cli, mk_ckpt, ck_name, base = _cli(kind)
    csv, nb = _write_inputs(tmp_path, kind, 4)
    outs = []
    for i, extra in enumerate(([], ["--slot_policy", "given"])):
        ck = tmp_path / f"one{i}" / "checkpoints" / ck_name
        mk_ckpt(ck)
        sidecar = tmp_path / f"logp{i}.csv"
        outs.append(_outputs(cli.main(["--ckpt", str(ck), "--data_fpath", str(csv), "--numbered_fpath", str(nb), "--logp_fpath", str(sidecar)]
                                      + base + extra)) + [open(sidecar, "rb").read()])
    assert outs[0] == outs[1]
    calls = []
    real = sampler.sample_jobs

    def recording(model, jobs, replicas, seed, **kw):
        res = real(model, jobs, replicas, seed, **kw)
        calls.append((list(jobs), dict(kw), res))
        return res
    monkeypatch.setattr(sampler, "sample_jobs", recording)
    if kind == "ab":
        monkeypatch.setattr(cli, "sample_jobs", recording)
    ck = tmp_path / "conf" / "checkpoints" / ck_name
    mk_ckpt(ck)
    sidecar = tmp_path / "logp_conf.csv"
    out = cli.main(["--ckpt", str(ck), "--data_fpath", str(csv), "--numbered_fpath", str(nb), "--logp_fpath", str(sidecar),
                    "--dropout", "off", "--slots_per_step", "4", "--slot_policy", "confident"] + base)
    monkeypatch.undo()
    assert open(out).read().count("humanization,") >= 4
    lines = open(sidecar).read().splitlines()[1:]
    assert calls and all(kw.get("slot_policy") == "confident" and kw.get("slots_per_step") == 4 and kw.get("return_logp") for _, kw, _ in calls)
    m = _mk(hip, kind, load_cfg(kind), load_weights(kind))
    totals = {}                                           # (name, sweep, replica) -> (T, total)
    try:
        for sweep, (jobs, kw, (res, res_lp)) in enumerate(calls):
            for a, job in enumerate(jobs):
                R, Tn = res.shape[2], len(job.loc)
                order = np.repeat(np.asarray(job.loc, np.int32)[None], R, 0)
                ch = None if kind == "nb" else np.array([job.chain[0]] * R + [job.chain[1]] * R, np.int32)
                lp = res_lp[a, 0]
                assert (lp[:, :Tn] < 0).all() and (lp[:, Tn:] == 0).all() and Tn > 20
                if sweep == 0:
                    sargs = (res[a, 0], np.repeat(job.region[None], R, 0), ch, order, np.full(R, Tn))
                    want = m.score(*sargs, slots_per_step=4, slot_policy="confident")
                    taken = m.sample_order()
                    err = float(np.abs(want - lp[:, :Tn]).max())
                    assert err < PAIR_TOL, (job.name, sweep, err)
                    assert all(sorted(taken[r].tolist()) == sorted(order[r].tolist()) for r in range(R))
                    assert not np.array_equal(taken, order)
                for r in range(R):
                    totals[(str(job.name), sweep, r)] = (Tn, float(lp[r].astype(np.float64).sum()))
        assert len(lines) == len(totals)
        for line in lines:
            f = line.split(",")
            key = (f[0], 0, int(f[2])) if kind == "ab" else (f[0], int(f[1]), int(f[3]))
            Tn, total = totals[key]
            assert int(f[-3]) == Tn and abs(float(f[-2]) - total) < 1e-6 + 1e-6 * abs(total), line
        # the score CLI with the flag
        if kind == "ab":
            csv.write_text("".join(l for l in open(csv).read().splitlines(True) if not l.startswith("human,")))
        mask = "pretrain" if kind == "ab" else "inpaint"
        sc = {}
        for policy in ("given", "confident"):
            sc[policy] = open(score_cli.main(["--ckpt", str(ck), "--kind", kind, "--data_fpath", str(csv), "--numbered_fpath", str(nb),
                                              "--seed", "8", "--mask", mask, "--out_fpath", str(tmp_path / f"scores_{policy}.csv"),
                                              "--slots_per_step", "4", "--slot_policy", policy])).read().splitlines()
        from hudiff_amd.cli.common import load_numbered
        jobs = score_cli.build_jobs(score_cli.read_rows(str(csv), kind), kind, mask, load_numbered(str(nb)), "auto")
        assert len(sc["confident"]) == 1 + len(jobs) and sc["confident"][0] == sc["given"][0]
        assert all(c.split(",")[:2] == g.split(",")[:2] and c != g for c, g in zip(sc["confident"][1:], sc["given"][1:]))
        with pytest.raises(SystemExit):
            score_cli.main(["--ckpt", str(ck), "--kind", kind, "--data_fpath", str(csv), "--orders", "2", "--slot_policy", "confident"])
    finally:
        m.close()
