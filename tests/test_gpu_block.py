"""Block decoding on the GPU (hd_set_slots_per_step): K slots of the visiting order per denoiser forward.

The definition replayed here (include/hudiff_hip.h "block decoding"): forward f runs the denoiser once on the current tokens and handles
the order positions t = f K + j; every live (b, t) is drawn from the hidden row of THAT forward with the noise, guide, target and logp
entry of position t.  Tolerances are the siblings' (tests/test_gpu_logp.py, tests/test_gpu_guide.py): a device log-probability is
within REF_TOL = 2e-4 of the float64 oracle, two device results within PAIR_TOL = 4e-4 of each other, and a drawn token can differ from
the oracle's only where the oracle's best two scores are closer than GAP_TOL = 4e-4; all divided by min(temperature, 1) when guided.

The library has no launch-tally id of its own for the block draw kernels (the table of ids is pinned by tests/test_host_logic.py
against tests/test_gpu_variants.py); the witness used here is the pruned tail: a one-slot session issues it (tail_sliced or
tail_launches > 0), a block session evaluates the last attention block for every row and issues none."""
import os

import numpy as np
import pytest

import hudiff_oracle as ho
from conftest import chain_or_none, load_cfg, load_golden, load_weights, prec
from test_gpu_guide import ALL, GAP_TOL, ROW0, SEED, _bits, _live, _oracle_batch, _visited
from test_gpu_logp import PAIR_TOL, REF_TOL, _ab_checkpoint, _load_prod, _mk, _nb_checkpoint, log_softmax64

pytestmark = pytest.mark.gpu

TRACE = {"ab": "micro_ab_sample_finetune.npz", "nb": "micro_nb_sample_plain.npz"}


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


_logits_cache, _batch_cache, _sample_cache = {}, {}, {}


def _batch(kind):
    if kind not in _batch_cache:
        _batch_cache[kind] = _oracle_batch(kind)
    return _batch_cache[kind]


def _logits64(micro, state, region, chain):
    """float64 [B, L, 22] of the float64 oracle at `state`; one forward per state, shared by every run that reaches it."""
    key = (micro["kind"], state.tobytes())
    if key not in _logits_cache:
        _logits_cache[key] = np.asarray(micro["o0"](state, region, chain)[:, :, :22], np.float64)
    return _logits_cache[key]


def _block_sample(micro, K, lanes=2, **kw):
    """(tokens, logp) of the block session of the oracle batch at dropout off; computed once per (kind, K, lanes)."""
    key = (micro["kind"], K, lanes, tuple(sorted(kw)))
    if kw or key not in _sample_cache:
        batch, order, T, _, _ = _batch(micro["kind"])
        res = micro["m0"].sample(batch["tokens"], batch["region"], batch["chain"], order, T, seed=SEED, row0=ROW0, dropout="off",
                                 lanes=lanes, return_logp=True, slots_per_step=K, **kw)
        if kw:
            return res
        _sample_cache[key] = res
    return _sample_cache[key]


def _pruned_tail(tally):
    return tally["tail_sliced"] + tally["tail_launches"]


def _replay(micro, tok, lp, K, allow=None, bias=None, temperature=1.0):
    """The definition, in float64: one oracle forward per group from the state at the group's start; every live (b, t) of the group is
    checked against that forward (drawn token, log-probability) and the DEVICE's token is written for the next group."""
    kind = micro["kind"]
    batch, order, T, _, _ = _batch(kind)
    B, tcap = order.shape
    scale = min(temperature, 1.0)
    state = batch["tokens"].copy()
    cases = left_out = 0
    worst_lp, smallest_gap = 0.0, np.inf
    for t0 in range(0, tcap, K):
        z = _logits64(micro, state, batch["region"], batch["chain"])
        nxt = state.copy()
        for t in range(t0, min(t0 + K, tcap)):
            q = ho.philox_exp_noise(SEED, ROW0 + np.arange(B), t).astype(np.float64)
            for b in range(B):
                if t >= T[b]:
                    continue
                s = order[b, t]
                ok = np.ones(22, bool) if allow is None else _bits(allow[b, s], np.arange(22))
                g = np.where(ok, (z[b, s] + (0.0 if bias is None else bias[b, s].astype(np.float64))) / temperature, -np.inf)
                lsm = g - g.max()
                lsm = lsm - np.log(np.exp(lsm).sum())
                score = np.where(ok, g - np.log(q[b]), -np.inf)
                got = int(tok[b, s])
                worst_lp = max(worst_lp, abs(float(lp[b, t]) - lsm[got]))
                top = np.sort(score[ok])[::-1]
                gap = top[0] - top[1] if len(top) > 1 else np.inf
                smallest_gap = min(smallest_gap, gap)
                cases += 1
                if gap < GAP_TOL / scale:
                    left_out += 1
                else:
                    assert got == int(np.argmax(score)), (b, t, got, int(np.argmax(score)), gap)
                nxt[b, s] = got
        state = nxt
    print(f"{kind} K {K} temperature {temperature}: {cases} draws, {left_out} left out, smallest oracle gap {smallest_gap:.2e}, "
          f"|logp - oracle| {worst_lp:.2e} (bound {REF_TOL / scale:.1e})")
    assert cases == int(T.sum()) == 231
    assert left_out <= 2
    assert worst_lp < REF_TOL / scale
    return state


# ---- 1. K = 1 is today's session -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["ab", "nb"])
def test_one_slot_per_step_is_todays_session(hip, kind):
    z = load_golden(TRACE[kind])
    tokens, region, chain, loc, q, final = z["tokens"], z["region"], chain_or_none(z), z["loc"], z["q"], z["final"]
    B = tokens.shape[0]
    order, T = np.repeat(loc[None], B, 0), np.full(B, len(loc))
    m = _mk(hip, kind, load_cfg(kind), load_weights(kind))
    try:
        m.debug_launch_tally()
        tok1, lp1 = m.sample(tokens, region, chain, order, T, q_noise=q, return_logp=True, slots_per_step=1)
        tally = m.debug_launch_tally()
        tok0, lp0 = m.sample(tokens, region, chain, order, T, q_noise=q, return_logp=True)
        assert np.array_equal(tok1, final)
        assert np.array_equal(tok1, tok0) and np.array_equal(lp1, lp0)
        assert np.array_equal(m.sample(tokens, region, chain, order, T, q_noise=q, slots_per_step=1), final)
        assert _pruned_tail(tally) > 0, tally
        # ... and the block session of the same inputs is another session: no pruned tail is issued
        m.debug_launch_tally()
        tokb = m.sample(tokens, region, chain, order, T, q_noise=q, slots_per_step=4)
        tally = m.debug_launch_tally()
        assert _pruned_tail(tally) == 0 and tally["sample_lanes_1"] > 0, tally
        assert np.array_equal(tokb == 22, final == 22)
        assert np.array_equal(m.sample(tokens, region, chain, order, T, q_noise=q), final)
    finally:
        m.close()


# ---- 2. against an oracle loop ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lanes", [1, 2])
@pytest.mark.parametrize("K", [2, 3, 4, 8])
def test_block_draw_against_an_oracle_loop(micro, K, lanes):
    batch, order, T, _, _ = _batch(micro["kind"])
    tcap = order.shape[1]
    micro["m0"].debug_launch_tally()
    tok, lp = micro["m0"].sample(batch["tokens"], batch["region"], batch["chain"], order, T, seed=SEED, row0=ROW0, dropout="off",
                                 lanes=lanes, return_logp=True, slots_per_step=K)
    tally = micro["m0"].debug_launch_tally()
    assert _pruned_tail(tally) == 0 and tally[f"sample_lanes_{lanes}"] > 0, tally
    cached = _block_sample(micro, K, lanes)               # (what the other tests use is this session's result)
    assert np.array_equal(cached[0], tok) and np.array_equal(cached[1], lp)
    live, vis = _live(T, tcap), _visited(order, T, tok.shape[1])
    assert (lp[~live] == 0).all() and (lp[live] < 0).all()
    assert np.array_equal(tok[~vis], batch["tokens"][~vis]) and np.array_equal(tok[5], batch["tokens"][5])
    assert not (tok[vis] == 22).any()
    final = _replay(micro, tok, lp, K)
    assert np.array_equal(final, tok)
    # the plain (not recording) block kernel draws the same tokens
    plain = micro["m0"].sample(batch["tokens"], batch["region"], batch["chain"], order, T, seed=SEED, row0=ROW0, dropout="off",
                               lanes=lanes, slots_per_step=K)
    assert np.array_equal(plain, tok)


# ---- 3. launch forms -----------------------------------------------------------------------------------------------------------------
def test_launch_forms_agree_bit_for_bit(hip, micro):
    kind, K = micro["kind"], 3
    batch, order, T, _, _ = _batch(kind)
    B, tcap = order.shape
    args = (batch["tokens"], batch["region"], batch["chain"], order, T)
    kw = dict(seed=SEED, row0=ROW0, dropout="off")
    m = micro["m0"]
    want_tok, want_lp = _block_sample(micro, K)
    got = {"eager": m.sample(*args, return_logp=True, slots_per_step=K, graph=False, **kw),
           "loop": m.sample(*args, return_logp=True, slots_per_step=K, graph="loop", **kw)}
    m2 = _mk(hip, kind, load_cfg(kind), load_weights(kind), options={"lane_min_rows": 2})
    try:
        got["lanes2"] = m2.sample(*args, return_logp=True, slots_per_step=K, lanes=2, **kw)
    finally:
        m2.close()
    m.sample_begin(*args, record_logp=True, slots_per_step=K, **kw)
    m.sample_run(0, 3)
    part = m.sample_logp()
    assert (part[:, 3:] == 0).all()
    m.sample_run(3, 6)
    assert m.last_run_ms()[1] == 3                        # order positions; one forward
    lp = m.sample_logp()
    got["split_call"] = (m.sample_end(), lp)
    q = np.stack([ho.philox_exp_noise(SEED, ROW0 + np.arange(B), t) for t in range(tcap)])
    got["q_noise"] = m.sample(*args, return_logp=True, slots_per_step=K, q_noise=q, **dict(kw, seed=1))
    for name, (tok, lp) in got.items():
        assert np.array_equal(tok, want_tok), name
        assert np.array_equal(lp, want_lp), name


# ---- 4. scoring -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [2, 4])
def test_scoring_a_block_session(micro, K):
    kind, m = micro["kind"], micro["m0"]
    batch, order, T, _, _ = _batch(kind)
    B, tcap = order.shape
    tok, lp = _block_sample(micro, K)
    args = (batch["region"], batch["chain"], order, T)
    seq = m.score(tok, *args, parallel=False, slots_per_step=K)
    par = m.score(tok, *args, parallel=True, device_batch=100, slots_per_step=K)
    one = m.score(tok, *args, parallel=False)
    live = _live(T, tcap)
    e = {"seq-par": np.abs(seq - par).max(), "seq-rec": np.abs(seq - lp).max(), "par-rec": np.abs(par - lp).max()}
    # the oracle: float64 log_softmax of the forward each group was drawn from
    want = np.zeros((B, tcap))
    state = batch["tokens"].copy()
    for t0 in range(0, tcap, K):
        lsm = log_softmax64(_logits64(micro, state, batch["region"], batch["chain"]))
        nxt = state.copy()
        for t in range(t0, min(t0 + K, tcap)):
            for b in np.flatnonzero(T > t):
                s = order[b, t]
                want[b, t] = lsm[b, s, tok[b, s]]
                nxt[b, s] = tok[b, s]
        state = nxt
    e_ref = {"seq": np.abs(seq - want).max(), "par": np.abs(par - want).max(), "rec": np.abs(lp - want).max()}
    first = (np.arange(tcap) % K == 0)[None, :] & live
    e_first, e_rest = np.abs(one - seq)[first].max(), np.abs(one - seq)[live & ~first].max()
    print(f"{kind} K {K}: " + "  ".join(f"|{k}| {v:.2e}" for k, v in e.items()) + "  oracle: " +
          "  ".join(f"{k} {v:.2e}" for k, v in e_ref.items()) + f"  K=1 score at t % K == 0: {e_first:.2e}, elsewhere up to {e_rest:.2e}")
    assert all(v < PAIR_TOL for v in e.values()), e
    assert all(v < REF_TOL for v in e_ref.values()), e_ref
    assert (seq[~live] == 0).all() and (par[~live] == 0).all() and (seq[live] < 0).all()
    assert e_first < PAIR_TOL and e_rest > 1e-2


# ---- 5. against the library's own forward, production width ------------------------------------------------------------------------------
@pytest.mark.parametrize("route", ["split", "f32_all"])
@pytest.mark.parametrize("kind", ["ab", "nb"])
def test_production_width_against_the_librarys_forward(hip, kind, route):
    K, groups = 4, 3
    z, cfg, sd = _load_prod(kind)
    chain = z["chain"] if z["chain"].size else None
    final, order, T = z["final"], z["order"], z["T"]
    B = final.shape[0]
    m = _mk(hip, kind, cfg, sd, precision=route)
    try:
        got = m.score(final, z["region"], chain, order, T, parallel=False, slots_per_step=K)
        worst = 0.0
        for f in range(groups):
            state = final.copy()
            for b in range(B):
                state[b, order[b, K * f:T[b]]] = 22
            lsm = log_softmax64(m.forward(state, z["region"], chain, dropout="off")[:, :, :22])
            for b in range(B):
                for t in range(K * f, min(K * f + K, int(T[b]))):
                    s = order[b, t]
                    worst = max(worst, abs(float(got[b, t]) - lsm[b, s, final[b, s]]))
        print(f"{kind} {route}: |score(K = 4) - log_softmax(forward)| over the first {groups} groups = {worst:.2e}")
        assert (T >= K * groups).all() and worst < PAIR_TOL
        assert (got[~_live(T, order.shape[1])] == 0).all()
    finally:
        m.close()


# ---- 6. guide and block together ------------------------------------------------------------------------------------------------------
def test_guide_and_block_together(micro):
    from hudiff_amd import Guide
    kind, m, K = micro["kind"], micro["m0"], 3
    batch, order, T, allow, bias = _batch(kind)
    B, L = batch["tokens"].shape
    args = (batch["tokens"], batch["region"], batch["chain"], order, T)
    kw = dict(seed=SEED, row0=ROW0, dropout="off", return_logp=True, slots_per_step=K)
    want_tok, want_lp = _block_sample(micro, K)
    neutral = Guide(np.full((B, L), ALL, np.uint32), np.zeros((B, L, 22), np.float32), 1.0)
    tok, lp = m.sample(*args, guide=neutral, **kw)
    assert np.array_equal(tok, want_tok) and np.array_equal(lp, want_lp)
    s0 = m.score(want_tok, *args[1:], parallel=False, slots_per_step=K)
    assert np.array_equal(m.score(want_tok, *args[1:], parallel=False, slots_per_step=K, guide=neutral), s0)
    # singletons
    vis, live = _visited(order, T, L), _live(T, order.shape[1])
    want = np.random.default_rng(8).integers(0, 22, (B, L))
    tok, lp = m.sample(*args, guide=Guide((1 << want).astype(np.uint32), bias, 1.0), **kw)
    assert np.array_equal(tok[vis], want[vis]) and np.array_equal(tok[~vis], batch["tokens"][~vis]) and (lp == 0.0).all()
    # the random guide at temperature 0.5
    g = Guide(allow, bias, 0.5)
    tok, lp = m.sample(*args, guide=g, **kw)
    assert _bits(allow[vis], tok[vis]).all() and np.array_equal(tok[~vis], batch["tokens"][~vis])
    assert (lp[~live] == 0).all()
    _replay(micro, tok, lp, K, allow, bias, 0.5)
    seq = m.score(tok, *args[1:], parallel=False, slots_per_step=K, guide=g)
    par = m.score(tok, *args[1:], parallel=True, device_batch=100, slots_per_step=K, guide=g)
    assert np.abs(seq - lp).max() < PAIR_TOL / 0.5 and np.abs(par - lp).max() < PAIR_TOL / 0.5


# ---- 7. generated dropout ----------------------------------------------------------------------------------------------------------------
def test_generated_dropout(micro):
    kind, m, K = micro["kind"], micro["m1"], 2
    batch, order, T, _, _ = _batch(kind)
    B, tcap = order.shape
    seed = 0xFEEDFACE1234
    args = (batch["tokens"], batch["region"], batch["chain"], order, T)
    kw = dict(seed=seed, dropout="faithful", return_logp=True, slots_per_step=K)
    tok, lp = m.sample(*args, row0=ROW0, **kw)
    tok2, lp2 = m.sample(*args, row0=ROW0, **kw)
    assert np.array_equal(tok, tok2) and np.array_equal(lp, lp2)
    tok_off, lp_off = m.sample(*args, row0=ROW0, **dict(kw, dropout="off"))
    assert not np.array_equal(lp_off, lp) and np.abs(lp_off - lp).max() > 1e-2
    # rows are keyed by row0 + b: the two halves, sampled apart, are the 40-row run
    for lo, hi in ((0, 20), (20, 40)):
        ch = None if batch["chain"] is None else np.concatenate([batch["chain"][lo:hi], batch["chain"][B + lo:B + hi]])
        th, lph = m.sample(batch["tokens"][lo:hi], batch["region"][lo:hi], ch, order[lo:hi], T[lo:hi], row0=ROW0 + lo, lanes=1, **kw)
        print(f"{kind} rows {lo}:{hi} apart: tokens equal {np.array_equal(th, tok[lo:hi])}, |logp - 40-row run| {np.abs(lph - lp[lo:hi]).max():.2e}")
        # (a launch of 20 rows may pick other GEMM tiles than a lane of the 40-row run: two device results, as in tests/test_gpu_logp.py)
        assert np.array_equal(th, tok[lo:hi])
        assert np.abs(lph - lp[lo:hi]).max() < PAIR_TOL
    # the masks of forward f are keyed by step = f K
    state = batch["tokens"].copy()
    for f in range(2):
        drop = ho.Dropout("philox", seed=seed, rows=np.arange(B) + ROW0, step=f * K)
        lsm = log_softmax64(micro["o1"](state, batch["region"], batch["chain"], dropout=drop)[:, :, :22])
        worst = 0.0
        for t in range(f * K, f * K + K):
            for b in np.flatnonzero(T > t):
                s = order[b, t]
                worst = max(worst, abs(float(lp[b, t]) - lsm[b, s, tok[b, s]]))
        print(f"{kind}: generated dropout, group {f} (step {f * K}): |logp - oracle| = {worst:.2e}")
        assert worst < REF_TOL
        for t in range(f * K, f * K + K):
            for b in np.flatnonzero(T > t):
                state[b, order[b, t]] = tok[b, order[b, t]]


# ---- 8. lifetime and errors --------------------------------------------------------------------------------------------------------------
def test_lifetime_and_errors(hip, micro):
    from hudiff_amd._lib import HD_ERR_INVALID, HD_ERR_STATE, HD_ERR_UNSUPPORTED, HudiffError
    kind, m = micro["kind"], micro["m0"]
    batch, order, T, _, _ = _batch(kind)
    B, tcap = order.shape
    args = (batch["tokens"], batch["region"], batch["chain"], order, T)
    kw = dict(seed=SEED, row0=ROW0, dropout="off")
    # (with these weights a block session happens to draw the one-slot session's tokens; the recorded log-probabilities tell them apart)
    rkw = dict(kw, return_logp=True)
    plain = m.sample(*args, **rkw)
    block = _block_sample(micro, 2)
    assert np.abs(block[1] - plain[1]).max() > 1e-2

    def same(a, b):
        return np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])

    def raises(status, fn, *a, **k):
        with pytest.raises(HudiffError) as e:
            fn(*a, **k)
        assert e.value.status == status, e.value

    # one shot
    assert same(m.sample(*args, slots_per_step=2, **rkw), block)
    assert same(m.sample(*args, **rkw), plain)
    m.set_slots_per_step(2)
    assert same(m.sample(*args, **rkw), block) and same(m.sample(*args, **rkw), plain)
    # hd_forward neither uses nor clears it
    m.set_slots_per_step(2)
    m(batch["tokens"][:2], batch["region"][:2], None if batch["chain"] is None else np.concatenate([batch["chain"][:2], batch["chain"][B:B + 2]]))
    assert same(m.sample(*args, **rkw), block)
    # a restart keeps K; K cannot be set inside a session; run takes whole groups
    m.sample_begin(*args, slots_per_step=2, record_logp=True, **kw)
    raises(HD_ERR_STATE, m.set_slots_per_step, 3)
    raises(HD_ERR_INVALID, m.sample_run, 1, 6)
    raises(HD_ERR_INVALID, m.sample_run, 0, 3)
    m.sample_run(0, tcap)
    assert same((m.sample_tokens(), m.sample_logp()), block)
    m.sample_restart(SEED + 1)
    m.sample_run(0, 4); m.sample_run(4, tcap)
    other = m.sample_tokens()
    assert not np.array_equal(other, block[0]) and not (other[_visited(order, T, other.shape[1])] == 22).any()
    m.sample_restart(SEED)
    m.sample_run(0, tcap)
    lp = m.sample_logp()
    assert same((m.sample_end(), lp), block)
    assert same(m.sample(*args, **rkw), plain)
    # K = 8 > Tmax = 6: t1 = Tmax is the one legal end
    m.sample_begin(*args, slots_per_step=8, record_logp=True, **kw)
    raises(HD_ERR_INVALID, m.sample_run, 0, 4)
    m.sample_run(0, tcap)
    lp = m.sample_logp()
    assert same((m.sample_end(), lp), _block_sample(micro, 8))
    # values outside [1, 64]
    raises(HD_ERR_INVALID, m.set_slots_per_step, 0)
    raises(HD_ERR_INVALID, m.set_slots_per_step, 65)
    raises(HD_ERR_INVALID, m.sample, *args, slots_per_step=0, **kw)
    raises(HD_ERR_INVALID, m.sample, *args, slots_per_step=65, **kw)
    assert same(m.sample(*args, **rkw), plain)
    # a slot repeated inside one group: an error at K = 2, legal at K = 1 (and at K = 2 when the repeat falls into two groups)
    rep = order.copy()
    rep[21, 3] = rep[21, 2]
    raises(HD_ERR_INVALID, m.sample, batch["tokens"], batch["region"], batch["chain"], rep, T, slots_per_step=2, **kw)
    assert same(m.sample(*args, **rkw), plain)                   # the failed begin left the handle on K = 1
    m.sample(batch["tokens"], batch["region"], batch["chain"], rep, T, **kw)
    rep = order.copy()
    rep[21, 2] = rep[21, 1]
    m.sample(batch["tokens"], batch["region"], batch["chain"], rep, T, slots_per_step=2, **kw)
    rep[17, 3] = rep[17, 2]                                      # (row 17 stops after three steps: position 3 is never visited)
    m.sample(batch["tokens"], batch["region"], batch["chain"], rep, T, slots_per_step=2, **kw)
    # injected masks
    raises(HD_ERR_UNSUPPORTED, m.sample, *args, slots_per_step=2, **dict(kw, dropout="inject"))
    assert same(m.sample(*args, **rkw), plain)
    raises(HD_ERR_UNSUPPORTED, m.score, block[0], *args[1:], parallel=False, slots_per_step=2, dropout="inject")
    assert same(m.sample(*args, **rkw), plain)


@pytest.mark.parametrize("kind", ["ab", "nb"])
def test_lnsync_guard_repeats_a_block_session(hip, kind):
    """Production width (the micro models' launches hold no ln_sync meeting), the batch of tests/test_gpu_x3.py's guard test: the
    repeat of a K = 2 session is a K = 2 session -- its tokens and, within PAIR_TOL (the repeat normalises in separate passes), its
    log-probabilities, which are not the one-slot session's."""
    from hudiff_amd import evalsets as E, synthetic as S
    cfg = dict(S.AB_CONFIG if kind == "ab" else S.NB_CONFIG, dropout=0.0)
    mx = _mk(hip, kind, cfg, S.random_state_dict(kind, cfg, seed=0), precision="split")
    try:
        big = E.eval_batch("huab348" if kind == "ab" else "vhh", 128 if kind == "ab" else 160, row0=0)
        args = (big["tokens"], big["region"], big["chain"], big["order"], np.minimum(big["T"], 4))
        kw = dict(seed=13, row0=0, return_logp=True)
        one = mx.sample(*args, **kw)
        want = mx.sample(*args, slots_per_step=2, **kw)
        assert np.abs(want[1] - one[1]).max() > 2 * PAIR_TOL          # (or the check below could not tell the two sessions apart)
        info = prec(mx, lnsync_in_use=True, lnsync_fallbacks=0, last_call_repeated=False)
        mx.debug_fail_next_lnsync()
        with pytest.warns(RuntimeWarning, match="ln_sync"):
            again = mx.sample(*args, slots_per_step=2, **kw)
        prec(mx, lnsync_in_use=False, lnsync_fallbacks=1, last_call_repeated=True)
        err = float(np.abs(again[1] - want[1]).max())
        print(f"{kind}: ln_sync guard in a block session: |repeat - undisturbed| {err:.2e}, |K = 2 - K = 1| {np.abs(want[1] - one[1]).max():.2e}")
        assert np.array_equal(again[0], want[0]) and err < PAIR_TOL
        assert np.abs(again[1] - one[1]).max() > PAIR_TOL
        assert np.array_equal(mx.sample(*args, **kw)[0], one[0])          # the session after it is a one-slot session
    finally:
        mx.close()


# ---- 9. CLIs ----------------------------------------------------------------------------------------------------------------------------
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
    """--slots_per_step 1 is the run without the flag, byte for byte.  With 4 (dropout off) the sidecar has one line per sampled row, its
    T the row's steps and its value the sum of that many recorded log-probabilities; scoring the sampled tokens along the sampler's own
    order with the same block size reproduces every one of them within PAIR_TOL (the sidecar rounds a total to 1e-6).  The score CLI
    draws its own orders, so it is compared with model.score(slots_per_step=4) along those orders, as tests/test_gpu_logp.py does."""
    from hudiff_amd import sampler, scoring
    from hudiff_amd.cli import score as score_cli
    from hudiff_amd.cli.common import load_numbered
    from test_gpu_cli import _write_inputs
    cli, mk_ckpt, ck_name, base = _cli(kind)
    csv, nb = _write_inputs(tmp_path, kind, 4)
    outs = []
    for i, extra in enumerate(([], ["--slots_per_step", "1"])):
        ck = tmp_path / f"one{i}" / "checkpoints" / ck_name
        mk_ckpt(ck)
        sidecar = tmp_path / f"logp{i}.csv"
        outs.append(_outputs(cli.main(["--ckpt", str(ck), "--data_fpath", str(csv), "--numbered_fpath", str(nb), "--logp_fpath", str(sidecar)]
                                      + base + extra)) + [open(sidecar, "rb").read()])
    assert outs[0] == outs[1]
    # K = 4, dropout off; every call of sample_jobs is kept
    calls = []
    real = sampler.sample_jobs

    def recording(model, jobs, replicas, seed, **kw):
        res = real(model, jobs, replicas, seed, **kw)
        calls.append((list(jobs), dict(kw), res))
        return res
    monkeypatch.setattr(sampler, "sample_jobs", recording)
    if kind == "ab":
        monkeypatch.setattr(cli, "sample_jobs", recording)
    ck = tmp_path / "block" / "checkpoints" / ck_name
    mk_ckpt(ck)
    sidecar = tmp_path / "logp_block.csv"
    out = cli.main(["--ckpt", str(ck), "--data_fpath", str(csv), "--numbered_fpath", str(nb), "--logp_fpath", str(sidecar),
                    "--dropout", "off", "--slots_per_step", "4"] + base)
    monkeypatch.undo()
    assert open(out).read().count("humanization,") >= 4
    lines = open(sidecar).read().splitlines()[1:]
    assert calls and all(kw.get("slots_per_step") == 4 and kw.get("return_logp") for _, kw, _ in calls)
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
                if sweep == 0:                            # (a re-sweep of the nanobody sampler redraws over filled tokens: nothing is masked)
                    want = m.score(res[a, 0], np.repeat(job.region[None], R, 0), ch, order, np.full(R, Tn), parallel=False, slots_per_step=4)
                    err = float(np.abs(want - lp[:, :Tn]).max())
                    assert err < PAIR_TOL, (job.name, sweep, err)
                    one = m.score(res[a, 0], np.repeat(job.region[None], R, 0), ch, order, np.full(R, Tn), parallel=False)
                    assert np.abs(one - want).max() > 1e-2
                for r in range(R):
                    totals[(str(job.name), sweep, r)] = (Tn, float(lp[r].astype(np.float64).sum()))
        assert len(lines) == len(totals)
        for line in lines:
            f = line.split(",")
            key = (f[0], 0, int(f[2])) if kind == "ab" else (f[0], int(f[1]), int(f[3]))
            Tn, total = totals[key]
            assert int(f[-3]) == Tn and abs(float(f[-2]) - total) < 1e-6 + 1e-6 * abs(total), line
        # the score CLI with the same flag
        if kind == "ab":
            csv.write_text("".join(l for l in open(csv).read().splitlines(True) if not l.startswith("human,")))
        mask = "pretrain" if kind == "ab" else "inpaint"
        sc = {}
        for K in (1, 4):
            sc[K] = open(score_cli.main(["--ckpt", str(ck), "--kind", kind, "--data_fpath", str(csv), "--numbered_fpath", str(nb), "--orders", "2",
                                         "--seed", "8", "--mask", mask, "--out_fpath", str(tmp_path / f"scores{K}.csv")]
                                        + (["--slots_per_step", "4"] if K == 4 else []))).read().splitlines()
        rows = score_cli.read_rows(str(csv), kind)
        jobs = score_cli.build_jobs(rows, kind, mask, load_numbered(str(nb)), "auto")
        assert len(sc[4]) == 1 + len(jobs) and sc[4] != sc[1]
        for j, job in enumerate(jobs):
            orders = scoring.draw_orders(job.loc, 2, 8, j)
            ch = None if kind == "nb" else np.array([job.chain[0]] * 2 + [job.chain[1]] * 2, np.int32)
            lp = m.score(np.repeat(job.tokens[None], 2, 0), np.repeat(job.region[None], 2, 0), ch, orders, np.full(2, len(job.loc)), slots_per_step=4)
            tot = lp.astype(np.float64).sum(axis=1)
            name, Tn, mean, std, per = sc[4][1 + j].split(",")
            assert name == job.name and int(Tn) == len(job.loc)
            assert abs(float(mean) - tot.mean()) < len(job.loc) * PAIR_TOL and abs(float(per) - tot.mean() / len(job.loc)) < PAIR_TOL
    finally:
        m.close()
