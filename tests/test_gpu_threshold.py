"""The confidence threshold on the GPU (hd_set_confidence, include/hudiff_hip.h "confidence threshold"): a forward fills every remaining
slot of a row whose top probability is at least tau -- at least one, at most K.

Three yardsticks, each for what it can decide:
  * bit-exact equivalences: with every finite key qualifying (tau = 0.04 <= 1/22) the session IS the confident K-session, with none
    qualifying (tau = 1 on a model whose distributions are never a point mass) it IS the confident 1-session;
  * the device's own keys (hd_sample_keys) for the RULE: a session driven one forward at a time must realise, bit for bit, the count and
    the permutation guide.threshold_select gives on the keys the device itself formed -- no near-tie exemption;
  * the float64 oracle for the KEYS and the log-probabilities: within REF_TOL in log space (divided by min(temperature, 1) when guided),
    the siblings' bound for a device log-probability.  The count is NOT judged against the oracle's keys: in a float64 simulation of
    these loops up to 0.33 % of the keys lay within 4e-4 of log cmax.
That simulation (oracle draws, K = 4, batch A) gave the per-row count histograms  ab: 117 / 13 / 12 / 13 (counts 1 / 2 / 3 / 4),
nb: 137 / 17 / 16 / 3; on batch L at K = 64 counts from 1 to 38 or 39, and 64, in 97 (ab) and 30 (nb) forwards.
Exact logits (tests/threshold_cases.py, decided on the CPU by tests/test_threshold_host.py) hold counts, orders and fwd exactly."""
import numpy as np
import pytest

import draw_cases as DC
import threshold_cases as TC
from conftest import load_cfg, load_weights, prec
from hudiff_amd.guide import confidence_cmax, confidence_keys, guided_log_probs, threshold_select
from test_gpu_adaptive import KW, _args, _confident, _data, _structure
from test_gpu_block import _batch, _logits64
from test_gpu_guide import ROW0, SEED, _live
from test_gpu_logp import PAIR_TOL, REF_TOL, _load_prod, _mk, log_softmax64

pytestmark = pytest.mark.gpu

ALL_QUALIFY = 0.04                                       # cmax = 25 > 22 >= every finite key
TAU = {"ab": 0.11, "nb": 0.14}                           # near the median of the oracle's forward-0 keys


@pytest.fixture(scope="module")
def hip():
    import hudiff_amd
    if hudiff_amd.device_count() < 1:
        pytest.fail("no MI355X visible: GPU tests must run on the GPU box (there is no CPU fallback)")
    return hudiff_amd


@pytest.fixture(scope="module", params=["ab", "nb"])
def micro(request, hip):
    import hudiff_oracle as ho
    kind = request.param
    cfg, sd = load_cfg(kind), load_weights(kind)
    p = 0.2 if kind == "ab" else 0.5
    models = {"kind": kind, "p": p, "m0": _mk(hip, kind, cfg, sd), "m1": _mk(hip, kind, dict(cfg, dropout=p), sd),
              "o0": ho.OracleNet(kind, cfg, sd, dtype=np.float64)}
    yield models
    models["m0"].close(); models["m1"].close()


@pytest.fixture(scope="module")
def handles(hip):
    cache = {}

    def get(kind, table="main"):
        if (kind, table) not in cache:
            cache[kind, table] = _mk(hip, kind, load_cfg(kind), DC.decoder_state(load_weights(kind), table), options={"lane_min_rows": 2})
        return cache[kind, table]
    yield get
    for m in cache.values():
        m.close()


def _want_fwd(T, tcap, K):
    t = np.arange(tcap)[None, :]
    return np.where(t < np.asarray(T)[:, None], t // K, -1).astype(np.int32)


def _run(m, data, K, tau, **kw):
    """(tokens, logp, order, fwd, filled) of a recording threshold session through hd_sample."""
    tok, lp = m.sample(*_args(data), return_logp=True, slots_per_step=K, slot_policy="confident", confidence=tau, **dict(KW, **kw))
    return tok, lp, m.sample_order(), m.sample_forwards(), m.sample_progress()


def _same(a, b):
    return len(a) == len(b) and all(np.array_equal(x, y) for x, y in zip(a, b))


# ---- 1. bit-exact equivalences -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,K,lanes", [("A", 1, 1), ("A", 1, 2), ("A", 2, 1), ("A", 2, 2), ("A", 4, 1), ("A", 4, 2), ("L", 64, 2)])
def test_every_key_qualifying_is_the_confident_session(micro, name, K, lanes):
    data = _data(micro["kind"], name)
    _, order, T = data
    want = _confident(micro, name, K, lanes)
    tok, lp, R, fwd, filled = _run(micro["m0"], data, K, ALL_QUALIFY, lanes=lanes)
    assert np.array_equal(tok, want[0]) and np.array_equal(lp, want[1]) and np.array_equal(R, want[2])
    assert np.array_equal(fwd, _want_fwd(T, order.shape[1], K)) and np.array_equal(filled, T)


def test_no_key_qualifying_is_the_one_slot_session(micro):
    kind = micro["kind"]
    data = _data(kind, "A")
    _, order, T = data
    want = _confident(micro, "A", 1)
    tok, lp, R, fwd, filled = _run(micro["m0"], data, 4, 1.0)
    assert np.array_equal(tok, want[0]) and np.array_equal(lp, want[1]) and np.array_equal(R, want[2])
    assert np.array_equal(fwd, _want_fwd(T, order.shape[1], 1)) and np.array_equal(filled, T)
    # generated dropout: forward f is keyed by step = f, as position f of the one-slot session is
    m = micro["m1"]
    kw = dict(seed=0xFEEDFACE1234, row0=ROW0, dropout="faithful", return_logp=True, slot_policy="confident")
    one = m.sample(*_args(data), **kw)
    R1 = m.sample_order()
    got = m.sample(*_args(data), slots_per_step=4, confidence=1.0, **kw)
    assert np.array_equal(got[0], one[0]) and np.array_equal(got[1], one[1]) and np.array_equal(m.sample_order(), R1)
    assert np.array_equal(m.sample_forwards(), _want_fwd(T, order.shape[1], 1))
    assert np.abs(one[1] - want[1]).max() > 1e-2             # (the masks did something)


# ---- 2. the selection against the device's own keys, the keys against the oracle ------------------------------------------------------------
def _drive(micro, data, K, tau, guide=None, allow=None, bias=None, temperature=1.0, oracle_every=1, label=""):
    m, kind = micro["m0"], micro["kind"]
    batch, order, T = data
    B, tcap = order.shape
    scale = min(temperature, 1.0) if temperature > 0 else 1.0
    cmax = confidence_cmax(tau)
    m.sample_begin(*_args(data), record_logp=True, slots_per_step=K, slot_policy="confident", confidence=tau, guide=guide, **KW)
    state, cur, filled = batch["tokens"].copy(), m.sample_order(), m.sample_progress()
    assert np.array_equal(cur, order) and (filled == 0).all() and (m.sample_forwards() == -1).all()
    counts, f, worst_key, worst_lp, checked = [], 0, 0.0, 0.0, 0
    while (filled < T).any():
        assert f < tcap
        m.sample_run(f, f + 1)
        keys, new, prog, fwd, tok, lp = m.sample_keys(), m.sample_order(), m.sample_progress(), m.sample_forwards(), m.sample_tokens(), m.sample_logp()
        assert m.last_run_ms()[1] == 1
        z = _logits64(micro, state, batch["region"], batch["chain"]) if f % oracle_every == 0 else None
        for b in range(B):
            n, Tb = int(filled[b]), int(T[b])
            if Tb - n <= 0:
                assert prog[b] == n and np.array_equal(new[b], cur[b]) and np.array_equal(tok[b], state[b])
                continue
            c = keys[b, n:Tb]
            assert np.isfinite(c).all() and (c >= 1.0).all() and (c <= 22.0 * (1 + 1e-6)).all()
            chosen, cnt, perm = threshold_select(c, K, cmax)
            assert prog[b] == n + cnt, (label, f, b, int(prog[b]), n, cnt)
            assert np.array_equal(new[b, n:Tb], cur[b, n:Tb][perm]), (label, f, b)
            assert np.array_equal(new[b, :n], cur[b, :n]) and np.array_equal(new[b, Tb:], cur[b, Tb:])
            assert (fwd[b, n:n + cnt] == f).all() and (fwd[b, n + cnt:] == -1).all() and (fwd[b, :n] >= 0).all() and (fwd[b, :n] < f).all()
            counts.append(cnt)
            if z is None:
                continue
            rem = cur[b, n:Tb]
            ref = confidence_keys(z[b, rem], None if allow is None else allow[b, rem], None if bias is None else bias[b, rem], temperature)
            worst_key = max(worst_key, float(np.abs(np.log(c.astype(np.float64)) - ref).max()))
            for t in range(n, n + cnt):
                s = int(new[b, t])
                lsm = guided_log_probs(z[b, s], np.uint32((1 << 22) - 1) if allow is None else allow[b, s], None if bias is None else bias[b, s],
                                       temperature)
                assert np.isfinite(lsm[tok[b, s]])
                worst_lp = max(worst_lp, abs(float(lp[b, t]) - float(lsm[tok[b, s]])))
                checked += 1
        state, cur, filled = tok, new, prog
        f += 1
    final = m.sample_end()
    assert np.array_equal(final, state) and np.array_equal(m.sample_progress(), T) and np.array_equal(m.sample_order(), cur)
    hist = np.bincount(counts, minlength=K + 1)[1:]
    print(f"{kind} {label} K {K} tau {tau}: {f} forwards, counts 1..{K}: {hist[:8].tolist()}{' ...' if K > 8 else ''} (max {max(counts)}); "
          f"|log key - oracle| {worst_key:.2e}, |logp - oracle| {worst_lp:.2e} over {checked} draws (bound {REF_TOL / scale:.1e})")
    assert checked > 0 and worst_key < REF_TOL / scale and worst_lp < REF_TOL / scale
    return counts, f, (final, m.sample_logp(), cur, m.sample_forwards(), m.sample_progress())


@pytest.mark.parametrize("name,K", [("A", 4), ("L", 64)])
def test_selection_against_the_devices_own_keys(micro, name, K):
    kind = micro["kind"]
    data = _data(kind, name)
    counts, forwards, got = _drive(micro, data, K, TAU[kind], oracle_every=1 if name == "A" else 8, label=f"batch {name}")
    _structure(data, got[0], got[2])
    # not vacuous: a forward took one slot, a forward took the cap, a forward took something strictly between
    assert 1 in counts and K in counts and any(1 < c < K for c in counts), np.bincount(counts).tolist()
    # the whole session through hd_sample is the same session
    assert _same(_run(micro["m0"], data, K, TAU[kind]), got)


def test_selection_under_a_guide(micro):
    from hudiff_amd import Guide
    kind = micro["kind"]
    data = _data(kind, "A")
    _, _, _, allow, bias = _batch(kind)
    for temperature in (0.5, 0.0):
        counts, _, got = _drive(micro, data, 3, TAU[kind], Guide(allow, bias, temperature), allow, bias, temperature, label=f"guided T {temperature}")
        assert max(counts) > 1
        again = micro["m0"].sample(*_args(data), return_logp=True, slots_per_step=3, slot_policy="confident", confidence=TAU[kind],
                                   guide=Guide(allow, bias, temperature), **KW)
        assert np.array_equal(again[0], got[0]) and np.array_equal(again[1], got[1])


# ---- 3. exact logits ---------------------------------------------------------------------------------------------------------------------
def _exact_kw(case, b, tau):
    from hudiff_amd import Guide
    return dict(dropout="off", guide=Guide(b.allow, b.bias, case.temperature) if case.guided else None, truncation=case.truncation,
                slots_per_step=case.K, slot_policy="confident", confidence=tau, lanes=2)


def _exact_check(case, b, mode, tok, lp, order, fwd, filled, perms, fwds, draws):
    want_order, want_tok = b.order.copy(), (b.full if mode == "score" else b.tokens).copy()
    want_fwd, ref = np.full((b.B, b.Tmax), -1, np.int32), np.zeros((b.B, b.Tmax))
    for r in range(b.B):
        for t, (e, (j, v)) in enumerate(zip(perms[r], draws[r])):
            want_order[r, t] = b.order[r, e]
            want_tok[r, want_order[r, t]] = j
            want_fwd[r, t] = fwds[r][t]
            ref[r, t] = v
    assert np.array_equal(order, want_order), (case.name, mode, order, want_order)
    assert np.array_equal(fwd, want_fwd), (case.name, mode, fwd, want_fwd)
    assert np.array_equal(filled, b.T)
    if tok is not None:
        assert np.array_equal(tok, want_tok), (case.name, mode)
    if lp is not None:
        live = np.arange(b.Tmax)[None, :] < b.T[:, None]
        assert (lp[~live] == 0).all() and np.isfinite(lp).all() and np.isfinite(ref).all()
        assert (np.abs(lp[live] - ref[live]) <= DC.logp_bound(ref[live])).all(), (case.name, mode, lp, ref)


@pytest.mark.parametrize("kind,name", [("ab", n) for n in sorted(TC.CASES)] + [("nb", "singletons_tau1"), ("nb", "pairs_tau05")])
def test_exact_logits(handles, kind, name):
    case, tau, perms, fwds, counts, draws = TC.expect(name, "record")
    b, m = DC.batch(case, kind), handles(kind)
    kw = _exact_kw(case, b, tau)
    args = (b.region, b.chain, b.order, b.T)
    tok, lp = m.sample(b.tokens, *args, q_noise=b.q, return_logp=True, **kw)
    _exact_check(case, b, "record", tok, lp, m.sample_order(), m.sample_forwards(), m.sample_progress(), perms, fwds, draws)
    R, F = m.sample_order(), m.sample_forwards()
    tok2 = m.sample(b.tokens, *args, q_noise=b.q, **dict(kw, lanes=1, graph=False))
    assert np.array_equal(tok2, tok) and np.array_equal(m.sample_order(), R) and np.array_equal(m.sample_forwards(), F)
    # scoring with the same list, K, tau and guide reproduces order and fwd exactly
    _, _, sperms, sfwds, _, sdraws = TC.expect(name, "score")
    assert sperms == perms and sfwds == fwds
    slp = m.score(b.full, *args, parallel=False, **kw)
    _exact_check(case, b, "score", None, slp, m.sample_order(), m.sample_forwards(), m.sample_progress(), sperms, sfwds, sdraws)
    assert np.array_equal(m.sample_order(), R) and np.array_equal(m.sample_forwards(), F)
    # the counts of every forward, driven one at a time
    m.sample_begin(b.tokens, *args, q_noise=b.q, **kw)
    prev = np.zeros(b.B, np.int32)
    for f in range(max(len(c) for c in counts)):
        m.sample_run(f, f + 1)
        now = m.sample_progress()
        assert (now - prev).tolist() == [c[f] if f < len(c) else 0 for c in counts], (name, f)
        prev = now
    assert np.array_equal(m.sample_end(), tok)


# ---- 4. session behaviour ----------------------------------------------------------------------------------------------------------------
def test_scoring_reproduces_the_session(micro):
    kind, m, K = micro["kind"], micro["m0"], 4
    data = _data(kind, "A")
    batch, order, T = data
    tok, lp, R, fwd, _ = _run(m, data, K, TAU[kind])
    sc = m.score(tok, batch["region"], batch["chain"], order, T, slots_per_step=K, slot_policy="confident", confidence=TAU[kind])
    err = float(np.abs(sc - lp).max())
    print(f"{kind}: |score under the threshold sampler - recorded| {err:.2e}")
    assert err < PAIR_TOL and (sc[~_live(T, order.shape[1])] == 0).all()
    assert np.array_equal(m.sample_progress(), T)
    with pytest.raises(ValueError):
        m.score(tok, batch["region"], batch["chain"], order, T, slots_per_step=K, slot_policy="confident", confidence=TAU[kind], parallel=True)


def test_launch_forms_agree_bit_for_bit(hip, micro):
    """Graph, eager, loop graph, restart, run_to_end in chunks of 1 / 3 / 4 and hd_sample, all on the 40 rows of batch A in two lanes.
    One lane against two is compared on the first 8 rows (a handle with lane_min_rows = 2, as the budget sibling does): the lane count
    picks GEMM tiles by launch size (kernel_set), and at 40 antibody rows the one-lane and two-lane launches of ANY session, the parent's
    confident K-session included, differ in the last bit of a few log-probabilities (measured: 7.2e-07, tokens and order equal); at 8
    rows both lane counts run the same kernels."""
    kind, K, m = micro["kind"], 4, micro["m0"]
    tau = TAU[kind]
    data = _data(kind, "A")
    _, order, T = data
    tcap = order.shape[1]
    want = _run(m, data, K, tau)
    assert not np.array_equal(want[3], _want_fwd(T, tcap, K)) and not np.array_equal(want[3], _want_fwd(T, tcap, 1))
    got = {"eager": _run(m, data, K, tau, graph=False), "loop": _run(m, data, K, tau, graph="loop")}
    batch, B = data[0], order.shape[0]
    small = (dict(batch, tokens=batch["tokens"][:8], region=batch["region"][:8],
                  chain=None if batch["chain"] is None else np.concatenate([batch["chain"][:8], batch["chain"][B:B + 8]])), order[:8], T[:8])
    m2 = _mk(hip, kind, load_cfg(kind), load_weights(kind), options={"lane_min_rows": 2})
    try:
        m2.debug_launch_tally()
        one = _run(m2, small, K, tau, lanes=1)
        assert m2.debug_launch_tally()["sample_lanes_1"] > 0
        two = _run(m2, small, K, tau, lanes=2)
        assert m2.debug_launch_tally()["sample_lanes_2"] > 0
        assert _same(one, two) and len(set(one[3].max(axis=1).tolist())) > 1          # (rows that need different numbers of forwards)
        assert _same(_run(m2, small, K, tau, lanes=2, graph=False), one)
    finally:
        m2.close()
    ckw = dict(KW, record_logp=True, slots_per_step=K, slot_policy="confident", confidence=tau)
    need = int(want[3].max()) + 1

    def split(chunk, restart=False):
        m.sample_begin(*_args(data), **ckw)
        if restart:                                  # another seed first; the restart puts list, progress and fwd back
            m.sample_restart(SEED + 1)
            m.sample_run_to_end(2)
            assert not np.array_equal(m.sample_tokens(), want[0])
            m.sample_restart(SEED)
            assert (m.sample_progress() == 0).all() and (m.sample_forwards() == -1).all() and np.array_equal(m.sample_order(), order)
        n = m.sample_run_to_end(chunk)
        assert n == min(-(-need // chunk) * chunk, tcap), (n, need, chunk)
        rest = (m.sample_logp(), m.sample_order(), m.sample_forwards(), m.sample_progress())
        return (m.sample_end(),) + rest
    got["chunk 1"], got["chunk 4"], got["restart"] = split(1), split(4), split(3, restart=True)
    for name, res in got.items():
        assert _same(res, want), name
    # read-backs stay legal after the end
    assert np.array_equal(m.sample_forwards(), want[3]) and np.array_equal(m.sample_progress(), T)


def test_two_thresholds_on_one_handle(micro):
    """A stale graph would replay the other session's cmax: each session equals its eager run."""
    kind, K, m = micro["kind"], 4, micro["m0"]
    data = _data(kind, "A")
    a, b = _run(m, data, K, TAU[kind]), _run(m, data, K, 0.3)
    assert not np.array_equal(a[3], b[3])
    assert _same(_run(m, data, K, TAU[kind]), a) and _same(_run(m, data, K, 0.3), b)
    assert _same(_run(m, data, K, TAU[kind], graph=False), a) and _same(_run(m, data, K, 0.3, graph=False), b)


def test_sessions_without_a_threshold_are_unchanged(micro):
    from hudiff_amd import Guide
    kind, m = micro["kind"], micro["m0"]
    data = _data(kind, "A")
    _, _, _, allow, bias = _batch(kind)
    rkw = dict(KW, return_logp=True)
    g = Guide(allow, bias, 0.5)
    before = {"given": m.sample(*_args(data), **rkw), "block": m.sample(*_args(data), slots_per_step=2, **rkw),
              "guided": m.sample(*_args(data), guide=g, slots_per_step=2, **rkw)}
    conf = _confident(micro, "A", 2)
    _run(m, data, 2, TAU[kind])
    after = {"given": m.sample(*_args(data), **rkw), "block": m.sample(*_args(data), slots_per_step=2, **rkw),
             "guided": m.sample(*_args(data), guide=g, slots_per_step=2, **rkw)}
    for k in before:
        assert _same(before[k], after[k]), k
    tok, lp = m.sample(*_args(data), slots_per_step=2, slot_policy="confident", **rkw)
    assert _same((tok, lp, m.sample_order()), conf)
    # hd_sample_keys is there for a confident session without a threshold: the keys of its last forward
    keys = m.sample_keys()
    live = _live(data[2], data[1].shape[1])
    assert np.isfinite(keys).all() and (keys[live & (np.arange(keys.shape[1])[None, :] >= 4)] >= 1.0).all()


def test_status(hip, micro):
    from hudiff_amd import Budget
    from hudiff_amd import _lib as L
    from hudiff_amd._lib import HD_ERR_INVALID, HD_ERR_STATE, HD_ERR_UNSUPPORTED, HudiffError
    kind, m, K = micro["kind"], micro["m0"], 4
    tau = TAU[kind]
    data = _data(kind, "A")
    batch, order, T = data
    B, tcap = order.shape
    args = _args(data)
    lib = L.load()
    want = _run(m, data, K, tau)
    conf = _confident(micro, "A", K)

    def raises(status, fn, *a, **k):
        with pytest.raises(HudiffError) as e:
            fn(*a, **k)
        assert e.value.status == status, e.value

    def confident_run():
        tok, lp = m.sample(*args, return_logp=True, slots_per_step=K, slot_policy="confident", **KW)
        return tok, lp, m.sample_order()
    # hd_set_confidence: values, NULL handle, tau == 0 clears
    assert lib.hd_set_confidence(None, 0.5) == HD_ERR_INVALID
    for bad in (float("nan"), float("inf"), -0.25, 1.5):
        assert lib.hd_set_confidence(m._h, bad) == HD_ERR_INVALID, bad
    with pytest.raises(ValueError):
        m.set_confidence(2.0)
    assert _same(confident_run(), conf)                      # (nothing was left pending)
    m.set_confidence(tau)
    m.set_confidence(0)
    assert _same(confident_run(), conf)
    # one-shot; hd_forward neither uses nor clears it
    m.set_confidence(tau)
    m(batch["tokens"][:2], batch["region"][:2], None if batch["chain"] is None else np.concatenate([batch["chain"][:2], batch["chain"][B:B + 2]]))
    tok, lp = m.sample(*args, return_logp=True, slots_per_step=K, slot_policy="confident", **KW)
    assert _same((tok, lp, m.sample_order(), m.sample_forwards(), m.sample_progress()), want)
    assert _same(confident_run(), conf)
    raises(HD_ERR_STATE, m.sample_progress)                  # the last session has no threshold
    raises(HD_ERR_STATE, m.sample_forwards)
    # at the begin: the given order, a budget; a failed begin consumes the threshold
    raises(HD_ERR_UNSUPPORTED, m.sample, *args, confidence=tau, **KW)
    raises(HD_ERR_UNSUPPORTED, m.sample, *args, confidence=tau, slots_per_step=K, **KW)
    origin = np.where(batch["tokens"] == 22, 0, 22).astype(np.int32)
    raises(HD_ERR_UNSUPPORTED, m.sample, *args, confidence=tau, slot_policy="confident", budget=Budget(origin, 2), **KW)
    raises(HD_ERR_UNSUPPORTED, m.score, want[0], *args[1:], confidence=tau)
    assert _same(confident_run(), conf)
    raises(HD_ERR_UNSUPPORTED, m.sample, *args, confidence=tau, slot_policy="confident", **dict(KW, dropout="inject"))
    rep = order.copy()
    rep[21, 4] = rep[21, 1]
    raises(HD_ERR_INVALID, m.sample, batch["tokens"], batch["region"], batch["chain"], rep, T, confidence=tau, slot_policy="confident", **KW)
    assert _same(confident_run(), conf)
    # a given-order session: no keys, no run to the end
    m.sample_begin(*args, **KW)
    raises(HD_ERR_STATE, m.sample_keys)
    raises(HD_ERR_STATE, m.sample_run_to_end, 4)
    raises(HD_ERR_STATE, m.sample_progress)
    m.sample_end()
    m.sample_begin(*args, slots_per_step=K, slot_policy="confident", **KW)
    raises(HD_ERR_STATE, m.sample_run_to_end, 4)
    raises(HD_ERR_INVALID, m.sample_run, 1, 2)               # (the K-session keeps its multiple-of-K rule)
    m.sample_end()
    # inside a threshold session
    m.sample_begin(*args, record_logp=True, slots_per_step=K, slot_policy="confident", confidence=tau, **KW)
    raises(HD_ERR_STATE, m.set_confidence, 0.5)
    assert lib.hd_set_confidence(m._h, 0.0) == HD_ERR_STATE
    raises(HD_ERR_INVALID, m.sample_run_to_end, 0)
    raises(HD_ERR_INVALID, m.sample_run_to_end, tcap + 1)
    raises(HD_ERR_INVALID, m.sample_run, 0, tcap + 1)
    raises(HD_ERR_INVALID, m.sample_run, 2, 1)
    raises(HD_ERR_INVALID, m.sample_run, -1, 1)
    m.sample_run(0, 0)
    m.sample_run(0, 1)                                       # forward numbers: no multiple-of-K rule
    m.sample_run(1, 3)
    m.sync()
    assert m.last_run_ms()[1] == 2                           # forwards
    p = m.sample_progress()
    assert (p >= np.minimum(T, 3)).all() and (p <= np.minimum(T, 3 * K)).all()
    n = m.sample_run_to_end(tcap)
    assert n == tcap - 3
    lp = m.sample_logp()
    assert _same((m.sample_end(), lp, m.sample_order(), m.sample_forwards(), m.sample_progress()), want)
    assert lib.hd_sample_run_to_end(m._h, 4, None) == HD_ERR_STATE          # no open session
    assert lib.hd_sample_run_to_end(None, 4, None) == HD_ERR_STATE
    # fresh handle: nothing to read back
    fresh = _mk(hip, kind, load_cfg(kind), load_weights(kind))
    try:
        raises(HD_ERR_STATE, fresh.sample_progress, B)
        raises(HD_ERR_STATE, fresh.sample_forwards, B, tcap)
        raises(HD_ERR_STATE, fresh.sample_keys, B, tcap)
    finally:
        fresh.close()


@pytest.mark.parametrize("kind", ["ab", "nb"])
def test_lnsync_guard_repeat_finishes_every_row(hip, kind):
    """Production width, the batch of the siblings' guard tests.  The repeat runs on other kernels, so its keys -- and with them the
    number of forwards -- may differ: what is asserted is that the repeat ran to ITS end (every row full, fwd set on every position, the
    order a permutation of the list) and that scoring the repeat's tokens on the same handle reproduces its order and fwd."""
    from hudiff_amd import evalsets as E, synthetic as S
    cfg = dict(S.AB_CONFIG if kind == "ab" else S.NB_CONFIG, dropout=0.0)
    mx = _mk(hip, kind, cfg, S.random_state_dict(kind, cfg, seed=0), precision="split")
    try:
        big = E.eval_batch("huab348" if kind == "ab" else "vhh", 128 if kind == "ab" else 160, row0=0)
        T = np.minimum(big["T"], 4)
        args = (big["tokens"], big["region"], big["chain"], big["order"], T)
        kw = dict(seed=13, row0=0, return_logp=True)
        ckw = dict(slots_per_step=2, slot_policy="confident", confidence=0.15)      # (near the median key of these weights: 1 / 6.8)
        mx.sample(*args, **kw)
        prec(mx, lnsync_in_use=True, lnsync_fallbacks=0, last_call_repeated=False)
        mx.debug_fail_next_lnsync()
        with pytest.warns(RuntimeWarning, match="ln_sync"):
            tok, lp = mx.sample(*args, **ckw, **kw)
        R, fwd, filled = mx.sample_order(), mx.sample_forwards(), mx.sample_progress()
        prec(mx, lnsync_in_use=False, lnsync_fallbacks=1, last_call_repeated=True)
        assert np.array_equal(filled, T)
        live = _live(T, big["order"].shape[1])
        assert (fwd[live] >= 0).all() and (fwd[~live] == -1).all() and (np.diff(fwd, axis=1)[live[:, 1:]] >= 0).all()
        assert not (tok[np.arange(len(T))[:, None], R][live] == 22).any()
        for b in range(len(T)):
            assert sorted(R[b, :T[b]].tolist()) == sorted(big["order"][b, :T[b]].tolist())
        sc = mx.score(tok, *args[1:], **ckw)
        assert np.array_equal(mx.sample_order(), R) and np.array_equal(mx.sample_forwards(), fwd)
        err = float(np.abs(sc - lp).max())
        print(f"{kind}: ln_sync guard in a threshold session: forwards per row max {int(fwd.max()) + 1}, |score - repeat| {err:.2e}")
        assert err < PAIR_TOL
    finally:
        mx.close()


@pytest.mark.parametrize("route", ["split", "f32_all"])
def test_production_width(hip, route):
    """4 rows, T = 8, K = 4 at production width: the device's keys and log-probabilities against the library's own hd_forward.  tau = 0.15
    sits near the median of these weights' forward-0 keys (1 / 6.9), so that the rows take different counts."""
    z, cfg, sd = _load_prod("ab")
    m = _mk(hip, "ab", cfg, sd, precision=route)
    try:
        B, Tn, K, tau = 4, 8, 4, 0.15
        n = z["tokens"].shape[0]
        idx = np.arange(B) % n                               # (the recorded batch has fewer rows: cycled; the noise is keyed by row)
        chain = np.concatenate([z["chain"][:n][idx], z["chain"][n:][idx]])
        assert (z["T"][idx] >= Tn).all()
        tokens, region, order, T = z["tokens"][idx], z["region"][idx], np.ascontiguousarray(z["order"][idx, :Tn]), np.full(B, Tn, np.int32)
        cmax = confidence_cmax(tau)
        m.sample_begin(tokens, region, chain, order, T, record_logp=True, slots_per_step=K, slot_policy="confident", confidence=tau, seed=3,
                       dropout="off")
        state, cur, filled, f, worst_key, worst_lp, counts, cnts = tokens.copy(), order.copy(), np.zeros(B, np.int32), 0, 0.0, 0.0, [], []
        while (filled < T).any():
            m.sample_run(f, f + 1)
            keys, new, prog, tok, lp = m.sample_keys(), m.sample_order(), m.sample_progress(), m.sample_tokens(), m.sample_logp()
            pending = (state, cur, filled, keys, new, prog, tok, lp)
            state, cur, filled, f = tok, new, prog, f + 1
            counts.append(pending)
        m.sample_end()
        for state, cur, filled, keys, new, prog, tok, lp in counts:
            lsm = log_softmax64(m(state, region, chain, dropout="off")[:, :, :22])
            for b in range(B):
                a, Tb = int(filled[b]), int(T[b])
                if a >= Tb:
                    continue
                chosen, cnt, perm = threshold_select(keys[b, a:Tb], K, cmax)
                assert prog[b] == a + cnt and np.array_equal(new[b, a:Tb], cur[b, a:Tb][perm])
                cnts.append(cnt)
                ref = -lsm[b, cur[b, a:Tb]].max(axis=-1)                              # log c = -log p_max
                worst_key = max(worst_key, float(np.abs(np.log(keys[b, a:Tb].astype(np.float64)) - ref).max()))
                for t in range(a, a + cnt):
                    s = int(new[b, t])
                    worst_lp = max(worst_lp, abs(float(lp[b, t]) - float(lsm[b, s, tok[b, s]])))
        print(f"ab production width, route {route}: {len(counts)} forwards, counts {np.bincount(cnts, minlength=K + 1)[1:].tolist()}; |log key - hd_forward| {worst_key:.2e}, |logp - hd_forward| {worst_lp:.2e}")
        assert worst_key < PAIR_TOL and worst_lp < PAIR_TOL and min(cnts) < max(cnts)
    finally:
        m.close()


# ---- 5. CLIs -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cli", ["sample", "nanosample", "sample_for_anti_cdr", "sample_for_nano_cdr"])
def test_cli_confidence(hip, tmp_path, monkeypatch, cli):
    """--confidence 0.04 (every key qualifies) writes the CSV of the confident run with the same cap, byte for byte, at dropout off; a
    higher threshold needs more forwards per row, and the sampler logs them."""
    import importlib
    from test_gpu_budget import _cli_args
    mod = importlib.import_module(f"hudiff_amd.cli.{cli}")
    seen = []
    real = mod.log_forward_stats
    monkeypatch.setattr(mod, "log_forward_stats", lambda stats, logger: (seen.append(dict(stats)), real(stats, logger))[1])
    base = ["--dropout", "off", "--slot_policy", "confident", "--slots_per_step", "4"]
    outs, stats = {}, {}
    for tag, extra in (("K4", []), ("all", ["--confidence", "0.04"]), ("some", ["--confidence", "0.2"])):
        seen.clear()
        outs[tag] = open(mod.main(_cli_args(cli, tmp_path, tag) + base + extra), "rb").read()
        stats[tag] = [s for s in seen if s]
    assert outs["all"] == outs["K4"]
    assert not stats["K4"] and stats["all"] and stats["some"]
    mean = {k: sum(s["forwards"] for s in v) / sum(s["rows"] for s in v) for k, v in stats.items() if v}
    print(f"{cli}: forwards per row, mean: tau 0.04 {mean['all']:.2f}, tau 0.2 {mean['some']:.2f}")
    assert mean["some"] > mean["all"]


def test_score_cli_confidence(hip, tmp_path):
    from hudiff_amd.cli import score as score_cli
    from test_gpu_cli import _write_inputs
    from test_gpu_logp import _nb_checkpoint
    csv, nb = _write_inputs(tmp_path, "nb", 3)
    ck = tmp_path / "run" / "checkpoints" / "hudiffnb.pt"
    _nb_checkpoint(ck)
    base = ["--ckpt", str(ck), "--kind", "nb", "--data_fpath", str(csv), "--numbered_fpath", str(nb), "--seed", "8", "--mask", "inpaint",
            "--slots_per_step", "4", "--slot_policy", "confident"]
    rows = {}
    for tag, extra in (("K4", []), ("all", ["--confidence", "0.04"]), ("some", ["--confidence", "0.2"])):
        rows[tag] = open(score_cli.main(base + extra + ["--out_fpath", str(tmp_path / f"scores_{tag}.csv")])).read().splitlines()
    assert rows["all"] == rows["K4"] and len(rows["some"]) == len(rows["K4"]) and rows["some"] != rows["K4"]
    with pytest.raises(SystemExit):
        score_cli.main(base[:-2] + ["--confidence", "0.2"])
