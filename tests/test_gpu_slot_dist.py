"""The distribution record on the GPU (include/hudiff_hip.h "distribution record": HD_RECORD_DIST, hd_sample_dist, model.sample_dist,
model.score(return_dist=True), scoring.scan_jobs, hudiff_amd.cli.scan).

  1. exact logits      every "draw" and "confident" case of tests/draw_cases.py, recording and scoring, with the flag: the -inf pattern of
                       all 22 values is that of guide.guided_log_probs on the exactly known g, finite values sit within
                       draw_cases.logp_bound of it, and the entry of the token written is logp's bits
  2. neutrality        tokens, logp and order with the flag are those without it, bit for bit, graph and eager, one case per family
  3. budget            an exhausted draw: +0.0f at the origin, -inf at the 21 others
  4. recorded traces   all 22 values of every step against the reference's recorded logits (REF_TOL), sequential against step-parallel
                       scoring (PAIR_TOL)
  5. production width  one row per (sequence, slot) of tail_cases against the float64 oracle (tail_cases' own yard-stick) and against the
                       22-copy scoring session the suite used until now
  6. layout            two lanes with T = 0 rows, zeros behind T[b], restart, the ln_sync guard's repeat, stale graphs
  7. statuses
  8. the mutational scan, both contexts, and its CLI

No bound here comes from what the record gave: logp_bound is derived in draw_cases, REF_TOL / PAIR_TOL in test_gpu_logp, the yard-stick
in tail_cases; the sum rule of (8) is derived where it is asserted.

OBSERVED (MI355X; profiles/slot_dist/README.md).  (1) worst |dist - float64| / logp_bound 0.228 (temp_001), at most 0.096 elsewhere.
(4) |record - reference| at most 1.29e-6, sequential and step-parallel scoring alike, |seq - par| at most 9.5e-7.  (5) yard-sticks
antibody 1.82e-6, nanobody 1.42e-6; worst of the 22 recorded values as a multiple of the yard-stick:
                 |record - float64| (bound 3)   |record - 22-copy session| (bound 6)   the 22-copy session against float64
  ab  split      0.63                            0.52                                   0.55
      f32_all    0.56                            0.52                                   0.67
  nb  split      0.83                            0.67                                   0.81
      f32_all    1.06                            0.67                                   1.06
(8) the scan against 132 separately scored point mutations: 4.8e-7 on both models.  No bound was widened.  The module takes 11 s, the
slowest case 2.5 s (the first production-width case of a kind builds its float64 reference, which tail_cases keeps for the whole run).
"""
import numpy as np
import pytest

import budget_cases as BC
import draw_cases as DC
import tail_cases as TC
import threshold_cases as TH
from conftest import load_cfg, load_golden, load_weights, chain_or_none, prec
from hudiff_amd.guide import guided_log_probs
from test_gpu_logp import MICRO, PAIR_TOL, REF_TOL, _ab_checkpoint, _mk, _ragged, log_softmax64, traces

pytestmark = pytest.mark.gpu

NUMERIC = ["guided_overflow"]                            # sessions that must end in HD_ERR_NUMERIC: their record is unspecified


@pytest.fixture(scope="module")
def hip():
    import hudiff_amd
    if hudiff_amd.device_count() < 1:
        pytest.fail("no MI355X visible: GPU tests must run on the GPU box (there is no CPU fallback)")
    return hudiff_amd


@pytest.fixture(scope="module")
def exact(hip):
    """The zeroed-decoder handles of tests/test_gpu_draw_exact.py: one per (kind, table), two lanes from 2 rows on."""
    cache = {}

    def get(kind, table="main"):
        if (kind, table) not in cache:
            cache[kind, table] = _mk(hip, kind, load_cfg(kind), DC.decoder_state(load_weights(kind), table), options={"lane_min_rows": 2})
        return cache[kind, table]
    yield get
    for m in cache.values():
        m.close()


@pytest.fixture(scope="module", params=["ab", "nb"])
def micro(request, hip):
    kind = request.param
    m = _mk(hip, kind, load_cfg(kind), load_weights(kind))
    yield kind, m
    m.close()


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


def _bitsame(a, b):
    return a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


def _live(T, Tmax):
    return np.arange(Tmax)[None, :] < np.asarray(T)[:, None]


def _check_against_logp(dist, logp, written, T, what):
    """The part of the definition that needs no reference: the shape, zeros behind T[b], nothing NaN or +inf, the written token's entry
    is logp's bits where logp is finite and -inf where logp is -inf.  written [B, Tmax]: the token at order[b, t]."""
    B, Tmax = logp.shape
    assert dist.shape == (B, Tmax, 22) and dist.dtype == np.float32, what
    live = _live(T, Tmax)
    assert (_bits(dist)[~live] == 0).all(), (what, "entries behind T[b] are not +0")
    assert not np.isnan(dist).any() and not np.isposinf(dist).any(), what
    at = np.take_along_axis(dist, np.clip(written, 0, 21)[..., None].astype(np.int64), axis=2)[..., 0]
    assert np.array_equal(_bits(at)[live], _bits(logp)[live]), (what, "dist[b, t, token written] != logp[b, t] as bits")


def _guide(case, b):
    from hudiff_amd import Guide
    return Guide(b.allow, b.bias, case.temperature) if case.guided else None


def _kw(case, b, **more):
    return dict(dropout="off", guide=_guide(case, b), truncation=case.truncation, slots_per_step=case.K, slot_policy=case.policy,
                prune=case.prune, **more)


def _session(m, case, b, mode, flag=True, **more):
    """-> (tokens, logp, order, dist | None) of one session of an exact-logit case."""
    kw = _kw(case, b, **more)
    args = (b.region, b.chain, b.order, b.T)
    if mode == "score":
        res = m.score(b.full, *args, parallel=False, return_dist=flag, **kw)
        tok, lp = b.full, (res[0] if flag else res)
        dist = res[1] if flag else None
    else:
        tok, lp = m.sample(b.tokens, *args, q_noise=b.q, return_logp=True, record_dist=flag, **kw)
        dist = m.sample_dist() if flag else None
    return tok, lp, m.sample_order(), dist


# ---- 1. exactly known logits --------------------------------------------------------------------------------------------------------------
EXACT = [c.name for c in DC.cases() if c.family in ("draw", "confident") and c.name not in NUMERIC]


def test_the_cases_left_out_are_the_numeric_ones():
    assert NUMERIC == [c.name for c in DC.cases() if c.error == "numeric"]
    assert all(not DC.case(n).error for n in EXACT)


@pytest.mark.parametrize("name", EXACT)
def test_exact_logits(exact, name):
    case = DC.case(name)
    m, b = exact("ab", case.table), DC.batch(case, "ab")
    worst = 0.0
    for mode in [x for x in case.modes if x in ("record", "score")]:
        perms = DC.expect_confident(case, mode)[0] if case.family == "confident" else [list(range(len(r))) for r in case.rows]
        tok, lp, order, dist = _session(m, case, b, mode)
        written = np.take_along_axis(np.asarray(tok), order.astype(np.int64), axis=1)
        _check_against_logp(dist, lp, written, b.T, (name, mode))
        for r, row in enumerate(case.rows):
            for t, e in enumerate(perms[r]):
                d = row[e]
                assert order[r, t] == b.order[r, e], (name, mode, r, t)
                want = guided_log_probs(DC.g_of(case, d), d.allow, truncation=case.truncation)
                got = dist[r, t]
                assert np.array_equal(np.isneginf(got), np.isneginf(want)), (name, mode, r, t, got, want)
                fin = np.isfinite(want)
                err, bound = np.abs(got[fin].astype(np.float64) - want[fin]), DC.logp_bound(want[fin])
                worst = max(worst, float((err / bound).max()))
                assert (err <= bound).all(), (name, mode, r, t, float(err.max()), got, want)
    print(f"{name}: worst |dist - float64| / bound {worst:.3f}")


def test_exact_logits_nanobody(exact):
    """The other Segs::row mapping: one truncated guided case and one confident case on the nanobody model."""
    for name in ("trunc_guided_topk2", "confident_K2"):
        case = DC.case(name)
        m, b = exact("nb"), DC.batch(case, "nb")
        for mode in ("record", "score"):
            perms = DC.expect_confident(case, mode)[0] if case.family == "confident" else [list(range(len(r))) for r in case.rows]
            tok, lp, order, dist = _session(m, case, b, mode)
            _check_against_logp(dist, lp, np.take_along_axis(np.asarray(tok), order.astype(np.int64), axis=1), b.T, (name, mode))
            for r, row in enumerate(case.rows):
                for t, e in enumerate(perms[r]):
                    want = guided_log_probs(DC.g_of(case, row[e]), row[e].allow, truncation=case.truncation)
                    assert np.array_equal(np.isneginf(dist[r, t]), np.isneginf(want)), (name, mode, r, t)
                    fin = np.isfinite(want)
                    assert (np.abs(dist[r, t][fin].astype(np.float64) - want[fin]) <= DC.logp_bound(want[fin])).all(), (name, mode, r, t)


# ---- 2. neutrality ------------------------------------------------------------------------------------------------------------------------
def _family(name):
    """-> (case, batch builder, extra session keywords) of a neutrality family."""
    from hudiff_amd import Budget
    if name == "threshold":
        case, tau = TH.CASES["pairs_tau05"]
        return case, lambda: DC.batch(case, "ab"), lambda b: dict(confidence=tau)
    if name == "budget":
        bc = BC.case("budget_draw")
        return bc.case, lambda: BC.batch(bc, "ab"), lambda b: dict(budget=Budget(b.origin, b.M))
    case = DC.case({"plain": "plain_argmax/pruned", "guided": "guided_argmax/pruned", "truncated": "trunc_guided_topk2", "K3": "plain_argmax/K3",
                    "confident": "confident_K2"}[name])
    return case, lambda: DC.batch(case, "ab"), lambda b: {}


@pytest.mark.parametrize("family", ["plain", "guided", "truncated", "K3", "confident", "threshold", "budget"])
def test_the_flag_changes_nothing_else(exact, family):
    case, mk, more = _family(family)
    assert (case.K == 3) == (family == "K3")
    m, b = exact("ab", case.table), mk()
    for graph in (True, False):
        for mode in ("record", "score"):
            off = _session(m, case, b, mode, flag=False, graph=graph, **more(b))
            on = _session(m, case, b, mode, flag=True, graph=graph, **more(b))
            assert np.array_equal(on[0], off[0]), (family, mode, graph, "tokens")
            assert _bitsame(on[1], off[1]), (family, mode, graph, "logp")
            assert np.array_equal(on[2], off[2]), (family, mode, graph, "order")
            assert on[3] is not None and np.isfinite(on[3]).any() and off[3] is None
        # a sampling session with the flag alone records logp too, and draws what the plain session draws
        plain = m.sample(b.tokens, b.region, b.chain, b.order, b.T, q_noise=b.q, graph=graph, **_kw(case, b, **more(b)))
        flagged = m.sample(b.tokens, b.region, b.chain, b.order, b.T, q_noise=b.q, graph=graph, record_dist=True, **_kw(case, b, **more(b)))
        assert np.array_equal(plain, flagged), (family, graph)
        assert _bitsame(m.sample_logp(), _session(m, case, b, "record", flag=False, graph=graph, **more(b))[1])


# ---- 3. the budget ------------------------------------------------------------------------------------------------------------------------
def test_exhausted_budget_records_its_origin_alone(exact):
    from hudiff_amd import Budget
    bc = BC.case("budget_draw")
    m, b = exact("ab"), BC.batch(bc, "ab")
    seen = 0
    for mode in ("record", "score"):
        x = BC.expect_draws(bc, mode)
        tok, lp, order, dist = _session(m, bc.case, b, mode, budget=Budget(b.origin, b.M))
        _check_against_logp(dist, lp, np.take_along_axis(np.asarray(tok), order.astype(np.int64), axis=1), b.T, ("budget", mode))
        for r, flags in enumerate(x.exhausted):
            for t, ex in enumerate(flags):
                o = bc.origin[r][t]
                if not ex:
                    assert np.isfinite(dist[r, t]).sum() > 1, (mode, r, t)
                    continue
                seen += 1
                assert _bits(dist)[r, t, o] == 0, (mode, r, t, dist[r, t, o])                    # +0.0f
                assert np.isneginf(np.delete(dist[r, t], o)).all(), (mode, r, t, dist[r, t])
                tgt = DC.target_of(bc.case.rows[r][t])
                if mode == "record":
                    assert tok[r, b.order[r, t]] == o and _bits(lp)[r, t] == 0
                elif tgt != o:                           # a mutation the budget no longer pays for: -inf in both
                    assert np.isneginf(lp[r, t]) and np.isneginf(dist[r, t, tgt])
    assert seen >= 7                                     # record: 2 + 3 + 2 positions (budget_cases), score: at least row 0's two and row 2's


# ---- 4. the reference's recording -----------------------------------------------------------------------------------------------------------
def test_all_22_values_against_the_recorded_logits(micro):
    kind, m = micro
    for mode in MICRO[kind]:
        z = load_golden(f"micro_{kind}_sample_{mode}.npz")
        tokens, region, chain, loc, q, final = z["tokens"], z["region"], chain_or_none(z), z["loc"], z["q"], z["final"]
        B, Tn = tokens.shape[0], len(loc)
        want = np.transpose(log_softmax64(z["step_logits"][..., :22]), (1, 0, 2))                # [T, B, 22] -> [B, T, 22]
        order, T = np.repeat(loc[None], B, 0), np.full(B, Tn)
        out, logp = m.sample(tokens, region, chain, order, T, q_noise=q, return_logp=True, record_dist=True)
        rec = m.sample_dist()
        assert np.array_equal(out, final)
        _check_against_logp(rec, logp, np.take_along_axis(out, order.astype(np.int64), 1), T, (kind, mode, "record"))
        lp_seq, seq = m.score(final, region, chain, order, T, parallel=False, return_dist=True)
        lp_par, par = m.score(final, region, chain, order, T, parallel=True, device_batch=64, return_dist=True)
        for lp, d, what in ((lp_seq, seq, "sequential"), (lp_par, par, "parallel")):
            _check_against_logp(d, lp, np.take_along_axis(final, order.astype(np.int64), 1), T, (kind, mode, what))
        e = [float(np.abs(x - want).max()) for x in (rec, seq, par)] + [float(np.abs(seq.astype(np.float64) - par).max())]
        print(f"{kind} {mode}: |record - ref| {e[0]:.2e}  |seq - ref| {e[1]:.2e}  |par - ref| {e[2]:.2e}  |seq - par| {e[3]:.2e}")
        assert e[0] < REF_TOL and e[1] < REF_TOL and e[2] < REF_TOL and e[3] < PAIR_TOL, (kind, mode, e)
        assert _bitsame(lp_seq, m.score(final, region, chain, order, T, parallel=False))         # the values without the flag
    assert len(traces(kind)) > len(MICRO[kind])          # (the traces of test_gpu_logp are these fixtures and one deep one)


# ---- 5. float64 at production width -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("route", ["split", "f32_all"])
@pytest.mark.parametrize("kind", ["ab", "nb"])
def test_production_width_against_float64(hip, kind, route):
    """One row per (sequence, slot) -- the token-0 copies of tail_cases.all_picks -- gives in one forward what the 22-copy session gives."""
    ref = TC.reference("prod", kind)
    picks = TC.all_picks(kind)
    one = [p for p in picks if p[2] == 0]
    assert len(one) * 22 == len(picks)
    m = _mk(hip, kind, *TC.weights("prod", kind), precision=route)
    try:
        s1 = TC.session("prod", kind, one)
        m.score_begin(s1.tokens, s1.region, s1.chain, s1.order, s1.T, record_dist=True)
        try:
            m.sample_run(0, 1)
            dist, lp1 = m.sample_dist()[:, 0, :].copy(), m.sample_logp()[:, 0].copy()
        finally:
            m.sample_end()
        s22 = TC.session("prod", kind, picks)
        m.score_begin(s22.tokens, s22.region, s22.chain, s22.order, s22.T)
        try:
            m.sample_run(0, 1)
            lp22 = m.sample_logp()[:, 0].reshape(len(one), 22).copy()
        finally:
            m.sample_end()
        prec(m, precision=route, range_fallbacks=0, lnsync_fallbacks=0)
    finally:
        m.close()
    want = TC.expected(ref, s22).reshape(len(one), 22)
    assert np.array_equal(_bits(dist[:, 0]), _bits(lp1)) and np.isfinite(dist).all() and (dist < 0).all()
    e_ref, e_pair = float(np.abs(dist.astype(np.float64) - want).max()), float(np.abs(dist.astype(np.float64) - lp22).max())
    e_old = float(np.abs(lp22.astype(np.float64) - want).max())
    print(f"\n[dist prod {kind} {route}] yard-stick {ref.yard:.3e}: |record - float64| {e_ref:.3e} = {e_ref / ref.yard:.2f} x (bound 3), "
          f"|record - 22 copies| {e_pair:.3e} = {e_pair / ref.yard:.2f} x (bound 6); the 22 copies themselves {e_old / ref.yard:.2f} x")
    assert e_ref <= ref.bound, (kind, route, e_ref, ref.bound)
    assert e_pair <= ref.pair, (kind, route, e_pair, ref.pair)


# ---- 6. layout ----------------------------------------------------------------------------------------------------------------------------
def test_two_lanes_row_order_fillers_and_restart(micro):
    """B = 19 (default options: two lanes of 10 + 9) with T = 0 rows: rows come back in whole-batch order, fillers and the entries behind
    T[b] are zeros, a restart zeroes the record, the pieces of a session give the one-shot record."""
    kind, m = micro
    B, tcap = 19, 5
    batch, order, T = _ragged(kind, B, 21, tcap)
    T[0] = 0; T[9] = 0; T[10] = 2; T[18] = 0
    args = (batch["tokens"], batch["region"], batch["chain"], order, T)
    kw = dict(seed=77, row0=3, dropout="off")
    m.debug_launch_tally()
    tok, lp = m.sample(*args, return_logp=True, record_dist=True, lanes=2, **kw)
    assert m.debug_launch_tally()["sample_lanes_2"] > 0
    dist = m.sample_dist()
    _check_against_logp(dist, lp, np.take_along_axis(tok, order.astype(np.int64), 1), T, "two lanes")
    for b in (0, 9, 18):
        assert (_bits(dist)[b] == 0).all()
    live = _live(T, tcap)
    _sum_rule(dist, T)
    assert T[1] == tcap and T[11] == tcap
    # every row is its own: one lane runs other GEMM tiles, so two device results -- but a row that landed elsewhere would be far off
    tok1, lp1 = m.sample(*args, return_logp=True, record_dist=True, lanes=1, **kw)
    assert np.array_equal(tok1, tok) and np.abs(m.sample_dist() - dist)[live].max() < PAIR_TOL
    assert np.abs(dist[1] - dist[11]).max() > 100 * PAIR_TOL                              # (rows do differ)
    # restart, and a session in pieces
    m.sample_begin(*args, record_dist=True, lanes=2, **dict(kw, seed=5))
    try:
        m.sample_run(0, 2)
        part = m.sample_dist()
        assert (part[:, 2:] == 0).all() and (part[:, :2][live[:, :2]] < 0).any()
        m.sample_restart(kw["seed"])
        m.sync()
        assert (_bits(m.sample_dist()) == 0).all() and (m.sample_logp() == 0).all()
        m.sample_run(0, 3); m.sample_run(3, tcap)
        assert _bitsame(m.sample_dist(), dist) and _bitsame(m.sample_logp(), lp)
    finally:
        assert np.array_equal(m.sample_end(), tok)
    assert _bitsame(m.sample_dist(), dist)               # still legal after the end


def test_flag_after_no_flag_and_back_never_replays_a_stale_graph(micro):
    """In the manner of tests/test_gpu_session_key.py: ONE handle, sessions of one shape that differ in the flag alone, each through the
    captured-graph path and then eagerly; a key without the field would replay a graph captured with (without) the buffer."""
    kind, m = micro
    z = load_golden(f"micro_{kind}_sample_{MICRO[kind][0]}.npz")
    B, loc = z["tokens"].shape[0], z["loc"][:8]
    args = (z["region"], chain_or_none(z), np.repeat(loc[None], B, 0), np.full(B, len(loc)))
    q = np.ascontiguousarray(z["q"][:len(loc)])
    for mode in ("record", "score"):
        for flag in (False, True, False, True):
            runs = []
            for graph in (True, False):
                if mode == "score":
                    r = m.score(z["final"], *args, parallel=False, graph=graph, return_dist=flag)
                    runs.append(r if flag else (r,))
                else:
                    r = m.sample(z["tokens"], *args, q_noise=q, return_logp=True, record_dist=flag, graph=graph)
                    runs.append(r + ((m.sample_dist(),) if flag else ()))
                if not flag:
                    from hudiff_amd._lib import HD_ERR_STATE, HudiffError
                    with pytest.raises(HudiffError) as e:
                        m.sample_dist()
                    assert e.value.status == HD_ERR_STATE
            for x, y in zip(*runs):
                assert x.tobytes() == y.tobytes(), (kind, mode, flag, "the graph run differs from the eager run of the same session")
            if flag:
                assert np.isfinite(runs[0][-1]).all() and (runs[0][-1] < 0).all()


def test_lnsync_guard_repeat_rewrites_the_record(hip):
    """Production width, the batch of the siblings' guard tests: the repeat runs on the ln_apply_k passes and the record read back comes
    from the repeat -- the bits of an eager session on the same handle, which stays on those kernels."""
    from hudiff_amd import evalsets as E, synthetic as S
    cfg = dict(S.AB_CONFIG, dropout=0.0)
    mx = _mk(hip, "ab", cfg, S.random_state_dict("ab", cfg, seed=0), precision="split")
    try:
        big = E.eval_batch("huab348", 128, row0=0)
        T = np.minimum(big["T"], 3)
        args = (big["tokens"], big["region"], big["chain"], big["order"][:, :3].copy(), T)
        kw = dict(seed=13, row0=0, return_logp=True, record_dist=True)
        mx.sample(*args, **kw)
        prec(mx, lnsync_in_use=True, lnsync_fallbacks=0, last_call_repeated=False)
        mx.debug_fail_next_lnsync()
        with pytest.warns(RuntimeWarning, match="ln_sync"):
            tok, lp = mx.sample(*args, **kw)
        dist = mx.sample_dist()
        prec(mx, lnsync_in_use=False, lnsync_fallbacks=1, last_call_repeated=True)
        _check_against_logp(dist, lp, np.take_along_axis(tok, args[3].astype(np.int64), 1), T, "guard repeat")
        tok2, lp2 = mx.sample(*args, graph=False, **kw)
        assert np.array_equal(tok2, tok) and _bitsame(lp2, lp) and _bitsame(mx.sample_dist(), dist)
    finally:
        mx.close()


# ---- 7. statuses --------------------------------------------------------------------------------------------------------------------------
def test_statuses(micro):
    from hudiff_amd._lib import HD_ERR_STATE, HD_ERR_UNSUPPORTED, HudiffError
    kind, m = micro
    z = load_golden(f"micro_{kind}_sample_{MICRO[kind][0]}.npz")
    B, loc = z["tokens"].shape[0], z["loc"][:4]
    args = (z["tokens"], z["region"], chain_or_none(z), np.repeat(loc[None], B, 0), np.full(B, len(loc)))

    def raises(status, f, *a, **k):
        with pytest.raises(HudiffError) as e:
            f(*a, **k)
        assert e.value.status == status, e.value
    m.sample(*args, return_logp=True, dropout="off")
    raises(HD_ERR_STATE, m.sample_dist)                                  # a session that recorded logp only
    m.sample(*args, dropout="off")
    raises(HD_ERR_STATE, m.sample_dist)
    m.sample_begin(*args, dropout="off", record_logp=True)
    try:
        raises(HD_ERR_STATE, m.sample_dist)                              # inside an open session without the flag
    finally:
        m.sample_end()
    # the flag with a beam width pending: refused, and the width is consumed by that begin
    m.set_beam(2)
    raises(HD_ERR_UNSUPPORTED, m.sample_begin, *args, dropout="off", record_dist=True)
    tok = m.sample(*args, dropout="off", record_dist=True, seed=4)      # an ordinary session: no beam is pending any more
    raises(HD_ERR_STATE, m.beam_state)
    assert np.array_equal(tok, m.sample(*args, dropout="off", seed=4))
    # a session with the flag: legal after the end, until the next begin or forward
    m.sample(*args, dropout="off", record_dist=True, seed=4)
    assert m.sample_dist().shape == (B, len(loc), 22)
    m(z["tokens"], z["region"], chain_or_none(z))
    raises(HD_ERR_STATE, m.sample_dist)


# ---- 8. the mutational scan -----------------------------------------------------------------------------------------------------------------
def _jobs(kind, nslots=3):
    from hudiff_amd.sampler import Job
    z = load_golden(f"micro_{kind}_sample_{MICRO[kind][0]}.npz")
    n = z["tokens"].shape[0]
    ch = chain_or_none(z)
    jobs = []
    for r in range(2):
        i = r % n
        loc = z["loc"][[1 + r, len(z["loc"]) // 2, len(z["loc"]) - 1 - r]][:nslots] if nslots else z["loc"]
        jobs.append(Job(tokens=z["final"][i].astype(np.int32), region=z["region"][i].astype(np.int32), loc=np.asarray(loc, np.int32),
                        chain=None if ch is None else (int(ch[i]), int(ch[n + i])), name=f"j{r}"))
    return jobs


def _sum_rule(dist, T):
    """|log sum_a exp dist_a| <= logp_bound(H): every finite entry is within logp_bound(its value) = 4e-6 + 2^-22 |lp_a| of a distribution
    that sums to 1 -- the record's esum IS the sum of its own e_a -- so the logarithm of the sum moves by at most the p-weighted mean of
    those errors, 4e-6 + 2^-22 sum_a p_a |lp_a| = logp_bound(entropy)."""
    from hudiff_amd.guide import dist_entropy
    live = _live(T, dist.shape[1])
    with np.errstate(divide="ignore"):
        s = np.log(np.exp(dist.astype(np.float64)).sum(-1))
    assert (np.abs(s)[live] <= DC.logp_bound(dist_entropy(dist))[live]).all(), float(np.abs(s)[live].max())


def test_scan_given_is_the_score_of_every_point_mutation(micro):
    from hudiff_amd import scoring
    kind, m = micro
    jobs = _jobs(kind)
    res = scoring.scan_jobs(m, jobs, context="given")
    assert res["dist"].shape == (2, 3, 22) and res["T"].tolist() == [3, 3]
    rows, where = [], []
    for j, job in enumerate(jobs):
        for t, s in enumerate(job.loc):
            assert res["slot"][j, t] == s and res["wt"][j, t] == job.tokens[s]
            for a in range(22):
                x = job.tokens.copy()
                x[s] = a
                rows.append((x, job.region, job.chain, s))
                where.append((j, t, a))
    n = len(rows)
    chain = None if kind == "nb" else np.array([r[2][0] for r in rows] + [r[2][1] for r in rows], np.int32)
    lp = m.score(np.stack([r[0] for r in rows]), np.stack([r[1] for r in rows]), chain, np.array([[r[3]] for r in rows], np.int32), np.ones(n, np.int32),
                 parallel=False)[:, 0]
    got = np.array([res["dist"][w] for w in where])
    err = float(np.abs(got.astype(np.float64) - lp).max())
    print(f"{kind}: scan (given) against {n} scored point mutations: {err:.2e}")
    assert np.isfinite(got).all() and err < PAIR_TOL
    _sum_rule(res["dist"], res["T"])
    wt = np.take_along_axis(res["dist"], res["wt"][..., None].astype(np.int64), 2)[..., 0]
    assert _bitsame(res["logp_wt"], wt) and np.allclose(res["pseudo_ll"], wt.astype(np.float64).sum(1), rtol=0, atol=1e-12)
    assert (res["entropy"] > 0).all() and (res["entropy"] < np.log(22)).all()


def test_scan_masked_is_the_first_step_of_the_sampler(micro):
    from hudiff_amd import scoring
    kind, m = micro
    jobs = _jobs(kind, nslots=0)                         # the whole loc of the trace: more than 64 slots on the antibody, so two groups
    res = scoring.scan_jobs(m, jobs, context="masked")
    T = np.array([len(j.loc) for j in jobs])
    Tmax = int(T.max())
    tok, reg = np.stack([j.tokens for j in jobs]), np.stack([j.region for j in jobs])
    chain = None if kind == "nb" else np.array([j.chain[0] for j in jobs] + [j.chain[1] for j in jobs], np.int32)
    loc = np.stack([j.loc for j in jobs])
    x = scoring.expand_scan(tok, reg, chain, loc, T, "masked")
    N = x.rows.shape[0]
    assert N == int(((T + 63) // 64).sum()) and (kind != "ab" or N > 2)
    for i in range(N):                                   # the wild type back at the scored slots: the targets of the session
        s = x.order[i, :x.T[i]]
        x.tokens[i, s] = tok[x.rows[i], s]
    lp, flat = m.score(x.tokens, x.region, x.chain, x.order, x.T, parallel=False, slots_per_step=64, return_dist=True)
    assert _bitsame(res["dist"], x.fold_dist(flat, Tmax))
    assert _bitsame(res["logp_wt"], x.fold(lp, Tmax))
    _sum_rule(res["dist"], res["T"])
    # the distribution the sampler meets at its first step: a block session over the same masked row records it
    g0 = np.flatnonzero(x.rows == 0)[0]
    masked = tok[:1].copy()
    masked[0, loc[0]] = 22
    ch1 = None if chain is None else chain[[0, 2]]
    # (one row where the scan ran N: other GEMM tiles, so two device results)
    m.sample(masked, reg[:1], ch1, x.order[g0:g0 + 1], x.T[g0:g0 + 1], dropout="off", slots_per_step=64, record_dist=True, seed=1)
    assert np.abs(m.sample_dist()[0, :x.T[g0]] - res["dist"][0, :x.T[g0]]).max() < PAIR_TOL


@pytest.mark.parametrize("context", ["given", "masked"])
def test_scan_cli_end_to_end(hip, tmp_path, context):
    """The CLI on the micro antibody checkpoint: the CSV parses back to scan_jobs' arrays, bit for bit (float32 in shortest round-trip form)."""
    from hudiff_amd import scoring, tables as TB
    from hudiff_amd.cli import scan as cli
    from hudiff_amd.cli.common import load_numbered
    from hudiff_amd.guide import LETTERS
    from test_gpu_cli import _write_inputs
    from test_slot_dist_host import read_scan_csv
    kind = "ab"
    csv, nb = _write_inputs(tmp_path, kind, 2)
    csv.write_text("".join(l for l in open(csv).read().splitlines(True) if not l.startswith("human,")))
    ckpt = tmp_path / "ck" / "hudiffab.pt"
    _ab_checkpoint(ckpt)
    out = cli.main(["--ckpt", str(ckpt), "--kind", kind, "--data_fpath", str(csv), "--numbered_fpath", str(nb), "--context", context,
                    "--device_batch", "100", "--out_fpath", str(tmp_path / "scan.csv")])
    head, rows = read_scan_csv(out)
    assert head == cli.COLUMNS
    jobs = cli.build_jobs(cli.read_rows(str(csv), kind), kind, "finetune", load_numbered(str(nb)), "auto")
    m = _mk(hip, kind, load_cfg(kind), load_weights(kind))
    try:
        res = scoring.scan_jobs(m, jobs, context=context, device_batch=100)
    finally:
        m.close()
    assert len(rows) == int(res["T"].sum()) > 100
    at = 0
    for j, job in enumerate(jobs):
        for t in range(int(res["T"][j])):
            name, chain, imgt, slot, wt, logp_wt, entropy, dist = rows[at]
            at += 1
            assert name == job.name and slot == res["slot"][j, t] == job.loc[t] and wt == LETTERS[res["wt"][j, t]]
            assert (chain, imgt) == (("H", TB.HEAVY_POSITIONS[slot]) if slot < TB.H_LEN else ("L", TB.LIGHT_POSITIONS[slot - TB.H_LEN]))
            assert dist.tobytes() == res["dist"][j, t].tobytes() and np.float32(logp_wt).tobytes() == res["logp_wt"][j, t].tobytes()
            assert entropy == res["entropy"][j, t]
    _sum_rule(res["dist"], res["T"])
