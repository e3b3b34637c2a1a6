"""Refinement rounds on the GPU (hd_set_refine, include/hudiff_hip.h "refinement rounds"): a row that has drawn its whole list re-masks
the live positions it was least sure about and redraws them; on the device a round is nothing but order positions appended to the row.

Two yardsticks, both exact -- there is no tolerance and no near-tie exemption anywhere in this file:

1. the rule against the device's OWN record (`_check_rule`).  A session is driven one forward at a time; at every step at which
   hd_refine_state shows a round opened, T_now, round_start, round_count, the appended order positions, the holes and the masked tokens
   must be what guide.refine_select gives on the logp and order read back just before that step.  (The tokens are read back after the
   step's draw: the chosen slots that this forward has not yet redrawn must still be 22, the others a residue; that the forward itself
   saw all of them masked is what yardstick 2 shows.)
2. the host-chained form, bit for bit (`_check_chain`).  For every round and every distinct base of the batch: the tokens before the
   round with the chosen slots masked, the chosen slots at order positions [base, base + R_b), T = base + R_b (0 for the rows with
   another base), begun WITHOUT refinement and run over those positions, must draw the same tokens and record the same logp and dist --
   the positions are keyed identically (Philox counter, q_noise entry, dropout step, guide entries of the slot).  With a guide this is
   also what shows that the guide's entries travelled with the appended positions.

Under the confident policy the step that opens a round also permutes the appended positions (the selection of that very forward), so
rule 1 compares them as a set there and the chained confident session must realise the same order."""
import numpy as np
import pytest

from conftest import load_cfg, load_weights, prec
from hudiff_amd.guide import refine_fold, refine_live, refine_select, refine_tcap
from test_gpu_adaptive import KW, _args, _batch, _data
from test_gpu_guide import ROW0, SEED, _bits, _visited
from test_gpu_logp import _load_prod, _mk

pytestmark = pytest.mark.gpu


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
    models = {"kind": kind, "m0": _mk(hip, kind, cfg, sd), "m1": _mk(hip, kind, dict(cfg, dropout=p), sd)}
    yield models
    models["m0"].close(); models["m1"].close()


def _ceil(a, K):
    return -(-int(a) // K) * K


def _drive(m, args, K, refine, **kw):
    """A session with refinement rounds, one forward at a time.  -> dict: `steps`, one entry per forward with the state read back
    before and after it (tokens, logp, order, T_now, round_start, round_count); the final tokens, logp, dist and order."""
    m.sample_begin(*args, slots_per_step=K, refine=refine, record_dist=True, **kw)
    Tmax = m._session_Tmax

    def state():
        return (m.sample_tokens(), m.sample_logp(), m.sample_order()) + m.refine_state()
    steps, pre = [], state()
    for s in range(0, Tmax, K):
        m.sample_run(s, min(s + K, Tmax))
        post = state()
        steps.append(dict(s=s, pre=pre, post=post))
        pre = post
    dist = m.sample_dist()
    return dict(steps=steps, logp=pre[1], order=pre[2], T_now=pre[3], start=pre[4], count=pre[5], dist=dist, tokens=m.sample_end(),
                Tmax=Tmax)


def _check_rule(rec, T, K, refine, confident=False):
    """Yardstick 1 of the module docstring.  -> the number of rounds opened with at least one slot, and with none."""
    rounds, R, below = refine["rounds"], refine["slots"], refine.get("below", 0.0)
    full = empty = 0
    for st in rec["steps"]:
        s = st["s"]
        tok0, lp0, od0, Tn0, st0, ct0 = st["pre"]
        tok1, lp1, od1, Tn1, st1, ct1 = st["post"]
        for b in range(len(T)):
            done = int((st0[b] >= 0).sum())
            assert (st0[b, :done] >= 0).all() and (st0[b, done:] == -1).all()
            t_end = int(Tn1[b])
            drawn = od1[b, s:min(s + K, t_end)] if s < t_end else od1[b, :0]
            want_tok = tok0[b].copy()
            if s >= Tn0[b] and done < rounds:
                slots, pos = refine_select(lp0[b], od0[b], Tn0[b], R, below)
                base, n = _ceil(Tn0[b], K), len(slots)
                # (base is the step, unless the row's previous round was empty: then nothing changed and this one is empty too)
                assert base == s or (done > 0 and ct0[b, done - 1] == 0 and n == 0), (b, s, base)
                assert st1[b, done] == base and ct1[b, done] == n and Tn1[b] == base + n, (b, s)
                assert np.array_equal(st1[b, :done], st0[b, :done]) and (st1[b, done + 1:] == -1).all()
                assert np.array_equal(ct1[b, :done], ct0[b, :done]) and (ct1[b, done + 1:] == 0).all()
                assert np.array_equal(od1[b, :Tn0[b]], od0[b, :Tn0[b]])
                assert (od1[b, Tn0[b]:base] == -1).all()                              # the holes
                got = od1[b, base:base + n]
                assert np.array_equal(np.sort(got), np.sort(slots)) if confident else np.array_equal(got, slots), (b, s, got, slots)
                assert np.array_equal(od1[b, base + n:], od0[b, base + n:])
                want_tok[slots] = 22
                full, empty = full + (n > 0), empty + (n == 0)
            else:
                assert Tn1[b] == Tn0[b] and np.array_equal(st1[b], st0[b]) and np.array_equal(ct1[b], ct0[b])
                if not confident:
                    assert np.array_equal(od1[b], od0[b])
            # the tokens behind the step: the chosen slots masked, then this forward's positions drawn
            rest = np.ones(tok0.shape[1], bool)
            rest[drawn] = False
            assert np.array_equal(tok1[b, rest], want_tok[rest]), (b, s)
            assert (tok1[b, drawn] <= 21).all() and (tok1[b, drawn] >= 0).all()
            # positions outside this forward keep their record
            keep = np.ones(lp0.shape[1], bool)
            keep[s:min(s + K, lp0.shape[1])] = False
            assert np.array_equal(lp1[b, keep], lp0[b, keep])
    return full, empty


def _check_chain(m, args, K, refine, rec, confident=False, **kw):
    """Yardstick 2 of the module docstring, on the handle that ran the refined session.  -> the number of chained sessions run."""
    tokens, region, chain, order, T = args
    B, L = tokens.shape
    rounds, R, below = refine["rounds"], refine["slots"], refine.get("below", 0.0)
    Tmax = rec["Tmax"]
    by_step = {st["s"]: st for st in rec["steps"]}
    runs = 0
    for r in range(rounds):
        for base in sorted(set(int(x) for x in rec["start"][:, r][rec["count"][:, r] > 0])):
            tok0, lp0, od0, Tn0 = by_step[base]["pre"][:4]
            rows = np.flatnonzero((rec["start"][:, r] == base) & (rec["count"][:, r] > 0))
            tok2, order2, T2 = tok0.copy(), np.zeros((B, Tmax), np.int32), np.zeros(B, np.int32)
            for b in rows:
                slots, _ = refine_select(lp0[b], od0[b], Tn0[b], R, below)
                assert len(slots) == rec["count"][b, r]
                tok2[b, slots] = 22
                # positions below base are never run: any slots that keep the list legal (no slot twice)
                free = np.setdiff1d(np.arange(L), slots)
                order2[b, :base] = free[np.arange(base) % len(free)] if not confident else free[:base]
                order2[b, base:base + len(slots)] = slots
                T2[b] = base + len(slots)
            m.sample_begin(tok2, region, chain, order2, T2, slots_per_step=K, record_logp=True, record_dist=True, **kw)
            m.sample_run(base, min(base + _ceil(R, K), Tmax))
            lp2, dist2, od2 = m.sample_logp(), m.sample_dist(), m.sample_order()
            out2 = m.sample_end()
            for b in rows:
                n = int(rec["count"][b, r])
                last = base + _ceil(n, K) - K                                          # the forward that drew the round's last position
                sl = slice(base, base + n)
                assert np.array_equal(lp2[b, sl], rec["logp"][b, sl]), (r, base, b)
                assert np.array_equal(dist2[b, sl], rec["dist"][b, sl]), (r, base, b)
                assert np.array_equal(od2[b, sl], rec["order"][b, sl]), (r, base, b)
                assert np.array_equal(out2[b], by_step[last]["post"][0][b]), (r, base, b)
            runs += 1
    return runs


def _check_invariants(m, args, K, rec, plain, **kw):
    """5 of the issue: slots outside the list untouched, no token 22 at the end, redrawn slots a subset of the list, and the first pass
    is the session without refinement (`plain` = its tokens and logp)."""
    tokens, region, chain, order, T = args
    B, L = tokens.shape
    vis = _visited(order, T, L)
    out = rec["tokens"]
    assert np.array_equal(out[~vis], tokens[~vis]) and not (out[vis] == 22).any()
    tcap = order.shape[1]
    for b in range(B):
        live = rec["order"][b, :rec["T_now"][b]]
        live = live[live >= 0]
        assert set(live.tolist()) == set(order[b, :T[b]].tolist()), b
        assert np.array_equal(rec["order"][b, :T[b]], order[b, :T[b]]) or kw.get("slot_policy") == "confident"
        # the first pass: tokens as they stand behind the forward that drew the row's last list position
        first = tokens[b] if T[b] == 0 else rec["steps"][(_ceil(T[b], K) - K) // K]["post"][0][b]
        assert np.array_equal(first, plain[0][b]), b
        assert np.array_equal(rec["logp"][b, :min(T[b], tcap)], plain[1][b, :T[b]]), b
    # the final token of a slot is the one written at its live position: its recorded distribution holds that token
    assert refine_live(rec["order"], rec["T_now"]).sum() == vis.sum()
    folded = refine_fold(rec["order"], rec["T_now"], rec["dist"], L)
    bb, ss = np.nonzero(vis)
    assert np.isfinite(folded[bb, ss, out[bb, ss]]).all()


def _plain(m, args, K, **kw):
    return m.sample(*args, slots_per_step=K, return_logp=True, **kw)


# ---- 1-3, 5. the rule, the chained form and the invariants on the shapes at which it can go wrong --------------------------------------
@pytest.mark.parametrize("lanes", [1, 2])
@pytest.mark.parametrize("K,R,rounds", [(1, 2, 2), (2, 3, 2), (4, 2, 2), (4, 4, 1)])
def test_batch_a(micro, K, R, rounds, lanes):
    """Batch A (40 rows, tcap 6, T[5] = 0, T[17] = 3): holes (K > 1), R < K, R > K, a row without a list."""
    m = micro["m0"]
    args = _args(_data(micro["kind"], "A"))
    refine = dict(rounds=rounds, slots=R)
    kw = dict(KW, lanes=lanes)
    rec = _drive(m, args, K, refine, **kw)
    full, empty = _check_rule(rec, args[4], K, refine)
    assert full >= 39 * rounds and empty >= rounds              # (T[5] = 0: its rounds are counted and append nothing)
    assert (rec["count"][5] == 0).all() and (rec["start"][5] == np.arange(rounds) * 0).all()
    if K > 1:
        assert (rec["order"] == -1).any()                       # holes were met
    assert _check_chain(m, args, K, refine, rec, **kw) >= rounds
    _check_invariants(m, args, K, rec, _plain(m, args, K, **kw), **kw)
    # hd_sample is the same session, and its read-backs stay legal behind the end
    tok = m.sample(*args, slots_per_step=K, refine=refine, **kw)
    assert np.array_equal(tok, rec["tokens"]) and np.array_equal(m.sample_logp(), rec["logp"]) and np.array_equal(m.sample_order(), rec["order"])
    Tn, start, count = m.refine_state()
    assert np.array_equal(Tn, rec["T_now"]) and np.array_equal(start, rec["start"]) and np.array_equal(count, rec["count"])


def test_below_leaves_rows_without_candidates(micro):
    """A bound that only some rows have a position under: the others' rounds are counted, append nothing and leave the tokens alone."""
    m, K = micro["m0"], 2
    args = _args(_data(micro["kind"], "A"))
    T = args[4]
    tok0, lp0 = _plain(m, args, K, **KW)
    worst = np.array([lp0[b, :T[b]].min() if T[b] else 0.0 for b in range(len(T))])
    below = float(np.float32(np.median(worst[T > 0])))
    refine = dict(rounds=2, slots=3, below=below)
    rec = _drive(m, args, K, refine, **KW)
    full, empty = _check_rule(rec, T, K, refine)
    assert full > 0 and empty > 2
    none = rec["count"].sum(axis=1) == 0
    assert none.sum() > 1 and (~none).sum() > 1
    assert np.array_equal(rec["tokens"][none], tok0[none])
    assert (rec["start"][none] >= 0).all()                      # counted all the same
    assert _check_chain(m, args, K, refine, rec, **KW) > 0
    _check_invariants(m, args, K, rec, (tok0, lp0), **KW)


def test_batch_l(micro):
    """Batch L: T = [L, 65, 1] at K = 64, R = 64: R_b is capped by the candidates (1 and 64 of 65) and the rank crosses wave boundaries."""
    m, K = micro["m0"], 64
    args = _args(_data(micro["kind"], "L"))
    refine = dict(rounds=2, slots=64)
    rec = _drive(m, args, K, refine, **KW)
    full, empty = _check_rule(rec, args[4], K, refine)
    assert full == 6 and empty == 0
    assert rec["count"][:, 0].tolist() == [64, 64, 1]
    assert _check_chain(m, args, K, refine, rec, **KW) >= 2
    _check_invariants(m, args, K, rec, _plain(m, args, K, **KW), **KW)


@pytest.mark.parametrize("what", ["philox", "q_noise", "dropout"])
def test_chained_form_noise_sources(micro, what):
    """Yardstick 2 with generated Philox noise, with injected q_noise and with generated dropout on."""
    K, refine = 2, dict(rounds=2, slots=3)
    args = _args(_data(micro["kind"], "A"))
    m, kw = micro["m0"], dict(KW)
    if what == "dropout":
        m, kw = micro["m1"], dict(KW, dropout="faithful")
    if what == "q_noise":
        tcap = refine_tcap(args[4], 2, 3, K)
        kw["q_noise"] = np.random.default_rng(11).exponential(1.0, (tcap, len(args[4]), 22)).astype(np.float32)
    rec = _drive(m, args, K, refine, **kw)
    _check_rule(rec, args[4], K, refine)
    assert _check_chain(m, args, K, refine, rec, **kw) >= 2
    if what == "dropout":                                        # (the masks really entered)
        off = _drive(m, args, K, refine, **dict(kw, dropout="off"))
        assert not np.array_equal(off["logp"], rec["logp"])


# ---- 4. composition -------------------------------------------------------------------------------------------------------------------
def test_composition(micro):
    """The confident policy, a guide with allowed bits, bias and temperature 0.7, a truncation and HD_RECORD_DIST together."""
    from hudiff_amd import Guide, Truncation
    m, K = micro["m0"], 2
    data = _data(micro["kind"], "A")
    args = _args(data)
    tokens, _, _, order, T = args
    _, _, _, allow, bias = _batch(micro["kind"])
    refine = dict(rounds=2, slots=3)
    kw = dict(KW, slot_policy="confident", guide=Guide(allow, bias, 0.7), truncation=Truncation(top_k=6, top_p=0.9))
    rec = _drive(m, args, K, refine, **kw)
    full, _ = _check_rule(rec, T, K, refine, confident=True)
    assert full >= 39
    assert _check_chain(m, args, K, refine, rec, confident=True, **kw) >= 2
    _check_invariants(m, args, K, rec, _plain(m, args, K, **kw), **kw)
    # the guide's entries of an appended position are those of its slot: the record's -inf pattern lies inside the slot's forbidden
    # tokens (the cut removes more), and a forbidden residue never appears
    out = rec["tokens"]
    for b in range(len(T)):
        for t in range(int(rec["T_now"][b])):
            s = int(rec["order"][b, t])
            if s < 0:
                assert (rec["dist"][b, t] == 0).all() and rec["logp"][b, t] == 0
                continue
            ok = _bits(allow[b, s], np.arange(22))
            assert np.isneginf(rec["dist"][b, t][~ok]).all(), (b, t)
            assert np.isfinite(rec["dist"][b, t][ok]).sum() <= 6 and np.isfinite(rec["dist"][b, t][ok]).any()
        vis = order[b, :T[b]]
        assert _bits(allow[b, vis], out[b, vis]).all(), b
    # the same seed through hd_sample_restart reproduces the sample; another seed does not
    m.sample_begin(*args, slots_per_step=K, refine=refine, record_dist=True, **kw)
    Tmax = m._session_Tmax
    m.sample_run(0, Tmax)
    m.sample_restart(SEED + 1)
    m.sample_run(0, Tmax)
    assert not np.array_equal(m.sample_tokens(), rec["tokens"])
    m.sample_restart(SEED)
    Tn, start, count = m.refine_state()
    assert np.array_equal(Tn, T) and (start == -1).all() and (count == 0).all() and np.array_equal(m.sample_order()[:, :order.shape[1]], order)
    assert (m.sample_order()[:, order.shape[1]:] == 0).all()
    m.sample_run(0, Tmax)
    lp, dist, od, st = m.sample_logp(), m.sample_dist(), m.sample_order(), m.refine_state()
    assert np.array_equal(m.sample_end(), rec["tokens"]) and np.array_equal(lp, rec["logp"]) and np.array_equal(dist, rec["dist"])
    assert np.array_equal(od, rec["order"]) and np.array_equal(st[0], rec["T_now"]) and np.array_equal(st[1], rec["start"])


def _same(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b)) and len(a) == len(b)


def _run(m, args, K, refine, **kw):
    tok = m.sample(*args, slots_per_step=K, refine=refine, **kw)
    return (tok, m.sample_logp(), m.sample_order()) + m.refine_state()


def test_launch_forms_agree_bit_for_bit(hip, micro):
    """Graph, HD_NO_GRAPH and HD_LOOP_GRAPH on batch A in two lanes.  One lane against two is compared on eight rows (rows 0-6 and 17) of
    a handle with lane_min_rows = 2: the lane count picks GEMM tiles by launch size, and at 40 antibody rows the one-lane and two-lane
    launches of any session differ in the last bit of a few log-probabilities (tests/test_gpu_threshold.py); at 8 rows both run the same
    kernels."""
    kind, K, m = micro["kind"], 4, micro["m0"]
    refine = dict(rounds=2, slots=2)
    args = _args(_data(kind, "A"))
    want = _run(m, args, K, refine, **KW)
    assert (want[5] > 0).any() and (want[2] == -1).any()
    assert _same(_run(m, args, K, refine, graph=False, **KW), want)
    assert _same(_run(m, args, K, refine, graph="loop", **KW), want)
    tokens, region, chain, order, T = args
    B, idx = len(T), np.array([0, 1, 2, 3, 4, 5, 6, 17])
    small = (tokens[idx], region[idx], None if chain is None else np.concatenate([chain[:B][idx], chain[B:][idx]]), order[idx], T[idx])
    m2 = _mk(hip, kind, load_cfg(kind), load_weights(kind), options={"lane_min_rows": 2})
    try:
        m2.debug_launch_tally()
        one = _run(m2, small, K, refine, lanes=1, **KW)
        assert m2.debug_launch_tally()["sample_lanes_1"] > 0
        two = _run(m2, small, K, refine, lanes=2, **KW)
        assert m2.debug_launch_tally()["sample_lanes_2"] > 0
        assert _same(one, two) and _same(_run(m2, small, K, refine, lanes=2, graph=False, **KW), one)
    finally:
        m2.close()


def test_no_stale_graph(micro):
    """One handle, sessions of one shape: two refinements, none, the first again.  Each equals its eager run, and the session without
    refinement is the one from before."""
    m, K = micro["m0"], 2
    args = _args(_data(micro["kind"], "A"))
    a, b = dict(rounds=1, slots=2), dict(rounds=2, slots=2, below=-1.0)
    plain = m.sample(*args, slots_per_step=K, return_logp=True, **KW)
    ra, rb = _run(m, args, K, a, **KW), _run(m, args, K, b, **KW)
    assert not _same(ra, rb)
    assert _same(m.sample(*args, slots_per_step=K, return_logp=True, **KW), plain)
    assert _same(_run(m, args, K, a, **KW), ra) and _same(_run(m, args, K, b, **KW), rb)
    assert _same(_run(m, args, K, a, graph=False, **KW), ra) and _same(_run(m, args, K, b, graph=False, **KW), rb)
    # the one-slot session keeps its pruned tail, with and without rounds
    m.debug_launch_tally()
    m.sample(*args, refine=a, **KW)
    t = m.debug_launch_tally()
    assert t["tail_sliced"] + t["tail_launches"] > 0


def test_lnsync_guard_repeat(hip):
    """Production width, the batch of the siblings' guard tests.  The repeat runs on the kernels the handle then stays on (separate
    LayerNorm passes), so it is held to the undisturbed session on THOSE kernels, bit for bit -- the state read back (T_now, rounds,
    order, logp) included; its agreement with the session on the ln_sync kernels is printed, as the budget's sibling does."""
    from hudiff_amd import evalsets as E, synthetic as S
    cfg = dict(S.AB_CONFIG, dropout=0.0)
    mx = _mk(hip, "ab", cfg, S.random_state_dict("ab", cfg, seed=0), precision="split", options={"lane_min_rows": 2})
    try:
        B8 = 8
        big = E.eval_batch("huab348", B8, row0=0)
        T = np.minimum(big["T"], 4)
        args = (big["tokens"], big["region"], big["chain"], np.ascontiguousarray(big["order"][:, :4]), T)
        refine = dict(rounds=1, slots=2)
        kw = dict(seed=13, row0=0)
        want = _run(mx, args, 2, refine, **kw)
        prec(mx, lnsync_in_use=True, lnsync_fallbacks=0, last_call_repeated=False)
        mx.debug_fail_next_lnsync()
        with pytest.warns(RuntimeWarning, match="ln_sync"):
            again = _run(mx, args, 2, refine, **kw)
        prec(mx, lnsync_in_use=False, lnsync_fallbacks=1, last_call_repeated=True)
        after = _run(mx, args, 2, refine, **kw)
        prec(mx, lnsync_fallbacks=1, last_call_repeated=False)
        assert _same(again, after)
        assert (again[5] == 2).all() and (again[3] == _ceil(4, 2) + 2).all() and not (again[0][_visited(args[3], T, again[0].shape[1])] == 22).any()
        agree = (again[0] == want[0]).all(axis=1)
        print(f"ln_sync guard in a session with refinement rounds: {int(agree.sum())} of {B8} rows draw the undisturbed tokens")
    finally:
        mx.close()


# ---- 6. production width ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["ab", "nb"])
def test_production_width(hip, kind):
    """The rows of the recorded production-width traces, default route, T cut to 8, K = 4, R = 4, one round: yardsticks 1 and 2."""
    z, cfg, sd = _load_prod(kind)
    m = _mk(hip, kind, cfg, sd)
    try:
        Tn = 8
        assert (z["T"] >= Tn).all()
        B = z["tokens"].shape[0]
        args = (z["tokens"], z["region"], z["chain"] if z["chain"].size else None, np.ascontiguousarray(z["order"][:, :Tn]),
                np.full(B, Tn, np.int32))
        refine = dict(rounds=1, slots=4)
        kw = dict(seed=3, row0=0, dropout="off")
        rec = _drive(m, args, 4, refine, **kw)
        full, empty = _check_rule(rec, args[4], 4, refine)
        assert full == B and empty == 0
        assert _check_chain(m, args, 4, refine, rec, **kw) == 1
        _check_invariants(m, args, 4, rec, _plain(m, args, 4, **kw), **kw)
    finally:
        m.close()


# ---- 7. the refusal table ---------------------------------------------------------------------------------------------------------------
def test_status(hip, micro):
    from hudiff_amd import Budget
    from hudiff_amd import _lib as L
    from hudiff_amd._lib import HD_ERR_INVALID, HD_ERR_STATE, HD_ERR_UNSUPPORTED, HudiffError
    kind, m, K = micro["kind"], micro["m0"], 2
    data = _data(kind, "A")
    batch, order, T = data
    args = _args(data)
    B, tcap = order.shape
    lib = L.load()
    refine = dict(rounds=1, slots=2)
    want = _run(m, args, K, refine, **KW)
    plain = m.sample(*args, slots_per_step=K, return_logp=True, **KW)

    def raises(status, fn, *a, **k):
        with pytest.raises(HudiffError) as e:
            fn(*a, **k)
        assert e.value.status == status, e.value

    def plain_run():
        return m.sample(*args, slots_per_step=K, return_logp=True, **KW)
    # hd_set_refine: values, NULL handle, rounds == 0 clears, one-shot
    assert lib.hd_set_refine(None, 1, 1, 0.0) == HD_ERR_INVALID
    for bad in ((-1, 1, 0.0), (17, 1, 0.0), (1, 0, 0.0), (1, 65, 0.0), (1, 1, 0.5), (1, 1, float("nan")), (1, 1, float("-inf"))):
        assert lib.hd_set_refine(m._h, *bad) == HD_ERR_INVALID, bad
    assert _same(plain_run(), plain)                             # (nothing was left pending)
    m.set_refine(2, 3, -0.5)
    m.set_refine(0)
    assert _same(plain_run(), plain)
    m.set_refine(1, 2)
    m(batch["tokens"][:2], batch["region"][:2], None if batch["chain"] is None else np.concatenate([batch["chain"][:2], batch["chain"][B:B + 2]]))
    pad = np.concatenate([order, np.zeros((B, refine_tcap(T, 1, 2, K) - tcap), np.int32)], axis=1)
    tok = m.sample(batch["tokens"], batch["region"], batch["chain"], pad, T, slots_per_step=K, **KW)     # hd_forward neither used nor cleared it
    assert np.array_equal(tok, want[0]) and np.array_equal(m.sample_logp(B, pad.shape[1]), want[1])
    assert _same(plain_run(), plain)                             # one-shot
    raises(HD_ERR_STATE, m.refine_state, B, 1)                   # the last session has no rounds
    # refused at the begin; the failed begin consumes the refinement
    m.set_refine(1, 2)
    raises(HD_ERR_UNSUPPORTED, m.beam_begin, *_beam_args(args, 2), 2)
    assert _same(plain_run(), plain)
    for more in (dict(slot_policy="confident", confidence=0.2), dict(budget=Budget(np.where(batch["tokens"] == 22, 0, 22).astype(np.int32), 2)),
                 dict(dropout="inject")):
        kk = dict(KW, **more)
        raises(HD_ERR_UNSUPPORTED, m.sample, *args, refine=refine, slots_per_step=1 if "budget" in more else K, **kk)
        assert _same(plain_run(), plain)
    m.set_refine(1, 2)
    raises(HD_ERR_UNSUPPORTED, m.score, want[0], *args[1:], parallel=False)
    assert _same(plain_run(), plain)
    rep = order.copy()
    rep[21, 4] = rep[21, 1]
    raises(HD_ERR_INVALID, m.sample, batch["tokens"], batch["region"], batch["chain"], rep, T, refine=refine, **KW)
    m.sample(batch["tokens"], batch["region"], batch["chain"], rep, T, **KW)                              # (legal without rounds at K = 1)
    m.set_refine(1, 2)
    with pytest.raises(HudiffError) as e:                         # Tmax too small: the message names the Tmax needed
        m.sample(batch["tokens"], batch["region"], batch["chain"], order, T, slots_per_step=K, **KW)
    assert e.value.status == HD_ERR_INVALID and f"Tmax >= {refine_tcap(T, 1, 2, K)}" in str(e.value)
    assert _same(plain_run(), plain)
    # inside a session
    m.sample_begin(*args, slots_per_step=K, refine=refine, **KW)
    raises(HD_ERR_STATE, m.set_refine, 1, 1)
    assert lib.hd_set_refine(m._h, 0, 0, 0.0) == HD_ERR_STATE
    Tn, start, count = m.refine_state()
    assert np.array_equal(Tn, T) and (start == -1).all() and (count == 0).all()
    m.sample_run(0, m._session_Tmax)
    lp, od = m.sample_logp(), m.sample_order()
    assert _same((m.sample_end(), lp, od) + m.refine_state(), want)
    m.sample_begin(*args, slots_per_step=K, **KW)
    raises(HD_ERR_STATE, m.refine_state, B, 1)
    m.sample_end()
    assert lib.hd_refine_state(None, None, None, None) == HD_ERR_STATE
    fresh = _mk(hip, kind, load_cfg(kind), load_weights(kind))
    try:
        raises(HD_ERR_STATE, fresh.refine_state, B, 1)
    finally:
        fresh.close()


def _beam_args(args, W):
    tokens, region, chain, order, T = args
    B = len(T)
    rep = np.repeat(np.arange(2), W)
    return (tokens[rep], region[rep], None if chain is None else np.concatenate([chain[:B][rep], chain[B:][rep]]), order[rep], T[rep])


# ---- the samplers -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cli", ["sample", "nanosample", "sample_for_anti_cdr", "sample_for_nano_cdr"])
def test_cli_refine(hip, tmp_path, caplog, cli):
    """A bound nothing lies under (--refine_below -1000) redraws nothing: the CSV is the one of the run without the flags, byte for byte,
    and the sidecar's logp column too; a real round changes the output, and the sidecar counts the redrawn positions.  (The nanobody CDR
    sampler writes only samples that number as a heavy domain, which the micro model's never do: there the samples are read from the
    lines it logs when it drops them.)"""
    import importlib
    import logging
    caplog.set_level(logging.INFO)
    from test_gpu_budget import _cli_args
    mod = importlib.import_module(f"hudiff_amd.cli.{cli}")
    side = cli in ("sample", "nanosample")
    outs, logs = {}, {}
    for tag, extra in (("plain", []), ("none", ["--refine_rounds", "2", "--refine_slots", "3", "--refine_below", "-1000"]),
                       ("some", ["--refine_rounds", "1", "--refine_slots", "3"])):
        more = ["--logp_fpath", str(tmp_path / f"{tag}.csv")] if side else []
        caplog.clear()
        outs[tag] = open(mod.main(_cli_args(cli, tmp_path, tag) + ["--dropout", "off", "--slots_per_step", "2"] + extra + more), "rb").read()
        if cli == "sample_for_nano_cdr":
            dropped = [r.getMessage() for r in caplog.records if "dropped:" in r.getMessage()]
            assert len(dropped) == 3
            outs[tag] += "\n".join(dropped).encode()
        if side:
            logs[tag] = [ln.split(",") for ln in open(tmp_path / f"{tag}.csv").read().splitlines()]
    assert outs["none"] == outs["plain"] and outs["some"] != outs["plain"]
    if side:
        assert logs["plain"][0][-1] == "chosen" and logs["none"][0][-1] == "redrawn" and logs["some"][0][-1] == "redrawn"
        assert [r[:-1] for r in logs["none"]] == logs["plain"]
        assert all(r[-1] == "0" for r in logs["none"][1:]) and all(r[-1] == "3" for r in logs["some"][1:])
        assert len(logs["some"]) == len(logs["plain"]) and all(float(r[-3]) < 0 for r in logs["some"][1:])
    with pytest.raises(SystemExit):
        mod.main(_cli_args(cli, tmp_path, "bad") + ["--refine_slots", "3"])
