"""The draw stage held to its definition on EXACTLY known logits (tests/draw_cases.py has the trick and the case table).

Every rule of include/hudiff_hip.h that decides something only at a tie or at a threshold -- the lowest index wins an argmax tie; the
truncation ranks on g with the lower index first among equals; `before_j < top_p * esum` is strict and `e_j >= min_p` is not; the rank-0
token is always kept; confident keys compare as (c_i, i); beam candidates tie to the smaller (w, j); -inf candidates rank behind every
finite one in (w, j) order -- is run on the device at an input built to decide it, through the public Python API, on the nine
instantiations of sample_step_k and on slot_conf_k / slot_select_k / beam_cand_k / beam_select_k.

The micro models are loaded with decoder.weight = 0 and decoder.bias[0:22] = P, so the logits are P bit for bit (test_premise; nothing
else in this module means anything if that fails).  Tokens, orders and parents are compared with array_equal, -inf positions must match
exactly, and a finite log-probability must sit within draw_cases.logp_bound = 4e-6 + 2^-22 |ref| of the float64 definition (derived there;
a beam score after t positions gets t times that).  tests/test_draw_cases_host.py proves that every comparison an expected result depends
on is a designed exact tie or has a margin of 1e-4: there is NO near-tie exemption here, no draw is left out.

One handle per (kind, decoder table), module scoped, lane_min_rows = 2 so that `lanes=2` really splits these tiny batches.  The antibody
model runs every case, the nanobody model (another Segs::row mapping) one case per kernel family."""
import numpy as np
import pytest

import draw_cases as DC
from conftest import load_cfg, load_weights
from test_gpu_logp import _mk

pytestmark = pytest.mark.gpu

WORST = {}                                               # kernel family -> worst |device - float64| / bound seen, and the absolute error


@pytest.fixture(scope="module")
def hip():
    import hudiff_amd
    if hudiff_amd.device_count() < 1:
        pytest.fail("no MI355X visible: GPU tests must run on the GPU box (there is no CPU fallback)")
    return hudiff_amd


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


def _names(family):
    return [c.name for c in DC.cases() if c.family == family and not c.error]


def _bitsame(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.int32), b.view(np.int32))


def _guide(case, b):
    from hudiff_amd import Guide
    return Guide(b.allow, b.bias, case.temperature) if case.guided else None


def _note(family, lp, ref, terms=1):
    """Finite values against the bound; the worst case of the family is kept for the report."""
    lp, ref = np.asarray(lp, np.float64).reshape(-1), np.asarray(ref, np.float64).reshape(-1)
    if not lp.size:
        return
    err, bound = np.abs(lp - ref), DC.logp_bound(ref, terms)
    i = int(np.argmax(err / bound))
    w = WORST.setdefault(family, [0.0, 0.0])
    if err[i] / bound[i] >= w[0]:
        w[0], w[1] = float(err[i] / bound[i]), float(err[i])
    w.append(float(err.max()))
    assert (err <= bound).all(), (family, float(err[i]), float(bound[i]), float(ref[i]), float(lp[i]))


def _fresh(m):
    """The launch tally counts a launch where it is issued, so a session that replays a graph the handle captured for an earlier session
    of the same shape counts nothing of its steps.  Changing an option (and putting it back) drops the captured graphs: the session that
    follows captures its own, and its tally is a witness."""
    m.set_option("lane_min_rows", 3)
    m.set_option("lane_min_rows", 2)
    m.debug_launch_tally()


def _path(tally, pruned, lanes, name):
    """The intended path ran: the lane count, and pruned tail against full block."""
    assert tally[f"sample_lanes_{lanes}"] > 0, (name, tally)
    assert (tally["tail_sliced"] + tally["tail_launches"] > 0) == pruned, (name, tally)


def _session(m, case, b, mode, lanes=2, graph=True, truncation="case", guide="case", q="case", full=None):
    """One session of the case through model.sample / model.score -> (tokens | None, logp | None, order); asserts from the launch tally that
    the intended path ran: pruned tail against full block, and the lane count."""
    kw = dict(dropout="off", guide=_guide(case, b) if guide == "case" else guide, truncation=case.truncation if truncation == "case" else truncation,
              slots_per_step=case.K, slot_policy=case.policy, prune=case.prune, lanes=lanes, graph=graph)
    args = (b.region, b.chain, b.order, b.T)
    q = b.q if isinstance(q, str) else q
    _fresh(m)
    if mode == "score":
        tok, lp = None, m.score(b.full if full is None else full, *args, parallel=False, **kw)
    elif mode == "record":
        tok, lp = m.sample(b.tokens, *args, q_noise=q, return_logp=True, **kw)
    else:
        tok, lp = m.sample(b.tokens, *args, q_noise=q, **kw), None
    _path(m.debug_launch_tally(), case.K == 1 and case.prune and case.policy == "given", lanes if b.B >= 2 else 1, case.name)
    return tok, lp, m.sample_order()


def _check(case, b, mode, got, perms, draws, family):
    """perms[b][t] = the entry that stands at position t, draws[b][t] = (token, float64 logp) expected there."""
    tok, lp, order = got
    want_order, want_tok = b.order.copy(), (b.full if mode == "score" else b.tokens).copy()
    ref = np.zeros((b.B, b.Tmax))
    for r in range(b.B):
        for t, (e, (j, v)) in enumerate(zip(perms[r], draws[r])):
            want_order[r, t] = b.order[r, e]
            want_tok[r, want_order[r, t]] = j
            ref[r, t] = v
    assert np.array_equal(order, want_order), (case.name, mode, order, want_order)
    if tok is not None:
        assert np.array_equal(tok, want_tok), (case.name, mode, np.argwhere(tok != want_tok), tok[tok != want_tok], want_tok[tok != want_tok])
    if lp is not None:
        live = np.arange(b.Tmax)[None, :] < b.T[:, None]
        assert (lp[~live] == 0).all() and not np.isnan(lp).any() and not np.isposinf(lp).any()
        assert np.array_equal(np.isneginf(lp), np.isneginf(ref)), (case.name, mode, lp, ref)
        fin = live & np.isfinite(ref)
        _note(family, lp[fin], ref[fin])
    return want_order


def _given(case):
    return [list(range(len(r))) for r in case.rows]


# ---- 0. the premise -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("table", ["main", "const", "huge"])
@pytest.mark.parametrize("kind", ["ab", "nb"])
def test_premise(handles, kind, table):
    """With the decoder zeroed the forward returns the table bit for bit, in every row and at every slot, masked tokens or not."""
    m = handles(kind, table)
    b = DC.batch(DC.case("plain_argmax/pruned"), kind)
    P = np.append(DC.TABLES[table], np.float32(DC.MASK_LOGIT))
    for tokens in (b.tokens, b.full):
        z = m(tokens, b.region, b.chain, dropout="off")
        assert z.shape == (b.B, b.L, 23) and _bitsame(z, np.broadcast_to(P, z.shape))


# ---- 1. the nine instantiations of the draw ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", _names("draw"))
def test_draw_case(handles, name):
    case = DC.case(name)
    m, b = handles("ab", case.table), DC.batch(case, "ab")
    fam = "draw/" + ("trunc" if case.truncation else "guided" if case.guided else "plain")
    for mode in case.modes:
        _check(case, b, mode, _session(m, case, b, mode), _given(case), DC.expect_draws(case, mode), fam)
    print(name, fam, WORST.get(fam, [0, 0])[:2])


def test_guided_overflow_is_numeric(handles):
    """A finite bias whose sum with the logit overflows to +inf at ONE allowed token: HD_ERR_NUMERIC, exactly as from a raw +inf logit.  The
    same bias in a truncated scoring session: esum is NaN, so every comparison of the cut fails, and the +inf token -- rank 0 on g -- is
    kept by the rank-0 rule alone: its log-probability is (g - mx) - logf(esum') = NaN by the formula, where a token that is not kept
    gets -inf."""
    from hudiff_amd import Truncation
    from hudiff_amd._lib import HD_ERR_NUMERIC, HudiffError
    case = DC.case("guided_overflow")
    m, b = handles("ab", "huge"), DC.batch(case, "ab")
    for mode in case.modes:
        with pytest.raises(HudiffError) as e:
            _session(m, case, b, mode)
        assert e.value.status == HD_ERR_NUMERIC, mode
    # the rows around it are untouched by the flag: the values of the scoring session (the last one) are the definition's
    lp = m.sample_logp(b.B, b.Tmax)
    ref = [DC.expect_entry(case, d, DC.noise_of(d), "score")[1] for d in (case.rows[0][0], case.rows[1][0])]
    _note("draw/guided", [lp[0, 0], lp[1, 0]], ref)
    # without the overflowing bias the same handle and batch run clean
    from hudiff_amd import Guide
    tok, lp, _ = _session(m, case, b, "record", guide=Guide(b.allow, None, 1.0))
    assert (tok[0, b.order[0, :2]] == 7).all() and np.isfinite(lp).all()
    with pytest.raises(HudiffError) as e:
        _session(m, case, b, "score", truncation=Truncation(top_p=0.5))
    assert e.value.status == HD_ERR_NUMERIC
    lp = m.sample_logp(b.B, b.Tmax)
    assert np.isnan(lp[0, 1]), lp                        # kept by the rank-0 rule (not -inf)
    assert lp[0, 0] == 0.0 and np.isneginf(lp[1, 0]), lp  # 2^104 stands alone at the top; token 5 is cut by top_p = 0.5


# ---- 2. the confident policy --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", _names("confident"))
def test_confident_case(handles, name):
    case = DC.case(name)
    m, b = handles("ab"), DC.batch(case, "ab")
    fam = "confident"
    got = {}
    for mode in case.modes:
        perms, states, draws = DC.expect_confident(case, mode)
        got[mode] = _session(m, case, b, mode)
        _check(case, b, mode, got[mode], perms, draws, fam)
    # recording and plain sampling sessions draw the same tokens in the same order
    assert np.array_equal(got["sample"][0], got["record"][0]) and np.array_equal(got["sample"][2], got["record"][2])
    # scoring the recorded tokens from the same candidate list, K and guide reproduces order and log-probabilities, bit for bit: targets,
    # allowed bits and bias travelled with their entries
    _, lp, order = _session(m, case, b, "score", full=np.where(got["record"][0] == 22, b.full, got["record"][0]))
    assert np.array_equal(order, got["record"][2]) and _bitsame(lp, got["record"][1])
    # the stable partition, seen after the first forward: chosen entries in (c, i) order, the others in their previous relative order
    perms, states, _ = DC.expect_confident(case, "record")
    m.sample_begin(b.tokens, b.region, b.chain, b.order, b.T, q_noise=b.q, dropout="off", record_logp=True, guide=_guide(case, b),
                   truncation=case.truncation, slots_per_step=case.K, slot_policy="confident")
    try:
        m.sample_run(0, min(case.K, b.Tmax))
        first = m.sample_order()
        if case.K < b.Tmax:
            m.sample_run(case.K, b.Tmax)
        last = m.sample_order()
    finally:
        tok = m.sample_end()
    for r in range(b.B):
        if b.T[r]:
            assert np.array_equal(first[r, :b.T[r]], b.order[r, states[r][0]]), (name, r, first[r], states[r][0])
        assert np.array_equal(first[r, b.T[r]:], b.order[r, b.T[r]:])
    assert np.array_equal(last, got["record"][2]) and np.array_equal(tok, got["record"][0]) and _bitsame(m.sample_logp(), got["record"][1])
    # replay: the given-order session at the realised order draws the same bits
    given = DC.replace(case, policy="given", prune=False)
    b2 = DC.batch(case, "ab")
    b2.order = last
    tok2, lp2, _ = _session(m, given, b2, "record")
    assert np.array_equal(tok2, tok) and _bitsame(lp2, got["record"][1])
    print(name, WORST.get(fam, [0, 0])[:2])


# ---- 3. the beam ----------------------------------------------------------------------------------------------------------------------------
def _beam(m, case, b, lanes=2, graph=True):
    """A beam session position by position -> [(score, parent, logp, tokens)] after every position, the final tokens."""
    _fresh(m)
    m.beam_begin(b.tokens, b.region, b.chain, b.order, b.T, case.W, guide=_guide(case, b), truncation=case.truncation, lanes=lanes, graph=graph)
    snaps = []
    try:
        for t in range(b.Tmax):
            m.sample_run(t, t + 1)
            score, parent, cand = m.beam_state()
            snaps.append((score, parent, m.sample_logp(), m.sample_tokens(), cand))
    finally:
        final = m.sample_end()
    _path(m.debug_launch_tally(), True, min(lanes, len(case.rows)), case.name)
    return snaps, final


def _check_beam(case, b, snaps, final, fam="beam"):
    steps = DC.expect_beam(case, b)
    for t, (st, (score, parent, lp, tokens, cand)) in enumerate(zip(steps, snaps)):
        ran = st["ran"]
        assert np.array_equal(parent[ran, t], st["parent"][ran]), (case.name, t, parent[:, t], st["parent"])
        assert np.array_equal(tokens, st["tokens"]), (case.name, t, np.argwhere(tokens != st["tokens"]))
        assert np.array_equal(tokens[ran, b.order[ran, t]], st["token"][ran])
        for dev, ref, terms in ((score, st["score"], t + 1), (lp[:, t], np.where(ran, st["logp"], 0.0), 1), (cand[ran], st["cand"][ran], t + 1)):
            assert not np.isnan(dev).any() and np.array_equal(np.isneginf(dev), np.isneginf(ref)), (case.name, t, dev, ref)
            fin = np.isfinite(ref)
            _note(fam, dev[fin], ref[fin], terms)
        assert (lp[~ran, t] == 0).all() and (parent[~ran, t] == 0).all()
        # rows stand in score order, and the device's own table selects what the device selected (guide.beam_select, bit for bit)
        from hudiff_amd.guide import beam_select
        for g in range(len(case.rows)):
            r0 = g * case.W
            if ran[r0]:
                w, j, v = beam_select(cand[r0:r0 + case.W], case.W)
                assert np.array_equal(w, parent[r0:r0 + case.W, t]) and _bitsame(v, score[r0:r0 + case.W])
    assert np.array_equal(final, steps[-1]["tokens"]) and ((final >= 0) & (final <= 22)).all()
    vis = np.zeros(final.shape, bool)
    for r in range(b.B):
        vis[r, b.order[r, :b.T[r]]] = True
    assert (final[vis] <= 21).all() and np.array_equal(final[~vis], b.tokens[~vis])      # dead rows keep valid tokens


@pytest.mark.parametrize("name", _names("beam"))
def test_beam_case(handles, name):
    case = DC.case(name)
    m, b = handles("ab"), DC.batch(case, "ab")
    _check_beam(case, b, *_beam(m, case, b))
    print(name, WORST.get("beam", [0, 0])[:2])


# ---- 4. the other model, the other launch forms ---------------------------------------------------------------------------------------------
FAMILY_CASE = {"draw": "trunc_guided_topk2", "confident": "confident_K2", "beam": "beam_W3"}


@pytest.mark.parametrize("family", sorted(FAMILY_CASE))
def test_nanobody_runs_one_case_per_family(handles, family):
    case = DC.case(FAMILY_CASE[family])
    m, b = handles("nb"), DC.batch(case, "nb")
    if family == "beam":
        _check_beam(case, b, *_beam(m, case, b), fam="beam/nb")
        return
    for mode in case.modes:
        if family == "draw":
            perms, draws = _given(case), DC.expect_draws(case, mode)
        else:
            perms, _, draws = DC.expect_confident(case, mode)
        _check(case, b, mode, _session(m, case, b, mode), perms, draws, family + "/nb")


@pytest.mark.parametrize("family", sorted(FAMILY_CASE))
def test_lanes_and_eager_launches_are_bit_equal(handles, family):
    """lanes = 2 (lane_min_rows = 2: the batch really splits), one lane, and graph=False give the same bits."""
    case = DC.case(FAMILY_CASE[family])
    m, b = handles("ab"), DC.batch(case, "ab")
    runs = []
    for lanes, graph in ((2, True), (1, True), (2, False)):
        if family == "beam":
            snaps, final = _beam(m, case, b, lanes=lanes, graph=graph)
            runs.append([final] + [x for s in snaps for x in s])
        else:
            runs.append([x for mode in case.modes for x in _session(m, case, b, mode, lanes=lanes, graph=graph) if x is not None])
    for other in runs[1:]:
        assert len(other) == len(runs[0])
        for x, y in zip(runs[0], other):
            assert _bitsame(x, y) if x.dtype == np.float32 else np.array_equal(x, y), family


# ---- 5. witnesses: every instantiation was reached ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["sample", "record", "score"])
def test_every_instantiation_changes_something(handles, mode):
    """<mode, plain>, <mode, guided> and <mode, guided + truncation>: the case differs from its neutral session -- without the truncation,
    without the guide, and (plain: there is nothing to take away but the noise) with all-ones noise or other targets."""
    m = handles("ab")

    def differs(x, y):
        return any(a is not None and not np.array_equal(a, c) for a, c in zip(x[:2], y[:2]))
    # guided + truncation against guided
    case = DC.case("trunc_guided_topk2")
    b = DC.batch(case, "ab")
    assert differs(_session(m, case, b, mode), _session(m, case, b, mode, truncation=None))
    # truncation without a guide against the plain kernel
    case = DC.case("trunc_topk3/pruned")
    b = DC.batch(case, "ab")
    assert differs(_session(m, case, b, mode), _session(m, case, b, mode, truncation=None))
    # guided against plain
    case = DC.case("guided_argmax/pruned")
    b = DC.batch(case, "ab")
    assert differs(_session(m, case, b, mode), _session(m, case, b, mode, guide=None))
    # plain: the noise of every position is read where it belongs (sampling), the target is the one scored (scoring)
    case = DC.case("plain_argmax/pruned")
    b = DC.batch(case, "ab")
    if mode == "score":
        other = b.full.copy()
        other[0, b.order[0, 0]] = 10
        assert differs(_session(m, case, b, mode), _session(m, case, b, mode, full=other))
    else:
        assert differs(_session(m, case, b, mode), _session(m, case, b, mode, q=np.ones_like(b.q)))


def test_report_worst_errors():
    """Not a check of its own (every value was asserted where it was measured): prints the worst |device - float64| per kernel family."""
    for fam in sorted(WORST):
        print(f"{fam}: worst |logp - float64| {max(WORST[fam][2:]):.3e}; worst error / bound {WORST[fam][0]:.3f} (absolute {WORST[fam][1]:.3e})")
    assert all(w[0] <= 1.0 for w in WORST.values())
