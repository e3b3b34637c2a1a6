"""Truncated sampling on the GPU (hd_set_truncation): top-k, top-p and min-p inside the device draw.

The yardstick is the float64 definition (hudiff_amd.guide.truncation_keep, include/hudiff_hip.h "truncated sampling") applied to the CPU
oracle's logits.  Tolerances are the siblings': REF_TOL = 2e-4 (device log-probability against the float64 oracle), PAIR_TOL = 4e-4 (two
device results), GAP_TOL = 4e-4 (twice the bound on one score: below it the oracle cannot call a comparison).  The device's g, and with
it its log e = g - max g and its head masses, sit within that bound of the oracle's, so a draw is "too close to call" -- and left out,
under a cap -- when a quantity the cut compares lies within GAP_TOL of its threshold (`_too_close`) or the two best kept scores lie
within GAP_TOL of each other.  Every other draw must be the oracle's argmax over the oracle's keep-set with the oracle's
log-probability within REF_TOL.

The batch is tests/test_gpu_guide.py's (40 rows, tcap 6, T[5] = 0, T[17] = 3, 231 draws, its random guide, SEED / ROW0, dropout off).
The cap on draws left out is 6 of 231 per case: computed on the CPU for exactly these inputs, with the oracle following its own
tokens, the reference alone leaves out at most 4 (per case, K = 6 then K = 1; ab | nb):
    (5, 1, 0)       0 / 0 | 1 / 0        (0, 0.9, 0)      2 / 1 | 4 / 4
    (0, 1, 0.1)     3 / 1 | 1 / 0        (8, 0.8, 0.05)   1 / 2 | 3 / 2
and these settings remove between 900 and 1501 allowed tokens over the 231 draws."""
import os

import numpy as np
import pytest

import hudiff_oracle as ho
from conftest import load_cfg, load_weights, prec
from test_gpu_block import _batch, _logits64
from test_gpu_guide import ALL, GAP_TOL, ROW0, SEED, _bits, _live, _visited
from test_gpu_logp import PAIR_TOL, REF_TOL, _ab_checkpoint, _mk

pytestmark = pytest.mark.gpu

KW = dict(seed=SEED, row0=ROW0, dropout="off")
SETTINGS = [(5, 1.0, 0.0), (0, 0.9, 0.0), (0, 1.0, 0.1), (8, 0.8, 0.05)]
MIXED = (8, 0.8, 0.05)
LEFT_OUT_CAP = 6


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
    models = {"kind": kind, "m0": _mk(hip, kind, cfg, sd), "o0": ho.OracleNet(kind, cfg, sd, dtype=np.float64)}
    yield models
    models["m0"].close()


def _tr(setting):
    from hudiff_amd import Truncation
    return Truncation(*setting)


def _guide(micro, temperature=1.0):
    from hudiff_amd import Guide
    _, _, _, allow, bias = _batch(micro["kind"])
    return Guide(allow, bias, temperature)


def _args(micro):
    batch, order, T, _, _ = _batch(micro["kind"])
    return (batch["tokens"], batch["region"], batch["chain"], order, T)


def _same(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b))


def _g64(z22, allow=None, bias=None):
    """The draw's g at temperature 1, float64: z + bias over the allowed tokens, -inf elsewhere."""
    g = np.asarray(z22, np.float64)
    if bias is not None:
        g = g + np.asarray(bias, np.float64)
    if allow is not None:
        g = np.where(_bits(allow, np.arange(22)), g, -np.inf)
    return g


def _too_close(g, tr, keep):
    """A comparison of the cut that the oracle cannot call for the device (module docstring): g [22] float64, keep = the oracle's set."""
    al = g > -np.inf
    mx = g.max()
    e = np.where(al, np.exp(g - mx), 0.0)
    gs = np.sort(g[al])[::-1]
    if 0 < tr.top_k < 22 and len(gs) > tr.top_k and gs[tr.top_k - 1] - gs[tr.top_k] < GAP_TOL:
        return True
    if tr.top_p < 1.0:
        idx = np.arange(22)
        ahead = al[None, :] & ((g[None, :] > g[:, None]) | ((g[None, :] == g[:, None]) & (idx[None, :] < idx[:, None])))
        before = np.where(ahead, e[None, :], 0.0).sum(-1)
        if (np.abs(before[al] / e.sum() - tr.top_p) < GAP_TOL).any():
            return True
    if tr.min_p > 0.0 and (np.abs(g[al] - mx - np.log(tr.min_p)) < GAP_TOL).any():
        return True
    dropped = al & ~keep
    if dropped.any() and g[keep].min() - g[dropped].max() < GAP_TOL:
        return True
    return False


def _replay(micro, tok, lp, K, tr, allow, bias, label):
    """The definition in float64, one oracle forward per group of K positions from the state at the group's start; the DEVICE's tokens
    are written for the next group (tests/test_gpu_block.py `_replay`, with the cut).  -> draws left out."""
    from hudiff_amd.guide import truncation_keep
    kind = micro["kind"]
    batch, order, T, _, _ = _batch(kind)
    B, tcap = order.shape
    state = batch["tokens"].copy()
    cases = left_out = removed = 0
    worst_lp = 0.0
    for t0 in range(0, tcap, K):
        z = _logits64(micro, state, batch["region"], batch["chain"])
        nxt = state.copy()
        for t in range(t0, min(t0 + K, tcap)):
            q = ho.philox_exp_noise(SEED, ROW0 + np.arange(B), t).astype(np.float64)
            for b in range(B):
                if t >= T[b]:
                    continue
                s = order[b, t]
                g = _g64(z[b, s], None if allow is None else allow[b, s], None if bias is None else bias[b, s])
                keep = truncation_keep(g, tr)
                removed += int((g > -np.inf).sum() - keep.sum())
                gk = np.where(keep, g, -np.inf)
                lsm = gk - gk.max()
                lsm = lsm - np.log(np.exp(lsm).sum())
                score = np.where(keep, g - np.log(q[b]), -np.inf)
                top = np.sort(score[keep])[::-1]
                gap = top[0] - top[1] if len(top) > 1 else np.inf
                got = int(tok[b, s])
                cases += 1
                if _too_close(g, tr, keep) or gap < GAP_TOL:
                    left_out += 1
                else:
                    assert got == int(np.argmax(score)), (label, b, t, got, int(np.argmax(score)), gap)
                    assert keep[got], (label, b, t, got)
                    err = abs(float(lp[b, t]) - lsm[got])
                    worst_lp = max(worst_lp, err)
                    assert err < REF_TOL, (label, b, t, err)
                nxt[b, s] = got
        state = nxt
    print(f"{kind} {label} K {K}: {cases} draws, {left_out} left out, {removed} allowed tokens removed, |logp - oracle| {worst_lp:.2e} "
          f"(bound {REF_TOL:.1e})")
    assert cases == int(T.sum()) == 231
    assert left_out <= LEFT_OUT_CAP
    return left_out, removed


# ---- 1. a neutral truncation is no truncation, bit for bit ---------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["K1", "K1_noprune", "K6", "K3_confident"])
def test_neutral_is_untouched(micro, form):
    from hudiff_amd import Truncation
    m = micro["m0"]
    more = {"K1": {}, "K1_noprune": {"prune": False}, "K6": {"slots_per_step": 6},
            "K3_confident": {"slots_per_step": 3, "slot_policy": "confident"}}[form]
    for guide in (None, _guide(micro)):
        kw = dict(KW, return_logp=True, guide=guide, **more)
        tok0, lp0 = m.sample(*_args(micro), **kw)
        od0 = m.sample_order()
        for tr in (Truncation(), Truncation(top_k=22)):
            tok1, lp1 = m.sample(*_args(micro), truncation=tr, **kw)
            assert _same((tok1, lp1, m.sample_order()), (tok0, lp0, od0)), (form, tr)
        # ... and a cut is another session
        tok2, lp2 = m.sample(*_args(micro), truncation=Truncation(top_k=2), **kw)
        assert not np.array_equal(lp2, lp0)


# ---- 2. against the float64 definition -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("setting", SETTINGS, ids=[str(s) for s in SETTINGS])
def test_truncated_draw_against_the_float64_definition(micro, setting):
    m, tr = micro["m0"], _tr(setting)
    _, _, T, allow, bias = _batch(micro["kind"])
    live = _live(T, 6)
    removed = []
    for K, lanes in ((6, 2), (1, 1), (1, 2)):
        tok, lp = m.sample(*_args(micro), return_logp=True, guide=_guide(micro), truncation=tr, slots_per_step=K, lanes=lanes, **KW)
        assert (lp[~live] == 0).all() and (lp[live] <= 0).all() and np.isfinite(lp).all()
        removed.append(_replay(micro, tok, lp, K, tr, allow, bias, f"guided {setting} lanes {lanes}")[1])
    assert all(r >= 900 for r in removed), removed               # the cut is exercised (of about 2650 allowed tokens over the draws)


def test_truncated_draw_without_a_guide(micro):
    m, tr = micro["m0"], _tr((5, 1.0, 0.0))
    for K in (6, 1):
        tok, lp = m.sample(*_args(micro), return_logp=True, truncation=tr, slots_per_step=K, **KW)
        _, removed = _replay(micro, tok, lp, K, tr, None, None, "unguided (5, 1, 0)")
        assert removed == 231 * 17


# ---- 3. exact identities ----------------------------------------------------------------------------------------------------------------
def test_top_k_1_is_the_greedy_decode(micro):
    m, tr = micro["m0"], _tr((1, 1.0, 0.0))
    _, order, T, _, _ = _batch(micro["kind"])
    live = _live(T, order.shape[1])
    for K in (1, 6):
        greedy = m.sample(*_args(micro), guide=_guide(micro, 0.0), slots_per_step=K, **KW)
        tok, lp = m.sample(*_args(micro), guide=_guide(micro), truncation=tr, return_logp=True, slots_per_step=K, **KW)
        assert np.array_equal(tok, greedy)
        assert (lp == 0.0).all() and live.sum() == 231
        # greedy with the cut: the same token again (the argmax is always kept), and its log-probability under the cut is 0
        tok, lp = m.sample(*_args(micro), guide=_guide(micro, 0.0), truncation=tr, return_logp=True, slots_per_step=K, **KW)
        assert np.array_equal(tok, greedy) and (lp == 0.0).all()


def test_top_k_1_confident_keys_are_all_one(micro):
    """Every key is exactly 1, so the rank is the list position and the order comes back unchanged."""
    m = micro["m0"]
    _, order, _, _, _ = _batch(micro["kind"])
    for guide in (None, _guide(micro)):
        m.sample(*_args(micro), guide=guide, truncation=_tr((1, 1.0, 0.0)), slots_per_step=3, slot_policy="confident", **KW)
        assert np.array_equal(m.sample_order(), order)
        m.sample(*_args(micro), guide=guide, slots_per_step=3, slot_policy="confident", **KW)
        assert not np.array_equal(m.sample_order(), order)


# ---- 4. sample, then score under the same truncation ---------------------------------------------------------------------------------------
def test_sample_then_score_under_the_same_truncation(micro):
    m, tr, g = micro["m0"], _tr(MIXED), _guide(micro)
    batch, order, T, allow, bias = _batch(micro["kind"])
    args = _args(micro)[1:]
    live = _live(T, order.shape[1])
    for K in (1, 3):
        tok, lp = m.sample(*_args(micro), return_logp=True, guide=g, truncation=tr, slots_per_step=K, **KW)
        seq = m.score(tok, *args, parallel=False, guide=g, truncation=tr, slots_per_step=K)
        par = m.score(tok, *args, parallel=True, device_batch=100, guide=g, truncation=tr, slots_per_step=K)
        e_seq, e_par = float(np.abs(seq - lp).max()), float(np.abs(par - lp).max())
        print(f"{micro['kind']} K {K}: |seq - record| {e_seq:.2e}  |par - record| {e_par:.2e}  (bound {PAIR_TOL:.1e})")
        assert np.isfinite(seq).all() and np.isfinite(par).all()
        assert e_seq < PAIR_TOL and e_par < PAIR_TOL
        assert (seq[~live] == 0).all() and (par[~live] == 0).all() and (seq[live] <= 0).all()
        # the cut really entered: the untruncated score of the same tokens is another number
        assert np.abs(m.score(tok, *args, parallel=False, guide=g, slots_per_step=K) - seq).max() > 1e-2
    # a target the cut removes: probability 0, no error, the tokens come back as given
    top1 = _tr((1, 1.0, 0.0))
    tok = m.sample(*_args(micro), guide=g, truncation=top1, **KW)
    b, t = 21, 2
    s = order[b, t]
    bad = tok.copy()
    bad[b, s] = next(j for j in range(22) if (int(allow[b, s]) >> j) & 1 and j != tok[b, s])
    for parallel in (False, True):
        sc = m.score(bad, *args, parallel=parallel, guide=g, truncation=top1)
        assert np.isneginf(sc[b, t]) and (sc[~live] == 0).all()
        rest = live.copy()
        rest[b, t:] = False                                   # (later steps of the row are conditioned on the changed token)
        # every other target is the top-1 token of its step: log-probability exactly 0 (an expanded row of the step-parallel form
        # runs in another batch, where a near tie for the top may fall the other way: -inf there, and nothing else)
        assert np.isin(sc[rest], (0.0, -np.inf)).all() and (sc[rest] == 0.0).sum() >= rest.sum() - (2 if parallel else 0)
    m.score_begin(bad, *args, guide=g, truncation=top1)
    m.sample_run(0, order.shape[1])
    assert np.array_equal(m.sample_end(), bad)
    assert np.isneginf(m.sample_logp()[b, t])
    # temperature 0 stays an error of the begin, and the failed begin consumed the truncation
    from hudiff_amd._lib import HD_ERR_INVALID, HudiffError
    with pytest.raises(HudiffError) as e:
        m.score(tok, *args, parallel=False, guide=_guide(micro, 0.0), truncation=top1)
    assert e.value.status == HD_ERR_INVALID
    assert np.isfinite(m.score(bad, *args, parallel=False, guide=g)).all()


# ---- 5. the confident policy uses the truncated key ------------------------------------------------------------------------------------------
def test_confident_selection_uses_the_truncated_key(micro):
    from hudiff_amd.guide import confidence_keys, truncation_keep
    m, tr, g = micro["m0"], _tr(MIXED), _guide(micro)
    kind = micro["kind"]
    batch, order, T, allow, bias = _batch(kind)
    K = 3
    tok, lp = m.sample(*_args(micro), return_logp=True, guide=g, truncation=tr, slots_per_step=K, slot_policy="confident", **KW)
    R = m.sample_order()
    z = _logits64(micro, batch["tokens"], batch["region"], batch["chain"])
    rows = skipped = differs = 0
    for b in range(len(T)):
        if T[b] <= K:
            continue
        rows += 1
        slots = order[b, :T[b]]
        gs = [_g64(z[b, s], allow[b, s], bias[b, s]) for s in slots]
        close = any(_too_close(gi, tr, truncation_keep(gi, tr)) for gi in gs)
        c = np.exp(confidence_keys(z[b, slots], allow[b, slots], bias[b, slots], 1.0, truncation=tr))
        rank = np.lexsort((np.arange(len(slots)), c))
        if close or abs(c[rank[K]] - c[rank[K - 1]]) < 1e-3 * c[rank[K - 1]]:
            skipped += 1
            continue
        assert set(R[b, :K].tolist()) == set(slots[rank[:K]].tolist()), (b, R[b, :T[b]], slots[rank])
        c0 = np.exp(confidence_keys(z[b, slots], allow[b, slots], bias[b, slots], 1.0))
        differs += set(slots[np.lexsort((np.arange(len(slots)), c0))[:K]].tolist()) != set(slots[rank[:K]].tolist())
        assert sorted(R[b, :T[b]].tolist()) == sorted(slots.tolist()) and np.array_equal(R[b, T[b]:], order[b, T[b]:])
    print(f"{kind}: {rows} rows, {skipped} skipped, the truncated choice differs from the untruncated one in {differs}")
    assert rows == 38 and skipped <= 4
    assert differs >= 1                                      # (or the untruncated key would pass this test as well)
    # replay with truncation: the given-order session at the realised order draws the same bits
    tok2, lp2 = m.sample(batch["tokens"], batch["region"], batch["chain"], R, T, return_logp=True, guide=g, truncation=tr, slots_per_step=K, **KW)
    assert np.array_equal(tok2, tok) and np.array_equal(lp2, lp)
    assert np.array_equal(m.sample_order(), R)


# ---- 6. lifetime ----------------------------------------------------------------------------------------------------------------------
def test_truncation_lifetime(micro):
    from hudiff_amd import Guide, Truncation
    from hudiff_amd._lib import HD_ERR_INVALID, HD_ERR_STATE, HdTruncation, HudiffError
    import ctypes as C
    m, tr = micro["m0"], _tr(MIXED)
    batch, order, T, allow, bias = _batch(micro["kind"])
    B, tcap = order.shape
    args = _args(micro)
    rkw = dict(KW, return_logp=True)
    plain = m.sample(*args, **rkw)
    cut = m.sample(*args, truncation=tr, **rkw)
    assert not np.array_equal(cut[1], plain[1])
    # one shot
    assert _same(m.sample(*args, **rkw), plain)
    m.set_truncation(tr)
    assert _same(m.sample(*args, **rkw), cut) and _same(m.sample(*args, **rkw), plain)
    # NULL clears; a neutral one clears as well; hd_forward neither uses nor clears it
    m.set_truncation(tr); m.set_truncation(None)
    assert _same(m.sample(*args, **rkw), plain)
    m.set_truncation(tr); m.set_truncation(Truncation(top_k=22))
    assert _same(m.sample(*args, **rkw), plain)
    m.set_truncation(tr)
    m(batch["tokens"][:2], batch["region"][:2], None if batch["chain"] is None else np.concatenate([batch["chain"][:2], batch["chain"][B:B + 2]]))
    assert _same(m.sample(*args, **rkw), cut)
    # consumed by a begin that fails: the wrong B of a guide
    m.set_truncation(tr)
    m.set_guide(Guide(allow[:B - 1], bias[:B - 1], 1.0))
    with pytest.raises(HudiffError) as e:
        m.sample(*args, **rkw)
    assert e.value.status == HD_ERR_INVALID
    assert _same(m.sample(*args, **rkw), plain)
    # kept by a restart; HD_ERR_STATE inside an open session
    m.sample_begin(*args, truncation=tr, record_logp=True, **KW)
    with pytest.raises(HudiffError) as e:
        m.set_truncation(tr)
    assert e.value.status == HD_ERR_STATE
    with pytest.raises(HudiffError) as e:
        m.set_truncation(None)
    assert e.value.status == HD_ERR_STATE
    m.sample_run(0, tcap)
    assert _same((m.sample_tokens(), m.sample_logp()), cut)
    m.sample_restart(SEED + 1)
    m.sample_run(0, tcap)
    other = m.sample_logp()
    assert not np.array_equal(other, cut[1])
    m.sample_restart(SEED)
    m.sample_run(0, tcap)
    lp = m.sample_logp()
    assert _same((m.sample_end(), lp), cut)
    assert _same(m.sample(*args, **rkw), plain)
    # with top_k = 1 every recorded log-probability is exactly 0, whatever the seed: the restarted sample was cut as well
    m.sample_begin(*args, truncation=Truncation(top_k=1), record_logp=True, **KW)
    m.sample_run(0, tcap)
    first = m.sample_tokens()
    m.sample_restart(SEED + 2)
    m.sample_run(0, tcap)
    lp = m.sample_logp()
    assert np.array_equal(m.sample_end(), first) and (lp == 0.0).all() and plain[1].min() < -1.0
    # what hd_set_truncation itself refuses (the Python value object refuses the same before the library sees it)
    for bad in ((-1, 1.0, 0.0), (23, 1.0, 0.0), (0, 0.0, 0.0), (0, 1.5, 0.0), (0, float("nan"), 0.0), (0, 1.0, -0.1), (0, 1.0, 1.5),
                (0, 1.0, float("nan")), (0, float("inf"), 0.0)):
        t = HdTruncation(*bad)
        assert m._lib.hd_set_truncation(m._h, C.byref(t)) == HD_ERR_INVALID, bad
    assert _same(m.sample(*args, **rkw), plain)


@pytest.mark.parametrize("kind", ["ab", "nb"])
def test_lnsync_guard_repeats_a_truncated_session(hip, kind):
    """Production width, the batch of the siblings' guard tests (the micro models' launches hold no ln_sync meeting).  With top_k = 1
    every recorded log-probability is exactly 0, which an untruncated session of these weights is far from: the repeat was cut.  The
    repeat normalises in separate passes, so the best token may legitimately change at a near tie against the undisturbed session; the
    rows that agree are counted and printed."""
    from hudiff_amd import Truncation, evalsets as E, synthetic as S
    cfg = dict(S.AB_CONFIG if kind == "ab" else S.NB_CONFIG, dropout=0.0)
    mx = _mk(hip, kind, cfg, S.random_state_dict(kind, cfg, seed=0), precision="split")
    try:
        big = E.eval_batch("huab348" if kind == "ab" else "vhh", 128 if kind == "ab" else 160, row0=0)
        T = np.minimum(big["T"], 4)
        args = (big["tokens"], big["region"], big["chain"], big["order"], T)
        kw = dict(seed=13, row0=0, return_logp=True)
        tr = Truncation(top_k=1)
        live = _live(T, big["order"].shape[1])
        one = mx.sample(*args, **kw)
        want = mx.sample(*args, truncation=tr, **kw)
        assert (want[1] == 0.0).all() and one[1][live].max() < -1.0 and not np.array_equal(want[0], one[0])
        prec(mx, lnsync_in_use=True, lnsync_fallbacks=0, last_call_repeated=False)
        mx.debug_fail_next_lnsync()
        with pytest.warns(RuntimeWarning, match="ln_sync"):
            again = mx.sample(*args, truncation=tr, **kw)
        prec(mx, lnsync_in_use=False, lnsync_fallbacks=1, last_call_repeated=True)
        assert (again[1] == 0.0).all()
        agree = (again[0] == want[0]).all(axis=1)
        print(f"{kind}: ln_sync guard in a truncated session: {int(agree.sum())} of {len(T)} rows draw the undisturbed tokens")
        assert not np.array_equal(again[0], one[0])
        assert np.array_equal(mx.sample(*args, **kw)[0], one[0])          # the session after it is untruncated
    finally:
        mx.close()


# ---- 7. CLI ------------------------------------------------------------------------------------------------------------------------------
def test_cli_top_p(hip, tmp_path, monkeypatch):
    """The antibody sampler with --top_p 0.9 --logp_fpath: every sidecar value is the sum of the row's recorded log-probabilities, and
    those are model.score(..., truncation=) of the sampled tokens along the sampler's own order, within PAIR_TOL."""
    from hudiff_amd import Truncation, sampler
    from hudiff_amd.cli import sample as cli
    from test_gpu_cli import _write_inputs
    csv, nb = _write_inputs(tmp_path, "ab", 3)
    calls = []
    real = sampler.sample_jobs

    def recording(model, jobs, replicas, seed, **kw):
        res = real(model, jobs, replicas, seed, **kw)
        calls.append((list(jobs), dict(kw), res))
        return res
    monkeypatch.setattr(sampler, "sample_jobs", recording)
    monkeypatch.setattr(cli, "sample_jobs", recording)
    ck = tmp_path / "cut" / "checkpoints" / "hudiffab.pt"
    _ab_checkpoint(ck)
    sidecar = tmp_path / "logp.csv"
    out = cli.main(["--ckpt", str(ck), "--data_fpath", str(csv), "--numbered_fpath", str(nb), "--logp_fpath", str(sidecar),
                    "--dropout", "off", "--top_p", "0.9", "--batch_size", "3", "--seed", "5"])
    monkeypatch.undo()
    assert open(out).read().count("humanization,") >= 3
    lines = open(sidecar).read().splitlines()[1:]
    tr = Truncation(top_p=0.9)
    assert calls and all(kw.get("truncation") == tr and kw.get("return_logp") for _, kw, _ in calls)
    m = _mk(hip, "ab", load_cfg("ab"), load_weights("ab"))
    totals = {}
    try:
        for jobs, kw, (res, res_lp) in calls:
            for a, job in enumerate(jobs):
                R, Tn = res.shape[2], len(job.loc)
                order = np.repeat(np.asarray(job.loc, np.int32)[None], R, 0)
                ch = np.array([job.chain[0]] * R + [job.chain[1]] * R, np.int32)
                lp = res_lp[a, 0]
                reg = np.repeat(job.region[None], R, 0)
                want = m.score(res[a, 0], reg, ch, order, np.full(R, Tn), parallel=False, truncation=tr)
                err = float(np.abs(want - lp[:, :Tn]).max())
                assert np.isfinite(want).all() and err < PAIR_TOL, (job.name, err)
                assert np.abs(m.score(res[a, 0], reg, ch, order, np.full(R, Tn), parallel=False) - want).max() > 1e-2
                for r in range(R):
                    totals[(str(job.name), r)] = (Tn, float(lp[r].astype(np.float64).sum()), float(want[r].astype(np.float64).sum()))
        assert len(lines) == len(totals)
        for line in lines:
            f = line.split(",")
            Tn, total, scored = totals[(f[0], int(f[2]))]
            assert int(f[-3]) == Tn and abs(float(f[-2]) - total) < 1e-6 + 1e-6 * abs(total), line
            assert abs(float(f[-2]) - scored) < Tn * PAIR_TOL, line
    finally:
        m.close()
    # without the flags the run is today's, byte for byte; --top_p 1 --top_k 0 --min_p 0 is no flag
    outs = []
    for i, extra in enumerate(([], ["--top_p", "1", "--top_k", "0", "--min_p", "0"])):
        ck = tmp_path / f"plain{i}" / "checkpoints" / "hudiffab.pt"
        _ab_checkpoint(ck)
        o = cli.main(["--ckpt", str(ck), "--data_fpath", str(csv), "--numbered_fpath", str(nb), "--batch_size", "3", "--seed", "5"] + extra)
        outs.append([open(o, "rb").read(), open(os.path.join(os.path.dirname(o), "sample_identity.fa"), "rb").read()])
    assert outs[0] == outs[1]
