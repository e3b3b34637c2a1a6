"""Guided sampling on the GPU (hd_set_guide): per-slot allowed residues, logit bias, temperature, greedy decode.

Tolerances.  The project bounds every logit by 1e-4 against the reference.  A guided log-probability is log_softmax of
g = (z + bias) / temperature over the allowed tokens, so it moves by at most 2 * 1e-4 / temperature (its own logit and the
log-sum-exp each by 1e-4 / temperature): REF_TOL / min(temperature, 1) against the float64 oracle, twice that between two device
results.  The drawn token is the argmax of g_j - log q_j; it can differ from the oracle's only where the oracle's best two scores are
closer than twice the bound on one score, 4e-4 / min(temperature, 1).  Such draws are left out, and their number is capped."""
import os

import numpy as np
import pytest

import hudiff_oracle as ho
from conftest import chain_or_none, load_cfg, load_golden, load_weights, prec
from test_gpu_logp import PAIR_TOL, REF_TOL, _ab_checkpoint, _load_prod, _mk, _nb_checkpoint, _ragged

pytestmark = pytest.mark.gpu

ALL = (1 << 22) - 1
GAP_TOL = 4e-4          # twice the bound on one score: below it the oracle cannot call a draw


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
    models = {"kind": kind, "m0": _mk(hip, kind, cfg, sd), "o0": ho.OracleNet(kind, cfg, sd)}
    yield models
    models["m0"].close()


def _bits(allow, tokens):
    """allow [...] uint32, tokens [...] -> bool: the token's bit is set."""
    return ((np.asarray(allow, np.int64) >> np.asarray(tokens, np.int64)) & 1).astype(bool)


def _random_guide(B, L, seed=5):
    """The guide of the issue's oracle test: random non-empty allowed sets, N(0, 1) bias."""
    rng = np.random.default_rng(seed)
    allow = rng.integers(1, 1 << 22, (B, L))
    allow = (allow | (1 << rng.integers(0, 22, (B, L)))).astype(np.uint32)
    bias = rng.normal(0, 1, (B, L, 22)).astype(np.float32)
    return allow, bias


def _live(T, tcap):
    return np.arange(tcap)[None, :] < np.asarray(T)[:, None]


def _visited(order, T, L):
    v = np.zeros((len(T), L), bool)
    for b in range(len(T)):
        v[b, order[b, :T[b]]] = True
    return v


# ---- 1. the neutral guide is the unguided session, bit for bit ---------------------------------------------------------------------
NEUTRAL_VARIANTS = [
    ("graph", {}, {}),
    ("eager", {}, {"graph": False}),
    ("loop", {}, {"graph": "loop"}),
    ("noprune", {}, {"prune": False}),
    ("tail0", {"options": {"tail_form": 0}}, {}),
    ("tail2", {"options": {"tail_form": 2}}, {}),
    ("lanes2", {"options": {"lane_min_rows": 2}}, {"lanes": 2}),
]
NEUTRAL_TRACE = {"ab": "micro_ab_sample_finetune.npz", "nb": "micro_nb_sample_plain.npz"}


@pytest.mark.parametrize("kind", ["ab", "nb"])
@pytest.mark.parametrize("variant", NEUTRAL_VARIANTS, ids=[v[0] for v in NEUTRAL_VARIANTS])
def test_neutral_guide_equals_unguided(hip, kind, variant):
    """All 22 bits, zero bias, temperature 1: the guided kernels draw the reference's recorded tokens, and their tokens and recorded
    log-probabilities are those of the unguided kernels bit for bit (sampling and scoring)."""
    from hudiff_amd import Guide
    _, mkw, skw = variant
    z = load_golden(NEUTRAL_TRACE[kind])
    tokens, region, chain, loc, q, final = z["tokens"], z["region"], chain_or_none(z), z["loc"], z["q"], z["final"]
    B, L = tokens.shape
    order, T = np.repeat(loc[None], B, 0), np.full(B, len(loc))
    neutral = Guide(np.full((B, L), ALL, np.uint32), np.zeros((B, L, 22), np.float32), 1.0)
    m = _mk(hip, kind, load_cfg(kind), load_weights(kind), **mkw)
    try:
        tok0, lp0 = m.sample(tokens, region, chain, order, T, q_noise=q, return_logp=True, **skw)
        tok1, lp1 = m.sample(tokens, region, chain, order, T, q_noise=q, return_logp=True, guide=neutral, **skw)
        assert np.array_equal(tok1, final)
        assert np.array_equal(tok1, tok0) and np.array_equal(lp1, lp0)
        assert (lp1 < 0).all()
        # the plain (not recording) guided kernel, and a guide without arrays (temperature only)
        assert np.array_equal(m.sample(tokens, region, chain, order, T, q_noise=q, guide=neutral, **skw), final)
        assert np.array_equal(m.sample(tokens, region, chain, order, T, q_noise=q, guide=Guide(), **skw), final)
        s0 = m.score(final, region, chain, order, T, parallel=False, **skw)
        s1 = m.score(final, region, chain, order, T, parallel=False, guide=neutral, **skw)
        assert np.array_equal(s1, s0)
    finally:
        m.close()


@pytest.mark.parametrize("kind", ["ab", "nb"])
def test_neutral_guide_equals_unguided_with_dropout(hip, kind):
    from hudiff_amd import Guide
    z = load_golden(NEUTRAL_TRACE[kind])
    tokens, region, chain, loc, q = z["tokens"], z["region"], chain_or_none(z), z["loc"], z["q"]
    B, L = tokens.shape
    order, T = np.repeat(loc[None], B, 0), np.full(B, len(loc))
    neutral = Guide(np.full((B, L), ALL, np.uint32), np.zeros((B, L, 22), np.float32), 1.0)
    m = _mk(hip, kind, dict(load_cfg(kind), dropout=0.2 if kind == "ab" else 0.5), load_weights(kind))
    try:
        kw = dict(q_noise=q, return_logp=True, dropout="faithful", seed=424242, row0=3)
        tok0, lp0 = m.sample(tokens, region, chain, order, T, **kw)
        tok1, lp1 = m.sample(tokens, region, chain, order, T, guide=neutral, **kw)
        assert np.array_equal(tok1, tok0) and np.array_equal(lp1, lp0)
        _, lp_off = m.sample(tokens, region, chain, order, T, **dict(kw, dropout="off"))
        assert not np.array_equal(lp_off, lp0)               # the masks really entered both
    finally:
        m.close()


# ---- 2. against an oracle loop --------------------------------------------------------------------------------------------------
SEED, ROW0 = 987654321, 50
_oracle_cache = {}


def _oracle_logits(micro, state, region, chain):
    """float64 [B, L, 22] of the CPU oracle at `state`; shared between the runs that reach the same state (step 0 of every run, and
    every step of the one-lane and two-lane runs of a temperature as long as they draw the same tokens)."""
    key = (micro["kind"], state.tobytes())
    if key not in _oracle_cache:
        _oracle_cache[key] = micro["o0"](state, region, chain)[:, :, :22].astype(np.float64)
    return _oracle_cache[key]


def _oracle_batch(kind):
    B, tcap = 40, 6
    batch, order, T = _ragged(kind, B, 33, tcap)
    T = T.copy()
    T[5] = 0
    T[17] = 3
    allow, bias = _random_guide(B, batch["tokens"].shape[1])
    return batch, order, T, allow, bias


@pytest.mark.parametrize("lanes", [1, 2])
@pytest.mark.parametrize("temperature", [1.0, 0.5, 2.0, 0.0])
def test_guided_draw_against_an_oracle_loop(micro, temperature, lanes):
    from hudiff_amd import Guide
    kind = micro["kind"]
    batch, order, T, allow, bias = _oracle_batch(kind)
    B, tcap = order.shape
    tok, lp = micro["m0"].sample(batch["tokens"], batch["region"], batch["chain"], order, T, seed=SEED, row0=ROW0, dropout="off",
                                 lanes=lanes, return_logp=True, guide=Guide(allow, bias, temperature))
    live = _live(T, tcap)
    vis = _visited(order, T, tok.shape[1])
    assert _bits(allow[vis], tok[vis]).all(), "a drawn token is not allowed at its slot"
    assert np.array_equal(tok[~vis], batch["tokens"][~vis]) and np.array_equal(tok[5], batch["tokens"][5])
    assert (lp[~live] == 0).all()
    scale = min(temperature, 1.0) if temperature > 0 else 1.0
    state = batch["tokens"].copy()
    cases = left_out = 0
    worst_lp, smallest_gap = 0.0, np.inf
    for t in range(tcap):
        z = _oracle_logits(micro, state, batch["region"], batch["chain"])
        q = ho.philox_exp_noise(SEED, ROW0 + np.arange(B), t).astype(np.float64)
        for b in range(B):
            if t >= T[b]:
                continue
            s = order[b, t]
            ok = _bits(allow[b, s], np.arange(22))
            g1 = np.where(ok, z[b, s] + bias[b, s].astype(np.float64), -np.inf)          # temperature 1
            g = g1 if temperature == 0 else g1 / temperature
            lsm = g - g.max()
            lsm = lsm - np.log(np.exp(lsm).sum())
            score = g if temperature == 0 else np.where(ok, g - np.log(q[b]), -np.inf)
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
            state[b, s] = got
    print(f"{kind} temperature {temperature} lanes {lanes}: {cases} draws, {left_out} left out, smallest oracle gap {smallest_gap:.2e}, "
          f"|logp - oracle| {worst_lp:.2e} (bound {REF_TOL / scale:.1e})")
    assert cases == int(T.sum())
    assert left_out <= 2, "more than 1 % of the draws are too close for the oracle to call"
    assert worst_lp < REF_TOL / scale


# ---- 3. singletons ----------------------------------------------------------------------------------------------------------------
def test_singleton_sets_are_certain(micro):
    from hudiff_amd import Guide
    batch, order, T, _, bias = _oracle_batch(micro["kind"])
    B, L = batch["tokens"].shape
    want = np.random.default_rng(8).integers(0, 22, (B, L))
    allow = (1 << want).astype(np.uint32)
    vis, live = _visited(order, T, L), _live(T, order.shape[1])
    for temperature in (1.0, 0.5, 0.0):
        tok, lp = micro["m0"].sample(batch["tokens"], batch["region"], batch["chain"], order, T, seed=SEED, row0=ROW0, dropout="off",
                                     return_logp=True, guide=Guide(allow, bias, temperature))
        assert np.array_equal(tok[vis], want[vis]) and np.array_equal(tok[~vis], batch["tokens"][~vis])
        assert (lp == 0.0).all() and live.sum() == T.sum()


# ---- 4. sample, then score under the same guide -----------------------------------------------------------------------------------
def test_sample_then_score_under_the_same_guide(micro):
    from hudiff_amd import Guide
    from hudiff_amd._lib import HD_ERR_INVALID, HudiffError
    m = micro["m0"]
    batch, order, T, allow, bias = _oracle_batch(micro["kind"])
    args = (batch["region"], batch["chain"], order, T)
    live = _live(T, order.shape[1])
    for temperature in (1.0, 0.5, 2.0):
        g = Guide(allow, bias, temperature)
        tok, lp = m.sample(batch["tokens"], *args, seed=SEED, row0=ROW0, dropout="off", return_logp=True, guide=g)
        tol = PAIR_TOL / min(temperature, 1.0)
        seq = m.score(tok, *args, parallel=False, guide=g)
        par = m.score(tok, *args, parallel=True, device_batch=100, guide=g)
        e_seq, e_par = float(np.abs(seq - lp).max()), float(np.abs(par - lp).max())
        print(f"{micro['kind']} temperature {temperature}: |seq - record| {e_seq:.2e}  |par - record| {e_par:.2e}  (bound {tol:.1e})")
        assert e_seq < tol and e_par < tol
        assert (seq[~live] == 0).all() and (par[~live] == 0).all() and (seq[live] <= 0).all()
        # the guide really entered: the unguided score of the same tokens is another number
        assert np.abs(m.score(tok, *args, parallel=False) - seq).max() > 1e-2
    # a target outside its allowed set
    b, s = 21, order[21, 2]
    bad = tok.copy()
    assert allow[b, s] != ALL
    bad[b, s] = next(j for j in range(22) if not (int(allow[b, s]) >> j) & 1)
    for parallel in (False, True):
        with pytest.raises(HudiffError) as e:
            m.score(bad, *args, parallel=parallel, guide=Guide(allow, bias, 1.0))
        assert e.value.status == HD_ERR_INVALID
    for parallel in (False, True):
        with pytest.raises(HudiffError) as e:
            m.score(tok, *args, parallel=parallel, guide=Guide(allow, bias, 0.0))
        assert e.value.status == HD_ERR_INVALID
    # the failed calls consumed their guides: the handle is unguided again
    plain = m.score(tok, *args, parallel=False)
    assert np.abs(plain - seq).max() > 1e-2


# ---- 5. lifetime -------------------------------------------------------------------------------------------------------------------
def test_guide_lifetime(micro):
    from hudiff_amd import Guide
    from hudiff_amd._lib import HD_ERR_INVALID, HD_ERR_STATE, HudiffError
    m = micro["m0"]
    batch, order, T, allow, bias = _oracle_batch(micro["kind"])
    B, L = batch["tokens"].shape
    tcap = order.shape[1]
    args = (batch["tokens"], batch["region"], batch["chain"], order, T)
    kw = dict(seed=SEED, row0=ROW0, dropout="off")
    g = Guide(allow, bias, 0.5)
    plain = m.sample(*args, **kw)
    guided = m.sample(*args, guide=g, **kw)
    assert not np.array_equal(guided, plain)
    # one shot: the session after a guided one is unguided
    assert np.array_equal(m.sample(*args, **kw), plain)
    # a restart inside a guided session keeps the guide
    m.sample_begin(*args, guide=g, **kw)
    m.sample_run(0, tcap)
    assert np.array_equal(m.sample_tokens(), guided)
    m.sample_restart(kw["seed"] + 1)
    m.sample_run(0, tcap)
    other = m.sample_tokens()
    vis = _visited(order, T, L)
    assert _bits(allow[vis], other[vis]).all() and not np.array_equal(other, guided)
    # ... and a guide cannot be set while the session is open
    with pytest.raises(HudiffError) as e:
        m.set_guide(g, B)
    assert e.value.status == HD_ERR_STATE
    m.sample_restart(kw["seed"])
    m.sample_run(0, tcap)
    assert np.array_equal(m.sample_end(), guided)
    assert np.array_equal(m.sample(*args, **kw), plain)
    # the wrong B: the begin fails and has consumed the guide
    m.set_guide(Guide(allow[:B - 1], bias[:B - 1], 0.5))
    with pytest.raises(HudiffError) as e:
        m.sample(*args, **kw)
    assert e.value.status == HD_ERR_INVALID
    assert np.array_equal(m.sample(*args, **kw), plain)
    # hd_forward neither uses nor clears a guide; NULL clears one
    m.set_guide(g, B)
    ch = None if batch["chain"] is None else np.concatenate([batch["chain"][:2], batch["chain"][B:B + 2]])
    m(batch["tokens"][:2], batch["region"][:2], ch)
    assert np.array_equal(m.sample(*args, **kw), guided)
    m.set_guide(g, B)
    m.set_guide(None)
    assert np.array_equal(m.sample(*args, **kw), plain)
    # an empty allowed set: an error at a visited slot, nothing at a slot nobody visits (bits above 21 do not count)
    b = 21
    empty = allow.copy()
    empty[b, order[b, T[b] - 1]] = 1 << 25
    with pytest.raises(HudiffError) as e:
        m.sample(*args, guide=Guide(empty, bias, 0.5), **kw)
    assert e.value.status == HD_ERR_INVALID
    unvisited = int(np.flatnonzero(~vis[b])[0])
    empty = allow.copy()
    empty[b, unvisited] = 0
    empty[17, order[17, 4]] = 0                               # (row 17 stops after three steps)
    assert np.array_equal(m.sample(*args, guide=Guide(empty, bias, 0.5), **kw), guided)
    # what hd_set_guide itself refuses
    for bad in (Guide(allow, bias, -1.0), Guide(allow, bias, 0.001), Guide(allow, bias, 1000.0), Guide(allow, bias, float("nan")),
                Guide(allow, np.where(np.arange(22) == 3, np.inf, bias).astype(np.float32), 1.0)):
        with pytest.raises(HudiffError) as e:
            m.set_guide(bad, B)
        assert e.value.status == HD_ERR_INVALID
    assert np.array_equal(m.sample(*args, **kw), plain)


# ---- 6. a guard repeats a guided call ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["ab", "nb"])
def test_range_guard_repeats_a_guided_call(hip, kind):
    from hudiff_amd import Guide
    from test_adversarial_golden import load_adv
    z, cfg, sd = load_adv(kind, "huge")
    chain = z["chain"] if z["chain"].size else None
    B, Tn = z["order"].shape
    T = np.full(B, Tn)
    allow, bias = _random_guide(B, z["tokens"].shape[1], seed=6)
    g = Guide(allow, bias, 1.0)
    mx, m32 = _mk(hip, kind, cfg, sd, precision="split"), _mk(hip, kind, cfg, sd, precision="f32_all")
    try:
        with pytest.warns(RuntimeWarning, match="left the fp16 range"):
            tok, lp = mx.sample(z["tokens"], z["region"], chain, z["order"], T, q_noise=z["q"], return_logp=True, guide=g)
        info = prec(mx, split_in_use=False, last_call_repeated=True)
        assert info["range_fallbacks"] >= 1
        vis = _visited(z["order"], T, tok.shape[1])
        assert _bits(allow[vis], tok[vis]).all() and np.array_equal(tok[~vis], z["tokens"][~vis])
        want = m32.score(tok, z["region"], chain, z["order"], T, parallel=False, guide=g)
        err = float(np.abs(want - lp).max())
        print(f"{kind}: guided record of the repeated call against the f32_all guided score: {err:.2e}")
        assert np.isfinite(lp).all() and err < PAIR_TOL
    finally:
        mx.close(); m32.close()


# ---- 7. production width ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["ab", "nb"])
def test_production_width_forbid_cm(hip, kind):
    from hudiff_amd import Guide
    from hudiff_amd.guide import letters_mask
    z, cfg, sd = _load_prod(kind)
    chain = z["chain"] if z["chain"].size else None
    B, L = z["tokens"].shape
    g = Guide(np.full(L, ALL & ~letters_mask("CM"), np.uint32), None, 0.7)
    ms, m32 = _mk(hip, kind, cfg, sd, precision="split"), _mk(hip, kind, cfg, sd, precision="f32_all")
    try:
        tok, lp = ms.sample(z["tokens"], z["region"], chain, z["order"], z["T"], q_noise=z["q"], return_logp=True, guide=g)
        vis = _visited(z["order"], z["T"], L)
        c, mm = 1, 10                                         # 'ACDEFGHIKLMNPQRSTVWY'
        assert not np.isin(tok[vis], (c, mm)).any() and np.isin(z["final"][vis], (c, mm)).any()
        assert np.array_equal(tok[~vis], z["tokens"][~vis])
        want = m32.score(tok, z["region"], chain, z["order"], z["T"], parallel=False, guide=g)
        err = float(np.abs(want - lp).max())
        print(f"{kind}: production width, split guided record against the f32_all guided score: {err:.2e} (bound {PAIR_TOL / 0.7:.1e})")
        assert err < PAIR_TOL / 0.7
        assert (lp[~_live(z["T"], z["order"].shape[1])] == 0).all()
    finally:
        ms.close(); m32.close()


# ---- 8. CLIs -------------------------------------------------------------------------------------------------------------------------
def _cli_case(kind):
    if kind == "ab":
        from hudiff_amd.cli import sample as cli
        return cli, _ab_checkpoint, "hudiffab.pt", ["--batch_size", "3", "--seed", "5"], ["H,48,VIL\n", "L,*,!W   # no Trp in VL\n"], "untokenize_antibody"
    from hudiff_amd.cli import nanosample as cli
    return (cli, _nb_checkpoint, "hudiffnb.pt", ["--model", "finetune_vh", "--batch_size", "2", "--try_number", "3", "--seed", "4"],
            ["H,48,VIL\n", "H,*,!W\n"], "untokenize_nanobody")


def _cli_jobs(kind, ckpt, nb_path):
    """The jobs as the CLI prepares them (hudiff_amd.inputs on the numbered rows): (masked tokens, sampled slots) per input."""
    from hudiff_amd import inputs as I
    from hudiff_amd.checkpoint import antibody_model_from_checkpoint, load_checkpoint
    from hudiff_amd.cli.common import load_numbered
    jobs = []
    if kind == "ab":
        config, _, finetune = antibody_model_from_checkpoint(load_checkpoint(str(ckpt)), "finetune")
        pad_region = 7 if config["model"]["n_region"] > 7 else 0
    for row in load_numbered(str(nb_path)):
        if kind == "ab":
            tok, _, _, loc = I.antibody_row(row["h"], row["l"], row.get("l_chain", "K"), finetune=finetune, pad_region=pad_region)
        else:
            tok, _, loc = I.nanobody_row(row["h"], inpaint_sample=False)
        jobs.append((np.asarray(tok), np.asarray(loc)))
    return jobs


@pytest.mark.parametrize("kind", ["ab", "nb"])
def test_cli_constraints(tmp_path, monkeypatch, kind):
    from hudiff_amd import inputs as I
    from hudiff_amd import parse_constraints, tables as T
    from hudiff_amd.guide import letters_mask
    from test_gpu_cli import _write_inputs
    cli, mk_ckpt, ck_name, base, lines, untok = _cli_case(kind)
    csv, nb = _write_inputs(tmp_path, kind, 3)
    cons = tmp_path / "constraints.txt"
    cons.write_text("".join(lines))
    ckpt = tmp_path / "guided" / "checkpoints" / ck_name
    mk_ckpt(ckpt)
    # the written sequences drop their gaps: keep the token rows they were made from
    rows, real = [], getattr(I, untok)

    def recording(row):
        s = real(row)
        rows.append((np.array(row), s))
        return s
    monkeypatch.setattr(I, untok, recording)
    out = cli.main(["--ckpt", str(ckpt), "--data_fpath", str(csv), "--numbered_fpath", str(nb)] + base +
                   ["--forbid", "CM", "--constraints_fpath", str(cons)])
    monkeypatch.setattr(I, untok, real)
    allow = parse_constraints(lines, kind) & np.uint32(ALL & ~letters_mask("CM"))
    jobs = _cli_jobs(kind, ckpt, nb)
    p48 = T.HEAVY_POSITIONS_dict["48"]
    assert any(p48 in loc for _, loc in jobs), "the position-specific constraint must meet a sampled slot"
    written = [l.rstrip("\n").split(",") for l in open(out) if l.startswith("humanization,")]
    assert len(written) >= 3
    for fields in written:
        seqs = tuple(fields[2:4]) if kind == "ab" else fields[2]
        mine = [r for r, s in rows if s == seqs]
        assert mine, "a written sequence was not made from a sampled row"
        j = int(fields[1][1:-len("human_sample")]) if kind == "ab" else int(fields[1][:-len("human_sample")])
        tok0, loc = jobs[j]
        fixed = np.ones(len(tok0), bool)
        fixed[loc] = False
        assert any(_bits(allow[loc], r[loc]).all() and np.array_equal(r[fixed], tok0[fixed]) for r in mine), fields[1]
    # every row the run decoded, written or not, obeys the guide at the slots it sampled
    for r, _ in rows:
        ok = False
        for tok0, loc in jobs:
            fixed = np.ones(len(tok0), bool)
            fixed[loc] = False
            ok = ok or (np.array_equal(r[fixed], tok0[fixed]) and _bits(allow[loc], r[loc]).all())
        assert ok
    # --temperature 1 alone is today's run, byte for byte
    outs = []
    for i, extra in enumerate(([], ["--temperature", "1"])):
        ck = tmp_path / f"plain{i}" / "checkpoints" / ck_name
        mk_ckpt(ck)
        outs.append(cli.main(["--ckpt", str(ck), "--data_fpath", str(csv), "--numbered_fpath", str(nb)] + base + extra))
    assert open(outs[0], "rb").read() == open(outs[1], "rb").read()
    fa = [open(os.path.join(os.path.dirname(o), "sample_identity.fa"), "rb").read() for o in outs]
    assert fa[0] == fa[1]
    assert open(outs[0], "rb").read() != open(out, "rb").read()
