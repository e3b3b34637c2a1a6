"""Per-token log-probabilities and likelihood scoring on the GPU (HD_RECORD_LOGP, hd_score, model.score, the CLIs).

Tolerances.  The project bounds every logit by 1e-4 against the reference; log_softmax_j = z_j - logsumexp(z) moves by at most
|dz_j| + max|dz|, so a device log-probability is within 2e-4 of float64 log_softmax of the reference's recorded fp32 logits (or of
the CPU oracle's), two device results that each hold that bound are within 4e-4 of each other, and a row total within T * 4e-4."""
import os

import numpy as np
import pytest

import hudiff_oracle as ho
from conftest import chain_or_none, load_cfg, load_deep, load_golden, load_weights, prec, unpack_masks

pytestmark = pytest.mark.gpu

REF_TOL = 2e-4          # device against the reference's recording / the oracle
PAIR_TOL = 4e-4         # device against device
MICRO = {"ab": ("finetune", "pretrain", "graft"), "nb": ("plain", "inpaint")}


@pytest.fixture(scope="module")
def hip():
    import hudiff_amd
    if hudiff_amd.device_count() < 1:
        pytest.fail("no MI355X visible: GPU tests must run on the GPU box (there is no CPU fallback)")
    return hudiff_amd


def _mk(hip, kind, cfg, sd, **kw):
    cls = hip.AntiTFNet if kind == "ab" else hip.NanoAntiTFNet
    m = cls(**cfg, **kw)
    m.load_state_dict(sd)
    return m


def log_softmax64(z):
    z = np.asarray(z, np.float64)
    z = z - z.max(axis=-1, keepdims=True)
    return z - np.log(np.exp(z).sum(axis=-1, keepdims=True))


def recorded_logp(step_logits, step_sampled):
    """float64 log_softmax of the reference's recorded fp32 logits at its recorded draw, [T, B] -> [B, T]."""
    return np.take_along_axis(log_softmax64(step_logits), np.asarray(step_sampled)[..., None], axis=-1)[..., 0].T


def traces(kind):
    """(name, weights group, masked tokens, region, chain, loc, q, final, recorded logp) of every fixture with step_logits."""
    out = []
    for mode in MICRO[kind]:
        z = load_golden(f"micro_{kind}_sample_{mode}.npz")
        out.append((f"micro_{mode}", "micro", z["tokens"], z["region"], chain_or_none(z), z["loc"], z["q"], z["final"],
                    recorded_logp(z["step_logits"], z["step_sampled"])))
    z = load_deep(kind)[0]
    out.append(("deep", "deep", z["s_tokens"], z["s_region"], z["s_chain"] if z["s_chain"].size else None, z["s_loc"], z["q"],
                z["final"], recorded_logp(z["step_logits"], z["step_sampled"])))
    return out


def weights(kind, group):
    if group == "micro":
        return load_cfg(kind), load_weights(kind)
    _, cfg, sd = load_deep(kind)
    return cfg, sd


# (id, constructor keywords, sample / score keywords)
VARIANTS = [
    ("graph", {}, {}),
    ("eager", {}, {"graph": False}),
    ("loop", {}, {"graph": "loop"}),
    ("noprune", {}, {"prune": False}),
    ("tail0", {"options": {"tail_form": 0}}, {}),
    ("tail2", {"options": {"tail_form": 2}}, {}),
    ("lanes1", {}, {"lanes": 1}),
    ("lanes2", {"options": {"lane_min_rows": 2}}, {"lanes": 2}),          # (the fixtures have 2-3 rows: make them split)
    ("f32_all", {"precision": "f32_all"}, {}),
    ("f32_gemm", {"precision": "f32_gemm"}, {}),
    ("split", {"precision": "split"}, {}),
]


@pytest.mark.parametrize("kind", ["ab", "nb"])
@pytest.mark.parametrize("variant", VARIANTS, ids=[v[0] for v in VARIANTS])
def test_recorded_traces_sample_logp_and_score(hip, kind, variant):
    """Against the reference's recordings: sample(q_noise, return_logp=True) draws the reference's tokens and records the
    log-probabilities the reference's logits give them; the bare sample() draws the same tokens; score(final, order=loc),
    sequential and step-parallel, finds the same values; the re-filled tokens of a score session are its input."""
    _, mkw, skw = variant
    models = {}
    try:
        for name, group, tokens, region, chain, loc, q, final, want in traces(kind):
            if group not in models:
                models[group] = _mk(hip, kind, *weights(kind, group), **mkw)
            m = models[group]
            B, Tn = tokens.shape[0], len(loc)
            order, T = np.repeat(loc[None], B, 0), np.full(B, Tn)
            out, logp = m.sample(tokens, region, chain, order, T, q_noise=q, return_logp=True, **skw)
            assert np.array_equal(out, final), (name, "tokens with HD_RECORD_LOGP")
            assert logp.shape == (B, Tn) and logp.dtype == np.float32
            e_rec = float(np.abs(logp - want).max())
            assert np.array_equal(m.sample(tokens, region, chain, order, T, q_noise=q, **skw), final), (name, "bare sample()")
            seq = m.score(final, region, chain, order, T, parallel=False, **skw)
            par = m.score(final, region, chain, order, T, parallel=True, device_batch=64, **skw)
            e_seq, e_par, e_pair = (float(np.abs(seq - want).max()), float(np.abs(par - want).max()), float(np.abs(seq - par).max()))
            print(f"{kind} {variant[0]} {name}: |record - ref| {e_rec:.2e}  |seq - ref| {e_seq:.2e}  |par - ref| {e_par:.2e}  |seq - par| {e_pair:.2e}")
            assert e_rec < REF_TOL and e_seq < REF_TOL and e_par < REF_TOL and e_pair < PAIR_TOL, name
            assert (logp < 0).all() and (seq < 0).all()
            m.score_begin(final, region, chain, order, T, **skw)
            m.sample_run(0, Tn)
            assert np.array_equal(m.sample_tokens(), final)
            assert np.array_equal(m.sample_logp(), seq)
            assert np.array_equal(m.sample_end(), final), (name, "hd_sample_end of a score session returns its input")
            assert np.array_equal(m.sample_logp(), seq)                   # still legal after the end
    finally:
        for m in models.values():
            m.close()


@pytest.fixture(scope="module", params=["ab", "nb"])
def micro(request, hip):
    kind = request.param
    cfg, sd = load_cfg(kind), load_weights(kind)
    p = 0.2 if kind == "ab" else 0.5
    models = {"kind": kind, "m0": _mk(hip, kind, cfg, sd), "m1": _mk(hip, kind, dict(cfg, dropout=p), sd),
              "o0": ho.OracleNet(kind, cfg, sd), "o1": ho.OracleNet(kind, dict(cfg, dropout=p), sd)}
    yield models
    models["m0"].close(); models["m1"].close()


def _ragged(kind, B, seed, tcap):
    from hudiff_amd import synthetic as S
    batch = S.synthetic_batch(kind, B, seed=seed)
    T = np.minimum(batch["T"], tcap)
    order = np.ascontiguousarray(batch["order"][:, :tcap])
    return batch, order, T


def test_ragged_batch_sample_then_score(micro):
    """T[b] = 0 and short rows, two lanes: the log-probabilities a sampling session records are those a scoring session finds for
    the sampled tokens along the same order; entries at t >= T[b] are exactly 0; the lane split does not reorder rows."""
    B, tcap = 40, 9
    batch, order, T = _ragged(micro["kind"], B, 33, tcap)
    T[5] = 0; T[17] = 3; T[39] = 1
    m = micro["m0"]
    args = (batch["region"], batch["chain"], order, T)
    kw = dict(seed=987654321, row0=50, dropout="off")
    tok2, lp2 = m.sample(batch["tokens"], *args, return_logp=True, lanes=2, **kw)
    tok1, lp1 = m.sample(batch["tokens"], *args, return_logp=True, lanes=1, **kw)
    assert np.array_equal(tok2, m.sample(batch["tokens"], *args, lanes=2, **kw))
    assert np.array_equal(tok1, tok2)
    # (the lane count picks GEMM tiles, so the two results are two device results, not one)
    assert np.abs(lp1 - lp2).max() < PAIR_TOL
    dead = np.arange(tcap)[None, :] >= T[:, None]
    assert (lp2[dead] == 0).all() and (lp1[dead] == 0).all() and (lp2[~dead] < 0).all()
    assert np.array_equal(tok2[5], batch["tokens"][5])
    for lanes in (1, 2):
        seq = m.score(tok2, *args, parallel=False, lanes=lanes)
        assert (seq[dead] == 0).all()
        assert np.abs(seq - lp2).max() < PAIR_TOL, lanes
    par = m.score(tok2, *args, parallel=True, device_batch=100)
    assert (par[dead] == 0).all() and np.abs(par - lp2).max() < PAIR_TOL
    # rows of the second lane against the oracle
    rows = [21, 39]
    chain = None if batch["chain"] is None else np.concatenate([batch["chain"][rows], batch["chain"][B:][rows]])
    state = batch["tokens"][rows].copy()
    for t in range(int(T[rows].max())):
        lsm = log_softmax64(micro["o0"](state, batch["region"][rows], chain)[:, :, :22])
        for i, b in enumerate(rows):
            if t < T[b]:
                s = order[b, t]
                assert abs(lsm[i, s, tok2[b, s]] - lp2[b, t]) < REF_TOL, (b, t)
                state[i, s] = tok2[b, s]


def test_session_interface_records_as_it_goes(micro):
    """begin / run in pieces / restart / end: steps not run yet read 0, a restart clears the record, the pieces give the one-shot values."""
    B, tcap = 20, 6
    batch, order, T = _ragged(micro["kind"], B, 12, tcap)
    T[2] = 0
    m = micro["m1"]
    args = (batch["tokens"], batch["region"], batch["chain"], order, T)
    kw = dict(seed=31337, row0=9, dropout="faithful")
    want_tok, want_lp = m.sample(*args, return_logp=True, **kw)
    m.sample_begin(*args, record_logp=True, **dict(kw, seed=1))
    m.sample_run(0, 3)
    part = m.sample_logp()
    assert (part[:, 3:] == 0).all() and (part[:, :3][np.arange(3)[None, :] < T[:, None]] < 0).all()
    m.sample_restart(kw["seed"])
    m.sync()
    assert (m.sample_logp() == 0).all()
    m.sample_run(0, 2); m.sample_run(2, tcap)
    assert np.array_equal(m.sample_tokens(), want_tok)
    assert np.array_equal(m.sample_logp(), want_lp)
    assert np.array_equal(m.sample_end(), want_tok)
    assert np.array_equal(m.sample_logp(), want_lp)
    # hd_forward ends the window in which the record can be read
    from hudiff_amd._lib import HD_ERR_STATE, HudiffError
    m(batch["tokens"][:2], batch["region"][:2], None if batch["chain"] is None else np.concatenate([batch["chain"][:2], batch["chain"][B:B + 2]]))
    with pytest.raises(HudiffError) as e:
        m.sample_logp(B, tcap)
    assert e.value.status == HD_ERR_STATE


def test_dropout_injected_masks(micro):
    z = load_golden(f"micro_{micro['kind']}_sample_dropout.npz")
    B, loc = z["tokens"].shape[0], z["loc"]
    order, T = np.repeat(loc[None], B, 0), np.full(B, len(loc))
    masks = dict(dropout="inject", enc_masks=unpack_masks(z, "enc_masks"), conv_masks=unpack_masks(z, "conv_masks"))
    m = micro["m1"]
    out, lp = m.sample(z["tokens"], z["region"], chain_or_none(z), order, T, q_noise=z["q"], return_logp=True, **masks)
    assert np.array_equal(out, z["final"])
    seq = m.score(z["final"], z["region"], chain_or_none(z), order, T, parallel=False, **masks)
    assert np.abs(seq - lp).max() < PAIR_TOL
    off = m.score(z["final"], z["region"], chain_or_none(z), order, T, dropout="off")
    assert np.abs(off - lp).max() > 1e-2                 # the masks really entered the recorded values
    with pytest.raises(ValueError):
        m.score(z["final"], z["region"], chain_or_none(z), order, T, parallel=True, **masks)
    with pytest.raises(ValueError):
        m.score(z["final"], z["region"], chain_or_none(z), order, T, parallel=True, dropout="faithful")


def test_dropout_generated_masks_against_an_oracle_loop(micro):
    B, tcap = 3, 6
    batch, order, T = _ragged(micro["kind"], B, 7, tcap)
    T[1] = 4
    full = np.where(batch["tokens"] == 22, batch["truth"], batch["tokens"]).astype(np.int32)
    seed, row0 = 0xFEEDFACE1234, 40
    got = micro["m1"].score(full, batch["region"], batch["chain"], order, T, dropout="faithful", seed=seed, row0=row0)
    state = full.copy()
    for b in range(B):
        state[b, order[b, :T[b]]] = 22
    want = np.zeros((B, tcap))
    for t in range(tcap):
        drop = ho.Dropout("philox", seed=seed, rows=np.arange(B) + row0, step=t)
        lsm = log_softmax64(micro["o1"](state, batch["region"], batch["chain"], dropout=drop)[:, :, :22])
        for b in range(B):
            if t < T[b]:
                s = order[b, t]
                want[b, t] = lsm[b, s, full[b, s]]
                state[b, s] = full[b, s]
    err = np.abs(got - want).max()
    print(f"{micro['kind']}: generated dropout, |score - oracle loop| = {err:.2e}")
    assert err < REF_TOL
    off = micro["m1"].score(full, batch["region"], batch["chain"], order, T, dropout="off")
    assert np.abs(off - got).max() > 1e-2


def test_error_paths(micro):
    from hudiff_amd._lib import HD_ERR_INVALID, HD_ERR_STATE, HudiffError
    B, tcap = 4, 5
    batch, order, T = _ragged(micro["kind"], B, 3, tcap)
    m = micro["m0"]
    full = np.where(batch["tokens"] == 22, batch["truth"], batch["tokens"]).astype(np.int32)
    bad = full.copy()
    bad[2, order[2, 1]] = 22                              # a mask where a residue is to be scored
    for parallel in (False, True):
        with pytest.raises(HudiffError) as e:
            m.score(bad, batch["region"], batch["chain"], order, T, parallel=parallel)
        assert e.value.status == HD_ERR_INVALID
    ok = bad.copy()                                       # ... but a mask at a slot nobody scores is context
    T2 = T.copy(); T2[2] = 1
    assert np.isfinite(m.score(ok, batch["region"], batch["chain"], order, T2)).all()
    # an empty batch is legal on both paths
    L = m.max_len
    for parallel in (False, True):
        e = m.score(np.zeros((0, L), np.int32), np.zeros((0, L), np.int32), np.zeros(0, np.int32) if micro["kind"] == "ab" else None,
                    np.zeros((0, 3), np.int32), np.zeros(0, np.int32), parallel=parallel)
        assert e.shape == (0, 3)
    # a session that does not record has nothing to read
    m.sample_begin(batch["tokens"], batch["region"], batch["chain"], order, T, dropout="off")
    m.sample_run(0, 2)
    with pytest.raises(HudiffError) as e:
        m.sample_logp()
    assert e.value.status == HD_ERR_STATE
    m.sample_end()
    with pytest.raises(HudiffError) as e:
        m.sample_logp()
    assert e.value.status == HD_ERR_STATE


def test_session_reuse_score_sample_score(micro):
    """One handle, alternating modes with the same shapes: a stale step graph of the other mode would show."""
    B, tcap = 24, 5
    batch, order, T = _ragged(micro["kind"], B, 19, tcap)
    m = micro["m0"]
    full = np.where(batch["tokens"] == 22, batch["truth"], batch["tokens"]).astype(np.int32)
    args = (batch["region"], batch["chain"], order, T)
    kw = dict(seed=5, row0=0, dropout="off")
    s1 = m.score(full, *args, parallel=False)
    t1 = m.sample(batch["tokens"], *args, **kw)
    t1r, l1r = m.sample(batch["tokens"], *args, return_logp=True, **kw)
    s2 = m.score(full, *args, parallel=False)
    t2 = m.sample(batch["tokens"], *args, **kw)
    s3 = m.score(full, *args, parallel=False)
    assert np.array_equal(s1, s2) and np.array_equal(s1, s3)
    assert np.array_equal(t1, t2) and np.array_equal(t1, t1r)
    assert not np.array_equal(t1, full)
    assert np.abs(m.score(t1, *args, parallel=False) - l1r).max() < PAIR_TOL


# ---- production width -----------------------------------------------------------------------------------------------------------
def _load_prod(kind):
    from test_prod_trace import _load
    return _load(kind, "")


@pytest.mark.parametrize("kind", ["ab", "nb"])
def test_production_width_three_routes_and_the_oracle(hip, kind):
    from hudiff_amd import scoring
    z, cfg, sd = _load_prod(kind)
    chain = z["chain"] if z["chain"].size else None
    args = (z["final"], z["region"], chain, z["order"], z["T"])
    res = {}
    for route in ("f32_all", "f32_gemm", "split"):
        m = _mk(hip, kind, cfg, sd, precision=route)
        try:
            res[route] = m.score(*args, parallel=False)
            if route == "split":
                res["split_parallel"] = m.score(*args, parallel=True)          # launches of 128-row-tile size: the split GEMMs themselves
                _, res["split_record"] = m.sample(z["tokens"], z["region"], chain, z["order"], z["T"], q_noise=z["q"], return_logp=True)
        finally:
            m.close()
    names = sorted(res)
    for i, a in enumerate(names):
        for b in names[i + 1:]:
            e = float(np.abs(res[a] - res[b]).max())
            print(f"{kind}: |{a} - {b}| = {e:.2e}")
            assert e < PAIR_TOL, (a, b)
    dead = np.arange(z["order"].shape[1])[None, :] >= z["T"][:, None]
    assert all((r[dead] == 0).all() for r in res.values())
    # 8 (row, step) pairs through one oracle forward of their expanded rows
    x = scoring.expand_steps(*args)
    pick = np.linspace(0, x.tokens.shape[0] - 1, 8).astype(int)
    n = len(pick)
    och = None if chain is None else np.concatenate([x.chain[pick], x.chain[x.tokens.shape[0] + pick]])
    lsm = log_softmax64(ho.OracleNet(kind, cfg, sd)(x.tokens[pick], x.region[pick], och)[np.arange(n), x.order[pick, 0], :22])
    want = lsm[np.arange(n), z["final"][x.rows[pick], x.order[pick, 0]]]
    for a in names:
        e = float(np.abs(res[a][x.rows[pick], x.steps[pick]] - want).max())
        print(f"{kind}: |{a} - oracle| over 8 (row, step) pairs = {e:.2e}")
        assert e < REF_TOL, a


@pytest.mark.parametrize("kind", ["ab", "nb"])
def test_range_guard_repeats_a_score_call(hip, kind):
    """Weights whose stream leaves the fp16 range: the split route's score call is repeated on the fp32 kernels inside the
    library, and the values come from the repeat."""
    from test_adversarial_golden import load_adv
    z, cfg, sd = load_adv(kind, "huge")
    chain = z["chain"] if z["chain"].size else None
    B, Tn = z["order"].shape
    args = (z["final"], z["region"], chain, z["order"], np.full(B, Tn))
    mx, m32 = _mk(hip, kind, cfg, sd, precision="split"), _mk(hip, kind, cfg, sd, precision="f32_all")
    try:
        want = m32.score(*args, parallel=False)
        with pytest.warns(RuntimeWarning, match="left the fp16 range"):
            got = mx.score(*args, parallel=False)
        info = prec(mx, split_in_use=False, last_call_repeated=True)
        assert info["range_fallbacks"] >= 1
        assert np.isfinite(got).all() and (got <= 0).all()
        assert np.abs(got - want).max() < PAIR_TOL
        mx.precision_reset()
        with pytest.warns(RuntimeWarning, match="left the fp16 range"):
            par = mx.score(*args, parallel=True)
        assert mx.precision_info()["range_fallbacks"] >= 2
        assert np.isfinite(par).all() and np.abs(par - want).max() < PAIR_TOL
        # a recording sampling session is repeated the same way
        mx.precision_reset()
        with pytest.warns(RuntimeWarning, match="left the fp16 range"):
            tok, lp = mx.sample(z["tokens"], z["region"], chain, z["order"], np.full(B, Tn), q_noise=z["q"], return_logp=True)
        assert np.array_equal(tok, z["final"]) and np.abs(lp - want).max() < PAIR_TOL
    finally:
        mx.close(); m32.close()


# ---- CLIs -----------------------------------------------------------------------------------------------------------------------
def _ab_checkpoint(path):
    import torch
    from hudiff_amd import checkpoint as ck
    cfg = dict(load_cfg("ab"), dropout=0.2)
    sd = {k: torch.from_numpy(v) for k, v in load_weights("ab").items()}
    path.parent.mkdir(parents=True, exist_ok=True)
    torch.save({"fineconfig": ck.EasyDict({}), "pretrain_config": ck.EasyDict({"name": "trans_oadm", "model": cfg}), "model": sd}, path)
    return cfg


def _nb_checkpoint(path):
    import torch
    from hudiff_amd import checkpoint as ck
    cfg = dict(load_cfg("nb"), dropout=0.5)
    sd = {"infilling_pretrain." + k: torch.from_numpy(v) for k, v in load_weights("nb").items()}
    path.parent.mkdir(parents=True, exist_ok=True)
    torch.save({"config": ck.EasyDict({"name": "infilling", "model": {}}), "infilling_params": ck.EasyDict(cfg),
                "abnativ_params": {}, "model": sd}, path)
    return cfg


def test_antibody_sampler_logp_sidecar(tmp_path):
    from hudiff_amd.cli import sample as cli
    from test_gpu_cli import _write_inputs
    csv, nb = _write_inputs(tmp_path, "ab", 4)
    outs = []
    for i, extra in enumerate(([], ["--logp_fpath", str(tmp_path / "logp.csv")])):
        ckpt = tmp_path / f"run{i}" / "checkpoints" / "hudiffab.pt"
        _ab_checkpoint(ckpt)
        outs.append(cli.main(["--ckpt", str(ckpt), "--data_fpath", str(csv), "--numbered_fpath", str(nb), "--batch_size", "3",
                              "--seed", "5"] + extra))
    assert open(outs[0], "rb").read() == open(outs[1], "rb").read()
    fa = [open(os.path.join(os.path.dirname(o), "sample_identity.fa"), "rb").read() for o in outs]
    assert fa[0] == fa[1]
    lines = open(tmp_path / "logp.csv").read().splitlines()
    assert lines[0] == "name,pass,replica,T,logp,chosen" and len(lines) == 1 + 4 * 3          # one row per sampled sequence
    rows = [l.split(",") for l in lines[1:]]
    for j in range(4):
        mine = rows[3 * j:3 * j + 3]
        assert [r[0] for r in mine] == [f"m{j}"] * 3 and [r[1] for r in mine] == ["0"] * 3 and [r[2] for r in mine] == ["0", "1", "2"]
        assert sum(int(r[5]) for r in mine) == 1                                              # similarity search writes one replica
        assert all(int(r[3]) > 50 and float(r[4]) < 0 for r in mine)


def test_nanobody_sampler_logp_sidecar(tmp_path):
    from hudiff_amd.cli import nanosample as cli
    from test_gpu_cli import _write_inputs
    csv, nb = _write_inputs(tmp_path, "nb", 3)
    outs = []
    for i, extra in enumerate(([], ["--logp_fpath", str(tmp_path / "logp.csv")])):
        ckpt = tmp_path / f"run{i}" / "checkpoints" / "hudiffnb.pt"
        _nb_checkpoint(ckpt)
        outs.append(cli.main(["--ckpt", str(ckpt), "--data_fpath", str(csv), "--numbered_fpath", str(nb), "--model", "finetune_vh",
                              "--batch_size", "2", "--try_number", "3", "--seed", "4"] + extra))
    assert open(outs[0], "rb").read() == open(outs[1], "rb").read()
    written = open(outs[1]).read().count("humanization,")
    lines = open(tmp_path / "logp.csv").read().splitlines()
    assert lines[0] == "name,sweep,pass,replica,T,logp,chosen"
    rows = [l.split(",") for l in lines[1:]]
    assert len(rows) % 2 == 0 and len(rows) >= 3 * 2                                          # every replica of every sweep
    assert sum(int(r[6]) for r in rows) == written
    assert all(float(r[5]) < 0 and int(r[4]) > 20 for r in rows)


@pytest.mark.parametrize("kind", ["ab", "nb"])
def test_score_cli_equals_model_score(hip, tmp_path, kind):
    from hudiff_amd import scoring
    from hudiff_amd.cli import score as cli
    from hudiff_amd.cli.common import load_numbered
    from test_gpu_cli import _write_inputs
    csv, nb = _write_inputs(tmp_path, kind, 3)
    if kind == "ab":                                      # (every row of the file is scored: keep the rows the numbering file describes)
        csv.write_text("".join(l for l in open(csv).read().splitlines(True) if not l.startswith("human,")))
    ckpt = tmp_path / "ck" / ("hudiffab.pt" if kind == "ab" else "hudiffnb.pt")
    (_ab_checkpoint if kind == "ab" else _nb_checkpoint)(ckpt)
    mask = "pretrain" if kind == "ab" else "inpaint"
    out = cli.main(["--ckpt", str(ckpt), "--kind", kind, "--data_fpath", str(csv), "--numbered_fpath", str(nb), "--orders", "3",
                    "--seed", "8", "--mask", mask, "--out_fpath", str(tmp_path / "scores.csv")])
    lines = open(out).read().splitlines()
    rows = cli.read_rows(str(csv), kind)
    assert lines[0] == "name,T,logp_mean,logp_std,logp_per_residue" and len(lines) == 1 + len(rows)
    jobs = cli.build_jobs(rows, kind, mask, load_numbered(str(nb)), "auto")
    m = _mk(hip, kind, load_cfg(kind), load_weights(kind))
    try:
        for j, job in enumerate(jobs):
            orders = scoring.draw_orders(job.loc, 3, 8, j)
            B = 3
            ch = None if kind == "nb" else np.array([job.chain[0]] * B + [job.chain[1]] * B, np.int32)
            lp = m.score(np.repeat(job.tokens[None], B, 0), np.repeat(job.region[None], B, 0), ch, orders, np.full(B, len(job.loc)))
            tot = lp.astype(np.float64).sum(axis=1)
            name, T, mean, std, per = lines[1 + j].split(",")
            assert name == job.name and int(T) == len(job.loc) > 20
            bound = len(job.loc) * PAIR_TOL
            assert abs(float(mean) - tot.mean()) < bound and abs(float(std) - tot.std()) < bound
            assert abs(float(per) - tot.mean() / len(job.loc)) < PAIR_TOL
            assert float(std) > 0
    finally:
        m.close()
    # the samplers' own output is an input too
    if kind == "ab":
        res = tmp_path / "sample_humanization_result.csv"
        res.write_text("Specific,name,hseq,lseq,\n" + "".join(f"mouse,{n},{h},{l}\n" for n, h, l in rows[:2]))
        got = cli.read_rows(str(res), kind)
        assert got == rows[:2]
