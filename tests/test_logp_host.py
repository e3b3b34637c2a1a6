"""Likelihood scoring, the parts that need no GPU: the C ABI's new entry points, scoring.expand_steps (also against the
reference's recorded per-step logits through the CPU oracle), the host plumbing of sample_jobs(return_logp=True) / score_jobs with
a fake model, and the sidecar CSV writer.

Tolerance of the oracle check: the project bounds the oracle's logits by 1e-5 against the reference (tests/test_oracle_golden.py);
log_softmax_j = z_j - logsumexp(z) moves by at most |dz_j| + max|dz|, so a log-probability is bounded by 2e-5."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from conftest import ROOT, load_cfg, load_deep, load_golden, load_weights

ORACLE_LOGP_TOL = 2e-5
MICRO = [("ab", "finetune"), ("ab", "pretrain"), ("ab", "graft"), ("nb", "plain"), ("nb", "inpaint")]


def recorded_logp(step_logits, step_sampled):
    """float64 log_softmax of the reference's recorded fp32 logits at the recorded draw: [T, B] -> [B, T]."""
    z = np.asarray(step_logits, np.float64)
    z = z - z.max(axis=-1, keepdims=True)
    lsm = z - np.log(np.exp(z).sum(axis=-1, keepdims=True))
    s = np.asarray(step_sampled)
    return np.take_along_axis(lsm, s[..., None], axis=-1)[..., 0].T


def trace_fixture(kind, mode):
    """-> (masked tokens, region, chain, loc, final, step_logits, step_sampled) of a micro or a deep fixture."""
    if mode == "deep":
        z = load_deep(kind)[0]
        return (z["s_tokens"], z["s_region"], z["s_chain"] if z["s_chain"].size else None, z["s_loc"], z["final"],
                z["step_logits"], z["step_sampled"])
    z = load_golden(f"micro_{kind}_sample_{mode}.npz")
    return (z["tokens"], z["region"], z["chain"] if z["chain"].size else None, z["loc"], z["final"], z["step_logits"],
            z["step_sampled"])


# ---- C ABI --------------------------------------------------------------------------------------------------------------------
def test_header_declares_and_library_exports_the_scoring_entry_points():
    from hudiff_amd import _lib
    text = open(os.path.join(ROOT, "include", "hudiff_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in ("hd_score", "hd_score_begin", "hd_sample_logp"):
        assert re.search(r"\b%s\s*\(" % name, code), f"{name} is not declared"
        assert name in _lib.EXPORTS
    assert re.search(r"\bHD_RECORD_LOGP\s*=\s*64u\b", code) and _lib.HD_RECORD_LOGP == 64
    assert re.search(r"#define HD_ABI_VERSION 1\b", text) and _lib.HD_ABI_VERSION == 1
    lib = _lib.load()
    for name in ("hd_score", "hd_score_begin", "hd_sample_logp"):
        assert hasattr(lib, name), f"{name} is not exported"


def test_scoring_entry_points_validate_without_a_device():
    from hudiff_amd import _lib
    lib = _lib.load()
    L = 152
    tok, reg = np.zeros((1, L), np.int32), np.zeros((1, L), np.int32)
    order, T, logp = np.zeros((1, 1), np.int32), np.ones(1, np.int32), np.zeros((1, 1), np.float32)
    p = lambda a, t=C.c_int32: a.ctypes.data_as(C.POINTER(t))
    assert lib.hd_score_begin(None, p(tok), p(reg), None, p(order), p(T), 1, 1, 0, 0, 0, None, None) == _lib.HD_ERR_INVALID
    assert lib.hd_score(None, p(tok), p(reg), None, p(order), p(T), 1, 1, 0, 0, 0, None, None, p(logp, C.c_float)) == _lib.HD_ERR_INVALID
    # no session (and no handle to have one): a call-order error, as hd_sample_tokens / hd_sample_end report it
    assert lib.hd_sample_logp(None, p(logp, C.c_float)) == _lib.HD_ERR_STATE
    assert lib.hd_sample_logp(None, None) == _lib.HD_ERR_STATE


# ---- expand_steps -------------------------------------------------------------------------------------------------------------
def test_expand_steps_on_a_ragged_batch():
    from hudiff_amd import scoring
    rng = np.random.default_rng(5)
    B, L, Tmax = 5, 30, 6
    tokens = rng.integers(0, 22, size=(B, L)).astype(np.int32)
    region = rng.integers(0, 7, size=(B, L)).astype(np.int32)
    chain = np.array([0] * B + [1, 2, 1, 2, 1], np.int32)
    T = np.array([3, 0, Tmax, 1, 4])
    order = np.stack([rng.permutation(L)[:Tmax] for _ in range(B)]).astype(np.int32)      # per-row orders
    x = scoring.expand_steps(tokens, region, chain, order, T)
    N = int(T.sum())
    assert x.tokens.shape == (N, L) and x.region.shape == (N, L) and x.order.shape == (N, 1) and x.chain.shape == (2 * N,)
    assert (x.T == 1).all() and x.B == B
    i = 0
    for b in range(B):
        for t in range(T[b]):
            assert (x.rows[i], x.steps[i]) == (b, t)
            masked = set(order[b, t:T[b]].tolist())
            for s in range(L):
                assert x.tokens[i, s] == (22 if s in masked else tokens[b, s]), (b, t, s)
            assert x.order[i, 0] == order[b, t]
            assert np.array_equal(x.region[i], region[b])
            assert x.chain[i] == chain[b] and x.chain[N + i] == chain[B + b]
            i += 1
    assert i == N
    # fold-back is exact: value (b, t) lands at [b, t], everything else is 0
    flat = rng.normal(size=N).astype(np.float32)
    folded = x.fold(flat, Tmax)
    assert folded.shape == (B, Tmax) and folded.dtype == np.float32
    i = 0
    for b in range(B):
        for t in range(Tmax):
            if t < T[b]:
                assert folded[b, t] == flat[i]
                i += 1
            else:
                assert folded[b, t] == 0.0
    # nanobody shape (no chain ids), empty batch
    y = scoring.expand_steps(tokens, region, None, order, np.zeros(B, np.int64))
    assert y.chain is None and y.tokens.shape == (0, L) and y.fold(np.zeros(0), Tmax).shape == (B, Tmax)
    # no rows at all: nothing to expand, the fold keeps Tmax
    for ch in (None, np.zeros(0, np.int32)):
        e = scoring.expand_steps(np.zeros((0, L), np.int32), np.zeros((0, L), np.int32), ch, np.zeros((0, Tmax), np.int32),
                                 np.zeros(0, np.int32))
        assert e.tokens.shape == (0, L) and e.order.shape == (0, 1) and e.B == 0 and e.fold(np.zeros(0), Tmax).shape == (0, Tmax)
        assert (e.chain is None) == (ch is None)
    with pytest.raises(ValueError):
        scoring.expand_steps(tokens, region, None, order, np.full(B, Tmax + 1))


@pytest.mark.parametrize("kind,mode", MICRO + [("ab", "deep"), ("nb", "deep")])
def test_expand_steps_rebuilds_the_reference_token_states(kind, mode):
    """Row (b, t) of the expansion of the reference's `final` along `loc` is the token state the reference's loop fed the model at
    step t: the t = 0 rows are the fixture's masked input, the last step's rows have one more slot masked than `final`."""
    from hudiff_amd import scoring
    tokens, region, chain, loc, final, step_logits, step_sampled = trace_fixture(kind, mode)
    B, Tn = final.shape[0], len(loc)
    assert step_logits.shape == (Tn, B, 22)
    x = scoring.expand_steps(final, region, chain, np.repeat(loc[None], B, 0), np.full(B, Tn))
    assert x.tokens.shape[0] == B * Tn
    assert np.array_equal(x.tokens[x.steps == 0], tokens)
    # (the deep fixtures record the first 16 steps of a longer schedule: their `final` keeps the slots never visited masked)
    assert np.array_equal((x.tokens[x.steps == Tn - 1] == 22).sum(axis=1), (final == 22).sum(axis=1) + 1)
    # the targets the library will take are the reference's draws
    assert np.array_equal(final[x.rows, x.order[:, 0]], np.asarray(step_sampled).T.reshape(-1))


@pytest.mark.parametrize("kind,mode", MICRO)
def test_one_oracle_forward_of_the_expanded_rows_gives_the_recorded_logp(kind, mode):
    import hudiff_oracle as ho
    from hudiff_amd import scoring
    tokens, region, chain, loc, final, step_logits, step_sampled = trace_fixture(kind, mode)
    B, Tn = final.shape[0], len(loc)
    x = scoring.expand_steps(final, region, chain, np.repeat(loc[None], B, 0), np.full(B, Tn))
    net = ho.OracleNet(kind, load_cfg(kind), load_weights(kind))
    N = x.tokens.shape[0]
    z = net(x.tokens, x.region, x.chain)[np.arange(N), x.order[:, 0], :22].astype(np.float64)
    z -= z.max(axis=-1, keepdims=True)
    lsm = z - np.log(np.exp(z).sum(axis=-1, keepdims=True))
    got = x.fold(lsm[np.arange(N), final[x.rows, x.order[:, 0]]], Tn)
    want = recorded_logp(step_logits, step_sampled)
    err = np.abs(got - want).max()
    print(f"{kind} {mode}: {N} expanded rows, max |logp - recorded| = {err:.3g}")
    assert err < ORACLE_LOGP_TOL


# ---- host plumbing with a fake model ------------------------------------------------------------------------------------------
class FakeModel:
    """Stands in for hudiff_amd.model._Denoiser: a draw is a function of (global row, step), its log-probability as well."""
    def __init__(self, kind="nb", L=12):
        self.kind, self.max_len = kind, L
        self.sample_calls, self.score_calls = [], []

    @staticmethod
    def value(row, t, seed):
        return -((row * 131 + t * 7 + seed) % 1000) / 64.0 - 0.015625

    def sample(self, tokens, region, chain, order, T, **kw):
        self.sample_calls.append(dict(kw, B=len(tokens)))
        out = np.array(tokens, np.int32, copy=True)
        lp = np.zeros(order.shape, np.float32)
        for b in range(len(out)):
            for t in range(int(T[b])):
                out[b, order[b, t]] = (kw["row0"] + b + t) % 20
                lp[b, t] = self.value(kw["row0"] + b, t, kw["seed"])
        return (out, lp) if kw.get("return_logp") else out

    def score(self, tokens, region, chain, order, T, **kw):
        self.score_calls.append(dict(kw, B=len(tokens), order=np.array(order), chain=chain))
        lp = np.zeros(order.shape, np.float32)
        for b in range(len(tokens)):
            for t in range(int(T[b])):
                lp[b, t] = self.value(kw["row0"] + b, int(order[b, t]), kw["seed"])
        return lp


def _jobs(L=12, complete=False):
    from hudiff_amd.sampler import Job
    jobs = []
    for j, n in enumerate((4, 0, 6)):
        tok = np.full(L, 3 + j, np.int32)
        loc = np.arange(1, 1 + n)
        if not complete:
            tok[loc] = 22
        jobs.append(Job(tokens=tok, region=np.zeros(L, np.int32), loc=loc, name=f"s{j}"))
    return jobs


def test_sample_jobs_return_logp_plumbing():
    from hudiff_amd.sampler import sample_jobs
    jobs, replicas, passes, seed = _jobs(), 3, 2, 11
    fake = FakeModel()
    plain = sample_jobs(fake, jobs, replicas, seed, passes=passes, device_batch=4)
    assert all("return_logp" not in c for c in fake.sample_calls), "without the flag model.sample gets no new keyword"
    assert set(fake.sample_calls[0]) == {"seed", "row0", "dropout", "q_noise", "B"}
    fake2 = FakeModel()
    tokens, logp = sample_jobs(fake2, jobs, replicas, seed, passes=passes, device_batch=4, return_logp=True)
    assert all(c.get("return_logp") is True for c in fake2.sample_calls)
    assert np.array_equal(tokens, plain)
    Tmax = 6
    assert tokens.shape == (3, passes, replicas, 12) and logp.shape == (3, passes, replicas, Tmax) and logp.dtype == np.float32
    for j, job in enumerate(jobs):
        for p in range(passes):
            for r in range(replicas):
                for t in range(Tmax):
                    want = FakeModel.value(j * replicas + r, t, seed + 1000003 * p) if t < len(job.loc) else 0.0
                    assert logp[j, p, r, t] == np.float32(want), (j, p, r, t)
    # keyed by job id, not by position in the batch
    _, sub = sample_jobs(FakeModel(), jobs[2:], replicas, seed, device_batch=4, return_logp=True, job_ids=[2])
    assert np.array_equal(sub[0, 0], logp[2, 0])


def test_retry_loop_records_every_sampled_row():
    from hudiff_amd.sampler import sample_jobs_with_retry
    jobs = _jobs()
    accept = lambda row: int(row[1]) % 2 == 0
    fake = FakeModel()
    plain = sample_jobs_with_retry(fake, jobs, 2, 5, want=2, tries=3, accept=accept)
    assert all("return_logp" not in c for c in fake.sample_calls)
    records = []
    out = sample_jobs_with_retry(FakeModel(), jobs, 2, 5, want=2, tries=3, accept=accept, logp_records=records)
    assert [[r.tolist() for r in o] for o in out] == [[r.tolist() for r in o] for o in plain]
    for j in range(len(jobs)):
        mine = [r for r in records if r[0] == j]
        assert sum(r[5] for r in mine) == len(out[j])                    # chosen rows = written rows
        assert all(r[3] == len(jobs[j].loc) for r in mine)
        sweeps = sorted(set(r[1] for r in mine))
        assert sweeps == list(range(len(sweeps))) and len(mine) == 2 * len(sweeps)
        for _, sweep, r, T, lp, _ in mine:
            want = sum(np.float32(FakeModel.value(j * 2 + r, t, 5 + 1000003 * sweep)) for t in range(T))
            assert abs(lp - want) < 1e-6


def test_score_jobs_plumbing():
    from hudiff_amd import scoring
    jobs, orders, seed = _jobs(complete=True), 4, 9
    fake = FakeModel()
    res = scoring.score_jobs(fake, jobs, orders=orders, seed=seed, device_batch=5)
    assert res["total"].shape == (3, orders) and res["logp"].shape == (3, orders, 6) and res["order"].shape == (3, orders, 6)
    assert res["mean"].shape == res["std"].shape == res["per_residue"].shape == (3,)
    assert res["T"].tolist() == [4, 0, 6]
    assert sum(c["B"] for c in fake.score_calls) == 3 * orders and max(c["B"] for c in fake.score_calls) <= 5
    assert all(c["dropout"] == "off" and c["seed"] == seed for c in fake.score_calls)
    for j, job in enumerate(jobs):
        for k in range(orders):
            o = res["order"][j, k, :len(job.loc)]
            assert sorted(o.tolist()) == sorted(job.loc.tolist())         # a visiting order of exactly the job's slots
            want = sum(np.float32(FakeModel.value(j * orders + k, int(s), seed)) for s in o)
            assert abs(res["total"][j, k] - want) < 1e-5
            assert (res["logp"][j, k, len(job.loc):] == 0).all()
        assert abs(res["mean"][j] - res["total"][j].mean()) < 1e-12 and abs(res["std"][j] - res["total"][j].std()) < 1e-12
    assert res["per_residue"][1] == 0.0 and abs(res["per_residue"][2] - res["mean"][2] / 6) < 1e-12
    assert len({tuple(res["order"][2, k]) for k in range(orders)}) > 1    # the orders differ ...
    again = scoring.score_jobs(FakeModel(), jobs, orders=orders, seed=seed, device_batch=64)
    assert np.array_equal(again["order"], res["order"]) and np.array_equal(again["total"], res["total"])      # ... and are reproducible
    other = scoring.score_jobs(FakeModel(), jobs, orders=orders, seed=seed + 1)
    assert not np.array_equal(other["order"], res["order"])
    # a job's orders do not depend on what else is scored
    sub = scoring.score_jobs(FakeModel(), jobs[2:], orders=orders, seed=seed, job_ids=[2])
    assert np.array_equal(sub["order"][0], res["order"][2]) and np.array_equal(sub["total"][0], res["total"][2])
    with pytest.raises(ValueError):
        scoring.score_jobs(FakeModel(), jobs, orders=0)


def test_score_jobs_passes_antibody_chain_ids():
    from hudiff_amd import scoring
    from hudiff_amd.sampler import Job
    L = 10
    jobs = [Job(tokens=np.full(L, 2, np.int32), region=np.zeros(L, np.int32), loc=np.array([1, 2]), chain=(0, 1 + j % 2), name=str(j))
            for j in range(3)]
    fake = FakeModel(kind="ab", L=L)
    scoring.score_jobs(fake, jobs, orders=2, device_batch=64)
    assert fake.score_calls[0]["chain"].tolist() == [0] * 6 + [1, 1, 2, 2, 1, 1]


def test_parallel_scoring_with_dropout_is_refused():
    """model.score(parallel=True) with dropout on raises before anything touches the device."""
    from hudiff_amd.model import _Denoiser
    m = object.__new__(_Denoiser)
    with pytest.raises(ValueError, match="dropout"):
        m.score(None, None, None, None, None, dropout="faithful", parallel=True)


# ---- sidecar CSV --------------------------------------------------------------------------------------------------------------
def test_logp_sidecar_writer(tmp_path):
    from hudiff_amd.cli.common import write_logp_csv
    path = str(tmp_path / "logp.csv")
    write_logp_csv(path, [("ab1", 0, 0, 98, -101.25, True), ("ab1", 0, 1, 98, np.float64(-99.5), False)])
    assert open(path).read() == "name,pass,replica,T,logp,chosen\nab1,0,0,98,-101.250000,1\nab1,0,1,98,-99.500000,0\n"
    write_logp_csv(path, [("7", 1, 0, 2, 60, -3.0, 1)], sweep=True)
    assert open(path).read() == "name,sweep,pass,replica,T,logp,chosen\n7,1,0,2,60,-3.000000,1\n"
    with pytest.raises(ValueError):
        write_logp_csv(path, [("7", 1, 0, 2, 60, -3.0, 1)])


# ---- score CLI, host side -----------------------------------------------------------------------------------------------------
def test_score_cli_readers_and_jobs(tmp_path):
    """Every row of a pairs CSV / VHH CSV / sampler output is read; the jobs carry COMPLETE tokens and the slots the sampler's mask
    mode would sample; the output has the documented header."""
    from hudiff_amd import inputs as I
    from hudiff_amd.cli import score as cli
    from test_host_logic import H_SEQ, L_SEQ, fake_numbering
    pairs = tmp_path / "pairs.csv"
    pairs.write_text(f"type,name,h_seq,l_seq\nmouse,a1,{H_SEQ},{L_SEQ}\nhuman,a1h,{H_SEQ},{L_SEQ}\n")
    assert cli.read_rows(str(pairs), "ab") == [("a1", H_SEQ, L_SEQ), ("a1h", H_SEQ, L_SEQ)]
    result = tmp_path / "sample_humanization_result.csv"
    result.write_text(f"Specific,name,hseq,lseq,\nmouse,a1,{H_SEQ},{L_SEQ}\nhumanization,a1human_sample,{H_SEQ},{L_SEQ}\n")
    assert cli.read_rows(str(result), "ab") == [("a1", H_SEQ, L_SEQ), ("a1human_sample", H_SEQ, L_SEQ)]
    vhh = tmp_path / "vhh.csv"
    vhh.write_text(f"vhhseq\n{H_SEQ}\n{H_SEQ[1:]}\n")
    assert cli.read_rows(str(vhh), "nb") == [("0", H_SEQ, None), ("1", H_SEQ[1:], None)]
    nres = tmp_path / "nano_result.csv"
    nres.write_text(f"Specific,name,hseq,\nnano,0,{H_SEQ}\nhumanization,0human_sample,{H_SEQ}\n")
    assert cli.read_rows(str(nres), "nb") == [("0", H_SEQ, None), ("0human_sample", H_SEQ, None)]
    numbered = [{"h": fake_numbering(H_SEQ, "H"), "l": fake_numbering(L_SEQ, "L"), "l_chain": "K"}]
    for mask, finetune in (("finetune", True), ("pretrain", False)):
        job, = cli.build_jobs([("a1", H_SEQ, L_SEQ)], "ab", mask, numbered, "auto")
        tok, reg, chain, loc = I.antibody_row(numbered[0]["h"], numbered[0]["l"], "K", finetune=finetune)
        assert np.array_equal(job.loc, loc) and job.chain == chain and np.array_equal(job.region, reg)
        assert (job.tokens != 22).all() and np.array_equal(np.where(tok == 22, job.tokens, tok), job.tokens) and (tok[loc] == 22).all()
    for mask, inpaint in (("plain", False), ("inpaint", True)):
        job, = cli.build_jobs([("0", H_SEQ, None)], "nb", mask, numbered, "auto")
        tok, reg, loc = I.nanobody_row(numbered[0]["h"], inpaint_sample=inpaint)
        assert np.array_equal(job.loc, loc) and (job.tokens != 22).all() and (job.tokens[loc] <= 21).all()
    res = {"T": np.array([len(job.loc)]), "mean": np.array([-12.5]), "std": np.array([0.25]), "per_residue": np.array([-12.5 / len(job.loc)])}
    out = cli.write_scores(str(tmp_path / "scores.csv"), [job], res)
    assert open(out).read().splitlines() == ["name,T,logp_mean,logp_std,logp_per_residue",
                                             f"0,{len(job.loc)},-12.500000,0.250000,{-12.5 / len(job.loc):.6f}"]
    p = cli.build_parser().parse_args(["--ckpt", "x.pt", "--kind", "nb", "--data_fpath", "v.csv"])
    assert (p.orders, p.seed, p.mask, p.dropout, p.precision, p.device_batch, p.gpus, p.numbering) == (1, 2023, None, "off", "default", 256, None, "auto")
