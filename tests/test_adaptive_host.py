"""Slot policy, host side (no GPU): the hd_set_slot_policy / hd_sample_order bindings, guide.confidence_keys, the sampler and scorer
plumbing with a stub model, the CLI flag."""
import os
import re

import numpy as np
import pytest

from conftest import ROOT


def test_header_binding_and_library_agree():
    from hudiff_amd import _lib
    text = open(os.path.join(ROOT, "include", "hudiff_hip.h")).read()
    assert re.search(r"HdStatus hd_set_slot_policy\(HdModel\* m, int32_t policy\);", text)
    assert re.search(r"HdStatus hd_sample_order\(HdModel\* m, int32_t\* order", text)
    assert re.search(r"enum \{ HD_SLOTS_GIVEN = 0, HD_SLOTS_CONFIDENT = 1 \};", text)
    assert (_lib.HD_SLOTS_GIVEN, _lib.HD_SLOTS_CONFIDENT) == (0, 1)
    assert _lib.SLOT_POLICIES == {"given": 0, "confident": 1}
    assert int(re.search(r"#define HD_ABI_VERSION (\d+)", text).group(1)) == _lib.HD_ABI_VERSION == 1
    lib = _lib.load()
    for name in ("hd_set_slot_policy", "hd_sample_order"):
        assert name in _lib.EXPORTS and hasattr(lib, name)


def test_null_handles():
    from hudiff_amd import _lib
    lib = _lib.load()
    for v in (0, 1, 2, -1):
        assert lib.hd_set_slot_policy(None, v) == _lib.HD_ERR_INVALID
    assert lib.hd_sample_order(None, None) == _lib.HD_ERR_STATE
    buf = np.zeros(4, np.int32)
    assert lib.hd_sample_order(None, _lib.ptr(buf, __import__("ctypes").c_int32)) == _lib.HD_ERR_STATE


def _direct(z, allow, bias, temperature):
    """One slot, written out: log sum_j exp(g_j - max g) over the allowed j."""
    g = []
    for j in range(22):
        if allow is not None and not (int(allow) >> j) & 1:
            continue
        v = float(z[j]) + (0.0 if bias is None else float(bias[j]))
        g.append(v if temperature == 0 else v / temperature)
    mx = max(g)
    return float(np.log(sum(np.exp(v - mx) for v in g)))


@pytest.mark.parametrize("temperature", [1.0, 0.5, 0.0])
@pytest.mark.parametrize("guided", [False, True])
def test_confidence_keys_against_a_direct_evaluation(temperature, guided):
    from hudiff_amd.guide import confidence_keys
    rng = np.random.default_rng(11)
    B, L = 3, 7
    z = rng.normal(0, 3, (B, L, 23))
    allow = bias = None
    if guided:
        allow = rng.integers(1, 1 << 22, (B, L)).astype(np.uint32)
        allow[0, 0] = 1 << 9                             # a singleton: c = 1, log c = 0
        bias = rng.normal(0, 1, (B, L, 22)).astype(np.float32)
    got = confidence_keys(z, allow, bias, temperature)
    assert got.shape == (B, L) and got.dtype == np.float64
    for b in range(B):
        for s in range(L):
            want = _direct(z[b, s], None if allow is None else allow[b, s], None if bias is None else bias[b, s], temperature)
            assert abs(got[b, s] - want) < 1e-12, (b, s)
    assert (got >= 0).all()
    if guided:
        assert got[0, 0] == 0.0
    # the key is 1 / p_max
    if not guided and temperature == 1.0:
        p = np.exp(z[..., :22] - z[..., :22].max(-1, keepdims=True))
        p /= p.sum(-1, keepdims=True)
        assert np.allclose(got, -np.log(p.max(-1)), atol=1e-12)
    # a 22-wide input is the same thing
    assert np.array_equal(confidence_keys(z[..., :22], allow, bias, temperature), got)


def test_confidence_keys_rank_a_broken_row_last():
    from hudiff_amd.guide import confidence_keys
    rng = np.random.default_rng(12)
    z = rng.normal(0, 3, (5, 22))
    z[1, 4] = np.nan
    z[3, 0] = np.inf
    k = confidence_keys(z)
    assert np.isposinf(k[1]) and np.isposinf(k[3]) and np.isfinite(k[[0, 2, 4]]).all()
    rank = np.lexsort((np.arange(5), k))
    assert rank[-2:].tolist() == [1, 3]                  # behind every finite key, the index breaks their tie
    # nothing allowed: no finite positive sum either
    assert np.isposinf(confidence_keys(z[:1], np.zeros(1, np.uint32)))[0]
    # a NaN in a token that is not allowed does not count
    allow = np.full(5, ((1 << 22) - 1) & ~(1 << 4), np.uint32)
    assert np.isfinite(confidence_keys(z, allow)[1])


class _Stub:
    """model.sample / score / sample_order as the sampler and the scorer call them; the 'realised order' is the list reversed."""
    kind, max_len = "nb", 8

    def __init__(self):
        self.calls, self.score_calls, self.last = [], [], None

    def sample(self, tokens, region, chain, order, T, **kw):
        self.calls.append(dict(kw))
        self.last = np.array(order, np.int32, copy=True)
        if kw.get("slot_policy") == "confident":
            for b in range(len(T)):
                self.last[b, :T[b]] = self.last[b, :T[b]][::-1]
        out = np.array(tokens, np.int32, copy=True)
        for b in range(len(T)):
            out[b, order[b, :T[b]]] = (kw["row0"] + b) % 20
        lp = np.where(np.arange(order.shape[1])[None, :] < np.asarray(T)[:, None], -1.0, 0.0).astype(np.float32)
        return (out, lp) if kw.get("return_logp") else out

    def score(self, tokens, region, chain, order, T, **kw):
        self.score_calls.append(dict(kw))
        self.last = np.array(order, np.int32, copy=True)[:, ::-1].copy() if kw.get("slot_policy") == "confident" else np.array(order, np.int32)
        return np.full(order.shape, -0.5, np.float32)

    def sample_order(self, B=None, Tmax=None):
        assert self.last.shape == (B, Tmax)
        return self.last


def _jobs():
    from hudiff_amd.sampler import Job
    return [Job(tokens=np.full(8, 22, np.int32), region=np.zeros(8, np.int32), loc=np.array([1, 2, 5]), name="a"),
            Job(tokens=np.full(8, 22, np.int32), region=np.zeros(8, np.int32), loc=np.array([3, 0]), name="b")]


def test_sampler_plumbing():
    from hudiff_amd.sampler import sample_jobs, sample_jobs_with_retry
    m = _Stub()
    base = sample_jobs(m, _jobs(), 2, 1)
    same = sample_jobs(m, _jobs(), 2, 1, slot_policy="given")
    assert np.array_equal(base, same)
    assert all(sorted(c) == ["dropout", "q_noise", "row0", "seed"] for c in m.calls), m.calls        # "given" passes nothing on
    m = _Stub()
    tok, lp, od = sample_jobs(m, _jobs(), 2, 1, slot_policy="confident", slots_per_step=4, return_logp=True, return_order=True)
    assert m.calls[0]["slot_policy"] == "confident" and m.calls[0]["slots_per_step"] == 4
    assert np.array_equal(tok, base) and lp.shape == (2, 1, 2, 3) and od.shape == (2, 1, 2, 3) and od.dtype == np.int32
    assert od[0, 0].tolist() == [[5, 2, 1]] * 2 and od[1, 0].tolist() == [[0, 3, 0]] * 2             # gathered per (job, replica)
    tok2, od2 = sample_jobs(m, _jobs(), 2, 1, return_order=True)                                    # given: the order handed in
    assert np.array_equal(tok2, base) and od2[0, 0].tolist() == [[1, 2, 5]] * 2 and od2[1, 0].tolist() == [[3, 0, 0]] * 2
    with pytest.raises(ValueError):
        sample_jobs(m, _jobs(), 2, 1, slot_policy="greedy")
    # the retry loop passes it to every sweep
    m = _Stub()
    sample_jobs_with_retry(m, _jobs(), 2, 1, want=1, tries=3, accept=lambda row: False, slot_policy="confident")
    assert len(m.calls) >= 2 and all(c.get("slot_policy") == "confident" for c in m.calls)
    m = _Stub()
    sample_jobs_with_retry(m, _jobs(), 2, 1, want=1, tries=3, accept=lambda row: False)
    assert all("slot_policy" not in c for c in m.calls)


def test_scorer_plumbing():
    from hudiff_amd.scoring import draw_orders, score_jobs
    jobs = _jobs()
    for j in jobs:
        j.tokens = np.arange(8, dtype=np.int32)
    m = _Stub()
    res = score_jobs(m, jobs, orders=2, seed=3)
    assert all("slot_policy" not in c for c in m.score_calls)
    assert np.array_equal(res["order"][0, :, :3], draw_orders(jobs[0].loc, 2, 3, 0))
    m = _Stub()
    res = score_jobs(m, jobs, orders=1, seed=3, slot_policy="confident", slots_per_step=2)
    assert m.score_calls[0]["slot_policy"] == "confident" and m.score_calls[0]["slots_per_step"] == 2
    assert res["order"][0, 0].tolist() == [5, 2, 1] and res["order"][1, 0].tolist() == [0, 0, 3]      # the order taken, from loc as it stands
    with pytest.raises(ValueError):
        score_jobs(m, jobs, orders=2, seed=3, slot_policy="confident")


def test_model_rejects_step_parallel_scoring_under_the_policy():
    """model.score raises before anything reaches the library (no handle is needed to see it)."""
    from hudiff_amd import model as M
    obj = object.__new__(M.AntiTFNet)
    with pytest.raises(ValueError, match="confident"):
        M.AntiTFNet.score(obj, None, None, None, None, None, parallel=True, slot_policy="confident")
    with pytest.raises(ValueError, match="slot_policy"):
        M.AntiTFNet.score(obj, None, None, None, None, None, slot_policy="surest")


@pytest.mark.parametrize("name", ["sample", "nanosample", "sample_for_anti_cdr", "sample_for_nano_cdr", "score"])
def test_cli_flag_parses(name, capsys):
    import importlib
    cli = importlib.import_module(f"hudiff_amd.cli.{name}")
    base = ["--ckpt", "x.pt"] + (["--kind", "ab", "--data_fpath", "d.csv"] if name == "score" else [])
    assert cli.build_parser().parse_args(base).slot_policy == "given"
    for v in ("given", "confident"):
        assert cli.build_parser().parse_args(base + ["--slot_policy", v]).slot_policy == v
    with pytest.raises(SystemExit):
        cli.build_parser().parse_args(base + ["--slot_policy", "random"])
    capsys.readouterr()


def test_cli_helper_and_score_cli_argument_error(capsys):
    import argparse
    from hudiff_amd.cli import score as score_cli
    from hudiff_amd.cli.common import add_block_args, apply_block_args
    p = add_block_args(argparse.ArgumentParser())
    assert apply_block_args(p.parse_args(["--slot_policy", "given"]), _jobs()) == {}
    assert apply_block_args(p.parse_args(["--slot_policy", "confident"]), _jobs()) == {"slot_policy": "confident"}
    assert apply_block_args(p.parse_args(["--slot_policy", "confident", "--slots_per_step", "4"]), _jobs()) == \
        {"slot_policy": "confident", "slots_per_step": 4}
    with pytest.raises(SystemExit) as e:
        score_cli.main(["--ckpt", "x.pt", "--kind", "ab", "--data_fpath", "d.csv", "--orders", "2", "--slot_policy", "confident"])
    assert e.value.code == 2 and "--orders 1" in capsys.readouterr().err
