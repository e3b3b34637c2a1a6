"""Truncated sampling, host side (no GPU): guide.Truncation and truncation_keep (the float64 definition of include/hudiff_hip.h
"truncated sampling"), guided_log_probs / confidence_keys with truncation=, the hd_set_truncation binding, and the plumbing from the CLI
flags through sample_jobs[_with_retry] / score_jobs with a recording stub model."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from conftest import ROOT
from test_adaptive_host import _Stub, _jobs

ALL = (1 << 22) - 1


def _g(values, fill=-np.inf):
    """22 values: the given ones first, `fill` (not allowed) behind them."""
    g = np.full(22, fill, np.float64)
    g[:len(values)] = values
    return g


# ---- the definition ------------------------------------------------------------------------------------------------------------------
def test_tie_on_g_keeps_the_lower_index_first():
    from hudiff_amd.guide import Truncation, truncation_keep
    g = _g([0.0, 2.0, 1.0, 2.0, 1.0])
    assert np.flatnonzero(truncation_keep(g, Truncation(top_k=1))).tolist() == [1]            # of the two best, token 1
    assert np.flatnonzero(truncation_keep(g, Truncation(top_k=2))).tolist() == [1, 3]
    assert np.flatnonzero(truncation_keep(g, Truncation(top_k=3))).tolist() == [1, 2, 3]      # of the two next, token 2
    assert np.flatnonzero(truncation_keep(g, Truncation(top_k=4))).tolist() == [1, 2, 3, 4]
    # every g equal, everything allowed: ranks are the indices
    assert np.flatnonzero(truncation_keep(np.zeros(22), Truncation(top_k=5))).tolist() == [0, 1, 2, 3, 4]


def test_top_p_keeps_the_token_that_crosses_the_mass_and_drops_the_next():
    from hudiff_amd.guide import Truncation, truncation_keep
    p = np.array([0.05, 0.5, 0.15, 0.3])                     # descending: tokens 1, 3, 2, 0; heads 0.5, 0.8, 0.95, 1
    g = _g(np.log(p) + 3.0)
    for top_p, want in ((0.4, [1]), (0.5, [1]), (0.51, [1, 3]), (0.79, [1, 3]), (0.81, [1, 2, 3]), (0.96, [0, 1, 2, 3])):
        got = np.flatnonzero(truncation_keep(g, Truncation(top_p=top_p))).tolist()
        assert got == want, (top_p, got)
    # before_j < top_p * sum: the token whose head reaches top_p exactly is the last one in (0.5 + 0.25 = 0.75, exact in binary)
    g = _g(np.log(np.array([0.5, 0.25, 0.125, 0.125])))
    assert np.flatnonzero(truncation_keep(g, Truncation(top_p=0.75))).tolist() == [0, 1]
    assert np.flatnonzero(truncation_keep(g, Truncation(top_p=0.76))).tolist() == [0, 1, 2]


def test_min_p_is_relative_to_the_best_token():
    from hudiff_amd.guide import Truncation, truncation_keep
    g = _g(np.log(np.array([0.5, 0.25, 0.125, 0.125])) - 7.0)
    assert np.flatnonzero(truncation_keep(g, Truncation(min_p=0.49))).tolist() == [0, 1]
    assert np.flatnonzero(truncation_keep(g, Truncation(min_p=0.3))).tolist() == [0, 1]
    assert np.flatnonzero(truncation_keep(g, Truncation(min_p=0.2))).tolist() == [0, 1, 2, 3]
    assert np.flatnonzero(truncation_keep(g, Truncation(min_p=0.51))).tolist() == [0]
    assert np.flatnonzero(truncation_keep(g, Truncation(min_p=1.0))).tolist() == [0]


def test_off_values_keep_every_allowed_token():
    from hudiff_amd.guide import Truncation, truncation_keep
    rng = np.random.default_rng(3)
    g = rng.normal(0, 3, (6, 5, 22))
    allow = rng.integers(1, 1 << 22, (6, 5))
    ok = ((allow[..., None] >> np.arange(22)) & 1).astype(bool)
    g = np.where(ok, g, -np.inf)
    for tr in (None, Truncation(), Truncation(top_k=0), Truncation(top_k=22), Truncation(top_p=1.0), Truncation(min_p=0.0),
               Truncation(22, 1.0, 0.0)):
        assert tr is None or tr.neutral
        assert np.array_equal(truncation_keep(g, tr), ok)
    assert not Truncation(top_k=21).neutral and not Truncation(top_p=0.999).neutral and not Truncation(min_p=1e-9).neutral


def test_best_survives_and_forbidden_tokens_never_do():
    from hudiff_amd.guide import Truncation, truncation_keep
    rng = np.random.default_rng(4)
    g = rng.normal(0, 3, (50, 22))
    allow = rng.integers(1, 1 << 22, 50)
    ok = ((allow[:, None] >> np.arange(22)) & 1).astype(bool)
    g = np.where(ok, g, -np.inf)
    best = g.argmax(-1)
    for tr in (Truncation(top_k=1), Truncation(top_p=1e-9), Truncation(min_p=1.0), Truncation(1, 1e-9, 1.0), Truncation(3, 0.5, 0.2),
               Truncation(8, 0.8, 0.05)):
        keep = truncation_keep(g, tr)
        assert keep.shape == g.shape and keep.dtype == bool
        assert keep[np.arange(50), best].all()
        assert not (keep & ~ok).any()
        assert (keep.sum(-1) >= 1).all() and (keep.sum(-1) <= ok.sum(-1)).all()
    # the three hardest settings keep the best token alone
    for tr in (Truncation(top_k=1), Truncation(top_p=1e-9), Truncation(min_p=1.0)):
        assert np.array_equal(truncation_keep(g, tr), np.arange(22)[None, :] == best[:, None])
    # the cuts intersect
    a, b, c = Truncation(top_k=4), Truncation(top_p=0.7), Truncation(min_p=0.1)
    both = truncation_keep(g, Truncation(4, 0.7, 0.1))
    assert np.array_equal(both, truncation_keep(g, a) & truncation_keep(g, b) & truncation_keep(g, c))


def test_keep_set_written_out_per_slot():
    """The vectorised definition against the loop of the header, slot by slot."""
    from hudiff_amd.guide import Truncation, truncation_keep
    rng = np.random.default_rng(5)
    g = np.round(rng.normal(0, 2, (40, 22)), 1)              # (rounded: ties on g occur)
    g[rng.random((40, 22)) < 0.3] = -np.inf
    g[:, 7] = np.where(np.isinf(g).all(-1), 0.0, g[:, 7])
    tr = Truncation(6, 0.85, 0.03)
    keep = truncation_keep(g, tr)
    for r in range(40):
        al = g[r] > -np.inf
        mx = g[r].max()
        e = np.where(al, np.exp(g[r] - mx), 0.0)
        for j in range(22):
            ahead = [i for i in range(22) if al[i] and (g[r, i] > g[r, j] or (g[r, i] == g[r, j] and i < j))]
            want = al[j] and ((len(ahead) < 6 and sum(e[i] for i in ahead) < 0.85 * e.sum() and e[j] >= 0.03) or not ahead)
            assert keep[r, j] == want, (r, j)


# ---- guided_log_probs / confidence_keys ---------------------------------------------------------------------------------------------------
def test_guided_log_probs_with_truncation():
    from hudiff_amd.guide import Truncation, confidence_keys, guided_log_probs, truncation_keep
    rng = np.random.default_rng(6)
    z = rng.normal(0, 3, (4, 9, 22))
    allow = rng.integers(1, 1 << 22, (4, 9)).astype(np.uint32)
    bias = rng.normal(0, 1, (4, 9, 22)).astype(np.float32)
    base = guided_log_probs(z, allow, bias, 0.7)
    # today's values without the keyword, with None and with a neutral truncation
    ok = ((allow.astype(np.int64)[..., None] >> np.arange(22)) & 1).astype(bool)
    g = np.where(ok, (z + bias.astype(np.float64)) / 0.7, -np.inf)
    want = g - g.max(-1, keepdims=True)
    want = want - np.log(np.exp(want).sum(-1, keepdims=True))
    assert np.array_equal(base, want)
    assert np.array_equal(guided_log_probs(z, allow, bias, 0.7, truncation=None), base)
    assert np.array_equal(guided_log_probs(z, allow, bias, 0.7, truncation=Truncation(top_k=22)), base)
    for tr in (Truncation(top_k=5), Truncation(top_p=0.9), Truncation(min_p=0.1), Truncation(8, 0.8, 0.05)):
        lp = guided_log_probs(z, allow, bias, 0.7, truncation=tr)
        keep = truncation_keep(g, tr)
        assert np.array_equal(np.isneginf(lp), ~keep)
        assert np.allclose(np.exp(lp).sum(-1), 1.0, atol=1e-12)
        # kept tokens keep their ratios: lp - base is one constant per slot
        shift = np.where(keep, lp - np.where(keep, base, 0.0), np.nan)
        assert np.nanmax(np.nanmax(shift, -1) - np.nanmin(shift, -1)) < 1e-12 and (np.nanmin(shift, -1) >= -1e-12).all()
        # the confidence key is 1 / max p'
        ck = confidence_keys(z, allow, bias, 0.7, truncation=tr)
        assert np.allclose(ck, -lp.max(-1), atol=1e-12)
        assert (ck <= confidence_keys(z, allow, bias, 0.7) + 1e-12).all()
    assert np.array_equal(confidence_keys(z, allow, bias, 0.7, truncation=Truncation()), confidence_keys(z, allow, bias, 0.7))
    # top_k = 1: one token with probability 1
    lp = guided_log_probs(z, allow, bias, 1.0, truncation=Truncation(top_k=1))
    assert ((lp == 0.0).sum(-1) == 1).all() and (np.isneginf(lp).sum(-1) == 21).all()
    assert (confidence_keys(z, allow, bias, 1.0, truncation=Truncation(top_k=1)) == 0.0).all()


# ---- validation ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kw", [dict(top_k=-1), dict(top_k=23), dict(top_p=0.0), dict(top_p=1.5), dict(top_p=float("nan")),
                                dict(min_p=-0.1), dict(min_p=1.5), dict(min_p=float("nan")), dict(top_k=2.5), dict(top_p=float("inf"))])
def test_truncation_rejects(kw):
    from hudiff_amd.guide import Truncation
    with pytest.raises(ValueError):
        Truncation(**kw)


def test_truncation_value_object():
    from hudiff_amd import Truncation
    t = Truncation()
    assert (t.top_k, t.top_p, t.min_p) == (0, 1.0, 0.0) and t.neutral
    t = Truncation(8, 0.8, 0.05)
    assert (t.top_k, t.top_p, t.min_p) == (8, 0.8, 0.05) and not t.neutral
    assert t == Truncation(8, 0.8, 0.05) and t != Truncation(8, 0.8, 0.0) and "top_p=0.8" in repr(t)
    assert Truncation(top_k=22, top_p=1, min_p=0).neutral


def test_header_binding_and_library_agree():
    from hudiff_amd import _lib
    text = open(os.path.join(ROOT, "include", "hudiff_hip.h")).read()
    assert re.search(r"typedef struct HdTruncation \{\s*int32_t top_k;[^}]*float top_p;[^}]*float min_p;[^}]*\} HdTruncation;", text)
    assert re.search(r"HdStatus hd_set_truncation\(HdModel\* m, const HdTruncation\* t\);", text)
    assert int(re.search(r"#define HD_ABI_VERSION (\d+)", text).group(1)) == _lib.HD_ABI_VERSION == 1
    assert [n for n, _ in _lib.HdTruncation._fields_] == ["top_k", "top_p", "min_p"] and C.sizeof(_lib.HdTruncation) == 12
    lib = _lib.load()
    assert "hd_set_truncation" in _lib.EXPORTS and hasattr(lib, "hd_set_truncation")


def test_null_handle():
    from hudiff_amd import _lib
    lib = _lib.load()
    assert lib.hd_set_truncation(None, None) == _lib.HD_ERR_INVALID
    t = _lib.HdTruncation(5, 0.9, 0.1)
    assert lib.hd_set_truncation(None, C.byref(t)) == _lib.HD_ERR_INVALID
    assert b"hd_set_truncation" in lib.hd_last_error()


# ---- pass-through -------------------------------------------------------------------------------------------------------------------------
def test_sampler_and_scorer_pass_it_through():
    from hudiff_amd.guide import Truncation
    from hudiff_amd.sampler import sample_jobs, sample_jobs_with_retry
    from hudiff_amd.scoring import score_jobs
    tr = Truncation(8, 0.8, 0.05)
    m = _Stub()
    base = sample_jobs(m, _jobs(), 2, 1)
    for neutral in (None, Truncation(), Truncation(top_k=22)):
        assert np.array_equal(sample_jobs(m, _jobs(), 2, 1, truncation=neutral), base)
    assert all(sorted(c) == ["dropout", "q_noise", "row0", "seed"] for c in m.calls), m.calls        # nothing is passed on
    m = _Stub()
    sample_jobs(m, _jobs(), 2, 1, truncation=tr, return_logp=True)
    assert m.calls and all(c["truncation"] is tr for c in m.calls)
    m = _Stub()
    sample_jobs_with_retry(m, _jobs(), 2, 1, want=1, tries=3, accept=lambda row: False, truncation=tr)
    assert len(m.calls) >= 2 and all(c.get("truncation") is tr for c in m.calls)               # every sweep
    m = _Stub()
    sample_jobs_with_retry(m, _jobs(), 2, 1, want=1, tries=3, accept=lambda row: False, truncation=Truncation())
    assert all("truncation" not in c for c in m.calls)
    jobs = _jobs()
    for j in jobs:
        j.tokens = np.arange(8, dtype=np.int32)
    m = _Stub()
    score_jobs(m, jobs, orders=2, seed=3)
    score_jobs(m, jobs, orders=2, seed=3, truncation=Truncation())
    assert all("truncation" not in c for c in m.score_calls)
    m = _Stub()
    score_jobs(m, jobs, orders=2, seed=3, truncation=tr)
    assert m.score_calls and all(c["truncation"] is tr for c in m.score_calls)


def test_score_jobs_carries_minus_infinity():
    from hudiff_amd.guide import Truncation
    from hudiff_amd.scoring import score_jobs

    class Cut(_Stub):
        def score(self, tokens, region, chain, order, T, **kw):
            out = super().score(tokens, region, chain, order, T, **kw)
            out[0, 0] = -np.inf
            return out
    jobs = _jobs()
    for j in jobs:
        j.tokens = np.arange(8, dtype=np.int32)
    res = score_jobs(Cut(), jobs[:1], orders=1, seed=3, truncation=Truncation(top_k=1))
    assert np.isneginf(res["total"][0, 0]) and np.isneginf(res["mean"][0]) and np.isneginf(res["per_residue"][0])
    assert f"{res['mean'][0]:.6f}" == "-inf"                  # what the score CLI writes


@pytest.mark.parametrize("name", ["sample", "nanosample", "sample_for_anti_cdr", "sample_for_nano_cdr", "score"])
def test_cli_flags_parse(name, capsys):
    import importlib
    cli = importlib.import_module(f"hudiff_amd.cli.{name}")
    base = ["--ckpt", "x.pt"] + (["--kind", "ab", "--data_fpath", "d.csv"] if name == "score" else [])
    a = cli.build_parser().parse_args(base)
    assert (a.top_k, a.top_p, a.min_p) == (0, 1.0, 0.0)
    a = cli.build_parser().parse_args(base + ["--top_k", "5", "--top_p", "0.9", "--min_p", "0.05"])
    assert (a.top_k, a.top_p, a.min_p) == (5, 0.9, 0.05)
    with pytest.raises(SystemExit):
        cli.build_parser().parse_args(base + ["--top_k", "many"])
    capsys.readouterr()


def test_cli_flags_reach_sample_jobs():
    import argparse
    from hudiff_amd.cli.common import add_block_args, apply_block_args
    from hudiff_amd.guide import Truncation
    from hudiff_amd.sampler import sample_jobs
    p = add_block_args(argparse.ArgumentParser())
    # none of the flags, or their off values: nothing for sample_jobs, nothing for the model
    for argv in ([], ["--top_k", "0"], ["--top_k", "22", "--top_p", "1", "--min_p", "0"]):
        more = apply_block_args(p.parse_args(argv), _jobs())
        assert more == {}
        m = _Stub()
        sample_jobs(m, _jobs(), 2, 1, **more)
        assert all(sorted(c) == ["dropout", "q_noise", "row0", "seed"] for c in m.calls)
    more = apply_block_args(p.parse_args(["--top_p", "0.9"]), _jobs())
    assert more == {"truncation": Truncation(top_p=0.9)}
    more = apply_block_args(p.parse_args(["--top_k", "8", "--top_p", "0.8", "--min_p", "0.05", "--slots_per_step", "4"]), _jobs())
    assert more == {"truncation": Truncation(8, 0.8, 0.05), "slots_per_step": 4}
    m = _Stub()
    sample_jobs(m, _jobs(), 2, 1, **more)
    assert m.calls and all(c["truncation"] == Truncation(8, 0.8, 0.05) and c["slots_per_step"] == 4 for c in m.calls)
    for argv in (["--top_k", "-1"], ["--top_k", "23"], ["--top_p", "0"], ["--top_p", "1.5"], ["--min_p", "-0.1"], ["--min_p", "1.5"]):
        with pytest.raises(ValueError):
            apply_block_args(p.parse_args(argv), _jobs())
