"""Beam search, host side (no GPU): the hd_set_beam / hd_beam_state declarations and exports, guide.beam_select (the numpy restatement
of the selection of include/hudiff_hip.h "beam search"), the argument checks and the host backtracking of model.beam_search on a fake
model, sampler.beam_jobs / beam_walk, and the CLI flag with its conflict errors."""
import importlib
import os
import re

import numpy as np
import pytest

from conftest import ROOT

NINF = -np.inf


# ---- header, binding, library -------------------------------------------------------------------------------------------------------
def test_header_binding_and_library_agree():
    from hudiff_amd import _lib
    text = open(os.path.join(ROOT, "include", "hudiff_hip.h")).read()
    assert re.search(r"HdStatus hd_set_beam\(HdModel\* m, int32_t width\);", text)
    assert re.search(r"HdStatus hd_beam_state\(HdModel\* m, float\* score.*, int32_t\* parent.*, float\* cand.*\);", text)
    assert "---- beam search ----" in text
    assert int(re.search(r"#define HD_ABI_VERSION (\d+)", text).group(1)) == _lib.HD_ABI_VERSION == 1
    assert "HD_DBG_COUNT = 38" in text                       # no launch-tally id was added
    lib = _lib.load()
    for name in ("hd_set_beam", "hd_beam_state"):
        assert name in _lib.EXPORTS and hasattr(lib, name)


def test_null_handle_and_range():
    from hudiff_amd import _lib
    lib = _lib.load()
    for w in (0, 1, 64):
        assert lib.hd_set_beam(None, w) == _lib.HD_ERR_INVALID
    assert b"hd_set_beam" in lib.hd_last_error()
    assert lib.hd_beam_state(None, None, None, None) == _lib.HD_ERR_STATE
    assert b"hd_beam_state" in lib.hd_last_error()


# ---- beam_select ---------------------------------------------------------------------------------------------------------------------
def _table(W, fill=NINF):
    return np.full((W, 22), fill, np.float32)


def test_select_orders_by_value_descending():
    from hudiff_amd.guide import beam_select
    c = _table(3)
    c[0, 5], c[1, 2], c[2, 21], c[2, 0] = -1.0, -0.5, -3.0, -2.0
    w, j, v = beam_select(c, 3)
    assert w.tolist() == [1, 0, 2] and j.tolist() == [2, 5, 0] and v.tolist() == [-0.5, -1.0, -2.0] and v.dtype == np.float32
    w, j, v = beam_select(c, 4)
    assert (w[3], j[3], v[3]) == (2, 21, -3.0)


def test_select_exact_ties_go_to_the_smaller_w_then_j():
    from hudiff_amd.guide import beam_select
    c = _table(3)
    c[2, 1] = c[0, 7] = c[0, 3] = c[1, 0] = -1.25
    c[1, 9] = -1.0
    w, j, _ = beam_select(c, 5)
    assert list(zip(w.tolist(), j.tolist())) == [(1, 9), (0, 3), (0, 7), (1, 0), (2, 1)]
    # every value equal: ranks are the (w, j) order
    w, j, v = beam_select(np.zeros((2, 22), np.float32), 30)
    assert w.tolist() == [0] * 22 + [1] * 8 and j.tolist() == list(range(22)) + list(range(8)) and (v == 0).all()


def test_select_dead_rows_and_width_beyond_the_finite_candidates():
    from hudiff_amd.guide import beam_select
    c = _table(4)
    c[0, 4], c[0, 9], c[0, 11] = -0.7, -0.2, -1.9        # rows 1..3 are dead (score -inf): the state after the begin
    w, j, v = beam_select(c, 4)
    assert list(zip(w.tolist(), j.tolist())) == [(0, 9), (0, 4), (0, 11), (0, 0)]
    assert v[:3].tolist() == pytest.approx([-0.2, -0.7, -1.9]) and np.isneginf(v[3])
    w, j, v = beam_select(c, 9)                          # the -inf candidates follow in (w, j) order
    assert list(zip(w.tolist(), j.tolist()))[3:] == [(0, 0), (0, 1), (0, 2), (0, 3), (0, 5), (0, 6)] and np.isneginf(v[3:]).all()


def test_select_nan_ranks_with_minus_infinity():
    from hudiff_amd.guide import beam_select
    c = _table(2)
    c[0, 3], c[1, 1], c[1, 2] = np.nan, -5.0, NINF
    c[0, 20] = -6.0
    w, j, v = beam_select(c, 4)
    assert list(zip(w.tolist(), j.tolist())) == [(1, 1), (0, 20), (0, 0), (0, 1)]
    w, j, v = beam_select(c, 6)
    assert list(zip(w.tolist(), j.tolist()))[2:] == [(0, 0), (0, 1), (0, 2), (0, 3)]
    assert np.isnan(v[5]) and np.isneginf(v[2:5]).all()   # the value is the table's own
    # a whole table of NaN: (w, j) order
    w, j, _ = beam_select(np.full((2, 22), np.nan, np.float32), 3)
    assert w.tolist() == [0, 0, 0] and j.tolist() == [0, 1, 2]


def test_select_against_the_definition_written_out():
    from hudiff_amd.guide import beam_select
    rng = np.random.default_rng(11)
    for W in (1, 3, 9, 64):
        c = np.round(rng.normal(-4, 2, (W, 22)), 1).astype(np.float32)      # (rounded: ties occur)
        c[rng.random((W, 22)) < 0.3] = NINF
        c[rng.random((W, 22)) < 0.02] = np.nan
        w, j, v = beam_select(c, W)
        flat = c.reshape(-1)
        bad = ~(flat > NINF)

        def ahead(a, b):                                     # candidate a ranks in front of candidate b
            if bad[a] != bad[b]:
                return bad[b]
            if not bad[a] and flat[a] != flat[b]:
                return flat[a] > flat[b]
            return a < b
        rank = [sum(ahead(a, b) for a in range(flat.size) if a != b) for b in range(flat.size)]
        want = sorted(range(flat.size), key=lambda b: rank[b])[:W]
        assert sorted(rank) == list(range(flat.size))        # the order is total
        assert (w * 22 + j).tolist() == want
        assert np.array_equal(v, flat[want], equal_nan=True)


def test_select_rejects():
    from hudiff_amd.guide import beam_select
    with pytest.raises(ValueError):
        beam_select(np.zeros((2, 21), np.float32), 1)
    with pytest.raises(ValueError):
        beam_select(np.zeros(22, np.float32), 1)
    for width in (0, 45):
        with pytest.raises(ValueError):
            beam_select(np.zeros((2, 22), np.float32), width)


# ---- beam_search on a fake model ---------------------------------------------------------------------------------------------------------
class _Fake:
    """The methods model.beam_search drives; `run` plays a finished session written by hand."""
    kind, max_len = "nb", 6

    def __init__(self, final=None, score=None, parent=None, logp=None):
        self.final, self.score, self.parent, self.logp = final, score, parent, logp
        self.calls = []

    def beam_begin(self, tokens, region, chain, order, T, width, **kw):
        self.calls.append(("begin", np.array(tokens), np.array(region), chain, np.array(order), np.array(T), width, kw))

    def sample_run(self, t0, t1):
        self.calls.append(("run", t0, t1))

    def sample_end(self):
        return self.final

    def beam_state(self, B, Tmax):
        return self.score, self.parent, np.zeros((B, 22), np.float32)

    def sample_logp(self, B, Tmax):
        return self.logp


def _search(fake, *a, **kw):
    from hudiff_amd.model import _Denoiser
    return _Denoiser.beam_search(fake, *a, **kw)


def test_beam_search_backtracks_parents_on_the_host():
    # G = 2 groups of W = 3, Tmax = 3, T = [3, 1]; group 0's history crosses rows, group 1 stops after one position
    final = np.arange(6 * 6, dtype=np.int32).reshape(6, 6)
    score = np.array([-1.0, -2.0, NINF, -0.5, -0.75, -3.0], np.float32)
    parent = np.array([[0, 1, 2], [0, 0, 0], [0, 1, 1],
                       [0, 0, 0], [0, 0, 0], [0, 0, 0]], np.int32)
    logp = np.array([[-0.1, -0.2, -0.3], [-0.4, -0.5, -0.6], [-0.7, -0.8, -0.9],
                     [-0.5, 0, 0], [-0.75, 0, 0], [-3.0, 0, 0]], np.float32)
    f = _Fake(final, score, parent, logp)
    tokens = np.full((2, 6), 22, np.int32)
    order = np.array([[1, 2, 3], [4, 0, 0]], np.int32)
    tok, sc, hist, live = _search(f, tokens, np.zeros((2, 6), np.int32), None, order, [3, 1], 3)
    assert tok.shape == (2, 3, 6) and np.array_equal(tok.reshape(6, 6), final)
    assert np.array_equal(sc, score.reshape(2, 3)) and live.tolist() == [[True, True, False], [True, True, True]]
    # final row (0, 0): position 2 is its own value, its parent there is row 2, whose parent at position 1 is row 1
    assert hist[0, 0].tolist() == pytest.approx([-0.4, -0.8, -0.3])
    assert hist[0, 1].tolist() == pytest.approx([-0.4, -0.2, -0.6])          # parents 0 at t = 2, then 1 at t = 1
    assert hist[0, 2].tolist() == pytest.approx([-0.1, -0.5, -0.9])          # parents 1, then 0
    # positions a group never ran are identity: row (1, r) reads its own value at position 0
    assert hist[1].tolist() == [[-0.5, 0, 0], [-0.75, 0, 0], [-3.0, 0, 0]]
    begin = [c for c in f.calls if c[0] == "begin"][0]
    assert begin[1].shape == (6, 6) and begin[4].tolist() == [[1, 2, 3]] * 3 + [[4, 0, 0]] * 3 and begin[5].tolist() == [3, 3, 3, 1, 1, 1]
    assert begin[6] == 3 and ("run", 0, 3) in f.calls


def test_beam_search_replicates_rows_chain_and_guide():
    from hudiff_amd.guide import Guide

    class Ab(_Fake):
        kind = "ab"
    W, G, L = 2, 2, 6
    f = Ab(np.zeros((4, L), np.int32), np.zeros(4, np.float32), np.zeros((4, 1), np.int32), np.zeros((4, 1), np.float32))
    allow = np.arange(G * L, dtype=np.uint32).reshape(G, L) + 1
    bias = np.arange(G * L * 22, dtype=np.float32).reshape(G, L, 22)
    tokens = np.array([[1] * L, [2] * L], np.int32)
    _search(f, tokens, np.zeros((G, L), np.int32), [0, 0, 1, 2], np.array([[3], [4]]), [1, 1], W, guide=Guide(allow, bias, 0.5), lanes=1)
    _, tok, reg, chain, order, T, width, kw = f.calls[0]
    assert tok[:, 0].tolist() == [1, 1, 2, 2] and chain.tolist() == [0, 0, 0, 0, 1, 1, 2, 2] and order[:, 0].tolist() == [3, 3, 4, 4]
    g = kw["guide"]
    assert np.array_equal(g.allow, allow[[0, 0, 1, 1]]) and np.array_equal(g.bias, bias[[0, 0, 1, 1]]) and g.temperature == 0.5
    assert kw["lanes"] == 1 and kw["truncation"] is None
    # an [L] guide describes every row as it is
    f.calls.clear()
    _search(f, tokens, np.zeros((G, L), np.int32), [0, 0, 1, 2], np.array([[3], [4]]), [1, 1], W, guide=Guide(allow[0]))
    assert f.calls[0][7]["guide"].allow.shape == (L,)


def test_beam_search_argument_checks():
    from hudiff_amd.guide import Guide
    f = _Fake()
    tok, reg, order = np.zeros((2, 6), np.int32), np.zeros((2, 6), np.int32), np.zeros((2, 2), np.int32)
    for width in (0, 65, -1, 2.5, True):
        with pytest.raises(ValueError, match="width"):
            _search(f, tok, reg, None, order, [1, 1], width)
    with pytest.raises(ValueError):
        _search(f, np.zeros((2, 5), np.int32), reg, None, order, [1, 1], 2)          # tokens are not [G, max_len]
    with pytest.raises(ValueError):
        _search(f, tok, reg[:1], None, order, [1, 1], 2)
    with pytest.raises(ValueError):
        _search(f, tok, reg, None, order, [1, 1, 1], 2)
    with pytest.raises(ValueError):
        _search(f, tok, reg, None, order[0], [1, 1], 2)
    with pytest.raises(ValueError):
        _search(f, tok, reg, None, order, [1, 1], 2, guide=Guide(np.ones((3, 6), np.uint32)))      # a guide of three rows

    class Ab(_Fake):
        kind = "ab"
    with pytest.raises(ValueError, match="chn_type"):
        _search(Ab(), tok, reg, None, order, [1, 1], 2)
    with pytest.raises(ValueError):
        _search(Ab(), tok, reg, [0, 0, 1], order, [1, 1], 2)
    assert not f.calls                                       # nothing reached the device


def test_backtrack_rejects():
    from hudiff_amd.guide import beam_backtrack
    tok, sc, par, lp = np.zeros((4, 6), np.int32), np.zeros(4, np.float32), np.zeros((4, 2), np.int32), np.zeros((4, 2), np.float32)
    with pytest.raises(ValueError):
        beam_backtrack(tok, sc, par, lp, [2, 2], 3)          # 4 rows are not groups of 3
    with pytest.raises(ValueError):
        beam_backtrack(tok, sc[:3], par, lp, [2, 2], 2)
    with pytest.raises(ValueError):
        beam_backtrack(tok, sc, par, lp, [2], 2)
    bad = par.copy()
    bad[1, 0] = 2
    with pytest.raises(ValueError, match="parent"):
        beam_backtrack(tok, sc, bad, lp, [2, 2], 2)


# ---- sampler -----------------------------------------------------------------------------------------------------------------------------
class _BeamStub:
    kind, max_len = "nb", 8

    def __init__(self):
        self.calls = []

    def beam_search(self, tokens, region, chain, order, T, width, **kw):
        G = tokens.shape[0]
        self.calls.append((G, width, kw))
        tok = np.repeat(tokens[:, None], width, 1) + np.arange(width, dtype=np.int32)[None, :, None]
        score = -np.arange(width, dtype=np.float32)[None, :] - tokens[:, :1].astype(np.float32)
        score[:, width - 1] = NINF if width > 1 else score[:, width - 1]
        return tok, score, np.zeros((G, width, order.shape[1]), np.float32), np.isfinite(score)


def _jobs(n):
    from hudiff_amd.sampler import Job
    return [Job(tokens=np.full(8, i, np.int32), region=np.zeros(8, np.int32), loc=np.arange(1 + i % 3), name=str(i)) for i in range(n)]


def test_beam_jobs_batches_by_groups():
    from hudiff_amd.guide import Guide, Truncation
    from hudiff_amd.sampler import beam_jobs
    m = _BeamStub()
    tok, score, logp, live = beam_jobs(m, _jobs(7), 4, device_batch=10)
    assert [c[0] for c in m.calls] == [2, 2, 2, 1] and all(c[1] == 4 and c[2] == {} for c in m.calls)      # floor(10 / 4) groups a launch
    assert tok.shape == (7, 4, 8) and score.shape == (7, 4) and logp.shape == (7, 4, 3) and live.shape == (7, 4)
    assert tok[5, 2].tolist() == [7] * 8 and score[5].tolist()[:3] == [-5.0, -6.0, -7.0] and np.isneginf(score[:, 3]).all()
    assert live[:, :3].all() and not live[:, 3].any()
    m = _BeamStub()
    beam_jobs(m, _jobs(3), 64, device_batch=10)             # a width beyond the device batch: one group a launch
    assert [c[0] for c in m.calls] == [1, 1, 1]
    # temperature, guides and the truncation travel; a neutral truncation does not
    jobs = _jobs(2)
    jobs[1].guide = Guide(np.full(8, 3, np.uint32))
    m = _BeamStub()
    beam_jobs(m, jobs, 2, temperature=0.5, truncation=Truncation(top_k=5))
    kw = m.calls[0][2]
    assert kw["guide"].temperature == 0.5 and kw["guide"].allow.shape == (2, 8) and kw["guide"].allow[1, 0] == 3
    assert kw["truncation"] == Truncation(top_k=5)
    m = _BeamStub()
    beam_jobs(m, _jobs(2), 2, truncation=Truncation())
    assert m.calls[0][2] == {}
    with pytest.raises(ValueError, match="temperature"):
        beam_jobs(m, _jobs(2), 2, temperature=0.0)


def test_beam_walk_is_one_pass_of_the_retry_walk():
    from hudiff_amd.sampler import beam_walk
    rows = [np.array([i]) for i in range(5)]
    even = lambda row: int(row[0]) % 2 == 0
    seen = []
    assert [int(r[0]) for r in beam_walk(rows, 5, 10, even, seen.append)] == [0, 2, 4] and [int(r[0]) for r in seen] == [1, 3]
    assert [int(r[0]) for r in beam_walk(rows, 2, 10, even)] == [0, 2]                       # nothing more is wanted
    assert [int(r[0]) for r in beam_walk(rows, 5, 2, even)] == [0, 1, 2, 4]                  # the row looked at with one try left is written
    assert beam_walk([], 3, 3, even) == []


# ---- CLI -----------------------------------------------------------------------------------------------------------------------------------
SAMPLERS = ["sample", "nanosample", "sample_for_anti_cdr", "sample_for_nano_cdr"]


@pytest.mark.parametrize("name", SAMPLERS)
def test_cli_flag_parses(name, capsys):
    from hudiff_amd.cli.common import parse_with_beam
    cli = importlib.import_module(f"hudiff_amd.cli.{name}")
    base = ["--ckpt", "x.pt"]
    assert parse_with_beam(cli.build_parser(), base).beam == 0
    a = parse_with_beam(cli.build_parser(), base + ["--beam", "8", "--top_k", "5", "--temperature", "0.5", "--forbid", "CM"])
    assert a.beam == 8 and a.top_k == 5 and a.temperature == 0.5 and a.forbid == "CM"
    assert parse_with_beam(cli.build_parser(), base + ["--beam", "64", "--slots_per_step", "1", "--slot_policy", "given"]).beam == 64
    for bad in ("0", "65", "-1", "wide"):
        with pytest.raises(SystemExit):
            cli.build_parser().parse_args(base + ["--beam", bad])
    capsys.readouterr()


@pytest.mark.parametrize("name", SAMPLERS)
@pytest.mark.parametrize("extra,word", [(["--slots_per_step", "2"], "slots_per_step"), (["--slot_policy", "confident"], "slot_policy"),
                                        (["--temperature", "0"], "temperature")])
def test_cli_conflicts_are_argparse_errors(name, extra, word, capsys):
    from hudiff_amd.cli.common import parse_with_beam
    cli = importlib.import_module(f"hudiff_amd.cli.{name}")
    with pytest.raises(SystemExit) as e:
        parse_with_beam(cli.build_parser(), ["--ckpt", "x.pt", "--beam", "4"] + extra)
    assert e.value.code == 2 and word in capsys.readouterr().err
    # without --beam the same flags are today's
    a = parse_with_beam(cli.build_parser(), ["--ckpt", "x.pt"] + extra)
    assert a.beam == 0


def test_score_cli_has_no_beam(capsys):
    from hudiff_amd.cli import score
    with pytest.raises(SystemExit):
        score.build_parser().parse_args(["--ckpt", "x.pt", "--kind", "ab", "--data_fpath", "d.csv", "--beam", "4"])
    capsys.readouterr()


def test_run_beam_applies_the_flags():
    import argparse
    from hudiff_amd.cli.common import add_beam_args, add_block_args, add_guide_args, parse_with_beam, run_beam
    from hudiff_amd.guide import Truncation, letters_mask, ALL_TOKENS
    p = add_beam_args(add_block_args(add_guide_args(argparse.ArgumentParser())))
    p.add_argument("--device_batch", type=int, default=256)
    args = parse_with_beam(p, ["--beam", "3", "--forbid", "CM", "--top_p", "0.9", "--temperature", "2", "--device_batch", "6"])
    m = _BeamStub()
    tokens, score, live = run_beam(m, _jobs(5), args, "nb")
    assert tokens.shape == (5, 3, 8) and score.shape == (5, 3) and live.shape == (5, 3)
    assert [c[0] for c in m.calls] == [2, 2, 1] and all(c[1] == 3 for c in m.calls)
    kw = m.calls[0][2]
    assert kw["truncation"] == Truncation(top_p=0.9) and kw["guide"].temperature == 2.0
    assert (kw["guide"].allow == (ALL_TOKENS & ~letters_mask("CM"))).all()
