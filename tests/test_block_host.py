"""Block decoding, host side (no GPU): the hd_set_slots_per_step binding, expand_steps with K slots per step, the CLI flag."""
import os
import re

import numpy as np
import pytest

from conftest import ROOT

MASK = 22


def test_header_declares_and_binding_exports():
    from hudiff_amd import _lib
    text = open(os.path.join(ROOT, "include", "hudiff_hip.h")).read()
    assert re.search(r"HdStatus hd_set_slots_per_step\(HdModel\* m, int32_t k\);", text)
    assert "hd_set_slots_per_step" in _lib.EXPORTS
    assert int(re.search(r"#define HD_ABI_VERSION (\d+)", text).group(1)) == _lib.HD_ABI_VERSION == 1
    assert hasattr(_lib.load(), "hd_set_slots_per_step")


def test_set_slots_per_step_rejects_a_null_handle():
    from hudiff_amd import _lib
    lib = _lib.load()
    for k in (1, 4, 0, 65):
        assert lib.hd_set_slots_per_step(None, k) == _lib.HD_ERR_INVALID


def _toy(ab):
    """A ragged toy batch: T = 0, 1, K-ish and longer rows, slots in no particular order."""
    rng = np.random.default_rng(3)
    B, L, Tmax = 6, 19, 9
    tokens = rng.integers(0, 22, (B, L)).astype(np.int32)
    region = rng.integers(0, 7, (B, L)).astype(np.int32)
    chain = np.concatenate([np.zeros(B, np.int32), rng.integers(1, 3, B).astype(np.int32)]) if ab else None
    order = np.stack([rng.permutation(L)[:Tmax] for _ in range(B)]).astype(np.int32)
    T = np.array([9, 0, 1, 4, 7, 8], np.int32)
    return tokens, region, chain, order, T


@pytest.mark.parametrize("ab", [False, True], ids=["nb", "ab"])
@pytest.mark.parametrize("K", [1, 2, 3, 8])
def test_expand_steps_matches_a_brute_force_construction(K, ab):
    from hudiff_amd import scoring
    tokens, region, chain, order, T = _toy(ab)
    B, L = tokens.shape
    Tmax = order.shape[1]
    x = scoring.expand_steps(tokens, region, chain, order, T, slots_per_step=K)
    want = []                                           # (b, first position, masked set, group)
    for b in range(B):
        for t0 in range(0, int(T[b]), K):
            want.append((b, t0, set(order[b, t0:T[b]].tolist()), order[b, t0:min(t0 + K, T[b])].tolist()))
    N = len(want)
    assert x.B == B and x.tokens.shape == (N, L) and x.region.shape == (N, L) and x.order.shape == (N, K) and x.T.shape == (N,)
    assert x.tokens.dtype == x.region.dtype == x.order.dtype == x.T.dtype == np.int32
    for i, (b, t0, masked, group) in enumerate(want):
        assert x.rows[i] == b and x.steps[i] == t0
        assert set(np.flatnonzero(x.tokens[i] == MASK).tolist()) == masked
        keep = np.array([s not in masked for s in range(L)])
        assert np.array_equal(x.tokens[i][keep], tokens[b][keep]) and np.array_equal(x.region[i], region[b])
        assert x.T[i] == len(group) and x.order[i, :len(group)].tolist() == group and (x.order[i, len(group):] == 0).all()
        if ab:
            assert x.chain[i] == chain[b] and x.chain[N + i] == chain[B + b]
    assert (x.chain is None) == (not ab) and (x.chain is None or x.chain.shape == (2 * N,))
    # fold: the value of row i at position j goes back to [b, t0 + j]; nothing else is written
    vals = np.random.default_rng(4).normal(0, 1, (N, K)).astype(np.float32)
    out = x.fold(vals if K > 1 else vals[:, 0], Tmax)
    assert out.shape == (B, Tmax) and out.dtype == np.float32
    ref = np.zeros((B, Tmax), np.float32)
    for i, (b, t0, _, group) in enumerate(want):
        ref[b, t0:t0 + len(group)] = vals[i, :len(group)]
    assert np.array_equal(out, ref)
    assert (out[np.arange(Tmax)[None, :] >= T[:, None]] == 0).all()


@pytest.mark.parametrize("ab", [False, True], ids=["nb", "ab"])
def test_expand_steps_at_one_slot_per_step_is_the_function_as_it_was(ab):
    from hudiff_amd import scoring
    tokens, region, chain, order, T = _toy(ab)
    a = scoring.expand_steps(tokens, region, chain, order, T)
    b = scoring.expand_steps(tokens, region, chain, order, T, slots_per_step=1)
    for f in ("tokens", "region", "chain", "order", "T", "rows", "steps"):
        va, vb = getattr(a, f), getattr(b, f)
        assert (va is None and vb is None) or (va.dtype == vb.dtype and np.array_equal(va, vb)), f
    assert a.B == b.B and a.order.shape[1] == 1 and (a.T == 1).all()
    # ... which is: one row per (b, t), order[b, t:T[b]] masked
    at = 0
    for r in range(tokens.shape[0]):
        for t in range(int(T[r])):
            assert a.rows[at] == r and a.steps[at] == t and a.order[at, 0] == order[r, t]
            assert set(np.flatnonzero(a.tokens[at] == MASK).tolist()) == set(order[r, t:T[r]].tolist())
            at += 1
    assert at == a.tokens.shape[0]
    for bad in (0, 65, -1):
        with pytest.raises(ValueError):
            scoring.expand_steps(tokens, region, chain, order, T, slots_per_step=bad)


@pytest.mark.parametrize("name", ["sample", "nanosample", "sample_for_anti_cdr", "sample_for_nano_cdr", "score"])
def test_cli_flag_parses_and_rejects_out_of_range(name, capsys):
    import importlib
    cli = importlib.import_module(f"hudiff_amd.cli.{name}")
    base = ["--ckpt", "x.pt"] + (["--kind", "ab", "--data_fpath", "d.csv"] if name == "score" else [])
    assert cli.build_parser().parse_args(base).slots_per_step == 1
    for k in (1, 4, 64):
        assert cli.build_parser().parse_args(base + ["--slots_per_step", str(k)]).slots_per_step == k
    for bad in ("0", "65", "-3", "2.5", "k"):
        with pytest.raises(SystemExit):
            cli.build_parser().parse_args(base + ["--slots_per_step", bad])
    capsys.readouterr()


def test_cli_helper_is_silent_at_one():
    import argparse
    import logging
    from hudiff_amd.cli.common import add_block_args, apply_block_args
    from hudiff_amd.sampler import Job
    jobs = [Job(tokens=np.zeros(8, np.int32), region=np.zeros(8, np.int32), loc=np.arange(n)) for n in (5, 7, 7)]
    p = add_block_args(argparse.ArgumentParser())
    records = []
    logger = logging.getLogger("test_block_host")
    logger.setLevel(logging.INFO)
    handler = logging.Handler()
    handler.emit = lambda r: records.append(r.getMessage())
    logger.addHandler(handler)
    try:
        assert apply_block_args(p.parse_args([]), jobs, logger) == {} and apply_block_args(p.parse_args(["--slots_per_step", "1"]), jobs, logger) == {}
        assert records == []
        assert apply_block_args(p.parse_args(["--slots_per_step", "4"]), jobs, logger) == {"slots_per_step": 4}
        assert len(records) == 1 and "Slots per step: 4" in records[0] and "2 (T = 5)" in records[0] and "2 (T = 7)" in records[0]
    finally:
        logger.removeHandler(handler)
