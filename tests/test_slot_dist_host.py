"""The distribution record off the GPU (include/hudiff_hip.h "distribution record"): the new symbol and flag of the built library,
`scoring.expand_scan` and `Expanded.fold_dist`, `guide.dist_entropy` / `guide.dist_log_odds`, the scan CLI's CSV writer, and the proof
that the expected distributions of tests/draw_cases.py hold every shape tests/test_gpu_slot_dist.py is there to see: a disallowed token,
a token removed by each of top-k, top-p and min-p, and a singleton."""
import csv
import os

import numpy as np
import pytest

import draw_cases as DC
from hudiff_amd import scoring as SC
from hudiff_amd.guide import LETTERS, Truncation, dist_entropy, dist_log_odds, guided_log_probs, truncation_keep


# ---- the library ---------------------------------------------------------------------------------------------------------------------
def test_symbol_flag_and_header():
    from hudiff_amd import _lib
    lib = _lib.load()
    assert "hd_sample_dist" in _lib.EXPORTS and hasattr(lib, "hd_sample_dist")
    assert lib.hd_sample_dist(None, None) == _lib.HD_ERR_STATE          # NULL handle: no device is touched
    flags = (_lib.HD_DROPOUT_OFF, _lib.HD_DROPOUT_INJECT, _lib.HD_NO_GRAPH, _lib.HD_NO_PRUNE, _lib.HD_ONE_LANE, _lib.HD_LOOP_GRAPH, _lib.HD_RECORD_LOGP)
    assert _lib.HD_RECORD_DIST == 128 and all(_lib.HD_RECORD_DIST & f == 0 for f in flags)         # the next free bit
    header = open(os.path.join(_lib.HERE, "..", "include", "hudiff_hip.h")).read()
    assert "#define HD_ABI_VERSION 1 " in header and "HD_RECORD_DIST      = 128u" in header
    assert "distribution record" in header and "hd_sample_dist(HdModel* m, float* dist" in header
    assert _lib.HD_ABI_VERSION == 1


def test_flags_of_the_binding():
    from hudiff_amd import _lib
    from hudiff_amd.model import _Denoiser
    base = _Denoiser._flags("off")
    assert _Denoiser._flags("off", dist=True) == base | _lib.HD_RECORD_DIST
    assert _Denoiser._flags("off", record=True, dist=True) == base | _lib.HD_RECORD_LOGP | _lib.HD_RECORD_DIST
    assert _Denoiser._flags("off", True, True, 2, False) == base                                  # without the flag: today's value


# ---- expand_scan ---------------------------------------------------------------------------------------------------------------------
def _ragged(L=200):
    """Three jobs: T = 70 (two groups of a masked scan), T = 0, T = 3.  Tokens are residues 0..19, distinct per job."""
    rng = np.random.default_rng(5)
    tokens = rng.integers(0, 20, (3, L)).astype(np.int32)
    region = rng.integers(0, 7, (3, L)).astype(np.int32)
    chain = np.array([0, 0, 0, 1, 2, 1], np.int32)
    T = np.array([70, 0, 3])
    loc = np.zeros((3, 70), np.int32)
    loc[0] = rng.permutation(L)[:70]
    loc[2, :3] = [199, 0, 64]
    return tokens, region, chain, loc, T


def test_expand_scan_given():
    tokens, region, chain, loc, T = _ragged()
    x = SC.expand_scan(tokens, region, chain, loc, T, "given")
    assert x.slots_per_step == 1 and x.B == 3 and x.tokens.shape == (73, 200) and x.order.shape == (73, 1)
    assert x.rows.tolist() == [0] * 70 + [2] * 3 and x.steps.tolist() == list(range(70)) + [0, 1, 2] and (x.T == 1).all()
    for i in range(73):
        b, t = x.rows[i], x.steps[i]
        s = loc[b, t]
        assert x.order[i, 0] == s
        masked = np.flatnonzero(x.tokens[i] == SC.MASK_TOKEN)
        assert masked.tolist() == [s]                                   # that slot alone
        keep = np.arange(200) != s
        assert np.array_equal(x.tokens[i, keep], tokens[b, keep]) and np.array_equal(x.region[i], region[b])
    assert x.chain[:73].tolist() == [0] * 70 + [0] * 3 and x.chain[73:].tolist() == [1] * 70 + [1] * 3      # chain ids follow their rows
    assert not (tokens == SC.MASK_TOKEN).any()                          # the input is untouched


def test_expand_scan_masked_groups_of_at_most_64():
    tokens, region, chain, loc, T = _ragged()
    x = SC.expand_scan(tokens, region, chain, loc, T, "masked")
    assert x.slots_per_step == 64 == SC.SCAN_GROUP and x.order.shape == (3, 64)
    assert x.rows.tolist() == [0, 0, 2] and x.steps.tolist() == [0, 64, 0] and x.T.tolist() == [64, 6, 3]      # ceil(T / 64) rows per job
    assert np.array_equal(x.order[0], loc[0, :64]) and np.array_equal(x.order[1, :6], loc[0, 64:70]) and (x.order[1, 6:] == 0).all()
    assert x.order[2, :3].tolist() == [199, 0, 64] and (x.order[2, 3:] == 0).all()
    for i, b in enumerate(x.rows):
        masked = np.flatnonzero(x.tokens[i] == SC.MASK_TOKEN)
        assert sorted(masked.tolist()) == sorted(loc[b, :T[b]].tolist())                          # ALL of loc, in every group's row
    assert x.chain.tolist() == [0, 0, 0, 1, 1, 1]


def test_expand_scan_edges():
    tokens, region, chain, loc, T = _ragged()
    for ctx in SC.SCAN_CONTEXTS:
        x = SC.expand_scan(tokens[1:2], region[1:2], None, loc[1:2], [0], ctx)                   # a T = 0 job alone: no row
        assert x.tokens.shape == (0, 200) and x.rows.shape == (0,) and x.chain is None
        assert x.fold_dist(np.zeros((0, x.slots_per_step, 22)), 5).shape == (1, 5, 22)
    with pytest.raises(ValueError):
        SC.expand_scan(tokens, region, chain, loc, T, "left")
    with pytest.raises(ValueError):
        SC.expand_scan(tokens, region, chain, loc, [71, 0, 3], "given")
    with pytest.raises(ValueError):
        SC.expand_scan(tokens, region, chain[:4], loc, T, "given")


# ---- fold_dist -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [1, 3, 64])
def test_fold_dist_against_a_loop(K):
    rng = np.random.default_rng(K)
    B, L, Tmax = 4, 90, 70
    T = np.array([70, 0, 5, 64])
    order = np.stack([rng.permutation(L)[:Tmax] for _ in range(B)]).astype(np.int32)
    tokens = rng.integers(0, 20, (B, L)).astype(np.int32)
    x = SC.expand_steps(tokens, np.zeros_like(tokens), None, order, T, slots_per_step=K)
    N = x.rows.shape[0]
    flat = rng.normal(size=(N, K, 22)).astype(np.float32)
    flat[rng.random((N, K, 22)) < 0.1] = -np.inf
    want = np.zeros((B, Tmax, 22), np.float32)
    for i in range(N):
        for j in range(int(x.T[i])):
            want[x.rows[i], x.steps[i] + j] = flat[i, j]
    got = x.fold_dist(flat, Tmax)
    assert got.dtype == np.float32 and got.tobytes() == want.tobytes()
    for b in range(B):
        assert (got[b, T[b]:] == 0).all()
    # one value per position folds the same way
    assert np.array_equal(x.fold(flat[:, :, 7].reshape(N, K) if K > 1 else flat[:, 0, 7], Tmax), got[:, :, 7])


# ---- entropy and log-odds --------------------------------------------------------------------------------------------------------------
def test_dist_entropy_and_log_odds():
    lp = np.full((3, 22), -np.inf)
    lp[0, [2, 9]] = np.log(0.5)                          # two tokens: ln 2
    lp[1, 4] = 0.0                                       # a singleton: 0
    lp[2] = np.log(1.0 / 22)                             # uniform: ln 22
    h = dist_entropy(lp.astype(np.float32))
    assert h.dtype == np.float64 and h.shape == (3,)
    assert np.allclose(h, [np.log(2), 0.0, np.log(22)], atol=1e-6) and h[1] == 0.0 and not np.isnan(h).any()
    odds = dist_log_odds(lp, [2, 4, 0])
    assert odds.dtype == np.float64 and odds.shape == (3, 22)
    assert odds[0, 2] == 0 and odds[0, 9] == 0 and np.isneginf(odds[0, 0]) and odds[1, 4] == 0 and np.isneginf(odds[1, 5])
    assert (odds[2] == 0).all()
    gone = dist_log_odds(lp, [0, 4, 0])                  # a wild type that is itself removed: +inf against it, nan for the removed ones
    assert np.isposinf(gone[0, 2]) and np.isnan(gone[0, 0])
    x = np.random.default_rng(0).normal(size=(2, 5, 22))
    wt = np.random.default_rng(1).integers(0, 22, (2, 5))
    assert np.array_equal(dist_log_odds(x, wt), x - np.take_along_axis(x, wt[..., None], -1))
    with pytest.raises(ValueError):
        dist_entropy(np.zeros((3, 21)))
    with pytest.raises(ValueError):
        dist_log_odds(lp, [0, 22, 0])


# ---- the CSV writer ------------------------------------------------------------------------------------------------------------------
def read_scan_csv(path):
    """The file back as arrays: per row (name, chain, imgt, slot, wt letter, logp_wt float32, entropy float64, dist float32 [22])."""
    with open(path, newline="") as f:
        rows = list(csv.reader(f))
    return rows[0], [(r[0], r[1], r[2], int(r[3]), r[4], np.float32(r[5]), float(r[6]), np.array(r[7:], np.float32)) for r in rows[1:]]


def test_scan_csv_writer(tmp_path):
    from types import SimpleNamespace
    from hudiff_amd import tables as TB
    from hudiff_amd.cli import scan
    rng = np.random.default_rng(2)
    T = np.array([3, 0, 2])
    dist = np.zeros((3, 3, 22), np.float32)
    dist[0], dist[2, :2] = rng.normal(size=(3, 22)), rng.normal(size=(2, 22))
    dist[0, 1, [0, 21]] = -np.inf
    dist[2, 0, :] = -np.inf
    dist[2, 0, 5] = 0.0
    slot = np.array([[0, 151, 152], [0, 0, 0], [290, 13, 0]], np.int32)
    wt = np.array([[3, 7, 21], [0, 0, 0], [5, 19, 0]], np.int32)
    res = {"dist": dist, "slot": slot, "wt": wt, "T": T, "logp_wt": np.take_along_axis(dist, wt[..., None].astype(np.int64), 2)[..., 0],
           "entropy": dist_entropy(dist)}
    jobs = [SimpleNamespace(name=n) for n in ("a", "b", "c")]
    path = scan.write_scan(str(tmp_path / "scan.csv"), jobs, res)
    head, rows = read_scan_csv(path)
    assert head == scan.COLUMNS and len(head) == 7 + 22 and head[7:] == ["lp_" + ("gap" if c == "-" else c) for c in LETTERS]
    assert [r[0] for r in rows] == ["a", "a", "a", "c", "c"]            # one row per (sequence, scanned position); T = 0 writes none
    assert [(r[1], r[2]) for r in rows] == [("H", TB.HEAVY_POSITIONS[0]), ("H", TB.HEAVY_POSITIONS[151]), ("L", TB.LIGHT_POSITIONS[0]),
                                            ("L", TB.LIGHT_POSITIONS[138]), ("H", TB.HEAVY_POSITIONS[13])]
    at = [(0, 0), (0, 1), (0, 2), (2, 0), (2, 1)]
    for r, (j, t) in zip(rows, at):
        assert r[3] == slot[j, t] and r[4] == LETTERS[wt[j, t]]
        assert r[7].tobytes() == dist[j, t].tobytes() and np.float32(r[5]).tobytes() == res["logp_wt"][j, t].tobytes()      # bit for bit
        assert r[6] == res["entropy"][j, t]
    text = open(path).read()
    assert ",-inf," in text and "-Infinity" not in text and "nan" not in text
    assert rows[3][7][5] == 0 and np.isneginf(np.delete(rows[3][7], 5)).all()


# ---- the expected distributions of the exact-logit cases hold every shape that matters ------------------------------------------------------
def _expected_dists():
    """(case, entry, expected float64 [22], g float32 [22]) of every entry of every "draw" and "confident" case that ends clean."""
    for case in DC.cases():
        if case.family not in ("draw", "confident") or case.error:
            continue
        for row in case.rows:
            for d in row:
                g = DC.g_of(case, d)
                yield case, d, guided_log_probs(g, d.allow, truncation=case.truncation), g


def test_draw_cases_hold_every_shape():
    seen = set()
    for case, d, lp, g in _expected_dists():
        assert lp.shape == (22,) and not np.isnan(lp).any() and not np.isposinf(lp).any()
        assert abs(np.log(np.exp(lp).sum())) < 1e-12                    # a distribution
        fin = np.isfinite(lp)
        if not DC.bits(d.allow).all():
            assert np.isneginf(lp[~DC.bits(d.allow)]).all()
            seen.add("disallowed")
        if fin.sum() == 1:
            assert lp[fin][0] == 0.0
            seen.add("singleton")
        tr = case.truncation
        if tr is not None:
            allowed = DC.bits(d.allow)
            for name, only in (("top_k", Truncation(top_k=tr.top_k)), ("top_p", Truncation(top_p=tr.top_p)), ("min_p", Truncation(min_p=tr.min_p))):
                if not only.neutral and (allowed & ~truncation_keep(g, only)).any():
                    assert (allowed & ~fin).any()                       # the whole cut removes at least what one of its parts removes
                    seen.add(name)
    assert seen == {"disallowed", "singleton", "top_k", "top_p", "min_p"}, seen


def test_numeric_cases_are_the_ones_left_out():
    assert [c.name for c in DC.cases() if c.error == "numeric"] == ["guided_overflow"]
