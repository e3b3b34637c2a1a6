"""Host side of the refinement rounds (include/hudiff_hip.h "refinement rounds"), no GPU: guide.refine_select against a brute-force
restatement of the rule, the capacity recurrence, the fold to live positions, argument and argparse checks, the new symbols of the
built library against the header and the binding, and the returns of hd_set_refine / hd_refine_state that need no device."""
import os

import numpy as np
import pytest

from hudiff_amd import _lib as L
from hudiff_amd.guide import refine_args, refine_fold, refine_live, refine_select, refine_tcap

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _brute(logp, order, T_now, slots, below):
    """The rule, restated slot by slot in plain Python: live position = the last position below T_now holding the slot; candidates have
    logp < below as float32; rank by (logp, position); the first min(slots, candidates)."""
    last = {}
    for t in range(T_now):
        if order[t] >= 0:
            last[int(order[t])] = t
    cand = []
    for s, u in last.items():
        v = np.float32(logp[u])
        if v < np.float32(below):                    # (False for NaN)
            cand.append((float(v), u, s))
    cand.sort(key=lambda c: (c[0], c[1]))
    cand = cand[:slots]
    return [c[2] for c in cand], [c[1] for c in cand]


def _random_record(rng, L_=40):
    """A row as rounds leave it: a list without repeats, then appended rounds with holes in front of them, logp on a coarse grid so that
    ties are common, a few exact zeros, -inf and NaN."""
    T = int(rng.integers(0, 12))
    order = list(rng.permutation(L_)[:T])
    for _ in range(int(rng.integers(0, 4))):
        order += [-1] * int(rng.integers(0, 3))
        live = sorted({s for s in order if s >= 0})
        n = int(rng.integers(0, min(4, len(live)) + 1))
        order += list(rng.permutation(live)[:n])
    T_now = len(order)
    order = np.array(order + list(rng.integers(0, L_, 5)), np.int64)       # (whatever lies behind T_now is never looked at)
    logp = -rng.integers(0, 4, len(order)).astype(np.float32) / 2
    logp[rng.random(len(order)) < 0.05] = -np.inf
    logp[rng.random(len(order)) < 0.05] = np.nan
    return logp, order, T_now


def test_refine_select_against_brute_force():
    rng = np.random.default_rng(0)
    seen = dict(ties=0, cut=0, holes=0, short=0, empty=0)
    for _ in range(400):
        logp, order, T_now = _random_record(rng)
        slots = int(rng.integers(1, 7))
        below = float(rng.choice([0.0, -0.5, -1.0, -2.0]))
        got_s, got_u = refine_select(logp, order, T_now, slots, below)
        want_s, want_u = _brute(logp, order, T_now, slots, below)
        assert got_s.tolist() == want_s and got_u.tolist() == want_u, (logp, order, T_now, slots, below)
        lv = logp[got_u]
        seen["ties"] += int(len(lv) > 1 and (np.diff(lv) == 0).any())
        seen["cut"] += int(below < 0 and (logp[:T_now][refine_live(order, [T_now])[:T_now]] >= below).any())
        seen["holes"] += int((order[:T_now] == -1).any())
        seen["short"] += int(0 < len(got_s) < slots)
        seen["empty"] += int(len(got_s) == 0)
        assert len(set(got_s.tolist())) == len(got_s) and (got_s >= 0).all()
        assert np.array_equal(order[got_u], got_s)
    assert all(v > 10 for v in seen.values()), seen


def test_refine_select_edges():
    lp = np.array([0.0, -1.0, -1.0, -3.0, -0.25], np.float32)
    od = np.array([4, 9, 2, 7, 9])
    # logp == 0 never qualifies at below == 0; the superseded position 1 of slot 9 is history; ties go to the lower position
    s, u = refine_select(lp, od, 5, 8)
    assert s.tolist() == [7, 2, 9] and u.tolist() == [3, 2, 4]
    s, u = refine_select(lp, od, 4, 8)                   # before the redraw of slot 9 its live position is 1
    assert s.tolist() == [7, 9, 2] and u.tolist() == [3, 1, 2]
    assert refine_select(lp, od, 5, 8, -1.0)[0].tolist() == [7]
    assert refine_select(lp, od, 5, 1)[0].tolist() == [7]
    assert refine_select(lp, od, 0, 3)[0].size == 0
    # the compare is on the float32 value
    assert refine_select(np.array([-1e-46], np.float64), np.array([0]), 1, 1)[0].size == 0
    with pytest.raises(ValueError):
        refine_select(lp, od, 6, 1)
    with pytest.raises(ValueError):
        refine_select(lp, od, 5, 0)
    with pytest.raises(ValueError):
        refine_select(lp[:4], od, 4, 1)


def test_refine_tcap_recurrence():
    for T in (0, 1, 3, 6, 64, 65, 291):
        for rounds in (0, 1, 2, 16):
            for R in (1, 3, 64):
                for K in (1, 2, 4, 64):
                    e = T
                    for _ in range(rounds):
                        e = -(-e // K) * K + R
                    assert refine_tcap(T, rounds, R, K) == e
    assert refine_tcap([6, 3, 0], 2, 3, 2) == 6 + 3 + 1 + 3 and refine_tcap(6, 2, 2, 1) == 10 and refine_tcap(6, 1, 4, 4) == 12
    assert refine_tcap([], 2, 3) == 0 and refine_tcap(np.array([5, 7]), 0, 3) == 7
    with pytest.raises(ValueError):
        refine_tcap(3, 1, 1, 0)


def test_refine_live_and_fold():
    order = np.array([[3, 1, 4, -1, 1, 3, 0, 0], [2, 0, 5, 5, 5, 5, 5, 5]])
    T_now = np.array([6, 2])
    live = refine_live(order, T_now)
    assert live.tolist() == [[False, False, True, False, True, True, False, False], [True, True] + [False] * 6]
    assert refine_live(order[0], [6]).tolist() == live[0].tolist()
    vals = np.arange(16, dtype=np.float32).reshape(2, 8) + 1
    f = refine_fold(order, T_now, vals, 6)
    assert f.shape == (2, 6)
    assert f[0].tolist() == [0, 5, 0, 6, 3, 0] and f[1].tolist() == [10, 0, 9, 0, 0, 0]
    d = np.stack([vals, -vals], axis=-1)
    f2 = refine_fold(order, T_now, d)                    # default L: the largest slot + 1
    assert f2.shape == (2, 6, 2) and np.array_equal(f2[..., 0], f) and np.array_equal(f2[..., 1], -f)
    with pytest.raises(ValueError):
        refine_fold(order, T_now, vals[:, :4])
    with pytest.raises(ValueError):
        refine_live(order, [6])


def test_refine_args():
    assert refine_args(None) is None and refine_args(dict(rounds=0, slots=99)) is None
    assert refine_args(dict(rounds=2, slots=3)) == (2, 3, 0.0)
    assert refine_args(dict(rounds=16, slots=64, below=-0.5)) == (16, 64, -0.5)
    assert refine_args(dict(rounds=1, slots=1, below=-0.1))[2] == float(np.float32(-0.1))
    for bad in (dict(rounds=17, slots=1), dict(rounds=-1, slots=1), dict(rounds=1, slots=0), dict(rounds=1, slots=65),
                dict(rounds=1, slots=1, below=0.5), dict(rounds=1, slots=1, below=float("nan")), dict(rounds=1, slots=1, below=float("-inf")),
                dict(rounds=1.5, slots=1), dict(rounds=1, slots=True), dict(rounds=1, slots=1, more=2), dict(slots=1), 3, "x"):
        with pytest.raises(ValueError):
            refine_args(bad)


def test_symbols_header_and_binding_agree():
    lib = L.load()
    header = open(os.path.join(ROOT, "include", "hudiff_hip.h")).read()
    for name in ("hd_set_refine", "hd_refine_state"):
        assert name in L.EXPORTS and hasattr(lib, name) and f"HdStatus {name}(" in header
    assert "refinement rounds" in header
    assert len(lib.hd_set_refine.argtypes) == 4 and len(lib.hd_refine_state.argtypes) == 4
    assert (L.REFINE_MAX_ROUNDS, L.REFINE_MAX_SLOTS) == (16, 64)


def test_returns_that_need_no_device():
    """hd_set_refine looks at its values before it looks at the handle, so every range check answers without a device; each message
    names the argument it refused."""
    lib = L.load()
    for bad, word in (((-1, 1, 0.0), b"rounds"), ((17, 1, 0.0), b"rounds"), ((1, 0, 0.0), b"slots"), ((1, 65, 0.0), b"slots"),
                      ((16, 64, 0.5), b"below"), ((1, 1, float("nan")), b"below"), ((1, 1, float("inf")), b"below"),
                      ((1, 1, float("-inf")), b"below"), ((1, 1, 0.0), b"null model"), ((16, 64, -3.0), b"null model"),
                      ((0, 0, 0.0), b"null model"), ((0, 99, 7.0), b"null model")):
        assert lib.hd_set_refine(None, *bad) == L.HD_ERR_INVALID, bad
        msg = lib.hd_last_error()
        assert b"hd_set_refine" in msg and word in msg, (bad, msg)
    assert lib.hd_refine_state(None, None, None, None) == L.HD_ERR_STATE
    assert b"hd_refine_state" in lib.hd_last_error()


def _parser(module):
    import importlib
    return importlib.import_module(f"hudiff_amd.cli.{module}").build_parser()


@pytest.mark.parametrize("module", ["sample", "nanosample", "sample_for_anti_cdr", "sample_for_nano_cdr"])
def test_cli_parsing(module):
    from hudiff_amd.cli.common import apply_refine_args, parse_with_beam
    p = _parser(module)
    req = [a for act in p._actions if act.required for a in (act.option_strings[0], "x")]
    args = parse_with_beam(p, req)
    assert args.refine_rounds == 0 and apply_refine_args(args) == {}
    args = parse_with_beam(p, req + ["--refine_rounds", "2"])
    assert apply_refine_args(args) == {"refine": dict(rounds=2, slots=8, below=0.0)}
    args = parse_with_beam(p, req + ["--refine_rounds", "3", "--refine_slots", "5", "--refine_below", "-0.7", "--slots_per_step", "4"])
    assert apply_refine_args(args) == {"refine": dict(rounds=3, slots=5, below=-0.7)}
    for bad in (["--refine_rounds", "17"], ["--refine_rounds", "-1"], ["--refine_rounds", "1", "--refine_slots", "0"],
                ["--refine_rounds", "1", "--refine_slots", "65"], ["--refine_rounds", "1", "--refine_below", "0.1"],
                ["--refine_rounds", "1", "--refine_below", "nan"], ["--refine_slots", "4"], ["--refine_below", "-1"],
                ["--refine_rounds", "1", "--beam", "4"], ["--refine_rounds", "1", "--max_mutations", "2"],
                ["--refine_rounds", "1", "--slot_policy", "confident", "--confidence", "0.5"]):
        with pytest.raises(SystemExit):
            parse_with_beam(p, req + bad)


def test_score_cli_does_not_take_the_flags():
    p = _parser("score")
    assert not any("--refine_rounds" in act.option_strings for act in p._actions)


def test_logp_sidecar_column(tmp_path):
    from hudiff_amd.cli.common import write_logp_csv
    a, b = str(tmp_path / "a.csv"), str(tmp_path / "b.csv")
    write_logp_csv(a, [("x", 0, 1, 7, -3.5, True)])
    assert open(a).read() == "name,pass,replica,T,logp,chosen\nx,0,1,7,-3.500000,1\n"        # without the flags: byte for byte as before
    write_logp_csv(b, [("x", 0, 1, 7, -3.5, True, 4)], redrawn=True)
    assert open(b).read() == "name,pass,replica,T,logp,chosen,redrawn\nx,0,1,7,-3.500000,1,4\n"
    write_logp_csv(b, [("x", 2, 0, 1, 7, -3.5, 0, 4)], sweep=True, redrawn=True)
    assert open(b).read() == "name,sweep,pass,replica,T,logp,chosen,redrawn\nx,2,0,1,7,-3.500000,0,4\n"
    with pytest.raises(ValueError):
        write_logp_csv(b, [("x", 0, 1, 7, -3.5, True)], redrawn=True)
