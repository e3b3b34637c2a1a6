"""Host side of the confidence threshold (include/hudiff_hip.h "confidence threshold"): guide.threshold_select against a plain-Python
statement of the rule, guide.confidence_cmax, the argument errors that need no device, the CLI flag, and the proof that every exact-logit
case of tests/threshold_cases.py is decided -- every key is a designed exact value (1.0 or 2.0 where it meets cmax) or at least 1e-4
(relative) away from cmax, and two keys of a row are equal or at least 1e-4 apart -- so the GPU test needs no near-tie exemption."""
import numpy as np
import pytest

import threshold_cases as TC
from hudiff_amd import guide as G

F32 = np.float32
MARGIN = 1e-4


def _same(keys, K, cmax):
    chosen, cnt, perm = G.threshold_select(np.asarray(keys, F32), K, cmax)
    want = TC.rule([float(F32(k)) for k in keys], K, float(F32(cmax)))
    assert (chosen.tolist(), cnt, perm.tolist()) == want, (keys, K, cmax, chosen, cnt, perm, want)
    return chosen.tolist(), cnt, perm.tolist()


def test_threshold_select_edge_cases():
    inf, nan = float("inf"), float("nan")
    # ties on (c, i): the lower position first
    assert _same([2.0, 1.0, 2.0, 1.0], 3, 2.0) == ([1, 3, 0], 3, [1, 3, 0, 2])
    # an infinite key never qualifies (nor a NaN, a zero, a negative one: all +inf), even under cmax = +inf
    assert _same([inf, 3.0, nan, 0.0, -1.0], 4, inf) == ([1], 1, [1, 0, 2, 3, 4])
    assert _same([inf, inf], 2, 5.0) == ([0], 1, [0, 1])
    # q = 0: one slot, the surest
    assert _same([5.0, 4.0, 6.0], 3, 1.5) == ([1], 1, [1, 0, 2])
    # q > K: the cap
    assert _same([1.0, 1.0, 1.0, 1.0, 9.0], 2, 1.0) == ([0, 1], 2, [0, 1, 2, 3, 4])
    # N < K
    assert _same([1.0, 1.0], 4, 1.0) == ([0, 1], 2, [0, 1])
    assert _same([7.0], 64, 22.0) == ([0], 1, [0])
    # an exact tie c == cmax qualifies, the next float above does not
    up = float(np.nextafter(F32(2.0), F32(3.0)))
    assert _same([2.0, up, 2.0], 3, 2.0) == ([0, 2], 2, [0, 2, 1])
    # the rest keeps its previous relative order
    assert _same([9.0, 8.0, 1.0, 7.0, 1.5], 4, 1.6) == ([2, 4], 2, [2, 4, 0, 1, 3])
    with pytest.raises(ValueError):
        G.threshold_select([], 2, 1.0)
    with pytest.raises(ValueError):
        G.threshold_select([1.0], 0, 1.0)


def test_threshold_select_random():
    rng = np.random.default_rng(5)
    for _ in range(300):
        N, K = int(rng.integers(1, 40)), int(rng.integers(1, 9))
        keys = rng.choice(np.array([1.0, 1.5, 2.0, 2.5, 3.0, 22.0, np.inf, np.nan], F32), N)
        _same(keys, K, float(rng.choice([1.0, 1.75, 2.0, 2.25, 25.0])))


def test_confidence_cmax_and_argument_errors():
    assert G.confidence_cmax(1.0) == F32(1.0) and G.confidence_cmax(0.5) == F32(2.0)
    c = G.confidence_cmax(0.11)
    assert isinstance(c, np.float32) and c == F32(1.0) / F32(0.11) and float(c) != 1.0 / 0.11       # one float32 division of the float32 tau
    assert G.confidence_cmax(0.04) > 22.0                    # every finite key (c <= 22) qualifies
    for bad in (float("nan"), float("inf"), -0.1, 1.0001, "0.5", None, True):
        with pytest.raises(ValueError):
            G.confidence_tau(bad)
        with pytest.raises(ValueError):
            G.confidence_cmax(bad)
    assert G.confidence_tau(0) == 0.0
    with pytest.raises(ValueError):
        G.confidence_cmax(0.0)


def test_model_refuses_step_parallel_scoring_and_bad_values():
    """The checks model.score and model._arm make before any call into the library."""
    from hudiff_amd import model as M

    class Stub(M._Denoiser):
        def __init__(self):
            pass
    m = Stub()
    m._policy_id = lambda p: {"given": 0, "confident": 1}[p]
    with pytest.raises(ValueError, match="threshold"):
        m.score(None, None, None, None, None, parallel=True, slot_policy="confident", confidence=0.5)
    with pytest.raises(ValueError, match="confidence"):
        m.score(None, None, None, None, None, slot_policy="confident", confidence=1.5)
    with pytest.raises(ValueError, match="confidence"):
        m._arm(None, 1, 1, "confident", None, None, float("nan"))


def test_exports_and_header_in_step():
    from hudiff_amd import _lib as L
    header = open(__import__("os").path.join(__import__("os").path.dirname(L.HERE), "include", "hudiff_hip.h")).read()
    for name in ("hd_set_confidence", "hd_sample_run_to_end", "hd_sample_progress", "hd_sample_forwards", "hd_sample_keys"):
        assert name in L.EXPORTS and f"HdStatus {name}(" in header


def _parsers():
    from hudiff_amd.cli import nanosample, sample, sample_for_anti_cdr, sample_for_nano_cdr
    return {"sample": (sample, ["--ckpt", "c", "--data_fpath", "d"]), "nanosample": (nanosample, ["--ckpt", "c", "--data_fpath", "d"]),
            "anti": (sample_for_anti_cdr, ["--ckpt", "c"]), "nano": (sample_for_nano_cdr, ["--ckpt", "c", "--nano_complex_fasta", "f"])}


@pytest.mark.parametrize("cli", ["sample", "nanosample", "anti", "nano"])
def test_argparse_errors(cli, capsys):
    from hudiff_amd.cli.common import apply_block_args, parse_with_beam
    mod, base = _parsers()[cli]

    def parse(*more):
        return parse_with_beam(mod.build_parser(), base + list(more))
    assert parse().confidence is None and "confidence" not in apply_block_args(parse(), [])
    ok = parse("--confidence", "0.8", "--slot_policy", "confident", "--slots_per_step", "4", "--top_k", "5", "--temperature", "0.5")
    stats = {}
    kw = apply_block_args(ok, [], forward_stats=stats)
    assert kw["confidence"] == 0.8 and kw["slots_per_step"] == 4 and kw["slot_policy"] == "confident" and kw["forward_stats"] is stats
    assert apply_block_args(parse("--confidence", "1", "--slot_policy", "confident"), []) == {"slot_policy": "confident", "confidence": 1.0}
    for bad in (["--confidence", "0.8"], ["--confidence", "0.8", "--slot_policy", "given"],
                ["--confidence", "0.8", "--slot_policy", "confident", "--max_mutations", "2"],
                ["--confidence", "0.8", "--beam", "4"], ["--confidence", "0.8", "--slot_policy", "confident", "--beam", "4"],
                ["--confidence", "0", "--slot_policy", "confident"], ["--confidence", "1.5", "--slot_policy", "confident"],
                ["--confidence", "nan", "--slot_policy", "confident"], ["--confidence", "x", "--slot_policy", "confident"]):
        with pytest.raises(SystemExit) as e:
            parse(*bad)
        assert e.value.code == 2, bad
        assert "confidence" in capsys.readouterr().err


def test_score_cli_flag(capsys):
    from hudiff_amd.cli import score
    from hudiff_amd.cli.common import check_confidence_args
    p = score.build_parser()
    base = ["--ckpt", "c", "--kind", "nb", "--data_fpath", "d"]
    args = check_confidence_args(p, p.parse_args(base + ["--confidence", "0.7", "--slot_policy", "confident", "--slots_per_step", "3"]))
    assert args.confidence == 0.7
    with pytest.raises(SystemExit) as e:
        check_confidence_args(p, p.parse_args(base + ["--confidence", "0.7"]))
    assert e.value.code == 2 and "confidence" in capsys.readouterr().err


# ---- the exact-logit cases are decided ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(TC.CASES))
def test_exact_cases_are_decided(name):
    case, tau = TC.CASES[name]
    cmax = float(G.confidence_cmax(tau))
    for row in case.rows:
        keys = [TC.key_of(case, d) for d in row]
        for d, c in zip(row, keys):
            n_allowed = int(TC.DC.bits(d.allow).sum())
            g = TC.DC.g_of(case, d)
            designed = (c == 1.0 and (n_allowed == 1 or (case.truncation is not None and case.truncation.top_k == 1))) or \
                       (c == 2.0 and n_allowed == 2 and len(set(g[TC.DC.bits(d.allow)].tolist())) == 1)
            assert np.isfinite(c) and c >= 1.0
            assert designed or abs(c / cmax - 1.0) >= MARGIN, (name, c, cmax)
            if c == cmax:
                assert designed and float(F32(c)) == c
        for a in keys:
            for b in keys:
                assert a == b or abs(a / b - 1.0) >= MARGIN, (name, a, b)
        # and the fp32 mirror decides every forward as the plain rule does
        lst, n = list(range(len(keys))), 0
        while n < len(keys):
            rem = [keys[e] for e in lst[n:]]
            _, cnt, perm = _same(rem, case.K, cmax)
            lst = lst[:n] + [lst[n + i] for i in perm]
            n += cnt


def test_exact_cases_cover_the_rules():
    e = {n: TC.expect(n) for n in TC.CASES}
    # singletons at tau = 1: K per forward while they last (5 qualify, the cap is 2), then one slot per forward
    _, _, perms, fwd, counts, _ = e["singletons_tau1"]
    assert perms[0] == [1, 3, 4, 6, 7, 0, 5, 2] and fwd[0] == [0, 0, 1, 1, 2, 3, 4, 5] and counts[0] == [2, 2, 1, 1, 1, 1]
    assert counts[1] == [1] and counts[2] == [] and perms[3] == [1, 2, 0] and fwd[3] == [0, 0, 1]
    # the exact tie qualifies
    _, _, perms, fwd, counts, _ = e["pairs_tau05"]
    assert perms[0] == [3, 0, 2, 4, 1] and fwd[0] == [0, 0, 0, 0, 1] and counts[1] == [2] and counts[3] == [3] and perms[3] == [0, 2, 1]
    # ... and 1/0.5001 < 2 does not
    _, _, perms, fwd, counts, _ = e["pairs_tau05001"]
    assert perms[0] == [3, 0, 2, 4, 1] and fwd[0] == [0, 1, 2, 3, 4] and counts[3] == [2, 1] and perms[3] == [0, 2, 1]
    _, _, perms, fwd, counts, _ = e["none_qualifying"]
    assert perms[0] == [2, 0, 1, 3] and fwd[0] == [0, 1, 2, 3] and perms[1] == [1, 0]
    _, _, perms, fwd, counts, _ = e["topk1_all_ones"]
    assert perms[0] == [0, 1, 2, 3, 4] and fwd[0] == [0, 0, 1, 1, 2] and fwd[1] == [0, 0]
