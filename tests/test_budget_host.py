"""The mutation budget off the GPU: the new symbols of the built library, `budget_walk` on hand-written rows, `Budget`, the argparse
errors of the samplers, and the proof that the case table of tests/budget_cases.py is DECIDED -- every comparison an expected result
rests on is a designed exact tie or has a margin of 1e-4 (tests/test_draw_cases_host.py gives the same proof for its cases, and its
`undecided` / `emulate32` are the ones used here, on the entry each draw really met)."""
import ctypes as C

import numpy as np
import pytest

import budget_cases as BC
import draw_cases as DC
from hudiff_amd.guide import FREE, Budget, budget_walk
from test_draw_cases_host import MARGIN, emulate32, undecided


# ---- the library ---------------------------------------------------------------------------------------------------------------------
def test_symbols_and_struct_layout():
    from hudiff_amd import _lib
    lib = _lib.load()
    for name in ("hd_set_budget", "hd_mutation_count"):
        assert name in _lib.EXPORTS and hasattr(lib, name)
    # typedef struct HdBudget { int32_t B; const int32_t* origin; const int32_t* max_mutations; }: 4 + 4 (padding) + 8 + 8
    assert C.sizeof(_lib.HdBudget) == 24
    assert (_lib.HdBudget.B.offset, _lib.HdBudget.origin.offset, _lib.HdBudget.max_mutations.offset) == (0, 8, 16)
    assert _lib.HD_ABI_VERSION == 1
    # NULL handle -> HD_ERR_INVALID (hd_set_budget), HD_ERR_STATE (hd_mutation_count): no device is touched
    assert lib.hd_set_budget(None, None) == _lib.HD_ERR_INVALID
    assert lib.hd_mutation_count(None, None) == _lib.HD_ERR_STATE
    header = open(__import__("os").path.join(_lib.HERE, "..", "include", "hudiff_hip.h")).read()
    assert "#define HD_ABI_VERSION 1 " in header and "hd_set_budget" in header and "mutation budget" in header


# ---- budget_walk ---------------------------------------------------------------------------------------------------------------------
def _walk(written, origin_by_slot, order, M, T=None):
    L = 8
    origin = np.full((1, L), FREE, np.int32)
    for s, o in origin_by_slot.items():
        origin[0, s] = o
    order = np.array([order], np.int32)
    ex, n = budget_walk(np.array([written]), origin, order, [len(written) if T is None else T], [M])
    return ex[0].tolist(), int(n[0])


def test_budget_walk_hand_written_rows():
    org = {0: 3, 1: 4, 2: 5, 3: 6}
    # M = 0: exhausted from the first position on; what is written is still counted
    assert _walk([3, 4, 5], org, [0, 1, 2], 0) == ([True, True, True], 0)
    assert _walk([3, 9, 5], org, [0, 1, 2], 0) == ([True, True, True], 1)
    # M reached mid-row: position 2 is the first exhausted one
    assert _walk([9, 9, 5, 6], org, [0, 1, 2, 3], 2) == ([False, False, True, True], 2)
    # equal to the origin everywhere: never exhausted
    assert _walk([3, 4, 5, 6], org, [0, 1, 2, 3], 1) == ([False] * 4, 0)
    # a free slot is never forced and never counted, whatever the count is
    assert _walk([9, 1, 5], {0: 3, 2: 5}, [0, 1, 2], 1) == ([False, False, True], 1)
    # a repeated slot: every visit is compared with the slot's origin on its own
    assert _walk([9, 3, 9], org, [0, 0, 0], 2) == ([False, False, False], 2)
    assert _walk([9, 9, 3, 9], org, [0, 0, 0, 0], 2) == ([False, False, True, True], 3)
    # targets of a scoring session overrun M: counted all the same
    assert _walk([9, 9, 9, 9], org, [0, 1, 2, 3], 1) == ([False, True, True, True], 4)
    # positions at t >= T are not walked
    assert _walk([9, 9, 9], org, [0, 1, 2], 1, T=1) == ([False, False, False], 1)
    # the gap (21) is an origin like any residue; 22 is not
    assert _walk([21, 20], {0: 21, 1: 22}, [0, 1], 0) == ([True, False], 0)
    with pytest.raises(ValueError):
        budget_walk(np.zeros((1, 2)), np.zeros((1, 8)), np.zeros((2, 2), int), [2, 2], [1, 1])


def test_budget_batch_take_stack():
    L = 5
    one = Budget(np.arange(L), 2)
    o, m = one.batch(3, L)
    assert o.shape == (3, L) and o.dtype == np.int32 and (o == np.arange(L)).all() and m.tolist() == [2, 2, 2] and m.dtype == np.int32
    per = Budget(np.arange(2 * L).reshape(2, L) % 23, [1, 4])
    assert per.batch(2, L)[1].tolist() == [1, 4]
    t = per.take([1, 1, 0])
    o, m = t.batch(3, L)
    assert np.array_equal(o, per.origin[[1, 1, 0]]) and m.tolist() == [4, 4, 1]
    assert one.take([0, 0]).batch(2, L)[1].tolist() == [2, 2]
    st = Budget.stack([one, None, Budget(np.full(L, 7), 0)], L)
    o, m = st.batch(3, L)
    assert np.array_equal(o[0], np.arange(L)) and (o[1] == FREE).all() and (o[2] == 7).all() and m.tolist() == [2, 0, 0]
    for bad in (lambda: Budget(np.zeros((1, 2, 3)), 1), lambda: Budget(np.zeros(L), -1), lambda: Budget(np.zeros(L), 1.5),
                lambda: one.batch(3, L + 1), lambda: per.batch(3, L)):
        with pytest.raises(ValueError):
            bad()


def test_sampler_jobs_carry_the_origin():
    from hudiff_amd.sampler import Job, _stack_budget
    jobs = [Job(tokens=np.zeros(4), region=np.zeros(4), loc=np.arange(2), origin=np.array([1, 2, 3, 4])),
            Job(tokens=np.zeros(4), region=np.zeros(4), loc=np.arange(2))]
    o, m = _stack_budget(jobs, 4, 3).batch(2, 4)
    assert o.tolist() == [[1, 2, 3, 4], [FREE] * 4] and m.tolist() == [3, 0]


# ---- the CLIs' flag ------------------------------------------------------------------------------------------------------------------
def _parsers():
    from hudiff_amd.cli import nanosample, sample, sample_for_anti_cdr, sample_for_nano_cdr
    return {"sample": (sample, ["--ckpt", "c", "--data_fpath", "d"]), "nanosample": (nanosample, ["--ckpt", "c", "--data_fpath", "d"]),
            "anti": (sample_for_anti_cdr, ["--ckpt", "c"]), "nano": (sample_for_nano_cdr, ["--ckpt", "c", "--nano_complex_fasta", "f"])}


@pytest.mark.parametrize("cli", ["sample", "nanosample", "anti", "nano"])
def test_argparse_errors(cli, capsys):
    from hudiff_amd.cli.common import apply_budget_args, parse_with_beam
    mod, base = _parsers()[cli]

    def parse(*more):
        return parse_with_beam(mod.build_parser(), base + list(more))
    assert parse().max_mutations is None and apply_budget_args(parse(), []) == {}
    assert parse("--max_mutations", "3").max_mutations == 3 and parse("--max_mutations", "0").max_mutations == 0
    assert apply_budget_args(parse("--max_mutations", "3"), []) == {"max_mutations": 3}
    # composes with the beam, the guide flags, the confident policy, the greedy decode -- and a truncation without a beam
    ok = parse("--max_mutations", "3", "--beam", "4", "--forbid", "C", "--temperature", "0.5")
    assert ok.beam == 4 and ok.max_mutations == 3
    parse("--max_mutations", "3", "--slot_policy", "confident", "--temperature", "0", "--top_k", "5")
    for bad in (["--max_mutations", "3", "--slots_per_step", "2"], ["--max_mutations", "3", "--beam", "4", "--top_k", "5"],
                ["--max_mutations", "3", "--beam", "4", "--top_p", "0.9"], ["--max_mutations", "3", "--beam", "4", "--min_p", "0.1"],
                ["--max_mutations", "-1"], ["--max_mutations", "x"]):
        with pytest.raises(SystemExit) as e:
            parse(*bad)
        assert e.value.code == 2, bad
        assert "max_mutations" in capsys.readouterr().err
    parse("--max_mutations", "3", "--beam", "4", "--top_k", "22")        # a cut that cuts nothing is none


def test_score_cli_has_no_budget_flag():
    from hudiff_amd.cli import score
    assert not any(a.dest == "max_mutations" for a in score.build_parser()._actions)


# ---- the case table is decided ---------------------------------------------------------------------------------------------------------
def _expect(bc, mode):
    return BC.expect_draws(bc, mode) if bc.case.family == "draw" else BC.expect_confident(bc, mode)


def test_every_budget_draw_is_decided():
    """Every draw, on the entry it really met (the allowed set of rule 1): draw_cases' proof -- float32 emulation and float64 agree on
    keep-set and token, and every ratio, top_p and min_p comparison is a designed tie or has the margin."""
    n, bad = 0, []
    for bc in BC.cases():
        for mode in bc.case.modes:
            x = _expect(bc, mode)
            for r, row in enumerate(x.met):
                for t, (met, q) in enumerate(row):
                    tok, lp = x.draws[r][t]
                    n += 1
                    if np.isneginf(lp) and mode == "score" and x.exhausted[r][t]:
                        continue                         # an exhausted position whose target is not o: nothing is compared
                    why = undecided(bc.case, met, q, mode)
                    if why:
                        bad.append((bc.name, mode, r, t, why))
                    if x.exhausted[r][t]:                # +0.0 exactly in the fp32 emulation as well
                        em = emulate32(DC.g_of(bc.case, met), bc.case.truncation, q, bc.case.temperature == 0)
                        assert lp == 0.0 and em["lp"][tok] == 0.0 and not np.signbit(em["lp"][tok]) and em["esum2"] == 1.0
    print(f"{n} draws, {len(bad)} undecided")
    assert n > 100 and not bad, bad


def test_confident_budget_keys_are_decided():
    """The keys every forward of the confident case compares: equal keys are bit-identical sums (list order decides), different keys
    are apart by the margin; an exhausted origin-bearing entry has the key exactly 1.0f."""
    bc = BC.case("budget_confident")
    pairs = 0
    for mode in bc.case.modes:
        x = BC.expect_confident(bc, mode)
        for keys in (k for row in x.keys for k in row):
            k64 = np.exp(keys)
            for i in range(len(k64)):
                for u in range(i):
                    pairs += 1
                    assert k64[i] == k64[u] or abs(k64[i] - k64[u]) >= MARGIN * max(k64[i], k64[u])
    assert pairs > 20
    row, org = bc.case.rows[0], bc.origin[0]
    for d, o in zip(row, org):
        if o <= 21:
            em = emulate32(DC.g_of(bc.case, BC.forced(d, o)), None, DC.noise_of(d), False)
            assert em["esum2"] == np.float32(1.0) and BC.key_of(bc.case, d, o, 1, 1) == 0.0
    assert BC.key_of(bc.case, row[2], org[2], 1, 1) == pytest.approx(np.log(4.0))        # the free entry keeps its key: 4 > 1


def test_the_cases_do_what_they_are_built_for():
    for bc in BC.cases():
        b = BC.batch(bc, "nb")
        assert b.B == len(bc.M) and (b.M >= 0).all() and ((b.origin >= 0) & (b.origin <= 22)).all()
        for r, (row, org) in enumerate(zip(bc.case.rows, bc.origin)):
            assert len(row) == len(org)
            for d, o in zip(row, org):                   # the origin is allowed at its slot: an exhausted row can draw
                assert o == FREE or DC.bits(d.allow)[o], (bc.name, r, o)
        for mode in bc.case.modes:
            x = _expect(bc, mode)
            # budget_walk on the tokens the expectation writes gives the same flags and counts
            perms = x.perms if bc.case.family == "confident" else [list(range(len(r))) for r in bc.case.rows]
            order, written = b.order.copy(), np.zeros_like(b.order)
            for r, perm in enumerate(perms):
                for t, e in enumerate(perm):
                    order[r, t], written[r, t] = b.order[r, e], x.draws[r][t][0]
            ex, n = budget_walk(written, b.origin, order, b.T, b.M)
            assert n.tolist() == x.n, (bc.name, mode)
            for r in range(b.B):
                assert ex[r, :b.T[r]].tolist() == x.exhausted[r], (bc.name, mode, r)
            if mode != "score":
                assert all(c <= m for c, m in zip(x.n, bc.M)), (bc.name, mode)           # a sampler never overruns its budget
            if mode == "record" and bc.exhausted_at is not None:
                assert [list(np.flatnonzero(f)) for f in x.exhausted] == bc.exhausted_at, (bc.name, x.exhausted)
    # the draw case: rows with T = 6 and M = 2 whose exhaustion falls at positions 4 and 2; scoring overruns M in row 0
    bc = BC.case("budget_draw")
    rec, sc = BC.expect_draws(bc, "record"), BC.expect_draws(bc, "score")
    assert [len(r) for r in bc.case.rows] == [6, 6, 3, 0] and bc.M == [2, 2, 0, 1]
    assert [t for t, _ in rec.draws[0]] == [19, 5, 1, 2, 11, 1] and [t for t, _ in rec.draws[1]] == [7, 9, 18, 12, 4, 21]
    assert [t for t, _ in rec.draws[2]] == [6, 5, 11] and rec.n == [2, 2, 0, 0]
    assert all(lp == 0.0 for row, fl in zip(rec.draws, rec.exhausted) for (_, lp), f in zip(row, fl) if f)
    assert sc.n == [3, 2, 0, 0] and np.isneginf(sc.draws[0][5][1]) and sc.draws[0][4][1] == 0.0 and np.isfinite(sc.draws[1][2][1])
    # the confident case: the exhausted row's origin-bearing entries first, in list order, ahead of the free one
    bc = BC.case("budget_confident")
    x = BC.expect_confident(bc, "record")
    assert x.perms == [[1, 0, 3, 4, 2], [1, 0, 2]] and x.n == [1, 1]
    assert [t for t, _ in x.draws[0]] == [5, 0, 10, 12, 8]
    nobudget = [DC.confident_orders(DC.log_keys(bc.case, row), 1)[0] for row in bc.case.rows]
    assert nobudget == [[1, 3, 0, 4, 2], [1, 0, 2]]      # what the same lists give without a budget: the test can fail
    s = BC.expect_confident(bc, "score")
    assert s.perms == x.perms and s.n == [2, 1] and np.isneginf(s.draws[0][2][1]) and s.draws[0][1][1] == 0.0
