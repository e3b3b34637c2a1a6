"""The case table of tests/draw_cases.py is DECIDED: no GPU.  For every draw of every case the quantities of the header are recomputed in
float64 and in a numpy float32 emulation of the header's formulas (`before` accumulated in ascending token index, one fp32 add for a beam
candidate), and every comparison the expected result depends on is one of two kinds:
  * an exact equality of bit-identical operands -- a tie the case builds on purpose, decided by the header's tie rule; or
  * a comparison with a relative margin of at least 1e-4 (beam candidates: 1e-3 absolute), two orders of magnitude above the error of an
    fp32 evaluation, so that no device arithmetic within the header's formulas can fall on the other side.
Comparisons on g itself (ranks, the greedy argmax) have exactly known operands and are always decided.  The float64 and the float32
evaluation must agree on every token, keep-set, order and selection, the number of undecided draws is ZERO -- which is why
tests/test_gpu_draw_exact.py has no near-tie exemption -- and every rule of the list is exercised by a case that carries its tag."""
import numpy as np
import pytest

import draw_cases as DC
from hudiff_amd.guide import N_DRAW, Truncation, beam_select, truncation_keep

F32 = np.float32
MARGIN = 1e-4
BEAM_GAP = 1e-3


def _sum32(x):
    s = F32(0)
    for v in x:
        s = F32(s + F32(v))
    return s


def emulate32(g, tr, q, greedy):
    """The header's formulas in fp32: -> dict(e, esum, before, keep, esum2, lp [22], token)."""
    g = np.asarray(g, F32)
    allowed = g > -np.inf
    mx = g.max()
    with np.errstate(under="ignore", invalid="ignore"):
        e = np.where(allowed, np.exp((g - mx).astype(F32)).astype(F32), F32(0))
    esum = _sum32(e)
    idx = np.arange(N_DRAW)
    rank, before = np.zeros(N_DRAW, int), np.zeros(N_DRAW, F32)
    for j in idx:
        ahead = allowed & ((g > g[j]) | ((g == g[j]) & (idx < j)))
        rank[j] = ahead.sum()
        before[j] = _sum32(e[ahead])                     # (boolean indexing keeps ascending token index)
    keep = allowed.copy()
    if tr is not None and not tr.neutral:
        if 0 < tr.top_k < N_DRAW:
            keep &= rank < tr.top_k
        if tr.top_p < 1.0:
            keep &= before < F32(F32(tr.top_p) * esum)
        if tr.min_p > 0.0:
            keep &= e >= F32(tr.min_p)
        keep |= allowed & (rank == 0)
    esum2 = _sum32(np.where(keep, e, F32(0)))
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        lp = np.where(keep, ((g - mx).astype(F32) - np.log(esum2)).astype(F32), F32(-np.inf))
        ratio = np.where(keep, g if greedy else (e / esum2).astype(F32) / np.asarray(q, F32), F32(-np.inf))
    return dict(e=e, esum=esum, before=before, rank=rank, keep=keep, esum2=esum2, lp=lp, token=int(np.argmax(ratio)), mx=mx, allowed=allowed)


def undecided(case, d, q, mode):
    """Why this draw is not decided; [] when it is.  Also asserts that float32 and float64 agree on the keep-set and the token."""
    g = DC.g_of(case, d)
    tr = case.truncation
    greedy = case.temperature == 0
    em = emulate32(g, tr, q, greedy)
    tok, lp64, keep64 = DC.expect_entry(case, d, q, mode)
    why = []
    assert np.array_equal(em["keep"], keep64), (case.name, em["keep"], keep64)
    al = em["allowed"]
    g64 = np.asarray(g, np.float64)
    e64 = np.where(al, np.exp(g64 - g64.max()), 0.0)
    if tr is not None and not tr.neutral:
        if tr.top_p < 1.0:
            thr64, thr32 = tr.top_p * e64.sum(), F32(F32(tr.top_p) * em["esum"])
            idx = np.arange(N_DRAW)
            for j in np.flatnonzero(al):
                ahead = al & ((g64 > g64[j]) | ((g64 == g64[j]) & (idx < j)))
                b64 = e64[ahead].sum()
                tie = b64 == thr64 and em["before"][j] == thr32 and float(thr32) == thr64 and float(em["before"][j]) == b64
                if not tie and abs(b64 - thr64) < MARGIN * thr64:
                    why.append(("top_p", int(j), b64, thr64))
        if tr.min_p > 0.0:
            for j in np.flatnonzero(al):
                tie = e64[j] == 1.0 and em["e"][j] == 1.0 and tr.min_p == 1.0
                if not tie and abs(e64[j] - tr.min_p) < MARGIN * tr.min_p:
                    why.append(("min_p", int(j), e64[j]))
    if mode != "score":
        assert em["token"] == tok, (case.name, em["token"], tok)
        if not greedy:
            lpk = np.where(keep64, g64 - g64.max(), -np.inf)
            with np.errstate(divide="ignore"):
                r = np.where(keep64, np.exp(lpk) / np.asarray(q, np.float64), -np.inf)
            for j in np.flatnonzero(keep64):
                if j == tok:
                    continue
                tie = g[j] == g[tok] and F32(q[j]) == F32(q[tok])
                if tie:
                    assert j > tok, (case.name, j, tok)          # the designed tie went to the lower index
                elif not r[tok] - r[j] >= MARGIN * r[tok]:
                    why.append(("ratio", int(j), r[tok], r[j]))
    else:
        assert np.isneginf(lp64) == (not keep64[tok])
        if np.isfinite(lp64):
            assert abs(float(em["lp"][tok]) - lp64) <= DC.logp_bound(lp64), (case.name, em["lp"][tok], lp64)
    return why


def _modes(case):
    return [m for m in case.modes if m != "beam"]


def test_every_draw_is_decided():
    n = 0
    bad = []
    for case in DC.cases():
        if case.error or case.family == "beam":
            continue
        for mode in _modes(case):
            if case.family == "draw":
                pairs = [(d, DC.noise_of(d)) for row in case.rows for d in row]
            else:
                perms = DC.expect_confident(case, mode)[0]
                pairs = [(row[e], DC.noise_of(row[t])) for row, perm in zip(case.rows, perms) for t, e in enumerate(perm)]
            for d, q in pairs:
                n += 1
                why = undecided(case, d, q, mode)
                if why:
                    bad.append((case.name, mode, why))
    print(f"{n} draws, {len(bad)} undecided")
    assert n > 200 and not bad, bad


def test_confident_keys_are_decided():
    pairs = 0
    for case in DC.cases():
        if case.family != "confident":
            continue
        for row in case.rows:
            k64 = np.exp(DC.log_keys(case, row))
            k32 = np.array([emulate32(DC.g_of(case, d), case.truncation, DC.noise_of(d), False)["esum2"] for d in row], F32)
            for i in range(len(row)):
                for u in range(i):
                    pairs += 1
                    if k32[i] == k32[u]:
                        assert k64[i] == k64[u], (case.name, i, u)                   # a designed tie: by list position
                    else:
                        assert abs(k64[i] - k64[u]) >= MARGIN * max(k64[i], k64[u]), (case.name, i, u, k64[i], k64[u])
            o64 = DC.confident_orders(list(k64), case.K)
            assert o64 == DC.confident_orders([float(x) for x in k32], case.K) == DC.confident_orders(DC.log_keys(case, row), case.K)
    assert pairs > 50
    # the keys the issue names: exactly 1, 2, 3, 4, and equal keys go by list position
    c = DC.case("confident_K2")
    assert np.array_equal(np.exp(DC.log_keys(c, c.rows[0])).round(12), [3, 1, 2, 4, 2, 1, 3])
    assert DC.confident_orders(DC.log_keys(c, c.rows[0]), 2)[0] == [1, 5, 2, 4, 0, 6, 3]
    assert [len(r) for r in c.rows] == [7, 5, 0, 4]
    # stable partition: after the first forward of K = 2 the five positions not chosen stand in their previous relative order
    assert DC.confident_orders(DC.log_keys(c, c.rows[0]), 2)[1][0] == [1, 5, 0, 2, 3, 4, 6]
    # the truncation changes the order
    on, off = DC.case("confident_trunc"), DC.case("confident_trunc_off")
    assert [DC.confident_orders(DC.log_keys(on, r), 1)[0] for r in on.rows] != [DC.confident_orders(DC.log_keys(off, r), 1)[0] for r in off.rows]


def _beam32(case, b):
    """The beam in the fp32 emulation: selections and scores per position."""
    W, G = case.W, len(case.rows)
    score = np.where(np.arange(b.B) % W == 0, F32(0), F32(-np.inf)).astype(F32)
    out = []
    for t in range(b.Tmax):
        sel = {}
        for g in range(G):
            if t >= len(case.rows[g]):
                continue
            d, r0 = case.rows[g][t], g * W
            lp = emulate32(DC.g_of(case, d), case.truncation, DC.noise_of(d), False)["lp"]
            cand = (score[r0:r0 + W, None] + lp[None, :]).astype(F32)
            w, j, v = beam_select(cand, W)
            sel[g] = (w, j, cand)
            score[r0:r0 + W] = v
        out.append(sel)
    return out


def test_beam_candidates_are_decided():
    seen = set()
    for case in DC.cases():
        if case.family != "beam":
            continue
        b = DC.batch(case, "nb")
        steps, em = DC.expect_beam(case, b), _beam32(case, b)
        for t, (st, sel) in enumerate(zip(steps, em)):
            for g, (w, j, cand32) in sel.items():
                r0 = g * case.W
                assert np.array_equal(st["parent"][r0:r0 + case.W], w) and np.array_equal(st["token"][r0:r0 + case.W], j), (case.name, t, g)
                c64 = st["cand"][r0:r0 + case.W].reshape(-1)
                c32 = cand32.reshape(-1)
                assert np.array_equal(np.isfinite(c64), np.isfinite(c32))
                fin = np.flatnonzero(np.isfinite(c64))
                for a in fin:
                    for u in fin[fin < a]:
                        if c32[a] == c32[u]:
                            assert c64[a] == c64[u], (case.name, t, g, a, u)         # bit-identical by symmetry
                        else:
                            assert abs(c64[a] - c64[u]) >= BEAM_GAP and abs(float(c32[a]) - float(c32[u])) >= BEAM_GAP, (case.name, t, g, a, u)
                chosen = w * N_DRAW + j
                live = [c for c in chosen if np.isfinite(c64[c])]
                # which rules this step decided
                if any(c32[c] == c32[u] and c // N_DRAW == u // N_DRAW and u not in chosen for c in live for u in fin):
                    seen.add("in_row_lost")
                if any(c32[a] == c32[u] and a // N_DRAW == u // N_DRAW for a in live for u in live if a != u):
                    seen.add("in_row")
                if any(c32[a] == c32[u] and a // N_DRAW != u // N_DRAW for a in live for u in fin if a != u):
                    seen.add("across_rows")
                if len(live) < case.W:
                    seen.add("dead")
                    dead = [c for c in chosen if not np.isfinite(c64[c])]
                    assert dead == sorted(np.flatnonzero(~np.isfinite(c64)).tolist())[:len(dead)]        # the -inf candidates in (w, j) order
    assert seen >= {"in_row", "across_rows", "dead"}, seen


def test_the_cases_do_what_their_names_say():
    tags = {t for c in DC.cases() for t in c.tags}
    assert tags == set(DC.RULES), (tags ^ set(DC.RULES))
    for c in DC.cases():
        b = DC.batch(c, "ab")
        assert b.B <= 8 and b.Tmax <= 8, c.name
        for row in c.rows:
            for d in row:
                assert DC.bits(d.allow)[DC.target_of(d)], c.name
    # top_p = m / n on n tied tokens keeps exactly m; top_k inside a tie keeps the lower indices; min_p = 1 keeps the whole tie
    for name, m_of in (("topp_1_2", {2: 1, 4: 2, 8: 4}), ("topp_3_4", {4: 3, 8: 6}), ("topp_3_8", {8: 3})):
        c = DC.case(name)
        for row in c.rows:
            for d in row:
                g = DC.g_of(c, d)
                top = np.flatnonzero(g == g.max())
                keep = truncation_keep(g, c.truncation)
                assert np.array_equal(np.flatnonzero(keep), top[:m_of[len(top)]]), name
    c = DC.case("trunc_topk3/pruned")
    assert np.array_equal(np.flatnonzero(truncation_keep(DC.g_of(c, c.rows[0][0]), c.truncation)), [1, 2, 5])
    c = DC.case("minp_1")
    assert np.array_equal(np.flatnonzero(truncation_keep(DC.g_of(c, c.rows[0][0]), c.truncation)), [1, 2, 5, 19])
    c = DC.case("topk_21")
    assert np.array_equal(np.flatnonzero(~truncation_keep(DC.g_of(c, c.rows[0][0]), c.truncation)), [21])
    c = DC.case("topp_tiny")
    assert np.array_equal(np.flatnonzero(truncation_keep(DC.g_of(c, c.rows[0][0]), c.truncation)), [1])
    a, b = DC.case("minp_036"), DC.case("minp_037")
    assert truncation_keep(DC.g_of(a, a.rows[0][0]), a.truncation).sum() == 2 and truncation_keep(DC.g_of(b, b.rows[0][0]), b.truncation).sum() == 1
    # all three cuts: each one alone is the binding one in some draw of the session
    c = DC.case("three_cuts")
    tr = c.truncation
    singles = {"top_k": Truncation(top_k=tr.top_k), "top_p": Truncation(top_p=tr.top_p), "min_p": Truncation(min_p=tr.min_p)}
    binding = set()
    for row in c.rows:
        for d in row:
            g = DC.g_of(c, d)
            full = truncation_keep(g, tr).sum()
            alone = {k: truncation_keep(g, v).sum() for k, v in singles.items()}
            tight = [k for k, v in alone.items() if v == full]
            assert tight and full < (g > -np.inf).sum()
            if len(tight) == 1:
                binding.add(tight[0])
    assert binding == {"top_k", "top_p", "min_p"}, binding
    # underflow: e is exactly 0 in fp32, the winner's logp exactly 0, the scored target's finite
    c = DC.case("underflow")
    for d in c.rows[0]:
        em = emulate32(DC.g_of(c, d), None, DC.noise_of(d), False)
        assert (em["e"] > 0).sum() == 1 and em["esum"] == 1.0
        assert DC.expect_entry(c, d, DC.noise_of(d), "record")[1] == 0.0
        lp = DC.expect_entry(c, d, DC.noise_of(d), "score")[1]
        assert np.isfinite(lp) and lp <= -110.0
    # magnitude: |g| = 1e30 with finite differences; the overflow case really overflows, from finite operands
    c = DC.case("magnitude")
    g = DC.g_of(c, c.rows[0][0])
    assert g.max() == F32(1e30) and np.isfinite(g).all() and np.isfinite(DC.expect_entry(c, c.rows[0][0], DC.noise_of(c.rows[0][0]), "score")[1])
    c = DC.case("guided_overflow")
    d = c.rows[0][1]
    assert np.isfinite(d.bias).all() and np.isfinite(c.P).all() and np.isposinf(DC.g_of(c, d)[7]) and np.isfinite(DC.g_of(c, c.rows[0][0])).all()
    # greedy: the token is the first maximum of g and its logp the temperature-1 one
    c = DC.case("greedy")
    assert [t for t, _ in DC.expect_draws(c, "record")[0]] == [1, 5, 3] and [t for t, _ in DC.expect_draws(c, "record")[1]] == [19, 1]
    # the all-equal distribution: -log n, argmin q
    c = DC.case("plain_all_equal")
    (t0, l0), (t1, l1) = DC.expect_draws(c, "record")[0]
    assert (t0, t1) == (int(np.argmin(c.rows[0][0].q)), 4) == (9, 4) and l0 == l1 == pytest.approx(-np.log(22), abs=1e-15)


def test_multiples_of_a_quarter_are_exact():
    """P + bias is exact in fp32 wherever a case builds a tie at a power-of-two temperature."""
    for c in DC.cases():
        if c.temperature not in (0.0, 0.5, 1.0) or c.name in ("magnitude", "guided_overflow"):
            continue
        for row in c.rows:
            for d in row:
                if d.bias is not None:
                    exact = np.asarray(c.P, np.float64) + np.asarray(d.bias, np.float64)
                    assert np.array_equal((c.P + d.bias).astype(np.float64), exact), c.name
