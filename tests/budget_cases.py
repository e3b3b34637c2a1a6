"""Case table for the mutation budget on EXACTLY known logits (include/hudiff_hip.h "mutation budget"), in the manner of
tests/draw_cases.py, whose zeroed-decoder trick, table `main`, `level` / `qv` builders and `logp_bound` it uses.  A plain helper module:
tests/test_budget_host.py proves on the CPU that every case is decided, tests/test_gpu_budget.py runs the cases on the device.

A budget case is a draw_cases.Case plus, per row, the budget M and, per entry, the origin token of the entry's slot (22 = free).  The
expected result walks every row position by position with rules 1 and 3: at an exhausted position the entry's allowed set is replaced
by {o} and the float64 definitions of draw_cases (guided_log_probs on the exactly known fp32 g) give token and logp; the count follows
the token written (the target, when scoring).  With a zeroed decoder the key of a confident session depends on its guide entry and on
the count alone, so its whole realised order is known before it runs.
"""
from dataclasses import dataclass, replace
from types import SimpleNamespace

import numpy as np

import draw_cases as DC
from draw_cases import Draw, level, qv
from hudiff_amd.guide import FREE, Truncation

P = DC.P_MAIN


@dataclass
class BCase:
    case: DC.Case
    origin: list                   # origin[r][e]: origin token at the slot of entry e of row r (FREE = 22: no origin)
    M: list                        # M[r]: the row's budget
    exhausted_at: list = None      # record / sample mode: positions at which row r is exhausted (what the case is built for)

    @property
    def name(self):
        return self.case.name


def _rows():
    """Four rows, two lanes of two.  Rows 0 and 1: T = 6, M = 2; exhaustion falls at position 4 (row 0: behind a free slot) and at
    position 2 (row 1).  Row 2: M = 0.  Row 3: T = 0."""
    N = Draw
    r0 = [N(q=qv((19,)), target=19),                     # origin 19: drawn            n = 0   | scored 19           n = 0
          N(q=qv((5,)), target=5),                       # origin 2: 5 drawn           n = 1   | scored 5            n = 1
          N(q=qv((1,)), target=2),                       # origin 5: 1 drawn           n = 2   | scored 2            n = 2
          N(q=qv((2,)), target=2),                       # free: 2 drawn, not counted          | free
          N(q=qv((19,)), target=11),                     # origin 11: exhausted, 11, logp 0    | exhausted, 11 = o: 0
          N(q=qv((5,)), target=7)]                       # origin 1: exhausted, 1, logp 0      | exhausted, 7 != o: -inf, n = 3 (overrun)
    o0 = [19, 2, 5, FREE, 11, 1]
    r1 = [level(P, {3: 2.0, 7: 2.0, 10: 2.0}, qv((7,)), 3),          # origin 3: 7 drawn     n = 1   | scored 3   n = 0
          level(P, {8: 1.0, 9: 1.0}, qv((9,)), 9),                   # origin 8: 9 drawn     n = 2   | scored 9   n = 1
          level(P, {0: 1.0, 6: 1.0, 18: 0.5}, qv((0,)), 18),         # origin 18: exhausted, 18      | not exhausted: 18 scored, finite
          N(q=qv((12,)), target=12),                                 # free: 12 drawn                | free
          N(q=qv((1,)), target=10),                                  # origin 4: exhausted, 4        | not exhausted: 10 scored  n = 2
          level(P, {20: -1.0, 21: -1.0}, qv((20,)), 21)]             # origin 21: exhausted, 21      | exhausted, 21 = o: 0
    o1 = [3, 8, 18, FREE, 4, 21]
    r2 = [N(q=qv((19,)), target=6), N(q=qv((5,)), target=3), level(P, {11: 2.0, 12: 2.0}, qv((12,)), 11)]
    o2 = [6, FREE, 11]                                   # M = 0: 6, then the free slot draws 5, then 11
    return [r0, r1, r2, []], [o0, o1, o2, []], [2, 2, 0, 1]


def _confident_rows():
    """Row 0, M = 1.  Keys without exhaustion: 3 2 4 2 3 -> entry 1 goes first and its draw (noise of position 0: token 5) is a
    mutation.  From then on every origin-bearing entry has the key exactly 1 and goes in list order -- 0, 3, 4 -- ahead of the free
    entry 2 whose key is 4.  Without a budget the order would be 1 3 0 4 2.  Row 1, M = 5: never exhausted, keys 2 1 3."""
    t2 = lambda js, lvl=2.0: {j: lvl for j in js}
    r0 = [level(P, t2((0, 1, 2)), qv((5,)), 0),          # entry 0: origin 0; scored 0 = o
          level(P, t2((4, 5)), qv((1,)), 5),             # entry 1: origin 4; draws 5 (position 0 meets entry 0's noise); scored 5
          level(P, t2((6, 7, 8, 9)), qv((10,)), 7),      # entry 2: free; drawn last, with the noise of position 4 (token 8)
          level(P, t2((10, 11)), qv((13,)), 11),         # entry 3: origin 10; scored 11 != o: -inf
          level(P, t2((12, 13, 14)), qv((8,)), 12)]      # entry 4: origin 12
    o0 = [0, 4, FREE, 10, 12]
    r1 = [level(P, t2((15, 16)), qv((16,)), 15), level(P, t2((17,)), qv((3,)), 17), level(P, t2((18, 19, 20)), qv((20,)), 19)]
    o1 = [15, 17, 18]
    return [r0, r1], [o0, o1], [1, 5]


_cases = None


def cases():
    global _cases
    if _cases is None:
        rows, origin, M = _rows()
        ex = [[4, 5], [2, 4, 5], [0, 2], []]
        base = DC.Case("budget_draw", (), "draw", rows=rows)
        _cases = [BCase(base, origin, M, ex),
                  BCase(replace(base, name="budget_noprune", prune=False), origin, M, ex),
                  BCase(replace(base, name="budget_greedy", temperature=0.0, modes=("record", "sample")), origin, M),
                  BCase(replace(base, name="budget_topk3", truncation=Truncation(top_k=3)), origin, M),
                  BCase(replace(base, name="budget_temp_half", temperature=0.5), origin, M, ex)]
        rows, origin, M = _confident_rows()
        _cases.append(BCase(DC.Case("budget_confident", (), "confident", rows=rows, K=1, policy="confident"), origin, M))
    return _cases


def case(name):
    return next(c for c in cases() if c.name == name)


def batch(bc, kind):
    """draw_cases.batch plus origin int32 [B, L] (FREE where the case says nothing) and M int32 [B]."""
    b = DC.batch(bc.case, kind)
    origin = np.full((b.B, b.L), FREE, np.int32)
    for r, row in enumerate(bc.origin):
        for e, o in enumerate(row):
            origin[r, b.order[r, e]] = o
    b.origin, b.M = origin, np.array(bc.M, np.int32)
    return b


def forced(d, o):
    """The entry as an exhausted row meets it: the allowed set is the origin alone."""
    return replace(d, allow=1 << int(o))


def _entry(case, d, o, n, M, q, mode):
    """One position: -> (token, float64 logp, exhausted, the entry the draw really met)."""
    ex = o <= 21 and n >= M
    met = forced(d, o) if ex else d
    if mode == "score" and ex and DC.target_of(d) != o:
        return DC.target_of(d), -np.inf, ex, met         # the target is written as always; it has probability 0
    if mode == "score":
        met = replace(met, target=DC.target_of(d))
    tok, lp, _ = DC.expect_entry(case, met, q, mode)
    return tok, lp, ex, met


def expect_draws(bc, mode):
    """A given-order session: per row [(token, logp)], the exhausted flags, the final count, and the entries the draws met."""
    draws, flags, counts, mets = [], [], [], []
    for row, org, M in zip(bc.case.rows, bc.origin, bc.M):
        n, dr, fl, mt = 0, [], [], []
        for d, o in zip(row, org):
            tok, lp, ex, met = _entry(bc.case, d, o, n, M, DC.noise_of(d), mode)
            n += int(o <= 21 and tok != o)
            dr.append((tok, lp)); fl.append(ex); mt.append((met, DC.noise_of(d)))
        draws.append(dr); flags.append(fl); counts.append(n); mets.append(mt)
    return SimpleNamespace(draws=draws, exhausted=flags, n=counts, met=mets)


def key_of(case, d, o, n, M):
    """log of the confident key of an entry as the row stands: exactly log 1 = 0 at an exhausted origin-bearing entry."""
    return DC.log_keys(case, [forced(d, o) if (o <= 21 and n >= M) else d])[0]


def expect_confident(bc, mode):
    """K = 1: forward by forward the remaining entry with the smallest (key, list position) -- keys formed on the allowed set of rule 1
    with the count as it stands -- moves to the front and is drawn with the noise of its POSITION.  -> perms, draws, exhausted, n, met,
    and the keys every forward saw (for the host proof)."""
    assert bc.case.K == 1
    perms, draws, flags, counts, mets, seen = [], [], [], [], [], []
    for row, org, M in zip(bc.case.rows, bc.origin, bc.M):
        lst, n, dr, fl, mt, ks = list(range(len(row))), 0, [], [], [], []
        for t in range(len(row)):
            rem = lst[t:]
            keys = [key_of(bc.case, row[e], org[e], n, M) for e in rem]
            ks.append(keys)
            i = min(range(len(rem)), key=lambda u: (keys[u], u))
            e = rem[i]
            lst = lst[:t] + [e] + rem[:i] + rem[i + 1:]
            q = DC.noise_of(row[t])
            tok, lp, ex, met = _entry(bc.case, row[e], org[e], n, M, q, mode)
            n += int(org[e] <= 21 and tok != org[e])
            dr.append((tok, lp)); fl.append(ex); mt.append((met, q))
        perms.append(lst); draws.append(dr); flags.append(fl); counts.append(n); mets.append(mt); seen.append(ks)
    return SimpleNamespace(perms=perms, draws=draws, exhausted=flags, n=counts, met=mets, keys=seen)
