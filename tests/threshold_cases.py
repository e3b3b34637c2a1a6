"""Exact-logit cases for the confidence threshold (include/hudiff_hip.h "confidence threshold"), on the zeroed-decoder loader of
tests/draw_cases.py: a plain helper module.  tests/test_threshold_host.py proves on the CPU that every case is decided,
tests/test_gpu_threshold.py runs the cases on the device.

With a zeroed decoder the key of a position depends on its guide entry alone, so the count, the order and the forward number of every
position are known before the session runs.  Designed exact keys: 1.0f for a single allowed token (expf(0)), 2.0f for two allowed tokens
with equal values (expf(0) + expf(0)); n tokens tied at the top and nothing else allowed give n exactly.  Every other comparison with
cmax = 1.0f / tau, and between two different keys, has a relative margin of at least 1e-4.
"""
import numpy as np

import draw_cases as DC
from hudiff_amd.guide import Truncation, confidence_cmax, truncation_keep

F32 = np.float32


def rule(keys, K, cmax):
    """Steps 2 to 4 of the definition in plain Python, on one row's remaining keys (any floats; not finite and positive = +inf):
    -> (chosen positions in rank order, cnt, the whole permutation)."""
    c = [float(x) if (x == x and 0.0 < x < float("inf")) else float("inf") for x in keys]
    N = len(c)
    q = sum(1 for x in c if x != float("inf") and x <= float(cmax))
    cnt = min(K, N, max(1, q))
    ranked = sorted(range(N), key=lambda i: (c[i], i))
    chosen = ranked[:cnt]
    return chosen, cnt, chosen + [i for i in range(N) if i not in chosen]


def key_of(case, d):
    """The key of an entry in float64, straight from the exactly known g (no logarithm in between: a designed 2.0 stays 2.0)."""
    g = DC.g_of(case, d).astype(np.float64)
    keep = truncation_keep(g, case.truncation)
    with np.errstate(invalid="ignore"):
        return float(np.exp(g[keep] - g.max()).sum())


def walk(keys, K, cmax):
    """A whole row: -> (perm: the entry at every position, fwd: the forward that drew every position, counts: per forward)."""
    lst, n, f, fwd, counts = list(range(len(keys))), 0, 0, [], []
    while n < len(keys):
        rem = lst[n:]
        _, cnt, perm = rule([keys[e] for e in rem], K, cmax)
        lst = lst[:n] + [rem[i] for i in perm]
        fwd += [f] * cnt
        counts.append(cnt)
        n += cnt
        f += 1
    return lst, fwd, counts


def _cases():
    P = DC.P_MAIN
    one = lambda j: DC.level(P, {j: 1.0})                                       # key 1.0
    pair = lambda a, b: DC.level(P, {a: 2.0, b: 2.0})                           # key 2.0
    three = lambda: DC.level(P, {3: 1.5, 7: 1.5, 10: 1.5})                      # key 3.0
    four = lambda: DC.level(P, {0: 0.5, 4: 0.5, 13: 0.5, 21: 0.5})              # key 4.0
    full = lambda: DC.Draw()                                                    # the table itself: 4 maxima and a tail, key about 7.9
    mk = lambda name, rows, K, tau, **kw: (DC.Case(name, (), "confident", rows=rows, K=K, policy="confident", **kw), tau)
    out = []
    # singletons at tau = 1 fill first, K per forward (more qualifiers than K), then one slot per forward; a row shorter than K; T = 0
    out.append(mk("singletons_tau1", [[pair(2, 9), one(4), full(), one(11), one(0), three(), one(20), one(6)],
                                      [one(5)], [], [full(), one(3), one(8)]], 2, 1.0))
    # an exact tie c == cmax qualifies; one part in 5000 above it does not; rows with N < K
    rows = [[pair(1, 2), three(), pair(5, 19), one(7), pair(11, 12)], [one(3), one(14)], [], [one(0), pair(8, 9), one(16)]]
    out.append(mk("pairs_tau05", rows, 4, 0.5))
    out.append(mk("pairs_tau05001", rows, 4, 0.5001))
    # none qualifying: one slot per forward, the surest first, whatever the cap
    out.append(mk("none_qualifying", [[three(), four(), pair(6, 18), full()], [four(), three()]], 3, 0.9))
    # top_k = 1 makes every key 1.0: everything qualifies at tau = 1, K per forward in list order (token 1, the first of the table's
    # maxima, is the one kept: the target a scoring session forces)
    out.append(mk("topk1_all_ones", [[DC.Draw(target=1) for _ in range(5)], [DC.Draw(target=1) for _ in range(2)]], 2, 1.0, guided=False,
                  truncation=Truncation(top_k=1)))
    return out


CASES = {c.name: (c, tau) for c, tau in _cases()}


def expect(name, mode="record"):
    """-> (case, tau, perms [B], fwd [B], counts [B], draws [B][t] = (token, float64 logp)) of a case."""
    case, tau = CASES[name]
    cmax = float(confidence_cmax(tau))
    perms, fwds, counts, draws = [], [], [], []
    for row in case.rows:
        perm, fwd, cn = walk([key_of(case, d) for d in row], case.K, cmax)
        perms.append(perm); fwds.append(fwd); counts.append(cn)
        draws.append([DC.expect_entry(case, row[e], DC.noise_of(row[t]), mode)[:2] for t, e in enumerate(perm)])
    return case, tau, perms, fwds, counts, draws
