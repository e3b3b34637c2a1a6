"""Case tables for the draw stage on EXACTLY known logits, and what the header says must come out (include/hudiff_hip.h "guided
sampling", "truncated sampling", "slot policy", "beam search").  A plain helper module: tests/test_draw_cases_host.py proves on the
CPU that every case is decided, tests/test_gpu_draw_exact.py runs the cases on the device.

The trick.  The micro model is loaded with ``decoder.weight = 0`` and ``decoder.bias[0:22] = P``, a fixed pattern of multiples of 0.25
with ties and gaps.  Every dot product of the decoder is then +-0 and the raw logit of token j is exactly P_j, in every row, at every
slot, in every forward and on every route; the rest of the network still runs, so rows, slots, lanes and buffers are indexed as
always -- they just cannot move the values.  The guided value g_j = (P_j + bias[b, s, j]) / temperature is known to the test bit for
bit whenever P + bias is exact in fp32 (multiples of 0.25 of moderate size) and the temperature is a power of two; for the other
temperatures g is one fp32 add and one correctly rounded fp32 division, formed here in numpy float32, and no tie is built between
different numerators.  The draw stage becomes a pure function of (allow, bias, temperature, truncation, q_noise, K, policy, W): ties
stand exactly where a case puts them, thresholds are hit exactly, everything else is kept far from one, and NO draw needs a near-tie
exemption.

A case is a list of rows, a row a list of ``Draw`` entries (one per order position): the allowed set and the bias of the slot, the
noise of the POSITION, and the target a scoring session forces there.  ``batch`` lays a case out on the real micro-trace tokens,
region and chain; ``expect_draws`` / ``expect_confident`` / ``expect_beam`` apply the float64 definitions of hudiff_amd.guide
(guided_log_probs, truncation_keep, confidence_keys, beam_select) to the exactly known fp32 g.  With a zeroed decoder the key of a
position depends on its guide entry alone, so the whole realised order of a confident session is known before it runs.
"""
import os
from dataclasses import dataclass, field, replace
from types import SimpleNamespace

import numpy as np

from hudiff_amd.guide import ALL_TOKENS, N_DRAW, Truncation, beam_select, confidence_keys, guided_log_probs, truncation_keep

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
TRACE = {"ab": "micro_ab_sample_finetune.npz", "nb": "micro_nb_sample_plain.npz"}
F32 = np.float32
NEG = F32(-np.inf)
FLT_MAX = np.finfo(F32).max

# ---- the decoder tables ------------------------------------------------------------------------------------------------------------------
# main: maxima tied at 1, 2, 5, 19; pairs at 2.0 (11, 12), 0.5 (8, 9), 0.0 (3, 16); a triple at 1.0 (0, 6, 18); gaps of up to 3.
P_MAIN = np.array([1.0, 2.5, 2.5, 0.0, -1.5, 2.5, 1.0, -3.0, 0.5, 0.5, -8.0, 2.0, 2.0, -0.25, 1.75, -2.0, 0.0, -5.0, 1.0, 2.5, -1.0, -4.0], F32)
P_CONST = np.full(N_DRAW, 1.25, F32)                     # the all-equal distribution
P_HUGE = P_MAIN.copy()
P_HUGE[7] = F32(2.0 ** 104)                              # one ulp of FLT_MAX: P_7 + FLT_MAX rounds to +inf (a finite bias that overflows)
TABLES = {"main": P_MAIN, "const": P_CONST, "huge": P_HUGE}
MASK_LOGIT = -2.0                                        # decoder.bias[22]: the <msk> token, outside the draw


def decoder_state(sd, table):
    """The micro state dict with the decoder replaced: weight 0, bias[0:22] = the table."""
    sd = dict(sd)
    sd["decoder.weight"] = np.zeros_like(np.asarray(sd["decoder.weight"], F32))
    b = np.full(sd["decoder.bias"].shape, MASK_LOGIT, F32)
    b[:N_DRAW] = TABLES[table]
    sd["decoder.bias"] = b
    return sd


# ---- cases -------------------------------------------------------------------------------------------------------------------------------
@dataclass
class Draw:
    allow: int = ALL_TOKENS
    bias: np.ndarray = None        # float32 [22]; None = zeros
    q: np.ndarray = None           # float32 [22], the noise of the POSITION this entry stands at; None = ones
    target: int = None             # what a scoring session forces here; None = the lowest allowed token


@dataclass
class Case:
    name: str
    tags: tuple
    family: str                    # "draw" | "confident" | "beam"
    rows: list                     # rows[b] = [Draw, ...] (beam: one list per GROUP)
    table: str = "main"
    guided: bool = True            # False: no guide is set (every Draw must then be neutral)
    with_bias: bool = True         # False: the guide carries allowed sets only
    temperature: float = 1.0
    truncation: Truncation = None
    K: int = 1
    prune: bool = True
    policy: str = "given"
    W: int = 0
    modes: tuple = ("record", "sample", "score")
    error: str = None              # "numeric": the session must end with HD_ERR_NUMERIC
    extra: dict = field(default_factory=dict)

    @property
    def P(self):
        return TABLES[self.table]


def mask(js):
    m = 0
    for j in js:
        m |= 1 << int(j)
    return m


def bits(allow):
    return ((int(allow) >> np.arange(N_DRAW)) & 1).astype(bool)


def qv(low=(), lo=0.5, hi=8.0):
    """Noise that favours the tokens `low` sixteen-fold: far from every tie that is not built on purpose."""
    q = np.full(N_DRAW, hi, F32)
    q[list(low)] = lo
    return q


def level(P, levels, q=None, target=None):
    """Exactly the tokens of `levels` = {token: value} are allowed and P_j + bias_j == value, exactly (checked)."""
    bias = np.zeros(N_DRAW, F32)
    for j, v in levels.items():
        bias[j] = F32(v) - P[j]
        assert F32(P[j] + bias[j]) == F32(v) and float(bias[j]) == float(v) - float(P[j]), (j, v)
    return Draw(mask(levels), bias, q, target)


def g_of(case, d):
    """The values the draw forms at an entry, as the device forms them: one fp32 add, one fp32 division, -inf where not allowed."""
    with np.errstate(over="ignore"):
        z = case.P if d.bias is None else (case.P + np.asarray(d.bias, F32)).astype(F32)
        g = (z / (F32(1.0) if case.temperature == 0 else F32(case.temperature))).astype(F32)
    return np.where(bits(d.allow), g, NEG)


def target_of(d):
    return int(np.flatnonzero(bits(d.allow))[0]) if d.target is None else int(d.target)


def noise_of(d):
    return np.ones(N_DRAW, F32) if d.q is None else np.asarray(d.q, F32)


def forms(case):
    """The three ways a given-order draw is launched: on the compact rows of the pruned tail, on the full hidden buffer at K = 1, and
    as a block of K > 1 workgroups per row."""
    kb = max(2, max(len(r) for r in case.rows))
    return [replace(case, name=case.name + "/pruned", tags=case.tags + ("argmax_k1_pruned",)),
            replace(case, name=case.name + "/noprune", prune=False, tags=case.tags + ("argmax_k1_noprune",)),
            replace(case, name=case.name + f"/K{kb}", K=kb, tags=case.tags + ("argmax_block",))]


def _draw_cases():
    P, out = P_MAIN, []
    N = Draw
    # plain kernels: the ties of the table itself, decided by which tokens share the small noise
    plain = Case("plain_argmax", ("argmax_tie_plain", "argmax_control_higher_wins"), "draw", guided=False, rows=[
        [N(q=qv((1, 2, 5, 19)), target=2), N(q=qv((5, 19)), target=19), N(q=qv((11, 12)), target=12)],
        [N(q=qv((2, 19)), target=10), N(q=qv((19,)), target=1), N(q=qv((8, 9)), target=9)],
        [N(q=qv((12,)), target=5), N(q=qv((1, 5)), target=17)],
        [N(q=qv((9,)), target=0), N(q=qv((2, 5)), target=21), N(q=qv((6, 18)), target=18)]])
    out += forms(plain)
    qa = (1.0 + ((7 * np.arange(N_DRAW) + 3) % N_DRAW) * 0.25).astype(F32)      # a permutation: one smallest entry (token 9)
    qb = qa.copy()
    qb[[4, 13]] = 0.5                                                           # the smallest value twice: the lower index
    out.append(Case("plain_all_equal", ("argmax_all_equal",), "draw", table="const", guided=False,
                    rows=[[N(q=qa, target=21), N(q=qb, target=0)], [N(q=qb[::-1].copy(), target=7)]]))
    five = mask((3, 8, 9, 14, 20))
    out.append(Case("guided_all_equal", ("argmax_all_equal",), "draw", table="const", with_bias=False,
                    rows=[[Draw(five, q=qa, target=14), Draw(five, q=qv((9, 20)), target=20)], [Draw(mask((21,)), q=qa)]]))
    # guided kernels at temperature 1/2 (g = 2 (P + bias), exact): ties built by the bias
    guided = Case("guided_argmax", ("argmax_tie_guided", "argmax_control_higher_wins", "score_target_in_tie", "score_singleton"), "draw",
                  temperature=0.5, rows=[
        [level(P, {3: 2.0, 7: 2.0, 10: 2.0}, qv((7, 10)), 10), Draw(bias=_b({4: 7.5, 15: 8.0}), target=15),
         Draw(bias=_b({4: 7.5, 15: 8.0}), q=qv((15,)), target=4)],
        [Draw(mask((13,)), q=qv((0,)), target=13), level(P, {20: -1.0, 21: -1.0}, None, 21), level(P, {0: 1.0, 6: 1.0, 18: 0.5}, qv((6, 18)), 18)],
        [level(P, {11: 3.0, 2: 3.0, 16: 3.0, 9: 3.0}, qv((9, 16)), 16)]])
    out += forms(guided)
    # truncating kernels without a guide: top_k = 3 cuts INSIDE the tie 1, 2, 5, 19 -- token 19 goes
    tk3 = Case("trunc_topk3", ("argmax_tie_trunc", "topk_cut_in_tie", "score_target_in_tie", "score_target_removed"), "draw", guided=False,
               truncation=Truncation(top_k=3), rows=[
        [N(q=qv((5, 19)), target=2), N(q=qv((19,)), target=19), N(q=qv((1, 2, 5, 19)), target=1)],
        [N(q=qv((2, 5)), target=5), N(q=qv((11, 12)), target=11)]])
    out += forms(tk3)
    out.append(Case("trunc_guided_topk2", ("argmax_tie_trunc", "topk_cut_in_tie", "score_target_removed", "score_singleton"), "draw",
                    truncation=Truncation(top_k=2), rows=[
        [level(P, {3: 1.0, 7: 1.0, 10: 1.0, 16: 1.0}, qv((10, 16)), 7), level(P, {3: 1.0, 7: 1.0, 10: 1.0, 16: 1.0}, qv((7, 16)), 10)],
        [Draw(mask((13,)), q=qv((2,)), target=13), level(P, {21: 0.5, 20: 0.5, 19: 0.5}, None, 21)]]))
    # greedy: no noise is read (the noise handed in favours other tokens); log-probabilities are those at temperature 1
    grows = [[Draw(q=qv((19,))), Draw(mask((5, 19, 11)), q=qv((11,))), level(P, {7: 3.0, 3: 3.0, 1: 2.5}, qv((1,)))],
             [Draw(bias=_b({19: 1.0}), q=qv((1,))), Draw(bias=_b({12: 0.5, 14: 0.75}), q=qv((0,)))]]
    out.append(Case("greedy", ("greedy_tie", "greedy_logp_temp1", "argmax_control_higher_wins"), "draw", temperature=0.0, rows=grows,
                    modes=("record", "sample")))
    out.append(Case("greedy_topk2", ("greedy_tie", "greedy_logp_temp1"), "draw", temperature=0.0, rows=grows, truncation=Truncation(top_k=2),
                    modes=("record", "sample")))
    # top_k at its ends
    out.append(Case("topk_1", ("topk_1",), "draw", guided=False, truncation=Truncation(top_k=1),
                    rows=[[N(q=qv((19,)), target=1), N(q=qv((2, 5)), target=2)], [N(q=qv((10,)), target=1)]]))
    flat = {j: 2.0 for j in range(N_DRAW)}
    out.append(Case("topk_21", ("topk_21",), "draw", truncation=Truncation(top_k=21),
                    rows=[[level(P, flat, qv((21,)), 21), level(P, flat, qv((20, 21)), 20)], [level(P, flat, qv((7, 21)), 0)]]))
    # top_p on n tokens tied at the top: every e is exactly 1, esum = n, before = 0, 1, ..., top_p * esum = m exactly: the strict < keeps m
    s2, s4, s8 = (6, 17), (0, 7, 13, 21), (1, 3, 4, 8, 10, 15, 18, 20)

    def tied(s, far=False, q=None, target=None):
        lv = {j: -120.0 for j in range(N_DRAW)} if far else {}
        lv.update({j: 2.0 for j in s})
        return level(P, lv, q, target)
    out.append(Case("topp_1_2", ("topp_exact_n2", "topp_exact_n4", "topp_exact_n8", "topp_far_below", "score_target_removed"), "draw",
                    truncation=Truncation(top_p=0.5), rows=[
        [tied(s2, q=qv((17,)), target=17), tied(s4, q=qv((7, 13)), target=7), tied(s8, q=qv((10,)), target=10)],
        [tied(s8, True, qv((10, 2)), 8), tied(s2, True, qv((17, 0)), 6), tied(s4, True, qv((13,)), 13)]]))
    out.append(Case("topp_3_4", ("topp_exact_n4", "topp_exact_n8", "topp_far_below"), "draw", truncation=Truncation(top_p=0.75), rows=[
        [tied(s4, q=qv((21,)), target=21), tied(s8, q=qv((18, 20)), target=15)],
        [tied(s8, True, qv((18,)), 18), tied(s4, True, qv((13, 21)), 13)]]))
    out.append(Case("topp_3_8", ("topp_exact_n8",), "draw", truncation=Truncation(top_p=0.375),
                    rows=[[tied(s8, q=qv((8,)), target=8), tied(s8, True, qv((4, 8)), 4)]]))
    # the smallest top_p there is (a denormal in fp32): only the rank-0 token stays.  For finite input the comparison itself keeps it
    # (before_0 = 0 < top_p * esum, the product is never 0); the rank-0 RULE decides alone only where esum is NaN (guided_overflow)
    out.append(Case("topp_tiny", ("topp_rank0_only",), "draw", guided=False, truncation=Truncation(top_p=1e-45),
                    rows=[[N(q=qv((2, 19)), target=1), N(q=qv((11,)), target=2)]]))
    # min_p
    out.append(Case("minp_1", ("minp_one_keeps_ties",), "draw", guided=False, truncation=Truncation(min_p=1.0),
                    rows=[[N(q=qv((11,)), target=19), N(q=qv((5, 19)), target=11)], [N(q=qv((19,)), target=5)]]))
    edge = {4: 2.0, 9: 1.0, 16: 0.0}                     # g - mx = 0, -1, -2: e = 1, 0.3679, 0.1353
    for name, mp in (("036", 0.36), ("037", 0.37)):
        out.append(Case("minp_" + name, ("minp_" + name,), "draw", truncation=Truncation(min_p=mp),
                        rows=[[level(P, edge, qv((9,)), 9), level(P, edge, qv((16,)), 4)]]))
    # all three cuts in one session; each is the one that binds in one of the draws (checked by the host test)
    X = {2: 2.0, 5: 1.75, 8: 1.5, 11: 1.25, 14: 1.0, 17: 0.75}
    Y = {0: 2.0, 6: -1.0, 12: -1.25, 18: -1.5}
    Z = {3: 2.0, **{j: -2.25 for j in (4, 7, 9, 10, 13, 15, 16, 19, 20, 21)}}
    out.append(Case("three_cuts", ("all_three_cuts",), "draw", truncation=Truncation(top_k=4, top_p=0.9, min_p=0.02),
                    rows=[[level(P, X, qv((14, 17)), 14), level(P, Y, qv((12,)), 6), level(P, Z, qv((4,)), 4)],
                          [level(P, Z, qv((21,)), 3), level(P, X, qv((11,)), 11)]], extra={"binding": ("top_k", "top_p", "min_p")}))
    # underflow: a token 112 below the best has e = 0 in fp32; the winner's logp is exactly 0, a scored target keeps a finite one
    deep = {j: -110.0 for j in range(N_DRAW)}
    deep[12] = 2.0
    out.append(Case("underflow", ("underflow_winner_zero", "underflow_scored_target"), "draw",
                    rows=[[level(P, {2: 2.5, 14: -109.5}, qv((14,)), 14), level(P, deep, qv((0, 21)), 21)]]))
    # magnitude: g = 1e30 on two tokens, one ulp less on a third, everything else 1e30 below; temperatures at both ends
    big = np.zeros(N_DRAW, F32)
    big[[4, 9]] = F32(1e30)
    big[6] = np.nextafter(F32(1e30), F32(0))
    out.append(Case("magnitude", ("magnitude_1e30",), "draw",
                    rows=[[Draw(bias=big, q=qv((9,)), target=6), Draw(bias=big, target=9)], [Draw(bias=-big, q=qv((6,)), target=4)]]))
    out.append(Case("temp_001", ("temperature_001",), "draw", temperature=0.01,
                    rows=[[Draw(q=qv((5, 19)), target=10), Draw(bias=_b({11: 0.5, 12: 0.5}), q=qv((12,)), target=12)], [Draw(q=qv((11,)), target=2)]]))
    out.append(Case("temp_100", ("temperature_100",), "draw", temperature=100.0,
                    rows=[[Draw(q=qv((11, 14)), target=14), Draw(q=qv((1, 19)), target=19)], [Draw(bias=_b({17: 64.0}), q=qv((10, 17)), target=10)]]))
    # a finite bias whose sum with the logit overflows: HD_ERR_NUMERIC, "exactly as from the raw one"
    out.append(Case("guided_overflow", ("guided_overflow_numeric",), "draw", table="huge", error="numeric", modes=("record", "sample", "score"),
                    rows=[[Draw(q=qv((1,)), target=7), Draw(bias=_b({7: FLT_MAX}), q=qv((2,)), target=7)], [Draw(q=qv((5,)), target=5)]]))
    return out


def _b(d):
    b = np.zeros(N_DRAW, F32)
    for j, v in d.items():
        b[j] = v
    return b


def _confident_cases():
    P, out = P_MAIN, []

    def n_tied(js, lvl=2.0):
        return {j: lvl for j in js}
    # row 0: keys exactly 3 1 2 4 2 1 3; row 1: keys 2, 1 + e^-1, 2, 1, 1 + e^-1; row 2: T = 0; row 3: keys 4 3 2 1
    r0 = [n_tied((0, 1, 2)), n_tied((3,)), n_tied((4, 5)), n_tied((6, 7, 8, 9)), n_tied((10, 11)), n_tied((12,)), n_tied((13, 14, 15), 1.0)]
    r1 = [n_tied((20, 21)), {7: 2.0, 3: 1.0}, n_tied((0, 19), -1.0), n_tied((11,)), {16: 1.0, 17: 0.0}]
    r3 = [n_tied((2, 8, 14, 20)), n_tied((1, 7, 13)), n_tied((0, 6)), n_tied((18,))]

    def row(entries, seed):
        ds = []
        for t, lv in enumerate(entries):
            js = sorted(lv)
            ds.append(level(P, lv, qv([j for j in range(N_DRAW) if (j + seed) % 3 == t % 3]), js[(t + seed) % len(js)]))
        return ds
    rows = [row(r0, 0), row(r1, 1), [], row(r3, 2)]
    tags = ("confident_keys_1234", "confident_tie_by_position", "confident_T_not_multiple", "confident_T0", "confident_stable_partition",
            "confident_entries_travel", "confident_score_matches_record")
    for K in (1, 2, 3):
        out.append(Case(f"confident_K{K}", tags + (f"confident_K{K}",), "confident", rows=rows, K=K, policy="confident", prune=True))
    # keys that change under a truncation: 4 tied (key 4) against 1 + 4 e^-1/4 (4.115); top_k = 3 makes them 3 and 2.558
    Xk = n_tied((2, 5, 11, 12))
    Yk = {1: 2.0, 4: 1.75, 9: 1.75, 16: 1.75, 20: 1.75}
    Zk = {j: 2.0 for j in range(8, 14)}
    rows = [row([Xk, Yk, Zk], 0), row([Yk, Zk, Xk, n_tied((0, 3))], 1)]
    out.append(Case("confident_trunc", ("confident_trunc_changes_keys",), "confident", rows=rows, K=1, policy="confident",
                    truncation=Truncation(top_k=3)))
    out.append(Case("confident_trunc_off", ("confident_trunc_changes_keys",), "confident", rows=rows, K=1, policy="confident"))
    return out


def _beam_cases():
    P, out = P_MAIN, []
    g0 = [level(P, {4: 2.0, 9: 2.0}), level(P, {2: 2.0, 17: 2.0}), level(P, {6: 2.0, 12: 1.5, 20: 0.0})]
    g1 = [level(P, {3: 2.0, 8: 2.0, 15: 1.25}), level(P, {5: 1.0, 11: 2.0})]
    tags = ("beam_tie_in_row", "beam_tie_across_rows", "beam_two_T")
    for W in (2, 3, 4):
        out.append(Case(f"beam_W{W}", tags + (f"beam_W{W}",) + (("beam_dead_rows",) if W > 2 else ()), "beam", rows=[g0, g1], W=W, modes=("beam",)))
    out.append(Case("beam_plain_W2", ("beam_tie_in_row", "beam_tie_across_rows", "beam_W2"), "beam", rows=[[Draw(), Draw()], [Draw()]], W=2,
                    guided=False, modes=("beam",)))
    out.append(Case("beam_trunc_W3", ("beam_dead_rows", "beam_W3"), "beam", rows=[g0, g1], W=3, truncation=Truncation(top_k=1), modes=("beam",)))
    return out


_cases = None


def cases():
    global _cases
    if _cases is None:
        _cases = _draw_cases() + _confident_cases() + _beam_cases()
        assert len({c.name for c in _cases}) == len(_cases)
    return _cases


def case(name):
    return next(c for c in cases() if c.name == name)


RULES = (
    "argmax_tie_plain", "argmax_tie_guided", "argmax_tie_trunc", "argmax_k1_pruned", "argmax_k1_noprune", "argmax_block", "argmax_all_equal",
    "argmax_control_higher_wins", "greedy_tie", "greedy_logp_temp1", "topk_cut_in_tie", "topk_1", "topk_21", "topp_exact_n2", "topp_exact_n4",
    "topp_exact_n8", "topp_far_below", "topp_rank0_only", "minp_one_keeps_ties", "minp_036", "minp_037", "all_three_cuts",
    "underflow_winner_zero", "underflow_scored_target", "magnitude_1e30", "temperature_001", "temperature_100", "score_target_in_tie",
    "score_target_removed", "score_singleton", "guided_overflow_numeric", "confident_keys_1234", "confident_tie_by_position", "confident_K1",
    "confident_K2", "confident_K3", "confident_T_not_multiple", "confident_T0", "confident_stable_partition", "confident_entries_travel",
    "confident_score_matches_record", "confident_trunc_changes_keys", "beam_tie_in_row", "beam_tie_across_rows", "beam_dead_rows", "beam_W2",
    "beam_W3", "beam_W4", "beam_two_T")


# ---- a case on the micro trace -----------------------------------------------------------------------------------------------------------
_trace = {}


def batch(case, kind):
    """The arrays of a session: real micro-trace tokens, region and chain (rows of the trace, cycled); the visiting order of row b
    starts at another place of the trace's own list for every row.  Beam: every group is replicated W times."""
    if kind not in _trace:
        z = np.load(os.path.join(GOLDEN, TRACE[kind]))
        _trace[kind] = {k: z[k] for k in ("tokens", "region", "chain", "loc", "final")}
    z = _trace[kind]
    W = max(case.W, 1)
    src = np.repeat(np.arange(len(case.rows)), W)        # the case row (group) every session row comes from
    B, n = len(src), z["tokens"].shape[0]
    idx = src % n
    L = z["tokens"].shape[1]
    T = np.array([len(case.rows[r]) for r in src], np.int32)
    Tmax = max(int(T.max()), 1)
    loc = z["loc"]
    order = np.array([[loc[(7 * r + t) % len(loc)] for t in range(Tmax)] for r in src], np.int32)
    chain = None if kind == "nb" else np.concatenate([z["chain"][:n][idx], z["chain"][n:][idx]]).astype(np.int32)
    allow = np.full((B, L), ALL_TOKENS, np.uint32)
    bias = np.zeros((B, L, N_DRAW), F32)
    q = np.ones((Tmax, B, N_DRAW), F32)
    target = np.zeros((B, Tmax), np.int32)
    full = z["final"][idx].astype(np.int32)
    for b, r in enumerate(src):
        for t, d in enumerate(case.rows[r]):
            s = order[b, t]
            allow[b, s] = d.allow
            if d.bias is not None:
                bias[b, s] = d.bias
            q[t, b] = noise_of(d)
            target[b, t] = full[b, s] = target_of(d)
            if not case.guided:
                assert d.allow == ALL_TOKENS and d.bias is None, case.name
            if not case.with_bias:
                assert d.bias is None, case.name
    return SimpleNamespace(tokens=z["tokens"][idx].astype(np.int32), full=full, region=z["region"][idx].astype(np.int32), chain=chain,
                           order=order, T=T, Tmax=Tmax, B=B, L=L, allow=allow, bias=bias if case.with_bias else None, q=q, target=target,
                           src=src)


# ---- what must come out: the float64 definitions on the exactly known g ------------------------------------------------------------------
def expect_entry(case, d, q, mode):
    """One draw: (token, float64 log-probability, keep-set) of the entry `d` under the noise `q` [22]."""
    g = g_of(case, d)
    lp = guided_log_probs(g, d.allow, truncation=case.truncation)
    keep = truncation_keep(g, case.truncation)
    if mode == "score":
        tok = target_of(d)
    elif case.temperature == 0:
        tok = int(np.argmax(g))                          # (first maximum; the best token is always kept)
    else:
        with np.errstate(divide="ignore"):
            tok = int(np.argmax(np.where(keep, np.exp(lp) / np.asarray(q, np.float64), -np.inf)))
    return tok, float(lp[tok]), keep


def expect_draws(case, mode):
    """A given-order session: tokens [B][t], logp [B][t] (the draws of a forward do not see each other, so K does not enter)."""
    return [[expect_entry(case, d, noise_of(d), mode)[:2] for d in row] for row in case.rows]


def log_keys(case, row):
    with np.errstate(divide="ignore"):
        return [float(confidence_keys(g_of(case, d), truncation=case.truncation)) for d in row]


def confident_orders(keys, K):
    """The list of a row after every forward, as entry indices: the min(K, remaining) smallest (key, position) move to the front of
    the remaining part in that order, the others follow in their previous relative order."""
    lst, n, states = list(range(len(keys))), 0, []
    while n < len(keys):
        rem = lst[n:]
        k = min(K, len(rem))
        ranked = sorted(range(len(rem)), key=lambda i: (keys[rem[i]], i))[:k]
        lst = lst[:n] + [rem[i] for i in ranked] + [rem[i] for i in range(len(rem)) if i not in ranked]
        states.append(list(lst))
        n += k
    return lst, states


def expect_confident(case, mode):
    """-> (perm [B] entry index at every position, states [B] the list after every forward, draws [B][t] = (token, logp)): position t
    meets the noise of position t and the guide and target of the entry the selection put there."""
    perms, states, draws = [], [], []
    for row in case.rows:
        perm, st = confident_orders(log_keys(case, row), case.K)
        perms.append(perm)
        states.append(st)
        draws.append([expect_entry(case, row[e], noise_of(row[t]), mode)[:2] for t, e in enumerate(perm)])
    return perms, states, draws


def expect_beam(case, b):
    """Position by position, from the batch `b`: a list over t of dicts score [B] f64, parent [B], token [B], logp [B] f64, tokens
    [B, L], ran [B]; selection = guide.beam_select on the float64 candidates rounded to fp32 (designed ties are equal in both)."""
    W, G = case.W, len(case.rows)
    score = np.where(np.arange(b.B) % W == 0, 0.0, -np.inf)
    tokens = b.tokens.copy()
    steps = []
    for t in range(b.Tmax):
        new = dict(score=score.copy(), parent=np.zeros(b.B, np.int64), token=np.zeros(b.B, np.int64), logp=np.zeros(b.B), tokens=tokens.copy(),
                   ran=np.zeros(b.B, bool), cand=np.full((b.B, N_DRAW), np.nan))
        for g in range(G):
            if t >= len(case.rows[g]):
                continue
            d, r0 = case.rows[g][t], g * W
            lp = guided_log_probs(g_of(case, d), d.allow, truncation=case.truncation)
            cand = score[r0:r0 + W, None] + lp[None, :]
            w, j, _ = beam_select(cand.astype(F32), W)
            for r in range(W):
                new["score"][r0 + r], new["parent"][r0 + r], new["token"][r0 + r] = cand[w[r], j[r]], w[r], j[r]
                new["logp"][r0 + r] = lp[j[r]]
                new["tokens"][r0 + r] = tokens[r0 + w[r]]
                new["tokens"][r0 + r, b.order[r0, t]] = j[r]
            new["ran"][r0:r0 + W] = True
            new["cand"][r0:r0 + W] = cand
        score, tokens = new["score"], new["tokens"]
        steps.append(new)
    return steps


# ---- the bound on a finite log-probability ------------------------------------------------------------------------------------------------
def logp_bound(ref, terms=1):
    """|device - float64| <= terms * (4e-6 + 2^-22 |float64|), derived, not tuned: the inputs g are exact and g - mx is one correctly
    rounded subtraction (relative 2^-24); expf and logf are each within a few ulp and the sum has at most 22 positive terms, so
    logf(esum') is off by at most a few 2^-24 relative to esum' <= 22 plus a few ulp of a value below log 22 = 3.1 (< 1e-6); the final
    subtraction rounds once more (2^-24 relative to the result).  The stated bound is about twice that cost.  A beam score is a sum
    of `terms` such values."""
    return terms * (4e-6 + 2.0 ** -22 * np.abs(ref))
