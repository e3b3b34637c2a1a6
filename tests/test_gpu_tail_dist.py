"""The pruned tail's whole 22-token distribution against the float64 oracle (hd_api.hip pruned_tail: the sliced form tail_pw_k ..
tail_ff2_k, the launches gather_rows_k .. head_proj_k, value through rows and through the projection).

Everywhere else the suite sees the tail through ONE number per draw (the drawn token's log-probability, to REF_TOL = 2e-4) or through
token equality.  Here a scoring session of 22 copies of a row that differ only in the probed token returns the device's whole
log-softmax at (sequence, slot) from one forward (tests/tail_cases.py), and every one of the 22 values is held to
    |device - float64 oracle| <= 3 x yard-stick,        |device - device| <= 6 x yard-stick  (forms, pruned against unpruned)
with the yard-stick = max |log_softmax(oracle float32) - log_softmax(oracle float64)| over all probes of the (group, kind, dropout),
computed on the CPU when the module runs; 3 x yard-stick < 2e-5 is asserted by tests/test_tail_cases_host.py.  No bound comes from a
tail form's own error.

Cases: every slot of tail_cases.SLOTS on two sequences, every form x route of tail_cases.main_matrix, each form witnessed in
hd_debug_launch_tally; batch edges (fillers with T = 0 between probe rows, rows per lane = 1, 2, 3 mod 4, exactly 64 and 65
sequences per lane with default options, one and two lanes); a probe at step 2; graph against eager, bit for bit; generated dropout
masks; the value a sampling session records for the token it drew against the scoring session's, bit for bit.

No yard-stick was widened: no form on no route needed the prune=False control's distance in place of the oracle's.

OBSERVED (MI355X).  Yard-sticks: production antibody 1.82e-6, nanobody 1.42e-6; under dropout 1.45e-6 / 1.25e-6 (12 values each); micro
antibody 3.87e-7, nanobody 3.57e-7.  Worst |device - float64| over all slots, as a multiple of the yard-stick (bound: 3):
  production     default (launches, rows)  sliced  launches_rows  launches_proj  prune=False
  ab  split      0.55                      0.50    0.55           0.57           0.57
      f32_all    0.67                      0.63    0.67           0.63           0.63
      f32_gemm   0.60                      0.58
  nb  split      0.81                      0.79    0.81           0.98           1.06
      f32_all    1.06                      1.06    1.06           1.06           1.06
      f32_gemm   0.66                      0.98
  micro          default                           launches_rows  launches_proj  prune=False
  ab  split      2.05                              2.05           2.05           2.05        (7.9e-7: three fp32 ulps of a value near -3;
      f32_all    1.41                              1.41           1.83           1.58         the unpruned block is as far)
      f32_gemm   2.05
  nb  split      1.57                              1.57           1.74           1.57
      f32_all    1.43                              1.43           1.43           1.29
      f32_gemm   1.57
The micro bound is 1.16e-6 / 1.07e-6, four to five fp32 ulps of a value near -3: little headroom, by the rule and not by tuning.
No slot stands out (per slot 0.29 .. 0.67 antibody, 0.44 .. 1.06 nanobody at production width).  Device against device (bound: 6):
production <= 0.67, micro <= 2.67.  The 64 / 65 switch with default options, split / f32_all / f32_gemm: antibody sliced (64, 128 rows)
0.45 / 0.44 / 0.45, launches (65, 130) 0.45 / 0.57 / 0.44; nanobody sliced 0.64 / 0.66 / 0.98, launches 0.65 / 0.83 / 0.66.  The other
edges: production <= 0.83 (sliced 23 + 22 antibody 0.71), micro <= 1.48; the later step 0.36 .. 0.84; under dropout <= 0.60 of that
yard-stick, pruned against unpruned <= 0.38.  Graph and eager, and the recorded against the scored value, agree bit for bit in every
form.  The module takes about 30 s, a case about 0.2 s (the first of a kind builds its oracle references: 2.4 s antibody, dropout 4.2 s).

MUTATIONS, each seen to fail this module on an MI355X (arithmetic only, applied to both forms at once, reverted): failed cases of this
module; then of tests/test_gpu_logp.py (42 cases) and of tests/test_gpu_variants.py -k sampling (26 cases)
  query rotated with RoPE row 0 instead of the slot (attn_row_k, tail_pw_k)          92 of 108    26   4
  Pw written without the rstd factor (attn_row_k, tail_pw_k)                         70 of 108    27   6
  light segment's accumulation skipped (row_value_k, tail_val_k)                     44 of 126    13   3   (antibody, value through rows)
  t_v dropped (head_proj_k, tail_out_k)                                              88 of 126    26   6   (not the projection form)
  LN2 statistics of ATc taken before the out-projection residual                    110 of 126    25   2
  t_v scaled by 1 - 1/128 (head_proj_k, tail_out_k)                                  80 of 126    11   0   (see below)
(The first two ran before the sliced x f32_gemm and the three-route 64 / 65 cases were added.)  The first five are gross: the older
modules notice each.  The sixth is the kind this module is for: at production width it moves the distribution by 1.08e-5 .. 1.14e-5
(antibody, 5.9 .. 6.2 x the yard-stick) and 4.7e-6 .. 5.5e-6 (nanobody, 3.3 .. 3.9 x), a twentieth of REF_TOL -- every production
case of this module without dropout fails, test_gpu_variants.py -k sampling and the production-width cases of test_gpu_logp.py pass;
test_gpu_logp.py notices it through the micro antibody model alone (2.8e-4 there).  Dropping t_v altogether moves the distribution by
5.7e-4 .. 1.4e-3 at production width and by 1.6e-5 .. 2.0e-5 under dropout (11 .. 16 x that yard-stick, a tenth of REF_TOL).
"""
import numpy as np
import pytest

import tail_cases as TC
from test_gpu_logp import _mk
from test_gpu_variants import _check_tally

pytestmark = pytest.mark.gpu

GROUP_KINDS = [("prod", "ab"), ("prod", "nb"), ("micro", "ab"), ("micro", "nb")]
PROD = [("prod", "ab"), ("prod", "nb")]


@pytest.fixture(scope="module")
def hip():
    import hudiff_amd
    if hudiff_amd.device_count() < 1:
        pytest.fail("no MI355X visible: GPU tests must run on the GPU box (there is no CPU fallback)")
    return hudiff_amd


@pytest.fixture(scope="module")
def refs():
    """(group, kind) -> the float64 reference and the yard-stick: built once per kind for the whole module (tail_cases keeps them)."""
    return TC.reference


TUNED = ("tail_form", "tail_max_rows", "prune_value_via_rows", "lane_min_rows")


@pytest.fixture(scope="module")
def handles(hip):
    """Handles are kept while the module stays with one (group, kind) and closed when it moves on.  A session with default options runs
    on a handle no option was ever set on, so what it witnesses is the library's own choice; the others share one handle per route, on
    which every option of TUNED is set for every session (the case's value, or the default the handle reported when it was made)."""
    live = {}

    def close_all():
        for m, _ in live.values():
            m.close()
        live.clear()

    def get(group, kind, route, opts, dropout=False):
        if live and next(iter(live))[:2] != (group, kind):
            close_all()
        key = (group, kind, route, dropout, bool(opts))
        if key not in live:
            m = _mk(hip, kind, *TC.weights(group, kind, dropout=dropout), precision=route)
            live[key] = (m, {k: m.get_option(k) for k in TUNED})
        m, defaults = live[key]
        if opts:
            assert set(opts) <= set(TUNED), opts
            for k, v in dict(defaults, **opts).items():
                m.set_option(k, v)
            assert {k: m.get_option(k) for k in opts} == opts
        return m

    yield get
    close_all()


def _form(form, opts=None):
    o, kw, expect, forbid = TC.FORMS[form] if form != "default" else ({}, {}, (), ())
    return dict(o, **(opts or {})), dict(kw), expect, forbid


def _score(m, s, **kw):
    """One scoring session up to the step that is read -> (logp [B] of that step, the whole record, tokens as they stand, tally, report)."""
    m.debug_launch_tally()
    m.score_begin(s.tokens, s.region, s.chain, s.order, s.T, **kw)
    try:
        m.sample_run(0, s.read + 1)
        logp = m.sample_logp()
        tokens = m.sample_tokens()
    finally:
        m.sample_end()
    return logp[:, s.read].copy(), logp, tokens, m.debug_launch_tally(), m.precision_info()


def _check_session(s, col, logp, tokens, info, route, what):
    """What holds for every session: fillers untouched with a record of zeros, probe rows re-filled with their own token, nothing
    recorded behind the step read, finite negative values, no guard."""
    assert np.array_equal(tokens[s.fill], s.tokens[s.fill]), (what, "a filler row's tokens changed")
    assert (logp[s.fill] == 0).all(), (what, "a filler row recorded something")
    assert (logp[:, s.read + 1:] == 0).all(), what
    for r, (q, slot, j) in zip(s.probe_rows, s.picks):
        assert tokens[r, slot] == j, (what, r)
    v = col[s.probe_rows]
    assert np.isfinite(v).all() and (v < 0).all(), what
    assert info["precision"] == route and info["range_fallbacks"] == 0 and info["lnsync_fallbacks"] == 0, (what, info)


def _worst(got, want):
    return float(np.abs(got.astype(np.float64) - want).max())


@pytest.fixture(scope="module")
def main_runs(handles, refs):
    """(group, kind, form, route) -> the 22-token values of every probe of the all-slots batch [n], run once and kept for the
    device-against-device comparisons."""
    memo = {}

    def run(group, kind, form, route):
        key = (group, kind, form, route)
        if key in memo:
            return memo[key]
        picks = TC.all_picks(kind)
        s = TC.session(group, kind, picks, B=len(picks) + 3)
        opts, kw, expect, forbid = _form(form)
        if form == "default":       # above 64 sequences per lane the library itself takes the launches (micro: at every size)
            expect, forbid = ("tail_launches", "value_via_rows", "sample_lanes_2"), ("tail_sliced", "value_via_projection", "sample_lanes_1")
        col, logp, tokens, tally, info = _score(handles(group, kind, route, opts), s, **kw)
        what = f"{group} {kind} {form} {route}"
        _check_tally(tally, kind, expect, forbid, what)
        _check_session(s, col, logp, tokens, info, route, what)
        memo[key] = (s, col[s.probe_rows])
        return memo[key]

    return run


@pytest.mark.parametrize("group,kind,form,route", [(g, k, f, r) for g, k in GROUP_KINDS for f, r in TC.main_matrix(g)],
                         ids=[f"{g}-{k}-{f}-{r}" for g, k in GROUP_KINDS for f, r in TC.main_matrix(g)])
def test_every_slot_every_form_vs_float64(main_runs, refs, group, kind, form, route):
    """All slots of the kind on two sequences, 22 tokens each, one forward: every value within 3 x yard-stick of float64; the worst
    per slot is printed as a multiple of the yard-stick."""
    ref = refs(group, kind)
    s, got = main_runs(group, kind, form, route)
    err = np.abs(got.astype(np.float64) - TC.expected(ref, s)).reshape(TC.N_SEQ, len(TC.SLOTS[kind]), 22)
    per_slot = err.max(axis=(0, 2)) / ref.yard
    print(f"\n[tail {group} {kind} {form} {route}] yard-stick {ref.yard:.3e} worst {err.max():.3e} = {err.max() / ref.yard:.2f} x | per slot "
          + " ".join(f"{sl}:{x:.2f}" for sl, x in zip(TC.SLOTS[kind], per_slot)))
    # the 22 values of a probe are a distribution (each within the bound of one that sums to 1: so does the logarithm of their sum)
    total = np.log(np.exp(got.astype(np.float64).reshape(-1, 22)).sum(-1))
    assert np.abs(total).max() <= ref.bound, np.abs(total).max()
    assert err.max() <= ref.bound, (err.max(), ref.bound, err.max() / ref.yard)


@pytest.mark.parametrize("group,kind", GROUP_KINDS)
def test_forms_agree_with_each_other_and_with_the_unpruned_block(main_runs, refs, group, kind):
    """Device against device on the same route: every tail form against every other and against prune=False, within 6 x yard-stick."""
    ref = refs(group, kind)
    for route in ("split", "f32_all"):
        vals = {f: main_runs(group, kind, f, route)[1] for f in ("default",) + TC.forms_of(group)}
        names = sorted(vals)
        worst = {(a, b): _worst(vals[a], vals[b].astype(np.float64)) for i, a in enumerate(names) for b in names[i + 1:]}
        print(f"\n[tail {group} {kind} {route}] device against device, x yard-stick: " + " ".join(f"{a}|{b}:{e / ref.yard:.2f}" for (a, b), e in worst.items()))
        bad = {k: e for k, e in worst.items() if not e <= ref.pair}
        assert not bad, (bad, ref.pair)


def _by_kind(forms):
    """(group, kind, form) with the kind outermost, so that the handles of a kind serve all its cases before they are closed."""
    return [(g, k, f) for g, k in PROD for f in forms]


def _edge_picks(kind):
    return TC.all_picks(kind, seqs=(0,), slots=TC.EDGE_SLOTS[kind])


EDGE_PARAMS = [(g, k, e, r) for g, k in GROUP_KINDS for e in TC.EDGES if g in e[6] for r in TC.edge_routes(e[0])]


@pytest.mark.parametrize("group,kind,edge,route", EDGE_PARAMS, ids=[f"{g}-{k}-{e[0]}-{r}" for g, k, e, r in EDGE_PARAMS])
def test_batch_edges(handles, refs, group, kind, edge, route):
    """Fillers between the probe rows, ragged groups of four, the 64 / 65 switch selected by the library, one and two lanes."""
    name, B, opts, kw, expect, forbid, _ = edge
    ref = refs(group, kind)
    s = TC.session(group, kind, _edge_picks(kind), B=B)
    col, logp, tokens, tally, info = _score(handles(group, kind, route, opts), s, **kw)
    what = f"{group} {kind} {name} {route}"
    e = _worst(col[s.probe_rows], TC.expected(ref, s))
    seen = [k for k in ("tail_sliced", "tail_launches", "value_via_rows", "value_via_projection", "sample_lanes_1", "sample_lanes_2") if tally[k]]
    print(f"\n[tail edge {what}] B {B} fillers at {[int(r) for r in s.fill]} worst {e:.3e} = {e / ref.yard:.2f} x | {seen}")
    _check_tally(tally, kind, expect, forbid, what)
    _check_session(s, col, logp, tokens, info, route, what)
    assert e <= ref.bound, (e, ref.bound, e / ref.yard)


@pytest.mark.parametrize("group,kind,form", _by_kind(TC.TAIL_FORMS + ("noprune",)), ids=str)
def test_a_later_step(handles, refs, group, kind, form):
    """order = [a, b, s, ...], three steps run, step 2 read: the device's step counter feeds the tail's row choice and RoPE row."""
    ref = refs(group, kind)
    q, slot = TC.LATER[kind]["seq"], TC.LATER[kind]["slot"]
    s = TC.session(group, kind, [(q, slot, j) for j in range(22)], B=23, later=True)
    opts, kw, expect, forbid = _form(form)
    col, logp, tokens, tally, info = _score(handles(group, kind, "split", opts), s, **kw)
    what = f"{group} {kind} later {form}"
    e = _worst(col[s.probe_rows], TC.expected(ref, s))
    print(f"\n[tail {what}] worst {e:.3e} = {e / ref.yard:.2f} x")
    _check_tally(tally, kind, expect, forbid, what)
    _check_session(s, col, logp, tokens, info, "split", what)
    assert (logp[s.probe_rows][:, :2] < 0).all()
    assert e <= ref.bound, (e, ref.bound, e / ref.yard)


@pytest.mark.parametrize("group,kind,form", _by_kind(TC.TAIL_FORMS), ids=str)
def test_graph_and_eager_give_the_same_bits(handles, refs, group, kind, form):
    ref = refs(group, kind)
    s = TC.session(group, kind, _edge_picks(kind), B=47)
    opts, kw, expect, forbid = _form(form)
    m = handles(group, kind, "split", opts)
    out = {g: _score(m, s, graph=g, **kw) for g in (True, False)}
    for g, (col, logp, tokens, tally, info) in out.items():
        _check_tally(tally, kind, expect, forbid, (form, g))
        _check_session(s, col, logp, tokens, info, "split", (form, g))
    assert np.array_equal(out[True][1], out[False][1]), form
    e = _worst(out[True][0][s.probe_rows], TC.expected(ref, s))
    assert e <= ref.bound, (e, ref.bound)


@pytest.mark.parametrize("group,kind,form", _by_kind(TC.TAIL_FORMS), ids=str)
def test_recorded_value_is_the_scored_value(handles, refs, group, kind, form):
    """A sampling session on the same rows draws some token j* per row and records its log-probability: bit for bit the value the
    scoring session finds for j* at that probe."""
    picks = _edge_picks(kind)
    s = TC.session(group, kind, picks, B=47)
    smp = TC.session(group, kind, picks, B=47, sampling=True)
    opts, kw, expect, forbid = _form(form)
    m = handles(group, kind, "split", opts)
    col, logp, tokens, tally, info = _score(m, s, **kw)
    m.sample_begin(smp.tokens, smp.region, smp.chain, smp.order, smp.T, seed=11, row0=5, dropout="off", record_logp=True, **kw)
    try:
        m.sample_run(0, 1)
        rec = m.sample_logp()[:, 0]
        drawn = m.sample_tokens()
    finally:
        m.sample_end()
    _check_tally(m.debug_launch_tally(), kind, expect, forbid, (form, "sampling session"))       # (the scoring session's was read and cleared by _score)
    _check_tally(tally, kind, expect, forbid, form)
    row_of = {p: int(r) for r, p in zip(s.probe_rows, s.picks)}
    stars = set()
    for r, (q, slot, _) in zip(smp.probe_rows, smp.picks):
        j = int(drawn[r, slot])
        assert 0 <= j < 22
        stars.add((slot, j))
        assert rec[r] == col[row_of[(q, slot, j)]], (form, r, slot, j, rec[r], col[row_of[(q, slot, j)]])
    assert (rec[smp.fill] == 0).all() and np.array_equal(drawn[smp.fill], smp.tokens[smp.fill])
    assert len(stars) > 2, stars                                             # (more than one token per slot was tied to its probe)


DROP_MATRIX = [("sliced", "split"), ("sliced", "f32_all"), ("launches_rows", "split"), ("launches_rows", "f32_all"), ("launches_proj", "split"),
               ("launches_proj", "f32_all")]


@pytest.mark.parametrize("kind,form,route", [(k, f, r) for k in ("ab", "nb") for f, r in DROP_MATRIX], ids=str)
def test_generated_dropout_masks(handles, kind, form, route):
    """dropout="faithful" with the production p: every copy has its own global row id, hence its own masks and its own oracle row; six
    tokens of two slots are held to the float64 oracle under the same masks, all 22 to prune=False on the same handle."""
    ref = TC.reference_dropout(kind)
    s = TC.drop_session(kind)
    opts, kw, expect, forbid = _form(form)
    m = handles("prod", kind, route, opts, dropout=True)
    col, logp, tokens, tally, info = _score(m, s, **TC.DROP_KW, **kw)
    full, logp_f, tokens_f, tally_f, info_f = _score(m, s, prune=False, **TC.DROP_KW)
    off = _score(m, s, dropout="off", **kw)[0]
    what = f"prod {kind} dropout {form} {route}"
    e = _worst(col[ref.rows], ref.want)
    e_ctl = _worst(full[ref.rows], ref.want)
    e_pair = _worst(col[s.probe_rows], full[s.probe_rows].astype(np.float64))
    print(f"\n[tail {what}] yard-stick {ref.yard:.3e} worst {e:.3e} = {e / ref.yard:.2f} x | prune=False control {e_ctl:.3e} = {e_ctl / ref.yard:.2f} x | "
          f"pruned against unpruned {e_pair:.3e} = {e_pair / ref.yard:.2f} x")
    _check_tally(tally, kind, expect, forbid, what)
    _check_tally(tally_f, kind, (), TC.FORMS["noprune"][3], what)
    _check_session(s, col, logp, tokens, info, route, what)
    _check_session(s, full, logp_f, tokens_f, info_f, route, what)
    assert np.abs(off[s.probe_rows] - col[s.probe_rows]).max() > 1e-2         # the masks really entered
    assert e <= ref.bound, (e, ref.bound, e / ref.yard)
    assert e_pair <= ref.pair, (e_pair, ref.pair, e_pair / ref.yard)
