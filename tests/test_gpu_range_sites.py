"""Every split-operand producer held to the range guard on its own, and the weight guard of the split weight images (the cases of
tests/range_cases.py, proven on the CPU by tests/test_range_cases_host.py).

include/hudiff_hip.h promises of the split route "never an error, never a silently wrong row": a value that leaves the fp16 range where
it is written in split form makes the library repeat the call on the fp32 kernels.  About twenty producer sites keep that promise, each
with its own absmax4 / raise_range_flag; here each of them meets an out-of-range value ALONE (nobody before it, nobody behind it), under
every kernel form that gives the site another producer or another epilogue instantiation (range_cases.PAIRS: the raise site and the
outcome of every pair, derived from the code).

  firing pair   range_fallbacks == 1, split_in_use false, last_call_repeated, no ln_sync fallback; the launch tally shows the form's split
                kernels (they ran in the first attempt: the repeat launches fp32 kernels only); logits -- or, for the stop-after cases, the
                stage buffer -- finite and BIT-IDENTICAL to a precision="f32_all" handle with the same weights and options
  its control   the same construction with the outlier at 2^14.5: no fallback, split kernels in use, result within the project's caps of the
                f32_all handle (1e-4 on logits; 5e-5 of the largest magnitude on a stage, and the same with the outlier's channel left out)
  quiet pair    Q and K under split_attn = 0 (attn_k reads fp32 Q | K | V and checks only the O it writes): the 2^20 outlier stays on the split
                route, no fallback, logits within 1e-4 of the f32_all handle
  exact         gamma = 0 / zero weight row, so the producer sees the parameter itself: 65 504 fires, nextafter(65 504, 0) does not
  two lanes     one sequence of the second lane alone carries the outlier: check_guards ORs the lanes' flags
  weights       one entry at 2^k times its matrix's largest |w|, on an input channel that is exactly zero: stages and logits within 3 x the
                float32 oracle's own distance from the float64 oracle (the bound of tests/test_gpu_variants.py), whatever k

OBSERVED (MI355X; every figure is printed by a run with -s)
controls against the f32_all handle: logits (71 pairs) at most 1.43e-6 (nb, k, default); stage buffers (16 pairs) at most 8.4e-8 of the
  largest magnitude with the outlier's channel (the 2^-22 of 23 170 itself) and 2.1e-7 without it; the quiet pairs 8.3e-7 .. 9.5e-7;
  the float below 65 504 (17 pairs) at most 9.5e-7.  The caps are 1e-4 and 5e-5: no bound comes from the split route.
weights, largest stage error as a multiple of the yard-stick (bound: 3) and logit error against float64, per k = 8 / 16 / 24 / 32:
  before the weight guard (the parent's packer)      antibody  pff1  2.1 / 2.1 / 19 / 4604     1.2e-6 / 1.3e-6 / 3.2e-5 / 6.9e-3
                                                               ff2   2.1 / 2.1 / 11 / 3110     1.2e-6 / 1.4e-6 / 1.8e-5 / 4.4e-3
                                                               wo    2.1 / 2.1 / 24 / 5546     1.3e-6 / 1.2e-6 / 2.4e-6 / 5.3e-4
                                                     nanobody  pff1  2.1 / 2.1 / 19 / 4864     1.2e-6 / 1.2e-6 / 2.0e-5 / 5.9e-3
                                                               ff2   2.1 / 2.1 / 13 / 3201     1.2e-6 / 1.2e-6 / 1.4e-5 / 3.2e-3
                                                               wo    2.1 / 2.1 / 34 / 7589     1.1e-6 / 1.1e-6 / 3.0e-6 / 6.3e-4
  with it: 2.1 at every k on both models, logits 1.1e-6 .. 1.3e-6 (k = 8 kept on the split kernels, 16 / 24 / 32 refused: the criterion is
  conservative at 2^16, where the old image still held the bound)
a pair takes about 1 s (four handles), the module (147 cases) 2 min 15 s
mutants (one library each, the module against it in its own process; the failing cases compared with range_cases.MASK_BITS / Pair.raises).
Every mutant fails exactly the cases that name its sites and no other; every failure is the missing fallback (the NaN rows behind it are
not reached by the assertion order), none a device fault:
  -DHD_GUARD_MASK=30 (GEMM epilogue)  the 34 cases that name epi.vmax -- yx_conv under split_layer_mask 2 (fp32 gemm_k) included -- and the
                                      two-lane session (its flag is the conv stack's YX copy)
  -DHD_GUARD_MASK=29 (ln_apply_k)     the 18 that name ln_apply_k            =27 (attn_k)  the 2 that name attn_k.O
  -DHD_GUARD_MASK=23 (K / V staging)  the 14 that name attn_x3_k.KV / qkv.KV    =15 (Q)       the 6 that name attn_x3_k.Q / qkv.Q
  the sites without a mask bit, all four mutated in a scratch copy of the source (the raise_range_flag call removed):
  ln_sync second pass (smax)          the 28 that name epi.smax              chain phase C operand path (vmaxc)  the 7 that name chain.norm_split
  chain finish_ln_split (vmax)        the 7 that name chain.finish           chain phase B X16 copy (vmaxy)      the 2 that name chain.epi_store
  not mutated: the raise behind the ln_sync meeting and bn_pair_a_k (range_cases.UNREACHED: no forward of the shipped library reaches them)
"""
import warnings

import numpy as np
import pytest

import hudiff_oracle as ho
import range_cases as rc
from test_gpu_components import _stages
from test_gpu_variants import LOGIT_CAP, MARGIN, STAGE_CAP, _err, _fmt, _keys

pytestmark = pytest.mark.gpu
KINDS = ("ab", "nb")


@pytest.fixture(scope="module")
def hip():
    import hudiff_amd
    if hudiff_amd.device_count() < 1:
        pytest.fail("no MI355X visible: GPU tests must run on the GPU box (there is no CPU fallback)")
    return hudiff_amd


def _model(hip, kind, sd, route, opts):
    cls = hip.AntiTFNet if kind == "ab" else hip.NanoAntiTFNet
    m = cls(**rc.config(kind), precision=route, options=opts)
    m.load_state_dict(sd)
    assert {k: m.get_option(k) for k in opts} == opts
    return m


def _inputs(kind):
    b, tokens = rc.rows(kind)
    return tokens, b["region"], b["chain"]


def _run(m, kind, site):
    """The logits of one forward or, for a stop-after site, the stage buffer right behind the site."""
    m.debug_stop_after(site.stop)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)                 # (the Python mirror announces a fallback; the counters are asserted below)
        out = m(*_inputs(kind), dropout="off")
    return m.debug_read(site.read, rc.N_SEQ) if site.read else out


def _both(hip, kind, site, form, v, exact):
    """(result, launch tally, precision report) of the form's handle and the result of the f32_all handle with the same weights and options."""
    sd, opts = rc.bent(kind, site, v, exact), form.options(kind)
    m, ref = _model(hip, kind, sd, form.route, opts), _model(hip, kind, sd, "f32_all", opts)
    try:
        m.debug_launch_tally()
        got = _run(m, kind, site)
        tally, info = m.debug_launch_tally(), m.precision_info()
        want = _run(ref, kind, site)
        assert ref.precision_info()["range_fallbacks"] == 0
    finally:
        m.close(); ref.close()
    expect, forbid = rc.witness(form, kind, site)
    missing, reached = [n for n in expect if tally[n] <= 0], [n for n in forbid if tally[n] != 0]
    assert not missing and not reached, (site.name, form.name, "never launched:", missing, "launched but must not be:", reached, {k: x for k, x in tally.items() if x})
    assert info["precision"] == form.route and info["split_built"] == (3 if form.route == "split" else 2), info
    return got, want, info


def fires(hip, kind, site, form, v, exact=False):
    got, want, info = _both(hip, kind, site, form, v, exact)
    assert (info["range_fallbacks"], info["split_in_use"], info["last_call_repeated"], info["lnsync_fallbacks"]) == (1, False, True, 0), (site.name, form.name, info)
    assert np.isfinite(got).all(), (site.name, form.name, "non-finite result")
    assert np.array_equal(got, want), (site.name, form.name, "the repeated call differs from the f32_all handle", float(np.abs(got - want).max()))


def quiet(hip, kind, site, form, v, exact=False):
    """-> the error against the f32_all handle, relative to the tensor's largest magnitude for a stage (whole tensor, outlier channel left out),
    absolute for logits."""
    got, want, info = _both(hip, kind, site, form, v, exact)
    assert (info["range_fallbacks"], info["split_in_use"], info["last_call_repeated"], info["lnsync_fallbacks"]) == (0, True, False, 0), (site.name, form.name, info)
    assert np.isfinite(got).all(), (site.name, form.name, "non-finite result")
    if not site.read:
        err = float(np.abs(got - want).max())
        assert err <= rc.LOGIT_TOL, (site.name, form.name, err)
        return (err,)
    rest = np.delete(np.arange(got.shape[-1]), site.channel)
    errs = tuple(float(np.abs(g - w).max()) / max(float(np.abs(w).max()), 1e-3) for g, w in ((got, want), (got[..., rest], want[..., rest])))
    assert max(errs) <= rc.STAGE_TOL, (site.name, form.name, errs)
    return errs


_PAIRS = rc.expanded(rc.PAIRS)


@pytest.mark.parametrize("kind,pair", _PAIRS, ids=[f"{k}-{p.site}-{p.form}" for k, p in _PAIRS])
def test_site_under_form(hip, kind, pair):
    """The pair's outcome with the outlier out of range, then its control."""
    site, form = rc.SITE[pair.site], rc.FORM[pair.form]
    if pair.fire:
        fires(hip, kind, site, form, site.value)
        errs = quiet(hip, kind, site, form, rc.CONTROL)
        print(f"\n[{kind} {site.name} {form.name}] fired at {pair.raises}; control vs f32_all: {' '.join('%.2e' % e for e in errs)}")
    else:
        errs = quiet(hip, kind, site, form, site.value)
        print(f"\n[{kind} {site.name} {form.name}] no split of the value, no fallback; vs f32_all: {' '.join('%.2e' % e for e in errs)}")


_EXACT = rc.expanded(rc.EXACT_PAIRS)


@pytest.mark.parametrize("kind,pair", _EXACT, ids=[f"{k}-{p.site}-{p.form}" for k, p in _EXACT])
def test_exact_threshold(hip, kind, pair):
    """The comparison is >= and the constant 65 504 at the site: the value reaches the producer unchanged."""
    site, form = rc.SITE[pair.site], rc.FORM[pair.form]
    fires(hip, kind, site, form, rc.LIMIT, exact=True)
    errs = quiet(hip, kind, site, form, rc.BELOW, exact=True)
    print(f"\n[{kind} {site.name} {form.name}] 65504 fired at {pair.raises}, {float(rc.BELOW)!r} did not; vs f32_all: {' '.join('%.2e' % e for e in errs)}")


@pytest.mark.parametrize("kind", KINDS)
def test_one_lane_of_two_raises_the_flag(hip, kind):
    """B = 4 on two lanes of two sequences, T = 2; only row 3 (second lane) carries the scaled token.  Tokens of the f32_all handle, one
    fallback; hd_sync notices the flag and sample_tokens() refuses the invalid steps (tests/test_gpu_adversarial.py
    ::test_range_guard_inside_a_sampling_session); the same batch without the token stays on the split kernels."""
    from hudiff_amd._lib import HudiffError
    sd, c = rc.lane_case(kind)
    opts = {"lanes": 2, "lane_min_rows": 2}
    args = lambda tok: (tok, c["region"], c["chain"], c["order"], c["T"])
    m, m2, ref = (_model(hip, kind, sd, r, opts) for r in ("split", "split", "f32_all"))
    try:
        m.debug_launch_tally()
        clean = m.sample(*args(c["clean"]), seed=5, row0=2, dropout="off")
        tally, info = m.debug_launch_tally(), m.precision_info()
        assert tally["sample_lanes_2"] > 0 and tally["sample_lanes_1"] == 0, {k: x for k, x in tally.items() if x}
        assert (info["range_fallbacks"], info["split_in_use"]) == (0, True), info
        assert np.array_equal(clean, ref.sample(*args(c["clean"]), seed=5, row0=2, dropout="off"))
        want = ref.sample(*args(c["hot"]), seed=5, row0=2, dropout="off")
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", RuntimeWarning)
            got = m.sample(*args(c["hot"]), seed=5, row0=2, dropout="off")
            info = m.precision_info()
            assert (info["range_fallbacks"], info["split_in_use"], info["last_call_repeated"], info["lnsync_fallbacks"]) == (1, False, True, 0), info
            assert np.array_equal(got, want)
            m2.sample_begin(*args(c["hot"]), seed=5, row0=2, dropout="off")
            m2.sample_run(0, 2)
            m2.sync()
            info = m2.precision_info()
            assert (info["range_fallbacks"], info["split_in_use"]) == (1, False), info
            with pytest.raises(HudiffError):
                m2.sample_tokens()
            assert np.array_equal(m2.sample_end(), want)
            assert m2.precision_info()["range_fallbacks"] == 1
    finally:
        m.close(); m2.close(); ref.close()


# ---- Part B ----------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def yards():
    """kind -> float64 trace of the unbent function (k = 0: all three zero-input constructions, no entry scaled) and the bound per stage:
    3 x the float32 oracle's own distance from it, under the caps (tests/test_gpu_variants.py)."""
    cache = {}

    def yard(kind):
        if kind not in cache:
            cfg = rc.config(kind)
            sd, _ = rc.weight_bent(kind, "pff1", 0)
            n_att = int(cfg["cs_layers"])
            keys = _keys(kind, n_att)
            traces = {}
            for dt in (np.float64, np.float32):
                net = ho.OracleNet(kind, cfg, sd, dtype=dt)
                net.trace = {}
                logits = net(*_inputs(kind))
                traces[dt] = dict(net.trace, logits=logits)
            e_ref = {k: _err(k, traces[np.float32][k], traces[np.float64][k]) for k in keys}
            bound = {k: min(MARGIN * v, LOGIT_CAP if k == "logits" else STAGE_CAP) for k, v in e_ref.items()}
            print(f"\n[yard {kind}] e_ref {_fmt(e_ref)}\n[yard {kind}] bound {_fmt(bound)}")
            cache[kind] = dict(keys=keys, t64=traces[np.float64], bound=bound, n_att=n_att, d=int(cfg["d_model"]))
        return cache[kind]
    return yard


_WEIGHTS = [(kind, name, k) for kind in KINDS for name in sorted(rc.WEIGHT_CASES) for k in rc.WEIGHT_KS]


@pytest.mark.parametrize("kind,name,k", _WEIGHTS, ids=[f"{a}-{b}-2^{c}" for a, b, c in _WEIGHTS])
def test_weight_dynamic_range(hip, yards, kind, name, k):
    """The function does not depend on k, so neither may the result: every stage within the yard-stick bound of the float64 trace.  An image
    the weight guard refuses (range_cases.weight_guard_holds, the mirror of X3Packer::add) is reported (split_built bit 0 clear) and its
    family runs the fp32 GEMMs."""
    Y = yards(kind)
    sd, arrays = rc.weight_bent(kind, name, k)
    holds, family = rc.weight_guard_holds(arrays), rc.WEIGHT_CASES[name][1]
    m = _model(hip, kind, sd, "split", {})
    try:
        m.debug_launch_tally()
        got = _stages(m, kind, *_inputs(kind), rc.N_SEQ, Y["d"], Y["n_att"])
        tally, info = m.debug_launch_tally(), m.precision_info()
    finally:
        m.close()
    errs = {key: float(np.abs(got[key].astype(np.float64) - Y["t64"][key]).max()) / (1.0 if key == "logits" else max(float(np.abs(Y["t64"][key]).max()), 1e-3))
            for key in Y["keys"]}
    worst = max(Y["keys"], key=lambda key: errs[key] / Y["bound"][key])
    print(f"\n[{kind} {name} 2^{k}] image {'kept' if holds else 'refused'}; split_built {info['split_built']}; logits {errs['logits']:.2e}; "
          f"worst {worst} {errs[worst]:.2e} = {errs[worst] / Y['bound'][worst] * MARGIN:.1f} x yard-stick")
    bad = {key: (errs[key], Y["bound"][key]) for key in Y["keys"] if not (np.isfinite(got[key]).all() and errs[key] <= Y["bound"][key])}
    assert not bad, ("stage error above 3 x yard-stick (error, bound)", bad)
    assert info["range_fallbacks"] == 0 and info["lnsync_fallbacks"] == 0 and info["split_in_use"], info
    assert info["split_built"] == (3 if holds else 2), (holds, info)
    assert info["lnsync_in_use"] == (holds or family != 1), (holds, family, info)      # (a refused ByteNet family runs no meeting epilogue)
    conv, core = sum(tally[n] for n in rc._CONV), tally[rc.CORE[kind]]
    if holds:
        assert conv > 0 and core > 0, {n: x for n, x in tally.items() if x}
    else:                               # the refused family on the fp32 GEMMs, the other one still on the split kernels
        assert (conv == 0 and core > 0) if family == 1 else (conv > 0 and core == 0 and tally["attn_f32"] > 0), {n: x for n, x in tally.items() if x}
