"""Every kernel variant that hd_set_option can select, held to a float64 evaluation of the oracle stage by stage.

include/hudiff_hip.h promises that no tuning option "changes results beyond the last-ulp reassociation".  Each case below builds one
handle with one set of options, runs three real sequences through it (456 heavy + 417 light rows / 456 nanobody rows: every tile
height has a ragged last tile in each segment, 128- and 256-row tiles span two or three sequences so that the dilated taps must
zero-pad INSIDE a tile, and heavy and light tiles use different weights) and checks, in this order,
  (a) the launch tally (hd_debug_launch_tally) shows the kernels the case is about and none of those it must not reach,
  (b) every stage read back from the HIP buffers is within 3 x the yard-stick of the float64 oracle's trace,
  (c) the logits are within 2e-5 of the same route's default-option handle,
  (d) a second identical call gives the same bits,
  (e) with generated dropout masks the logits are within 3 x the yard-stick of the float64 oracle under the same masks,
  (f) no guard fired.

The yard-stick of a stage is the float32 oracle's own distance from the float64 oracle (same weights, same rows), relative to the
tensor's largest magnitude (absolute for the logits), computed on the CPU when the module runs; the bound is 3 x that, the margin
tests/test_gpu_x3.py::test_x3_logits_vs_float64_oracle gives a route over the fp32 arithmetic's own distance: it covers another
summation order, not a missing term.  No stage needs more: on an MI355X the default-option f32_all handle is within 1.8 x the
yard-stick at every stage (OBSERVED), so no yard-stick is widened by a device measurement, no bound comes near the project's caps
(5e-5 relative per stage, 1e-4 on the logits) and none is derived from the variant being judged.

The sampling variants (lanes, forms of the pruned tail, loop graph, fp32 tiles on a handful of rows) are compared through the
log-probabilities they record and score: those move when the pruned tail is wrong by far less than a token flip.

OBSERVED (MI355X; three sequences, weights seed 3, rows from row0 = 17)
yard-stick, float32 oracle against float64 oracle, antibody / nanobody:
  aa_encoder 1.45e-7 / 1.35e-7, pos 3.32e-7 / 3.94e-7, chn 3.76e-7 / -, conv 3.50e-7 / 3.80e-7, att{n}_at1 3.44e-7 .. 3.72e-7 /
  3.62e-7 .. 3.85e-7, att{n} 3.44e-7 .. 3.81e-7 / 3.69e-7 .. 3.89e-7, last at2 3.54e-7 / 3.76e-7, logits 2.75e-6 / 2.39e-6,
  logits under dropout 2.96e-6 / 3.50e-6
default-option f32_all handle against float64, as a multiple of the yard-stick: antibody 0.97 .. 1.28 per stage (pos 4.24e-7),
  logits 0.50 (1.38e-6), under dropout 1.12 (3.33e-6); nanobody 1.15 .. 1.51 per stage (aa_encoder 2.04e-7, pos 5.25e-7), logits
  0.58 (1.38e-6), under dropout 1.76 (6.14e-6)
worst case per route (largest stage error; logits; logits under dropout; logits against the default options; largest multiple
of the yard-stick and where):
  antibody  split     4.24e-7  1.44e-6  3.33e-6  1.19e-6   1.36 (aa_encoder, tiny_grid 0)
            f32_all   4.24e-7  1.38e-6  3.45e-6  9.54e-7   1.28 (pos)
            f32_gemm  4.24e-7  1.38e-6  3.57e-6  1.07e-6   1.28 (pos)
  nanobody  split     5.25e-7  1.41e-6  6.62e-6  1.07e-6   1.89 (logits under dropout, split_layer_mask 2)
            f32_all   5.70e-7  1.39e-6  6.14e-6  8.34e-7   1.75 (logits under dropout, default options)
            f32_gemm  5.43e-7  1.38e-6  4.54e-6  9.54e-7   1.51 (aa_encoder)
sampling: baseline against float64 4.77e-7 (antibody) / 1.19e-6 (nanobody), recorded and scored; every variant within 7.2e-7 of it
every case is bit-repeatable; a forward case takes about 1 s, a sampling case less
"""
import numpy as np
import pytest

import hudiff_oracle as ho
from test_gpu_components import _stages
from test_gpu_logp import PAIR_TOL, REF_TOL, log_softmax64

pytestmark = pytest.mark.gpu

STAGE_CAP, LOGIT_CAP, MARGIN, DEFAULT_TOL = 5e-5, 1e-4, 3.0, 2e-5
DROP_KW = dict(dropout="faithful", seed=99, row0=3, step=17)
N_SEQ = 3

X3_IDS = ("x3_256x256_s2", "x3_256x128_s3", "x3_128x128_plain", "x3_128x128_lnsync", "x3_64x128_s2", "x3_64x128_s3", "x3_32x128_s2",
          "x3_32x128_s3", "x3_32x128_s3_loaders")
X3_ALL = tuple(n + c for n in X3_IDS for c in ("", "_conv"))
X3_32 = tuple(n for n in X3_ALL if n.startswith("x3_32x128"))
X3_64 = tuple(n for n in X3_ALL if n.startswith("x3_64x128"))
X3_128 = tuple(n for n in X3_ALL if n.startswith("x3_128x128"))
X3_8WAVE = tuple(n for n in X3_ALL if n.startswith("x3_256"))
# per kind: the split attention core of the two-launch form, the fused projection + attention kernel
CORE = {"ab": "attn_x3_19_w12", "nb": "attn_x3_10"}
FUSED = {"ab": "qkv_attn_19", "nb": "qkv_attn_10"}
CORES = ("attn_x3_19_w12", "attn_x3_19_w8", "attn_x3_10")
FUSEDS = ("qkv_attn_19", "qkv_attn_10")


def _but(names, *keep):
    return tuple(n for n in names if n not in keep)


def V(id, route, opts, expect, forbid=(), kinds=("ab", "nb"), check=None):
    return dict(id=id, route=route, opts=opts, expect=expect, forbid=forbid, kinds=kinds, check=check)


# "CORE" / "FUSED" in expect stand for the kind's kernel; a dict {kind: names} adds names for one kind only.
# Three sequences: every split launch's 128 x 128 grid is below small_grid (320) and nearly every 64 x 128 grid below tiny_grid (150),
# so the default lands on 32 x 128 tiles -- except the antibody Q|K|V projection (14 x 12 = 168 tiles of 64 rows), which keeps 64 x 128.
FORWARD_VARIANTS = [
    V("default", "split", {}, ("x3_32x128_s3_loaders", "x3_32x128_s3_loaders_conv", "CORE", "attn_qsplit"), X3_128 + X3_8WAVE + FUSEDS + ("attn_f32",)),
    V("no_loaders", "split", {"loader_waves": 0}, ("x3_32x128_s3", "x3_32x128_s3_conv"), ("x3_32x128_s3_loaders", "x3_32x128_s3_loaders_conv", "x3_32x128_s2", "x3_32x128_s2_conv")),
    V("tiny2", "split", {"tiny_stages": 2}, ("x3_32x128_s2", "x3_32x128_s2_conv"), _but(X3_32, "x3_32x128_s2", "x3_32x128_s2_conv")),
    V("small3", "split", {"tiny_grid": 0}, ("x3_64x128_s3", "x3_64x128_s3_conv"), X3_32 + ("x3_64x128_s2", "x3_64x128_s2_conv") + X3_128 + X3_8WAVE),
    V("small2_forced", "split", {"tiny_grid": 0, "small_stages": 2}, ("x3_64x128_s2", "x3_64x128_s2_conv"), X3_32 + ("x3_64x128_s3", "x3_64x128_s3_conv")),
    V("small2_by_limit", "split", {"tiny_grid": 0, "small_stages3_max_grid": 0}, ("x3_64x128_s2", "x3_64x128_s2_conv"), X3_32 + ("x3_64x128_s3", "x3_64x128_s3_conv")),
    # the kernels of the 256-row metric on three sequences (level 2: every tap GEMM meets, so the plain tap tile is the lnsync0 case's)
    V("big_fused", "split", {"small_grid": 0, "fused_attn_min_grid": 0}, ("x3_128x128_plain", "x3_128x128_lnsync", "x3_128x128_lnsync_conv", "FUSED"),
      X3_32 + X3_64 + X3_8WAVE + CORES + ("attn_f32", "x3_128x128_plain_conv")),
    V("big_lnsync1", "split", {"small_grid": 0, "lnsync_level": 1}, ("x3_128x128_plain", "x3_128x128_lnsync", "x3_128x128_lnsync_conv"), X3_32 + X3_64 + X3_8WAVE),
    V("big_lnsync0", "split", {"small_grid": 0, "lnsync_level": 0}, ("x3_128x128_plain", "x3_128x128_plain_conv"), _but(X3_ALL, "x3_128x128_plain", "x3_128x128_plain_conv")),
    V("tile256_lnsync0", "split", {"split_tile": 256, "lnsync_level": 0}, ("x3_256x128_s3", "x3_256x128_s3_conv"), _but(X3_ALL, "x3_256x128_s3", "x3_256x128_s3_conv")),
    # ln_sync launches never take the 8-wave tiles: they fall back to the 128-row shape, which the default small_grid / tiny_grid then
    # size to this grid (32 x 128); with small_grid = 0 they stay on the 128 x 128 meeting tile (next case)
    V("tile256", "split", {"split_tile": 256}, ("x3_256x128_s3", "x3_32x128_s3_loaders", "x3_32x128_s3_loaders_conv"),
      ("x3_256x128_s3_conv", "x3_256x256_s2", "x3_256x256_s2_conv", "x3_128x128_plain", "x3_128x128_plain_conv") + X3_64),
    V("tile256_big", "split", {"split_tile": 256, "small_grid": 0}, ("x3_256x128_s3", "x3_128x128_lnsync", "x3_128x128_lnsync_conv"),
      ("x3_256x128_s3_conv", "x3_256x256_s2", "x3_256x256_s2_conv", "x3_128x128_plain", "x3_128x128_plain_conv") + X3_64 + X3_32),
    # N in {256, 512, 768, 1536} takes 256 x 256; the tap GEMMs have N = 128 (token encoder) and 384 (antibody) / 256 (nanobody): only the
    # nanobody's can; N % 256 != 0 keeps 128-wide tiles (sized to the grid: 32 x 128)
    V("tile512", "split", {"split_tile": 512, "lnsync_level": 0, "fused_attn": 0},
      ("x3_256x256_s2", "x3_32x128_s3_loaders", "x3_32x128_s3_loaders_conv", "CORE", {"nb": ("x3_256x256_s2_conv",)}),
      ("x3_256x128_s3", "x3_256x128_s3_conv", {"ab": ("x3_256x256_s2_conv",)}) + X3_128 + X3_64 + FUSEDS),
    V("no_qsplit", "split", {"fused_attn": 0, "attn_qsplit_max_grid": 0}, ("CORE",), ("attn_qsplit", "attn_f32") + FUSEDS),
    V("attn_8_waves", "split", {"fused_attn": 0, "attn_waves": 8}, ("attn_x3_19_w8",), ("attn_x3_19_w12", "attn_f32") + FUSEDS, kinds=("ab",)),
    V("fp32_attention_core", "split", {"split_attn": 0}, ("attn_f32", "x3_32x128_s3_loaders", "x3_32x128_s3_loaders_conv"), CORES + FUSEDS),
    V("split_bytenet_only", "split", {"split_layer_mask": 1}, ("attn_f32", "x3_32x128_s3_loaders", "x3_32x128_s3_loaders_conv", "f32_32x128"), CORES + FUSEDS,
      check="no_split_attention_gemm"),
    V("split_attention_only", "split", {"split_layer_mask": 2}, ("CORE", "x3_32x128_s3_loaders", "f32_32x128"), tuple(n for n in X3_ALL if n.endswith("_conv")) + ("attn_f32",),
      check="no_split_bytenet_gemm"),
    V("split_min_rows_above", "split", {"split_min_rows": 10 ** 6}, ("f32_32x128", "attn_f32"), X3_ALL + CORES + FUSEDS),
    # (the handle the (c) baseline of its route comes from: (c) says nothing here; (b) and (e) hold it to 3 x the oracle's distance like every case)
    V("f32_default", "f32_all", {}, ("f32_32x128", "attn_f32"), X3_ALL + CORES + FUSEDS + ("f32_64x128", "f32_128x128_bk16", "f32_128x128_bk32")),
    V("f32_64", "f32_all", {"big_min_rows": 1}, ("f32_64x128", "attn_f32"), X3_ALL + CORES + ("f32_32x128", "f32_128x128_bk16", "f32_128x128_bk32")),
    V("f32_128", "f32_all", {"big_min_rows": 1, "gemm_small_tiles": 0}, ("f32_128x128_bk16", "attn_f32"), X3_ALL + CORES + ("f32_32x128", "f32_64x128")),
    V("f32_128_nt", "f32_all", {"big_min_rows": 1, "gemm_small_tiles": 0, "store_nt": 1}, ("f32_128x128_bk16", "attn_f32"), X3_ALL + CORES + ("f32_32x128", "f32_64x128")),
    V("f32_gemm_split_core", "f32_gemm", {"big_min_rows": 1}, ("CORE", "f32_64x128"), X3_ALL + FUSEDS + ("attn_f32", "f32_32x128")),
]

# (id, route, options, sample / score keywords, must witness, must not reach)
SAMPLING_VARIANTS = [
    ("lanes2", "split", {"lanes": 2, "lane_min_rows": 2}, {}, ("sample_lanes_2", "tail_sliced"), ("sample_lanes_1", "sample_lanes_3", "sample_lanes_4")),
    ("lanes3", "split", {"lanes": 3, "lane_min_rows": 2}, {}, ("sample_lanes_3", "tail_sliced"), ("sample_lanes_1", "sample_lanes_2", "sample_lanes_4")),
    ("lanes4", "split", {"lanes": 4, "lane_min_rows": 2}, {}, ("sample_lanes_4", "tail_sliced"), ("sample_lanes_1", "sample_lanes_2", "sample_lanes_3")),
    ("tail_launches", "split", {"tail_form": 0}, {}, ("tail_launches", "value_via_rows"), ("tail_sliced", "value_via_projection")),
    ("tail_max_rows0", "split", {"tail_max_rows": 0}, {}, ("tail_launches", "value_via_rows"), ("tail_sliced", "value_via_projection")),
    ("value_projection", "split", {"prune_value_via_rows": 0}, {}, ("tail_launches", "value_via_projection"), ("tail_sliced", "value_via_rows")),
    ("loop_graph", "split", {"loop_graph": 1}, {}, ("loop_graph", "tail_sliced", "sample_lanes_1"), ("tail_launches", "value_via_projection", "sample_lanes_2")),
    ("no_prune", "split", {}, {"prune": False}, ("sample_lanes_1",), ("tail_sliced", "tail_launches", "value_via_rows", "value_via_projection")),
    ("one_lane_flag", "split", {"lane_min_rows": 2}, {"lanes": 1}, ("sample_lanes_1",), ("sample_lanes_2",)),
    # the fp32 128-row-tile family on a handful of rows: the step's full GEMMs, and (tail_form 0) the compact GEMMs of five rows
    ("f32_64", "f32_all", {"big_min_rows": 1}, {}, ("f32_64x128", "tail_sliced"), ("f32_32x128",) + X3_ALL),
    ("f32_64_tail_launches", "f32_all", {"big_min_rows": 1, "tail_form": 0}, {}, ("f32_64x128", "tail_launches"), ("f32_32x128", "tail_sliced") + X3_ALL),
    ("f32_128_tail_launches", "f32_all", {"big_min_rows": 1, "gemm_small_tiles": 0, "tail_form": 0}, {}, ("f32_128x128_bk16", "tail_launches"), ("f32_32x128", "f32_64x128") + X3_ALL),
]

# options no case above sets, and the test that covers them
ELSEWHERE = {
    "bn_chain": "tests/test_gpu_chain.py",
    "bn_chain_min_tiles": "tests/test_gpu_chain.py",
}
# kernel ids no case above can witness: the 32-deep fp32 128 x 128 tile is chosen by the HUDIFF_GEMM_BK environment variable (read once per
# process) or by a K that is no multiple of 16, which neither model has
UNREACHED = ("f32_128x128_bk32",)


def _names(kind, spec):
    out = []
    for n in spec:
        if isinstance(n, dict):
            out += list(n.get(kind, ()))
        else:
            out.append({"CORE": CORE[kind], "FUSED": FUSED[kind]}.get(n, n))
    return out


@pytest.fixture(scope="module")
def hip():
    import hudiff_amd
    if hudiff_amd.device_count() < 1:
        pytest.fail("no MI355X visible: GPU tests must run on the GPU box (there is no CPU fallback)")
    return hudiff_amd


def _model(hip, kind, cfg, sd, route, opts):
    cls = hip.AntiTFNet if kind == "ab" else hip.NanoAntiTFNet
    m = cls(**cfg, precision=route, options=opts)
    m.load_state_dict(sd)
    return m


def _weights(kind):
    from hudiff_amd import synthetic as S
    cfg = dict(S.AB_CONFIG if kind == "ab" else S.NB_CONFIG)              # (dropout > 0: the dropout epilogues are compiled in and case (e) runs them)
    assert cfg["dropout"] > 0
    return cfg, S.random_state_dict(kind, cfg, seed=3)


def _rows(kind, B):
    """B real rows with half of each row's masked slots filled from the truth (test_gpu_x3.py test_small_batches_...)."""
    from hudiff_amd import evalsets as E
    b = E.eval_batch("huab348" if kind == "ab" else "vhh", B, row0=17)
    tokens = b["tokens"].copy()
    for r in range(B):
        loc = b["order"][r, :b["T"][r] // 2]
        tokens[r, loc] = b["truth"][r, loc]
    return b, tokens


def _keys(kind, n_att):
    return (["aa_encoder", "pos"] + (["chn"] if kind == "ab" else []) + ["conv"] + [f"att{n}_at1" for n in range(n_att)] +
            [f"att{n}" for n in range(n_att)] + [f"att{n_att - 1}_at2", "logits"])


def _err(key, got, want):
    """Distance of a stage from the float64 trace: relative to the tensor's largest magnitude (test_gpu_components._close), absolute for logits."""
    assert got.shape == want.shape, (key, got.shape, want.shape)
    assert np.isfinite(got).all(), key
    err = float(np.abs(got.astype(np.float64) - want).max())
    return err if key.startswith("logits") else err / max(float(np.abs(want).max()), 1e-3)


def _measure(m, Y):
    """One handle against the float64 trace: ({stage: error}, logits, second call identical, logits under dropout)."""
    kind, (tok, reg, chn) = Y["kind"], Y["rows"]
    got = _stages(m, kind, tok, reg, chn, N_SEQ, Y["d"], Y["n_att"])
    errs = {k: _err(k, got[k], Y["t64"][k]) for k in Y["keys"]}
    again = m(tok, reg, chn, dropout="off")
    drop = m(tok, reg, chn, **DROP_KW)
    errs["logits_drop"] = _err("logits_drop", drop, Y["t64"]["logits_drop"])
    return errs, got["logits"], bool(np.array_equal(again, got["logits"])), drop


def _fmt(d):
    return " ".join(f"{k}={v:.2e}" for k, v in d.items())


@pytest.fixture(scope="module")
def yards(hip):
    """kind -> the yard-stick (module docstring), computed once on the CPU from the float64 and float32 oracle traces; and
    (kind, route) -> logits of the route's default-option handle."""
    cache = {}

    def yard(kind):
        if kind in cache:
            return cache[kind]
        cfg, sd = _weights(kind)
        b, tokens = _rows(kind, N_SEQ)
        rows = (tokens, b["region"], b["chain"])
        n_att = int(cfg["cs_layers"])
        keys = _keys(kind, n_att)
        drop = ho.Dropout("philox", seed=DROP_KW["seed"], rows=np.arange(N_SEQ) + DROP_KW["row0"], step=DROP_KW["step"])
        traces = {}
        for dt in (np.float64, np.float32):
            net = ho.OracleNet(kind, cfg, sd, dtype=dt)
            net.trace = {}
            logits = net(*rows)
            t = dict(net.trace, logits=logits)
            net.trace = None
            t["logits_drop"] = net(*rows, dropout=drop)
            traces[dt] = t
        t64 = traces[np.float64]
        e_ref = {k: _err(k, traces[np.float32][k], t64[k]) for k in keys + ["logits_drop"]}
        Y = dict(kind=kind, cfg=cfg, sd=sd, rows=rows, d=int(cfg["d_model"]), n_att=n_att, keys=keys, t64=t64, e_ref=e_ref, default_logits={})
        Y["bound"] = {k: min(MARGIN * v, LOGIT_CAP if k.startswith("logits") else STAGE_CAP) for k, v in e_ref.items()}
        print(f"\n[yard {kind}] e_ref {_fmt(e_ref)}\n[yard {kind}] bound {_fmt(Y['bound'])}")
        cache[kind] = Y
        return Y

    def default_logits(kind, route):
        Y = yard(kind)
        if route not in Y["default_logits"]:
            m = _model(hip, kind, Y["cfg"], Y["sd"], route, {})
            try:
                Y["default_logits"][route] = m(*Y["rows"], dropout="off")
            finally:
                m.close()
        return Y["default_logits"][route]

    return yard, default_logits


def _x3_total(t):
    return sum(t[n] for n in X3_ALL)


def _check_tally(tally, kind, expect, forbid, what):
    missing = [n for n in _names(kind, expect) if tally[n] <= 0]
    reached = [n for n in _names(kind, forbid) if tally[n] != 0]
    assert not missing and not reached, (what, "never launched:", missing, "launched but must not be:", reached, {k: v for k, v in tally.items() if v})


@pytest.mark.parametrize("kind,var", [(k, v) for v in FORWARD_VARIANTS for k in v["kinds"]],
                         ids=[f"{k}-{v['route']}-{v['id']}" for v in FORWARD_VARIANTS for k in v["kinds"]])
def test_forward_variant_vs_float64_oracle(hip, yards, kind, var):
    """One handle per (kind, route, options) row: conditions (a) .. (f) of the module docstring."""
    yard, default_logits = yards
    Y = yard(kind)
    base = default_logits(kind, var["route"])
    m = _model(hip, kind, Y["cfg"], Y["sd"], var["route"], var["opts"])
    try:
        assert {k: m.get_option(k) for k in var["opts"]} == var["opts"]
        m.debug_launch_tally()
        errs, logits, same, _ = _measure(m, Y)
        tally = m.debug_launch_tally()
        info = m.precision_info()
        layers = None
        if var["check"]:            # which LAYERS took split GEMMs: the ByteNet stacks alone (stage 2 = in front of the first attention block) against a whole forward
            tok, reg, chn = Y["rows"]
            m.debug_stop_after(2); m(tok, reg, chn, dropout="off")
            bytenet = _x3_total(m.debug_launch_tally())
            m.debug_stop_after(0); m(tok, reg, chn, dropout="off")
            layers = (bytenet, _x3_total(m.debug_launch_tally()))
    finally:
        m.close()
    e_def = float(np.abs(logits - base).max())
    print(f"\n[{kind} {var['route']} {var['id']}] errors {_fmt(errs)} | vs default {e_def:.2e} | repeat identical {same} | "
          f"x3 launches (ByteNet only, whole) {layers} | tally {({k: v for k, v in tally.items() if v})}")
    # (a) witness
    _check_tally(tally, kind, var["expect"], var["forbid"], var["id"])
    if var["check"] == "no_split_attention_gemm":
        assert layers[0] > 0 and layers[1] == layers[0], layers
    if var["check"] == "no_split_bytenet_gemm":
        assert layers[0] == 0 and layers[1] > 0, layers
    # (b) every stage against the float64 trace
    bad = {k: (errs[k], Y["bound"][k]) for k in Y["keys"] if not errs[k] <= Y["bound"][k]}
    assert not bad, ("stage error above 3 x yard-stick (error, bound), first stage first", bad)
    # (c) against the route's default options
    assert e_def <= DEFAULT_TOL, e_def
    # (d) repeatable
    assert same
    # (e) dropout epilogues
    assert errs["logits_drop"] <= Y["bound"]["logits_drop"], (errs["logits_drop"], Y["bound"]["logits_drop"])
    # (f) guards
    assert info["precision"] == var["route"] and info["range_fallbacks"] == 0 and info["lnsync_fallbacks"] == 0, info


@pytest.fixture(scope="module", params=["ab", "nb"])
def sampled(request, hip):
    """Five real rows, at most three steps, one row with none and one with two, sampled and scored by the default-option split
    handle; and the float64 log-probabilities of the drawn tokens from one oracle forward of the (row, step) expansion (11 rows)."""
    from hudiff_amd import scoring
    kind = request.param
    cfg, sd = _weights(kind)
    b, _ = _rows(kind, 5)
    T = np.minimum(b["T"], 3)
    T[1], T[3] = 0, 2
    order = np.ascontiguousarray(b["order"][:, :3])
    args = (b["region"], b["chain"], order, T)
    m = _model(hip, kind, cfg, sd, "split", {})
    try:
        tokens, logp = m.sample(b["tokens"], *args, seed=6, dropout="off", return_logp=True)
        score = m.score(tokens, *args, parallel=False)
        info = m.precision_info()
    finally:
        m.close()
    x = scoring.expand_steps(tokens, *args)
    assert x.tokens.shape[0] == int(T.sum()) <= 11
    lsm = log_softmax64(ho.OracleNet(kind, cfg, sd, dtype=np.float64)(x.tokens, x.region, x.chain)[:, :, :22])
    slot = x.order[:, 0]
    want = x.fold(lsm[np.arange(len(slot)), slot, tokens[x.rows, slot]], 3)
    return dict(kind=kind, cfg=cfg, sd=sd, start=b["tokens"], args=args, T=T, tokens=tokens, logp=logp, score=score, want=want, info=info)


def test_sampling_baseline_vs_float64_oracle(sampled):
    """The baseline of the sampling variants is itself within REF_TOL of the float64 oracle, recorded and scored."""
    s = sampled
    dead = np.arange(3)[None, :] >= s["T"][:, None]
    e_rec, e_score = float(np.abs(s["logp"] - s["want"]).max()), float(np.abs(s["score"] - s["want"]).max())
    print(f"\n[{s['kind']} sampling baseline] |recorded - float64| {e_rec:.2e}  |scored - float64| {e_score:.2e}")
    assert np.array_equal(s["tokens"][1], s["start"][1])                      # T = 0: untouched
    assert (s["logp"][dead] == 0).all() and (s["score"][dead] == 0).all() and (s["logp"][~dead] < 0).all()
    assert e_rec < REF_TOL and e_score < REF_TOL, (e_rec, e_score)
    assert s["info"]["range_fallbacks"] == 0 and s["info"]["lnsync_fallbacks"] == 0, s["info"]


@pytest.mark.parametrize("var", SAMPLING_VARIANTS, ids=[v[0] for v in SAMPLING_VARIANTS])
def test_sampling_variant_vs_default(hip, sampled, var):
    """Lanes, forms of the pruned tail, the loop graph, the full last block and the fp32 tile family on five rows: the baseline's
    tokens, its recorded and scored log-probabilities within PAIR_TOL, the witness in the tally, no guard."""
    name, route, opts, kw, expect, forbid = var
    s = sampled
    m = _model(hip, s["kind"], s["cfg"], s["sd"], route, opts)
    try:
        m.debug_launch_tally()
        tokens, logp = m.sample(s["start"], *s["args"], seed=6, dropout="off", return_logp=True, **kw)
        score = m.score(s["tokens"], *s["args"], parallel=False, **kw)
        tally = m.debug_launch_tally()
        info = m.precision_info()
    finally:
        m.close()
    e_rec, e_score = float(np.abs(logp - s["logp"]).max()), float(np.abs(score - s["score"]).max())
    print(f"\n[{s['kind']} {route} {name}] |recorded - default| {e_rec:.2e}  |scored - default| {e_score:.2e} | tally {({k: v for k, v in tally.items() if v})}")
    _check_tally(tally, s["kind"], expect, forbid + (() if "loop_graph" in expect else ("loop_graph",)), name)
    assert np.array_equal(tokens, s["tokens"]), name
    dead = np.arange(3)[None, :] >= s["T"][:, None]
    assert (logp[dead] == 0).all() and (score[dead] == 0).all()
    assert e_rec < PAIR_TOL and e_score < PAIR_TOL, (e_rec, e_score)
    assert info["precision"] == route and info["range_fallbacks"] == 0 and info["lnsync_fallbacks"] == 0, info
