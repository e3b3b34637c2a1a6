"""Constructions that hold every split-operand producer of the split route to its range guard ONE AT A TIME, and the weight guard of
the split weight images to its criterion (include/hudiff_hip.h "range guard", "weight guard").  A plain helper
module: tests/test_range_cases_host.py proves on the CPU that every case is what it claims, tests/test_gpu_range_sites.py runs the
cases on the device.

Part A.  Split operands are fp16 (hi, lo) pairs that are NOT scaled, so the route is valid while every value written in split form stays
below 65 504; whoever writes one checks it (absmax4 / raise_range_flag in hudiff_amd/csrc) and the call is repeated on the fp32 kernels.
A case bends the weights of a production-width, two-layer-per-stage model so that exactly ONE named producer meets an out-of-range value:
  dead channel   the outlier sits in one channel of a tensor that is not the residual stream (a LayerNorm beta, a projection bias) and the
                 consumer's weights for that channel are zero: the value vanishes right behind the site and the function is the one of the
                 same weights without the outlier;
  stop-after     the outlier sits in the residual stream (an output bias of a residual branch) and hd_debug_stop_after ends the forward
                 behind the first split copy of it (hd_forward still reads the guards after an early return).
SITES holds the constructions, FORMS the option sets that give a site another producer kernel or another epilogue instantiation, PAIRS
the (site, form) pairs that are run with the raise site each must reach (RAISE_SITES) and what must happen -- written down from the code
before anything ran on a device.  Every firing pair has a control (the same construction with the outlier at 2^14.5) and the sites whose
value is exact in fp32 pin the comparison itself: 65 504 fires, the float below it does not.

Part B.  X3Packer::add scales a whole weight matrix by one power of two; WEIGHT_CASES multiply one entry whose input channel is exactly
zero by 2^k, which leaves the function alone and takes significand bits off every ordinary entry of the image -- or makes the packer
refuse the image (weight_guard_holds mirrors its criterion).
"""
import functools
import math
from dataclasses import dataclass
from typing import Callable, Optional, Tuple

import numpy as np

import hudiff_oracle as ho

F32 = np.float32
LIMIT = F32(65504.0)                                   # X16_LIMIT (hd_kernels.hip.h): the largest finite fp16 number
BELOW = np.nextafter(LIMIT, F32(0))                    # 65503.996
CONTROL = F32(2.0 ** 14.5)                             # 23 170.475: in range, and still far above everything an ordinary row holds
OUT = F32(7.0e4)
OUT_QK = F32(2.0 ** 20)                                # Q is checked behind the rotation and the log2(e) / 8 scale: 2^20 -> 1.9e5
QS = 0.125 * 1.44269504088896340736                    # attn_x3_k / qkv_attn_x3_k
N_SEQ = 3
LOGIT_TOL, STAGE_TOL = 1e-4, 5e-5                      # tests/test_adversarial_golden.py, tests/test_gpu_components.py::_close
WEIGHT_KS = (8, 16, 24, 32)


def config(kind):
    """Production width, two layers per stage, no dropout."""
    from hudiff_amd import synthetic as S
    return dict(S.AB_CONFIG if kind == "ab" else S.NB_CONFIG, n_encoder_layers=2, dual_layers=2, cs_layers=2, dropout=0.0)


@functools.lru_cache(maxsize=None)
def base_weights(kind):
    """Shared: every user copies before it bends (bent, lane_case, weight_bent)."""
    from hudiff_amd import synthetic as S
    return S.random_state_dict(kind, config(kind), seed=3)


@functools.lru_cache(maxsize=None)
def rows(kind, B=N_SEQ):
    """B real rows with half of each row's masked slots filled from the truth (tests/test_gpu_variants.py::_rows)."""
    from hudiff_amd import evalsets as E
    b = E.eval_batch("huab348" if kind == "ab" else "vhh", B, row0=17)
    tokens = b["tokens"].copy()
    for r in range(B):
        loc = b["order"][r, :b["T"][r] // 2]
        tokens[r, loc] = b["truth"][r, loc]
    return b, tokens


# ---- where a split operand is written: one name per raise_range_flag in hudiff_amd/csrc -----------------------------------------------------
RAISE_SITES = {
    "ln_apply_k": "hd_kernels.hip.h ln_apply_k, split_out (HD_GUARD_MASK bit 2)",
    "epi.vmax": "hd_kernels.hip.h gemm_epilogue, store_out of a launch without a meeting: raise behind the row loop, conditioned on F (bit 1)",
    "epi.vmax_lnsync": "hd_kernels.hip.h gemm_epilogue, store_out behind the ln_sync meeting (bit 1)",
    "epi.smax": "hd_kernels.hip.h gemm_epilogue, second pass of an ln_sync launch: S = act(LN(row)) (no mask bit)",
    "attn_k.O": "hd_kernels.hip.h attn_k, o_split (bit 4)",
    "attn_x3_k.Q": "hd_kernels.hip.h attn_x3_k, Q fragments (bit 16)",
    "attn_x3_k.KV": "hd_kernels.hip.h attn_x3_k, K and V staging: one flag for both (bit 8)",
    "qkv.Q": "hd_attn_fused.hip.h qkv_attn_x3_k, Q hand-over (bit 16)",
    "qkv.KV": "hd_attn_fused.hip.h qkv_attn_x3_k, K (PART 1) and V (PART 2) hand-over (bit 8)",
    "chain.norm_split": "hd_chain.hip.h phase C, act(LN1(x)) in the operand path (no mask bit)",
    "chain.finish": "hd_chain.hip.h finish_ln_split: h2 behind phase A, h1 behind phase C (no mask bit)",
    "chain.epi_store": "hd_chain.hip.h phase B, X16 copy of the last block's output (no mask bit)",
    "chain.pair_a": "hd_chain.hip.h bn_pair_a_k (no mask bit)",
}
# raise sites no forward can reach, and why
UNREACHED = {
    "epi.vmax_lnsync": "no launch combines a meeting with a split copy: ln_sync launches are PFF1 and the tap GEMM (S is their only output) and a "
                       "PFF3 with a following block, while the split copy of a stack's output (C2) is asked of its LAST block, which has none",
    "chain.pair_a": "bn_pair_a_k is launched under #ifdef HD_CHAIN_EXPERIMENT only (a timing experiment; the shipped library does not hold the call)",
}
MASK_BITS = {1: ("epi.vmax",), 2: ("ln_apply_k",), 4: ("attn_k.O",), 8: ("attn_x3_k.KV", "qkv.KV"), 16: ("attn_x3_k.Q", "qkv.Q")}


# ---- bending ---------------------------------------------------------------------------------------------------------------------------
def bn_prefix(kind, stack, seg, n):
    root = "aa_encoder" if stack == "enc" else ("dual_conv_block" if kind == "ab" else "nano_conv_block")
    name = {"h": "h_layers", "l": "l_layers"}[seg] if kind == "ab" else "layers"
    return f"{root}.{name}.{n}."


def _ln_dead(sd, ln, c, consumer, v, exact):
    """LayerNorm `ln` (state-dict prefix without .weight / .bias): beta[c] = v (exact: gamma[c] = 0, the value is then v itself in every row);
    input channel c of the conv-shaped consumer weight [out, in, taps] zeroed."""
    sd[ln + ".bias"][c] = v
    if exact:
        sd[ln + ".weight"][c] = 0.0
    sd[consumer][:, c, :] = 0.0


def bend_s1(stack, seg, n, c):
    def f(sd, kind, v, exact=False):
        p = bn_prefix(kind, stack, seg, n)
        _ln_dead(sd, p + "sequence1.0", c, p + "sequence1.2.conv.weight", v, exact)
    return f


def bend_h1(stack, seg, n, c):
    def f(sd, kind, v, exact=False):
        p = bn_prefix(kind, stack, seg, n)
        _ln_dead(sd, p + "sequence1.3", c, p + "conv.weight", v, exact)
    return f


def bend_h2(stack, seg, n, c):
    def f(sd, kind, v, exact=False):
        p = bn_prefix(kind, stack, seg, n)
        _ln_dead(sd, p + "sequence2.0", c, p + "sequence2.2.conv.weight", v, exact)
    return f


def bend_ff1(n, j):
    def f(sd, kind, v, exact=False):
        p = f"self_at.layers.{n}."
        sd[p + "ff_hl.0.bias"][j] = v                  # unit j: zero weight row, so relu(0 + v) = v whatever the row (exact as it stands)
        sd[p + "ff_hl.0.weight"][j, :] = 0.0
        sd[p + "ff_hl.2.weight"][:, j] = 0.0
    return f


def bend_v(n, att, c):
    def f(sd, kind, v, exact=False):
        p = f"self_at.layers.{n}.{att}."
        sd[p + "value.bias"][c] = v
        if exact:
            sd[p + "value.weight"][c, :] = 0.0
        sd[p + "out_put.weight"][:, c] = 0.0
    return f


def bend_qk(n, att, c, which):
    """RoPE rotates the complex pairs (2k, 2k + 1) of a head (oracle apply_rope; the kernels index rope_cs by c4 >> 1 and rotate (v0, v1),
    (v2, v3)): the outlier of channel c spreads over both channels of its pair, so the OTHER operand is zeroed on both and no score moves."""
    mine, other = ("query", "key") if which == "q" else ("key", "query")

    def f(sd, kind, v, exact=False):
        p = f"self_at.layers.{n}.{att}."
        pair = [c & ~1, c | 1]
        sd[p + mine + ".bias"][c] = v
        sd[p + other + ".weight"][pair, :] = 0.0
        sd[p + other + ".bias"][pair] = 0.0
    return f


def bend_bias(key_of, c):
    def f(sd, kind, v, exact=False):
        sd[key_of(kind)][c] = v
    return f


@dataclass(frozen=True)
class Site:
    name: str
    bend: Callable
    probe: Callable                    # kind -> key of ProbeNet.peaks where the outlier shows
    value: float = float(OUT)
    dead: bool = True                  # dead-channel construction: the logits are those of the same weights without the outlier
    exact: bool = False                # the value at the site is exactly the parameter (gamma = 0 / zero weight row)
    stop: int = 0                      # hd_debug_stop_after stage of the stop-after constructions
    read: Optional[str] = None         # ... and the buffer compared instead of the logits
    also: Tuple[str, ...] = ()         # further probe suffixes that legitimately carry the outlier (see the site's comment)
    channel: int = 0


def _bn_site(stack, what, seg, n, c):
    bend = {"s1": bend_s1, "h1": bend_h1, "h2": bend_h2}[what](stack, seg, n, c)
    return Site(f"{stack}.{what}_b{n}", bend, lambda kind: bn_prefix(kind, stack, seg, n) + what, exact=True, channel=c)


LAST = 1                               # index of the last block of every two-layer stage
SITES = [
    # ByteNet operands (act(LN(.)) in split form).  Antibody: about half of them in the light chain's weights, so that only segment 1's tiles see
    # the outlier.  s1_b0 is written by ln_apply_k (the stack's input has no GEMM producer of this kind), s1_b1 by block 0's PFF3 (level 2).
    _bn_site("enc", "s1", "h", 0, 133), _bn_site("enc", "s1", "l", 1, 41), _bn_site("enc", "h1", "h", 0, 77), _bn_site("enc", "h2", "l", 1, 5),
    _bn_site("conv", "s1", "l", 0, 301), _bn_site("conv", "s1", "h", 1, 470), _bn_site("conv", "h1", "l", 0, 201), _bn_site("conv", "h2", "h", 1, 66),
    # attention blocks
    Site("ff1", bend_ff1(0, 130), lambda kind: "self_at.layers.0.ff1", exact=True, channel=130),
    # V: O is a convex combination of the V rows, so channel c of O carries the outlier as well (attn_x3_k does not check O for that reason;
    # attn_k, which reads fp32 Q | K | V, checks the split O it writes and nothing else)
    Site("v", bend_v(0, "attn_hl", 203), lambda kind: "self_at.layers.0.attn_hl.v", exact=True, also=("self_at.layers.0.attn_hl.o",), channel=203),
    Site("q", bend_qk(0, "attn_hl", 90, "q"), lambda kind: "self_at.layers.0.attn_hl.q", value=float(OUT_QK), channel=90),
    Site("k", bend_qk(LAST, "attn_hl_c", 333, "k"), lambda kind: f"self_at.layers.{LAST}.attn_hl_c.k", value=float(OUT_QK), channel=333),
    # split copies of the raw residual stream
    Site("yx_conv", bend_bias(lambda kind: bn_prefix(kind, "conv", "l", LAST) + "sequence2.2.conv.bias", 257), lambda kind: "conv_out",
         dead=False, stop=2, read="Y", channel=257),
    Site("atx_a1", bend_bias(lambda kind: "self_at.layers.0.attn_hl.out_put.bias", 12), lambda kind: "self_at.layers.0.at1",
         dead=False, stop=100, read="AT", channel=12),
    Site("yx_ff2", bend_bias(lambda kind: "self_at.layers.0.ff_hl.2.bias", 399), lambda kind: "self_at.layers.0.out",
         dead=False, stop=3, read="Y", channel=399),
    # the second attention of the LAST block writes at2 in split form only (c_split).  The whole forward runs: FF1 reads at2 through the folded
    # LayerNorm (its output is normalised), the block's last residual comes from the block INPUT (forward_body: p.resid = ws.Y), and behind the
    # last block only the decoder follows -- no later raw-stream copy sees the outlier (ProbeNet confirms it stage by stage)
    Site("atx_a2", bend_bias(lambda kind: f"self_at.layers.{LAST}.attn_hl_c.out_put.bias", 500), lambda kind: f"self_at.layers.{LAST}.at2",
         dead=False, channel=500),
]
SITE = {s.name: s for s in SITES}


def bent(kind, site, v, exact=False, sd=None):
    sd = {k: a.copy() for k, a in (sd or base_weights(kind)).items()}
    site.bend(sd, kind, F32(v), exact)
    return sd


# ---- kernel forms ----------------------------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class Form:
    name: str
    opts: dict
    gemm: Tuple[str, ...] = ()         # launch-tally names a ByteNet stack + attention GEMMs must show (tests/test_gpu_variants.py)
    attn: Tuple[str, ...] = ()         # ... and a run that reaches the attention core ("CORE" / "FUSED": the kind's kernel)
    forbid: Tuple[str, ...] = ()
    route: str = "split"
    ab_opts: Optional[dict] = None     # antibody only

    def options(self, kind):
        return dict(self.opts, **(self.ab_opts or {})) if kind == "ab" else dict(self.opts)


_CONV = tuple(n + "_conv" for n in ("x3_256x256_s2", "x3_256x128_s3", "x3_128x128_plain", "x3_128x128_lnsync", "x3_64x128_s2", "x3_64x128_s3",
                                    "x3_32x128_s2", "x3_32x128_s3", "x3_32x128_s3_loaders"))
FORMS = [
    Form("default", {}, ("x3_32x128_s3_loaders", "x3_32x128_s3_loaders_conv"), ("CORE", "attn_qsplit"), ("qkv_attn_19", "qkv_attn_10")),
    Form("big", {"small_grid": 0}, ("x3_128x128_plain", "x3_128x128_lnsync", "x3_128x128_lnsync_conv"), ("CORE",)),
    Form("s64", {"tiny_grid": 0}, ("x3_64x128_s3", "x3_64x128_s3_conv"), ("CORE",)),
    Form("ln1", {"lnsync_level": 1}, ("x3_32x128_s3_loaders", "x3_32x128_s3_loaders_conv"), ("CORE",)),
    Form("ln0", {"lnsync_level": 0}, ("x3_32x128_s3_loaders", "x3_32x128_s3_loaders_conv"), ("CORE",)),
    Form("t256", {"split_tile": 256, "lnsync_level": 0}, ("x3_256x128_s3", "x3_256x128_s3_conv"), ("CORE",)),
    Form("t512", {"split_tile": 512, "lnsync_level": 0}, ("x3_256x256_s2",), ("CORE",)),
    Form("fused", {"fused_attn_min_grid": 0}, (), ("FUSED",), ("attn_x3_19_w12", "attn_x3_19_w8", "attn_x3_10")),
    Form("two", {"fused_attn": 0, "attn_qsplit_max_grid": 0}, (), ("CORE",), ("attn_qsplit", "qkv_attn_19", "qkv_attn_10"), ab_opts={"attn_waves": 8}),
    Form("f32core", {"split_attn": 0}, ("x3_32x128_s3_loaders",), ("attn_f32",), ("attn_x3_19_w12", "attn_x3_19_w8", "attn_x3_10", "qkv_attn_19", "qkv_attn_10")),
    Form("f32gemm", {"big_min_rows": 1}, ("f32_64x128",), ("CORE",), ("qkv_attn_19", "qkv_attn_10"), route="f32_gemm"),
    # (the chain kernel has no tally entry: its witness is that no tap GEMM was launched although the ByteNet stacks ran split)
    Form("chain", {"bn_chain": 3, "bn_chain_min_tiles": 0}, (), ("CORE",), _CONV),
    Form("mask2", {"split_layer_mask": 2}, ("f32_32x128",), ("CORE",), _CONV),
]
FORM = {f.name: f for f in FORMS}
CORE = {"ab": "attn_x3_19_w12", "nb": "attn_x3_10"}
FUSED = {"ab": "qkv_attn_19", "nb": "qkv_attn_10"}


def witness(form, kind, site):
    """(must show, must not show) in the launch tally of a run of `site` under `form`.  The tally adds up both attempts of a repeated call; the
    repeat launches fp32 kernels only, so a split kernel in it ran in the first attempt and no fp32 kernel is ever in `must not show`."""
    core = "attn_x3_19_w8" if (kind == "ab" and form.name == "two") else CORE[kind]
    names = list(form.gemm)
    if site.stop == 0 or site.stop >= 100:
        names += [{"CORE": core, "FUSED": FUSED[kind]}.get(n, n) for n in form.attn]
    return tuple(names), form.forbid


# ---- (site, form) -> raise site, outcome ------------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class Pair:
    site: str
    form: str
    raises: Optional[str]              # RAISE_SITES key the outlier must reach; None: nobody splits the value under this form
    kinds: Tuple[str, ...] = ("ab",)
    fire: bool = True


def _pairs():
    P, both = [], ("ab", "nb")
    # ByteNet operands.  Levels 2 / 1: the producing GEMM's second pass (smax) on whatever tile the grid takes; level 0: ln_apply_k; the first
    # operand of a stack always ln_apply_k; level 1: the next block's first operand from ln_apply_k again.  Full matrix on the antibody's
    # Dual stack; its token encoder under default, chain, big and ln0 (both tile families of the meeting epilogue and ln_apply_k; s64, ln1, t256
    # and t512 would run the very instantiations the Dual stack's pairs run, chosen by the same launch_gemm on the same grid rule, at N = 128 /
    # 256 instead of 384 / 768); default (+ chain for the conv stack) on the nanobody.
    for st in ("enc", "conv"):
        nb_chain = both if st == "conv" else ("ab",)
        P += [Pair(f"{st}.s1_b0", "default", "ln_apply_k", both), Pair(f"{st}.s1_b0", "chain", "chain.norm_split", nb_chain),
              Pair(f"{st}.s1_b1", "default", "epi.smax", both), Pair(f"{st}.s1_b1", "chain", "chain.norm_split", nb_chain),
              Pair(f"{st}.h1_b0", "default", "epi.smax", both), Pair(f"{st}.h1_b0", "chain", "chain.finish", nb_chain),
              Pair(f"{st}.h2_b1", "default", "epi.smax", both), Pair(f"{st}.h2_b1", "chain", "chain.finish", nb_chain)]
    P += [Pair("conv.s1_b0", "ln0", "ln_apply_k")]
    P += [Pair("enc.s1_b0", f, "ln_apply_k") for f in ("big", "ln0")] + [Pair(f"enc.{s}", "ln0", "ln_apply_k") for s in ("s1_b1", "h1_b0", "h2_b1")]
    P += [Pair(f"enc.{s}", "big", "epi.smax") for s in ("s1_b1", "h1_b0", "h2_b1")]
    P += [Pair("conv.s1_b1", f, "epi.smax") for f in ("big", "s64")] + [Pair("conv.s1_b1", f, "ln_apply_k") for f in ("ln1", "ln0")]
    P += [Pair("conv.h1_b0", f, "epi.smax") for f in ("big", "s64")] + [Pair("conv.h1_b0", f, "ln_apply_k") for f in ("ln0", "t256")]
    P += [Pair("conv.h2_b1", f, "epi.smax") for f in ("big", "s64")] + [Pair("conv.h2_b1", "ln0", "ln_apply_k")]
    # GEMM epilogues that write a split copy (C2) or split rows only (c_split): one instantiation per tile shape and feature set
    # (RESID | PART | C2: yx_conv, atx_a1, yx_ff2; RESID | PART | CSPLIT: atx_a2; FOLD | ACT | CSPLIT: ff1)
    P += [Pair("yx_conv", "default", "epi.vmax", both), Pair("yx_conv", "chain", "chain.epi_store", both)]
    P += [Pair("yx_conv", f, "epi.vmax") for f in ("big", "s64", "t256", "t512")]
    # ByteNet stacks on the fp32 GEMMs beside split attention blocks (split_layer_mask 2; what a ByteNet image refused by the weight guard gives
    # as well): the fp32 gemm_k of the conv stack's last block writes the YX copy through the same gemm_epilogue
    P += [Pair("yx_conv", "mask2", "epi.vmax", both)]
    P += [Pair("atx_a1", "default", "epi.vmax", both)] + [Pair("atx_a1", f, "epi.vmax") for f in ("big", "s64", "t256", "t512")]
    P += [Pair("atx_a2", "default", "epi.vmax", both)] + [Pair("atx_a2", f, "epi.vmax") for f in ("big", "s64", "t256", "t512")]
    P += [Pair("ff1", "default", "epi.vmax", both)] + [Pair("ff1", f, "epi.vmax") for f in ("big", "s64", "t256", "t512")]
    P += [Pair("yx_ff2", "default", "epi.vmax", both)] + [Pair("yx_ff2", f, "epi.vmax") for f in ("big", "s64", "t256", "t512")]
    # attention core.  split_attn 0: attn_k reads fp32 Q | K | V and checks the split O it writes -- a Q or K outlier meets no split at all and
    # the handle must stay on the split route with a correct result; a V outlier reaches O
    for s, r in (("q", "Q"), ("k", "KV")):
        P += [Pair(s, "default", f"attn_x3_k.{r}", both), Pair(s, "fused", f"qkv.{r}", both), Pair(s, "two", f"attn_x3_k.{r}"),
              Pair(s, "f32gemm", f"attn_x3_k.{r}"), Pair(s, "f32core", None, both if s == "q" else ("ab",), fire=False)]
    P += [Pair("v", "default", "attn_x3_k.KV", both), Pair("v", "fused", "qkv.KV", both), Pair("v", "two", "attn_x3_k.KV"),
          Pair("v", "f32core", "attn_k.O", both)]
    return P


PAIRS = _pairs()
# exact threshold: 65 504 must fire, the float below must not -- at every raise site a value reaches unchanged
EXACT_PAIRS = [Pair("conv.s1_b0", "default", "ln_apply_k", ("ab", "nb")), Pair("enc.s1_b0", "default", "ln_apply_k"),
               Pair("conv.s1_b1", "default", "epi.smax"), Pair("enc.s1_b1", "default", "epi.smax"),
               Pair("conv.h1_b0", "default", "epi.smax", ("ab", "nb")), Pair("enc.h1_b0", "default", "epi.smax"),
               Pair("conv.h2_b1", "default", "epi.smax"), Pair("enc.h2_b1", "default", "epi.smax"),
               Pair("ff1", "default", "epi.vmax", ("ab", "nb")), Pair("v", "default", "attn_x3_k.KV", ("ab", "nb")), Pair("v", "fused", "qkv.KV"),
               Pair("conv.s1_b0", "chain", "chain.norm_split"), Pair("conv.h1_b0", "chain", "chain.finish")]


def expanded(pairs):
    return [(k, p) for p in pairs for k in p.kinds]


# ---- what every producer of the network sees: the oracle with a peak recorder ----------------------------------------------------------------
class ProbeNet(ho.OracleNet):
    """OracleNet that records max |x| of every tensor the split route writes in split form, in forward order, under the state-dict prefix
    of its producer: <bytenet block>s1 / h1 / h2, conv_out (YX), <attention>q (rotated, x log2(e) / 8) / k (rotated) / v / o, and per block
    at1 (ATX), at2 (ATX, c_split), ff1, out (YX)."""

    def __init__(self, *a, **k):
        super().__init__(*a, **k)
        self.peaks = {}

    def _peak(self, key, x):
        self.peaks[key] = max(self.peaks.get(key, 0.0), float(np.abs(x).max()))

    def _bytenet_block(self, x, pre, dil, act):
        s = self.sd
        h = act(ho.layer_norm(x, s[pre + "sequence1.0.weight"], s[pre + "sequence1.0.bias"]))
        self._peak(pre + "s1", h)
        h = ho.linear(h, s[pre + "sequence1.2.conv.weight"][:, :, 0], s[pre + "sequence1.2.conv.bias"])
        h = act(ho.layer_norm(h, s[pre + "sequence1.3.weight"], s[pre + "sequence1.3.bias"]))
        self._peak(pre + "h1", h)
        h = ho.dilated_conv(h, s[pre + "conv.weight"], s[pre + "conv.bias"], dil)
        h = act(ho.layer_norm(h, s[pre + "sequence2.0.weight"], s[pre + "sequence2.0.bias"]))
        self._peak(pre + "h2", h)
        h = ho.linear(h, s[pre + "sequence2.2.conv.weight"][:, :, 0], s[pre + "sequence2.2.conv.bias"])
        return x + h

    def _attn(self, x, pre):
        s = self.sd
        B, L, _ = x.shape
        H, hd = self.nhead, self.att // self.nhead
        q = ho.linear(x, s[pre + "query.weight"], s[pre + "query.bias"]).reshape(B, L, H, hd)
        k = ho.linear(x, s[pre + "key.weight"], s[pre + "key.bias"]).reshape(B, L, H, hd)
        v = ho.linear(x, s[pre + "value.weight"], s[pre + "value.bias"]).reshape(B, L, H, hd)
        q, k = ho.apply_rope(q, self.cos, self.sin), ho.apply_rope(k, self.cos, self.sin)
        self._peak(pre + "q", q * self.dt(QS)); self._peak(pre + "k", k); self._peak(pre + "v", v)
        q, k, v = (t.transpose(0, 2, 1, 3) for t in (q, k, v))
        w = (q @ k.transpose(0, 1, 3, 2)) / self.dt(math.sqrt(hd))
        w = np.exp(w - w.max(axis=-1, keepdims=True))
        w = w / w.sum(axis=-1, keepdims=True, dtype=self.dt)
        o = (w @ v).transpose(0, 2, 1, 3).reshape(B, L, H * hd)
        self._peak(pre + "o", o)
        return ho.linear(o, s[pre + "out_put.weight"], s[pre + "out_put.bias"])

    def _self_att_block(self, x, n):
        s = self.sd
        pre = f"self_at.layers.{n}."
        if n == 0:
            self._peak("conv_out", x)
        at = x + self._attn(x, pre + "attn_hl.")
        self._peak(pre + "at1", at)
        at = at + self._attn(ho.layer_norm(at, s[pre + "norm_hl1.weight"], s[pre + "norm_hl1.bias"]), pre + "attn_hl_c.")
        self._peak(pre + "at2", at)
        f = ho.layer_norm(at, s[pre + "norm_hl2.weight"], s[pre + "norm_hl2.bias"])
        f = ho.relu(ho.linear(f, s[pre + "ff_hl.0.weight"], s[pre + "ff_hl.0.bias"]))
        self._peak(pre + "ff1", f)
        out = ho.linear(f, s[pre + "ff_hl.2.weight"], s[pre + "ff_hl.2.bias"]) + x
        self._peak(pre + "out", out)
        return out


def peaks(kind, sd, dtype=F32):
    """-> (ordered {producer: max |x|}, logits) of the three test rows."""
    b, tokens = rows(kind)
    net = ProbeNet(kind, config(kind), sd, dtype=dtype)
    logits = net(tokens, b["region"], b["chain"])
    return net.peaks, logits


def ran_until(site, kind, pk):
    """The producers a run of `site` reaches, in order: all of them, or those up to the site's own (the stop-after stage lies right behind it)."""
    keys = list(pk)
    return keys if site.stop == 0 else keys[:keys.index(site.probe(kind)) + 1]


# ---- two-lane session ------------------------------------------------------------------------------------------------------------------
LANE_TOKEN = 20                        # 'X': in no evaluation row
LANE_SCALE = F32(2.0 ** 16)


def lane_case(kind):
    """B = 4, T = 2: token 20, whose embedding row is scaled by 2^16, in ONE sequence of the second lane (row 3), at a slot the steps do not
    visit.  The raw stream of that sequence alone passes the range (first split copy: the conv stack's YX) -> (weights, batch with and without it)."""
    sd = {k: a.copy() for k, a in base_weights(kind).items()}
    sd["aa_encoder.embedder.weight"][LANE_TOKEN] *= LANE_SCALE
    b, tokens = rows(kind, 4)
    assert not (tokens == LANE_TOKEN).any()
    T = np.minimum(b["T"], 2).astype(b["T"].dtype)
    order = np.ascontiguousarray(b["order"][:, :2])
    free = [s for s in range(tokens.shape[1]) if tokens[3, s] < 20 and s not in set(order[3].tolist())]
    hot = tokens.copy()
    hot[3, free[len(free) // 2]] = LANE_TOKEN
    return sd, dict(region=b["region"], chain=b["chain"], order=order, T=T, clean=tokens, hot=hot)


# ---- Part B: weight dynamic range ------------------------------------------------------------------------------------------------------
def _w_pff1(sd, kind, k):
    p, c, o = bn_prefix(kind, "conv", "h", 0), 97, 11
    sd[p + "sequence1.0.weight"][c] = 0.0
    sd[p + "sequence1.0.bias"][c] = 0.0                # act(0) = 0 for ReLU and GELU: input channel c of PFF1 is exactly zero
    w = sd[p + "sequence1.2.conv.weight"]
    w[o, c, 0] = np.abs(w).max() * F32(2.0 ** k)
    stacked = [sd[bn_prefix(kind, "conv", s, 0) + "sequence1.2.conv.weight"] for s in (("h", "l") if kind == "ab" else ("h",))]
    return stacked                                     # what one X3Packer::add call sees (one scale for both chains' matrices)


def _w_ff2(sd, kind, k):
    p, j, o = "self_at.layers.0.", 77, 300
    sd[p + "ff_hl.0.weight"][j, :] = 0.0
    sd[p + "ff_hl.0.bias"][j] = -1.0                   # relu(-1) = 0
    w = sd[p + "ff_hl.2.weight"]
    w[o, j] = np.abs(w).max() * F32(2.0 ** k)
    return [w]


def _w_wo(sd, kind, k):
    p, c, o = "self_at.layers.0.attn_hl.", 140, 201
    sd[p + "value.weight"][c, :] = 0.0
    sd[p + "value.bias"][c] = 0.0                      # V[:, c] = 0, so O[:, c] = 0
    w = sd[p + "out_put.weight"]
    w[o, c] = np.abs(w).max() * F32(2.0 ** k)
    return [w]


# name -> (bend, family whose split images the weight guard takes off the split kernels: 1 ByteNet stacks, 2 attention blocks)
WEIGHT_CASES = {"pff1": (_w_pff1, 1), "ff2": (_w_ff2, 2), "wo": (_w_wo, 2)}


def weight_bent(kind, name, k):
    """All three zero-input constructions at once, the entry of matrix `name` at 2^k times that matrix's largest |w| and the other two at
    2^0: one unbent function (k = 0) serves every (name, k).  -> (state dict, the arrays of `name`'s split image)."""
    sd = {key: a.copy() for key, a in base_weights(kind).items()}
    arrays = None
    for other, (bend, _) in WEIGHT_CASES.items():
        got = bend(sd, kind, k if other == name else 0)
        arrays = got if other == name else arrays
    return sd, arrays


def weight_guard_holds(arrays):
    """X3Packer::add's criterion on the matrices of one image: scaled so that the largest |w| lands in [2^13, 2^14), every entry's
    fp16 (hi, lo) pair is within 2^-22 of the entry or, where that is larger, of the median |w| of the non-zero entries."""
    w = np.concatenate([np.asarray(a, F32).ravel() for a in arrays])
    mx = float(np.abs(w).max())
    if mx == 0.0:
        return True
    sc = F32(2.0 ** (14 - math.frexp(mx)[1]))
    v = w * sc
    with np.errstate(over="ignore"):
        hi = v.astype(np.float16).astype(F32)
        lo = (v - hi).astype(np.float16).astype(F32)
    err = np.abs(v.astype(np.float64) - (hi.astype(np.float64) + lo.astype(np.float64)))
    a = np.abs(w[w != 0])
    med = float(np.partition(a, a.size // 2)[a.size // 2]) * float(sc)
    return bool((err <= 2.0 ** -22 * np.maximum(np.abs(v).astype(np.float64), med)).all())
