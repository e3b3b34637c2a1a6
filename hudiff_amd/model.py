"""Host-side mirror of the reference's model-call boundary, backed by libhudiff_hip.so.

Reference interface mirrored (file:line under /root/reference):
  * ``AntiTFNet(**config.model)`` / ``NanoAntiTFNet(**config.model)``   model/encoder/model.py:325-349,
    model/nanoencoder/model.py:290-311 -- same constructor keywords
  * ``model_selected(config)``                                          utils/train_utils.py:43-55
  * ``model.load_state_dict(ckpt['model'])`` / ``.eval()`` / ``.to(device)``   antibody_scripts/sample.py:456-458
  * ``model(H_L_seq, H_L_region_type, H_L_chn_type) -> logits[B, L, n_tokens]``  model/encoder/model.py:366-384
so the reference-shaped loop (sample.py:499-513) can drive it unchanged; ``.sample`` runs the whole loop
on the device (hd_sample).  torch is used only to read checkpoints / to hand tensors back in the
caller's type -- no torch op is on the hot path.
"""
from __future__ import annotations

import ctypes as C
from typing import Mapping, Optional

import numpy as np

from . import _lib as L

_ACT = {"relu": L.HD_ACT_RELU, "gelu": L.HD_ACT_GELU}
AB_H_LEN = 152


def _get(cfg, key, default=None):
    if isinstance(cfg, Mapping):
        return cfg.get(key, default)
    return getattr(cfg, key, default)


def _tau(confidence):
    """A confidence threshold as hd_set_confidence takes it (ValueError outside [0, 1])."""
    from .guide import confidence_tau
    return confidence_tau(confidence)


def _to_numpy(x):
    if x is None:
        return None, False
    if hasattr(x, "detach") and hasattr(x, "cpu"):       # torch.Tensor without importing torch
        return x.detach().cpu().numpy(), True
    return np.asarray(x), False


def _sinusoid_pe(max_len, d_model):
    f32 = np.float32
    position = np.arange(max_len, dtype=f32)[:, None]
    div = np.exp(np.arange(0, d_model, 2).astype(f32) * f32(-np.log(10000.0) / d_model)).astype(f32)
    ang = (position * div).astype(f32)
    pe = np.zeros((max_len, d_model), dtype=f32)
    pe[:, 0::2], pe[:, 1::2] = np.sin(ang), np.cos(ang)
    return pe


def _rope_table(head_dim, length, theta=10000.0):
    f32 = np.float32
    freqs = (f32(1.0) / (f32(theta) ** (np.arange(0, head_dim, 2)[: head_dim // 2].astype(f32) / f32(head_dim)))).astype(f32)
    ang = np.outer(np.arange(length, dtype=f32), freqs).astype(f32)
    return np.stack([np.cos(ang), np.sin(ang)], axis=-1).astype(f32)


class _Denoiser:
    kind = None            # 'ab' | 'nb'

    def __init__(self, n_tokens, d_embedding, d_model, n_encoder_layers, aa_kernel_size, r,
                 n_region, r_embedding, r_model, n_pos_model, max_len, sum_d_model, dual_layers,
                 att_model, dim_feedforward, nhead, cs_layers, n_side=3, s_embedding=4, s_model=None,
                 rank=None, n_frozen_embs=None, padding_idx=None, causal=False, dropout=0.0, slim=True,
                 activation="relu", down_embed=False, timesteps=None, device=0, precision=None, options=None):
        if rank is not None or n_frozen_embs is not None or causal or not slim or down_embed or padding_idx is not None:
            raise NotImplementedError("only the configuration HuDiff ships (rank=None, causal=False, slim=True, "
                                      "down_embed=False, padding_idx=None) is implemented")
        if not (d_embedding == d_model == r_model == n_pos_model) or (s_model not in (None, d_model)):
            raise ValueError("d_embedding, d_model, r_model, n_pos_model (and s_model) must be equal")
        self.config = dict(n_tokens=n_tokens, d_embedding=d_embedding, d_model=d_model,
                           n_encoder_layers=n_encoder_layers, aa_kernel_size=aa_kernel_size, r=r,
                           n_region=n_region, r_embedding=r_embedding, r_model=r_model, n_pos_model=n_pos_model,
                           max_len=max_len, sum_d_model=sum_d_model, dual_layers=dual_layers, att_model=att_model,
                           dim_feedforward=dim_feedforward, nhead=nhead, cs_layers=cs_layers, dropout=float(dropout),
                           activation=activation)
        if self.kind == "ab":
            self.config.update(n_side=n_side, s_embedding=s_embedding, s_model=d_model)
        c = L.HdConfig()
        c.abi_version = L.HD_ABI_VERSION
        c.kind = L.HD_KIND_ANTIBODY if self.kind == "ab" else L.HD_KIND_NANOBODY
        c.n_tokens, c.max_len = n_tokens, max_len
        c.h_len = AB_H_LEN if self.kind == "ab" else max_len
        c.d_model, c.sum_d_model = d_model, sum_d_model
        c.n_encoder_layers, c.dual_layers, c.kernel_size, c.r = n_encoder_layers, dual_layers, aa_kernel_size, r
        c.att_model, c.nhead, c.dim_feedforward, c.cs_layers = att_model, nhead, dim_feedforward, cs_layers
        c.n_region, c.r_embedding = n_region, r_embedding
        c.n_side, c.s_embedding = (n_side, s_embedding) if self.kind == "ab" else (0, 0)
        c.enc_act = _ACT[activation]
        # DualConv is constructed with its default activation='relu' (model/encoder/model.py:345),
        # NanoConv with its default 'gelu' (model/nanoencoder/model.py:242, 308)
        c.conv_act = L.HD_ACT_RELU if self.kind == "ab" else L.HD_ACT_GELU
        c.dropout = float(dropout)
        self._cfg = c
        self.max_len, self.n_tokens = max_len, n_tokens
        self._lib = L.load()
        self._h = C.c_void_p()
        L.check(self._lib.hd_create(C.byref(c), int(device), C.byref(self._h)))
        # precision route (include/hudiff_hip.h "precision routes"; not a keyword of the reference's constructor, which computes in
        # fp32 on whatever torch gives it): None / "default" = the library default (split precision; the environment may override
        # the default), "split" | "f32_gemm" | "f32_all" = that route whatever the environment says
        if precision is not None:
            if precision not in L.PRECISIONS:
                raise ValueError(f"precision must be one of {sorted(L.PRECISIONS)}, got {precision!r}")
            L.check(self._lib.hd_set_precision(self._h, L.PRECISIONS[precision]))
        self._loaded = False
        self._seen_fallbacks = (0, 0)
        self.device_index = int(device)
        # tuning options (include/hudiff_hip.h "tuning options"): {name: value}, e.g. {"lanes": 1, "lnsync_level": 0}
        for k, v in (options or {}).items():
            self.set_option(k, v)

    # -- tuning options (hd_set_option / hd_get_option) --------------------------------------------
    @staticmethod
    def _option_id(name):
        if isinstance(name, str):
            key = name.lower().removeprefix("hd_opt_")
            if key not in L.OPTIONS:
                raise ValueError(f"unknown option {name!r}; known: {sorted(L.OPTIONS)}")
            return L.OPTIONS[key]
        return int(name)

    def set_option(self, name, value):
        """An explicit choice of a kernel-selecting knob; wins over the HUDIFF_* environment variable of the same meaning."""
        L.check(self._lib.hd_set_option(self._h, self._option_id(name), int(value)))
        return self

    def get_option(self, name):
        v = C.c_int64()
        L.check(self._lib.hd_get_option(self._h, self._option_id(name), C.byref(v)))
        return int(v.value)

    def options(self):
        return {n: self.get_option(i) for n, i in L.OPTIONS.items()}

    # -- nn.Module-shaped surface ---------------------------------------------------------------
    def load_state_dict(self, state_dict, strict=True):
        if self._loaded:
            raise RuntimeError("weights already loaded into this handle")
        if not strict:
            raise NotImplementedError("strict=False is not supported")
        keys = set()
        for key, val in state_dict.items():
            arr, _ = _to_numpy(val)
            if np.iscomplexobj(arr):             # '...rope' complex64 [L, hd/2] -> float32 [L, hd/2, 2]
                arr = np.stack([arr.real, arr.imag], axis=-1)
            self._load(key, arr)
            keys.add(key[7:] if key.startswith("module.") else key)
        # Buffers a stripped state_dict may lack: built the way torch builds them (float32 arithmetic),
        # model/encoder/model.py:70-78 and model/encoder/cross_attention.py:35-56.
        if "pos_encoder.pos_embedding.pe" not in keys:
            self._load("pos_encoder.pos_embedding.pe", _sinusoid_pe(self.max_len, self.config["d_model"])[:, None, :])
        if not any(k.endswith(".rope") for k in keys):
            self._load("self_at.layers.0.attn_hl.rope",
                       _rope_table(self.config["att_model"] // self.config["nhead"], self.max_len))
        L.check(self._lib.hd_finalize(self._h))
        self._loaded = True
        return self

    def _load(self, key, arr):
        arr = np.ascontiguousarray(arr, dtype=np.float32)
        shape = (C.c_int64 * max(arr.ndim, 1))(*arr.shape)
        L.check(self._lib.hd_load_tensor(self._h, key.encode(), L.ptr(arr, C.c_float), shape, arr.ndim))

    def eval(self):
        return self

    def to(self, *a, **k):
        return self

    def close(self):
        if getattr(self, "_h", None) is not None and self._h:
            self._lib.hd_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _warn_on_guard(self):
        """A guard of the split-precision kernels repeated the last call on safer kernels (results are correct; the handle is slower
        from here on until precision_reset()): say so once per event -- the C library only counts it (hd_precision_report)."""
        r = L.HdPrecisionInfo()
        if self._lib.hd_precision_report(self._h, C.byref(r), C.sizeof(r)) != L.HD_OK:
            return
        now = (int(r.range_fallbacks), int(r.lnsync_fallbacks))
        if now != self._seen_fallbacks:
            import warnings
            what = []
            if now[0] > self._seen_fallbacks[0]:
                what.append("an activation left the fp16 range (|x| >= 65504): the call was repeated on the all-fp32 kernels and the handle stays on them")
            if now[1] > self._seen_fallbacks[1]:
                what.append("an ln_sync meeting failed: the call was repeated with separate LayerNorm passes and the handle keeps them")
            self._seen_fallbacks = now
            warnings.warn("hudiff_amd: " + "; ".join(what) + " (precision_info(); precision_reset() re-arms the split kernels)", RuntimeWarning, stacklevel=3)

    # -- forward ---------------------------------------------------------------------------------
    def _prep(self, tokens, region, chain):
        tok, was_torch = _to_numpy(tokens)
        reg, _ = _to_numpy(region)
        chn, _ = _to_numpy(chain)
        if tok.ndim != 2 or tok.shape[1] != self.max_len:
            # the reference asserts L == rolength in RoPE (cross_attention.py:29-30)
            raise AssertionError(f"tokens must be [B, {self.max_len}], got {tok.shape}")
        B = tok.shape[0]
        tok = L.as_i32(tok)
        reg = L.as_i32(reg, (B, self.max_len))
        if self.kind == "ab":
            if chn is None:
                raise ValueError("AntiTFNet needs H_L_chn_type [2B]")
            chn = L.as_i32(np.asarray(chn).reshape(-1), (2 * B,))
        else:
            chn = None
        return tok, reg, chn, B, was_torch

    @staticmethod
    def _flags(dropout, graph=True, prune=True, lanes=2, record=False, dist=False):
        f = {"faithful": L.HD_DROPOUT_FAITHFUL, "off": L.HD_DROPOUT_OFF, "inject": L.HD_DROPOUT_INJECT}[dropout]
        # graph: True = one hipGraph per step replayed T times, "loop" = the whole T-step loop as one hipGraph, False = eager
        return (f | (0 if graph else L.HD_NO_GRAPH) | (L.HD_LOOP_GRAPH if graph == "loop" else 0) | (0 if prune else L.HD_NO_PRUNE)
                | (0 if lanes == 2 else L.HD_ONE_LANE) | (L.HD_RECORD_LOGP if record else 0) | (L.HD_RECORD_DIST if dist else 0))

    def forward(self, H_L_seq, H_L_region_type, H_L_chn_type=None, *, dropout="faithful", seed=0, row0=0,
                step=0, enc_masks=None, conv_masks=None):
        if not self._loaded:
            raise RuntimeError("load_state_dict first")
        tok, reg, chn, B, was_torch = self._prep(H_L_seq, H_L_region_type, H_L_chn_type)
        logits = np.empty((B, self.max_len, self.n_tokens), dtype=np.float32)
        em = None if enc_masks is None else np.ascontiguousarray(enc_masks, dtype=np.uint8)
        cm = None if conv_masks is None else np.ascontiguousarray(conv_masks, dtype=np.uint8)
        L.check(self._lib.hd_forward(self._h, L.ptr(tok, C.c_int32), L.ptr(reg, C.c_int32), L.ptr(chn, C.c_int32),
                                     B, self._flags(dropout), int(seed), int(row0), int(step),
                                     L.ptr(em, C.c_uint8), L.ptr(cm, C.c_uint8), L.ptr(logits, C.c_float)))
        self._warn_on_guard()
        if was_torch:
            import torch
            return torch.from_numpy(logits)
        return logits

    __call__ = forward

    # -- whole loop on the device ----------------------------------------------------------------
    def _sample_args(self, tokens, region, chain, order, T, q_noise, enc_masks, conv_masks):
        tok, reg, chn, B, was_torch = self._prep(tokens, region, chain)
        order = np.asarray(order)
        Tmax = int(order.shape[1]) if order.ndim == 2 else 0
        order = L.as_i32(order.reshape(B, Tmax), (B, Tmax))
        T = L.as_i32(np.asarray(T).reshape(-1), (B,))
        q = None if q_noise is None else np.ascontiguousarray(q_noise, dtype=np.float32)
        if q is not None and q.shape != (Tmax, B, 22):
            raise ValueError(f"q_noise must be [{Tmax}, {B}, 22], got {q.shape}")
        em = None if enc_masks is None else np.ascontiguousarray(enc_masks, dtype=np.uint8)
        cm = None if conv_masks is None else np.ascontiguousarray(conv_masks, dtype=np.uint8)
        return tok, reg, chn, order, T, B, Tmax, q, em, cm, was_torch

    def set_guide(self, guide, B=None):
        """hd_set_guide: the guide (hudiff_amd.guide.Guide; None clears) of the NEXT sample / sample_begin / score / score_begin on
        this handle, which consumes it whether it succeeds or fails.  ``B``: rows of that session (needed by the [L] forms; default:
        the rows of a [B, L] / [B, L, 22] array)."""
        if guide is None:
            L.check(self._lib.hd_set_guide(self._h, None))
            return
        if B is None:
            B = guide.allow.shape[0] if guide.allow is not None and guide.allow.ndim == 2 else \
                guide.bias.shape[0] if guide.bias is not None and guide.bias.ndim == 3 else None
            if B is None:
                raise ValueError("set_guide: a guide in the [L] forms needs the number of rows B")
        allow, bias = guide.batch(int(B), self.max_len)
        g = L.HdGuide(int(B), float(guide.temperature), L.ptr(allow, C.c_uint32), L.ptr(bias, C.c_float))
        L.check(self._lib.hd_set_guide(self._h, C.byref(g)))

    def set_slots_per_step(self, k):
        """hd_set_slots_per_step: the block size K in [1, 64] of the NEXT sample / sample_begin / score / score_begin on this handle,
        which consumes it whether it succeeds or fails (include/hudiff_hip.h "block decoding")."""
        L.check(self._lib.hd_set_slots_per_step(self._h, int(k)))

    def set_slot_policy(self, policy):
        """hd_set_slot_policy: "given" (follow the order as written) or "confident" (the device picks, forward by forward, the
        remaining slots it is surest about; include/hudiff_hip.h "slot policy") for the NEXT sample / sample_begin / score /
        score_begin on this handle, which consumes it whether it succeeds or fails."""
        L.check(self._lib.hd_set_slot_policy(self._h, self._policy_id(policy)))

    def set_truncation(self, truncation):
        """hd_set_truncation: the top-k / top-p / min-p cut (hudiff_amd.guide.Truncation; None clears) of the NEXT sample /
        sample_begin / score / score_begin on this handle, which consumes it whether it succeeds or fails (include/hudiff_hip.h
        "truncated sampling")."""
        if truncation is None:
            L.check(self._lib.hd_set_truncation(self._h, None))
            return
        t = L.HdTruncation(int(truncation.top_k), float(truncation.top_p), float(truncation.min_p))
        L.check(self._lib.hd_set_truncation(self._h, C.byref(t)))

    @staticmethod
    def _policy_id(policy):
        if isinstance(policy, str):
            if policy not in L.SLOT_POLICIES:
                raise ValueError(f"slot_policy must be one of {sorted(L.SLOT_POLICIES)}, got {policy!r}")
            return L.SLOT_POLICIES[policy]
        return int(policy)

    def sample_order(self, B=None, Tmax=None):
        """hd_sample_order: the order int32 [B, Tmax] of the open session as it stands, or of the last session: positions below
        min(steps run, T[b]) are the slots row b visited, in visiting order (a given-order session returns the order it was given)."""
        B = self._session_B if B is None else B
        Tmax = self._session_Tmax if Tmax is None else Tmax
        order = np.zeros((B, Tmax), dtype=np.int32)
        L.check(self._lib.hd_sample_order(self._h, L.ptr(order, C.c_int32)))
        return order

    def set_budget(self, budget, B=None):
        """hd_set_budget: the mutation budget (hudiff_amd.guide.Budget; None clears) of the NEXT sample / sample_begin / score /
        score_begin on this handle, which consumes it whether it succeeds or fails (include/hudiff_hip.h "mutation budget").  ``B``:
        rows of that session (needed when the origin is given as [L]; default: the rows of a [B, L] origin)."""
        if budget is None:
            L.check(self._lib.hd_set_budget(self._h, None))
            return
        if B is None:
            if budget.origin.ndim != 2:
                raise ValueError("set_budget: a budget whose origin is [L] needs the number of rows B")
            B = budget.origin.shape[0]
        origin, max_mut = budget.batch(int(B), self.max_len)
        b = L.HdBudget(int(B), L.ptr(origin, C.c_int32), L.ptr(max_mut, C.c_int32))
        L.check(self._lib.hd_set_budget(self._h, C.byref(b)))

    def mutation_count(self, B=None):
        """hd_mutation_count: int32 [B], the mutations every row of the open budgeted session has spent so far, or of the last one."""
        B = self._session_B if B is None else B
        n = np.zeros(B, dtype=np.int32)
        L.check(self._lib.hd_mutation_count(self._h, L.ptr(n, C.c_int32)))
        return n

    # -- confidence threshold ----------------------------------------------------------------------
    def set_confidence(self, tau):
        """hd_set_confidence: the confidence threshold tau in (0, 1] (0 clears) of the NEXT sample / sample_begin / score / score_begin
        on this handle, which consumes it whether it succeeds or fails (include/hudiff_hip.h "confidence threshold")."""
        L.check(self._lib.hd_set_confidence(self._h, _tau(tau)))

    def sample_progress(self, B=None):
        """hd_sample_progress: int32 [B], the order positions every row of the open threshold session has filled, or of the last one."""
        B = self._session_B if B is None else B
        filled = np.zeros(B, dtype=np.int32)
        L.check(self._lib.hd_sample_progress(self._h, L.ptr(filled, C.c_int32)))
        return filled

    def sample_forwards(self, B=None, Tmax=None):
        """hd_sample_forwards: int32 [B, Tmax], the forward number that drew every order position of the threshold session (open, or
        the last one); -1 where nothing was drawn."""
        B = self._session_B if B is None else B
        Tmax = self._session_Tmax if Tmax is None else Tmax
        fwd = np.full((B, Tmax), -1, dtype=np.int32)
        L.check(self._lib.hd_sample_forwards(self._h, L.ptr(fwd, C.c_int32)))
        return fwd

    def sample_keys(self, B=None, Tmax=None):
        """hd_sample_keys: float32 [B, Tmax], the keys c = 1 / p_max of the last forward of a confident session (with or without a
        threshold), by order position as the order stood BEFORE that forward's permutation; meaningful for the positions that were
        still to fill in that forward."""
        B = self._session_B if B is None else B
        Tmax = self._session_Tmax if Tmax is None else Tmax
        conf = np.zeros((B, Tmax), dtype=np.float32)
        L.check(self._lib.hd_sample_keys(self._h, L.ptr(conf, C.c_float)))
        return conf

    def sample_run_to_end(self, chunk=4):
        """hd_sample_run_to_end: runs the open threshold session in chunks of ``chunk`` forwards, looking at the rows' progress after
        each, until every row is full (or Tmax forwards have run); returns the number of forwards it enqueued."""
        n = C.c_int32()
        L.check(self._lib.hd_sample_run_to_end(self._h, int(chunk), C.byref(n)))
        return int(n.value)

    # -- refinement rounds -----------------------------------------------------------------------
    def set_refine(self, rounds, slots=1, below=0.0):
        """hd_set_refine: ``rounds`` in [1, 16] refinement rounds (0 clears) of ``slots`` in [1, 64] slots each, redrawing the live
        positions whose recorded logp is < ``below`` (finite, <= 0), for the NEXT sample / sample_begin on this handle, which consumes
        it whether it succeeds or fails (include/hudiff_hip.h "refinement rounds")."""
        L.check(self._lib.hd_set_refine(self._h, int(rounds), int(slots), float(below)))

    def refine_state(self, B=None, rounds=None):
        """hd_refine_state: ``(T_now int32 [B], round_start int32 [B, rounds], round_count int32 [B, rounds])`` of the open session
        with refinement rounds, or of the last one: the order positions every row has come to use, and the first appended position
        (-1: not opened) and the number of slots of every round."""
        B = self._session_B if B is None else B
        rounds = getattr(self, "_session_rounds", 0) if rounds is None else int(rounds)
        T_now = np.zeros(B, dtype=np.int32)
        start = np.full((B, rounds), -1, dtype=np.int32)
        count = np.zeros((B, rounds), dtype=np.int32)
        L.check(self._lib.hd_refine_state(self._h, L.ptr(T_now, C.c_int32), L.ptr(start, C.c_int32), L.ptr(count, C.c_int32)))
        return T_now, start, count

    def _refine_pad(self, order, T, refine, slots_per_step):
        """``refine`` checked, and ``order`` padded with zeros to the positions its rounds can come to use (guide.refine_tcap)."""
        from .guide import refine_args, refine_tcap
        ra = refine_args(refine)
        if ra is None:
            return order, None
        order = np.asarray(order)
        if order.ndim == 2:
            need = refine_tcap(np.asarray(T).reshape(-1), ra[0], ra[1], int(slots_per_step))
            if order.shape[1] < need:
                order = np.concatenate([order, np.zeros((order.shape[0], need - order.shape[1]), dtype=order.dtype)], axis=1)
        return order, ra

    def _arm(self, guide, B, slots_per_step, slot_policy="given", truncation=None, budget=None, confidence=None, refine=None):
        """What the next begin consumes: the block size (the library is told only when it is not 1), the slot policy (told only when
        it is not "given"), the truncation (told only when it cuts something), the budget (told only when there is one), the
        confidence threshold (told only when there is one), the refinement (``refine``: None or the checked (rounds, slots, below);
        told only when there is one) and the guide."""
        policy = self._policy_id(slot_policy)
        block = int(slots_per_step) != 1
        trunc = truncation is not None and not truncation.neutral
        tau = None if confidence is None else _tau(confidence)
        thresh = tau is not None and tau != 0.0
        if block:
            self.set_slots_per_step(slots_per_step)
        try:
            if policy != L.HD_SLOTS_GIVEN:
                L.check(self._lib.hd_set_slot_policy(self._h, policy))
            if thresh:
                L.check(self._lib.hd_set_confidence(self._h, tau))
            if trunc:
                self.set_truncation(truncation)
            if budget is not None:
                self.set_budget(budget, B)
            if refine is not None:
                self.set_refine(*refine)
            if guide is not None:
                self.set_guide(guide, B)
        except Exception:
            if refine is not None:
                self._lib.hd_set_refine(self._h, 0, 0, 0.0)
            if block:
                self.set_slots_per_step(1)           # (no begin will follow to consume it)
            if policy != L.HD_SLOTS_GIVEN:
                self._lib.hd_set_slot_policy(self._h, L.HD_SLOTS_GIVEN)
            if trunc:
                self._lib.hd_set_truncation(self._h, None)
            if budget is not None:
                self._lib.hd_set_budget(self._h, None)
            if thresh:
                self._lib.hd_set_confidence(self._h, 0.0)
            raise

    def sample(self, tokens, region, chain, order, T, *, seed=0, row0=0, q_noise=None, dropout="faithful",
               enc_masks=None, conv_masks=None, graph=True, prune=True, lanes=2, return_logp=False, guide=None, slots_per_step=1,
               slot_policy="given", truncation=None, budget=None, confidence=None, record_dist=False, refine=None):
        """Run the T-step loop (sample.py:499-513) for B independent rows; returns the filled tokens.

        ``guide``: a hudiff_amd.guide.Guide (allowed residues per slot, logit bias, temperature) for this call only.

        ``slots_per_step``: block decoding, for this call only -- K in [1, 64] slots of the visiting order are drawn per denoiser
        forward, independently from that forward's conditionals: ceil(T / K) forwards instead of T; slots drawn in one forward do not
        see each other.  Position t keeps the noise and the guide it has at K = 1.  1 (default) = the one-slot loop.

        ``slot_policy``: "given" (default) visits ``order`` as written; "confident" treats ``order[b, :T[b]]`` as the row's candidate
        list (no slot twice) and lets the device fill, in every forward, the K remaining slots whose distribution is most peaked in
        that forward (include/hudiff_hip.h "slot policy"); ``sample_order()`` afterwards returns the order taken.

        ``truncation``: a hudiff_amd.guide.Truncation (top_k, top_p, min_p) for this call only: every draw is taken from its
        distribution cut to the kept tokens and renormalised, and a recorded logp is the token's under that distribution.  None or a
        neutral one (nothing cut) makes no call into the library.

        ``budget``: a hudiff_amd.guide.Budget (origin tokens, max_mutations) for this call only: a row that has changed max_mutations
        of its origin-bearing slots draws its origin from then on (include/hudiff_hip.h "mutation budget"); ``mutation_count()``
        afterwards returns what every row spent.  One slot per forward only.

        ``confidence``: a threshold tau in (0, 1] for this call only, with ``slot_policy="confident"``: every forward fills, per row,
        all remaining slots whose top probability is at least tau -- at least one, at most ``slots_per_step`` -- so the number of
        forwards follows the model's certainty (include/hudiff_hip.h "confidence threshold"); ``sample_forwards()`` afterwards returns
        the forward that drew every position.  None or 0 = no threshold.

        ``return_logp``: the session records (HD_RECORD_LOGP) and the call returns ``(tokens, logp)``, logp float32 [B, Tmax] = the
        log-probability of the token row b drew at step t under the distribution it was drawn from; 0 where t >= T[b].  The tokens
        are the same with and without it.

        ``record_dist``: the session keeps the whole 22-token distribution of every draw (HD_RECORD_DIST, include/hudiff_hip.h
        "distribution record") and records logp too; ``sample_dist()`` / ``sample_logp()`` afterwards return them.  The tokens are the
        same with and without it.

        ``refine``: ``dict(rounds=, slots=, below=0.0)`` for this call only -- after a row has drawn its whole list, its ``slots``
        least likely live positions with logp < ``below`` are masked again and redrawn with everything else as context, ``rounds``
        times (include/hudiff_hip.h "refinement rounds").  The session records; ``order`` is padded to ``guide.refine_tcap`` positions
        (a ``q_noise`` must have that many), and ``sample_logp()`` / ``sample_order()`` / ``refine_state()`` afterwards have that
        width.  None = none."""
        order, ra = self._refine_pad(order, T, refine, slots_per_step)
        tok, reg, chn, order, T, B, Tmax, q, em, cm, was_torch = self._sample_args(
            tokens, region, chain, order, T, q_noise, enc_masks, conv_masks)
        out = tok.copy()
        self._arm(guide, B, slots_per_step, slot_policy, truncation, budget, confidence, ra)
        self._session_B, self._session_Tmax = B, Tmax
        self._session_rounds = ra[0] if ra else 0
        L.check(self._lib.hd_sample(self._h, L.ptr(out, C.c_int32), L.ptr(reg, C.c_int32), L.ptr(chn, C.c_int32),
                                    L.ptr(order, C.c_int32), L.ptr(T, C.c_int32), B, Tmax,
                                    self._flags(dropout, graph, prune, lanes, bool(return_logp), bool(record_dist)), int(seed), int(row0), L.ptr(q, C.c_float),
                                    L.ptr(em, C.c_uint8), L.ptr(cm, C.c_uint8)))
        self._warn_on_guard()
        logp = self.sample_logp(B, Tmax) if return_logp else None
        if was_torch:
            import torch
            out = torch.from_numpy(out.astype(np.int64))
            logp = None if logp is None else torch.from_numpy(logp)
        return (out, logp) if return_logp else out

    def sample_logp(self, B=None, Tmax=None):
        """hd_sample_logp: logp float32 [B, Tmax] of the open session, or of the last one that recorded."""
        B = self._session_B if B is None else B
        Tmax = self._session_Tmax if Tmax is None else Tmax
        logp = np.zeros((B, Tmax), dtype=np.float32)
        L.check(self._lib.hd_sample_logp(self._h, L.ptr(logp, C.c_float)))
        return logp

    def sample_dist(self, B=None, Tmax=None):
        """hd_sample_dist: dist float32 [B, Tmax, 22] of the open session, or of the last one that kept the record (``record_dist``):
        the log-probability of every token at every position a forward drew or scored, -inf for a token the guide, the budget or the
        cut removed, 0 where t >= T[b]; ``dist[b, t, token written] == logp[b, t]`` bit for bit."""
        B = self._session_B if B is None else B
        Tmax = self._session_Tmax if Tmax is None else Tmax
        dist = np.zeros((B, Tmax, 22), dtype=np.float32)
        L.check(self._lib.hd_sample_dist(self._h, L.ptr(dist, C.c_float)))
        return dist

    # -- beam search -------------------------------------------------------------------------------
    def set_beam(self, width):
        """hd_set_beam: the beam width W in [1, 64] (0 clears) of the NEXT sample / sample_begin on this handle, which consumes it
        whether it succeeds or fails (include/hudiff_hip.h "beam search")."""
        L.check(self._lib.hd_set_beam(self._h, int(width)))

    def beam_state(self, B=None, Tmax=None):
        """hd_beam_state: (score float32 [B], parent int32 [B, Tmax], cand float32 [B, 22]) of the open beam session, or of the last
        one; cand is the candidate table of the last position run."""
        B = self._session_B if B is None else B
        Tmax = self._session_Tmax if Tmax is None else Tmax
        score = np.zeros(B, dtype=np.float32)
        parent = np.zeros((B, Tmax), dtype=np.int32)
        cand = np.zeros((B, 22), dtype=np.float32)
        L.check(self._lib.hd_beam_state(self._h, L.ptr(score, C.c_float), L.ptr(parent, C.c_int32), L.ptr(cand, C.c_float)))
        return score, parent, cand

    def beam_begin(self, tokens, region, chain, order, T, width, *, guide=None, truncation=None, dropout="off", graph=True, prune=True,
                   lanes=2, seed=0, row0=0, budget=None):
        """hd_set_beam + hd_sample_begin: a beam session of width W on rows that are ALREADY replicated -- tokens [G*W, L], every row
        of a group equal to its first.  sample_run / sample_restart / sync / sample_tokens / sample_logp / beam_state / sample_end
        work on it; it always records."""
        tok, reg, chn, order, T, B, Tmax, _, _, _, _ = self._sample_args(tokens, region, chain, order, T, None, None, None)
        self.set_beam(width)
        try:
            self._arm(guide, B, 1, "given", truncation, budget)
        except Exception:
            self._lib.hd_set_beam(self._h, 0)        # (no begin will follow to consume it)
            raise
        L.check(self._lib.hd_sample_begin(self._h, L.ptr(tok, C.c_int32), L.ptr(reg, C.c_int32), L.ptr(chn, C.c_int32),
                                          L.ptr(order, C.c_int32), L.ptr(T, C.c_int32), B, Tmax,
                                          self._flags(dropout, graph, prune, lanes), int(seed), int(row0), None, None, None))
        self._session_B, self._session_Tmax = B, Tmax

    def beam_search(self, tokens, region, chain, order, T, width, *, guide=None, truncation=None, lanes=2, graph=True, budget=None):
        """The W most likely, pairwise different completions of every row along its visiting order, ranked: tokens [G, L], order
        [G, Tmax], T [G] as for ``sample``; ``width`` = W in [1, 64].  Each row is replicated W times, a [G, ...] guide is expanded to
        [G*W, ...], the session runs on the device (include/hudiff_hip.h "beam search": dropout off, no noise) and ``parent`` is
        followed backwards on the host.  Returns numpy arrays
            tokens [G, W, L]     the final rows of every group, best first
            score  [G, W]        their cumulative log-probability (-inf for a dead row: fewer than W sequences exist)
            logp   [G, W, Tmax]  the step values along each final row's own history, aligned to order positions
            live   [G, W]        score is finite.
        ``budget``: a hudiff_amd.guide.Budget over the G groups: the W most likely completions with at most max_mutations changes from
        the origin, ranked by their log-likelihood under the guide alone (the budget removes candidates, it does not rescale them)."""
        from .guide import beam_backtrack
        W = int(width)
        if isinstance(width, (bool, float)) or W != width or not 1 <= W <= L.BEAM_MAX_WIDTH:
            raise ValueError(f"width must be an integer in [1, {L.BEAM_MAX_WIDTH}], got {width!r}")
        tok, _ = _to_numpy(tokens)
        reg, _ = _to_numpy(region)
        chn, _ = _to_numpy(chain)
        tok, reg, order, T = np.asarray(tok), np.asarray(reg), np.asarray(order), np.asarray(T).reshape(-1)
        if tok.ndim != 2 or tok.shape[1] != self.max_len:
            raise ValueError(f"tokens must be [G, {self.max_len}], got {tok.shape}")
        G = tok.shape[0]
        if reg.shape != tok.shape or order.ndim != 2 or order.shape[0] != G or T.shape != (G,):
            raise ValueError(f"region must be {tok.shape}, order [{G}, Tmax] and T [{G}]; got {reg.shape}, {order.shape}, {T.shape}")
        rep = np.repeat(np.arange(G), W)
        if self.kind == "ab":
            if chn is None:
                raise ValueError("AntiTFNet needs H_L_chn_type [2G]")
            chn = np.asarray(chn).reshape(-1)
            if chn.shape != (2 * G,):
                raise ValueError(f"chain must be [{2 * G}], got {chn.shape}")
            chn = np.concatenate([chn[:G][rep], chn[G:][rep]])
        else:
            chn = None
        if guide is not None:
            guide.batch(G, self.max_len)             # (shape check against the groups as given)
            guide = guide.take(rep)
        if budget is not None:
            budget.batch(G, self.max_len)            # (shape check against the groups as given)
            budget = budget.take(rep)
        self.beam_begin(tok[rep], reg[rep], chn, order[rep], T[rep], W, guide=guide, truncation=truncation, lanes=lanes, graph=graph,
                        budget=budget)
        Tmax = order.shape[1]
        if G and Tmax:
            try:
                self.sample_run(0, Tmax)
            except Exception:
                self._lib.hd_sample_end(self._h, None)       # (closes the session; the error of the run is the one that travels)
                raise
        out = self.sample_end()
        score, parent, _ = self.beam_state(G * W, Tmax)
        return beam_backtrack(out, score, parent, self.sample_logp(G * W, Tmax), T, W)

    # -- likelihood of given sequences -------------------------------------------------------------
    def _score_seq(self, tok, reg, chn, order, T, B, Tmax, flags, seed, row0, em, cm, guide=None, slots_per_step=1, slot_policy="given",
                   truncation=None, budget=None, confidence=None, want_dist=False):
        logp = np.zeros((B, Tmax), dtype=np.float32)
        self._arm(guide, B, slots_per_step, slot_policy, truncation, budget, confidence)
        self._session_B, self._session_Tmax = B, Tmax
        L.check(self._lib.hd_score(self._h, L.ptr(tok, C.c_int32), L.ptr(reg, C.c_int32), L.ptr(chn, C.c_int32),
                                   L.ptr(order, C.c_int32), L.ptr(T, C.c_int32), B, Tmax, flags, int(seed), int(row0),
                                   L.ptr(em, C.c_uint8), L.ptr(cm, C.c_uint8), L.ptr(logp, C.c_float)))
        self._warn_on_guard()
        return (logp, self.sample_dist(B, Tmax)) if want_dist else logp

    def score(self, tokens, region, chain, order, T, *, dropout="off", parallel=None, device_batch=256, seed=0, row0=0,
              enc_masks=None, conv_masks=None, graph=True, prune=True, lanes=2, guide=None, slots_per_step=1, slot_policy="given",
              truncation=None, budget=None, confidence=None, record_dist=False, return_dist=False):
        """Log-probability of every given token along a visiting order: logp float32 [B, Tmax],
        logp[b, t] = log p(tokens[b, order[b, t]] | tokens[b] with order[b, t:T[b]] masked); 0 where t >= T[b].  Its sum over t is a
        one-order estimate of the order-agnostic log-likelihood of the scored slots.  ``tokens`` are complete sequences.

        ``parallel``: the tokens are given, so the T steps of a row do not depend on each other: True expands every (row, step) to a
        row of its own (scoring.expand_steps) and runs them as one-step device batches of at most ``device_batch`` rows; False runs
        the sequential T-step loop (hd_score), which is what dropout needs -- generated masks are keyed by (row, step), which an
        expanded row does not carry.  None: parallel when ``dropout == "off"``.

        ``guide``: the values are log-probabilities under the guided distribution (hudiff_amd.guide); a token its slot does not allow,
        or temperature 0, is an error.  Step-parallel: an expanded row takes the guide of the row it came from.

        ``truncation``: the values are log-probabilities under the truncated distribution (hudiff_amd.guide.Truncation); a token the
        cut of its step removes has probability 0 under that sampler and scores -inf (no error).  Step-parallel: every expanded
        session gets the same truncation.

        ``slots_per_step`` = K > 1: the log-likelihood under the block sampler -- logp[b, t] is conditioned on the tokens with
        ``order[b, (t // K) * K : T[b]]`` masked (the whole group of t, not only t onwards), which is what a sampling session with
        the same K recorded.  Step-parallel: one expanded row per (row, group), run in sessions of block size K.

        ``slot_policy`` = "confident": teacher-forced under the confident sampler -- ``order[b, :T[b]]`` is the candidate list, the
        library picks the visiting order (``sample_order()`` afterwards) and logp[b, t] belongs to position t of THAT order.  The slot
        of step t depends on the steps before it, so there is no step-parallel form: ``parallel=True`` raises, None runs the loop.

        ``confidence``: teacher-forced under the threshold sampler (needs ``slot_policy="confident"``; ``slots_per_step`` is the cap):
        the library picks order and forwards by the same rule (``sample_order()`` / ``sample_forwards()`` afterwards).  No
        step-parallel form.

        ``budget``: the values are log-probabilities under the budgeted sampler (hudiff_amd.guide.Budget): at a position where the row
        has spent its budget the origin scores 0 and any other token -inf (no error).  Whether a position is exhausted depends on the
        steps before it, so there is no step-parallel form either.

        ``return_dist``: the sessions keep the distribution record (HD_RECORD_DIST) and the call returns ``(logp, dist)``, dist float32
        [B, Tmax, 22] = the log-probability of EVERY token at the position logp[b, t] belongs to, under the same distribution (-inf for
        a token the guide, the budget or the cut removed; 0 where t >= T[b]); ``dist[b, t, target] == logp[b, t]`` bit for bit.
        Step-parallel: the expanded rows' records fold back by ``Expanded.fold_dist``.  ``record_dist`` alone keeps the record of a
        sequential call for ``sample_dist()`` without returning it."""
        K = int(slots_per_step)
        want_dist = bool(return_dist)
        rec_dist = want_dist or bool(record_dist)
        confident = self._policy_id(slot_policy) != L.HD_SLOTS_GIVEN
        if budget is not None:
            if parallel:
                raise ValueError("step-parallel scoring cannot follow a mutation budget: whether step t is exhausted depends on the "
                                 "steps before it; use parallel=False (or None)")
            parallel = False
        if confidence is not None and _tau(confidence) != 0.0:
            if parallel:
                raise ValueError("step-parallel scoring cannot follow a confidence threshold: the slots of a forward depend on the "
                                 "forwards before it; use parallel=False (or None)")
            parallel = False
        if confident and parallel:
            raise ValueError("step-parallel scoring cannot follow slot_policy='confident': the slot of step t depends on the steps "
                             "before it; use parallel=False (or None)")
        if parallel is None:
            parallel = dropout == "off" and not confident
        if parallel and dropout != "off":
            raise ValueError("step-parallel scoring needs dropout='off': dropout masks are keyed by (row, step), "
                             "which an expanded row does not carry; use parallel=False")
        tok, reg, chn, order, T, B, Tmax, _, em, cm, was_torch = self._sample_args(
            tokens, region, chain, order, T, None, enc_masks, conv_masks)
        flags = self._flags(dropout, graph, prune, lanes, dist=rec_dist)
        dist = None
        if not parallel:
            logp = self._score_seq(tok, reg, chn, order, T, B, Tmax, flags, seed, row0, em, cm, guide, K, slot_policy, truncation, budget,
                                   confidence, want_dist)
            if want_dist:
                logp, dist = logp
        else:
            from . import scoring
            x = scoring.expand_steps(tok, reg, chn, order, T, slots_per_step=K)      # (K outside [1, 64]: ValueError)
            if guide is not None:
                guide.batch(B, self.max_len)         # (shape check against the batch as given)
            n = x.tokens.shape[0]
            # hd_score takes its targets from the tokens it is given (and masks the slots itself): hand each row the targets of its
            # group back (one slot at K = 1)
            live = np.arange(K)[None, :] < x.T[:, None]
            rr = np.broadcast_to(np.arange(n)[:, None], (n, K))[live]
            x.tokens[rr, x.order[live]] = tok[x.rows[rr], x.order[live]]
            flat = np.zeros((n, K), dtype=np.float32)
            flat_dist = np.zeros((n, K, 22), dtype=np.float32) if want_dist else None
            for s in range(0, n, int(device_batch)):
                e = min(n, s + int(device_batch))
                ch = None if x.chain is None else np.ascontiguousarray(np.concatenate([x.chain[s:e], x.chain[n + s:n + e]]))
                got = self._score_seq(np.ascontiguousarray(x.tokens[s:e]), np.ascontiguousarray(x.region[s:e]), ch,
                                      np.ascontiguousarray(x.order[s:e]), np.ascontiguousarray(x.T[s:e]), e - s, K, flags,
                                      seed, 0, None, None, None if guide is None else guide.take(x.rows[s:e]), K,
                                      truncation=truncation, want_dist=want_dist)
                if want_dist:
                    flat[s:e], flat_dist[s:e] = got
                else:
                    flat[s:e] = got
            logp = x.fold(flat, Tmax)
            if want_dist:
                dist = x.fold_dist(flat_dist, Tmax)
        if was_torch:
            import torch
            logp = torch.from_numpy(logp)
            dist = None if dist is None else torch.from_numpy(dist)
        return (logp, dist) if want_dist else logp

    def score_begin(self, tokens, region, chain, order, T, *, seed=0, row0=0, dropout="off", enc_masks=None, conv_masks=None,
                    graph=True, prune=True, lanes=2, guide=None, slots_per_step=1, slot_policy="given", truncation=None, budget=None, confidence=None,
                    record_dist=False):
        """hd_score_begin: a teacher-forced recording session; sample_run / sample_restart / sync / sample_end / sample_tokens /
        last_run_ms / sample_logp work on it as on a sampling session, and sample_dist with ``record_dist``."""
        tok, reg, chn, order, T, B, Tmax, _, em, cm, _ = self._sample_args(tokens, region, chain, order, T, None, enc_masks, conv_masks)
        self._arm(guide, B, slots_per_step, slot_policy, truncation, budget, confidence)
        L.check(self._lib.hd_score_begin(self._h, L.ptr(tok, C.c_int32), L.ptr(reg, C.c_int32), L.ptr(chn, C.c_int32),
                                         L.ptr(order, C.c_int32), L.ptr(T, C.c_int32), B, Tmax,
                                         self._flags(dropout, graph, prune, lanes, dist=bool(record_dist)), int(seed), int(row0),
                                         L.ptr(em, C.c_uint8), L.ptr(cm, C.c_uint8)))
        self._session_B, self._session_Tmax = B, Tmax

    def sample_begin(self, tokens, region, chain, order, T, *, seed=0, row0=0, q_noise=None, dropout="faithful",
                     enc_masks=None, conv_masks=None, graph=True, prune=True, lanes=2, record_logp=False, guide=None, slots_per_step=1,
                     slot_policy="given", truncation=None, budget=None, confidence=None, record_dist=False, refine=None):
        """hd_sample_begin with what ``sample`` takes.  ``refine``: as there -- ``order`` is padded to ``guide.refine_tcap`` positions,
        which is then the session's Tmax (``sample_run`` takes positions up to it)."""
        order, ra = self._refine_pad(order, T, refine, slots_per_step)
        tok, reg, chn, order, T, B, Tmax, q, em, cm, _ = self._sample_args(
            tokens, region, chain, order, T, q_noise, enc_masks, conv_masks)
        self._arm(guide, B, slots_per_step, slot_policy, truncation, budget, confidence, ra)
        self._session_rounds = ra[0] if ra else 0
        L.check(self._lib.hd_sample_begin(self._h, L.ptr(tok, C.c_int32), L.ptr(reg, C.c_int32), L.ptr(chn, C.c_int32),
                                          L.ptr(order, C.c_int32), L.ptr(T, C.c_int32), B, Tmax,
                                          self._flags(dropout, graph, prune, lanes, bool(record_logp), bool(record_dist)), int(seed), int(row0), L.ptr(q, C.c_float),
                                          L.ptr(em, C.c_uint8), L.ptr(cm, C.c_uint8)))
        self._session_B, self._session_Tmax = B, Tmax

    def sample_run(self, t0, t1):
        """hd_sample_run: order positions [t0, t1); in a session with K slots per step t0 is a multiple of K and t1 a multiple of K
        or Tmax, and ceil((t1 - t0) / K) forwards are enqueued.  A threshold session takes forward numbers: t1 - t0 forwards."""
        L.check(self._lib.hd_sample_run(self._h, int(t0), int(t1)))

    def sample_restart(self, seed):
        L.check(self._lib.hd_sample_restart(self._h, int(seed)))

    def sync(self):
        L.check(self._lib.hd_sync(self._h))

    def sample_end(self):
        out = np.empty((self._session_B, self.max_len), dtype=np.int32)
        L.check(self._lib.hd_sample_end(self._h, L.ptr(out, C.c_int32)))
        self._warn_on_guard()
        return out

    def sample_tokens(self):
        """Tokens of the open session as they stand (hd_sample_tokens: synchronises, the session stays open)."""
        out = np.empty((self._session_B, self.max_len), dtype=np.int32)
        L.check(self._lib.hd_sample_tokens(self._h, L.ptr(out, C.c_int32)))
        return out

    def last_run_ms(self):
        ms, steps = C.c_float(), C.c_int32()
        L.check(self._lib.hd_last_run_ms(self._h, C.byref(ms), C.byref(steps)))
        return float(ms.value), int(steps.value)

    def precision_info(self):
        """hd_precision_report: {'precision': 'split' | 'f32_gemm' | 'f32_all' (the resolved route), 'split_built' (bit 0 GEMM weight
        images, bit 1 attention core), 'split_in_use', 'lnsync_in_use', 'range_fallbacks' (calls repeated on the fp32 kernels because
        an operand left the fp16 range), 'lnsync_fallbacks' (calls repeated with separate LayerNorm passes because an ln_sync meeting
        failed), 'last_call_repeated'}."""
        r = L.HdPrecisionInfo()
        L.check(self._lib.hd_precision_report(self._h, C.byref(r), C.sizeof(r)))
        return {"precision": L.PRECISION_NAMES[int(r.precision)], "split_built": int(r.split_built), "split_in_use": bool(r.split_in_use),
                "lnsync_in_use": bool(r.lnsync_in_use), "range_fallbacks": int(r.range_fallbacks),
                "lnsync_fallbacks": int(r.lnsync_fallbacks), "last_call_repeated": bool(r.last_call_repeated),
                "lnsync_cross_xcd": bool(r.lnsync_cross_xcd)}

    def precision_reset(self):
        """hd_precision_reset: back on the configured route after a guard switched kernels off."""
        L.check(self._lib.hd_precision_reset(self._h))
        r = L.HdPrecisionInfo()
        if self._lib.hd_precision_report(self._h, C.byref(r), C.sizeof(r)) == L.HD_OK:
            self._seen_fallbacks = (int(r.range_fallbacks), int(r.lnsync_fallbacks))

    def debug_fail_next_lnsync(self):
        L.check(self._lib.hd_debug_fail_next_lnsync(self._h))

    def debug_scatter_lnsync(self, on=True):
        L.check(self._lib.hd_debug_scatter_lnsync(self._h, 1 if on else 0))

    def debug_launch_tally(self):
        """hd_debug_launch_tally: {kernel name: launches issued since the last call} (host-side count, cleared by the call; a launch
        captured into a graph counts once, so read it as "> 0").  Names: hudiff_amd._lib.DEBUG_KERNELS."""
        counts = (C.c_int64 * len(L.DEBUG_KERNELS))()
        L.check(self._lib.hd_debug_launch_tally(self._h, counts, len(L.DEBUG_KERNELS)))
        return {n: int(counts[i]) for i, n in enumerate(L.DEBUG_KERNELS)}

    def debug_stop_after(self, stage):
        L.check(self._lib.hd_debug_stop_after(self._h, int(stage)))

    def debug_read(self, name, B):
        width = {"FEAT": "sum_d_model", "Y": "sum_d_model", "AT": "sum_d_model", "ATX": "sum_d_model", "YX": "sum_d_model", "O": "att_model"}.get(name, "d_model")
        w = 3 * self.config["att_model"] if name == "QKV" else self.config[width]
        out = np.empty((B, self.max_len, w), dtype=np.float32)
        L.check(self._lib.hd_debug_read(self._h, name.encode(), B, L.ptr(out, C.c_float), out.size))
        return out

    def flops_per_row_forward(self):
        return float(self._lib.hd_flops_per_row_forward(C.byref(self._cfg)))

    def flops_per_row_sample_step(self):
        return float(self._lib.hd_flops_per_row_sample_step(C.byref(self._cfg)))


class AntiTFNet(_Denoiser):
    """model/encoder/model.py:325 -- antibody (VH + VL, 291 slots) denoiser."""
    kind = "ab"


class NanoAntiTFNet(_Denoiser):
    """model/nanoencoder/model.py:290 -- nanobody (VHH, 152 slots) denoiser."""
    kind = "nb"

    def __init__(self, n_tokens, d_embedding, d_model, n_encoder_layers, aa_kernel_size, r, n_region, r_embedding,
                 r_model, n_pos_model, max_len, sum_d_model, dual_layers, att_model, dim_feedforward, nhead, cs_layers,
                 **kw):
        super().__init__(n_tokens, d_embedding, d_model, n_encoder_layers, aa_kernel_size, r, n_region, r_embedding,
                         r_model, n_pos_model, max_len, sum_d_model, dual_layers, att_model, dim_feedforward, nhead,
                         cs_layers, **kw)


def model_selected(config, pretrained_model=None, tokenizer=None, device=0, precision=None, options=None):
    """utils/train_utils.py:43-55 for the two inference models (the training-only wrappers are out of scope)."""
    name = _get(config, "name")
    params = dict(_get(config, "model"))
    if name == "trans_oadm":
        return AntiTFNet(**params, device=device, precision=precision, options=options)
    if name == "nano":
        return NanoAntiTFNet(**params, device=device, precision=precision, options=options)
    raise NotImplementedError(f"config.name={name!r}: only 'trans_oadm' and 'nano' are sampling models")


def device_info(device=0):
    lib = L.load()
    name = C.create_string_buffer(256)
    cu, mem = C.c_int32(), C.c_int64()
    L.check(lib.hd_device_info(int(device), name, 256, C.byref(cu), C.byref(mem)))
    return {"name": name.value.decode(), "cu_count": int(cu.value), "hbm_bytes": int(mem.value)}


def device_count():
    return int(L.load().hd_device_count())
