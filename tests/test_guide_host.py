"""Guided sampling, host side (no GPU): the constraints parser, Guide broadcasting, the float64 definition, the HdGuide binding
and the CLI flags."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

from conftest import ROOT


def test_parse_constraints_forms():
    from hudiff_amd import parse_constraints, tables as T
    from hudiff_amd.guide import ALL_TOKENS, LETTERS, letters_mask
    assert LETTERS == "ACDEFGHIKLMNPQRSTVWYX-" and ALL_TOKENS == 0x3FFFFF
    assert letters_mask("A") == 1 and letters_mask("C") == 2 and letters_mask("-") == 1 << 21 and letters_mask("X") == 1 << 20
    a = parse_constraints(["# a comment", "", "H,48,VIL   # Vernier", "L,2,!C", "H,111A,G-"], "ab")
    assert a.shape == (T.AB_LEN,) and a.dtype == np.uint32
    h48, l2, h111a = T.HEAVY_POSITIONS_dict["48"], T.H_LEN + T.LIGHT_POSITIONS_dict["2"], T.HEAVY_POSITIONS_dict["111A"]
    assert a[h48] == letters_mask("VIL") and a[l2] == ALL_TOKENS & ~letters_mask("C") and a[h111a] == letters_mask("G-")
    rest = np.ones(T.AB_LEN, bool)
    rest[[h48, l2, h111a]] = False
    assert (a[rest] == ALL_TOKENS).all()
    # nothing given: everything allowed
    assert (parse_constraints([], "nb") == ALL_TOKENS).all() and parse_constraints([], "nb").shape == (T.H_LEN,)


def test_parse_constraints_star_and_intersection():
    from hudiff_amd import parse_constraints, tables as T
    from hudiff_amd.guide import ALL_TOKENS, letters_mask
    a = parse_constraints(["H,*,!CM", "H,48,VILM", "H,48,!V"], "ab")
    assert (a[:T.H_LEN] & letters_mask("CM") == 0).all()
    assert (a[T.H_LEN:] == ALL_TOKENS).all()                  # the light chain was not named
    assert a[T.HEAVY_POSITIONS_dict["48"]] == letters_mask("IL")
    assert a[T.HEAVY_POSITIONS_dict["47"]] == ALL_TOKENS & ~letters_mask("CM")
    b = parse_constraints(["L,*,AG", "L,127,G"], "ab")
    assert (b[T.H_LEN:-1] == letters_mask("AG")).all() and b[-1] == letters_mask("G") and (b[:T.H_LEN] == ALL_TOKENS).all()
    assert parse_constraints(["H,1,A", "H,1,C"], "nb")[0] == 0           # an empty intersection is the caller's to find


@pytest.mark.parametrize("lines, kind, needle", [
    (["H,48,VIL", "H,999,A"], "ab", "line 2"),
    (["H,48,VB"], "ab", "'B'"),
    (["L,2,A"], "nb", "line 1"),
    (["K,2,A"], "ab", "chain"),
    (["H,48"], "ab", "chain,position,residues"),
    (["L,111L,A"], "ab", "111L"),                             # a heavy-only insertion label
])
def test_parse_constraints_errors_name_the_line(lines, kind, needle):
    from hudiff_amd import parse_constraints
    with pytest.raises(ValueError) as e:
        parse_constraints(lines, kind)
    assert needle in str(e.value) and "constraints line" in str(e.value)
    with pytest.raises(ValueError):
        parse_constraints([], "xx")


def test_guide_broadcasting():
    from hudiff_amd import Guide
    L = 7
    allow = np.arange(1, L + 1, dtype=np.int64)
    bias = np.arange(L * 22, dtype=np.float64).reshape(L, 22)
    g = Guide(allow, bias, temperature=0.5)
    a, b = g.batch(3, L)
    assert a.shape == (3, L) and a.dtype == np.uint32 and a.flags.c_contiguous and (a == allow[None]).all()
    assert b.shape == (3, L, 22) and b.dtype == np.float32 and b.flags.c_contiguous and (b == bias[None]).all()
    assert g.temperature == 0.5
    # [B, L] forms pass through, a wrong B or L is an error
    g2 = Guide(np.tile(allow, (3, 1)), None)
    a2, b2 = g2.batch(3, L)
    assert b2 is None and (a2 == a).all()
    for bad in (lambda: g2.batch(4, L), lambda: g.batch(3, L + 1), lambda: Guide(np.zeros((2, 3, 4))), lambda: Guide(None, np.zeros((L, 21)))):
        with pytest.raises(ValueError):
            bad()
    assert Guide().batch(5, L) == (None, None)
    # rows of a batch guide (step-parallel scoring) and the stack of per-row guides (the batched sampler)
    per_row = Guide(np.arange(3 * L).reshape(3, L), np.arange(3 * L * 22).reshape(3, L, 22), 2.0)
    t = per_row.take([2, 0, 2, 1])
    assert (t.allow == per_row.allow[[2, 0, 2, 1]]).all() and (t.bias == per_row.bias[[2, 0, 2, 1]]).all() and t.temperature == 2.0
    assert g.take([1, 1]).allow.shape == (L,)
    s = Guide.stack([None, Guide(allow), Guide(None, bias)], L, temperature=0.7)
    sa, sb = s.batch(3, L)
    assert (sa[0] == 0x3FFFFF).all() and (sa[1] == allow).all() and (sa[2] == 0x3FFFFF).all()
    assert (sb[:2] == 0).all() and (sb[2] == bias).all() and s.temperature == 0.7
    assert Guide.stack([None, Guide(allow)], L).bias is None


def test_guided_log_probs_hand_computed():
    from hudiff_amd import guided_log_probs
    z = np.zeros(22)
    z[[3, 5, 7]] = [1.0, 2.0, -1.0]
    bias = np.zeros(22)
    bias[5] = -1.0
    bias[7] = 3.0
    allow = (1 << 3) | (1 << 5) | (1 << 7) | (1 << 20)
    # g = (z + bias) / 0.5 over tokens {3, 5, 7, 20}: 2, 2, 4, 0
    lse = math.log(math.exp(2) + math.exp(2) + math.exp(4) + 1.0)
    got = guided_log_probs(z, allow, bias, 0.5)
    assert got.shape == (22,)
    for j, g in ((3, 2.0), (5, 2.0), (7, 4.0), (20, 0.0)):
        assert abs(got[j] - (g - lse)) < 1e-14
    off = np.ones(22, bool)
    off[[3, 5, 7, 20]] = False
    assert np.isneginf(got[off]).all() and abs(np.exp(got[~off]).sum() - 1) < 1e-14
    # neutral guide = log_softmax; temperature 0 = the temperature-1 distribution (what a greedy session records under)
    zz = np.random.default_rng(0).normal(0, 2, (4, 5, 22))
    ref = zz - zz.max(-1, keepdims=True)
    ref = ref - np.log(np.exp(ref).sum(-1, keepdims=True))
    assert np.abs(guided_log_probs(zz, np.full((4, 5), 0x3FFFFF, np.uint32)) - ref).max() < 1e-14
    assert np.array_equal(guided_log_probs(zz, 0x3FFFFF, None, 0.0), guided_log_probs(zz, 0x3FFFFF, None, 1.0))
    # a singleton is certain; batched allow / bias broadcast
    one = guided_log_probs(zz, np.full((4, 5), 1 << 21, np.uint32), np.ones((4, 5, 22)), 2.0)
    assert (one[..., 21] == 0).all() and np.isneginf(one[..., :21]).all()


def test_hdguide_layout_matches_header():
    from hudiff_amd import _lib
    text = open(os.path.join(ROOT, "include", "hudiff_hip.h")).read()
    body = re.search(r"typedef struct HdGuide \{(.*?)\} HdGuide;", text, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = re.findall(r"(int32_t|float|const uint32_t\*|const float\*)\s+([a-zA-Z_]+);", body)
    assert [n for _, n in fields] == [n for n, _ in _lib.HdGuide._fields_] == ["B", "temperature", "allow", "bias"]
    ctype = {"int32_t": C.c_int32, "float": C.c_float, "const uint32_t*": C.POINTER(C.c_uint32), "const float*": C.POINTER(C.c_float)}
    assert [ctype[t] for t, _ in fields] == [c for _, c in _lib.HdGuide._fields_]
    assert C.sizeof(_lib.HdGuide) == 4 + 4 + 2 * C.sizeof(C.c_void_p)
    assert _lib.HdGuide.allow.offset == 8 and _lib.HdGuide.bias.offset == 8 + C.sizeof(C.c_void_p)
    assert re.search(r"HdStatus hd_set_guide\(HdModel\* m, const HdGuide\* g\);", text)
    assert "hd_set_guide" in _lib.EXPORTS
    assert int(re.search(r"#define HD_ABI_VERSION (\d+)", text).group(1)) == _lib.HD_ABI_VERSION == 1


def test_set_guide_rejects_a_null_handle():
    from hudiff_amd import _lib
    lib = _lib.load()
    assert lib.hd_set_guide(None, None) == _lib.HD_ERR_INVALID
    g = _lib.HdGuide(1, 1.0, None, None)
    assert lib.hd_set_guide(None, C.byref(g)) == _lib.HD_ERR_INVALID


@pytest.mark.parametrize("name", ["sample", "nanosample", "sample_for_anti_cdr", "sample_for_nano_cdr"])
def test_cli_flags_exist_with_neutral_defaults(name):
    import importlib
    cli = importlib.import_module(f"hudiff_amd.cli.{name}")
    base = ["--ckpt", "x.pt"]
    a = cli.build_parser().parse_args(base)
    assert a.temperature == 1.0 and a.forbid == "" and a.constraints_fpath is None and a.bias_fpath is None
    b = cli.build_parser().parse_args(base + ["--temperature", "0", "--forbid", "CM", "--constraints_fpath", "c.txt", "--bias_fpath", "b.npz"])
    assert b.temperature == 0.0 and b.forbid == "CM" and b.constraints_fpath == "c.txt" and b.bias_fpath == "b.npz"


def test_cli_helper_builds_per_job_guides(tmp_path):
    import argparse
    import logging
    from hudiff_amd import tables as T
    from hudiff_amd.cli.common import add_guide_args, apply_guide_args
    from hudiff_amd.guide import ALL_TOKENS, letters_mask
    from hudiff_amd.sampler import Job
    L = T.H_LEN
    p48, p49 = T.HEAVY_POSITIONS_dict["48"], T.HEAVY_POSITIONS_dict["49"]

    def jobs():
        return [Job(tokens=np.zeros(L, np.int32), region=np.zeros(L, np.int32), loc=np.array([p48, 3, 9]), name="a"),
                Job(tokens=np.zeros(L, np.int32), region=np.zeros(L, np.int32), loc=np.array([p49, p48]), name="b")]
    parser = add_guide_args(argparse.ArgumentParser())
    # no flag: nothing happens to the jobs
    js = jobs()
    assert apply_guide_args(parser.parse_args([]), "nb", js) == 1.0 and all(j.guide is None for j in js)
    assert apply_guide_args(parser.parse_args(["--temperature", "0.7"]), "nb", js) == 0.7 and all(j.guide is None for j in js)
    cons = tmp_path / "c.txt"
    cons.write_text("H,48,VILC\nH,49,!A   # alanine scan says no\n")
    bias = np.random.default_rng(1).normal(0, 1, (L, 22)).astype(np.float32)
    np.savez(tmp_path / "b.npz", bias=bias)
    records = []
    logger = logging.getLogger("test_guide_host")
    logger.setLevel(logging.INFO)
    handler = logging.Handler()
    handler.emit = lambda r: records.append(r)
    logger.addHandler(handler)
    js = jobs()
    t = apply_guide_args(parser.parse_args(["--forbid", "CM", "--constraints_fpath", str(cons), "--bias_fpath", str(tmp_path / "b.npz"),
                                            "--temperature", "0"]), "nb", js, logger)
    assert t == 0.0
    for j in js:
        a, b = j.guide.batch(1, L)
        assert a[0, p48] == letters_mask("VIL") and a[0, p49] == ALL_TOKENS & ~letters_mask("ACM")
        assert a[0, 3] == ALL_TOKENS & ~letters_mask("CM") and np.array_equal(b[0], bias)
    # job "a" does not sample IMGT 49: one ignored constraint, said once at INFO
    said = [r for r in records if r.levelno == logging.INFO and "ignored" in r.getMessage()]
    assert len(said) == 1 and said[0].getMessage().endswith(": 1")
    for bad in (["--forbid", "-"], ["--forbid", "B"], ["--temperature", "-1"], ["--temperature", "0.001"], ["--temperature", "nan"]):
        with pytest.raises(ValueError):
            apply_guide_args(parser.parse_args(bad), "nb", jobs())
    cons.write_text("H,48,C\n")
    with pytest.raises(ValueError, match="sampled slot"):
        apply_guide_args(parser.parse_args(["--forbid", "C", "--constraints_fpath", str(cons)]), "nb", jobs())
    cons.write_text("H,48,C\nH,4711,A\n")
    with pytest.raises(ValueError, match="line 2"):
        apply_guide_args(parser.parse_args(["--constraints_fpath", str(cons)]), "nb", jobs())


def test_sampler_passes_none_without_a_guide():
    """No job guide and temperature 1: the calls into the model are exactly the unguided ones (no `guide` keyword at all)."""
    from hudiff_amd import Guide
    from hudiff_amd.sampler import Job, sample_jobs

    class Fake:
        max_len, kind = 6, "nb"

        def __init__(self):
            self.calls = []

        def sample(self, tok, reg, chain, order, T, **kw):
            self.calls.append(kw)
            return tok

    def jobs(guide=None):
        return [Job(tokens=np.full(6, 22, np.int32), region=np.zeros(6, np.int32), loc=np.array([1, 2]), name="a"),
                Job(tokens=np.full(6, 22, np.int32), region=np.zeros(6, np.int32), loc=np.array([3]), name="b", guide=guide)]
    m = Fake()
    sample_jobs(m, jobs(), 2, 1)
    assert len(m.calls) == 1 and "guide" not in m.calls[0] and sorted(m.calls[0]) == ["dropout", "q_noise", "row0", "seed"]
    m = Fake()
    sample_jobs(m, jobs(Guide(np.arange(6) + 1)), 2, 1, temperature=0.5)
    g = m.calls[0]["guide"]
    a, b = g.batch(4, 6)
    assert g.temperature == 0.5 and b is None and (a[:2] == 0x3FFFFF).all() and (a[2:] == np.arange(6) + 1).all()
    m = Fake()
    sample_jobs(m, jobs(), 2, 1, temperature=0.0)
    assert m.calls[0]["guide"].temperature == 0.0
