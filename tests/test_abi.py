"""The C-ABI shared object loads on a machine without a GPU, exports every symbol include/hudiff_hip.h declares,
and refuses to run (no CPU fallback)."""
import ctypes as C
import os
import re

import pytest

from conftest import ROOT


def header_functions():
    text = open(os.path.join(ROOT, "include", "hudiff_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(hd_[a-z_0-9]+)\s*\(", text)))


def test_library_exports_every_declared_symbol():
    from hudiff_amd import _lib
    lib = _lib.load()
    declared = header_functions()
    assert len(declared) >= 15
    for name in declared:
        assert hasattr(lib, name), f"{name} declared in hudiff_hip.h but not exported"
    assert sorted(_lib.EXPORTS) == declared, "ctypes binding and header disagree"


def test_config_struct_layout_matches_header():
    from hudiff_amd import _lib
    text = open(os.path.join(ROOT, "include", "hudiff_hip.h")).read()
    body = re.search(r"typedef struct HdConfig \{(.*?)\} HdConfig;", text, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = re.findall(r"(int32_t|float)\s+([a-z_]+);", body)
    assert [n for _, n in fields] == [n for n, _ in _lib.HdConfig._fields_]
    assert C.sizeof(_lib.HdConfig) == 4 * len(fields)


def test_precision_report_struct_layout_matches_header():
    from hudiff_amd import _lib
    text = open(os.path.join(ROOT, "include", "hudiff_hip.h")).read()
    body = re.search(r"typedef struct HdPrecisionInfo \{(.*?)\} HdPrecisionInfo;", text, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = re.findall(r"(int32_t|int64_t)\s+([a-z_]+);", body)
    assert [n for _, n in fields] == [n for n, _ in _lib.HdPrecisionInfo._fields_]
    assert [t for t, _ in fields] == ["int32_t" if c is C.c_int32 else "int64_t" for _, c in _lib.HdPrecisionInfo._fields_]
    assert C.sizeof(_lib.HdPrecisionInfo) == sum(4 if t == "int32_t" else 8 for t, _ in fields) == 40
    enum = re.search(r"enum \{ (HD_PRECISION_DEFAULT[^}]*)\}", text).group(1)
    vals = dict((k.strip(), int(v)) for k, v in (e.split("=") for e in enum.split(",")))
    assert vals == {"HD_PRECISION_DEFAULT": _lib.HD_PRECISION_DEFAULT, "HD_PRECISION_F32_GEMM": _lib.HD_PRECISION_F32_GEMM,
                    "HD_PRECISION_F32_ALL": _lib.HD_PRECISION_F32_ALL, "HD_PRECISION_SPLIT": _lib.HD_PRECISION_SPLIT}


def test_precision_entry_points_reject_null_handles():
    """The route is part of the C ABI (VERDICT r3 "Next" #1): hd_set_precision / hd_precision_report / hd_precision_reset exist and
    validate their arguments without a device."""
    from hudiff_amd import _lib
    lib = _lib.load()
    assert lib.hd_set_precision(None, _lib.HD_PRECISION_SPLIT) == _lib.HD_ERR_INVALID
    r = _lib.HdPrecisionInfo()
    assert lib.hd_precision_report(None, C.byref(r), C.sizeof(r)) == _lib.HD_ERR_INVALID
    assert lib.hd_precision_reset(None) == _lib.HD_ERR_INVALID
    assert lib.hd_sample_tokens(None, None) == _lib.HD_ERR_STATE


def test_option_table_matches_header():
    """hd_set_option / hd_get_option (VERDICT r4 "Next" #7): the ctypes binding's option names are the header's HdOption enum, in
    order, and the entry points validate their arguments without a device."""
    from hudiff_amd import _lib
    text = open(os.path.join(ROOT, "include", "hudiff_hip.h")).read()
    body = re.search(r"typedef enum HdOption \{(.*?)\} HdOption;", text, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    enum = [(n, int(v)) for n, v in re.findall(r"(HD_OPT_[A-Z0-9_]+)\s*=\s*(\d+)", body)]
    assert enum[-1][0] == "HD_OPT_COUNT" and enum[-1][1] == len(enum) - 1
    assert [(n[len("HD_OPT_"):].lower(), v) for n, v in enum[:-1]] == sorted(_lib.OPTIONS.items(), key=lambda kv: kv[1])
    lib = _lib.load()
    v = C.c_int64()
    assert lib.hd_set_option(None, 0, 1) == _lib.HD_ERR_INVALID
    assert lib.hd_get_option(None, 0, C.byref(v)) == _lib.HD_ERR_INVALID
    assert lib.hd_debug_scatter_lnsync(None, 1) == _lib.HD_ERR_INVALID


def test_launch_tally_table_matches_header():
    """hd_debug_launch_tally: the binding's kernel names are the header's HdDebugKernel enum, in order; every split GEMM id is
    followed by its tap (conv) twin; the entry point validates its arguments without a device."""
    from hudiff_amd import _lib
    text = open(os.path.join(ROOT, "include", "hudiff_hip.h")).read()
    body = re.search(r"typedef enum HdDebugKernel \{(.*?)\} HdDebugKernel;", text, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    enum = [(n, int(v)) for n, v in re.findall(r"(HD_DBG_[A-Z0-9_]+)\s*=\s*(\d+)", body)]
    assert enum[-1][0] == "HD_DBG_COUNT" and enum[-1][1] == len(enum) - 1
    assert [v for _, v in enum] == list(range(len(enum)))
    assert [n[len("HD_DBG_"):].lower() for n, _ in enum[:-1]] == list(_lib.DEBUG_KERNELS)
    x3 = [n for n in _lib.DEBUG_KERNELS if n.startswith("x3_")]
    assert len(x3) == 18 and all(x3[i + 1] == x3[i] + "_conv" for i in range(0, len(x3), 2))
    lib = _lib.load()
    counts = (C.c_int64 * len(_lib.DEBUG_KERNELS))()
    assert lib.hd_debug_launch_tally(None, counts, len(counts)) == _lib.HD_ERR_INVALID


def test_no_cpu_fallback():
    import hudiff_amd
    from hudiff_amd._lib import HD_ERR_NO_DEVICE, HudiffError
    if hudiff_amd.device_count() > 0:
        pytest.skip("a GPU is visible")
    with pytest.raises(HudiffError) as e:
        hudiff_amd.NanoAntiTFNet(23, 16, 16, 2, 7, 128, 7, 4, 16, 16, 152, 32, 2, 128, 32, 2, 2)
    assert e.value.status == HD_ERR_NO_DEVICE


def test_config_validation_needs_no_gpu():
    """hd_create checks the configuration before it looks for a device, so these fail the same way everywhere."""
    import ctypes as C
    from hudiff_amd import _lib
    from hudiff_amd import synthetic as S
    lib = _lib.load()

    def create(**over):
        cfg = dict(S.AB_CONFIG, **over)
        c = _lib.HdConfig()
        c.abi_version = over.get("abi_version", _lib.HD_ABI_VERSION)
        c.kind = over.get("kind", _lib.HD_KIND_ANTIBODY)
        c.n_tokens, c.max_len, c.h_len = cfg["n_tokens"], cfg["max_len"], over.get("h_len", 152)
        c.d_model, c.sum_d_model = cfg["d_model"], cfg["sum_d_model"]
        c.n_encoder_layers, c.dual_layers, c.kernel_size, c.r = 6, 6, cfg["aa_kernel_size"], 128
        c.att_model, c.nhead, c.dim_feedforward, c.cs_layers = cfg["att_model"], cfg["nhead"], 256, 5
        c.n_region, c.r_embedding, c.n_side, c.s_embedding = 7, 4, 3, 4
        c.enc_act, c.conv_act, c.dropout = over.get("enc_act", _lib.HD_ACT_GELU), _lib.HD_ACT_RELU, cfg["dropout"]
        h = C.c_void_p()
        st = lib.hd_create(C.byref(c), 0, C.byref(h))
        if st == _lib.HD_OK:
            lib.hd_destroy(h)
        return st, lib.hd_last_error().decode()

    assert create(abi_version=99)[0] == _lib.HD_ERR_INVALID
    assert create(kind=7)[0] == _lib.HD_ERR_INVALID
    st, msg = create(nhead=4)                       # head dim 128
    assert st == _lib.HD_ERR_UNSUPPORTED and "head dim" in msg
    assert create(max_len=400)[0] == _lib.HD_ERR_UNSUPPORTED           # attention kernels are instantiated for <= 304 / <= 160 slots
    assert create(sum_d_model=512)[0] == _lib.HD_ERR_INVALID          # antibody needs 3 * d_model
    assert create(dropout=1.5)[0] == _lib.HD_ERR_INVALID
    assert create(enc_act=9)[0] == _lib.HD_ERR_INVALID
    assert create(aa_kernel_size=9)[0] == _lib.HD_ERR_UNSUPPORTED
    assert create()[0] in (_lib.HD_OK, _lib.HD_ERR_NO_DEVICE)          # a valid config only fails for lack of a GPU


def test_product_package_never_imports_the_oracle():
    pkg = os.path.join(ROOT, "hudiff_amd")
    for dirpath, _, files in os.walk(pkg):
        for fn in files:
            if fn.endswith((".py", ".hip", ".h")):
                src = open(os.path.join(dirpath, fn)).read()
                assert "hudiff_oracle" not in src and "import oracle" not in src and "from oracle" not in src, fn


def test_flops_formula_matches_survey():
    from hudiff_amd import _lib
    from hudiff_amd import synthetic as S
    import hudiff_oracle as ho
    assert abs(ho.flops_per_forward(S.AB_CONFIG) - 18.336296448e9) < 1
    assert abs(ho.flops_per_forward(S.NB_CONFIG) - 5.706522624e9) < 1
    lib = _lib.load()
    c = _lib.HdConfig()
    c.max_len, c.d_model, c.sum_d_model, c.att_model, c.dim_feedforward, c.kernel_size = 291, 256, 768, 512, 256, 7
    c.n_encoder_layers, c.dual_layers, c.cs_layers, c.n_tokens = 6, 6, 5, 23
    assert abs(lib.hd_flops_per_row_forward(C.byref(c)) - 18.336296448e9) < 1


def test_bench_route_peaks_follow_the_library_flop_formula():
    """bench.py prices the default route against a time-weighted peak built from the attention core's share of the algorithmic
    FLOPs; that share must come out of the same formula the library exports (hd_flops_per_row_forward)."""
    import ctypes as C
    import importlib.util
    from hudiff_amd import _lib as L
    from hudiff_amd import synthetic as S
    spec = importlib.util.spec_from_file_location("bench_mod2", os.path.join(ROOT, "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    lib = L.load()
    for kind, cfg, want_total in (("ab", S.AB_CONFIG, 18.336e9), ("nb", S.NB_CONFIG, 5.707e9)):
        c = L.HdConfig()
        c.abi_version, c.kind = L.HD_ABI_VERSION, (0 if kind == "ab" else 1)
        c.n_tokens, c.max_len, c.d_model, c.sum_d_model = cfg["n_tokens"], cfg["max_len"], cfg["d_model"], cfg["sum_d_model"]
        c.n_encoder_layers, c.dual_layers, c.kernel_size = cfg["n_encoder_layers"], cfg["dual_layers"], cfg["aa_kernel_size"]
        c.att_model, c.nhead, c.dim_feedforward, c.cs_layers = cfg["att_model"], cfg["nhead"], cfg["dim_feedforward"], cfg["cs_layers"]
        total = float(lib.hd_flops_per_row_forward(C.byref(c)))
        assert abs(total - want_total) / want_total < 1e-3
        core = 2.0 * cfg["cs_layers"] * 4 * cfg["max_len"] * cfg["att_model"] * cfg["max_len"]
        share = bench.attention_core_share(cfg)
        assert abs(share - core / total) < 1e-9
        pk = bench.route_peak(cfg, "default")
        assert bench.route_peak(cfg, "all_fp32") == 157.3 and abs(bench.route_peak(cfg, "split") - 2500 / 3) < 1e-9
        assert abs(1.0 / pk - ((1 - share) / 157.3 + share / (2500 / 3))) < 1e-12 and 157.3 < pk < 175
