"""The constructions of tests/range_cases.py are what they claim -- on the CPU, before a device sees them.

For every site: the bent state dict has the reference's keys and shapes (a strict load), the named producer -- and nobody that runs
before or after it -- meets the outlier (ProbeNet: the oracle with max |x| recorded at every tensor the split route writes in split
form), the control keeps every producer in range, and a dead-channel construction computes the function of the same weights without the
outlier.  For the tables: every firing pair names a raise site of hudiff_amd/csrc, every raise site is named by a firing pair or listed
as unreachable with the reason, the pairs are unique.  For Part B: the float64 logits do not move with k, and the Python mirror of the
packer's criterion keeps every ordinary matrix and refuses the bent ones from k = 16 on."""
import os
import re

import numpy as np
import pytest

import range_cases as rc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KINDS = ("ab", "nb")
CASES = [(k, s) for k in KINDS for s in rc.SITES]
IDS = [f"{k}-{s.name}" for k, s in CASES]


def _shapes(kind):
    from hudiff_amd import synthetic as S
    return S.state_dict_shapes(kind, rc.config(kind))


def _strict(kind, sd):
    want = _shapes(kind)
    assert set(sd) == set(want)
    assert all(sd[k].shape == tuple(want[k]) and sd[k].dtype == np.float32 for k in want)


@pytest.mark.parametrize("kind,site", CASES, ids=IDS)
def test_site_is_isolated(kind, site):
    """Float32 oracle: the site's producer holds the outlier, every other producer the run reaches stays below 65 504; the control keeps
    all of them below it and the site at 2^14.5."""
    v = np.float32(site.value)
    sd = rc.bent(kind, site, v)
    _strict(kind, sd)
    pk, logits = rc.peaks(kind, sd)
    key = site.probe(kind)
    ran = rc.ran_until(site, kind, pk)
    assert key in ran and np.isfinite(logits).all()
    scale = rc.QS if site.name == "q" else 1.0                            # (Q is checked behind its scale)
    assert pk[key] >= float(rc.LIMIT) and abs(pk[key] / (float(v) * scale) - 1.0) < 1e-3, (key, pk[key])
    others = {k: pk[k] for k in ran if k != key and k not in site.also}
    assert max(others.values()) < 100.0, {k: x for k, x in others.items() if x >= 100.0}      # (ordinary rows stay below 10)
    for k in site.also:
        assert pk[k] >= float(rc.LIMIT) * 0.999, (k, pk[k])
    ck, _ = rc.peaks(kind, rc.bent(kind, site, rc.CONTROL))
    assert abs(ck[key] / (float(rc.CONTROL) * scale) - 1.0) < 1e-3
    assert max(ck[k] for k in ran) < float(rc.LIMIT)


@pytest.mark.parametrize("kind,site", [c for c in CASES if c[1].exact], ids=[i for i, c in zip(IDS, CASES) if c[1].exact])
def test_exact_sites_hold_the_parameter_itself(kind, site):
    """gamma = 0 / a zero weight row: the value the producer splits IS the parameter, in float32, in every row -- for 65 504 and the float below."""
    for v in (rc.LIMIT, rc.BELOW):
        pk, _ = rc.peaks(kind, rc.bent(kind, site, v, exact=True))
        assert np.float32(pk[site.probe(kind)]) == v, (pk[site.probe(kind)], v)
    assert rc.BELOW < rc.LIMIT and np.nextafter(rc.BELOW, np.float32(np.inf)) == rc.LIMIT == np.float32(np.finfo(np.float16).max)


@pytest.mark.parametrize("kind,site", [c for c in CASES if c[1].dead], ids=[i for i, c in zip(IDS, CASES) if c[1].dead])
def test_dead_channel_leaves_the_function_alone(kind, site):
    """Float64 logits with the outlier against the same construction with 0 in its place: the consumer's weights for the channel are zero."""
    _, hot = rc.peaks(kind, rc.bent(kind, site, site.value), np.float64)
    _, cold = rc.peaks(kind, rc.bent(kind, site, 0.0), np.float64)
    err = float(np.abs(hot - cold).max())
    print(f"\n[{kind} {site.name}] |logits(outlier) - logits(0)| in float64: {err:.2e}")
    assert err < 1e-9, err


def test_tables_are_complete():
    pairs = rc.expanded(rc.PAIRS)
    assert len({(k, p.site, p.form) for k, p in pairs}) == len(pairs)                     # one entry per (site, form, kind) that is run
    for k, p in pairs + rc.expanded(rc.EXACT_PAIRS):
        assert p.site in rc.SITE and p.form in rc.FORM and k in KINDS
        assert (p.raises in rc.RAISE_SITES) if p.fire else (p.raises is None), p
    for k, p in rc.expanded(rc.EXACT_PAIRS):
        assert rc.SITE[p.site].exact and p.fire, p
    named = {p.raises for _, p in pairs if p.fire}
    assert named | set(rc.UNREACHED) == set(rc.RAISE_SITES) and not named & set(rc.UNREACHED)
    assert {s.name for s in rc.SITES} == {p.site for _, p in pairs}                       # no site thinned away
    assert {f.name for f in rc.FORMS} == {p.form for _, p in pairs}
    for k in KINDS:                                                                        # ... on either model
        assert {s.name for s in rc.SITES} == {p.site for kk, p in pairs if kk == k and p.fire}
    # the quiet pairs are exactly those the header allows: Q and K under the fp32 attention core
    assert {(p.site, p.form) for _, p in pairs if not p.fire} == {("q", "f32core"), ("k", "f32core")}
    assert {r for names in rc.MASK_BITS.values() for r in names} <= named


def test_raise_sites_match_the_sources():
    """One RAISE_SITES entry per raise_range_flag call of the kernels (the constructions were derived from this list: a new producer must
    get a case)."""
    calls = 0
    for f in ("hd_kernels.hip.h", "hd_attn_fused.hip.h", "hd_chain.hip.h"):
        src = open(os.path.join(ROOT, "hudiff_amd", "csrc", f)).read()
        calls += len(re.findall(r"raise_range_flag\((?!const)", src))
    assert calls == len(rc.RAISE_SITES), calls
    opts = open(os.path.join(ROOT, "include", "hudiff_hip.h")).read().lower()
    for f in rc.FORMS:
        for o in dict(f.opts, **(f.ab_opts or {})):
            assert "hd_opt_" + o in opts, o


@pytest.mark.parametrize("kind", KINDS)
def test_lane_case(kind):
    """Token 20 occurs in row 3 alone (the second of two lanes of two rows), at a slot no step visits, and its raw stream passes the range at
    the conv stack's output while the clean batch stays ordinary."""
    sd, c = rc.lane_case(kind)
    _strict(kind, sd)
    where = np.argwhere(c["hot"] == rc.LANE_TOKEN)
    assert where.shape == (1, 2) and where[0, 0] == 3 and where[0, 1] not in c["order"][3].tolist()
    assert (c["hot"] != c["clean"]).sum() == 1 and (c["T"] == 2).all() and c["hot"].shape[0] == 4
    net = rc.ProbeNet(kind, rc.config(kind), sd)
    net(c["hot"], c["region"], c["chain"])
    hot = dict(net.peaks)
    first_out = [k for k, x in hot.items() if x >= float(rc.LIMIT)][0]
    assert first_out == "conv_out", first_out                              # every ByteNet operand before it is normalised
    net.peaks = {}
    net(c["clean"], c["region"], c["chain"])
    assert max(net.peaks.values()) < 100.0


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", sorted(rc.WEIGHT_CASES))
def test_weight_cases(kind, name):
    """One entry at 2^k times the largest |w| on an input channel that is exactly zero: float64 logits identical for every k; the criterion
    of X3Packer::add (mirrored in weight_guard_holds) keeps k = 0 and 8 -- ordinary entries still have a normal lo part there -- and refuses
    16, 24 and 32."""
    sd0, arrays0 = rc.weight_bent(kind, name, 0)
    _strict(kind, sd0)
    _, want = rc.peaks(kind, sd0, np.float64)
    assert rc.weight_guard_holds(arrays0)
    for k in rc.WEIGHT_KS:
        sd, arrays = rc.weight_bent(kind, name, k)
        _strict(kind, sd)
        _, got = rc.peaks(kind, sd, np.float64)
        assert np.array_equal(got, want), k
        assert rc.weight_guard_holds(arrays) == (k < 16), k


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("variant", ["plain", "massive", "dc"])
def test_weight_guard_keeps_ordinary_matrices(kind, variant):
    """Production depth, the adversarial variants included: every GEMM matrix of the state dict passes the criterion as it stands and with a
    LayerNorm gain folded into its rows (x 30 in `massive`), so no existing model leaves the split route."""
    from hudiff_amd import synthetic as S
    cfg = dict(S.AB_CONFIG if kind == "ab" else S.NB_CONFIG)
    sd = S.adversarial_state_dict(kind, cfg, 5, variant)
    n = 0
    for key, w in sd.items():
        if w.ndim >= 2 and ("conv_block" in key or "aa_encoder." in key and "embedder" not in key or "self_at" in key):
            assert rc.weight_guard_holds([w]), key
            n += 1
    for blk in range(cfg["cs_layers"]):
        p = f"self_at.layers.{blk}."
        for g, ws in ((p + "norm_hl1.weight", [p + "attn_hl_c." + x + ".weight" for x in ("query", "key", "value")]), (p + "norm_hl2.weight", [p + "ff_hl.0.weight"])):
            folded = np.concatenate([sd[k] for k in ws]) * sd[g][None, :]
            assert rc.weight_guard_holds([folded - folded.mean(axis=1, keepdims=True)]), (g, variant)
    assert n > 80
