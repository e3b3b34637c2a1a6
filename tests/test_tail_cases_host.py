"""CPU checks of tests/tail_cases.py: the probe construction is what tests/test_gpu_tail_dist.py believes it is, before any device runs."""
import numpy as np
import pytest

import hudiff_oracle as ho
import tail_cases as TC

GROUPS = [("prod", "ab"), ("prod", "nb"), ("micro", "ab"), ("micro", "nb")]


def test_slot_lists_are_the_named_ones():
    assert TC.SLOTS["ab"] == (0, 15, 16, 63, 64, 151, 152, 255, 256, 287, 288, 290)
    assert TC.SLOTS["nb"] == (0, 15, 16, 63, 64, 127, 128, 143, 144, 151)
    for kind, L in TC.LENGTH.items():
        s = TC.SLOTS[kind]
        assert s[0] == 0 and s[-1] == L - 1                                          # first and last slot
        for k in {"ab": (64, 256), "nb": (64, 128)}[kind]:
            assert k - 1 in s and k in s                                             # both sides of a 64-key stride (the first and the last one)
        last = (L - 1) // 16 * 16
        assert last - 1 in s and last in s                                           # both sides of the last 16-key tile
        assert set(TC.DROP_SLOTS[kind]) <= set(s) and set(TC.EDGE_SLOTS[kind]) <= set(s) and TC.LATER[kind]["slot"] in s
    assert TC.H_LEN - 1 in TC.SLOTS["ab"] and TC.H_LEN in TC.SLOTS["ab"]              # both sides of the chain boundary
    assert TC.DROP_SLOTS["ab"][0] < TC.H_LEN <= TC.DROP_SLOTS["ab"][1]                # one in each chain
    assert TC.DROP_TOKENS == (0, 5, 10, 15, 20, 21)


@pytest.mark.parametrize("group,kind", GROUPS)
def test_sequences_are_half_masked_real_rows(group, kind):
    seqs = TC.sequences(group, kind)
    assert len(seqs) == TC.N_SEQ == 2
    for q in seqs:
        assert q.full.shape == (TC.LENGTH[kind],) and q.full.min() >= 0 and q.full.max() < TC.MASK          # complete: every slot can be scored
        assert set(TC.SLOTS[kind]) <= set(q.M) and set(q.own) <= set(q.M) and len(q.own) >= 20
        assert (q.masked[q.M] == TC.MASK).all() and (np.delete(q.masked, q.M) == np.delete(q.full, q.M)).all()
        assert 0.1 < len(q.M) / TC.LENGTH[kind] < 0.6                                                       # a realistic half-masked context
    cfg, _ = TC.weights(group, kind)
    assert float(cfg["dropout"]) == 0.0 and int(cfg["max_len"]) == TC.LENGTH[kind]
    if group == "prod":
        assert float(TC.weights(group, kind, dropout=True)[0]["dropout"]) > 0


@pytest.mark.parametrize("group,kind", GROUPS)
def test_copies_and_probes_share_one_denoiser_input(group, kind):
    """The masked input is identical across the 22 copies and across a sequence's probes; the copies differ in the probed token only."""
    seqs = TC.sequences(group, kind)
    s = TC.session(group, kind, TC.all_picks(kind), B=len(TC.all_picks(kind)) + 3)
    assert s.B % 4 == 3 and len(s.fill) == 3 and len(s.probe_rows) == TC.N_SEQ * len(TC.SLOTS[kind]) * 22
    seen = set()
    for r, (q, slot, j) in zip(s.probe_rows, s.picks):
        assert np.array_equal(TC.denoiser_input(s, r), seqs[q].masked)
        assert s.order[r, 0] == slot and s.tokens[r, slot] == j and s.T[r] == len(seqs[q].M)
        assert sorted(s.order[r, :s.T[r]]) == sorted(seqs[q].M)                                              # no slot twice
        rest = np.delete(s.tokens[r], slot)
        assert np.array_equal(rest, np.delete(seqs[q].full, slot))
        seen.add((q, slot, j))
    assert len(seen) == len(s.picks)
    if kind == "ab":
        assert np.array_equal(s.chain[:s.B][s.probe_rows], [seqs[q].chain[0] for q, _, _ in s.picks])
        assert np.array_equal(s.chain[s.B:][s.probe_rows], [seqs[q].chain[1] for q, _, _ in s.picks])
    # a sampling session on the same rows starts from that very input
    smp = TC.session(group, kind, TC.all_picks(kind), B=s.B, sampling=True)
    for r, (q, _, _) in zip(smp.probe_rows, smp.picks):
        assert np.array_equal(smp.tokens[r], seqs[q].masked)
    assert np.array_equal(smp.order, s.order) and np.array_equal(smp.T, s.T)


@pytest.mark.parametrize("kind", ["ab", "nb"])
def test_fillers_sit_between_probe_rows(kind):
    for name, B, opts, kw, _, _, groups in TC.EDGES:
        picks = TC.all_picks(kind, seqs=(0,), slots=TC.EDGE_SLOTS[kind])
        s = TC.session("prod", kind, picks, B=B)
        assert len(picks) == 44 and s.B == B and len(s.fill) == B - 44 >= 1, name
        assert (s.T[s.fill] == 0).all() and (s.order[s.fill] == 0).all() and (s.T[s.probe_rows] > 0).all()
        assert ((s.probe_rows.min() < s.fill) & (s.fill < s.probe_rows.max())).any(), name                    # not only at the end
        lanes = kw["lanes"] if B >= opts.get("lane_min_rows", 16) else 1
        per = [B // lanes + (1 if l < B % lanes else 0) for l in range(lanes)]                                # balanced contiguous row blocks
        if lanes == 2:
            assert (s.fill < per[0]).any() and (s.fill >= per[0]).any() or len(s.fill) == 1, name             # both lanes hold one
        if name.startswith(("one_lane", "two_lanes")):
            assert set(per) == {64} or set(per) == {65}, (name, per)
    mods = {n: [(B // kw["lanes"] + (1 if l < B % kw["lanes"] else 0)) % 4 for l in range(kw["lanes"])] for n, B, _, kw, _, _, _ in TC.EDGES}
    assert {1, 2, 3} <= {m for n, v in mods.items() if n.startswith(("launches", "projection")) for m in v}
    assert TC.filler_positions(531, 3) == [88, 265, 442]


@pytest.mark.parametrize("group,kind", GROUPS)
def test_later_step_context(group, kind):
    seqs = TC.sequences(group, kind)
    q, slot = TC.LATER[kind]["seq"], TC.LATER[kind]["slot"]
    s = TC.session(group, kind, [(q, slot, j) for j in range(22)], B=23, later=True)
    ctx = TC.later_context(group, kind)
    a, b = seqs[q].own[:2]
    assert s.read == 2 and ctx[a] == seqs[q].full[a] != TC.MASK and ctx[b] == seqs[q].full[b] and ctx[slot] == TC.MASK
    assert (ctx == TC.MASK).sum() == len(seqs[q].M) - 2
    for r, (_, _, j) in zip(s.probe_rows, s.picks):
        assert list(s.order[r, :3]) == [a, b, slot] and s.tokens[r, slot] == j
        assert np.array_equal(TC.denoiser_input(s, r), ctx)


@pytest.mark.parametrize("group,kind", GROUPS)
def test_oracle_pair_gives_a_yard_stick_under_the_cap(group, kind):
    """... and the reference IS the scoring definition: a float64 forward with M masked, log-softmax at s."""
    ref = TC.reference(group, kind)
    print(f"\n[{group} {kind}] yard-stick {ref.yard:.3e}  device bound {ref.bound:.3e}  pair bound {ref.pair:.3e}")
    assert np.isfinite(ref.yard) and 0 < ref.yard and ref.bound == TC.MARGIN * ref.yard and ref.pair == 2 * ref.bound
    assert ref.bound < TC.CAP == 2e-5
    assert ref.want.shape == (TC.N_SEQ, TC.LENGTH[kind], 22) and np.allclose(np.exp(ref.want).sum(-1), 1.0, atol=1e-12)
    # the definition, spelled out for one sequence with plain numpy
    cfg, sd = TC.weights(group, kind)
    Q = TC.sequences(group, kind)[1]
    chain = None if kind == "nb" else np.array(Q.chain, np.int32)
    z = ho.OracleNet(kind, cfg, sd, dtype=np.float64)(Q.masked[None], Q.region[None], chain)[0, :, :22].astype(np.float64)
    lsm = z - np.log(np.exp(z - z.max(-1, keepdims=True)).sum(-1, keepdims=True)) - z.max(-1, keepdims=True)
    slots = list(TC.SLOTS[kind])
    assert np.abs(lsm[slots] - ref.want[1, slots]).max() < 1e-10
    s = TC.session(group, kind, TC.all_picks(kind))
    want = TC.expected(ref, s)
    for i in (0, 21, 22, len(s.picks) - 1):
        q, slot, j = s.picks[i]
        assert want[i] == ref.want[q, slot, j]


@pytest.mark.parametrize("kind", ["ab", "nb"])
def test_oracle_pair_under_dropout(kind):
    ref = TC.reference_dropout(kind)
    s = TC.drop_session(kind)
    print(f"\n[prod {kind} dropout] yard-stick {ref.yard:.3e}  device bound {ref.bound:.3e}")
    assert len(ref.rows) == len(ref.want) == 2 * len(TC.DROP_TOKENS) and len(set(ref.rows)) == len(ref.rows)
    assert all(s.picks[list(s.probe_rows).index(r)][2] in TC.DROP_TOKENS for r in ref.rows)
    assert np.isfinite(ref.yard) and 0 < ref.yard and ref.bound < TC.CAP
    assert (ref.want < 0).all()
    # the masks really enter: the same rows without dropout score something else
    off = TC.reference("prod", kind)
    plain = np.array([off.want[s.picks[list(s.probe_rows).index(r)]] for r in ref.rows])
    assert np.abs(plain - ref.want).max() > 1e-2
