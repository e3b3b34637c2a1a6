"""Oracle vs the REFERENCE's own classes at PRODUCTION width (configs/antibody_train.yml, heavy_train.yml).

tests/golden/prodwidth_{kind}.npz (oracle/make_golden_prodwidth.py) holds what the reference's ``AntiTFNet`` /
``NanoAntiTFNet`` computed for two rows with seeded weights: its logits with dropout off, and its logits with dropout on
together with the keep-masks it drew.  This is the committed form of the check DESIGN.md §3 quotes: with the same seeded
weights in the numpy oracle, the logits agree to float32 round-off (tolerance 2e-5; observed 2e-6 .. 4e-6), with dropout
off and under the reference's own recorded dropout masks.
"""
import hashlib

import numpy as np
import pytest

import hudiff_oracle as ho
from conftest import chain_or_none, load_golden, unpack_masks

TOL = 2e-5


@pytest.mark.parametrize("kind", ["ab", "nb"])
def test_production_width_oracle_matches_reference(kind):
    from hudiff_amd import synthetic as S
    z = load_golden(f"prodwidth_{kind}.npz")
    cfg = dict(S.AB_CONFIG if kind == "ab" else S.NB_CONFIG)
    sd = S.random_state_dict(kind, cfg, seed=int(z["weight_seed"]))
    h = hashlib.sha256()
    for k in sorted(sd):
        h.update(k.encode())
        h.update(np.ascontiguousarray(sd[k], dtype=np.float32).tobytes())
    assert h.hexdigest() == str(z["weight_sha256"]), "regenerated weights differ from the ones the reference ran with"
    tokens, region, chain = z["tokens"], z["region"], chain_or_none(z)
    B = tokens.shape[0]
    want = z["logits"]
    got = ho.OracleNet(kind, dict(cfg, dropout=0.0), sd)(tokens, region, chain)
    err = float(np.abs(got - want).max())
    assert err < TOL, err
    # dropout ON (the reference's inference behaviour): replay the masks the reference drew
    want_d = z["logits_dropout"]
    enc, conv = unpack_masks(z, "enc_masks"), unpack_masks(z, "conv_masks")
    assert enc.shape[1] == conv.shape[1] == B
    got_d = ho.OracleNet(kind, cfg, sd)(tokens, region, chain, dropout=ho.Dropout("inject", enc_masks=enc, conv_masks=conv))
    err_d = float(np.abs(got_d - want_d).max())
    assert err_d < 2 * TOL, err_d
    assert np.abs(want_d - want).max() > 1e-2
    print(f"{kind}: max|dlogit| oracle vs reference = {err:.2e} (dropout off), {err_d:.2e} (reference's masks)")
