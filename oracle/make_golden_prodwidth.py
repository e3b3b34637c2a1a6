"""TEST INFRASTRUCTURE ONLY -- production-width golden vectors from the REFERENCE's own classes.

    python oracle/make_golden_prodwidth.py         (needs the reference tree that oracle/ref_import.py imports)

tests/test_oracle_vs_reference.py holds the numpy oracle to the reference's ``AntiTFNet`` / ``NanoAntiTFNet`` at
PRODUCTION width (configs/antibody_train.yml, heavy_train.yml).  This script runs the reference once and stores what
that test compares against, so that the test runs wherever the repository is checked out.

Weights are NOT stored: they are ``hudiff_amd.synthetic.random_state_dict(kind, CONFIG, seed=5)`` (numpy PCG64, stable
across machines); the fixture carries their SHA-256.  Stored (data only): the two input rows, the reference's logits with
dropout off, its logits with dropout on (torch seed 7) and the keep-masks it drew, in the canonical slot layout.
"""
from __future__ import annotations

import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
sys.path.insert(0, ROOT)
import make_golden as mg  # noqa: E402  (Recorder, canonical_masks, ref_forward)
import make_golden_deep as deep  # noqa: E402  (build, weights_digest)
from hudiff_amd import synthetic as S  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden")
WEIGHT_SEED = 5
B = 2


def main():
    torch.set_num_threads(8)
    for kind in ("ab", "nb"):
        cfg = dict(S.AB_CONFIG if kind == "ab" else S.NB_CONFIG)
        sd = S.random_state_dict(kind, cfg, seed=WEIGHT_SEED)
        batch = S.synthetic_batch(kind, B, seed=17)
        tokens = batch["tokens"].astype(np.int64)
        tokens[1] = np.where(tokens[1] == 22, batch["truth"][1], tokens[1])          # row 1: every slot filled
        region = batch["region"].astype(np.int64)
        chain = None if batch["chain"] is None else batch["chain"].astype(np.int64)
        logits = mg.ref_forward(deep.build(kind, dict(cfg, dropout=0.0), sd), tokens, region, chain)
        ref1 = deep.build(kind, cfg, sd)
        torch.manual_seed(7)
        with mg.Recorder() as rec:
            logits_d = mg.ref_forward(ref1, tokens, region, chain)
        enc, conv = mg.canonical_masks(kind, rec.masks, cfg, B)
        np.savez_compressed(
            os.path.join(OUT, f"prodwidth_{kind}.npz"),
            weight_seed=np.int64(WEIGHT_SEED), weight_sha256=np.array(deep.weights_digest(sd)),
            tokens=tokens, region=region, chain=(np.zeros(0, np.int64) if chain is None else chain),
            logits=logits.astype(np.float32), logits_dropout=logits_d.astype(np.float32),
            enc_masks=np.packbits(enc), conv_masks=np.packbits(conv), enc_shape=np.array(enc.shape), conv_shape=np.array(conv.shape))
        print(kind, "production-width golden written:", logits.shape, "dropout shift", float(np.abs(logits_d - logits).max()))


if __name__ == "__main__":
    main()
