"""f-1 evidence held by the reference's DATA (VERDICT r2 "Next" #6b): HuAb348 ships each mouse antibody with its
experimentally humanized partner.  CDR grafting keeps the CDR residues, so under a consistent numbering both partners carry
the same residues in the same CDR slots.  The yard-stick is numbering-free (a Needleman-Wunsch alignment of the raw chains,
tests/golden/make_pair_cdr_fixture.py): every pair whose Kabat CDRs are >= 95 % identical by alignment must be >= 95 %
identical SLOT FOR SLOT as numbered by hudiff_amd.numbering; the few graft pairs whose residues do not all land in the same
slots are listed in tests/golden/pair_cdr_review.json (where an ANARCI run should look first)."""
import json
import os
import sys

import numpy as np

from conftest import GOLDEN
from hudiff_amd import evalsets as E

sys.path.insert(0, GOLDEN)
from make_pair_cdr_fixture import pair_cdr_numbers  # noqa: E402


def test_humanized_partners_share_cdr_slots_with_their_mouse_antibodies():
    z = np.load(os.path.join(GOLDEN, "huab348_humanized_partners.npz"))
    M, H = E.load_rows()["huab348_tokens"], z["tokens"]
    assert M.shape == H.shape == (348, 291)
    rows = [pair_cdr_numbers(M[i], H[i]) for i in range(348)]
    slot_id, nw_id, same_slot = (np.array([r[k] for r in rows]) for k in (1, 2, 3))
    graft = nw_id >= 0.95
    assert graft.sum() >= 280                                   # 289 of the 348 pairs are CDR grafts by the numbering-free criterion
    assert (slot_id[graft] >= 0.95).all(), [str(z["names"][i]) for i in np.where(graft & (slot_id < 0.95))[0]]
    assert ((slot_id >= 0.95) == graft).all()                   # and no pair looks like a graft only through the numbering
    assert slot_id[graft].mean() > 0.985 and (slot_id[graft] == nw_id[graft]).mean() > 0.98      # almost always the very same number
    listed = {p["pair"] for p in json.load(open(os.path.join(GOLDEN, "pair_cdr_review.json")))["pairs"]}
    shifted = {str(z["names"][i]) for i in np.where(graft & (same_slot < 1.0) & (slot_id < 1.0))[0]}
    assert shifted == listed and len(listed) <= 6               # the exceptions are exactly the committed review list
    # the slot identity can never exceed what an optimal alignment finds by more than ties allow
    assert (slot_id <= nw_id + 1e-9).all()


def test_partner_fixture_is_what_the_slotter_gives_today():
    """The stored partner tokens are what hudiff_amd.numbering makes of the humanized partners' raw chains today."""
    from hudiff_amd import inputs as I
    from hudiff_amd.numbering import number_sequence_builtin
    seqs = json.load(open(os.path.join(GOLDEN, "huab348_humanized_partner_seqs.json")))
    assert len(seqs["h_seq"]) == len(seqs["l_seq"]) == 348
    z = np.load(os.path.join(GOLDEN, "huab348_humanized_partners.npz"))
    for i in range(0, 348, 7):
        h_seq, l_seq = seqs["h_seq"][i], seqs["l_seq"][i]
        tok = np.array(I._TK.seq2idx(I.slot_residues(number_sequence_builtin(h_seq)[0], "H") +
                                     I.slot_residues(number_sequence_builtin(l_seq)[0], "L")))
        assert np.array_equal(tok, z["tokens"][i].astype(tok.dtype)), i
