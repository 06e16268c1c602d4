"""The skip-padding schedule with dropout, without a GPU: the fp64 restatement tests/test_ragged_dropout_gpu.py holds the native tape to
(tests/ragged_restated.py) is checked against the padded oracle with dropout off, shown to tell compacted-row masks from padded-position
masks on every case the GPU test runs, its index is checked on a hand-written example, and the cases' claims about the schedule
(csrc/train.hip, plan_rows: which towers end in a tail layer, frames per backward group, longest segments) are checked against the batches.
The case table, the batches and the fp64 references are tests/ragged_cases.py's."""
import numpy as np
import pytest
import torch

import ragged_restated as RR
from oracle import stlt_oracle as O
from ragged_cases import CASES, FLOOR_LOGITS, GRAD_BOUND, case_inputs, grad_errors, is_dead, logit_bound, padded_reference, ragged_reference




def test_ragged_index_on_a_hand_written_example():
    """2 clips, T = 3, N = 3.  Clip 0: frames 0-2 real with slots {0,2}, {0}, {0,1,2} (a masked slot in the middle of frame 0), lengths 3.
    Clip 1: a short clip, frame 0 real with slots {0,1}, frames 1-2 padded (their slot 0 unmasked, as the collater leaves it), lengths 1."""
    kb = torch.tensor([[[0, 1, 0], [0, 1, 1], [0, 0, 0]],
                       [[0, 0, 1], [0, 1, 1], [0, 1, 1]]], dtype=torch.bool)
    kf = torch.tensor([[0, 0, 0], [0, 1, 1]], dtype=torch.bool)
    ix = RR.ragged_index({"src_key_padding_mask_boxes": kb, "src_key_padding_mask_frames": kf, "lengths": torch.tensor([3, 1])})
    flat = lambda b, t, n: (b * 3 + t) * 3 + n  # noqa: E731
    assert ix["t_orig"].tolist() == [flat(0, 0, 0), flat(0, 0, 2), flat(0, 1, 0), flat(0, 2, 0), flat(0, 2, 1), flat(0, 2, 2), flat(1, 0, 0), flat(1, 0, 1)]
    assert ix["t_seg_start"].tolist() == [0, 0, 2, 3, 3, 3, 6, 6]
    assert ix["t_seg_end"].tolist() == [2, 2, 3, 6, 6, 6, 8, 8]
    assert ix["f_orig"].tolist() == [0, 1, 2, 3]
    assert ix["f_seg_start"].tolist() == [0, 0, 0, 3] and ix["f_seg_end"].tolist() == [3, 3, 3, 4]
    assert ix["f_cls_row"].tolist() == [0, 2, 3, 6]
    assert ix["last_row"].tolist() == [2, 3]
    # a masked frame in the middle of a clip is left out and the frames behind it move up; lengths-1 must be real, slot 0 too
    kf2 = torch.tensor([[0, 1, 0], [0, 1, 1]], dtype=torch.bool)
    ix2 = RR.ragged_index({"src_key_padding_mask_boxes": kb, "src_key_padding_mask_frames": kf2, "lengths": torch.tensor([3, 1])})
    assert ix2["f_orig"].tolist() == [0, 2, 3] and ix2["f_cls_row"].tolist() == [0, 2, 5] and ix2["last_row"].tolist() == [1, 2]
    assert ix2["f_seg_end"].tolist() == [2, 2, 3]
    with pytest.raises(ValueError):
        RR.ragged_index({"src_key_padding_mask_boxes": kb, "src_key_padding_mask_frames": kf2, "lengths": torch.tensor([2, 1])})
    kb_bad = kb.clone()
    kb_bad[0, 1, 0] = True
    with pytest.raises(ValueError):
        RR.ragged_index({"src_key_padding_mask_boxes": kb_bad, "src_key_padding_mask_frames": kf, "lengths": torch.tensor([3, 1])})


def test_ragged_attention_mask_indices_on_the_hand_written_example():
    """RaggedDropout.attention against the element index written out by hand: row 4 (clip 0, frame 2, slot 1; its segment starts at row 3),
    head 1 of 2, column 5 is key position 2 -> idx = ((4*2 + 1) << 8) | 2."""
    ix = dict(t_seg_start=np.array([0, 0, 2, 3, 3, 3, 6, 6]), f_seg_start=np.array([0, 0, 0, 3]))
    drop = RR.RaggedDropout(0.5, 77, ix, 2)
    probs = torch.ones(1, 2, 8, 8, dtype=torch.float64)
    for site, (i, h, j, kpos) in ((8, (4, 1, 5, 2)), (16, (7, 0, 6, 0)), (16, (1, 1, 1, 1))):
        keep = O.dropout_keep(0.5, 77, site, np.array([((i * 2 + h) << 8) | kpos], dtype=np.uint64))[0]
        assert drop.attention(site, probs)[0, h, i, j].item() == (drop.scale if keep else 0.0)
    tp = drop.attention(24, torch.ones(1, 2, 4, 4, dtype=torch.float64))  # the first temporal site: the frames' segments
    keep = O.dropout_keep(0.5, 77, 24, np.array([((3 * 2 + 1) << 8) | 0], dtype=np.uint64))[0]
    assert tp[0, 1, 3, 3].item() == (drop.scale if keep else 0.0)


@pytest.mark.parametrize("name", sorted(CASES))
def test_cases_reach_the_schedules_they_claim(name):
    """plan_rows (csrc/train.hip) restated: a tower ends in a tail layer iff twice the rows it picks fit its rows; the spatial backward
    groups floor(32 / N) whole frames (one when N > 32).  And what each case is there for."""
    c = CASES[name]
    batch = case_inputs(name)[1]
    ix = RR.ragged_index(batch)
    n_tok, n_frm, B = len(ix["t_orig"]), len(ix["f_orig"]), c["B"]
    assert n_tok < 300
    assert (2 * n_frm <= n_tok) == c["sp_tail"], (n_tok, n_frm)
    assert (2 * B <= n_frm) == c["tp_tail"], (n_frm, B)
    assert (32 // c["N"] if c["N"] <= 32 else 1) == c["fpg"]
    if c["batch"] == "H":  # stlt_ffn_hidden_bwd (csrc/blocks.hip) fuses the GELU backward into the product only when d % 32 == 0
        assert c["d"] % 32 != 0 and c["d"] % 4 == 0 and c["d"] % c["H"] == 0
    else:
        assert c["d"] % 32 == 0
    sp_len, tp_len = ix["t_seg_end"] - ix["t_seg_start"], ix["f_seg_end"] - ix["f_seg_start"]
    padded_pos = ix["t_orig"] % c["N"]
    inside = np.arange(n_tok) - ix["t_seg_start"]
    if name != "B" and c["batch"] not in ("F",):
        assert n_tok < B * c["T"] * c["N"] and n_tok > n_frm  # something to skip, and frames of more than one token
    if c["batch"] == "B":
        assert n_tok == n_frm
    if c["batch"] == "E":
        assert sp_len.max() == 36 and (inside != padded_pos).any()
    if c["batch"] == "F":
        assert tp_len.max() == 70 and c["T"] > 64
    if c["batch"] == "G":
        assert (inside != padded_pos).any()                                             # a key position that is not the slot number
        assert ((np.arange(n_frm) - ix["f_seg_start"]) != ix["f_orig"] % c["T"]).any()  # a frame position that is not the frame number
    else:
        assert ((np.arange(n_frm) - ix["f_seg_start"]) == ix["f_orig"] % c["T"]).all()
    if c["batch"] in ("A", "D", "H"):
        assert (inside == padded_pos).all()  # the collater fills slots from the left: only the ROW differs from the padded index here


@pytest.mark.parametrize("recipe", sorted({c["batch"] for c in CASES.values()}))
def test_without_dropout_the_restatement_is_the_padded_oracle(recipe):
    """p = 0: stlt_forward_ragged equals O.stlt_forward on the same padded batch in fp64 — logits and every parameter gradient to 1e-10 relative."""
    name = next(n for n in sorted(CASES) if CASES[n]["batch"] == recipe)
    logits, grads = ragged_reference(name, 0.0)
    ref_logits, ref_grads = padded_reference(name, 0.0)
    assert (logits - ref_logits).abs().max().item() <= 1e-10 * ref_logits.abs().max().item()
    errs = grad_errors(grads, ref_grads)
    assert len(errs) == sum(not is_dead(k) for k in ref_grads) and max(errs.values()) <= 1e-10, max(errs.items(), key=lambda kv: kv[1])


@pytest.mark.parametrize("name", sorted(CASES))
def test_compacted_row_masks_are_told_from_padded_position_masks(name):
    """The comparison of the GPU test discriminates: on every (model, batch, p, seed) it runs, the ragged oracle and the padded oracle —
    the same function but for where the masks are drawn — differ in the logits by at least 100 x that case's logit bound, so "the ragged
    kernels used the padded index" cannot pass.  No case is exempt: every batch has padded rows in front of real ones."""
    logits, grads = ragged_reference(name)
    other, other_grads = padded_reference(name)
    gap = (logits - other).abs().max().item()
    print(f"{name}: ragged-vs-padded masks, logits differ by {gap:.3e} ({gap / logit_bound(name):.0f} x the bound {logit_bound(name):.1e})")
    assert gap >= 100 * logit_bound(name)
    k = "backbone.transformer.layers.0.linear1.weight"
    assert grad_errors({k: grads[k]}, {k: other_grads[k]})[k] >= 100 * GRAD_BOUND


@pytest.mark.parametrize("name", sorted(CASES))
def test_fp32_floor_of_the_measured_cases(name):
    """The fp32 rounding floor of the restatement itself (float32 against float64, same masks), printed for every case; where a bound of
    the GPU test is made from it (FLOOR_LOGITS), the recorded figure must be the measured one to within a factor of two."""
    logits, grads = ragged_reference(name)
    l32, g32 = ragged_reference(name, None, torch.float32)
    floor = (l32.double() - logits).abs().max().item()
    errs = grad_errors(g32, grads)
    print(f"{name}: fp32 floor: logits {floor:.2e}, gradients {max(errs.values()):.2e} ({max(errs, key=errs.get)})")
    if name in FLOOR_LOGITS:
        assert 0.5 * FLOOR_LOGITS[name] <= floor <= 2.0 * FLOOR_LOGITS[name], floor
        assert max(errs.values()) <= GRAD_BOUND / 4  # the project's gradient bound already leaves the 4 x
