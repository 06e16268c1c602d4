"""The skip-padding (ragged) schedule of the native training tape, restated on the oracle's building blocks.  TEST INFRASTRUCTURE ONLY.

Plain numpy / torch, nothing imported from the package under test.  The padded schedule and the ragged one compute the same function
while dropout is off (a padded row never reaches a real one); with dropout on they do not, because the counter-based masks are drawn
from (seed, site, element index) and the ragged schedule's element indices are those of the COMPACTED rows (csrc/train.hip, plan_open:
"dropout masks are drawn per compacted row"; csrc/ragged.hip's header and ragged_fill_kernel define the compaction):

  * element-wise sites (both embedding outputs, dropout1, the FFN hidden, dropout2): idx = row * width + e with `row` the row of the
    compacted (n_rows, width) buffer — width d everywhere but the FFN hidden, which is 4d wide (rowwise.hip embed / frames_embed / add_ln
    kernels: `row * d`; gelu_fwd_kernel's drop_index and the GELU_KEEP / GELU_BWD product epilogues: `drow * N` with N = 4d).  A tail layer
    computes the picked rows only and hands the kernels `drop_rows` = the picked rows' own compacted rows, so it draws the masks those
    rows would have had: computing every row and picking afterwards — what this file does — is the same function.
  * attention probabilities: idx = ((query row * H + head) << 8) | (key row - first row of the query's segment) & 0xff, with compacted
    rows on both sides (attn.hip's VARLEN branch, attn_any.hip's key_pos, attn_bwd16.hip's RAGGED meta_of, backward.hip's ragged
    attn_bwd_kernel and attn_bwd_long_kernel, whose group is one segment).
"""
from __future__ import annotations

from typing import Dict

import numpy as np
import torch

from oracle import stlt_oracle as O


def ragged_index(batch: Dict[str, torch.Tensor]) -> Dict[str, np.ndarray]:
    """The compaction csrc/ragged.hip defines.  A frame is real iff its frame-mask byte is 0; a token is real iff its frame is real and
    its box-mask byte is 0.  Real tokens keep (clip, frame, slot) order, real frames (clip, frame) order; a frame's tokens are one
    spatial segment, a clip's frames one temporal segment.  The contract ragged_fill_kernel enforces: slot 0 of every real frame is
    real, and frame lengths-1 of every clip is real.
      t_orig (n_tok,) flat (b*T + t)*N + n        t_seg_start / t_seg_end (n_tok,)   the token's frame as rows [start, end)
      f_orig (n_frm,) flat b*T + t                f_seg_start / f_seg_end (n_frm,)   the frame's clip as rows [start, end)
      f_cls_row (n_frm,) token row of the frame's slot 0           last_row (B,) frame row of frame lengths-1"""
    kb = batch["src_key_padding_mask_boxes"].numpy().astype(bool)
    kf = batch["src_key_padding_mask_frames"].numpy().astype(bool)
    lengths = batch["lengths"].numpy()
    B, T, N = kb.shape
    t_orig, t_s, t_e, f_orig, f_s, f_e, f_cls, last = [], [], [], [], [], [], [], []
    for b in range(B):
        frm0 = len(f_orig)
        n_frm = int((~kf[b]).sum())
        row_of = {}
        for t in range(T):
            if kf[b, t]:
                continue
            if kb[b, t, 0]:
                raise ValueError(f"clip {b} frame {t}: slot 0 of a real frame is masked")
            slots = [n for n in range(N) if not kb[b, t, n]]
            row0 = len(t_orig)
            row_of[t] = len(f_orig)
            f_orig.append(b * T + t)
            f_cls.append(row0)
            f_s.append(frm0)
            f_e.append(frm0 + n_frm)
            for n in slots:
                t_orig.append((b * T + t) * N + n)
                t_s.append(row0)
                t_e.append(row0 + len(slots))
        t_last = int(lengths[b]) - 1
        t_last = t_last + T if t_last < 0 else t_last
        if t_last not in row_of:
            raise ValueError(f"clip {b}: frame lengths-1 = {t_last} is not a real frame")
        last.append(row_of[t_last])
    arr = lambda v: np.asarray(v, dtype=np.int64)  # noqa: E731
    return dict(t_orig=arr(t_orig), t_seg_start=arr(t_s), t_seg_end=arr(t_e), f_orig=arr(f_orig), f_seg_start=arr(f_s), f_seg_end=arr(f_e),
                f_cls_row=arr(f_cls), last_row=arr(last), shape=(B, T, N))


class RaggedDropout(O.Dropout):
    """The masks of the ragged schedule.  `elementwise` is the base class's (flat index over the (1, n_rows, width) tensor it is given:
    row * width + e, the FFN hidden with width 4d — confirmed from the kernels, see the module docstring).  `attention` takes the
    (1, H, n, n) probabilities over the compacted rows of a tower: element (row i, head h, column j) uses
    idx = ((i*H + h) << 8) | ((j - seg_start[i]) & 0xff).  Which tower a site belongs to follows from the site number: the spatial layers
    are sites 8*(l+1), l < n_spatial, the temporal ones follow."""

    def __init__(self, p: float, seed: int, index: Dict[str, np.ndarray], n_spatial: int):
        super().__init__(p, seed)
        self.index, self.n_spatial = index, int(n_spatial)

    def attention(self, site: int, probs: torch.Tensor) -> torch.Tensor:
        if self.p <= 0:
            return probs
        seg_start = self.index["t_seg_start" if site < 8 * (self.n_spatial + 1) else "f_seg_start"]
        one, H, n, n2 = probs.shape
        assert one == 1 and n == n2 == len(seg_start), (probs.shape, len(seg_start))
        h_, i_, j_ = np.meshgrid(np.arange(H, dtype=np.int64), np.arange(n, dtype=np.int64), np.arange(n, dtype=np.int64), indexing="ij")
        kpos = (j_ - seg_start[i_]) & 0xFF  # (columns outside the row's segment carry probability 0: their index does not matter)
        idx = (((i_ * H + h_) << 8) | kpos).astype(np.uint64)
        keep = O.dropout_keep(self.p, self.seed, site, idx)[None]
        return probs * (torch.from_numpy(keep).to(probs.dtype) * self.scale)


def _segment_mask(seg_start: np.ndarray, seg_end: np.ndarray, causal: bool, dtype) -> torch.Tensor:
    """(1, n, n) additive mask: 0 where column j lies inside row i's segment (and j <= i when causal), -inf elsewhere."""
    n = len(seg_start)
    j = np.arange(n)[None, :]
    ok = (j >= seg_start[:, None]) & (j < seg_end[:, None])
    if causal:
        ok &= j <= np.arange(n)[:, None]
    return torch.zeros(1, n, n, dtype=dtype).masked_fill(torch.from_numpy(~ok)[None], float("-inf"))


def stlt_forward_ragged(sd: Dict[str, torch.Tensor], batch: Dict[str, torch.Tensor], H: int, drop=None, layer_norm_eps: float = 1e-12,
                        dtype=torch.float64) -> Dict[str, torch.Tensor]:
    """Stlt.forward on the real rows only, in the order of stlt_train_forward with STLT_FLAG_SKIP_PADDING.  `drop`: None, or a
    RaggedDropout built on `ragged_index(batch)`.  -> {"stlt": (B, num_classes)}"""
    ix = drop.index if drop is not None else ragged_index(batch)
    B, T, N = ix["shape"]
    sd = {k: (v.to(dtype) if v.is_floating_point() else v) for k, v in sd.items()}
    batch = {k: (v.to(dtype) if v.is_floating_point() else v) for k, v in batch.items()}
    dz = (lambda site, t: drop.elementwise(site, t)) if drop is not None else (lambda site, t: t)
    FE = "backbone.frames_embeddings."
    LE = FE + "layout_embedding."
    # category / box / score embeddings of the padded batch, the real tokens gathered, the embedding dropout over the compacted rows
    x = O.category_box_embeddings(sd, LE + "category_box_embeddings.", batch, layer_norm_eps)
    d = x.shape[-1]
    x = dz(O.SITE_EMBED, x.reshape(B * T * N, d)[torch.from_numpy(ix["t_orig"])])[None]
    m_sp = _segment_mask(ix["t_seg_start"], ix["t_seg_end"], False, dtype)
    n_sp = 0
    while f"{LE}transformer.layers.{n_sp}.norm1.weight" in sd:
        x = O.encoder_layer(x, sd, f"{LE}transformer.layers.{n_sp}.", m_sp, H, drop, 8 * (n_sp + 1))
        n_sp += 1
    if drop is not None:
        assert n_sp == drop.n_spatial, (n_sp, drop.n_spatial)
    # the CLS row of every real frame + the frame's own position and type
    f = x[0][torch.from_numpy(ix["f_cls_row"])]
    t_of = torch.from_numpy(ix["f_orig"] % T)
    types = batch["frame_types"].reshape(B * T)[torch.from_numpy(ix["f_orig"])]
    g = O.layer_norm(f + sd[FE + "position_embeddings.weight"][t_of] + sd[FE + "frame_type_embedding.weight"][types],
                     sd[FE + "layer_norm.weight"], sd[FE + "layer_norm.bias"], layer_norm_eps)
    x = dz(O.SITE_FRAMES, g)[None]
    m_tp = _segment_mask(ix["f_seg_start"], ix["f_seg_end"], True, dtype)
    n_tp = 0
    while f"backbone.transformer.layers.{n_tp}.norm1.weight" in sd:
        x = O.encoder_layer(x, sd, f"backbone.transformer.layers.{n_tp}.", m_tp, H, drop, 8 * (n_sp + n_tp + 1))
        n_tp += 1
    h = x[0][torch.from_numpy(ix["last_row"])]
    return {"stlt": O.head_forward(sd, h, layer_norm_eps)}
