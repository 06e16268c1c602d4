"""Attention maps restated in plain torch (fp64 by default): TEST INFRASTRUCTURE ONLY.

`ops.attn_probs` (include/stlt_hip.h: stlt_attn_probs_fwd) returns the probabilities the attention core multiplies the values with, and
`Stlt.forward_attention` (stlt_forward_attention) returns them for every encoder layer beside the logits: what the reference's
nn.MultiheadAttention layers (models.py:46-55,118-128) return with need_weights=True.  Both are written here from that header's words with
the oracle's own functions.  tests/test_attention_cpu.py holds this restatement to fixtures captured from the reference's own modules
(tools/gen_golden_attention.py); the GPU tests hold the library to the restatement.
"""
import math

import torch

from oracle import stlt_oracle as O


def attn_probs(qkv: torch.Tensor, kpm: torch.Tensor, causal: bool, H: int, per_head: bool = False) -> torch.Tensor:
    """qkv (S,L,3d) packed [q;k;v], kpm (S,L) bool (True = key masked). -> (S,H,L,L) per head, or their mean over the heads (S,L,L).
    Entry (i, j) is masked when key j is padded or (causal and j > i); masked entries are exactly 0, a row whose keys are all masked is
    zeros.  Query rows are not filtered by kpm."""
    S, L, d3 = qkv.shape
    d = d3 // 3
    dh = d // H
    q, k, _ = qkv.split(d, dim=-1)
    q = q.reshape(S, L, H, dh).transpose(1, 2)
    k = k.reshape(S, L, H, dh).transpose(1, 2)
    masked = kpm.bool()[:, None, :].expand(S, L, L)
    if causal:
        masked = masked | torch.triu(torch.ones(L, L, dtype=torch.bool), diagonal=1)[None]
    s = ((q @ k.transpose(-1, -2)) * (1.0 / math.sqrt(dh))).masked_fill(masked[:, None], float("-inf"))
    p = torch.nan_to_num(torch.softmax(s, dim=-1), nan=0.0)  # a fully masked row: zeros, the core's rule
    return p if per_head else p.mean(dim=1)


def masked_entries(kpm: torch.Tensor, causal: bool) -> torch.Tensor:
    """(S,L,L) bool: the entries attn_probs writes as exactly 0"""
    S, L = kpm.shape
    m = kpm.bool()[:, None, :].expand(S, L, L).clone()
    if causal:
        m |= torch.triu(torch.ones(L, L, dtype=torch.bool), diagonal=1)[None]
    return m


def _layer(x, sd, prefix, kpm, causal, H):
    """one post-norm encoder layer (oracle.encoder_layer's arithmetic) that also hands back its per-head probabilities"""
    w = lambda k: sd[prefix + k]  # noqa: E731
    qkv = x @ w("self_attn.in_proj_weight").t() + w("self_attn.in_proj_bias")
    S, L, _ = x.shape
    masked = masked_entries(kpm, causal)
    a = O.attention_core(qkv, O._neg_inf_mask(masked, x.dtype), H)
    x = O.layer_norm(x + a @ w("self_attn.out_proj.weight").t() + w("self_attn.out_proj.bias"), w("norm1.weight"), w("norm1.bias"), 1e-5)
    h = O.gelu(x @ w("linear1.weight").t() + w("linear1.bias"))
    x = O.layer_norm(x + h @ w("linear2.weight").t() + w("linear2.bias"), w("norm2.weight"), w("norm2.bias"), 1e-5)
    return x, attn_probs(qkv, kpm, causal, H, per_head=True)


def forward_attention(sd, batch, H: int, eps: float = 1e-12, dtype=torch.float64):
    """-> {"stlt": (B,K), "spatial_attention": (n_spatial,B,T,H,N,N), "temporal_attention": (n_temporal,B,H,T,T)}: Stlt.forward
    (models.py:185-195) with every layer run in full on every row, per head; the head-averaged maps are `.mean` over the H axis."""
    sd = {k: (v.to(dtype) if v.is_floating_point() else v) for k, v in sd.items()}
    pre = "backbone."
    FE = pre + "frames_embeddings."
    LE = FE + "layout_embedding."
    B, T, N = batch["categories"].shape
    x = O.category_box_embeddings(sd, LE + "category_box_embeddings.", batch, eps)
    d = x.shape[-1]
    x = x.reshape(B * T, N, d)
    kpm_boxes = batch["src_key_padding_mask_boxes"].reshape(B * T, N)
    spatial, temporal = [], []
    n = 0
    while f"{LE}transformer.layers.{n}.norm1.weight" in sd:
        x, p = _layer(x, sd, f"{LE}transformer.layers.{n}.", kpm_boxes, False, H)
        spatial.append(p.reshape(B, T, H, N, N))
        n += 1
    f = x.reshape(B, T, N, d)[:, :, 0, :]
    P, Ft = sd[FE + "position_embeddings.weight"], sd[FE + "frame_type_embedding.weight"]
    g = O.layer_norm(f + P[:T][None] + Ft[batch["frame_types"]], sd[FE + "layer_norm.weight"], sd[FE + "layer_norm.bias"], eps)
    kpm_frames = batch["src_key_padding_mask_frames"]
    n = 0
    while f"{pre}transformer.layers.{n}.norm1.weight" in sd:
        g, p = _layer(g, sd, f"{pre}transformer.layers.{n}.", kpm_frames, True, H)
        temporal.append(p)
        n += 1
    h = g[torch.arange(B), batch["lengths"] - 1]
    return {"stlt": O.head_forward(sd, h, eps),
            "spatial_attention": torch.stack(spatial) if spatial else torch.zeros(0, B, T, H, N, N, dtype=dtype),
            "temporal_attention": torch.stack(temporal) if temporal else torch.zeros(0, B, H, T, T, dtype=dtype)}
