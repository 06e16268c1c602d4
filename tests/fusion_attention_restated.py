"""The fusion models' attention maps restated in plain torch (fp64 by default): TEST INFRASTRUCTURE ONLY.

`ops.attn_probs_cross` (include/stlt_hip.h: stlt_attn_probs_cross_fwd) returns the probabilities the cross-attention core multiplies the
values with, and `forward_attention` of CrossAttentionFusion / CrossAttentionCentralNetFusion / LateConcatenationFusion
(stlt_caf_forward_attention) returns them for every attention layer beside the logits: what the reference's nn.MultiheadAttention modules
return with need_weights=True (models.py:46-55,118-128, 239-246, 353-388).  Both are written here from that header's words with the
oracles' own functions (oracle.stlt_oracle, oracle.caf_oracle) and tests/attention_restated.py.  tests/test_fusion_attention_cpu.py holds
this restatement to fixtures captured from the reference's own modules (tools/gen_golden_fusion_attention.py); the GPU tests hold the
library to the restatement.  Every map is per head; the head-averaged maps are `.mean` over the H axis.
"""
import math

import torch

import attention_restated as R
from oracle import caf_oracle as CO
from oracle import stlt_oracle as O


def attn_probs_cross(q, k, kpm, causal: bool, H: int, per_head: bool = False):
    """q (S,Lq,d) projected queries, k (S,Lk,d) projected keys, kpm (S,Lk) bool over the keys (True = masked) or None.
    -> (S,H,Lq,Lk) per head, or their mean over the heads (S,Lq,Lk).  Entry (i, j) is masked when key j is padded or (causal and j > i);
    masked entries are exactly 0, a row whose keys are all masked is zeros.  Query rows are not filtered by any mask."""
    S, Lq, d = q.shape
    Lk, dh = k.shape[1], d // H
    qh = q.reshape(S, Lq, H, dh).transpose(1, 2)
    kh = k.reshape(S, Lk, H, dh).transpose(1, 2)
    masked = masked_entries(kpm, causal, S, Lq, Lk)
    s = ((qh @ kh.transpose(-1, -2)) * (1.0 / math.sqrt(dh))).masked_fill(masked[:, None], float("-inf"))
    p = torch.nan_to_num(torch.softmax(s, dim=-1), nan=0.0)  # a fully masked row: zeros, the core's rule
    return p if per_head else p.mean(dim=1)


def masked_entries(kpm, causal: bool, S: int, Lq: int, Lk: int):
    """(S,Lq,Lk) bool: the entries attn_probs_cross writes as exactly 0"""
    m = torch.zeros(S, Lq, Lk, dtype=torch.bool) if kpm is None else kpm.bool()[:, None, :].expand(S, Lq, Lk).clone()
    if causal:
        assert Lq == Lk
        m |= torch.triu(torch.ones(Lq, Lk, dtype=torch.bool), diagonal=1)[None]
    return m


def _layout(sd, pre, batch, H, eps):
    """StltBackbone.forward (models.py:57-81, 136-153) with every layer run in full: -> ((B,T,d) state, spatial (n,B,T,H,N,N), temporal (n,B,H,T,T))"""
    FE = pre + "frames_embeddings."
    LE = FE + "layout_embedding."
    B, T, N = batch["categories"].shape
    x = O.category_box_embeddings(sd, LE + "category_box_embeddings.", batch, eps)
    d, dtype = x.shape[-1], x.dtype
    x = x.reshape(B * T, N, d)
    kpm_boxes = batch["src_key_padding_mask_boxes"].reshape(B * T, N)
    spatial, temporal = [], []
    n = 0
    while f"{LE}transformer.layers.{n}.norm1.weight" in sd:
        x, p = R._layer(x, sd, f"{LE}transformer.layers.{n}.", kpm_boxes, False, H)
        spatial.append(p.reshape(B, T, H, N, N))
        n += 1
    f = x.reshape(B, T, N, d)[:, :, 0, :]
    P, Ft = sd[FE + "position_embeddings.weight"], sd[FE + "frame_type_embedding.weight"]
    g = O.layer_norm(f + P[:T][None] + Ft[batch["frame_types"]], sd[FE + "layer_norm.weight"], sd[FE + "layer_norm.bias"], eps)
    n = 0
    while f"{pre}transformer.layers.{n}.norm1.weight" in sd:
        g, p = R._layer(g, sd, f"{pre}transformer.layers.{n}.", batch["src_key_padding_mask_frames"], True, H)
        temporal.append(p)
        n += 1
    return (g, torch.stack(spatial) if spatial else torch.zeros(0, B, T, H, N, N, dtype=dtype),
            torch.stack(temporal) if temporal else torch.zeros(0, B, H, T, T, dtype=dtype))


def _appearance(sd, pre, feats, H):
    """TransformerResnet.forward_features from the feature map on (models.py:257-271): -> ((B,A,d) tokens, maps (n,B,H,A,A)).  ReLU
    post-norm encoder layers, eps 1e-5, no mask."""
    B, Cc = feats.shape[0], feats.shape[1]
    x = feats.flatten(2).transpose(1, 2) @ sd[pre + "projector.weight"].reshape(-1, Cc).t() + sd[pre + "projector.bias"]
    x = torch.cat((sd[pre + "cls_token"].reshape(1, 1, -1).expand(B, -1, -1), x), dim=1) + sd[pre + "pos_embed"].reshape(1, -1, x.shape[-1])
    A, d = x.shape[1], x.shape[2]
    maps = []
    n = 0
    while f"{pre}transformer.layers.{n}.norm1.weight" in sd:
        w = lambda k: sd[f"{pre}transformer.layers.{n}.{k}"]  # noqa: E731
        qkv = x @ w("self_attn.in_proj_weight").t() + w("self_attn.in_proj_bias")
        a = O.attention_core(qkv, torch.zeros(B, A, A, dtype=x.dtype), H)
        maps.append(attn_probs_cross(qkv[..., :d], qkv[..., d:2 * d], None, False, H, per_head=True))
        x = O.layer_norm(x + a @ w("self_attn.out_proj.weight").t() + w("self_attn.out_proj.bias"), w("norm1.weight"), w("norm1.bias"), 1e-5)
        h = torch.relu(x @ w("linear1.weight").t() + w("linear1.bias"))
        x = O.layer_norm(x + h @ w("linear2.weight").t() + w("linear2.bias"), w("norm2.weight"), w("norm2.bias"), 1e-5)
        n += 1
    return x, torch.stack(maps) if maps else torch.zeros(0, B, H, A, A, dtype=x.dtype)


def _block(sd, pre, x, ctx, H, eps, kpm_k, causal):
    """SelfAttentionLayer (ctx is x) / CrossAttentionLayer (models.py:345-382) through the oracle, and the block's per-head probabilities
    from its own in-projection: queries from x, keys from ctx"""
    d = x.shape[-1]
    W, b = sd[pre + "attn.in_proj_weight"], sd[pre + "attn.in_proj_bias"]
    probs = attn_probs_cross(x @ W[:d].t() + b[:d], ctx @ W[d:2 * d].t() + b[d:2 * d], kpm_k, causal, H, per_head=True)
    return CO.attn_layer(sd, pre, x, ctx, H, eps, kpm_k=kpm_k, causal=causal, dtype=x.dtype), probs


def forward_attention(model_name: str, sd, batch, H: int, eps: float = 1e-12, dtype=torch.float64):
    """model_name in ("caf", "cacnf", "lcf").  -> the model's logits under their names and, per head,
    spatial_attention (n_spatial,B,T,H,N,N), temporal_attention (n_temporal,B,H,T,T), appearance_attention (n_app,B,H,A,A),
    layout_to_appearance (n_fusion,B,H,T,A), appearance_to_layout (n_fusion,B,H,A,T), fusion_layout_attention (n_fusion,B,H,T,T),
    fusion_appearance_attention (n_fusion,2,B,H,A,A): CrossAttentionFusionBackbone.forward (models.py:446-483) with every layer run in full."""
    sd = {k: (v.to(dtype) if v.is_floating_point() else v) for k, v in sd.items()}
    pre = {"caf": "caf_backbone.", "cacnf": "backbone.", "lcf": ""}[model_name]
    B, T, N = batch["categories"].shape
    Lh, spatial, temporal = _layout(sd, pre + "layout_branch.", batch, H, eps)
    Ah, appearance = _appearance(sd, pre + "appearance_branch.", batch["appearance_features"].to(dtype), H)
    A = Ah.shape[1]
    idx = torch.arange(B)
    lay_state, app_state = Lh[idx, batch["lengths"] - 1], Ah[:, 0]
    kpm = batch["src_key_padding_mask_frames"]
    l2a, a2l, f_lay, f_app = [], [], [], []
    n = 0
    while f"{pre}mm_fusion.{n}.cross_attn.ln.weight" in sd:  # CrossModalModule.forward, models.py:403-431
        m = f"{pre}mm_fusion.{n}."
        la, p = _block(sd, m + "cross_attn.", Lh, Ah, H, eps, None, False)
        l2a.append(p)
        aa, p = _block(sd, m + "cross_attn.", Ah, Lh, H, eps, kpm, False)
        a2l.append(p)
        la, p = _block(sd, m + "layout_attn.", la, la, H, eps, kpm, True)
        f_lay.append(p)
        aa, p0 = _block(sd, m + "appearance_attn.", aa, aa, H, eps, None, False)
        f = O.gelu(la @ sd[m + "layout_ffn.linear1.weight"].t() + sd[m + "layout_ffn.linear1.bias"])
        f = f @ sd[m + "layout_ffn.linear2.weight"].t() + sd[m + "layout_ffn.linear2.bias"]
        Lh = O.layer_norm(f + la, sd[m + "layout_ffn.ln.weight"], sd[m + "layout_ffn.ln.bias"], eps)
        Ah, p1 = _block(sd, m + "appearance_ffn.", aa, aa, H, eps, None, False)  # a SelfAttentionLayer (models.py:401)
        f_app.append(torch.stack((p0, p1)))
        n += 1
    fused = torch.cat((Lh[idx, batch["lengths"] - 1], Ah[:, 0]), dim=-1)
    stack = lambda xs, *shape: torch.stack(xs) if xs else torch.zeros(0, *shape, dtype=dtype)  # noqa: E731
    out = {"spatial_attention": spatial, "temporal_attention": temporal, "appearance_attention": appearance,
           "layout_to_appearance": stack(l2a, B, H, T, A), "appearance_to_layout": stack(a2l, B, H, A, T),
           "fusion_layout_attention": stack(f_lay, B, H, T, T), "fusion_appearance_attention": stack(f_app, 2, B, H, A, A)}
    if model_name == "cacnf":
        out["stlt"] = O.head_forward(sd, lay_state, eps, prefix="layout_classifier.")
        out["resnet3d"] = O.head_forward(sd, app_state, eps, prefix="appearance_classifier.")
        out["caf"] = O.head_forward(sd, fused, eps, prefix="fusion_classifier.")
        out["ensemble"] = (out["stlt"] + out["resnet3d"] + out["caf"]) / 3
    else:
        out[model_name] = O.head_forward(sd, fused, eps, prefix="classifier.")
    return out


MAP_KEYS = ("spatial_attention", "temporal_attention", "appearance_attention", "layout_to_appearance", "appearance_to_layout",
            "fusion_layout_attention", "fusion_appearance_attention")
# fixture array of each map (tests/golden/*_attention_cfg1.npz)
FIXTURE_KEYS = dict(zip(MAP_KEYS, ("spatial", "temporal", "appearance", "layout_to_appearance", "appearance_to_layout", "fusion_layout", "fusion_appearance")))


def head_mean(maps):
    """per-head maps -> head-averaged maps (the H axis is third from the end)"""
    return {k: maps[k].mean(dim=-3) for k in MAP_KEYS}
