"""CPU oracle of CAF / CACNF on precomputed appearance features.  TEST INFRASTRUCTURE ONLY (see stlt_oracle.py header).

Plain-tensor restatement of the reference's CrossAttentionFusionBackbone / CrossAttentionFusion /
CrossAttentionCentralNetFusion (src/modelling/models.py:434-549) with the appearance branch starting from the feature
map that Resnet3D.forward_features returns (models.py:221-222, 253-271).  Pinned by tests/golden/caf_*.npz, captured from
the reference's own modules (tools/gen_golden_caf.py).

``dtype`` runs the whole restatement in that precision (float64 for gradient checks: an fp32 oracle is itself off by
rounding wherever a ReLU / GELU input sits within an ulp of zero).  ``drop`` (a ``stlt_oracle.CallSeeds``) applies the
training composition's dropout masks (modelling/fusion.py ``run_train``): one seed per native call in forward order —
the layout branch (its tape, or its op-level calls), then the appearance encoder (two block calls per layer at the fixed
rate 0.1 of nn.TransformerEncoderLayer), then six block calls per cross-modal layer at ``hidden_dropout_prob``.
"""
import math
from typing import Dict, Optional

import torch

from . import stlt_oracle as O

APPEARANCE_DROPOUT = 0.1  # nn.TransformerEncoderLayer's default dropout, which TransformerResnet does not override


def _cast(sd, dtype, pre=""):
    return {k: (v.to(dtype) if v.is_floating_point() else v) for k, v in sd.items() if k.startswith(pre)}


def _block(drop: Optional[O.CallSeeds], kind, shape, p):
    return drop.take(kind, shape, p) if drop is not None else None


def mha(sd, pre, q_in, kv_in, H, kpm_k=None, causal=False, dtype=torch.float32, drop: Optional[O.Dropout] = None,
        site: int = O.CallSeeds.SITE_BLOCK):
    """nn.MultiheadAttention forward (batch-major here): q_in (B,Lq,d), kv_in (B,Lk,d) -> (B,Lq,d).  ``drop`` masks the
    attention probabilities (after the softmax, before ·V) at ``site``."""
    sd = _cast(sd, dtype, pre)
    q_in, kv_in = q_in.to(dtype), kv_in.to(dtype)
    W, b = sd[pre + "in_proj_weight"], sd[pre + "in_proj_bias"]
    d = q_in.shape[-1]
    q = q_in @ W[:d].t() + b[:d]
    k = kv_in @ W[d:2 * d].t() + b[d:2 * d]
    v = kv_in @ W[2 * d:].t() + b[2 * d:]
    B, Lq, Lk, dh = q.shape[0], q.shape[1], k.shape[1], d // H
    qh = q.reshape(B, Lq, H, dh).transpose(1, 2)
    kh = k.reshape(B, Lk, H, dh).transpose(1, 2)
    vh = v.reshape(B, Lk, H, dh).transpose(1, 2)
    s = qh @ kh.transpose(-1, -2) / math.sqrt(dh)
    if kpm_k is not None:
        s = s.masked_fill(kpm_k[:, None, None, :], float("-inf"))
    if causal:
        s = s.masked_fill(torch.triu(torch.ones(Lq, Lk, dtype=torch.bool), diagonal=1), float("-inf"))
    pr = torch.softmax(s, -1)
    if drop is not None:
        pr = drop.attention(site, pr)
    o = (pr @ vh).transpose(1, 2).reshape(B, Lq, d)
    return o @ sd[pre + "out_proj.weight"].t() + sd[pre + "out_proj.bias"]


def attn_layer(sd, pre, x, ctx, H, eps, kpm_k=None, causal=False, dtype=torch.float32, drop: Optional[O.Dropout] = None):
    """SelfAttentionLayer (ctx is x) / CrossAttentionLayer, models.py:345-382: LN(drop(MHA(x, ctx, ctx)) + x).  ``drop`` is
    the block call's mask source: probabilities at SITE_BLOCK, the dropout in front of the residual at SITE_BLOCK + 1."""
    sd = _cast(sd, dtype, pre)
    x, ctx = x.to(dtype), ctx.to(dtype)
    a = mha(sd, pre + "attn.", x, ctx, H, kpm_k, causal, dtype, drop)
    if drop is not None:
        a = drop.elementwise(O.CallSeeds.SITE_BLOCK + 1, a)
    return O.layer_norm(a + x, sd[pre + "ln.weight"], sd[pre + "ln.bias"], eps)


def appearance_forward(sd, pre, feats, H, dtype=torch.float32, drop: Optional[O.CallSeeds] = None):
    """TransformerResnet.forward_features from the feature map on, models.py:257-271. -> (B, S+1, d)"""
    sd = _cast(sd, dtype, pre)
    feats = feats.to(dtype)
    B, Cc = feats.shape[0], feats.shape[1]
    Wp = sd[pre + "projector.weight"].reshape(-1, Cc)
    x = feats.flatten(2).transpose(1, 2) @ Wp.t() + sd[pre + "projector.bias"]            # (B,S,d)
    x = torch.cat((sd[pre + "cls_token"].reshape(1, 1, -1).expand(B, -1, -1), x), dim=1)
    x = x + sd[pre + "pos_embed"].reshape(1, -1, x.shape[-1])
    L = x.shape[1]
    l = 0
    while f"{pre}transformer.layers.{l}.norm1.weight" in sd:  # ReLU encoder layers (nn.TransformerEncoderLayer default)
        p = lambda k: sd[f"{pre}transformer.layers.{l}.{k}"]
        da = _block(drop, "attn", (B, L, L), APPEARANCE_DROPOUT)
        df = _block(drop, "ffn", (B * L,), APPEARANCE_DROPOUT)
        a = mha({k[len(f"{pre}transformer.layers.{l}.self_attn."):]: v for k, v in sd.items()
                 if k.startswith(f"{pre}transformer.layers.{l}.self_attn.")}, "", x, x, H, dtype=dtype, drop=da)
        if da is not None:
            a = da.elementwise(O.CallSeeds.SITE_BLOCK + 1, a)
        x = O.layer_norm(x + a, p("norm1.weight"), p("norm1.bias"), 1e-5)
        h = torch.relu(x @ p("linear1.weight").t() + p("linear1.bias"))
        if df is None:  # (x + h W2ᵀ) + b2: the fp32 defaults keep their order of additions (the goldens pin them)
            x = O.layer_norm(x + h @ p("linear2.weight").t() + p("linear2.bias"), p("norm2.weight"), p("norm2.bias"), 1e-5)
        else:  # inner dropout after the ReLU at site0, dropout2 at site0 + 1
            h = df.elementwise(O.CallSeeds.SITE_BLOCK, h)
            f = df.elementwise(O.CallSeeds.SITE_BLOCK + 1, h @ p("linear2.weight").t() + p("linear2.bias"))
            x = O.layer_norm(x + f, p("norm2.weight"), p("norm2.bias"), 1e-5)
        l += 1
    return x


def backbone(sd, pre, batch, H, eps, dtype=torch.float32, drop: Optional[O.CallSeeds] = None, p: float = 0.0):
    """CrossAttentionFusionBackbone.forward, models.py:446-483 (batch-major).  ``p``: hidden_dropout_prob (with ``drop``)."""
    sd = _cast(sd, dtype, pre)
    B, T, N = batch["categories"].shape
    lay_drop = None
    if drop is not None and drop.layout == "tape":
        lay_drop = drop.take("tape", (B, T, N), p)
    elif drop is not None and drop.layout == "ops":
        lay_drop = drop
    Lh = O.backbone_forward(sd, batch, H, eps, prefix=pre + "layout_branch.", dtype=dtype, drop=lay_drop, drop_p=p)
    Ah = appearance_forward(sd, pre + "appearance_branch.", batch["appearance_features"], H, dtype, drop)
    idx = torch.arange(B)
    lay_state, app_state = Lh[idx, batch["lengths"] - 1], Ah[:, 0]
    kpm = batch["src_key_padding_mask_frames"]
    S1 = Ah.shape[1]
    l = 0
    while f"{pre}mm_fusion.{l}.cross_attn.ln.weight" in sd:  # CrossModalModule.forward, models.py:403-431
        m = f"{pre}mm_fusion.{l}."
        la = attn_layer(sd, m + "cross_attn.", Lh, Ah, H, eps, dtype=dtype, drop=_block(drop, "attn", (B, T, S1), p))
        aa = attn_layer(sd, m + "cross_attn.", Ah, Lh, H, eps, kpm_k=kpm, dtype=dtype, drop=_block(drop, "attn", (B, S1, T), p))
        la = attn_layer(sd, m + "layout_attn.", la, la, H, eps, kpm_k=kpm, causal=True, dtype=dtype,
                        drop=_block(drop, "attn", (B, T, T), p))
        aa = attn_layer(sd, m + "appearance_attn.", aa, aa, H, eps, dtype=dtype, drop=_block(drop, "attn", (B, S1, S1), p))
        df = _block(drop, "ffn", (B * T,), p)
        f = O.gelu(la @ sd[m + "layout_ffn.linear1.weight"].t() + sd[m + "layout_ffn.linear1.bias"])
        f = f @ sd[m + "layout_ffn.linear2.weight"].t() + sd[m + "layout_ffn.linear2.bias"]
        if df is not None:  # no inner dropout in the fusion models' feed-forward block (models.py:384-401)
            f = df.elementwise(O.CallSeeds.SITE_BLOCK + 1, f)
        Lh = O.layer_norm(f + la, sd[m + "layout_ffn.ln.weight"], sd[m + "layout_ffn.ln.bias"], eps)
        # appearance_ffn is a SelfAttentionLayer (models.py:401)
        Ah = attn_layer(sd, m + "appearance_ffn.", aa, aa, H, eps, dtype=dtype, drop=_block(drop, "attn", (B, S1, S1), p))
        l += 1
    fused = torch.cat((Lh[idx, batch["lengths"] - 1], Ah[:, 0]), dim=-1)
    return lay_state, app_state, fused


def caf_forward(sd, batch, H, eps=1e-12, dtype=torch.float32, drop: Optional[O.CallSeeds] = None, p: float = 0.0
                ) -> Dict[str, torch.Tensor]:
    sd = _cast(sd, dtype)
    _, _, fused = backbone(sd, "caf_backbone.", batch, H, eps, dtype, drop, p)
    return {"caf": O.head_forward(sd, fused, eps, prefix="classifier.")}


def cacnf_forward(sd, batch, H, eps=1e-12, dtype=torch.float32, drop: Optional[O.CallSeeds] = None, p: float = 0.0
                  ) -> Dict[str, torch.Tensor]:
    sd = _cast(sd, dtype)
    lay, app, fused = backbone(sd, "backbone.", batch, H, eps, dtype, drop, p)
    out = {"stlt": O.head_forward(sd, lay, eps, prefix="layout_classifier."),
           "resnet3d": O.head_forward(sd, app, eps, prefix="appearance_classifier."),
           "caf": O.head_forward(sd, fused, eps, prefix="fusion_classifier.")}
    out["ensemble"] = (out["stlt"] + out["resnet3d"] + out["caf"]) / 3
    return out


def lcf_forward(sd, batch, H, eps=1e-12, dtype=torch.float32, drop: Optional[O.CallSeeds] = None, p: float = 0.0
                ) -> Dict[str, torch.Tensor]:
    """LateConcatenationFusion.forward, models.py:296-322: FusionHead on [layout state at lengths-1 ; appearance CLS state]
    (the backbone above with no cross-modal module and no key prefix)."""
    sd = _cast(sd, dtype)
    _, _, fused = backbone(sd, "", batch, H, eps, dtype, drop, p)
    return {"lcf": O.head_forward(sd, fused, eps, prefix="classifier.")}
