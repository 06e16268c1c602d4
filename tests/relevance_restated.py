"""Attention relevance restated in plain torch (fp64 by default): TEST INFRASTRUCTURE ONLY.

`Stlt.forward_relevance` (include/stlt_hip.h: stlt_train_backward_relevance) returns gradient-weighted attention rollout (Chefer, Gur, Wolf
2021).  Written here straight from that header's formulas, on a differentiable forward in the style of tests/attention_restated.py: the
oracle's own functions for the embedding, LayerNorm, GELU and the head, and each layer's attention output written as ctx_h = P_h @ V_h with
P_h a graph node, so that G_h — the gradient wrt P_h as an independent variable — is what torch.autograd.grad gives for it.

    abar[s,i,j] = (1/H) sum_h max(P_h[s,i,j] * G_h[s,i,j], 0)         per layer
    R_0 = I,  R_l = R_{l-1} + abar_l @ R_{l-1}                        per tower
    rel[b,t,n] = R_temporal[b, lengths[b]-1, t] * R_spatial[b,t,0,n]
"""
import torch

import attention_restated as AR
from oracle import stlt_oracle as O


def _layer(x, sd, prefix, kpm, causal, H, nodes):
    """one post-norm encoder layer (oracle.encoder_layer's arithmetic) with ctx_h = P_h @ V_h; appends (P, V, ctx) — (S,H,L,L), (S,H,L,dh),
    (S,H,L,dh) graph nodes — to `nodes`"""
    w = lambda k: sd[prefix + k]  # noqa: E731
    qkv = x @ w("self_attn.in_proj_weight").t() + w("self_attn.in_proj_bias")
    S, L, d3 = qkv.shape
    d = d3 // 3
    P = AR.attn_probs(qkv, kpm, causal, H, per_head=True)
    V = qkv[..., 2 * d:].reshape(S, L, H, d // H).transpose(1, 2)
    ctx = P @ V
    nodes.append((P, V, ctx))
    a = ctx.transpose(1, 2).reshape(S, L, d)
    x = O.layer_norm(x + a @ w("self_attn.out_proj.weight").t() + w("self_attn.out_proj.bias"), w("norm1.weight"), w("norm1.bias"), 1e-5)
    h = O.gelu(x @ w("linear1.weight").t() + w("linear1.bias"))
    return O.layer_norm(x + h @ w("linear2.weight").t() + w("linear2.bias"), w("norm2.weight"), w("norm2.bias"), 1e-5)


def forward(sd, batch, H: int, eps: float = 1e-12, dtype=torch.float64):
    """Stlt.forward (models.py:185-195) -> (logits (B,K), spatial nodes, temporal nodes): per layer the (P, V, ctx) graph nodes of _layer"""
    sd = {k: (v.to(dtype) if v.is_floating_point() else v) for k, v in sd.items()}
    batch = {k: (v.to(dtype) if v.is_floating_point() else v) for k, v in batch.items()}
    batch["boxes"] = batch["boxes"].clone().requires_grad_(True)  # a leaf, so that every P below is a node of the graph
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
        x = _layer(x, sd, f"{LE}transformer.layers.{n}.", kpm_boxes, False, H, spatial)
        n += 1
    f = x.reshape(B, T, N, d)[:, :, 0, :]  # models.py:79
    P, Ft = sd[FE + "position_embeddings.weight"], sd[FE + "frame_type_embedding.weight"]
    g = O.layer_norm(f + P[:T][None] + Ft[batch["frame_types"]], sd[FE + "layer_norm.weight"], sd[FE + "layer_norm.bias"], eps)
    n = 0
    while f"{pre}transformer.layers.{n}.norm1.weight" in sd:
        g = _layer(g, sd, f"{pre}transformer.layers.{n}.", batch["src_key_padding_mask_frames"], True, H, temporal)
        n += 1
    h = g[torch.arange(B), batch["lengths"] - 1]  # models.py:189-192
    return O.head_forward(sd, h, eps), spatial, temporal


def seed_of(logits, target):
    """d(objective)/d(logits) for the three target forms (stlt_saliency_seed) -> (seed (B,K), the classes or None)"""
    if isinstance(target, torch.Tensor) and target.is_floating_point():
        return target.to(logits.dtype), None
    classes = logits.detach().argmax(dim=1) if target is None else target  # argmax: the lowest index on ties
    return torch.nn.functional.one_hot(classes, logits.shape[1]).to(logits.dtype), classes


def grad_probs(logits, seed, nodes):
    """[G (S,H,L,L)] per layer: the gradient of sum(seed * logits) wrt each layer's P as an independent variable"""
    return list(torch.autograd.grad((logits * seed).sum(), [P for P, _, _ in nodes], retain_graph=True))


def abar_of(P, G):
    return (P * G).clamp(min=0).mean(dim=1)


def rollout(abar):
    """abar (n_layers, S, L, L), or a list of (S, L, L), with at least one layer -> R (S, L, L)"""
    R = None
    for a in abar:
        if R is None:
            R = torch.eye(a.shape[-1], dtype=a.dtype).expand_as(a).clone()
        R = R + a @ R
    return R


def relevance(sd, batch, H: int, target=None, eps: float = 1e-12, dtype=torch.float64):
    """-> {"stlt", "target", "seed", "spatial_layers" (n_sp,B,T,N,N), "temporal_layers" (n_tp,B,T,T), "spatial_rollout" (B,T,N,N),
    "temporal_rollout" (B,T,T), "relevance" (B,T,N)} in `dtype`, straight from the formulas above"""
    B, T, N = batch["categories"].shape
    logits, spatial, temporal = forward(sd, batch, H, eps, dtype)
    seed, classes = seed_of(logits, target)
    G = grad_probs(logits, seed, spatial + temporal)
    sp = [abar_of(P, g) for (P, _, _), g in zip(spatial, G[:len(spatial)])]
    tp = [abar_of(P, g) for (P, _, _), g in zip(temporal, G[len(spatial):])]
    eye = lambda S, L: torch.eye(L, dtype=dtype).expand(S, L, L).clone()  # noqa: E731
    R_sp = (rollout(sp) if sp else eye(B * T, N)).reshape(B, T, N, N)
    R_tp = rollout(tp) if tp else eye(B, T)
    rel = R_tp[torch.arange(B), batch["lengths"] - 1][:, :, None] * R_sp[:, :, 0, :]
    return {"stlt": logits.detach(), "target": classes, "seed": seed.detach(),
            "spatial_layers": (torch.stack(sp) if sp else torch.zeros(0, B * T, N, N, dtype=dtype)).reshape(-1, B, T, N, N).detach(),
            "temporal_layers": (torch.stack(tp) if tp else torch.zeros(0, B, T, T, dtype=dtype)).detach(),
            "spatial_rollout": R_sp.detach(), "temporal_rollout": R_tp.detach(), "relevance": rel.detach()}


def padded_entries(batch):
    """(B,T,N) bool: object slots that are padded or lie in a padded frame — where rel is exactly 0"""
    return batch["src_key_padding_mask_boxes"].bool() | batch["src_key_padding_mask_frames"].bool()[:, :, None]


def attn_grad_probs(qkv, dctx, kpm, causal: bool, H: int):
    """One layer alone (include/stlt_hip.h: stlt_attn_grad_probs): qkv (S,L,3d) packed [q;k;v], dctx (S,L,d), kpm (S,L) bool -> abar (S,L,L)
    with G_h = dctx_h @ V_h^T, the closed form of the gradient wrt P_h (tests/test_relevance_cpu.py holds it to autograd's)"""
    S, L, d3 = qkv.shape
    d = d3 // 3
    P = AR.attn_probs(qkv, kpm, causal, H, per_head=True)
    V = qkv[..., 2 * d:].reshape(S, L, H, d // H).transpose(1, 2)
    D = dctx.reshape(S, L, H, d // H).transpose(1, 2)
    return abar_of(P, D @ V.transpose(-1, -2))
