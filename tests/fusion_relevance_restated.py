"""Attention relevance of the fusion models restated in plain torch (fp64 by default): TEST INFRASTRUCTURE ONLY.

`forward_relevance` of CrossAttentionFusion / CrossAttentionCentralNetFusion / LateConcatenationFusion (include/stlt_hip.h:
stlt_attn_grad_probs_cross, stlt_attn_rollout_joint, stlt_relevance_combine_joint) is gradient-weighted attention rollout over two token sets
(Chefer, Gur, Wolf, ICCV 2021, the bi-modal rule without its row normalisation).  Written here straight from that header's formulas, in the
style of tests/relevance_restated.py: a differentiable forward of the three models (the oracles' LayerNorm / GELU / head functions,
tests/fusion_attention_restated.attn_probs_cross) in which every attention output is ctx_h = P_h @ V_h with P_h a graph node, the boxes AND
the appearance features leaves, so that G_h — the gradient wrt P_h as an independent variable — is what torch.autograd.grad gives; a head that
does not read a block gives None there, which is zeros.

    abar[s,i,j] = (1/H) sum_h max(P_h[s,i,j] * G_h[s,i,j], 0)                                   per attention block
    unimodal:   R_0 = I,  R_l = R_{l-1} + abar_l @ R_{l-1}                                      spatial, temporal, appearance
    joint (J = T + A; index t = frame t, T + a = appearance token a):
        R_0 = blockdiag(temporal_rollout, appearance_rollout); per fusion layer three steps R <- R + X @ R with
        X = [[0, l2a], [a2l, 0]],  X = blockdiag(f_layout, f_appearance[0]),  X = blockdiag(0, f_appearance[1])
    row[b] = w_l R[b, lengths[b]-1] + w_a R[b, T];  frame_relevance = row[:, :T];  appearance_relevance = row[:, T:]
    relevance[b,t,n] = frame_relevance[b,t] * spatial_rollout[b,t,0,n]
"""
import torch

import fusion_attention_restated as FR
import relevance_restated as R
from oracle import stlt_oracle as O

PREFIX = {"caf": "caf_backbone.", "cacnf": "backbone.", "lcf": ""}
HEADS = {"caf": ("caf",), "cacnf": ("stlt", "resnet3d", "caf", "ensemble"), "lcf": ("lcf",)}
WEIGHTS = {"stlt": (1.0, 0.0), "resnet3d": (0.0, 1.0)}  # every fused head: (1, 1)
LAYER_KEYS = ("spatial_layers", "temporal_layers", "appearance_layers", "layout_to_appearance_layers", "appearance_to_layout_layers",
              "fusion_layout_layers", "fusion_appearance_layers")
ROLLOUT_KEYS = ("spatial_rollout", "temporal_rollout", "appearance_rollout", "fusion_rollout")
OUTPUT_KEYS = ("relevance", "frame_relevance", "appearance_relevance") + ROLLOUT_KEYS


def _heads(x, H):
    S, L, d = x.shape
    return x.reshape(S, L, H, d // H).transpose(1, 2)


def _attend(q, k, v, kpm_k, causal, H, nodes):
    """ctx = P @ V per head with P a graph node; appends (P, V, ctx) to `nodes` -> (S, Lq, d)"""
    P = FR.attn_probs_cross(q, k, kpm_k, causal, H, per_head=True)
    V = _heads(v, H)
    ctx = P @ V
    nodes.append((P, V, ctx))
    return ctx.transpose(1, 2).reshape(q.shape)


def _layout(sd, pre, batch, H, eps, spatial, temporal):
    """StltBackbone.forward (models.py:57-81, 136-153) on tests/relevance_restated._layer -> (B,T,d)"""
    FE = pre + "frames_embeddings."
    LE = FE + "layout_embedding."
    B, T, N = batch["categories"].shape
    x = O.category_box_embeddings(sd, LE + "category_box_embeddings.", batch, eps)
    d = x.shape[-1]
    x = x.reshape(B * T, N, d)
    kpm_boxes = batch["src_key_padding_mask_boxes"].reshape(B * T, N)
    n = 0
    while f"{LE}transformer.layers.{n}.norm1.weight" in sd:
        x = R._layer(x, sd, f"{LE}transformer.layers.{n}.", kpm_boxes, False, H, spatial)
        n += 1
    f = x.reshape(B, T, N, d)[:, :, 0, :]
    P, Ft = sd[FE + "position_embeddings.weight"], sd[FE + "frame_type_embedding.weight"]
    g = O.layer_norm(f + P[:T][None] + Ft[batch["frame_types"]], sd[FE + "layer_norm.weight"], sd[FE + "layer_norm.bias"], eps)
    n = 0
    while f"{pre}transformer.layers.{n}.norm1.weight" in sd:
        g = R._layer(g, sd, f"{pre}transformer.layers.{n}.", batch["src_key_padding_mask_frames"], True, H, temporal)
        n += 1
    return g


def _appearance(sd, pre, feats, H, nodes):
    """TransformerResnet.forward_features from the feature map on (models.py:257-271): ReLU post-norm layers, eps 1e-5, no mask -> (B,A,d)"""
    B, Cc = feats.shape[0], feats.shape[1]
    x = feats.flatten(2).transpose(1, 2) @ sd[pre + "projector.weight"].reshape(-1, Cc).t() + sd[pre + "projector.bias"]
    x = torch.cat((sd[pre + "cls_token"].reshape(1, 1, -1).expand(B, -1, -1), x), dim=1) + sd[pre + "pos_embed"].reshape(1, -1, x.shape[-1])
    d = x.shape[2]
    n = 0
    while f"{pre}transformer.layers.{n}.norm1.weight" in sd:
        w = lambda k: sd[f"{pre}transformer.layers.{n}.{k}"]  # noqa: E731
        qkv = x @ w("self_attn.in_proj_weight").t() + w("self_attn.in_proj_bias")
        a = _attend(qkv[..., :d], qkv[..., d:2 * d], qkv[..., 2 * d:], None, False, H, nodes)
        x = O.layer_norm(x + a @ w("self_attn.out_proj.weight").t() + w("self_attn.out_proj.bias"), w("norm1.weight"), w("norm1.bias"), 1e-5)
        h = torch.relu(x @ w("linear1.weight").t() + w("linear1.bias"))
        x = O.layer_norm(x + h @ w("linear2.weight").t() + w("linear2.bias"), w("norm2.weight"), w("norm2.bias"), 1e-5)
        n += 1
    return x


def _block(sd, pre, x, ctx, H, eps, kpm_k, causal, nodes):
    """SelfAttentionLayer (ctx is x) / CrossAttentionLayer (models.py:345-382): LN(MHA(x, ctx, ctx) + x), queries from x, keys and values from ctx"""
    d = x.shape[-1]
    W, b = sd[pre + "attn.in_proj_weight"], sd[pre + "attn.in_proj_bias"]
    a = _attend(x @ W[:d].t() + b[:d], ctx @ W[d:2 * d].t() + b[d:2 * d], ctx @ W[2 * d:].t() + b[2 * d:], kpm_k, causal, H, nodes)
    return O.layer_norm(a @ sd[pre + "attn.out_proj.weight"].t() + sd[pre + "attn.out_proj.bias"] + x, sd[pre + "ln.weight"], sd[pre + "ln.bias"], eps)


def forward(model_name: str, sd, batch, H: int, eps: float = 1e-12, dtype=torch.float64):
    """-> (logits under the model's head names, nodes): nodes[kind] the (P, V, ctx) graph nodes of every attention block, kinds "spatial",
    "temporal", "appearance" (one per layer), "l2a", "a2l", "f_layout", "f_app0", "f_app1" (one per fusion layer)"""
    sd = {k: (v.to(dtype) if v.is_floating_point() else v) for k, v in sd.items()}
    batch = {k: (v.to(dtype) if v.is_floating_point() else v) for k, v in batch.items()}
    batch["boxes"] = batch["boxes"].clone().requires_grad_(True)  # leaves, so that every P below is a node of the graph
    feats = batch["appearance_features"].clone().requires_grad_(True)
    pre = PREFIX[model_name]
    B = batch["categories"].shape[0]
    nodes = {k: [] for k in ("spatial", "temporal", "appearance", "l2a", "a2l", "f_layout", "f_app0", "f_app1")}
    Lh = _layout(sd, pre + "layout_branch.", batch, H, eps, nodes["spatial"], nodes["temporal"])
    Ah = _appearance(sd, pre + "appearance_branch.", feats, H, nodes["appearance"])
    idx = torch.arange(B)
    lay_state, app_state = Lh[idx, batch["lengths"] - 1], Ah[:, 0]
    kpm = batch["src_key_padding_mask_frames"]
    n = 0
    while f"{pre}mm_fusion.{n}.cross_attn.ln.weight" in sd:  # CrossModalModule.forward, models.py:403-431
        m = f"{pre}mm_fusion.{n}."
        la = _block(sd, m + "cross_attn.", Lh, Ah, H, eps, None, False, nodes["l2a"])
        aa = _block(sd, m + "cross_attn.", Ah, Lh, H, eps, kpm, False, nodes["a2l"])
        la = _block(sd, m + "layout_attn.", la, la, H, eps, kpm, True, nodes["f_layout"])
        aa = _block(sd, m + "appearance_attn.", aa, aa, H, eps, None, False, nodes["f_app0"])
        f = O.gelu(la @ sd[m + "layout_ffn.linear1.weight"].t() + sd[m + "layout_ffn.linear1.bias"])
        f = f @ sd[m + "layout_ffn.linear2.weight"].t() + sd[m + "layout_ffn.linear2.bias"]
        Lh = O.layer_norm(f + la, sd[m + "layout_ffn.ln.weight"], sd[m + "layout_ffn.ln.bias"], eps)
        Ah = _block(sd, m + "appearance_ffn.", aa, aa, H, eps, None, False, nodes["f_app1"])  # a SelfAttentionLayer (models.py:401)
        n += 1
    fused = torch.cat((Lh[idx, batch["lengths"] - 1], Ah[:, 0]), dim=-1)
    if model_name == "cacnf":
        logits = {"stlt": O.head_forward(sd, lay_state, eps, prefix="layout_classifier."),
                  "resnet3d": O.head_forward(sd, app_state, eps, prefix="appearance_classifier."),
                  "caf": O.head_forward(sd, fused, eps, prefix="fusion_classifier.")}
        logits["ensemble"] = (logits["stlt"] + logits["resnet3d"] + logits["caf"]) / 3
    else:
        logits = {model_name: O.head_forward(sd, fused, eps, prefix="classifier.")}
    return logits, nodes


def grad_probs(logit, seed, nodes):
    """{kind: [G (S,H,Lq,Lk)]}: the gradient of sum(seed * logit) wrt every block's P as an independent variable; a block the head does not
    read (autograd gives None) has zeros"""
    flat = [(k, P) for k, ns in nodes.items() for P, _, _ in ns]
    gs = torch.autograd.grad((logit * seed).sum(), [P for _, P in flat], retain_graph=True, allow_unused=True)
    out = {k: [] for k in nodes}
    for (k, P), g in zip(flat, gs):
        out[k].append(torch.zeros_like(P) if g is None else g)
    return out


def attn_grad_probs_cross(q, k, v, dctx, kpm, causal: bool, H: int):
    """One block alone (include/stlt_hip.h: stlt_attn_grad_probs_cross): q, dctx (S,Lq,d), k, v (S,Lk,d), kpm (S,Lk) bool or None -> abar
    (S,Lq,Lk) with G_h = dctx_h @ V_h^T, the closed form of the gradient wrt P_h (tests/test_fusion_relevance_cpu.py holds it to autograd's)"""
    P = FR.attn_probs_cross(q, k, kpm, causal, H, per_head=True)
    return R.abar_of(P, _heads(dctx, H) @ _heads(v, H).transpose(-1, -2))


def blockdiag(a, b):
    """(S,T,T), (S,A,A) -> (S,T+A,T+A)"""
    S, T, A = a.shape[0], a.shape[1], b.shape[1]
    out = torch.zeros(S, T + A, T + A, dtype=a.dtype)
    out[:, :T, :T], out[:, T:, T:] = a, b
    return out


def joint_rollout_dense(r_layout, r_appearance, l2a, a2l, f_layout, f_appearance):
    """the joint chain as dense J x J products: r_layout (S,T,T), r_appearance (S,A,A), l2a (n,S,T,A), a2l (n,S,A,T), f_layout (n,S,T,T),
    f_appearance (n,2,S,A,A) -> R (S,J,J)"""
    T = r_layout.shape[1]
    Rj = blockdiag(r_layout, r_appearance)
    for l in range(l2a.shape[0]):
        X = torch.zeros_like(Rj)
        X[:, :T, T:], X[:, T:, :T] = l2a[l], a2l[l]
        Rj = Rj + X @ Rj
        Rj = Rj + blockdiag(f_layout[l], f_appearance[l, 0]) @ Rj
        Rj = Rj + blockdiag(torch.zeros_like(f_layout[l]), f_appearance[l, 1]) @ Rj
    return Rj


def joint_rollout_quadrants(r_layout, r_appearance, l2a, a2l, f_layout, f_appearance):
    """the same chain reading only the non-zero quadrants, as the kernel does: the top T rows and the bottom A rows of R separately"""
    T = r_layout.shape[1]
    Rj = blockdiag(r_layout, r_appearance)
    top, bot = Rj[:, :T].clone(), Rj[:, T:].clone()
    for l in range(l2a.shape[0]):
        top, bot = top + l2a[l] @ bot, bot + a2l[l] @ top
        top, bot = top + f_layout[l] @ top, bot + f_appearance[l, 0] @ bot
        bot = bot + f_appearance[l, 1] @ bot
    return torch.cat((top, bot), dim=1)


def read_out(Rj, r_spatial, lengths, T: int, w_layout: float, w_appearance: float):
    """-> (relevance (B,T,N), frame_relevance (B,T), appearance_relevance (B,A)); r_spatial (B,T,N,N)"""
    B = Rj.shape[0]
    row = w_layout * Rj[torch.arange(B), lengths - 1] + w_appearance * Rj[:, T]
    return row[:, :T, None] * r_spatial[:, :, 0, :], row[:, :T], row[:, T:]


def relevance(model_name: str, sd, batch, H: int, head=None, target=None, eps: float = 1e-12, dtype=torch.float64):
    """-> the logits under their names (detached), "target", "seed", OUTPUT_KEYS and LAYER_KEYS in `dtype`, straight from the formulas above.
    `head` one of HEADS[model_name], default the last; `target` None (top-1), int64 classes or a float (B,K) seed."""
    B, T, N = batch["categories"].shape
    logits, nodes = forward(model_name, sd, batch, H, eps, dtype)
    head = HEADS[model_name][-1] if head is None else head
    seed, classes = R.seed_of(logits[head], target)
    G = grad_probs(logits[head], seed, nodes)
    abar = {k: [R.abar_of(P, g) for (P, _, _), g in zip(nodes[k], G[k])] for k in nodes}
    A = nodes["appearance"][0][0].shape[-1] if nodes["appearance"] else batch["appearance_features"][0, 0].numel() + 1
    stack = lambda xs, *shape: torch.stack(xs) if xs else torch.zeros(0, *shape, dtype=dtype)  # noqa: E731
    eye = lambda S, L: torch.eye(L, dtype=dtype).expand(S, L, L).clone()  # noqa: E731
    layers = {"spatial_layers": stack(abar["spatial"], B * T, N, N).reshape(-1, B, T, N, N), "temporal_layers": stack(abar["temporal"], B, T, T),
              "appearance_layers": stack(abar["appearance"], B, A, A), "layout_to_appearance_layers": stack(abar["l2a"], B, T, A),
              "appearance_to_layout_layers": stack(abar["a2l"], B, A, T), "fusion_layout_layers": stack(abar["f_layout"], B, T, T),
              "fusion_appearance_layers": stack([torch.stack(p) for p in zip(abar["f_app0"], abar["f_app1"])], 2, B, A, A)}
    R_sp = (R.rollout(abar["spatial"]) if abar["spatial"] else eye(B * T, N)).reshape(B, T, N, N)
    R_tp = R.rollout(abar["temporal"]) if abar["temporal"] else eye(B, T)
    R_app = R.rollout(abar["appearance"]) if abar["appearance"] else eye(B, A)
    Rj = joint_rollout_dense(R_tp, R_app, layers["layout_to_appearance_layers"], layers["appearance_to_layout_layers"], layers["fusion_layout_layers"],
                             layers["fusion_appearance_layers"])
    rel, frame_rel, app_rel = read_out(Rj, R_sp, batch["lengths"], T, *WEIGHTS.get(head, (1.0, 1.0)))
    out = {k: v.detach() for k, v in logits.items()}
    out.update(target=classes, seed=seed.detach(), relevance=rel, frame_relevance=frame_rel, appearance_relevance=app_rel, fusion_rollout=Rj,
               spatial_rollout=R_sp, temporal_rollout=R_tp, appearance_rollout=R_app, **layers)
    return {k: (v.detach() if isinstance(v, torch.Tensor) else v) for k, v in out.items()}


def padded_joint_columns(batch, A: int):
    """(B, T+A) bool: the joint tokens that are padded layout frames"""
    pad = batch["src_key_padding_mask_frames"].bool()
    return torch.cat((pad, torch.zeros(pad.shape[0], A, dtype=torch.bool)), dim=1)
