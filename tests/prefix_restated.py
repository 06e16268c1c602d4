"""The per-prefix forward restated in plain torch (fp64 by default): TEST INFRASTRUCTURE ONLY.

`Stlt.forward_prefixes` (include/stlt_hip.h: stlt_forward_prefixes) returns the model's logits after every number of observed frames.
Its definition is `oracle.stlt_oracle.stlt_forward` on `collate.prefix_batch(batch, t)`; what the library computes is the two-stream
form below, written from that header's words with the oracle's own functions: the frame stream is the ordinary causal temporal tower,
the probe stream holds one row per (clip, t) — the clip's extract frame embedded at position t — which in every temporal layer attends
to the frame stream's keys j < t (not key-padded) and to its own key, and never to another probe.  tests/test_prefix_cpu.py holds this
restatement to the definition; the GPU tests hold the library to the restatement.
"""
import math

import torch

from oracle import stlt_oracle as O


def probe_attention(qkv_f: torch.Tensor, qkv_p: torch.Tensor, kpm: torch.Tensor, H: int) -> torch.Tensor:
    """qkv_f, qkv_p (S,T,3d) packed [q;k;v] rows of the two streams, kpm (S,T) bool (True = frame masked as a key). -> ctx (S,T,d):
    one softmax over the scores of the frame keys strictly below the diagonal and the probe's own key."""
    S, T, d3 = qkv_p.shape
    d = d3 // 3
    dh = d // H
    sp = lambda z: z.reshape(S, T, H, dh).transpose(1, 2)  # noqa: E731
    _, kf, vf = [sp(z) for z in qkv_f.split(d, -1)]
    qp, kp, vp = [sp(z) for z in qkv_p.split(d, -1)]
    sc = 1.0 / math.sqrt(dh)
    seen = torch.tril(torch.ones(T, T, dtype=torch.bool), diagonal=-1)[None] & ~kpm.bool()[:, None, :]  # (S, probe t, frame j)
    s = ((qp @ kf.transpose(-1, -2)) * sc).masked_fill(~seen[:, None], float("-inf"))
    s_self = (qp * kp).sum(-1, keepdim=True) * sc
    pr = torch.softmax(torch.cat([s, s_self], -1), -1)
    a = pr[..., :T] @ vf + pr[..., T:] * vp
    return a.transpose(1, 2).reshape(S, T, d)


def forward_prefixes(sd, batch, H: int, eps: float = 1e-12, dtype=torch.float64):
    """-> (logits (B,T,K), valid (B,T)): the two-stream computation, every layer of the frame stream run in full (the library skips what
    the last layer's frame rows would only compute for themselves); invalid entries are zero."""
    sd = {k: (v.to(dtype) if v.is_floating_point() else v) for k, v in sd.items()}
    pre = "backbone."
    FE = pre + "frames_embeddings."
    LE = FE + "layout_embedding."
    B, T, N = batch["categories"].shape
    x = O.category_box_embeddings(sd, LE + "category_box_embeddings.", batch, eps)
    d = x.shape[-1]
    x = x.reshape(B * T, N, d)
    kpm_boxes = batch["src_key_padding_mask_boxes"].reshape(B * T, N)
    m_sp = O._neg_inf_mask(kpm_boxes[:, None, :].expand(B * T, N, N), x.dtype)
    n = 0
    while f"{LE}transformer.layers.{n}.norm1.weight" in sd:
        x = O.encoder_layer(x, sd, f"{LE}transformer.layers.{n}.", m_sp, H)
        n += 1
    f = x.reshape(B, T, N, d)[:, :, 0, :]
    P, Ft = sd[FE + "position_embeddings.weight"], sd[FE + "frame_type_embedding.weight"]
    lnw, lnb = sd[FE + "layer_norm.weight"], sd[FE + "layer_norm.bias"]
    g = O.layer_norm(f + P[:T][None] + Ft[batch["frame_types"]], lnw, lnb, eps)  # frame stream (B,T,d)
    rows, ext = torch.arange(B), batch["lengths"] - 1
    f_e, ty_e = f[rows, ext], Ft[batch["frame_types"][rows, ext]]  # the clip's own extract frame: its spatial row and its frame type
    p = O.layer_norm(f_e[:, None] + P[:T][None] + ty_e[:, None], lnw, lnb, eps)  # probe stream (B,T,d): probe t sits at position t
    kpm = batch["src_key_padding_mask_frames"]
    causal = torch.triu(torch.ones(T, T, dtype=torch.bool), diagonal=1)
    m_tp = O._neg_inf_mask(causal[None] | kpm[:, None, :], g.dtype)
    n = 0
    while f"{pre}transformer.layers.{n}.norm1.weight" in sd:
        L = f"{pre}transformer.layers.{n}."
        w = lambda k: sd[L + k]  # noqa: E731
        qkv_f = g @ w("self_attn.in_proj_weight").t() + w("self_attn.in_proj_bias")
        qkv_p = p @ w("self_attn.in_proj_weight").t() + w("self_attn.in_proj_bias")
        a = probe_attention(qkv_f, qkv_p, kpm, H)
        p = O.layer_norm(p + a @ w("self_attn.out_proj.weight").t() + w("self_attn.out_proj.bias"), w("norm1.weight"), w("norm1.bias"), 1e-5)
        h = O.gelu(p @ w("linear1.weight").t() + w("linear1.bias"))
        p = O.layer_norm(p + h @ w("linear2.weight").t() + w("linear2.bias"), w("norm2.weight"), w("norm2.bias"), 1e-5)
        g = O.encoder_layer(g, sd, L, m_tp, H)
        n += 1
    logits = O.head_forward(sd, p, eps)
    valid = torch.arange(T)[None] < batch["lengths"][:, None]
    return logits * valid[..., None].to(logits.dtype), valid


def truncated_oracle(sd, batch, H: int, prefix_batch, dtype=torch.float64):
    """The definition, prefix by prefix: O.stlt_forward on prefix_batch(batch, t) for the clips that have that prefix.
    -> (logits (B,T,K) with zeros where invalid, valid (B,T))"""
    B, T = batch["categories"].shape[:2]
    valid = torch.arange(T)[None] < batch["lengths"][:, None]
    out = None
    for t in range(T):
        keep = valid[:, t]
        if not bool(keep.any()):
            continue
        tb = {k: (v[keep] if isinstance(v, torch.Tensor) and v.dim() >= 1 and v.shape[0] == B else v) for k, v in prefix_batch(batch, t).items()}
        ref = O.stlt_forward(sd, tb, H, dtype=dtype)["stlt"]
        if out is None:
            out = torch.zeros(B, T, ref.shape[-1], dtype=ref.dtype)
        out[keep, t] = ref
    return out, valid
