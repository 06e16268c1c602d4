"""Integrated gradients restated from the words of include/stlt_hip.h (stlt_ig_path, stlt_ig_path_dense, stlt_ig_reduce, stlt_ig_delta,
stlt_cell_pool_sum / _abs): the path, the weights and the accumulation in NumPy float32 — every operation separately rounded, so the bits
are the kernels' —, the delta and the pools in float64, and an integrated-gradients loop over the autograd of oracle.stlt_oracle /
oracle.caf_oracle in any dtype.  No package import, no GPU.  The reference project has no integrated gradients: this is the method of
Sundararajan, Taly and Yan (2017) on the trapezoid rule."""
import numpy as np
import torch

F32 = np.float32
LAYOUT_COPIED = ("categories", "src_key_padding_mask_boxes", "frame_types", "src_key_padding_mask_frames", "lengths")


def alpha(s, steps):
    return F32(s) / F32(steps)


def weight(s, steps):
    return F32(1) / F32(2 * steps) if s in (0, steps) else F32(1) / F32(steps)


def point(x, x0, s, steps):
    """step s of the path in float32: x0's bits at s = 0, x's bits at s = steps, fadd(x0, fmul(alpha, fsub(x, x0))) between"""
    x, x0 = np.asarray(x, dtype=F32), np.asarray(x0, dtype=F32)
    if s == 0:
        return np.broadcast_to(x0, x.shape).copy()
    if s == steps:
        return x.copy()
    d = (x - x0).astype(F32)
    return (x0 + (alpha(s, steps) * d).astype(F32)).astype(F32)


def path_dense(x, x0, steps, s0, s1):
    """x (B, ...) float32, x0 the same shape or a scalar fill -> ((s1-s0+1)*B, ...) step-major"""
    x = np.asarray(x, dtype=F32)
    x0 = np.broadcast_to(np.asarray(x0, dtype=F32), x.shape)
    return np.concatenate([point(x, x0, s, steps) for s in range(s0, s1 + 1)], axis=0)


def path_layout(batch, steps, s0, s1, boxes0=None, scores0=None):
    """batch: numpy arrays under the collated keys (scores optional) -> the same keys for (s1-s0+1)*B clips, step-major"""
    n = s1 - s0 + 1
    out = {k: np.concatenate([np.asarray(batch[k])] * n, axis=0) for k in LAYOUT_COPIED}
    out["boxes"] = path_dense(batch["boxes"], 0.0 if boxes0 is None else boxes0, steps, s0, s1)
    if "scores" in batch:
        out["scores"] = path_dense(batch["scores"], 0.0 if scores0 is None else scores0, steps, s0, s1)
    return out


def reduce(g, steps, s0, s1, acc=None):
    """g ((s1-s0+1)*B, ...) float32 step-major -> acc (B, ...) continued (None: from +0), ascending s, fadd(acc, fmul(w_s, g_s))"""
    g = np.asarray(g, dtype=F32)
    n = s1 - s0 + 1
    g = g.reshape((n, g.shape[0] // n) + g.shape[1:])
    acc = np.zeros(g.shape[1:], dtype=F32) if acc is None else np.asarray(acc, dtype=F32).copy()
    for i, s in enumerate(range(s0, s1 + 1)):
        acc = (acc + (weight(s, steps) * g[i]).astype(F32)).astype(F32)
    return acc


def finish(acc, x, x0):
    """attr = fmul(fsub(x, x0), acc); x0 the same shape or a scalar fill"""
    x = np.asarray(x, dtype=F32)
    d = (x - np.broadcast_to(np.asarray(x0, dtype=F32), x.shape)).astype(F32)
    return (d * np.asarray(acc, dtype=F32)).astype(F32)


def grouped(attr, group, extra=None):
    """the sum of each run of `group` consecutive attributions, left to right, then extra: (B, n/group) float32"""
    a = np.asarray(attr, dtype=F32)
    a = a.reshape(a.shape[0], -1, group)
    s = a[:, :, 0].copy()
    for c in range(1, group):
        s = (s + a[:, :, c]).astype(F32)
    if extra is not None:
        s = (s + np.asarray(extra, dtype=F32).reshape(s.shape)).astype(F32)
    return s


def delta(attrs, seed, logits_x, logits_x0):
    """float64: per clip, the sum of the float32 attributions minus seed . (logits_x - logits_x0); also the sum of |attr| and the number of
    attribution addends per clip (the terms of stlt_ig_delta's bound)"""
    B = np.asarray(seed).shape[0]
    flat = [np.asarray(a, dtype=np.float64).reshape(B, -1) for a in attrs]
    total = sum(f.sum(axis=1) for f in flat)
    gap = (np.asarray(seed, dtype=np.float64) * (np.asarray(logits_x, dtype=np.float64) - np.asarray(logits_x0, dtype=np.float64))).sum(axis=1)
    return total - gap, sum(np.abs(f).sum(axis=1) for f in flat), sum(f.shape[1] for f in flat)


def _cells(shape, cell):
    _, _, T, H, W = shape
    ct, ch, cw = cell
    for t0 in range(0, T, ct):
        for h0 in range(0, H, ch):
            for w0 in range(0, W, cw):
                yield slice(t0, min(t0 + ct, T)), slice(h0, min(h0 + ch, H)), slice(w0, min(w0 + cw, W))


def cell_pool(g, cell, absolute=False):
    """float64 pool: (B,C), the sum of g (or |g|) over every cell and all channels, cells in (gt, gh, gw) order"""
    g = np.asarray(g, dtype=np.float64)
    g = np.abs(g) if absolute else g
    return np.stack([g[:, :, t, h, w].reshape(g.shape[0], -1).sum(axis=1) for t, h, w in _cells(g.shape, cell)], axis=1)


def cell_pool_abs_bits(g, cell):
    """stlt_cell_pool_abs as it stood before it had a signed twin, bit for bit in float32: element e of a cell (channel-major, then frame,
    row, column) goes to accumulator (e // 256) % 4 of thread e % 256; (a0 + a1) + (a2 + a3); the wave's butterfly over lane ^ 32, 16, 8,
    4, 2, 1; the four waves as (w0 + w1) + (w2 + w3)."""
    g = np.abs(np.asarray(g, dtype=F32))
    B = g.shape[0]
    lanes = np.arange(256)
    cols = []
    for t, h, w in _cells(g.shape, cell):
        v = g[:, :, t, h, w].reshape(B, -1)
        rounds = -(-v.shape[1] // 256)
        v = np.concatenate([v, np.zeros((B, rounds * 256 - v.shape[1]), dtype=F32)], axis=1).reshape(B, rounds, 256)
        acc = np.zeros((B, 4, 256), dtype=F32)
        for r in range(rounds):
            acc[:, r % 4] = (acc[:, r % 4] + v[:, r]).astype(F32)
        s = ((acc[:, 0] + acc[:, 1]).astype(F32) + (acc[:, 2] + acc[:, 3]).astype(F32)).astype(F32)
        for o in (32, 16, 8, 4, 2, 1):
            s = (s + s[:, (lanes & ~63) | ((lanes & 63) ^ o)]).astype(F32)
        wv = s[:, ::64]
        cols.append(((wv[:, 0] + wv[:, 1]).astype(F32) + (wv[:, 2] + wv[:, 3]).astype(F32)).astype(F32))
    return np.stack(cols, axis=1)


# ---- integrated gradients over an autograd oracle ----------------------------------------------------------------------------------
def oracle_ig(forward, batch, moved, seed, steps, baseline=None, dtype=torch.float64):
    """`forward(batch) -> (n, K) logits` (an oracle in `dtype`, differentiable in the entries of `batch`), `moved` the keys the path moves,
    `seed` (B,K), baseline {key: tensor} (missing: zeros).  All S = steps + 1 points run as one step-major batch of S*B clips.
    -> {"attr": {key: (B, ...)}, "logits_x", "logits_x0", "delta" (B,), "grad_max": {key: max_s max |g_s|}, "diff_max": {key: max |x - x0|}}"""
    S = steps + 1
    B = seed.shape[0]
    x = {k: batch[k].to(dtype) for k in moved}
    x0 = {k: (baseline[k].to(dtype) if baseline and k in baseline else torch.zeros_like(x[k])) for k in moved}
    tile = lambda v: v.repeat((S,) + (1,) * (v.dim() - 1))  # noqa: E731
    cast = lambda v: v.to(dtype) if v.is_floating_point() else v  # noqa: E731
    big = {k: (cast(tile(v)) if isinstance(v, torch.Tensor) and v.dim() >= 1 and v.shape[0] == B else v) for k, v in batch.items()}
    leaves = {}
    for k in moved:
        pts = [x0[k] if s == 0 else (x[k] if s == steps else x0[k] + (s / steps) * (x[k] - x0[k])) for s in range(S)]
        leaves[k] = torch.cat(pts, dim=0).detach().requires_grad_(True)
    logits = forward(dict(big, **leaves))
    grads = torch.autograd.grad(logits, [leaves[k] for k in moved], grad_outputs=tile(seed.to(logits.dtype)))
    w = torch.tensor([1.0 / (2 * steps) if s in (0, steps) else 1.0 / steps for s in range(S)], dtype=dtype)
    out = {"attr": {}, "grad_max": {}, "diff_max": {}}
    for k, g in zip(moved, grads):
        g = g.reshape((S, B) + tuple(x[k].shape[1:]))
        acc = (w.reshape((S,) + (1,) * (g.dim() - 1)) * g).sum(dim=0)
        out["attr"][k] = ((x[k] - x0[k]) * acc).detach()
        out["grad_max"][k] = g.abs().max().item()
        out["diff_max"][k] = (x[k] - x0[k]).abs().max().item()
    lg = logits.detach().reshape(S, B, -1)
    out["logits_x"], out["logits_x0"] = lg[steps], lg[0]
    total = sum(a.reshape(B, -1).sum(dim=1) for a in out["attr"].values())
    out["delta"] = total - (seed.to(lg.dtype) * (lg[steps] - lg[0])).sum(dim=1)
    return out


def stlt_ig(sd, batch, heads, seed, steps, baseline=None, dtype=torch.float64):
    """integrated gradients of oracle.stlt_oracle.stlt_forward with respect to boxes (and scores, when the batch has them)"""
    from oracle import stlt_oracle as O
    sd = {k: (v.to(dtype) if v.is_floating_point() else v) for k, v in sd.items()}
    moved = ["boxes"] + (["scores"] if "scores" in batch else [])
    return oracle_ig(lambda b: O.stlt_forward(sd, b, heads, dtype=dtype)["stlt"], batch, moved, seed, steps, baseline, dtype)


def caf_ig(sd, batch, heads, seed, steps, moved=("boxes", "appearance_features"), baseline=None, dtype=torch.float64):
    """integrated gradients of oracle.caf_oracle.caf_forward with respect to `moved`"""
    from oracle import caf_oracle as CO
    sd = {k: (v.to(dtype) if v.is_floating_point() else v) for k, v in sd.items()}
    return oracle_ig(lambda b: CO.caf_forward(sd, b, heads, dtype=dtype)["caf"], batch, list(moved), seed, steps, baseline, dtype)
