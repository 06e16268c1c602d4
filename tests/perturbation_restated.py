"""The perturbation test restated in NumPy from the words of include/stlt_hip.h (stlt_perturb_rank, stlt_perturb_apply, stlt_perturb_curve):
loops and a stable argsort, float64 arithmetic, no package import, no GPU.  tools/gen_golden_perturbation.py builds the fixtures with it,
tests/test_perturbation_cpu.py holds collate.perturb_batch's torch form to it and tests/test_perturbation_gpu.py the kernels."""
import numpy as np

UNITS = ("object", "frame")
ORDERS = ("descending", "ascending")


def candidates(kpm_boxes, lengths, unit):
    """(B,T,N) bool for unit object — slots (t,n) with t < lengths[b]-1, n >= 1, mask False — or (B,T) for unit frame: frames holding one."""
    kpm = np.asarray(kpm_boxes).astype(bool)
    B, T, N = kpm.shape
    cand = np.zeros((B, T, N), dtype=bool)
    for b in range(B):
        for t in range(min(max(int(lengths[b]) - 1, 0), T)):
            cand[b, t, 1:] = ~kpm[b, t, 1:]
    return cand if unit == "object" else cand.any(axis=2)


def rank(scores, kpm_boxes, lengths, unit="object", descending=True):
    """-> (rank int32 of scores' shape: position in the removal order for candidates, -1 elsewhere; n_candidates (B,) int32).  Order: by
    score as float32 values with -0 == +0, descending or ascending; ties to the lower flat index; NaN last in both orders."""
    cand = candidates(kpm_boxes, lengths, unit)
    scores = np.asarray(scores, dtype=np.float32)
    assert scores.shape == cand.shape, (scores.shape, cand.shape)
    B = cand.shape[0]
    out = np.full(cand.shape, -1, dtype=np.int32).reshape(B, -1)
    n_cand = np.zeros(B, dtype=np.int32)
    for b in range(B):
        idx = np.flatnonzero(cand[b].reshape(-1))
        v = scores[b].reshape(-1)[idx].astype(np.float64)
        nan = np.isnan(v)
        v = np.where(nan | (v == 0), 0.0, -v if descending else v)   # canonical: one zero; NaN is placed by the partition below
        order = np.argsort(v, kind="stable")
        order = order[np.argsort(nan[order], kind="stable")]
        out[b, idx[order]] = np.arange(len(idx), dtype=np.int32)
        n_cand[b] = len(idx)
    return out.reshape(cand.shape), n_cand


def removal_counts(n_candidates, steps):
    """(steps+1, B) int32: k = floor(s * n_candidates[b] / steps), in Python integers"""
    return np.array([[(s * int(n)) // steps for n in n_candidates] for s in range(steps + 1)], dtype=np.int32)


def apply(batch, rank_, n_candidates, steps, s0, s1, empty_frame_type):
    """batch: dict of NumPy arrays (categories, boxes, [scores], src_key_padding_mask_boxes, frame_types, src_key_padding_mask_frames,
    lengths).  -> the same keys for (s1-s0+1)*B clips, step-major, and "removed" (s1-s0+1, B) int32."""
    assert steps >= 1 and 0 <= s0 <= s1 <= steps
    cats = batch["categories"]
    B, T, N = cats.shape
    kpm = batch["src_key_padding_mask_boxes"].astype(bool)
    unit_frame = rank_.ndim == 2
    counts = removal_counts(n_candidates, steps)[s0:s1 + 1]
    n = s1 - s0 + 1
    out = {k: np.concatenate([batch[k]] * n, axis=0).copy() for k in batch if k in ("categories", "boxes", "scores", "src_key_padding_mask_boxes", "frame_types",
                                                                                    "src_key_padding_mask_frames", "lengths")}
    for i in range(n):
        for b in range(B):
            c, k = i * B + b, int(counts[i, b])
            real = ~kpm[b]                      # (T,N): the real object slots of every frame
            real[:, 0] = False
            r = np.broadcast_to(rank_[b][:, None], (T, N)) if unit_frame else rank_[b]
            gone = real & (r >= 0) & (r < k)
            out["categories"][c][gone] = 0
            out["boxes"][c][gone] = 0
            if "scores" in out:
                out["scores"][c][gone] = 0
            out["src_key_padding_mask_boxes"][c][gone] = True
            before_extract = np.arange(T) < int(batch["lengths"][b]) - 1
            out["frame_types"][c][before_extract & real.any(axis=1) & ~(real & ~gone).any(axis=1)] = empty_frame_type
    out["removed"] = counts
    return out


def curve(logits, target=None, activation="softmax"):
    """logits (S,B,K) -> (prob (S,B) float64, hit (S,B) bool, target (B,) int64).  target None: the arg-max of the step-0 row, first maximum."""
    x = np.asarray(logits, dtype=np.float64)
    S, B, K = x.shape
    if target is None:
        target = np.array([int(np.flatnonzero(x[0, b] == x[0, b].max())[0]) for b in range(B)], dtype=np.int64)
    target = np.asarray(target, dtype=np.int64)
    prob = np.zeros((S, B))
    hit = np.zeros((S, B), dtype=bool)
    for s in range(S):
        for b in range(B):
            y = int(target[b])
            if not 0 <= y < K:
                continue
            row = x[s, b]
            if activation == "sigmoid":
                with np.errstate(over="ignore"):
                    prob[s, b] = 1.0 / (1.0 + np.exp(-row[y]))
                hit[s, b] = row[y] > 0
            else:
                e = np.exp(row - row.max())
                prob[s, b] = e[y] / e.sum()
                hit[s, b] = not any(row[j] > row[y] or (row[j] == row[y] and j < y) for j in range(K))
    return prob, hit, target


def margin(logits, target):
    """(S,B) float64: how far the target's logit is from the best other class — the distance to the decision `hit` makes"""
    x = np.asarray(logits, dtype=np.float64)
    S, B, K = x.shape
    out = np.full((S, B), np.inf)
    for b in range(B):
        y = int(target[b])
        if K > 1 and 0 <= y < K:
            out[:, b] = np.abs(x[:, b, y] - np.delete(x[:, b], y, axis=1).max(axis=1))
    return out
