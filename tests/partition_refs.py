"""Hand-written fp64 references of the embedding parameter gradients, shared by tests/test_partition_regimes_gpu.py (which holds the
kernels to them) and tests/test_partition_regimes_cpu.py (which holds THEM to torch autograd through the oracle's embeddings, so that
a wrong reference cannot make a GPU case vacuous).  Plain torch on the CPU, no package import."""
import torch


def embed_param_grads(d_pre, categories, boxes, scores, n_categories):
    """Parameter gradients of CategoryBoxEmbeddings from d_pre (n, d), the gradient wrt the pre-LayerNorm sum
    E[cat] + boxes·Wbᵀ + bb (+ score·Ws + bs).  Row 0 of the category table is the padding index: no gradient.
    -> {"g_cat" (C, d), "g_box_w" (d, 4), "g_box_b" (d,) [, "g_score_w" (d, 1), "g_score_b" (d,)]} in fp64, and the same dict of
    sum|terms| per element (what the a-priori bound of a k-term fp32 sum is made of)."""
    g = d_pre.double()
    n, d = g.shape
    cats = categories.reshape(-1)
    bx = boxes.reshape(n, 4).double()
    ref = {"g_cat": torch.zeros(n_categories, d, dtype=torch.float64).index_add_(0, cats, g), "g_box_w": g.t() @ bx, "g_box_b": g.sum(0)}
    mag = {"g_cat": torch.zeros(n_categories, d, dtype=torch.float64).index_add_(0, cats, g.abs()), "g_box_w": g.abs().t() @ bx.abs(),
           "g_box_b": g.abs().sum(0)}
    ref["g_cat"][0] = 0.0
    mag["g_cat"][0] = 0.0
    if scores is not None:
        sc = scores.reshape(n).double()
        ref["g_score_w"], ref["g_score_b"] = (g * sc[:, None]).sum(0)[:, None], g.sum(0)
        mag["g_score_w"], mag["g_score_b"] = (g.abs() * sc.abs()[:, None]).sum(0)[:, None], g.abs().sum(0)
    return ref, mag


def frames_param_grads(d_pre, frame_types, n_types=5):
    """Parameter gradients of FramesEmbeddings from d_pre (B, T, d), the gradient wrt the pre-LayerNorm sum cls + P[t] + F[type]:
    g_pos[t] = sum over the clips, g_type[k] = sum over the frames of type k; type 0 is the padding index: no gradient.
    -> ({"g_pos" (T, d), "g_type" (n_types, d)}, the same of sum|terms|) in fp64."""
    g = d_pre.double()
    B, T, d = g.shape
    ft = frame_types.reshape(-1)
    ref = {"g_pos": g.sum(0), "g_type": torch.zeros(n_types, d, dtype=torch.float64).index_add_(0, ft, g.reshape(-1, d))}
    mag = {"g_pos": g.abs().sum(0), "g_type": torch.zeros(n_types, d, dtype=torch.float64).index_add_(0, ft, g.abs().reshape(-1, d))}
    ref["g_type"][0] = 0.0
    mag["g_type"][0] = 0.0
    return ref, mag
