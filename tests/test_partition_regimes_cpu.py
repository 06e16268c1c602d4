"""The hand-written fp64 references of tests/partition_refs.py against torch autograd through the oracle's embeddings
(oracle/stlt_oracle.py: category_box_embeddings, and backbone_forward with no encoder layer = the frames embedding on the CLS rows).
The gradient wrt a pre-LayerNorm sum is read off a bias that is handed to the oracle at the sum's full shape."""
import pytest
import torch

import partition_refs as R
from oracle import stlt_oracle as O


def _rand(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return ((torch.rand(*shape, generator=g) * 2 - 1) * scale).double()


def _embed_sd(prefix, C, d, seed):
    return {prefix + "category_embeddings.weight": _rand(C, d, seed=seed), prefix + "box_embedding.weight": _rand(d, 4, seed=seed + 1, scale=0.5),
            prefix + "box_embedding.bias": _rand(d, seed=seed + 2, scale=0.5), prefix + "score_embeddings.weight": _rand(d, 1, seed=seed + 3),
            prefix + "score_embeddings.bias": _rand(d, seed=seed + 4, scale=0.5), prefix + "layer_norm.weight": 1 + _rand(d, seed=seed + 5, scale=0.1),
            prefix + "layer_norm.bias": _rand(d, seed=seed + 6, scale=0.1)}


@pytest.mark.parametrize("B,T,N,d,C,with_scores", [(2, 3, 4, 8, 5, True), (3, 2, 5, 12, 7, False)])
def test_embedding_gradient_reference_matches_autograd_through_the_oracle(B, T, N, d, C, with_scores):
    g0 = torch.Generator().manual_seed(B * 100 + N)
    cats = torch.randint(0, C - 1, (B, T, N), generator=g0)  # row C - 1 is named by no token; row 0 is the padding index
    cats[0, 0, 0], cats[0, 0, 1] = 0, 1
    batch = {"categories": cats, "boxes": torch.rand(B, T, N, 4, generator=g0)}
    if with_scores:
        batch["scores"] = torch.rand(B, T, N, generator=g0)
    sd = _embed_sd("", C, d, seed=3)
    sd["box_embedding.bias"] = sd["box_embedding.bias"].expand(B, T, N, d).clone()  # one bias per element of the sum: its gradient IS d_pre
    leaves = {k: v.requires_grad_(True) for k, v in sd.items()}
    O.category_box_embeddings(leaves, "", batch, 1e-12).backward(_rand(B, T, N, d, seed=9))
    d_pre = leaves["box_embedding.bias"].grad
    ref, mag = R.embed_param_grads(d_pre.reshape(-1, d), cats, batch["boxes"], batch.get("scores"), C)
    auto = {"g_cat": leaves["category_embeddings.weight"].grad.clone(), "g_box_w": leaves["box_embedding.weight"].grad, "g_box_b": d_pre.sum((0, 1, 2))}
    assert auto["g_cat"][0].abs().max().item() > 0  # plain indexing gives the padding row a gradient; nn.Embedding(padding_idx=0) does not
    auto["g_cat"][0] = 0.0
    if with_scores:
        auto["g_score_w"], auto["g_score_b"] = leaves["score_embeddings.weight"].grad, leaves["score_embeddings.bias"].grad
    assert set(ref) == set(auto)
    for k in ref:
        assert ref[k].shape == auto[k].shape, k
        assert (ref[k] - auto[k]).abs().max().item() <= 1e-12 * max(1.0, auto[k].abs().max().item()), k
        assert bool((mag[k] >= ref[k].abs() - 1e-12).all()), k
    assert ref["g_cat"][0].abs().max().item() == 0.0 and ref["g_cat"][C - 1].abs().max().item() == 0.0
    assert ref["g_cat"][1].abs().max().item() > 0


@pytest.mark.parametrize("B,T,N,d", [(2, 5, 3, 8), (4, 3, 2, 12)])
def test_frames_embedding_gradient_reference_matches_autograd_through_the_oracle(B, T, N, d):
    g0 = torch.Generator().manual_seed(B * 10 + T)
    C = 4
    ft = torch.randint(0, 5, (B, T), generator=g0)
    ft[0, :] = 0       # one clip entirely of the padding type
    ft[1, :3] = torch.tensor([1, 2, 4])
    batch = {"categories": torch.randint(0, C, (B, T, N), generator=g0), "boxes": torch.rand(B, T, N, 4, generator=g0),
             "src_key_padding_mask_boxes": torch.zeros(B, T, N, dtype=torch.bool), "frame_types": ft,
             "src_key_padding_mask_frames": torch.zeros(B, T, dtype=torch.bool)}
    FE = "frames_embeddings."
    LE = FE + "layout_embedding.category_box_embeddings."
    sd = _embed_sd(LE, C, d, seed=5)
    for k in (LE + "score_embeddings.weight", LE + "score_embeddings.bias"):
        del sd[k]
    sd[LE + "layer_norm.bias"] = sd[LE + "layer_norm.bias"].expand(B, T, N, d).clone()  # gradient = that of the embedding's output; its CLS rows feed the frames sum
    sd.update({FE + "position_embeddings.weight": _rand(T + 2, d, seed=20), FE + "frame_type_embedding.weight": _rand(5, d, seed=21),
               FE + "layer_norm.weight": 1 + _rand(d, seed=22, scale=0.1), FE + "layer_norm.bias": _rand(d, seed=23, scale=0.1)})
    leaves = {k: v.requires_grad_(True) for k, v in sd.items()}
    out = O.backbone_forward(leaves, batch, num_heads=1, dtype=torch.float64)  # no encoder layer in sd: embeddings -> CLS rows -> frames embedding
    assert out.shape == (B, T, d)
    out.backward(_rand(B, T, d, seed=24))
    d_pre = leaves[LE + "layer_norm.bias"].grad[:, :, 0, :]
    assert leaves[LE + "layer_norm.bias"].grad[:, :, 1:, :].abs().max().item() == 0.0
    ref, mag = R.frames_param_grads(d_pre, ft)
    g_pos = leaves[FE + "position_embeddings.weight"].grad
    g_type = leaves[FE + "frame_type_embedding.weight"].grad.clone()
    assert g_pos[T:].abs().max().item() == 0.0 and g_type[0].abs().max().item() > 0
    g_type[0] = 0.0  # the padding type
    for got, want, name in ((ref["g_pos"], g_pos[:T], "g_pos"), (ref["g_type"], g_type, "g_type")):
        assert got.shape == want.shape, name
        assert (got - want).abs().max().item() <= 1e-12 * max(1.0, want.abs().max().item()), name
        assert bool((mag[name] >= got.abs() - 1e-12).all()), name
    assert ref["g_type"][0].abs().max().item() == 0.0 and ref["g_type"][1].abs().max().item() > 0
