"""Training step parity: the native forward/backward against torch autograd on the CPU oracle."""
import importlib
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import golden_case
from oracle import stlt_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _oracle_grads(sd, batch, H, labels, dtype=torch.float64):
    leaves = {k: (v.detach().to(dtype).requires_grad_(True) if v.is_floating_point() else v) for k, v in sd.items()}
    b = {k: (v.to(dtype) if v.is_floating_point() else v) for k, v in batch.items()}
    logits = O.stlt_forward(leaves, b, H, dtype=dtype)["stlt"]
    loss = F.cross_entropy(logits, labels)
    loss.backward()
    return loss.item(), logits.detach(), {k: v.grad for k, v in leaves.items() if v.is_floating_point()}


@pytest.mark.parametrize("skip_padding", [False, True])
@pytest.mark.parametrize("name,B,with_scores", [("cfg1", 3, False), ("cfg1", 5, True), ("cfg2", 2, False), ("cfg4", 2, True)])
def test_gradients_match_oracle_autograd(pkg, name, B, with_scores, skip_padding):
    _check_gradients(pkg, name, B, with_scores, skip_padding)


@pytest.mark.parametrize("T,N,B", [(20, 9, 3), (29, 16, 2), (32, 5, 3), (24, 3, 3), (17, 2, 4), (32, 7, 5)])
def test_gradients_match_oracle_autograd_other_layouts(pkg, T, N, B):
    """Frame / object counts around the block sizes of the MFMA attention backward (two 16-row blocks per item: one
    sequence of 17-32 frames, or floor(16/N) frames per block; last item partly filled), cfg1's widths."""
    _check_gradients(pkg, "cfg1", B, False, False, T=T, N=N)


@pytest.mark.parametrize("skip_padding", [False, True])
@pytest.mark.parametrize("B,T,N,min_len", [(3, 1, 3, 1), (3, 5, 1, 2), (4, 1, 1, 1)])
def test_gradients_match_oracle_autograd_without_tail_layers(pkg, B, T, N, min_len, skip_padding):
    """Layouts whose towers have no tail layer (csrc/train.hip: a tail needs twice as many rows as it picks): one frame per clip (no
    temporal tail: the clips' last rows are scattered), one object slot per frame (no spatial tail: the strided CLS scatter of the
    padded schedule, the CLS gather / scatter of skip-padding), and both.  cfg1's widths (head dim 64), scores given."""
    _check_gradients(pkg, "cfg1", B, True, skip_padding, T=T, N=N, min_len=min_len)


def _check_gradients(pkg, name, B, with_scores, skip_padding, T=None, N=None, min_len=None):
    c = dict(pkg.synth.CONFIGS[name])
    if T is not None:
        c["T"], c["N"] = T, N
    H = c["num_attention_heads"]
    m = pkg.Stlt(pkg.StltModelConfig(**pkg.synth.model_kwargs(name)))
    sd = pkg.synth.make_state_dict({k: tuple(v.shape) for k, v in m.state_dict().items()}, seed=31, gain=1.5)
    m.load_state_dict(sd)
    m.train(True)  # hidden_dropout_prob = 0 in model_kwargs
    m.to(DEV)
    m.backbone.skip_padding = skip_padding  # forward + reverse sweep on the real tokens / frames only
    batch = pkg.synth.make_batch(B, c["T"], c["N"], dataset=c["dataset"], seed=77, with_scores=with_scores, min_len=min_len)
    labels = torch.randint(0, c["num_classes"], (B,), generator=torch.Generator().manual_seed(5))
    ref_loss, ref_logits, ref_g = _oracle_grads(sd, batch, H, labels)

    out = m({k: v.to(DEV) for k, v in batch.items()})["stlt"]
    assert out.requires_grad
    assert (out.detach().cpu().double() - ref_logits).abs().max().item() <= 1e-4
    loss = F.cross_entropy(out, labels.to(DEV))
    assert abs(loss.item() - ref_loss) <= 1e-5
    loss.backward()

    worst = ("", 0.0)
    n_checked = 0
    for k, p in m.named_parameters():
        g_ref = ref_g[k]
        dead = "encoder_layer." in k or ("score_embeddings" in k and not with_scores)
        if dead:
            assert p.grad is None or p.grad.abs().max().item() == 0.0, k
            assert g_ref is None or g_ref.abs().max().item() == 0.0, k
            continue
        assert p.grad is not None, k
        scale = max(g_ref.abs().max().item(), 1e-6)
        err = (p.grad.cpu().double() - g_ref).abs().max().item() / scale
        n_checked += 1
        if err > worst[1]:
            worst = (k, err)
        assert err <= 2e-4, f"{k}: relative grad error {err:.2e} (|g|max={scale:.2e})"
    print(f"{name} B={B} skip_padding={skip_padding}: {n_checked} gradients checked, worst {worst[0]} rel err {worst[1]:.2e}")
    # padding_idx rows get no gradient (models.py:22,91)
    assert m.backbone.frames_embeddings.frame_type_embedding.weight.grad[0].abs().max().item() == 0.0
    assert m.backbone.frames_embeddings.layout_embedding.category_box_embeddings.category_embeddings.weight.grad[0].abs().max().item() == 0.0


@pytest.mark.parametrize("skip_padding", [False, True])
def test_training_pass_over_more_than_32768_tokens_agrees_with_its_two_halves(pkg, skip_padding):
    """Round 6: from 32 768 tokens the embedding runs 8 tokens per wave (rowwise.hip embed_rows_kernel), also when it writes the training
    tape's pre-LayerNorm rows and when it reads the ragged index.  cfg2's widths with one layer per tower, 148 clips x 224 tokens: the
    logits of the whole batch are those of its halves (each below the threshold) and the gradients are their mean."""
    c = pkg.synth.CONFIGS["cfg2"]
    B = 148
    assert B * c["T"] * c["N"] >= 32768 > (B // 2) * c["T"] * c["N"]
    m = pkg.Stlt(pkg.StltModelConfig(num_classes=c["num_classes"], unique_categories=4, hidden_size=c["hidden_size"],
                                     num_attention_heads=c["num_attention_heads"], num_spatial_layers=1, num_temporal_layers=1,
                                     hidden_dropout_prob=0.0))
    m.load_state_dict(pkg.synth.make_state_dict({k: tuple(v.shape) for k, v in m.state_dict().items()}, seed=31, gain=1.5))
    m.train(True)
    m.to(DEV)
    m.backbone.skip_padding = skip_padding
    batch = {k: v.to(DEV) for k, v in pkg.synth.make_batch(B, c["T"], c["N"], dataset=c["dataset"], seed=77, with_scores=True).items()}
    labels = torch.randint(0, c["num_classes"], (B,), generator=torch.Generator().manual_seed(5)).to(DEV)

    def run(lo, hi):
        m.zero_grad(set_to_none=True)
        out = m({k: v[lo:hi].contiguous() for k, v in batch.items()})["stlt"]
        F.cross_entropy(out, labels[lo:hi]).backward()
        return out.detach().clone(), {k: p.grad.clone() for k, p in m.named_parameters() if p.grad is not None}

    out, g = run(0, B)
    out_a, g_a = run(0, B // 2)
    out_b, g_b = run(B // 2, B)
    assert (out - torch.cat([out_a, out_b])).abs().max().item() <= 2e-5
    assert set(g) == set(g_a) == set(g_b)
    for k in g:
        mean = 0.5 * (g_a[k] + g_b[k])
        scale = max(mean.abs().max().item(), 1e-6)
        assert (g[k] - mean).abs().max().item() / scale <= 2e-4, k


def test_backward_is_bitwise_reproducible_and_accumulates(pkg):
    name = "cfg1"
    c = pkg.synth.CONFIGS[name]
    sd, batch, z, meta = golden_case(name)
    m = pkg.Stlt(pkg.StltModelConfig(**pkg.synth.model_kwargs(name)))
    m.load_state_dict(sd)
    m.train(True).to(DEV)
    b = {k: v.to(DEV) for k, v in batch.items()}
    labels = torch.arange(batch["categories"].shape[0], device=DEV) % c["num_classes"]
    grads = []
    for _ in range(2):
        m.zero_grad(set_to_none=True)
        F.cross_entropy(m(b)["stlt"], labels).backward()
        grads.append({k: p.grad.clone() for k, p in m.named_parameters() if p.grad is not None})
    assert all(torch.equal(grads[0][k], grads[1][k]) for k in grads[0])  # slab reductions, no float atomics
    F.cross_entropy(m(b)["stlt"], labels).backward()  # second backward without zero_grad: autograd accumulates
    k0 = "prediction_head.fc2.weight"
    assert (dict(m.named_parameters())[k0].grad - 2 * grads[0][k0]).abs().max().item() <= 1e-6 * grads[0][k0].abs().max().item() + 1e-9


def test_frozen_backbone_trains_head_only(pkg, tmp_path):
    kw = pkg.synth.model_kwargs("cfg1")
    c = pkg.synth.CONFIGS["cfg1"]
    bb = pkg.StltBackbone(pkg.StltModelConfig(**kw))
    path = str(tmp_path / "bb.pt")
    torch.save(bb.state_dict(), path)
    m = pkg.Stlt(pkg.StltModelConfig(**kw, load_backbone_path=path, freeze_backbone=True))
    m.train(True).to(DEV)
    batch = {k: v.to(DEV) for k, v in pkg.synth.make_batch(4, c["T"], c["N"], seed=3).items()}
    F.cross_entropy(m(batch)["stlt"], torch.tensor([1, 2, 3, 4], device=DEV)).backward()
    assert all(p.grad is None for p in m.backbone.parameters())
    assert all(p.grad is not None and p.grad.abs().max().item() > 0 for p in m.prediction_head.parameters())


def test_three_training_steps_match_reference_golden(pkg):
    """Reference train step (train.py:119-135 with parser defaults, warm-up 2 of 10 steps) captured by
    tools/gen_golden_train.py: loss, clip_grad_norm_ value and parameter slices after each step."""
    from conftest import GOLDEN
    import os
    z = np.load(os.path.join(GOLDEN, "train_cfg1.npz"))
    name = "cfg1"
    c = pkg.synth.CONFIGS[name]
    B = int(z["batch"][0])
    m = pkg.Stlt(pkg.StltModelConfig(**pkg.synth.model_kwargs(name)))
    sd = pkg.synth.make_state_dict({k: tuple(v.shape) for k, v in m.state_dict().items()}, seed=1234)
    m.load_state_dict(sd)
    m.to(DEV)
    tr = pkg.train.Trainer(m, "something", learning_rate=5e-5, weight_decay=1e-3, clip_val=5.0, warmup_steps=2, total_steps=10)
    watch = ["prediction_head.fc2.bias", "prediction_head.fc2.weight",
             "backbone.frames_embeddings.layout_embedding.category_box_embeddings.category_embeddings.weight",
             "backbone.frames_embeddings.layout_embedding.transformer.layers.0.self_attn.in_proj_weight",
             "backbone.transformer.layers.7.linear2.weight", "backbone.frames_embeddings.position_embeddings.weight",
             "backbone.transformer.layers.3.norm1.weight"]
    params = dict(m.named_parameters())
    for s in range(int(z["steps"][0])):
        batch = pkg.synth.make_batch(B, c["T"], c["N"], seed=500 + s)
        batch["labels"] = torch.randint(0, c["num_classes"], (B,), generator=torch.Generator().manual_seed(900 + s))
        out = tr.step({k: v.to(DEV) for k, v in batch.items()})
        assert abs(float(out["loss"]) - float(z[f"loss{s}"][0])) <= 2e-5, s
        assert abs(float(out["grad_norm"]) - float(z[f"gnorm{s}"][0])) <= 2e-4 * float(z[f"gnorm{s}"][0]), s
        for i, k in enumerate(watch):
            got = params[k].detach().reshape(-1)[:64].cpu().numpy()
            assert np.abs(got - z[f"p{s}_{i}"]).max() <= 2.5e-5, (s, k)  # < lr/2 (Adam amplifies last-bit gradient noise)
    # 14 dead / unused parameters get no gradient (the fused optimiser path keeps gradients in the flat buffer only)
    assert tr.fused and len(list(m.parameters())) - len(m._flat_layout) == int(z["n_grad_none"][0])


@pytest.mark.parametrize("name,B,p", [("cfg1", 3, 0.1), ("cfg1", 2, 0.5)])
def test_dropout_forward_and_gradients_match_masked_oracle(pkg, name, B, p):
    """hidden_dropout_prob > 0 in train mode: the six dropout sites of the reference (both embedding outputs, attention
    probabilities, dropout1, FFN dropout, dropout2) with the build's counter-based masks, against the oracle applying
    the same masks under torch autograd."""
    c = pkg.synth.CONFIGS[name]
    H = c["num_attention_heads"]
    kw = dict(pkg.synth.model_kwargs(name), hidden_dropout_prob=p)
    m = pkg.Stlt(pkg.StltModelConfig(**kw))
    sd = pkg.synth.make_state_dict({k: tuple(v.shape) for k, v in m.state_dict().items()}, seed=41, gain=1.5)
    m.load_state_dict(sd)
    m.train(True).to(DEV)
    seed = 123456789
    m._dropout_seed_override = seed
    batch = pkg.synth.make_batch(B, c["T"], c["N"], seed=9)
    labels = torch.randint(0, c["num_classes"], (B,), generator=torch.Generator().manual_seed(1))
    drop = O.Dropout(p, seed)
    leaves = {k: (v.detach().double().requires_grad_(True) if v.is_floating_point() else v) for k, v in sd.items()}
    b64 = {k: (v.double() if v.is_floating_point() else v) for k, v in batch.items()}
    ref_logits = O.stlt_forward(leaves, b64, H, dtype=torch.float64, drop=drop)["stlt"]
    F.cross_entropy(ref_logits, labels).backward()

    out = m({k: v.to(DEV) for k, v in batch.items()})["stlt"]
    # fp32 against the fp64 oracle under the same masks.  The rounding noise grows steeply with p (measured over three seeds, tools/scratch
    # runs of round 5: p = 0.1: 3 - 5e-6; 0.3: 2 - 3e-5; 0.5: 0.6 - 2.5e-4 — the same band with the FFN GELU in the product's epilogue
    # (branch-free erf fit) and as a separate pass (library erff)); the gradient check below and the small-vs-large-tile
    # comparison of test_ffn_block_backward_gelu_epilogue_on_small_tiles are what would catch a wrong mask index
    assert (out.detach().cpu().double() - ref_logits.detach()).abs().max().item() <= (2e-5 if p <= 0.1 else 4e-4)
    F.cross_entropy(out, labels.to(DEV)).backward()
    for k, prm in m.named_parameters():
        if "encoder_layer." in k or "score_embeddings" in k:
            continue
        g_ref = leaves[k].grad
        scale = max(g_ref.abs().max().item(), 1e-6)
        assert (prm.grad.cpu().double() - g_ref).abs().max().item() / scale <= 5e-4, k
    # dropout really is on: a different seed changes the logits, eval mode ignores it, and the rate is right
    m._dropout_seed_override = seed + 1
    with torch.enable_grad():
        other = m({k: v.to(DEV) for k, v in batch.items()})["stlt"]
    assert (other - out).abs().max().item() > 1e-3
    keep = O.dropout_keep(p, seed, 17, np.arange(200000, dtype=np.uint64))
    assert abs(1.0 - keep.mean() - p) < 0.01


def test_skip_padding_training_edge_layouts_and_alternation(pkg):
    """Ragged row counts change from step to step and the padded schedule can follow a ragged step on the same tape /
    scratch buffers: gradients must match the padded schedule's every time (stale rows past the row count must not leak)."""
    name = "cfg1"
    c = pkg.synth.CONFIGS[name]
    m = pkg.Stlt(pkg.StltModelConfig(**pkg.synth.model_kwargs(name)))
    m.load_state_dict(pkg.synth.make_state_dict({k: tuple(v.shape) for k, v in m.state_dict().items()}, seed=8, gain=1.5))
    m.train(True).to(DEV)
    B = 6
    batches = [pkg.synth.make_batch(B, c["T"], c["N"], seed=41, dense=True),          # nothing to skip
               pkg.synth.make_batch(B, c["T"], c["N"], seed=42, min_len=2),            # short clips
               pkg.synth.make_batch(B, c["T"], c["N"], seed=43),
               pkg.synth.make_batch(B, c["T"], c["N"], seed=44, min_len=2)]
    empty = pkg.synth.make_batch(B, c["T"], c["N"], seed=45)
    empty["categories"][:, :, 1:] = 0
    empty["boxes"][:, :, 1:] = 0
    empty["src_key_padding_mask_boxes"] = empty["categories"] == 0                       # CLS-only frames
    batches.append(empty)
    labels = torch.randint(0, c["num_classes"], (B,), generator=torch.Generator().manual_seed(5)).to(DEV)

    def grads(batch, skip):
        m.backbone.skip_padding = skip
        m.zero_grad(set_to_none=True)
        out = m({k: v.to(DEV) for k, v in batch.items()})["stlt"]
        F.cross_entropy(out, labels).backward()
        return out.detach().clone(), {k: p.grad.detach().clone() for k, p in m.named_parameters() if p.grad is not None}

    for batch in batches:
        ref_out, ref = grads(batch, False)
        out, got = grads(batch, True)
        assert (out - ref_out).abs().max().item() <= 2e-5
        assert set(got) == set(ref)
        for k in ref:
            scale = max(ref[k].abs().max().item(), 1e-6)
            assert (got[k] - ref[k]).abs().max().item() / scale <= 2e-4, k
        again_out, again = grads(batch, True)
        assert torch.equal(out, again_out) and all(torch.equal(got[k], again[k]) for k in got)  # reproducible


def test_skip_padding_training_with_the_batchs_row_counts_is_the_same_step(pkg):
    """Round 6: with num_real_tokens / num_real_frames in the batch (collate.real_counts) the skip-padding training step reads nothing back —
    forward and reverse sweep take the caller's counts — and is the step without them, bit for bit; wrong counts give a NaN loss."""
    name = "cfg1"
    c = pkg.synth.CONFIGS[name]
    runs = []
    for with_counts in (False, True):
        m = pkg.Stlt(pkg.StltModelConfig(**pkg.synth.model_kwargs(name)))
        m.load_state_dict(pkg.synth.make_state_dict({k: tuple(v.shape) for k, v in m.state_dict().items()}, seed=1234))
        m.to(DEV)
        m.backbone.skip_padding = True
        tr = pkg.train.Trainer(m, "something", learning_rate=1e-3, warmup_steps=0, total_steps=100)
        log = []
        for s in range(2):
            cpu = pkg.synth.make_batch(12, c["T"], c["N"], seed=40 + s)
            cpu["labels"] = torch.randint(0, c["num_classes"], (12,), generator=torch.Generator().manual_seed(s))
            b = {k: v.to(DEV) for k, v in cpu.items()}
            if with_counts:
                b.update(pkg.collate.real_counts(cpu))
            out = tr.step(b)
            log.append((float(out["loss"]), float(out["grad_norm"])))
        runs.append((log, [p.detach().clone() for p in m.parameters()]))
        if with_counts:
            bad = dict(b, num_real_tokens=b["num_real_tokens"] - 1)
            assert math.isnan(float(tr.step(bad)["loss"]))
    assert runs[0][0] == runs[1][0]
    assert all(torch.equal(a, b_) for a, b_ in zip(runs[0][1], runs[1][1]))


def test_skip_padding_training_with_dropout_is_seeded_and_finite(pkg):
    name = "cfg1"
    c = pkg.synth.CONFIGS[name]
    kw = pkg.synth.model_kwargs(name)
    kw["hidden_dropout_prob"] = 0.1
    m = pkg.Stlt(pkg.StltModelConfig(**kw))
    m.load_state_dict(pkg.synth.make_state_dict({k: tuple(v.shape) for k, v in m.state_dict().items()}, seed=8))
    m.train(True).to(DEV)
    m.backbone.skip_padding = True
    batch = {k: v.to(DEV) for k, v in pkg.synth.make_batch(4, c["T"], c["N"], seed=3).items()}
    labels = torch.randint(0, c["num_classes"], (4,), generator=torch.Generator().manual_seed(5)).to(DEV)

    def run(seed):
        torch.manual_seed(seed)
        m.zero_grad(set_to_none=True)
        out = m(batch)["stlt"]
        F.cross_entropy(out, labels).backward()
        g = m.backbone.transformer.layers[0].linear1.weight.grad.detach().clone()
        return out.detach().clone(), g

    a, ga = run(1)
    b, gb = run(1)
    c2, gc = run(2)
    assert torch.isfinite(a).all() and torch.isfinite(ga).all()
    assert torch.equal(a, b) and torch.equal(ga, gb)          # same seed -> same masks in forward and backward
    assert not torch.equal(a, c2)                             # another seed -> another mask
    m.train(False)
    with torch.no_grad():
        e = m(batch)["stlt"]
    assert (e - a).abs().max().item() > 1e-4                  # dropout really was applied in training mode


def test_fused_adamw_matches_torch_adamw_and_clip(pkg):
    """stlt_grad_norm + stlt_adamw_step against clip_grad_norm_ + torch.optim.AdamW on odd-sized tensors, 4 steps, two
    weight-decay groups, clipping active (large gradients) and inactive."""
    T = importlib.import_module("revisiting-spatial-temporal-layouts_amd.train")
    g0 = torch.Generator().manual_seed(0)
    shapes = [(174, 96), (174,), (33, 7), (50000,), (3,)]
    ref_p = [torch.nn.Parameter(torch.randn(*s, generator=g0).to(DEV)) for s in shapes]
    our_p = [torch.nn.Parameter(p.detach().clone()) for p in ref_p]
    groups = lambda ps: [{"params": [ps[1], ps[4]], "weight_decay": 0.0}, {"params": [ps[0], ps[2], ps[3]], "weight_decay": 1e-2}]
    ref = torch.optim.AdamW(groups(ref_p), lr=3e-3)
    ours = T.FusedAdamW(groups(our_p), lr=3e-3)
    layout, off = [], 0
    for p in our_p:
        layout.append((p, off, p.numel()))
        off += (p.numel() + 3) // 4 * 4
    for step in range(4):
        scale = 10.0 if step % 2 == 0 else 0.01  # norm above / below max_norm = 5
        grads = [torch.randn(*s, generator=g0).to(DEV) * scale for s in shapes]
        for p, g in zip(ref_p, grads):
            p.grad = g.clone()
        n_ref = torch.nn.utils.clip_grad_norm_(ref_p, 5.0)
        ref.step()
        flat = torch.zeros(off, device=DEV)
        for (p, o, n), g in zip(layout, grads):
            flat[o:o + n] = g.reshape(-1)
        n_got = ours.step_flat(flat, layout, 5.0)
        assert abs(n_got.item() - n_ref.item()) <= 1e-5 * n_ref.item()
        for a, b in zip(our_p, ref_p):
            assert (a - b).abs().max().item() <= 2e-6
    # the state has torch's layout: it loads into a stock AdamW
    stock = torch.optim.AdamW(groups([torch.nn.Parameter(p.detach().clone()) for p in our_p]), lr=3e-3)
    stock.load_state_dict(ours.state_dict())
    assert int(stock.state[stock.param_groups[0]["params"][0]]["step"]) == 4


def test_trainer_fused_and_stock_optimizer_agree(pkg):
    name = "cfg1"
    c = pkg.synth.CONFIGS[name]
    sd = None
    runs = []
    for fused in (True, False):
        m = pkg.Stlt(pkg.StltModelConfig(**pkg.synth.model_kwargs(name)))
        if sd is None:
            sd = pkg.synth.make_state_dict({k: tuple(v.shape) for k, v in m.state_dict().items()}, seed=8, gain=1.5)
        m.load_state_dict(sd)
        m.to(DEV)
        tr = pkg.train.Trainer(m, "something", learning_rate=1e-3, warmup_steps=1, total_steps=10, fused_optimizer=fused)
        assert tr.fused == fused
        log = []
        for s in range(3):
            batch = pkg.synth.make_batch(4, c["T"], c["N"], seed=60 + s)
            batch["labels"] = torch.randint(0, c["num_classes"], (4,), generator=torch.Generator().manual_seed(s))
            out = tr.step({k: v.to(DEV) for k, v in batch.items()})
            log.append((float(out["loss"]), float(out["grad_norm"])))
        runs.append((log, {k: v.detach().clone() for k, v in m.state_dict().items()}))
    (la, pa), (lb, pb) = runs
    for (l1, n1), (l2, n2) in zip(la, lb):
        assert abs(l1 - l2) <= 1e-5 and abs(n1 - n2) <= 1e-4 * max(n2, 1.0)
    for k in pa:
        if not pa[k].is_floating_point():
            continue
        a, b = pa[k], pb[k]
        if k.endswith("in_proj_bias"):
            # the key bias has no true gradient (softmax is shift-invariant along the keys): what arrives is rounding
            # noise, chaotic under the 1e-7 parameter differences of the previous step, and Adam normalises it to a full
            # step — compare the query / value parts only
            d = a.numel() // 3
            a, b = torch.cat([a[:d], a[2 * d:]]), torch.cat([b[:d], b[2 * d:]])
        # lr = 1e-3: agreement to 2 % of one step (Adam turns rounding-level differences of a near-zero gradient element into
        # a visible fraction of a step; 5e-6 held for one summation order of the forward and 6.8e-6 showed up with another)
        assert (a - b).abs().max().item() <= 2e-5, k


@pytest.mark.parametrize("kind", ["something", "action_genome"])
def test_fused_criterion_matches_torch(pkg, kind):
    T = importlib.import_module("revisiting-spatial-temporal-layouts_amd.train")
    g0 = torch.Generator().manual_seed(3)
    B, K = 37, 157
    logits = (torch.randn(B, K, generator=g0) * 3).to(DEV).requires_grad_(True)
    if kind == "something":
        labels = torch.randint(0, K, (B,), generator=g0).to(DEV)
    else:
        labels = (torch.rand(B, K, generator=g0) < 0.1).float().to(DEV)
    ref = T.criterion({"a": logits}, labels, kind)
    ref.backward()
    loss, dl = T.fused_criterion(logits, labels, kind)
    assert abs(loss.item() - ref.item()) <= 2e-6 * max(1.0, abs(ref.item()))
    assert (dl - logits.grad).abs().max().item() <= 1e-7
    half, dl_half = T.fused_criterion(logits, labels, kind, 0.5)  # two logit heads: each contributes half
    assert abs(half.item() - 0.5 * ref.item()) <= 2e-6 and (dl_half - 0.5 * logits.grad).abs().max().item() <= 1e-7


def test_fused_adamw_resumes_from_a_loaded_state_dict(pkg):
    """step, save, load into the SAME optimizer (and into a fresh one), step: the moments the kernel updates must be the
    loaded ones (torch's loader replaces the state tensors, so the flat buffers have to be re-bound)."""
    import copy
    T = importlib.import_module("revisiting-spatial-temporal-layouts_amd.train")
    g0 = torch.Generator().manual_seed(3)
    shapes = [(64, 40), (40,), (1000,)]
    ref_p = [torch.nn.Parameter(torch.randn(*s, generator=g0).to(DEV)) for s in shapes]
    our_p = [torch.nn.Parameter(p.detach().clone()) for p in ref_p]
    groups = lambda ps: [{"params": [ps[1]], "weight_decay": 0.0}, {"params": [ps[0], ps[2]], "weight_decay": 1e-2}]
    ref, ours = torch.optim.AdamW(groups(ref_p), lr=1e-2), T.FusedAdamW(groups(our_p), lr=1e-2)
    layout, off = [], 0
    for p in our_p:
        layout.append((p, off, p.numel()))
        off += (p.numel() + 3) // 4 * 4

    def both_step():
        grads = [torch.randn(*s, generator=g0).to(DEV) for s in shapes]
        for p, g in zip(ref_p, grads):
            p.grad = g.clone()
        ref.step()
        flat = torch.zeros(off, device=DEV)
        for (p, o, n), g in zip(layout, grads):
            flat[o:o + n] = g.reshape(-1)
        ours.step_flat(flat, layout, 0.0)

    both_step(); both_step()
    saved = copy.deepcopy(ours.state_dict())
    both_step()                              # moves the moments on ...
    snap_ref = copy.deepcopy(ref.state_dict())
    ours.load_state_dict(copy.deepcopy(saved))   # ... and the optimizer goes back to the saved state (torch's loader keeps
    ref.load_state_dict(copy.deepcopy(saved))    # the tensors it is handed: each optimizer gets its own copy)
    for a, b in zip(our_p, ref_p):
        b.data.copy_(a.data)
    both_step(); both_step()
    for a, b in zip(our_p, ref_p):
        assert (a - b).abs().max().item() <= 2e-6
    st_o, st_r = ours.state_dict()["state"], ref.state_dict()["state"]
    for k in st_r:
        assert float(st_o[k]["step"]) == float(st_r[k]["step"]) == 4.0
        assert (st_o[k]["exp_avg"] - st_r[k]["exp_avg"]).abs().max().item() <= 1e-6
        assert (st_o[k]["exp_avg_sq"] - st_r[k]["exp_avg_sq"]).abs().max().item() <= 1e-6
    del snap_ref


def test_fused_adamw_keeps_its_step_count_across_a_rebind(pkg):
    """A re-bind in the middle of training (the layout key changes: other offsets in the flat buffer, a parameter that moved,
    a second Trainer) must carry the AdamW step count on — exp_avg / exp_avg_sq carry over, so a count that restarts at 1 would
    scale the bias correction wrongly with no error raised (round-3 advisor finding).  Four steps with the flat layout changed
    after the second and the third one, against torch.optim.AdamW; the kernel's step argument is checked as well."""
    T = importlib.import_module("revisiting-spatial-temporal-layouts_amd.train")
    L = importlib.import_module("revisiting-spatial-temporal-layouts_amd._lib")
    g0 = torch.Generator().manual_seed(11)
    shapes = [(48, 20), (20,), (333,)]
    ref_p = [torch.nn.Parameter(torch.randn(*s, generator=g0).to(DEV)) for s in shapes]
    our_p = [torch.nn.Parameter(p.detach().clone()) for p in ref_p]
    groups = lambda ps: [{"params": [ps[1]], "weight_decay": 0.0}, {"params": [ps[0], ps[2]], "weight_decay": 1e-2}]
    ref, ours = torch.optim.AdamW(groups(ref_p), lr=1e-2), T.FusedAdamW(groups(our_p), lr=1e-2)

    def make_layout(order, gap):
        layout, off = {}, 0
        for i in order:
            layout[i] = (our_p[i], off, our_p[i].numel())
            off += (our_p[i].numel() + 3) // 4 * 4 + gap
        return [layout[i] for i in range(len(our_p))], off

    seen_steps = []
    lib = L.load()
    real = lib.stlt_adamw_step

    def spy(*args):
        seen_steps.append(int(args[10]))
        return real(*args)

    lib.stlt_adamw_step = spy
    try:
        for step, (order, gap) in enumerate([((0, 1, 2), 0), ((0, 1, 2), 0), ((2, 0, 1), 8), ((1, 2, 0), 4)]):
            layout, total = make_layout(order, gap)
            grads = [torch.randn(*s, generator=g0).to(DEV) for s in shapes]
            for p, g in zip(ref_p, grads):
                p.grad = g.clone()
            ref.step()
            flat = torch.zeros(total, device=DEV)
            for (p, o, n), g in zip(layout, grads):
                flat[o:o + n] = g.reshape(-1)
            ours.step_flat(flat, layout, 0.0)
            for a, b in zip(our_p, ref_p):
                assert (a - b).abs().max().item() <= 2e-6, step
    finally:
        lib.stlt_adamw_step = real
    assert seen_steps == [1, 1, 2, 2, 3, 3, 4, 4]  # two parameter groups per step
    for k, st in ours.state_dict()["state"].items():
        assert float(st["step"]) == 4.0


def test_alternating_batch_shapes_reuse_the_training_buffers_safely(pkg):
    """(B,T,N) = (4,6,4) and (4,5,4) round to the same tape / scratch byte counts with different row layouts: a step with
    the shorter clips after one with the longer ones must not pick up stale gradient rows (dW contracts over the row count
    rounded up to 32).  Gradients of every step are compared with the oracle's autograd."""
    name = "cfg1"
    c = pkg.synth.CONFIGS[name]
    H = c["num_attention_heads"]
    kw = pkg.synth.model_kwargs(name)
    m = pkg.Stlt(pkg.StltModelConfig(**kw))
    sd = pkg.synth.make_state_dict({k: tuple(v.shape) for k, v in m.state_dict().items()}, seed=41, gain=1.5)
    m.load_state_dict(sd)
    m.train(True)
    m.to(DEV)
    lib = pkg._lib.load()
    d, n_sp, n_tp = kw["hidden_size"], kw["num_spatial_layers"], kw["num_temporal_layers"]
    assert lib.stlt_train_tape_bytes(4, 6, 4, d, n_sp, n_tp) == lib.stlt_train_tape_bytes(4, 5, 4, d, n_sp, n_tp)
    for it, T in enumerate([6, 5, 6, 5]):
        batch = pkg.synth.make_batch(4, T, 4, dataset=c["dataset"], seed=90 + it)
        labels = torch.randint(0, c["num_classes"], (4,), generator=torch.Generator().manual_seed(it))
        ref_loss, _, ref_g = _oracle_grads(sd, batch, H, labels)
        for q in m.parameters():
            q.grad = None
        out = m({k: v.to(DEV) for k, v in batch.items()})["stlt"]
        F.cross_entropy(out, labels.to(DEV)).backward()
        worst = 0.0
        for k, q in m.named_parameters():
            if q.grad is None:
                continue
            r = ref_g[k].float()
            worst = max(worst, float((q.grad.cpu() - r).abs().max() / (r.abs().max() + 1e-6)))
        assert worst <= 2e-4, (it, T, worst)


def test_backward_refuses_a_tape_overwritten_by_a_later_forward(pkg):
    name = "cfg1"
    c = pkg.synth.CONFIGS[name]
    m = pkg.Stlt(pkg.StltModelConfig(**pkg.synth.model_kwargs(name)))
    m.train(True)
    m.to(DEV)
    b1 = {k: v.to(DEV) for k, v in pkg.synth.make_batch(2, c["T"], c["N"], seed=1).items()}
    b2 = {k: v.to(DEV) for k, v in pkg.synth.make_batch(2, c["T"], c["N"], seed=2).items()}
    l1 = m(b1)["stlt"]
    l2 = m(b2)["stlt"]  # a second grad-enabled forward re-records the one tape of the backbone
    with pytest.raises(pkg._lib.StltHipError, match="tape was overwritten"):
        l1.sum().backward()
    l2.sum().backward()  # the newest graph still owns the tape
    with torch.no_grad():
        m(b1)            # forwards without a graph leave the tape alone
    l3 = m(b1)["stlt"]
    l3.sum().backward()


def test_trainer_step_leaves_the_model_usable_by_a_plain_autograd_loop(pkg):
    name = "cfg1"
    c = pkg.synth.CONFIGS[name]
    m = pkg.Stlt(pkg.StltModelConfig(**pkg.synth.model_kwargs(name)))
    m.to(DEV)
    tr = pkg.train.Trainer(m, "something", learning_rate=1e-3, warmup_steps=0, total_steps=4)
    batch = pkg.synth.make_batch(2, c["T"], c["N"], seed=7)
    batch["labels"] = torch.randint(0, c["num_classes"], (2,))
    dev_batch = {k: v.to(DEV) for k, v in batch.items()}
    tr.step(dev_batch)
    assert not m._flat_grads_only and m._grad_sync is None
    F.cross_entropy(m(dev_batch)["stlt"], dev_batch["labels"]).backward()
    got = [q.grad is not None for k, q in m.named_parameters() if "prediction_head" in k]
    assert got and all(got)


def test_fused_criterion_flags_an_out_of_range_label(pkg):
    """torch raises on a class index outside [0, K); the fused criterion makes the loss (and that row's gradient) NaN instead
    of training on a clamped label."""
    x = torch.randn(5, 7, generator=torch.Generator().manual_seed(0)).to(DEV)
    y = torch.tensor([0, 6, 7, 2, -1])
    loss, dl = pkg.train.fused_criterion(x, y.to(DEV), "something")
    assert torch.isnan(loss)
    assert torch.isnan(dl[2]).all() and torch.isnan(dl[4]).all() and torch.isfinite(dl[[0, 1, 3]]).all()


def test_fused_criterion_ignores_label_minus_100_like_torch(pkg):
    """nn.CrossEntropyLoss (train_inference_utils.py:67-76) keeps torch's default ignore_index = -100: such clips add nothing
    and the mean runs over the others; a batch of only ignored clips gives NaN (torch's 0/0)."""
    g = torch.Generator().manual_seed(0)
    x = torch.randn(37, 174, generator=g)
    y = torch.randint(0, 174, (37,), generator=g)
    y[[3, 11, 36]] = -100
    xr = x.clone().requires_grad_(True)
    ref = torch.nn.functional.cross_entropy(xr, y)
    ref.backward()
    loss, dl = pkg.train.fused_criterion(x.cuda(), y.cuda(), "something")
    assert abs(loss.item() - ref.item()) <= 1e-5 and (dl.cpu() - xr.grad).abs().max().item() <= 1e-7
    assert (dl.cpu()[[3, 11, 36]] == 0).all()
    loss2, dl2 = pkg.train.fused_criterion(x.cuda(), torch.full((37,), -100).cuda(), "something")
    assert loss2.item() != loss2.item() and (dl2 == 0).all()


def test_transposed_weight_copies_serve_the_input_gradient_products(pkg):
    """csrc/wt_cache.hip: stlt_ctx_wt_refresh writes wt[k][n] = w[n][k] for every registered weight (ragged 64 x 64 tiles included) and,
    until stlt_ctx_wt_clear, the input-gradient products of calls that NAME THAT CONTEXT and route to the small tiles read the copy — a row
    range of a packed weight included (the cross-attention blocks' k | v rows of in_proj_weight).  Same dx as with the weight read as it
    lies (summation order aside), and as torch in fp64.  A call naming another context, or none, never reads a copy; a row range that
    starts off a multiple of four rows is not served (its copy would not be 16-byte aligned); hits count launched products."""
    import os
    if os.environ.get("STLT_GEMM16") == "0":
        pytest.skip("the small-tile kernel is switched off in this run: stlt_input_grad_small(tile 0) has nothing to route to")
    lib = pkg._lib.load()
    g = torch.Generator().manual_seed(3)
    shapes = [(768, 768), (2304, 768), (96, 100), (3072, 768), (160, 36)]
    ws = [(torch.randn(n, k, generator=g) / math.sqrt(k)).to(DEV) for n, k in shapes]
    wts = [torch.full((k, n), float("nan"), device=DEV) for n, k in shapes]
    ent = (pkg._lib.WtEntry * len(ws))()
    for e, w, t in zip(ent, ws, wts):
        e.w, e.wt, e.n_out, e.k_in = w.data_ptr(), t.data_ptr(), w.shape[0], w.shape[1]
    tctx, other = pkg.ops.TrainContext(), pkg.ops.TrainContext()
    side = torch.cuda.Stream()
    try:
        # the refresh runs on a stream of its own; the consumers below run on the current stream WITHOUT joining it: the library orders
        # every call that names the context behind the refresh's event
        side.wait_stream(torch.cuda.current_stream())
        pkg._lib.check(lib.stlt_ctx_wt_refresh(tctx.handle, ent, len(ws), side.cuda_stream), "stlt_ctx_wt_refresh")
        M = 2048
        x = torch.randn(M, 768, generator=g).to(DEV)
        cases = [(ws[0], 768), (ws[1][768:], 1536), (ws[3], 3072)]  # whole weights and the k | v rows of the packed in-projection
        with_copy = []
        for w, n_out in cases:
            dy = torch.randn(M, n_out, generator=torch.Generator().manual_seed(n_out)).to(DEV)
            with_copy.append((pkg.ops.input_grad_small(dy, w, 0, context=tctx), dy))
        assert tctx.wt_hits() == len(cases)
        torch.cuda.current_stream().wait_stream(side)
        for w, t in zip(ws, wts):
            assert torch.equal(t, w.t().contiguous())
        # another context, no context, a plain autograd backward, and a row range starting at row 770 (770 % 4 != 0): nothing reads a copy
        dy = with_copy[0][1]
        d_other = pkg.ops.input_grad_small(dy, ws[0], 0, context=other)
        d_none = pkg.ops.input_grad_small(dy, ws[0], 0)
        xr = x.clone().requires_grad_(True)
        pkg.ops.LinearFn.apply(xr, ws[0], None).backward(dy)
        dy_odd = torch.randn(M, 1504, generator=torch.Generator().manual_seed(9)).to(DEV)
        d_odd = pkg.ops.input_grad_small(dy_odd, ws[1][770:770 + 1504], 0, context=tctx)
        assert tctx.wt_hits() == len(cases) and other.wt_hits() == 0
        assert torch.equal(d_other, d_none) and torch.equal(xr.grad, d_none)
        assert (d_odd.double() - dy_odd.double() @ ws[1][770:770 + 1504].double()).abs().max().item() <= 1e-4
        pkg._lib.check(lib.stlt_ctx_wt_clear(tctx.handle), "stlt_ctx_wt_clear")
        for (dx_copy, dy), (w, n_out) in zip(with_copy, cases):
            dx_plain = pkg.ops.input_grad_small(dy, w, 0, context=tctx)  # withdrawn: the weights are read as they lie
            ref = dy.double() @ w.double()
            scale = ref.abs().max().item()
            assert (dx_plain.double() - ref).abs().max().item() / scale <= 1e-5  # fp32 accumulation over up to 3072 terms
            assert (dx_copy.double() - ref).abs().max().item() / scale <= 1e-5
        assert tctx.wt_hits() == len(cases)
        bad = (pkg._lib.WtEntry * 1)()
        bad[0].w, bad[0].wt, bad[0].n_out, bad[0].k_in = ws[0].data_ptr(), wts[0].data_ptr(), 767, 768
        assert lib.stlt_ctx_wt_refresh(tctx.handle, bad, 1, torch.cuda.current_stream().cuda_stream) != 0
        assert lib.stlt_ctx_wt_refresh(None, ent, len(ws), torch.cuda.current_stream().cuda_stream) != 0  # no context, no registry
    finally:
        torch.cuda.synchronize()
        tctx.close(); other.close()
    assert lib.stlt_ctx_wt_hits(None) == -1 and lib.stlt_ctx_destroy(None) == 0


def test_large_tile_input_gradients_run_as_forward_products_on_the_copies(pkg):
    """Round 6: an input-gradient product that stays on the large-tile kernel (the 14 336-row spatial products of a 64-clip step) is served
    from the context's transposed copy as well — the forward (NT) layout on Wt, add-source included — and gives the NN layout's result to
    the rounding of a different summation order; without a context the weight is read as it lies."""
    lib = pkg._lib.load()
    g = torch.Generator().manual_seed(11)
    M = 14336
    tctx = pkg.ops.TrainContext()
    try:
        for n_out, k_in in ((768, 3072), (3072, 768), (2304, 768)):
            assert lib.stlt_input_grad_small_choice(M, n_out, k_in) == 0  # the routing keeps these on the large tiles
            w = (torch.randn(n_out, k_in, generator=g) / math.sqrt(k_in)).to(DEV)
            wt = torch.empty(k_in, n_out, device=DEV)
            dy = torch.randn(M, n_out, generator=g).to(DEV)
            x = torch.zeros(M, k_in, device=DEV)
            ent = (pkg._lib.WtEntry * 1)()
            ent[0].w, ent[0].wt, ent[0].n_out, ent[0].k_in = w.data_ptr(), wt.data_ptr(), n_out, k_in
            stream = torch.cuda.current_stream().cuda_stream
            sc = torch.empty(int(lib.stlt_linear_bwd_scratch_bytes(n_out)), dtype=torch.uint8, device=DEV)

            def dx_of(handle):
                dx = torch.empty(M, k_in, device=DEV)
                pkg._lib.check(lib.stlt_linear_bwd(x.data_ptr(), w.data_ptr(), dy.data_ptr(), M, n_out, k_in, dx.data_ptr(), None, None, handle, sc.data_ptr(), sc.numel(),
                                                   stream), "stlt_linear_bwd")
                return dx

            plain = dx_of(None)
            pkg._lib.check(lib.stlt_ctx_wt_refresh(tctx.handle, ent, 1, stream), "stlt_ctx_wt_refresh")
            h0 = tctx.wt_hits()
            on_copy = dx_of(tctx.handle)
            assert tctx.wt_hits() == h0 + 1
            assert torch.equal(dx_of(None), plain)  # no context: never the copy
            pkg._lib.check(lib.stlt_ctx_wt_clear(tctx.handle), "stlt_ctx_wt_clear")
            ref = dy[:512].double() @ w.double()
            scale = ref.abs().max().item()
            assert (plain[:512].double() - ref).abs().max().item() / scale <= 1e-5
            assert (on_copy[:512].double() - ref).abs().max().item() / scale <= 1e-5
            assert (on_copy - plain).abs().max().item() / scale <= 1e-5
    finally:
        torch.cuda.synchronize()
        tctx.close()


def test_trainer_steps_agree_with_and_without_transposed_weight_copies(pkg, monkeypatch):
    """train.Trainer refreshes the copies at the start of every step and withdraws them at its end: three steps with dropout off give the
    same losses, gradient norms and parameters as with STLT_TRAIN_WT=0 (to the rounding of a different summation order in dX), the copies
    really served products, and none is current after a step."""
    name = "cfg1"
    c = pkg.synth.CONFIGS[name]
    lib = pkg._lib.load()
    runs = []
    for on in ("1", "0"):
        monkeypatch.setenv("STLT_TRAIN_WT", on)
        kw = dict(pkg.synth.model_kwargs(name), hidden_dropout_prob=0.0)
        m = pkg.Stlt(pkg.StltModelConfig(**kw))
        m.load_state_dict(pkg.synth.make_state_dict({k: tuple(v.shape) for k, v in m.state_dict().items()}, seed=1234))
        m.to(DEV)
        tr = pkg.train.Trainer(m, "something", learning_rate=1e-3, weight_decay=1e-3, clip_val=5.0, warmup_steps=0, total_steps=100)
        assert (tr.transposed is not None) == (on == "1")
        hits0 = tr.context.wt_hits()
        log = []
        for s in range(3):
            batch = pkg.synth.make_batch(48, c["T"], c["N"], seed=700 + s)
            batch["labels"] = torch.randint(0, c["num_classes"], (48,), generator=torch.Generator().manual_seed(800 + s))
            out = tr.step({k: v.to(DEV) for k, v in batch.items()})
            log.append((float(out["loss"]), float(out["grad_norm"])))
        used = tr.context.wt_hits() - hits0
        assert (used > 0) == (on == "1"), used
        # after the step: nothing is current, even for a call that names the trainer's context
        w2 = m.backbone.transformer.layers[0].linear2.weight
        rows = next((M for M in (2048, 1024, 512, 256, 128, 64) if lib.stlt_input_grad_small_choice(M, w2.shape[0], w2.shape[1]) != 0), None)
        if rows is not None:  # (None: the small-tile kernel is switched off in this run)
            h = tr.context.wt_hits()
            pkg.ops.input_grad_small(torch.randn(rows, w2.shape[0], device=DEV), w2, 0, context=tr.context)
            assert tr.context.wt_hits() == h
        runs.append((log, [p.detach().clone() for p in m.parameters()]))
    (log_a, pa), (log_b, pb) = runs
    for (la, ga), (lb, gb) in zip(log_a, log_b):
        assert abs(la - lb) <= 2e-6 * max(1.0, abs(lb)) and abs(ga - gb) <= 2e-5 * max(1.0, gb)
    assert max((a - b).abs().max().item() for a, b in zip(pa, pb)) <= 5e-4  # lr / 2 (Adam amplifies last-bit gradient noise up to the step size)
