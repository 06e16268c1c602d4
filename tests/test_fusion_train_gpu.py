"""CAF / CACNF / LCF (BASELINE config 5) against the fp64 fusion oracle across shapes: native inference, the training
gradients of the three layout-branch schedules (native tape, op-level with skip_padding, frozen), train mode with dropout
against the masked oracle (the appearance encoder's fixed 0.1 beside hidden_dropout_prob), the bench's full width, and the
Trainer in train mode.  Each test prints its worst error / bound."""
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import caf_oracle as CO
from oracle import stlt_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda"
FWD = {"caf": CO.caf_forward, "cacnf": CO.cacnf_forward, "lcf": CO.lcf_forward}
PREFIX = {"caf": "caf_backbone.", "cacnf": "backbone.", "lcf": ""}
# cfg1 widths (d = 256, 4 heads), layers trimmed so the fp64 oracle stays fast: two spatial layers (the tape runs the last one on
# the CLS rows only), one temporal, one appearance and one cross-modal layer
SMALL = dict(num_spatial_layers=2, num_temporal_layers=1, num_appearance_layers=1, num_fusion_layers=1)
# (B, T, N, appearance grid): S + 1 = 9 / 17 / 33 / 65 appearance tokens; T and N across 32 and 64; 1 024 / 2 112 rows at B = 64
SHAPES = [(1, 2, 1, (1, 2, 4)), (3, 16, 4, (1, 4, 4)), (2, 17, 5, (2, 4, 4)), (4, 33, 8, (2, 4, 4)), (2, 9, 33, (2, 4, 4)),
          (2, 65, 3, (2, 4, 4)), (2, 16, 4, (4, 4, 4)), (1, 100, 2, (4, 4, 4)), (64, 16, 4, (2, 4, 4))]
LOGIT_TOL = 1e-4
GRAD_TOL = 3e-4  # x max|g| per parameter tensor
DROP_LOGIT_TOL, DROP_GRAD_TOL = 4e-4, 5e-4  # test_dropout_forward_and_gradients_match_masked_oracle's bars (p > 0.1)
RELU_FED_TOL = 5e-3  # full width only: see test_full_width_cacnf_matches_fp64_oracle


def _report(name, ratio):
    print(f"\n[worst err/bound] {name}: {ratio:.3f}", file=sys.stderr)


def _model(pkg, name, S, p=0.0, seed=17, **extra):
    kw = dict(pkg.synth.model_kwargs("cfg1"), **SMALL, appearance_num_frames=S, hidden_dropout_prob=p)
    kw.update(extra)
    m = pkg.models_factory[name](pkg.MultimodalModelConfig(**kw))
    sd = pkg.synth.make_state_dict({k: tuple(v.shape) for k, v in m.state_dict().items()}, seed=seed)
    m.load_state_dict(sd)
    return m.to(DEV), sd, kw["num_attention_heads"]


def _batch(pkg, B, T, N, grid, seed):
    batch = pkg.synth.make_batch(B, T, N, seed=seed, min_len=2)
    batch["appearance_features"] = pkg.synth.make_appearance_features(B, seed=seed + 1, grid=grid)
    labels = torch.randint(0, 174, (B,), generator=torch.Generator().manual_seed(seed + 2))
    return batch, labels


def _layout_branch(pkg, m):
    (bb,) = [mod for mod in m.modules() if isinstance(mod, pkg.StltBackbone)]
    return bb


def _loss(out, labels):
    return sum(F.cross_entropy(v, labels) for v in out.values()) / len(out)


def _oracle(name, sd, batch, H, labels, drop=None, p=0.0):
    """fp64 autograd on the oracle -> (loss, logits, {key: grad or None})"""
    leaves = {k: (v.detach().double().requires_grad_(True) if v.is_floating_point() else v) for k, v in sd.items()}
    out = FWD[name](leaves, batch, H, dtype=torch.float64, drop=drop, p=p)
    loss = _loss(out, labels)
    loss.backward()
    return loss.item(), {k: v.detach() for k, v in out.items()}, {k: leaves[k].grad for k in sd if sd[k].is_floating_point()}


def _check_logits(out, ref, tol):
    assert set(out) == set(ref)
    worst = 0.0
    for k in ref:
        err = (out[k].detach().cpu().double() - ref[k]).abs().max().item()
        assert err <= tol, (k, err)
        worst = max(worst, err / tol)
    return worst


def _check_grads(m, ref_g, tol, frozen=(), minimum=20, relu_fed_tol=None):
    """every gradient within tol * max|g_ref| of fp64 autograd; ``relu_fed_tol``: the bar of the appearance encoder's linear1 weight /
    bias instead, whose gradient flips with any ReLU input that fp32 rounding moves across zero"""
    worst, checked = 0.0, 0
    for k, prm in m.named_parameters():
        g_ref = ref_g[k]
        if frozen and k.startswith(frozen):
            assert prm.grad is None or prm.grad.abs().max().item() == 0.0, k
            continue
        if g_ref is None or g_ref.abs().max().item() == 0.0:  # never read: the dead encoder_layer copy, scores, the unused classifier
            assert prm.grad is None or prm.grad.abs().max().item() == 0.0, k
            continue
        assert prm.grad is not None, k
        relu_fed = relu_fed_tol is not None and "appearance_branch.transformer.layers." in k and ".linear1." in k
        bound = (relu_fed_tol if relu_fed else tol) * g_ref.abs().max().item()
        err = (prm.grad.detach().cpu().double() - g_ref).abs().max().item()
        assert err <= bound, (k, err / bound)
        worst = max(worst, err / bound)
        checked += 1
    assert checked >= minimum, checked
    return worst


@pytest.mark.parametrize("B,T,N,grid", SHAPES)
@pytest.mark.parametrize("name", ["caf", "cacnf", "lcf"])
def test_inference_and_gradients_match_fp64_oracle(pkg, name, B, T, N, grid):
    S = int(np.prod(grid))
    m, sd, H = _model(pkg, name, S)
    batch, labels = _batch(pkg, B, T, N, grid, seed=100 * T + N + B)
    ref_loss, ref_out, ref_g = _oracle(name, sd, batch, H, labels)
    dev = {k: v.to(DEV) for k, v in batch.items()}
    bb = _layout_branch(pkg, m)
    m.train(False)  # eval mode: no dropout, the appearance encoder's fixed 0.1 included; grad on -> the training composition
    worst_fwd = 0.0
    with torch.no_grad():  # native inference (stlt_caf_forward_flags), padded and on the real tokens only
        for skip in (False, True):
            bb.skip_padding = skip
            worst_fwd = max(worst_fwd, _check_logits(m(dev), ref_out, LOGIT_TOL))
    worst_grad = 0.0
    frozen_prefix = PREFIX[name] + "layout_branch."
    for schedule in ("tape", "ops", "frozen"):
        bb.skip_padding = schedule == "ops"
        for q in bb.parameters():
            q.requires_grad_(schedule != "frozen")
        m.zero_grad(set_to_none=True)
        out = m(dev)
        worst_fwd = max(worst_fwd, _check_logits(out, ref_out, LOGIT_TOL))
        loss = _loss(out, labels.to(DEV))
        assert abs(loss.item() - ref_loss) <= 1e-5, (schedule, loss.item(), ref_loss)
        loss.backward()
        frozen = frozen_prefix if schedule == "frozen" else ()
        worst_grad = max(worst_grad, _check_grads(m, ref_g, GRAD_TOL, frozen))
    _report(f"{name} {(B, T, N, grid)} logits", worst_fwd)
    _report(f"{name} {(B, T, N, grid)} gradients", worst_grad)


def _record_block_calls(monkeypatch, pkg):
    """Wrap ops._block_dropout: every block call that draws a seed, as (kind, shape, seed) in call order."""
    ops = pkg.ops
    real = ops._block_dropout
    log = []

    def wrapped(p):
        res = real(p)
        if res[0] > 0:  # the caller is AttnBlockFn.forward (it has Lk) or FfnBlockFn.forward (it has inner_dropout)
            loc = sys._getframe(1).f_locals
            if "Lk" in loc:
                log.append(("attn", (int(loc["S"]), int(loc["Lq"]), int(loc["Lk"])), res[1]))
            elif "inner_dropout" in loc:
                log.append(("ffn", (int(loc["M"]),), res[1]))
            else:
                log.append(("?", (), res[1]))
        return res

    monkeypatch.setattr(ops, "_block_dropout", wrapped)
    return log


def _replayed_seeds(k, n=400):
    """The seeds the native calls draw after torch.manual_seed(k): torch.randint(0, 2**62, (1,)) on the default CPU generator."""
    g = torch.Generator().manual_seed(k)
    return [int(torch.randint(0, 2 ** 62, (1,), generator=g).item()) for _ in range(n)]


# T = 56 against 33 appearance tokens: the cross-attention backward of 49 - 64 tokens (bwd_api.hip's LDS kernel; Lq != Lk, so a
# query-token index built from the key count fails here); up to 48 tokens it is attn_bwdx16.hip, above 64 the streamed kernel
DROP_CASES = [("caf", 3, 16, 4, (1, 4, 4)), ("caf", 2, 65, 3, (2, 4, 4)), ("caf", 2, 56, 3, (2, 4, 4)), ("cacnf", 2, 17, 5, (2, 4, 4)),
              ("cacnf", 1, 100, 2, (4, 4, 4)), ("lcf", 2, 9, 33, (2, 4, 4))]


@pytest.mark.parametrize("schedule", ["tape", "ops"])
@pytest.mark.parametrize("name,B,T,N,grid", DROP_CASES)
def test_train_mode_dropout_matches_masked_fp64_oracle(pkg, monkeypatch, name, B, T, N, grid, schedule):
    """hidden_dropout_prob = 0.3 in train mode: every dropout of the training composition — the layout branch's (one tape seed, or
    one seed per DropoutFn / block call), the appearance encoder's fixed 0.1 (attention probabilities, dropout1, the ReLU FFN's
    inner dropout, dropout2), the two sites of each cross-modal block — against the oracle applying the same masks.  The block
    calls must come in the oracle's order with the oracle's seeds, so a reordering fails here rather than misaligning masks."""
    p = 0.3
    S = int(np.prod(grid))
    m, sd, H = _model(pkg, name, S, p=p, seed=23)
    batch, labels = _batch(pkg, B, T, N, grid, seed=7 * T + N)
    bb = _layout_branch(pkg, m)
    bb.skip_padding = schedule == "ops"
    m.train(True)
    k = 1000 + T
    calls = O.CallSeeds(_replayed_seeds(k), schedule)
    ref_loss, ref_out, ref_g = _oracle(name, sd, batch, H, labels, drop=calls, p=p)
    log = _record_block_calls(monkeypatch, pkg)
    dev = {key: v.to(DEV) for key, v in batch.items()}
    torch.manual_seed(k)
    out = m(dev)
    assert log == [e for e in calls.log if e[0] in ("attn", "ffn")]
    n_blocks = 2 * SMALL["num_appearance_layers"] + (6 * SMALL["num_fusion_layers"] if name != "lcf" else 0)
    if schedule == "ops":
        n_blocks += 2 * (SMALL["num_spatial_layers"] + SMALL["num_temporal_layers"])
    assert len(log) == n_blocks
    worst_fwd = _check_logits(out, ref_out, DROP_LOGIT_TOL)
    loss = _loss(out, labels.to(DEV))
    assert abs(loss.item() - ref_loss) <= 1e-4, (loss.item(), ref_loss)
    loss.backward()
    worst_grad = _check_grads(m, ref_g, DROP_GRAD_TOL)
    _report(f"dropout p={p} (appearance 0.1) {name} {schedule} {(B, T, N, grid)} logits", worst_fwd)
    _report(f"dropout p={p} (appearance 0.1) {name} {schedule} {(B, T, N, grid)} gradients", worst_grad)
    # dropout really is on: another seed, other logits
    with torch.no_grad():
        torch.manual_seed(k + 1)
        other = m(dev)
        torch.manual_seed(k)
        again = m(dev)
    assert max((other[h] - out[h]).abs().max().item() for h in out) > 1e-3
    assert all(torch.equal(again[h], out[h].detach()) for h in out)


def _full_width(pkg, B):
    c = pkg.synth.CONFIGS["cfg2"]
    kw = dict(pkg.synth.model_kwargs("cfg2"), appearance_num_frames=32)  # 4 spatial, 8 temporal, 4 appearance, 4 fusion layers
    m = pkg.CrossAttentionCentralNetFusion(pkg.MultimodalModelConfig(**kw))
    sd = pkg.synth.make_state_dict({k: tuple(v.shape) for k, v in m.state_dict().items()}, seed=5)
    m.load_state_dict(sd)
    batch = pkg.synth.make_batch(B, c["T"], c["N"], seed=8, min_len=2)
    batch["appearance_features"] = pkg.synth.make_appearance_features(B, seed=9)
    labels = torch.randint(0, 174, (B,), generator=torch.Generator().manual_seed(3))
    return m.to(DEV), sd, batch, labels, c["num_attention_heads"]


def test_full_width_cacnf_matches_fp64_oracle(pkg):
    """The bench's shard: CACNF at d = 768, 12 heads, 4 spatial / 8 temporal / 4 appearance / 4 fusion layers, B = 64, T = 32, N = 7:
    native logits (padded and skip_padding), gradients through plain autograd and inside a Trainer step with the grouped
    weight-gradient launches (ops.deferred_block_weight_grads)."""
    B = 64
    m, sd, batch, labels, H = _full_width(pkg, B)
    ref_loss, ref_out, ref_g = _oracle("cacnf", sd, batch, H, labels)
    dev = {k: v.to(DEV) for k, v in batch.items()}
    bb = _layout_branch(pkg, m)
    m.train(False)
    worst_fwd = 0.0
    with torch.no_grad():
        for skip in (False, True):
            bb.skip_padding = skip
            worst_fwd = max(worst_fwd, _check_logits(m(dev), ref_out, LOGIT_TOL))
    bb.skip_padding = False
    out = m(dev)
    loss = _loss(out, labels.to(DEV))
    assert abs(loss.item() - ref_loss) <= 1e-5
    loss.backward()
    # 2 112 appearance rows x 3 072 ReLU units: fp32 moves some ReLU inputs across zero.  The fp32 CPU oracle is itself 5.6x the 3e-4
    # bar from fp64 on those linear1 tensors (1.7e-3 of max|g|; 1.1e-3 measured here); every other gradient keeps the bar
    worst_plain = _check_grads(m, ref_g, GRAD_TOL, minimum=150, relu_fed_tol=RELU_FED_TOL)
    # inside a Trainer step: .grad views of one flat buffer, native criterion, the blocks' weight-gradient products deferred and grouped
    tr = pkg.train.Trainer(m, "something", learning_rate=1e-3, weight_decay=1e-3, clip_val=5.0, warmup_steps=0, total_steps=1000)
    tr.bound.zero()
    heads = list(m(dev).values())
    grads = [pkg.train.fused_criterion(v, labels.to(DEV), "something", 1.0 / len(heads))[1] for v in heads]
    tr.bound.accumulating = True
    try:
        with pkg.ops.deferred_block_weight_grads(tr.context):
            torch.autograd.backward(heads, grads)
            assert tr.context.dw_pending() > 0
    finally:
        tr.bound.accumulating = False
    assert tr.context.dw_pending() == 0
    worst_trainer = _check_grads(m, ref_g, GRAD_TOL, minimum=150, relu_fed_tol=RELU_FED_TOL)
    _report("full width CACNF B=64 logits", worst_fwd)
    _report("full width CACNF B=64 gradients (autograd)", worst_plain)
    _report("full width CACNF B=64 gradients (Trainer, deferred)", worst_trainer)


def test_trainer_in_train_mode_with_dropout_matches_the_stock_loop(pkg):
    """test_trainer_on_a_fusion_model_matches_the_stock_loop in train mode, hidden_dropout_prob = 0.1: the two twins draw the same
    masks (torch.manual_seed before each step), so losses, gradient norms and parameters still agree after three steps."""
    kw = dict(pkg.synth.model_kwargs("cfg1"), appearance_num_frames=32, num_appearance_layers=2, num_fusion_layers=2, hidden_dropout_prob=0.1)
    c = pkg.synth.CONFIGS["cfg1"]
    batch = pkg.synth.make_batch(6, c["T"], c["N"], seed=21)
    batch["appearance_features"] = pkg.synth.make_appearance_features(6, seed=22)
    batch = {k: v.to(DEV) for k, v in batch.items()}
    labels = torch.randint(0, c["num_classes"], (6,), generator=torch.Generator().manual_seed(5)).to(DEV)
    batch["labels"] = labels
    twins = []
    for _ in range(2):
        m = pkg.CrossAttentionCentralNetFusion(pkg.MultimodalModelConfig(**kw))
        m.load_state_dict(pkg.synth.make_state_dict({k: tuple(v.shape) for k, v in m.state_dict().items()}, seed=7))
        twins.append(m.to(DEV))
    ours, ref = twins
    tr = pkg.train.Trainer(ours, "something", learning_rate=1e-3, weight_decay=1e-3, clip_val=5.0, warmup_steps=0, total_steps=1000)
    ref.train(True)
    opt = torch.optim.AdamW(pkg.train.add_weight_decay(ref, 1e-3), lr=1e-3)
    sched = pkg.train.linear_schedule_with_warmup(opt, 0, 1000)
    for step in range(3):
        torch.manual_seed(50 + step)
        res = tr.step(batch)
        assert ours.training
        torch.manual_seed(50 + step)
        opt.zero_grad(set_to_none=True)
        out = ref(batch)
        loss = sum(F.cross_entropy(v, labels) for v in out.values()) / len(out)
        loss.backward()
        norm = torch.nn.utils.clip_grad_norm_(ref.parameters(), 5.0)
        opt.step(); sched.step()
        assert abs(res["loss"].item() - loss.item()) <= 2e-5, (step, res["loss"].item(), loss.item())
        assert abs(res["grad_norm"].item() - norm.item()) <= 2e-4 * max(1.0, norm.item()), (step, res["grad_norm"].item(), norm.item())
    worst = max((a - b).abs().max().item() for a, b in zip(ours.parameters(), ref.parameters()))
    assert worst <= 5e-4, worst  # lr / 2, as in the eval-mode comparison
