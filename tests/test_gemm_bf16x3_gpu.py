"""The opt-in split-bf16 forward GEMM (csrc/gemm_bf16x3.hip): f32-equivalent results from six bf16 MFMA products per f32
product.  Parity bar: its error against an fp64 product is within 1.5x the f32-MFMA kernel's on the same inputs (tolerance
written below), shapes it does not take give the f32 kernel's bits, and the whole forward's logits agree to 2e-4."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.fixture
def split(pkg):
    yield pkg.ops.set_gemm_split_bf16
    pkg.ops.set_gemm_split_bf16(0)


def _operands(M, N, K, seed):
    g = torch.Generator(device=DEV).manual_seed(seed)
    x = torch.randn(M, K, device=DEV, generator=g)
    w = torch.randn(N, K, device=DEV, generator=g) / math.sqrt(K)
    b = torch.randn(N, device=DEV, generator=g)
    return x, w, b


# whole-tile launches that fill at least half of the chip's workgroups: (M, N, K, act, bias?)
SHAPES = [(12345, 777, 96, 0, True),      # ragged both ways, 49 x 7 tiles = two rounds at fill 0.67
          (16347, 507, 96, 0, True),      # ragged last row block and column block (64 x 4 tiles)
          (10240, 768, 768, 1, True),     # GELU epilogue, 40 x 6 tiles
          (16384, 512, 64, 2, True),      # ReLU, the shortest contraction the kernel takes (two k-steps)
          (65536, 256, 3072, 0, False),   # no bias, 256 x 2 tiles = two rounds
          (13312, 2304, 768, 0, True)]    # an in-projection shape, 52 x 18 tiles = four rounds at fill 0.91


@pytest.mark.parametrize("M,N,K,act,with_bias", SHAPES)
def test_split_bf16_linear_error_vs_fp64_is_the_f32_kernels(pkg, split, M, N, K, act, with_bias):
    x, w, b = _operands(M, N, K, seed=M + N)
    bias = b if with_bias else None
    with pkg.ops.gemm_scratch(DEV):
        split(0)
        y0 = pkg.ops.linear(x, w, bias, act=act)
        split(6)
        y6 = pkg.ops.linear(x, w, bias, act=act)
    g = torch.Generator(device=DEV).manual_seed(1)
    idx = torch.cat([torch.randperm(M, device=DEV, generator=g)[:1500], torch.arange(M - 40, M, device=DEV)])
    ref = x[idx].double() @ w.double().t()
    if with_bias:
        ref = ref + b.double()
    if act == 1:
        ref = torch.nn.functional.gelu(ref)
    elif act == 2:
        ref = torch.relu(ref)
    e0 = (y0[idx].double() - ref).abs()
    e6 = (y6[idx].double() - ref).abs()
    assert not torch.equal(y0, y6), "the split-bf16 kernel did not run (results are the f32 kernel's bits)"
    assert e6.max().item() <= 1.5 * e0.max().item() + 1e-7
    assert e6.mean().item() <= 1.1 * e0.mean().item() + 1e-9
    assert torch.isfinite(y6).all()


@pytest.mark.parametrize("M,N,K", [(4000, 777, 96),     # 16 x 7 tiles: launch fill 0.44, stream-K stays
                                   (16384, 512, 32),    # a single k-step
                                   (300, 130, 64)])
def test_split_bf16_leaves_other_shapes_to_the_f32_kernel(pkg, split, M, N, K):
    x, w, b = _operands(M, N, K, seed=7)
    with pkg.ops.gemm_scratch(DEV):
        split(0)
        y0 = pkg.ops.linear(x, w, b, act=1)
        split(6)
        y6 = pkg.ops.linear(x, w, b, act=1)
    assert torch.equal(y0, y6)


def test_split_bf16_special_operands_fall_in_the_f32_kernels_result_class(pkg, split):
    """inf / NaN / subnormal / +-FLT_MAX operands (round-3 review): wherever the f32 kernel's output is finite the split kernel's is
    finite and within the eps * sqrt(K) bound of it; wherever the f32 kernel's is not (an infinite or NaN operand, an overflowing
    sum) the split kernel's is not either — as NaN where the f32 kernel may say +-inf (a - a0 of an infinity is NaN), which is the
    documented difference (include/stlt_hip.h).  Rows without special operands keep the ordinary error bound."""
    M, N, K = 10240, 768, 768
    x, w, b = _operands(M, N, K, seed=99)
    FLT_MAX, tiny = 3.4028234663852886e38, 1e-41  # 1e-41: an f32 subnormal
    x[5, 17] = float("inf")
    x[6, 100] = float("-inf")
    x[7, 3] = float("nan")
    x[8, :] = tiny * torch.arange(1, K + 1, device=DEV)         # a whole row of subnormals
    x[9, 40] = FLT_MAX                                            # one huge element: finite outputs of ~1e37
    x[10, 41] = -FLT_MAX
    x[11, 50] = FLT_MAX; x[11, 51] = FLT_MAX                      # two of them against weights of one sign: the sum overflows
    w[3, :] = tiny                                                # a subnormal weight row
    w[:, 50] = w[:, 50].abs() + 0.75; w[:, 51] = w[:, 51].abs() + 0.75
    with pkg.ops.gemm_scratch(DEV):
        split(0)
        y0 = pkg.ops.linear(x, w, b)
        split(6)
        y6 = pkg.ops.linear(x, w, b)
    assert not torch.equal(y0[100:], y6[100:]), "the split-bf16 kernel did not run"
    fin0, fin6 = torch.isfinite(y0), torch.isfinite(y6)
    assert torch.equal(fin0, fin6), f"finite / non-finite pattern differs in {int((fin0 != fin6).sum())} outputs"
    assert not fin0[5].any() and not fin0[6].any() and not fin0[7].any() and not fin0[11].any()  # the special rows really are special
    assert fin0[8].all() and fin0[9].all() and fin0[10].all() and fin0[:, 3][fin0[:, 3]].numel() > M - 10
    assert torch.isnan(y6[7]).all() and torch.isnan(y0[7]).all()
    # finite outputs: the bound of one sequential f32 accumulation, relative to the row's largest output
    scale = y0.masked_fill(~fin0, 0).abs().amax(dim=1, keepdim=True).clamp_min(1e-30)
    rel = ((y6 - y0).masked_fill(~fin0, 0).abs() / scale).max().item()
    assert rel <= 1.2e-7 * math.sqrt(K) * 4, rel


def test_split_bf16_setter_rejects_other_term_counts(pkg):
    with pytest.raises(pkg.StltHipError):
        pkg.ops.set_gemm_split_bf16(3)
    pkg.ops.set_gemm_split_bf16(0)


def test_split_bf16_forward_logits_agree_with_the_f32_forward(pkg, split):
    """cfg2 (12 layers, d = 768) at 64 clips: every product of the spatial tower — residual-add epilogues included — and the
    temporal FFN products run split-bf16; logits within 2e-4 of the f32 forward (both are f32-rounding-level from fp64)."""
    c = pkg.synth.CONFIGS["cfg2"]
    kw = pkg.synth.model_kwargs("cfg2")
    model = pkg.Stlt(pkg.StltModelConfig(**kw))
    model.load_state_dict(pkg.synth.make_state_dict({k: tuple(v.shape) for k, v in model.state_dict().items()}, seed=1234))
    model.train(False).to(DEV)
    batch = {k: v.to(DEV) for k, v in pkg.synth.make_batch(64, c["T"], c["N"], dataset=c["dataset"], seed=5).items()}
    with torch.no_grad():
        split(0)
        l0 = model(batch)["stlt"].clone()
        split(6)
        l6 = model(batch)["stlt"].clone()
    assert not torch.equal(l0, l6), "the split-bf16 kernel did not run inside the forward"
    assert (l0 - l6).abs().max().item() <= 2e-4


def test_split_bf16_wide_dynamic_range(pkg, split):
    """Rows of X scaled over 24 decades and columns of W over 12: the error relative to sum |x||w| (what an f32 dot product
    guarantees) stays within 1.5x the f32 kernel's — the three pieces follow each element's own exponent."""
    M, N, K = 16384, 512, 256
    g = torch.Generator(device=DEV).manual_seed(11)
    x = torch.randn(M, K, device=DEV, generator=g) * torch.pow(10.0, torch.rand(M, 1, device=DEV, generator=g) * 24 - 12)
    w = torch.randn(N, K, device=DEV, generator=g) * torch.pow(10.0, torch.rand(N, 1, device=DEV, generator=g) * 12 - 6)
    with pkg.ops.gemm_scratch(DEV):
        split(0)
        y0 = pkg.ops.linear(x, w, None)
        split(6)
        y6 = pkg.ops.linear(x, w, None)
    idx = torch.randperm(M, device=DEV, generator=g)[:1024]
    ref = x[idx].double() @ w.double().t()
    cond = x[idx].double().abs() @ w.double().abs().t()
    e0 = ((y0[idx].double() - ref).abs() / cond).max().item()
    e6 = ((y6[idx].double() - ref).abs() / cond).max().item()
    assert not torch.equal(y0, y6)
    assert torch.isfinite(y6).all()
    assert e6 <= 1.5 * e0 and e6 < 2e-6, (e0, e6)


def test_split_bf16_training_forward_gives_the_same_loss_and_gradients(pkg, split):
    """cfg2 / 64 clips, dropout 0.1 (counter-based masks: the same in both runs): with the forward and
    input-gradient products of the step on the split-bf16 kernel (blocks.hip: stlt_input_grad transposes the weight and runs the NT
    form), the loss and every parameter gradient agree with the f32 run to rounding level; the weight-gradient products stay
    on the f32 kernel."""
    c = pkg.synth.CONFIGS["cfg2"]
    kw = dict(pkg.synth.model_kwargs("cfg2"), hidden_dropout_prob=0.1)
    batch = {k: v.to(DEV) for k, v in pkg.synth.make_batch(64, c["T"], c["N"], dataset=c["dataset"], seed=9).items()}
    labels = torch.randint(0, c["num_classes"], (64,), generator=torch.Generator().manual_seed(3)).to(DEV)

    def run(terms):
        m = pkg.Stlt(pkg.StltModelConfig(**kw))
        m.load_state_dict(pkg.synth.make_state_dict({k: tuple(v.shape) for k, v in m.state_dict().items()}, seed=1234))
        m.train(True).to(DEV)
        split(terms)
        torch.manual_seed(0)  # the dropout seed is drawn from torch's CPU generator
        loss = torch.nn.functional.cross_entropy(m(batch)["stlt"], labels)
        loss.backward()
        return loss.item(), {k: p.grad.detach().clone() for k, p in m.named_parameters() if p.grad is not None}

    l0, g0 = run(0)
    l6, g6 = run(6)
    assert abs(l0 - l6) <= 2e-5, (l0, l6)
    worst = 0.0
    for k in g0:
        scale = max(g0[k].abs().max().item(), 1e-8)
        worst = max(worst, (g0[k] - g6[k]).abs().max().item() / scale)
    assert worst <= 2e-4, worst
    assert any(not torch.equal(g0[k], g6[k]) for k in g0), "the split-bf16 kernel did not run in the training forward"


def test_split_bf16_fusion_training_step_gives_the_same_loss_and_gradients(pkg, split):
    """CACNF (layout branch + appearance features through the block-level training API, csrc/blocks.hip) at 64 clips: forward and
    input-gradient products on the split-bf16 kernel, loss and every parameter gradient against the f32 run."""
    c = pkg.synth.CONFIGS["cfg2"]
    kw = dict(pkg.synth.model_kwargs("cfg2"), appearance_num_frames=32, hidden_dropout_prob=0.1)
    batch = pkg.synth.make_batch(64, c["T"], c["N"], seed=21)
    batch["appearance_features"] = pkg.synth.make_appearance_features(64, seed=2)
    batch = {k: v.to(DEV) for k, v in batch.items()}
    labels = torch.randint(0, c["num_classes"], (64,), generator=torch.Generator().manual_seed(4)).to(DEV)

    def run(terms):
        m = pkg.models_factory["cacnf"](pkg.MultimodalModelConfig(**kw))
        m.load_state_dict(pkg.synth.make_state_dict({k: tuple(v.shape) for k, v in m.state_dict().items()}, seed=1234))
        m.train(True).to(DEV)
        split(terms)
        torch.manual_seed(0)  # dropout seeds come from torch's CPU generator
        out = m(batch)
        loss = sum(torch.nn.functional.cross_entropy(v, labels) for v in out.values())
        loss.backward()
        return loss.item(), {k: p.grad.detach().clone() for k, p in m.named_parameters() if p.grad is not None}

    l0, g0 = run(0)
    l6, g6 = run(6)
    assert abs(l0 - l6) <= 1e-4, (l0, l6)
    for k in g0:
        scale = max(g0[k].abs().max().item(), 1e-8)
        err = (g0[k] - g6[k]).abs().max().item() / scale
        # the appearance branch's encoder layers use ReLU: a hidden unit within rounding of zero switches its derivative between
        # the two runs (about ten of 6.5 M units at these sizes), which moves single rows of linear1's gradient by ~1e-3 of the
        # largest entry — not a rounding-level effect of the products themselves; every other parameter agrees to 5e-4
        tol = 1e-2 if ("appearance_branch.transformer.layers" in k and ".linear1." in k) else 5e-4
        assert err <= tol, (k, err)
    assert any(not torch.equal(g0[k], g6[k]) for k in g0), "the split-bf16 kernel did not run"
