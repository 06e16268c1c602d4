"""The cases of tests/scale_cases.py held to their own conditions, without a GPU: every reference is finite, the rows of an output cover
all of it, and torch's fp32 error E_t stays within 256 u in every group (past that the bar 4 * max(E_t, u) means nothing).  Also the
metric itself, and on the CPU the finding that started the module: the cross-entropy gradient written as exp(x - (m + log sum)) misses the
bar from logit scale 8 on while exp((x - m) - log sum) keeps it."""
import math

import pytest
import torch

import scale_cases as C

ALL_CASES = (
    [("cross entropy", C.cross_entropy_case, (B, K, variant, w)) for B, K in C.CE_SHAPES for variant in (0, 1) for w in C.WEIGHTS]
    + [("cross entropy", C.cross_entropy_case, (6, 174, 0, w, 2)) for w in C.WEIGHTS]
    + [("bce", C.bce_case, (B, K, w)) for B, K in C.BCE_SHAPES for w in C.WEIGHTS]
    + [("adamw", C.adamw_case, (lr, clip, late)) for lr in C.OPT_LRS for clip in (True, False) for late in (False, True)]
    + [("norm", C.norm_case, (n, s, clip)) for n in C.NORM_SIZES for s in C.NORM_SCALES for clip in (True, False)]
    + [("layernorm", C.layernorm_case, (d, eps, res)) for d in C.LN_D for eps in C.LN_EPS for res in (True, False)]
    + [("layernorm parameter gradients", C.layernorm_param_grad_case, (d, eps, c)) for d in C.LN_D for eps in C.LN_EPS for c in range(len(C.LN_COMBOS))]
    + [("frames_embed", C.frames_embed_case, (d,)) for d in C.LN_D]
    + [("embed", C.embed_case, (d, s)) for d in C.LN_D for s in (True, False)]
    + [("attention", C.attention_case, (L, L, causal)) for L in C.ATTN_L for causal in (False, True)]
    + [("cross attention", C.attention_case, (3, 70, False))]
    + [("mhsa", C.mhsa_case, (L, causal)) for L in (5, 33) for causal in (True, False)]
)


@pytest.mark.parametrize("name,make,args", ALL_CASES, ids=[f"{n}-{'-'.join(str(a) for a in args)}" for n, _, args in ALL_CASES])
def test_case_keeps_the_three_conditions(name, make, args):
    case = make(*args)
    bad = []
    for key, o in case["outs"].items():
        assert o.ref.dtype == torch.float64 and o.ref.dim() == 2 and len(o.group) == o.ref.shape[0]
        bad += [f"{key}: {b}" for b in C.conditions(o)]
        for g, e in C.yardstick(o).items():
            print(f"[scale] {name} {args} {key} | {g} | E_t/u {e / C.U:.2f}")
    assert not bad, "\n".join(bad)


def test_gelu_points_keep_the_three_conditions_and_every_point_is_in_a_row():
    case = C.gelu_case()
    x = case["x"]
    lo, hi = C.GELU_BINADES
    assert x.numel() == 2 * (64 * (hi - lo) + len(C.GELU_SPECIALS))
    for e in range(lo, hi):
        for sign in (1, -1):
            assert int(((x * sign >= 2.0 ** e) & (x * sign < 2.0 ** (e + 1))).sum()) >= 64
    for s in C.GELU_SPECIALS:
        assert bool((x == torch.tensor(s, dtype=torch.float32)).any()) and bool((x == -torch.tensor(s, dtype=torch.float32)).any())
    assert bool(((x == 0) & torch.signbit(x)).any())
    for which in ("fwd", "bwd"):
        o = C.gelu_out(case, which)
        assert sorted(set(C.gelu_rows(case, torch.arange(x.numel())).reshape(-1).tolist())) == list(range(x.numel()))
        bad = C.conditions(o)
        for g, e in C.yardstick(o).items():
            print(f"[scale] gelu {which} | {g} | E_t/u {e / C.U:.2f}")
        assert not bad, "\n".join(bad)


def test_gelu_block_chunks_hold_every_point_and_scaled_derivative_keeps_the_conditions():
    case = C.gelu_case()
    n = case["x"].numel()
    chunks = C.gelu_block_chunks(case, 768)
    assert sorted(set(torch.cat([c[0] for c in chunks]).tolist())) == list(range(n))
    for pos, b1, w2, alpha in chunks:
        assert torch.equal(b1, case["x"][pos]) and int((w2 != 0).sum()) == b1.numel() and bool(((w2 != 0).sum(0) == 1).all())
        assert bool((torch.log2(alpha) == torch.log2(alpha).round()).all())                       # powers of two: the products with them are exact
        h = torch.nn.functional.gelu(b1.double()) * alpha.double()
        assert bool(torch.isfinite(h).all()) and h.abs().max().item() <= 2.0
    v = torch.randn(n, generator=torch.Generator().manual_seed(0)) * 1e-3
    assert C.conditions(C.gelu_scaled_derivative_out(case, v)) == []


def test_rows_cover_every_element():
    """An output's rows are a reshape of all of it: nothing is masked out of a comparison."""
    case = C.attention_case(33, 33, True)
    S, L, d = case["q"].shape
    assert case["outs"]["ctx"].ref.numel() == S * L * d and case["outs"]["dqkv"].ref.numel() == 3 * S * L * d
    assert case["outs"]["probabilities per head"].ref.numel() == S * C.ATTN_H * L * L
    t = torch.arange(S * L * d, dtype=torch.float64).reshape(S, L, d)
    assert sorted(C.head_rows(t).reshape(-1).tolist()) == list(range(S * L * d))
    head0 = C.head_rows(t)[0].reshape(L, C.ATTN_DH)
    assert torch.equal(head0, t[0, :, :C.ATTN_DH])
    ln = C.layernorm_case(64, 1e-5, True)
    assert ln["outs"]["forward"].ref.shape == ln["x"].shape and ln["outs"]["ds"].ref.shape == ln["x"].shape


def test_metric_judges_rows_on_their_own_scale():
    ref = torch.tensor([[1.0, -2.0], [1e-6, 2e-6], [0.0, 0.0]], dtype=torch.float64)
    yard = ref.clone()
    yard[0, 0] += 2 * C.U          # e_t = u on the first row
    o = C.out(ref, yard, ["a", "b", "c"])
    good = ref.clone()
    good[1, 0] += 2e-6 * 3.9 * C.U   # under 4 u of the small row's own scale
    assert C.judge("ok", good, o)[1] == []
    bad = ref.clone()
    bad[1, 0] += 2e-6 * 4.1 * C.U    # 4.1 u of the small row; a global max-abs bar would not see 1e-11 beside 2.0
    fails = C.judge("small row", bad, o)[1]
    assert len(fails) == 1 and "[b]" in fails[0]
    assert C.judge("first row", ref + torch.tensor([[2.0 * 4.1 * C.U, 0.0], [0, 0], [0, 0]], dtype=torch.float64), o)[1]
    bad = ref.clone()
    bad[2, 1] = 1e-30                # a zero row must be exactly zero
    assert len(C.judge("zero row", bad, o)[1]) == 1
    bad = ref.clone()
    bad[0, 1] = math.nan
    assert len(C.judge("nan", bad, o)[1]) == 1
    six = ref + torch.tensor([[2.0 * 6 * C.U, 0.0], [0, 0], [0, 0]], dtype=torch.float64)
    term = torch.tensor([[2.0 * 2.5 * C.U, 0.0], [0, 0], [0, 0]], dtype=torch.float64)   # an absolute allowance on that one element
    assert C.judge("term", six, o, term=term)[1] == [] and len(C.judge("term elsewhere", six, o, term=term.flip(1))[1]) == 1
    # E_t is shared by the rows of a group: the lucky second row takes the first row's bar
    o2 = C.out(ref[:2], yard[:2] + torch.tensor([[20 * C.U, 0.0], [0.0, 0.0]], dtype=torch.float64), ["a", "a"])
    shifted = ref[:2].clone()
    shifted[1, 1] += 2e-6 * 30 * C.U
    assert C.judge("group", shifted, o2)[1] == []


def _ce_gradient_fp32(logits, labels, weight, sound):
    """The criterion kernel's arithmetic in fp32 on the CPU: the row gradient through lse = m + log(sum) (the form the kernel had) or
    through (x - m) - log(sum) (the form it has now)."""
    B = logits.shape[0]
    m = logits.amax(1, keepdim=True)
    log_sum = torch.exp(logits - m).sum(1, keepdim=True).log()
    p = torch.exp((logits - m) - log_sum) if sound else torch.exp(logits - (m + log_sum))
    onehot = torch.zeros_like(logits).scatter_(1, labels[:, None], 1.0)
    return (p - onehot) * torch.tensor(weight / B, dtype=torch.float32)


@pytest.mark.parametrize("B,K", C.CE_SHAPES)
def test_cross_entropy_gradient_through_the_rounded_lse_misses_the_bar(B, K):
    """... at every shape from logit scale 30 on, and from 8 on once a row has 174 classes or more (at K = 5 the scale-8 row stays at 0.85 of the bar)."""
    worst = {}
    for variant in (0, 1):
        case = C.cross_entropy_case(B, K, variant, 1.0)
        o = case["outs"]["gradient"]
        assert C.judge(f"cpu emulation, (x - m) - log sum, B={B} K={K}", _ce_gradient_fp32(case["logits"], case["labels"], 1.0, True), o)[1] == []
        e_k, _ = C.row_errors(_ce_gradient_fp32(case["logits"], case["labels"], 1.0, False), o.ref)
        e_t = C.yardstick(o)
        for e, g in zip(e_k.tolist(), o.group):
            s = float(g.split()[1])
            worst[s] = max(worst.get(s, 0.0), e / (C.MARGIN * max(e_t[g], C.U)))
    print(f"[scale] cpu emulation, x - lse, B={B} K={K}: share of the bar by logit scale {worst}")
    assert all(worst[s] > 1.0 for s in worst if s >= (8.0 if K >= 174 else 30.0)) and all(worst[s] < 1.0 for s in worst if s <= 1.0)


def test_adamw_layout_has_an_unaligned_parameter_and_a_two_chunk_parameter():
    p_off, f_off, total, chunks = C.opt_layout()
    assert any(o % 4 for o in p_off) and all(o % 4 == 0 for o in f_off) and total % 4 == 0
    assert sum(1 for i, _, _ in chunks if i == len(C.OPT_SIZES) - 1) == 2 and sum(n for _, _, n in chunks) == sum(C.OPT_SIZES)
    assert set(C.OPT_GRAD_SCALES) == {1e-12, 1e-6, 1e-3, 1.0, 1e3} and set(C.OPT_PARAM_SCALES) == {1e-3, 1.0, 1e2} and set(C.OPT_DECAYS) == {0.0, 1e-2}
