"""The cases of tests/product_cases.py held to their own conditions, without a GPU: every reference is finite, the blocks of an output
cover all of it, and the yardstick max(E_t, E_c) stays within 256 u in every group (past that torch itself is lost on the input and the
bar 4 * max(E_t, E_c, u) means nothing).  Then, on a CPU emulation of a matrix-core kernel (fp32 accumulators, one rounding per four
products), the two claims that make tests/test_product_scale_gpu.py worth running: a chain that starts from zero and adds the bias once
after the sum passes every group, and the same chain started from the bias (the form the whole-tile kernels had) misses the bar in the
groups whose output is mostly bias."""
import pytest
import torch

import product_cases as P
import scale_cases as SC


@pytest.mark.parametrize("name,make,args", P.ALL_CASES, ids=[f"{n}-{'-'.join(str(a) for a in args)}" for n, _, args in P.ALL_CASES])
def test_case_keeps_the_three_conditions(name, make, args):
    case = make(*args)
    bad = []
    for key, o in case["outs"].items():
        assert o.ref.dtype == torch.float64 and o.ref.dim() == 2 and len(o.group) == o.ref.shape[0] and o.yard2 is not None
        bad += [f"{key}: {b}" for b in SC.conditions(o)]
        e_t, e_c = SC.yardsticks(o)
        for g in e_t:
            print(f"[scale] {name} {args} {key} | {g} | E_t/u {e_t[g] / SC.U:.2f} | E_c/u {e_c[g] / SC.U:.2f}")
    assert not bad, "\n".join(bad)


def test_blocks_cover_every_element_and_hold_one_regime_each():
    case = P.linear_case(P.M_MAIN, 64, P.ACT_RELU)
    M, N = P.M_MAIN, P.BLOCK * len(case["regimes"])
    o = case["outs"]["y"]
    assert len(case["regimes"]) == 6 and o.ref.shape == (M * N // P.BLOCK, P.BLOCK) and o.ref.numel() == M * N
    t = torch.arange(M * N, dtype=torch.float64).reshape(M, N)
    blocks = SC.rows(t, M * N // P.BLOCK)
    assert sorted(blocks.reshape(-1).tolist()) == list(range(M * N))
    assert torch.equal(blocks[7], t[1, 64:128]) and o.group[7] == "x 0.03 | w 0.03 b 0.1"       # row 1, second column group
    # rows of different x scale never share a group, and every tile height used holds all four scales
    assert all(g.startswith(f"x {P.X_SCALES[(i // 6) % 4]:g} |") for i, g in enumerate(o.group))
    conv = P.conv_case("1x1x1_s1_residual")
    B, Co = conv["shape"][0], conv["shape"][5]
    assert conv["outs"]["y"].ref.shape[0] == B * Co and conv["outs"]["y"].ref.numel() == B * Co * 3 * 5 * 7
    assert set(conv["outs"]["y"].group) == {r[0] for r in P.CONV_REGIMES}
    dw = P.weight_grad_case(96)
    assert dw["outs"]["dW"].ref.numel() == 260 * 128


@pytest.mark.parametrize("K", P.K_STEPS + (P.K_ANY,))
def test_relu_regime_of_bias_minus_30_is_identically_zero(K):
    case = P.linear_case(P.M_MAIN, K, P.ACT_RELU)
    o = case["outs"]["y"]
    zero = o.ref.abs().amax(1) == 0
    for i, g in enumerate(o.group):
        assert bool(zero[i]) == g.endswith("b = -30"), g
    assert int(zero.sum()) == P.M_MAIN
    # ... and the metric demands exact zeros there
    wrong = o.ref.clone()
    wrong[int(torch.nonzero(zero)[0]), 3] = 1e-30
    assert len(SC.judge("zero block", wrong, o)[1]) == 1


def test_conv_zero_regime_and_gamma_zero():
    for name in sorted(P.CONV_SHAPES):
        case = P.conv_case(name)
        o = case["outs"]["y"]
        gamma, beta = case["bn"][0], case["bn"][1]
        Co = case["shape"][5]
        for r in range(o.ref.shape[0]):
            c = r % Co
            if o.group[r].startswith("beta = -30") and case["relu"]:
                assert float(o.ref[r].abs().max()) == 0.0
            if o.group[r] == "gamma exactly 0":
                assert float(gamma[c]) == 0.0
                if case["res"] is None:  # the shift alone, then ReLU
                    assert torch.equal(o.ref[r], torch.full_like(o.ref[r], max(float(beta[c].double()), 0.0) if case["relu"] else float(beta[c].double())))


def _bias_dominated(group):
    return any(group.endswith(f"w {w:g} b {b:g}") for w, b in P.BIAS_DOMINATED) and (group.startswith("x 0.001 |") or group.startswith("x 0.03 |"))


@pytest.mark.parametrize("act", [P.ACT_NONE, P.ACT_RELU])
@pytest.mark.parametrize("K", P.K_STEPS)
def test_chain_from_zero_passes_and_chain_from_the_bias_misses_the_bar(K, act):
    """The emulated kernel rounds once per four products.  From zero, bias added after the sum: every group passes.  From the bias: the K / 4
    additions round at the bias's magnitude, and the groups whose output is mostly bias — regimes (1e-3, 1) and (1, 30) at x scale <= 0.03 —
    miss the bar at K = 768 and 3072.  The failure is asserted from K = 768 on and only in those groups, and only where this module's own
    cases show at least 6 x the yardstick (1.5 x the bar): 14 - 21 x at K = 768, 10 - 43 x at K = 3072.  At K = 64 (16 additions) the
    bias-first chain sits at 4 - 7 x, on either side of the bar, and nothing is claimed; other groups whose output is mostly bias (x scale
    1e-3 under (0.03, 0.1)) miss as well and are printed, not asserted."""
    case = P.linear_case(P.M_MAIN, K, act)
    o = case["outs"]["y"]
    assert SC.judge(f"cpu emulation, from zero, K={K} act={act}", P.emulate(case, False), o)[1] == []
    e_k, _ = SC.row_errors(P.emulate(case, True), o.ref)
    yard = SC.yardstick(o)
    worst = {}
    for e, g in zip(e_k.tolist(), o.group):
        worst[g] = max(worst.get(g, 0.0), e / max(yard[g], SC.U))
    hit = {g: r for g, r in worst.items() if _bias_dominated(g)}
    print(f"[scale] cpu emulation, from the bias, K={K} act={act}: x the yardstick in the bias-dominated groups "
          + ", ".join(f"{g}: {r:.1f}" for g, r in hit.items()))
    print(f"[scale] ... and the largest elsewhere: {max(r for g, r in worst.items() if g not in hit):.2f}")
    assert len(hit) == 4
    if K >= 768:
        assert all(r >= 6.0 for r in hit.values()), hit
