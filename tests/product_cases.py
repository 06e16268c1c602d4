"""Cases, fp64 references and yardsticks that hold the GEMM and Conv3d products to fp32 error off the unit scale: tests/test_product_scale_gpu.py
runs every route a product can take on them, tests/test_product_scale_cpu.py holds THEM to their own conditions and shows on an emulation
that the bar can fail.  Plain torch on the CPU, no package import, no GPU.

The metric is the one of tests/scale_cases.py (u = 2^-24, margin 4, a block of exact zeros must stay exactly zero; out / judge /
conditions / row_errors are reused), with these choices for a product:
  * block: the unit judged on its own scale is one output row within one group of 64 columns that share a weight / bias regime: an
    (M, N) output is compared as (M * N / 64, 64) rows.  Conv3d: one output channel of one sample.
  * group: (x scale of the row, column regime[, add-source regime]).  Rows of different x scale never share a group: in a mixed group
    the unit-scale rows set the yardstick and hide the bias-dominated ones.
  * yardstick of a group: max(E_t, E_c, u).  E_t: torch's own fp32 op on the same fp32 inputs on the CPU (F.linear, @, F.conv3d +
    F.batch_norm).  E_c: an in-order fp32 chain from zero with one rounding per product, bias / add-source added once afterwards
    (`chain`).  The second yardstick is needed because torch's blocked CPU sum is 3 - 6 x more accurate than ANY in-order chain from
    K = 768 on (a healthy chain that rounds once per four products reaches 4.1 x E_t at K = 3072); both are independent of the code
    under test.

Inputs: rows of x at the scales X_SCALES, interleaved (row i has X_SCALES[i % 4]) so that every tile holds all four; N is a whole
number of 64-column regimes (weight std, bias std) of REGIMES; with ReLU a further regime RELU_ZERO (bias exactly -30, small weights)
whose reference is identically zero, so the result must be exactly zero.  Its weights have the std 4e-3 / sqrt(K) (5e-4 at K = 64), not
a flat 1e-3: at x scale 1e3 a weight std of 1e-3 gives sums of std sqrt(K), up to 55, which cross the -30 — the block is then no zero
block but a cancellation on which torch itself is lost (E_t = 400 u at K = 3072); with 4e-3 / sqrt(K) the sums have std 4 at x scale
1e3 and -30 is 7.5 sigma away at every row.  The add-source R comes in two regimes by row, 1e3 x and 1e-3 x the
scale of the block it is added to; no cancelling R: torch itself is lost there (the E <= 256 u condition).
"""
import functools

import torch
import torch.nn.functional as F

import scale_cases as SC

ACT_NONE, ACT_GELU, ACT_RELU = 0, 1, 2
BLOCK = 64
X_SCALES = (1e-3, 0.03, 1.0, 1e3)
REGIMES = ((0.03, 0.0), (0.03, 0.1), (1e-3, 1.0), (30.0, 1e-3), (1.0, 30.0))   # (weight std, bias std) of a group of 64 columns
RELU_ZERO = (None, -30.0)                                                        # weights of std 4e-3 / sqrt(K), every bias exactly -30
GELU_REGIMES = ((0.03, 0.1), (0.03, 0.1))                                        # a whole 128-column tile of the one regime GELU is run on
R_FACTORS = (1e3, 1e-3)
K_STEPS = (64, 768, 3072)    # 2, 24 and 96 k-steps of 32
K_ANY = 100                  # no multiple of 32: the compatibility kernel
BIAS_DOMINATED = ((1e-3, 1.0), (1.0, 30.0))


def chain(x, w, start=None, per=1):
    """x (M, K) · w (N, K)ᵀ as an in-order fp32 accumulation along k: `per` exact products join the accumulator per rounding (1: the
    second yardstick; 4: the emulation of a matrix-core step); start (N,): the accumulators' initial value (None: zero)."""
    M, K = x.shape
    acc = torch.zeros(M, w.shape[0]) if start is None else start.float().expand(M, -1).clone()
    xd, wd = x.double(), w.double()
    for k in range(0, K, per):
        acc = (acc.double() + xd[:, k:k + per] @ wd[:, k:k + per].T).float()
    return acc


def finish(acc, bias, act, res):
    """What follows the sum, in the dtype of acc: + bias, the activation, + add-source."""
    v = acc if bias is None else acc + bias.to(acc.dtype)
    if act == ACT_GELU:
        v = F.gelu(v)
    elif act == ACT_RELU:
        v = v.relu()
    return v if res is None else v + res.to(acc.dtype)


def regimes_of(act, kind):
    if kind == "gelu":
        return GELU_REGIMES
    return REGIMES + ((RELU_ZERO,) if act == ACT_RELU else ())


def _regime_name(r, with_bias):
    if r == RELU_ZERO:
        return "w 4e-3/sqrt(K) b = -30"
    return f"w {r[0]:g} b {r[1]:g}" if with_bias else f"w {r[0]:g}"


@functools.lru_cache(maxsize=None)
def linear_case(M, K, act=ACT_NONE, with_res=False, with_bias=True, kind="full"):
    """y (M, N) = act(x wᵀ + b) (+ R): the forward of nn.Linear, and with with_bias = False and R the input gradient dX = dY · W
    (x is dY, w is Wᵀ).  -> x (M, K), w (N, K), bias (N,) or None, res (M, N) or None and the output "y" as blocks."""
    regs = regimes_of(act, kind)
    N = BLOCK * len(regs)
    g = SC._gen("product", M, K, act, with_res, with_bias, kind)
    x = torch.randn(M, K, generator=g) * torch.tensor([X_SCALES[i % 4] for i in range(M)])[:, None]
    w = torch.randn(N, K, generator=g) * torch.tensor([4e-3 / K ** 0.5 if r == RELU_ZERO else r[0] for r in regs]).repeat_interleave(BLOCK)[:, None]
    bias = None
    if with_bias:
        bias = torch.randn(N, generator=g) * torch.tensor([r[1] for r in regs]).repeat_interleave(BLOCK)
        for j, r in enumerate(regs):
            if r == RELU_ZERO:
                bias[j * BLOCK:(j + 1) * BLOCK] = r[1]
    pre = finish(x.double() @ w.double().T, bias, act, None)
    res = None
    if with_res:  # 1e3 x / 1e-3 x the scale of the block it joins, by row
        block_scale = pre.reshape(M, len(regs), BLOCK).abs().amax(2).repeat_interleave(BLOCK, 1)
        factor = torch.tensor([R_FACTORS[(i // 4) % 2] for i in range(M)])[:, None]
        res = (torch.randn(M, N, generator=g).double() * factor * block_scale).float()
    ref = pre if res is None else pre + res.double()
    yard = finish(F.linear(x, w), bias, act, res)
    yard2 = finish(chain(x, w), bias, act, res)
    group = []
    for i in range(M):
        for r in regs:
            group.append(f"x {X_SCALES[i % 4]:g} | {_regime_name(r, with_bias)}" + (f" | R {R_FACTORS[(i // 4) % 2]:g}x" if with_res else ""))
    n_rows = M * len(regs)
    return {"x": x, "w": w, "bias": bias, "res": res, "act": act, "regimes": regs,
            "outs": {"y": SC.out(SC.rows(ref, n_rows), yard, group, yard2)}}


def emulate(case, bias_first, per=4):
    """The forward of `case` as a matrix-core kernel sums it: fp32 accumulators, one rounding per `per` products; the bias as the
    accumulators' initial value (the form the whole-tile kernels had) or added once after the sum."""
    if bias_first and case["bias"] is not None:
        return finish(chain(case["x"], case["w"], start=case["bias"], per=per), None, case["act"], case["res"])
    return finish(chain(case["x"], case["w"], per=per), case["bias"], case["act"], case["res"])


DY_SCALES = (1e-3, 1.0, 1e3)


@functools.lru_cache(maxsize=None)
def weight_grad_case(rows, n_out=260, k_in=128):
    """dW (n_out, k_in) = dYᵀ · X + G0: the contraction runs over `rows` rows of the four x scales (interleaved), column m of dY has
    the scale DY_SCALES[m % 3], and G0 is 1e3 x (even 64-column groups) or 1e-3 x (odd ones) the scale of the update's block.  The chain
    yardstick runs along the rows.  Group: (dY scale, G0 regime)."""
    g = SC._gen("product dW", rows, n_out, k_in)
    x = torch.randn(rows, k_in, generator=g) * torch.tensor([X_SCALES[i % 4] for i in range(rows)])[:, None]
    dy = torch.randn(rows, n_out, generator=g) * torch.tensor([DY_SCALES[m % 3] for m in range(n_out)])[None, :]
    upd = dy.double().T @ x.double()
    nb = k_in // BLOCK
    block_scale = upd.reshape(n_out, nb, BLOCK).abs().amax(2).repeat_interleave(BLOCK, 1)
    factor = torch.tensor([R_FACTORS[j % 2] for j in range(nb)]).repeat_interleave(BLOCK)[None, :]
    g0 = (torch.randn(n_out, k_in, generator=g).double() * factor * block_scale).float()
    ref = upd + g0.double()
    yard = dy.T @ x + g0
    yard2 = chain(dy.T.contiguous(), x.T.contiguous()) + g0
    group = [f"dY {DY_SCALES[m % 3]:g} | G0 {R_FACTORS[j % 2]:g}x" for m in range(n_out) for j in range(nb)]
    return {"x": x, "dy": dy, "g0": g0, "outs": {"dW": SC.out(SC.rows(ref, n_out * nb), yard, group, yard2)}}


# ---- Conv3d + BatchNorm (+ residual) (+ ReLU) ------------------------------------------------------------------------------------------
# (B, Cin, T, H, W, Cout, kernel, stride, pad, residual, relu, n_split): three of the cases of tests/test_r3d_gpu.py (which asserts the match)
CONV_SHAPES = {
    "3x3x3_s1_odd_cout": (2, 64, 4, 7, 7, 96, (3, 3, 3), (1, 1, 1), (1, 1, 1), False, True, 1),          # K = 1728
    "1x1x1_s1_residual": (3, 128, 3, 5, 7, 200, (1, 1, 1), (1, 1, 1), (0, 0, 0), True, True, 1),
    "with_split5_uneven_3x3x3": (1, 128, 3, 4, 5, 96, (3, 3, 3), (1, 1, 1), (1, 1, 1), True, False, 5),   # explicit split-K
}
BN_EPS = 1e-5
# channel regimes, channel c has CONV_REGIMES[c % 7]: (name, gamma, running_var, |beta| scale or the exact beta)
CONV_REGIMES = (
    ("BN scale 1e-3", 1.0, 1e6 - BN_EPS, 0.1),
    ("BN scale 1", 1.0, 1.0 - BN_EPS, 0.1),
    ("BN scale 1e3", 2e-5 ** 0.5 * 1e3, 1e-5, 0.1),
    ("negative gamma", -1.0, 1.0 - BN_EPS, 0.1),
    ("gamma exactly 0", 0.0, 1.0 - BN_EPS, 0.1),
    ("shift-dominated, beta 30", 1.0, 1.0 - BN_EPS, 30.0),
    ("beta = -30 under BN scale 1e-3", 1.0, 1e6 - BN_EPS, -30.0),
)


def unfold3d(x, k, s, p):
    """(B, C, T, H, W) -> (B * To * Ho * Wo, C * kt * kh * kw): the rows a convolution contracts with weight.reshape(Cout, -1)."""
    x = F.pad(x, (p[2], p[2], p[1], p[1], p[0], p[0]))
    u = x.unfold(2, k[0], s[0]).unfold(3, k[1], s[1]).unfold(4, k[2], s[2])   # (B, C, To, Ho, Wo, kt, kh, kw)
    B, C, To, Ho, Wo = u.shape[:5]
    return u.permute(0, 2, 3, 4, 1, 5, 6, 7).reshape(B * To * Ho * Wo, -1), (To, Ho, Wo)


@functools.lru_cache(maxsize=None)
def conv_case(name):
    """relu(BN(conv3d(x, w)) + residual) with the flags of the shape; the input is relu'd as in tests/test_r3d_gpu.py.  Block: one
    output channel of one sample; group: the channel's regime.  With ReLU (and whatever the residual) the last regime is identically
    zero; gamma exactly 0 gives the shift, then residual / ReLU."""
    B, Ci, T, H, W, Co, k, s, p, with_res, relu, n_split = CONV_SHAPES[name]
    g = SC._gen("product conv", name)
    x = torch.randn(B, Ci, T, H, W, generator=g).relu_()
    fan = Ci * k[0] * k[1] * k[2]
    w = torch.randn(Co, Ci, *k, generator=g) * (2.0 / fan) ** 0.5
    regs = [CONV_REGIMES[c % len(CONV_REGIMES)] for c in range(Co)]
    gamma = torch.tensor([r[1] for r in regs], dtype=torch.float32)
    var = torch.tensor([r[2] for r in regs], dtype=torch.float32)
    beta = torch.tensor([r[3] for r in regs], dtype=torch.float32)
    rnd = torch.randn(Co, generator=g)
    beta = torch.where(beta.abs() < 1.0, beta * rnd, beta * torch.where(beta > 0, rnd.sign(), torch.ones(Co)))  # |beta| = 30 of either sign; -30 exactly
    mean = 0.1 * torch.randn(Co, generator=g)
    cols, (To, Ho, Wo) = unfold3d(x, k, s, p)
    res = torch.randn(B, Co, To, Ho, Wo, generator=g) if with_res else None

    def tail(conv, dt):   # BatchNorm as torch writes it, residual, ReLU
        v = (conv - mean.to(dt).view(1, -1, 1, 1, 1)) * (gamma.to(dt) / torch.sqrt(var.to(dt) + BN_EPS)).view(1, -1, 1, 1, 1) + beta.to(dt).view(1, -1, 1, 1, 1)
        if res is not None:
            v = v + res.to(dt)
        return v.relu() if relu else v

    ref = tail(F.conv3d(x.double(), w.double(), stride=s, padding=p), torch.float64)
    yard = F.batch_norm(F.conv3d(x, w, stride=s, padding=p), mean, var, gamma, beta, False, 0.0, BN_EPS)
    if res is not None:
        yard = yard + res
    if relu:
        yard = yard.relu()
    conv_chain = chain(cols, w.reshape(Co, -1)).reshape(B, To, Ho, Wo, Co).permute(0, 4, 1, 2, 3)
    yard2 = tail(conv_chain, torch.float32)
    group = [regs[c][0] for _ in range(B) for c in range(Co)]
    return {"x": x, "w": w, "bn": [gamma, beta, mean, var], "res": res, "relu": relu, "n_split": n_split, "shape": CONV_SHAPES[name],
            "outs": {"y": SC.out(SC.rows(ref, B * Co), yard, group, yard2)}}


# ---- what the GPU test runs, for the CPU test to hold to the conditions -------------------------------------------------------------
M_MAIN, M_SKINNY = 260, 8            # 260: a second row tile of 4 rows (256 x 128 tiles), ragged tiles of 128 / 64 / 32 rows
DW_ROWS = (96, 2048)
FORWARD_CASES = (
    [(M_MAIN, K, act, False, True, "full") for K in K_STEPS for act in (ACT_NONE, ACT_RELU)]
    + [(M_MAIN, K, ACT_GELU, False, True, "gelu") for K in K_STEPS]
    + [(M_MAIN, K, ACT_NONE, True, True, "full") for K in K_STEPS]          # bias + residual (linear_small)
    + [(M_SKINNY, K, ACT_NONE, False, True, "full") for K in K_STEPS]
    + [(M_MAIN, K_ANY, act, False, True, "full") for act in (ACT_NONE, ACT_RELU)]
)
BACKWARD_CASES = [(M_MAIN, K, ACT_NONE, True, False, "full") for K in K_STEPS]   # dX = dY · W + R
ALL_CASES = ([("linear", linear_case, a) for a in FORWARD_CASES] + [("input gradient", linear_case, a) for a in BACKWARD_CASES]
             + [("weight gradient", weight_grad_case, (r,)) for r in DW_ROWS] + [("conv3d", conv_case, (n,)) for n in sorted(CONV_SHAPES)])
