"""The softmax, LayerNorm, GELU, criterion and optimizer kernels off the unit scale, held to torch's own fp32 error row by row.

The op-level tests beside this one draw their inputs from about [-1, 1] and compare against fp64 with a fixed max-abs bar, where a lazy
formulation (no stabilised softmax, a one-pass variance, exp(x - lse), a clamped erf) passes and a small row inside a batch of large ones
is compared at the large rows' scale.  Here every case comes from tests/scale_cases.py (whose docstring states the metric): rows of very
different magnitudes in one batch, each row judged on its own scale, the bar 4 * max(E_t, u) measured from torch's fp32 implementation on
the same inputs; tests/test_off_unit_scale_cpu.py holds the cases to the conditions that make that bar mean something.  Kernels are
reached through pkg.ops.* and the C ABI, as in tests/test_partition_regimes_gpu.py.  Every case prints e_k / u, E_t / u and their ratio
per scale group (profiles/off_unit_scale.md keeps the table of one run).  The products themselves — every GEMM route and the Conv3d forward — are
held to the same rule, block by block, in tests/test_product_scale_gpu.py (profiles/product_scale.md).

No kernel needed an analytic term (scale_cases.judge can take one off element by element for a documented approximation of a kernel, such
as the stated 1.1e-7 of the epilogue's erf fit): every case holds the plain bar.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import scale_cases as SC

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.fixture(scope="module")
def lib(pkg):
    return pkg._lib.load()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _hold(tag, results, case, terms=None):
    """results: {output name: what the kernel gave}; every output of the case must be among them."""
    assert set(results) == set(case["outs"]), (sorted(results), sorted(case["outs"]))
    fails = []
    for name, got in results.items():
        fails += SC.judge(f"{tag} {name}", got, case["outs"][name], term=(terms or {}).get(name))[1]
    assert not fails, "\n".join(fails)


# ---- stlt_loss_fwd_bwd -------------------------------------------------------------------------------------------------------------
def _loss(pkg, lib, case):
    logits, labels = case["logits"].to(DEV), case["labels"].to(DEV)
    B, K = logits.shape
    sc, loss, dl = torch.empty(B, device=DEV), torch.empty(1, device=DEV), torch.empty(B, K, device=DEV)
    pkg._lib.check(lib.stlt_loss_fwd_bwd(logits.data_ptr(), labels.data_ptr(), case["kind"], B, K, case["weight"], sc.data_ptr(), loss.data_ptr(), dl.data_ptr(), _stream()),
                   "stlt_loss_fwd_bwd")
    return {"gradient": dl, "loss": loss}


@pytest.mark.parametrize("weight", SC.WEIGHTS)
@pytest.mark.parametrize("variant", [0, 1])
@pytest.mark.parametrize("B,K", SC.CE_SHAPES)
def test_cross_entropy_rows_of_every_logit_scale(pkg, lib, B, K, variant, weight):
    """Logit rows of scale 1e-3 .. 1000 in one batch, the label on the arg-max (p_y - 1 cancels) or on the arg-min.  A gradient written as
    exp(x - (m + log sum)) inherits ulp(m) / 2 as a relative error of every probability and misses these bars from scale 8 on (by 3x at
    30, 700x at 1000); K = 300 takes the second trip of the class loop."""
    case = SC.cross_entropy_case(B, K, variant, weight)
    _hold(f"cross entropy B={B} K={K} variant={variant} weight={weight}", _loss(pkg, lib, case), case)


@pytest.mark.parametrize("weight", SC.WEIGHTS)
def test_cross_entropy_ignored_row_among_off_scale_rows(pkg, lib, weight):
    """A label of -100 on the scale-8 row: its gradient row is exactly zero and the other rows, already written with 1 / B, are rescaled."""
    case = SC.cross_entropy_case(6, 174, 0, weight, 2)
    got = _loss(pkg, lib, case)
    _hold(f"cross entropy with an ignored row weight={weight}", got, case)
    assert got["gradient"][2].abs().max().item() == 0.0


@pytest.mark.parametrize("weight", SC.WEIGHTS)
@pytest.mark.parametrize("B,K", SC.BCE_SHAPES)
def test_bce_rows_of_every_logit_scale(pkg, lib, B, K, weight):
    """Scale 100: exp(-v) overflows fp32 for v < -88; the gradient there is 0 - t, not NaN."""
    case = SC.bce_case(B, K, weight)
    got = _loss(pkg, lib, case)
    assert torch.isfinite(got["gradient"]).all() and torch.isfinite(got["loss"]).all()
    _hold(f"bce B={B} K={K} weight={weight}", got, case)


# ---- stlt_grad_norm, stlt_adamw_step -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("clipping", [True, False])
@pytest.mark.parametrize("scale", SC.NORM_SCALES)
@pytest.mark.parametrize("n", SC.NORM_SIZES)
def test_grad_norm_of_every_magnitude(pkg, lib, n, scale, clipping):
    """Gradients of 1e-15 .. 1e15 (the squares stay normal numbers); 5: the vector and a tail; 4099 and 70001: several blocks and a tail."""
    case = SC.norm_case(n, scale, clipping)
    g, sc, res = case["g"].to(DEV), torch.empty(1024, device=DEV), torch.empty(2, device=DEV)
    pkg._lib.check(lib.stlt_grad_norm(g.data_ptr(), n, case["max_norm"], sc.data_ptr(), res.data_ptr(), _stream()), "stlt_grad_norm")
    _hold(f"grad_norm n={n} scale={scale:g} clipping={int(clipping)}", {"norm": res[0], "coefficient": res[1]}, case)


@pytest.mark.parametrize("late", [False, True])
@pytest.mark.parametrize("clipping", [True, False])
@pytest.mark.parametrize("lr", SC.OPT_LRS)
def test_adamw_parameters_of_every_scale(pkg, lib, lr, clipping, late):
    """Six parameters with their own gradient scale (1e-12 .. 1e3), value scale and weight decay in one table: three steps from zero
    moments, or one step at step 100000 from given moments.  The parameters lie back to back (two of them off the 16-byte grid: the
    one-element path), the last spans two chunks."""
    case = SC.adamw_case(lr, clipping, late)
    p_off, f_off, total, chunks = SC.opt_layout()
    sizes = SC.OPT_SIZES
    params = torch.zeros(sum(sizes), device=DEV)
    m, v = torch.zeros(total, device=DEV), torch.zeros(total, device=DEV)
    for i, n in enumerate(sizes):
        params[p_off[i]:p_off[i] + n] = case["p0"][i].to(DEV)
        m[f_off[i]:f_off[i] + n] = case["m0"][i].to(DEV)
        v[f_off[i]:f_off[i] + n] = case["v0"][i].to(DEV)
    table = np.zeros(len(chunks), dtype=np.dtype([("param", "<u8"), ("off", "<i8"), ("n", "<i4"), ("wd", "<f4")]))
    assert table.dtype.itemsize == C.sizeof(pkg._lib.OptChunk)
    for j, (i, c0, n) in enumerate(chunks):
        table[j] = (params.data_ptr() + 4 * (p_off[i] + c0), f_off[i] + c0, n, SC.OPT_DECAYS[i])
    assert any(int(row["param"]) % 16 for row in table) and any(int(row["param"]) % 16 == 0 for row in table)
    table_dev = torch.from_numpy(table.view(np.uint8).copy()).to(DEV)
    sc, res = torch.empty(1024, device=DEV), torch.empty(2, device=DEV)
    got = {}
    for step, grads, max_norm in zip(case["steps"], case["grads"], case["max_norms"]):
        flat = torch.zeros(total, device=DEV)
        for i, n in enumerate(sizes):
            flat[f_off[i]:f_off[i] + n] = grads[i].to(DEV)
        pkg._lib.check(lib.stlt_grad_norm(flat.data_ptr(), total, max_norm, sc.data_ptr(), res.data_ptr(), _stream()), "stlt_grad_norm")
        pkg._lib.check(lib.stlt_adamw_step(table_dev.data_ptr(), len(chunks), flat.data_ptr(), m.data_ptr(), v.data_ptr(), res.data_ptr(), lr, SC.BETAS[0], SC.BETAS[1],
                                           SC.ADAM_EPS, step, _stream()), "stlt_adamw_step")
        for i, n in enumerate(sizes):
            got[f"step {step} parameters [{i}]"] = params[p_off[i]:p_off[i] + n].clone()
            got[f"step {step} exp_avg [{i}]"] = m[f_off[i]:f_off[i] + n].clone()
            got[f"step {step} exp_avg_sq [{i}]"] = v[f_off[i]:f_off[i] + n].clone()
        got[f"step {step} norm"], got[f"step {step} coefficient"] = res[0].clone(), res[1].clone()
    _hold(f"adamw lr={lr:g} clipping={int(clipping)} {'step 100000' if late else 'steps 1-3'}", got, case)


# ---- LayerNorm ---------------------------------------------------------------------------------------------------------------------
def _ln_bwd(pkg, lib, case, M, d):
    dev = torch.device(DEV, torch.cuda.current_device())
    nbytes = int(lib.stlt_add_layernorm_bwd_scratch_bytes(d))
    sc = pkg.ops._scratch(nbytes, dev)
    x, r, w, dy = case["x"].to(DEV), None if case["res"] is None else case["res"].to(DEV), case["w"].to(DEV), case["dy"].to(DEV)
    ds, gw, gb = torch.empty(M, d, device=DEV), torch.zeros(d, device=DEV), torch.zeros(d, device=DEV)
    pkg._lib.check(lib.stlt_add_layernorm_bwd(dy.data_ptr(), x.data_ptr(), None if r is None else r.data_ptr(), w.data_ptr(), case["eps"], M, d, ds.data_ptr(), gw.data_ptr(),
                                              gb.data_ptr(), sc.data_ptr(), nbytes, _stream()), "stlt_add_layernorm_bwd")
    return ds, gw, gb


@pytest.mark.parametrize("with_res", [True, False])
@pytest.mark.parametrize("eps", SC.LN_EPS)
@pytest.mark.parametrize("d", SC.LN_D)
def test_layernorm_rows_of_every_mean_and_spread(pkg, lib, d, eps, with_res):
    """ops.add_layernorm and stlt_add_layernorm_bwd's input gradient: rows with mean / spread 0, 10, 100 at spreads 1e-4, 1, 1e4, two
    constant rows and two rows whose residual cancels x, gradient rows of scales 1e-4, 1, 1e4.  A one-pass variance E[x^2] - mean^2 loses
    the rows at mean / spread 100 entirely; d = 260: a second vector group of one lane; 1028: the wide backward kernel."""
    case = SC.layernorm_case(d, eps, with_res)
    M = case["x"].shape[0]
    fwd = pkg.ops.add_layernorm(case["x"].to(DEV), None if case["res"] is None else case["res"].to(DEV), case["w"].to(DEV), case["b"].to(DEV), eps)
    ds, _, _ = _ln_bwd(pkg, lib, case, M, d)
    _hold(f"layernorm d={d} eps={eps:g} res={int(with_res)}", {"forward": fwd, "ds": ds}, case)


@pytest.mark.parametrize("eps", SC.LN_EPS)
@pytest.mark.parametrize("d", SC.LN_D)
def test_layernorm_scale_and_shift_gradients_one_scale_per_batch(pkg, lib, d, eps):
    for combo in range(len(SC.LN_COMBOS)):
        case = SC.layernorm_param_grad_case(d, eps, combo)
        _, gw, gb = _ln_bwd(pkg, lib, case, case["x"].shape[0], d)
        _hold(f"layernorm parameter gradients d={d} eps={eps:g}", {"g_w": gw, "g_b": gb}, case)


@pytest.mark.parametrize("d", SC.LN_D)
def test_embedding_layernorms_at_eps_1e_12(pkg, d):
    """ops.frames_embed and ops.embed (with and without scores) at the embeddings' eps = 1e-12 on the same rows."""
    case = SC.frames_embed_case(d)
    got = pkg.ops.frames_embed(case["spatial"].to(DEV), case["frame_types"].to(DEV), case["pos"].to(DEV), case["type"].to(DEV), case["w"].to(DEV), case["b"].to(DEV), case["eps"])
    _hold(f"frames_embed d={d}", {"forward": got}, case)
    for with_scores in (True, False):
        case = SC.embed_case(d, with_scores)
        t = {k: (None if case[k] is None else case[k].to(DEV)) for k in ("categories", "boxes", "scores", "table", "box_w", "box_b", "score_w", "score_b", "w", "b")}
        got = pkg.ops.embed(t["categories"], t["boxes"], t["scores"], t["table"], t["box_w"], t["box_b"], t["score_w"] if with_scores else None,
                            t["score_b"] if with_scores else None, t["w"], t["b"], case["eps"])
        _hold(f"embed d={d} scores={int(with_scores)}", {"forward": got}, case)


# ---- GELU --------------------------------------------------------------------------------------------------------------------------
def _padded(x, multiple):
    pad = (-x.numel()) % multiple
    return torch.cat([x, x[-1:].expand(pad)]) if pad else x


def test_gelu_kernels_in_every_binade(pkg, lib):
    """stlt_gelu_fwd / stlt_gelu_bwd (erff): 64 points per binade from 2^-30 to 2^6, both signs, the zeros, subnormals, the fit's clamp
    point, +-8, +-20, +-1e4, +-1e30 and +-FLT_MAX, each binade judged at its own scale."""
    case = SC.gelu_case()
    n = case["x"].numel()
    u = _padded(case["x"], 4).to(DEV)
    h, du, dh = torch.empty_like(u), torch.empty_like(u), torch.ones_like(u)
    pkg._lib.check(lib.stlt_gelu_fwd(u.data_ptr(), h.data_ptr(), u.numel(), _stream()), "stlt_gelu_fwd")
    pkg._lib.check(lib.stlt_gelu_bwd(dh.data_ptr(), u.data_ptr(), du.data_ptr(), u.numel(), _stream()), "stlt_gelu_bwd")
    fails = SC.judge("gelu_fwd", SC.gelu_rows(case, h[:n]), SC.gelu_out(case, "fwd"))[1]
    fails += SC.judge("gelu_bwd", SC.gelu_rows(case, du[:n]), SC.gelu_out(case, "bwd"))[1]
    assert not fails, "\n".join(fails)


def test_gelu_epilogue_fit_in_every_binade(pkg):
    """The fitted GELU of the product epilogue, reached through ops.linear with one-hot weight rows and a zero bias: the same call
    without the activation must hand every point back bit for bit (a zero may change its sign: -0 * 1 + 0 * x is +0), then the reference
    is gelu at the points.  csrc/common.h states an absolute error of 1.1e-7 for the erf fit, which would allow a term of 0.5 |x| 1.1e-7;
    the fit keeps the plain bar (worst ratio 1.45 on the GPU), so none is taken."""
    case = SC.gelu_case()
    n = case["x"].numel()
    x = _padded(case["x"], 64).reshape(-1, 64).to(DEV)
    w, b = torch.eye(64, device=DEV), torch.zeros(64, device=DEV)
    same = pkg.ops.linear(x, w, b, pkg._lib.ACT_NONE)
    nonzero = x != 0
    assert torch.equal(same[nonzero].view(torch.int32), x[nonzero].view(torch.int32)) and bool((same[~nonzero] == 0).all())
    got = pkg.ops.linear(x, w, b, pkg._lib.ACT_GELU).reshape(-1)[:n]
    fails = SC.judge("gelu epilogue", SC.gelu_rows(case, got), SC.gelu_out(case, "fwd"))[1]
    assert not fails, "\n".join(fails)


def test_gelu_epilogue_derivative_fit_in_every_binade(pkg):
    """gelu' of the hidden-gradient product's epilogue (gelu_grad_epilogue: the same erf fit and two v_exp_f32), reached through
    FfnBlockFn's backward on a block of one row whose pre-activations are the points (scale_cases.gelu_block_chunks): the block returns
    ds as dx and du as the first bias's gradient, so du_j / (ds[j % d] * alpha_j) is the kernel's gelu'(u_j).  The launch recorder shows
    that the product's epilogue took the derivative (no stand-alone gelu_bwd+colsum pass, whose gelu' is the erff one)."""
    case, d = SC.gelu_case(), 768
    n = case["x"].numel()
    v, du = torch.zeros(n), torch.zeros(n)
    g0 = torch.Generator().manual_seed(3)
    for pos, b1, w2, alpha in SC.gelu_block_chunks(case, d):
        host = (torch.randn(1, d, generator=g0), torch.zeros(4 * d, d), b1, w2, torch.zeros(d), 1 + 0.1 * torch.randn(d, generator=g0), 0.1 * torch.randn(d, generator=g0))
        leaves = [t.clone().to(DEV).requires_grad_(True) for t in host]
        out = pkg.ops.FfnBlockFn.apply(leaves[0], 1e-5, pkg._lib.ACT_GELU, True, 0.0, *leaves[1:])
        assert torch.isfinite(out).all()
        pkg.ops.prof_enable(True)
        try:
            pkg.ops.prof_launches()
            out.backward((torch.randn(1, d, generator=g0) * 2.0 ** 20).to(DEV))  # ds of order 1e6: ds * alpha stays a normal number at alpha = 2^-127
            torch.cuda.synchronize()
            notes = [r["note"] for r in pkg.ops.prof_launches()]
        finally:
            pkg.ops.prof_enable(False)
        assert not [x for x in notes if "gelu_bwd" in x], notes
        ds = leaves[0].grad.cpu().reshape(d)
        v[pos] = ds[torch.arange(4 * d) % d] * alpha          # exact: alpha is a power of two
        du[pos] = leaves[2].grad.cpu()
    assert bool((v.abs() >= 2.0 ** -126).all())
    fails = SC.judge("gelu epilogue derivative", SC.gelu_rows(case, du), SC.gelu_scaled_derivative_out(case, v))[1]
    assert not fails, "\n".join(fails)


# ---- attention ---------------------------------------------------------------------------------------------------------------------
def _packed(case):
    return torch.cat([case["q"], case["k"], case["v"]], -1).to(DEV)


@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("L", SC.ATTN_L)
def test_attention_sequences_of_every_score_scale(pkg, L, causal):
    """ops.attn_core, attn_probs (per head and averaged) and attn_core_bwd on sequences with score std 1e-3 .. 300, scores rising along
    the keys, and a fully masked sequence (exact zeros), 30 % of the keys masked; each (sequence, head) block judged on its own scale."""
    case = SC.attention_case(L, L, causal)
    qkv, kpm = _packed(case), case["kpm"].to(DEV)
    H = SC.ATTN_H
    got = {"ctx": SC.head_rows(pkg.ops.attn_core(qkv, kpm, causal, H)),
           "probabilities per head": pkg.ops.attn_probs(qkv, kpm, causal, H, per_head=True),
           "probabilities": pkg.ops.attn_probs(qkv, kpm, causal, H),
           "dqkv": SC.head_rows(pkg.ops.attn_core_bwd(qkv, case["dctx"].to(DEV), kpm, causal, H))}
    _hold(f"attention L={L} causal={int(causal)}", got, case)


def test_cross_attention_sequences_of_every_score_scale(pkg):
    """ops.attn_cross and attn_probs_cross: three queries over 70 keys."""
    case = SC.attention_case(3, 70, False)
    q, kv, kpm = case["q"].to(DEV), torch.cat([case["k"], case["v"]], -1).to(DEV), case["kpm"].to(DEV)
    H, d = SC.ATTN_H, case["q"].shape[-1]
    got = {"ctx": SC.head_rows(pkg.ops.attn_cross(q, kv, kpm, H)),
           "probabilities per head": pkg.ops.attn_probs_cross(q, kv[..., :d], kpm, False, H, per_head=True),
           "probabilities": pkg.ops.attn_probs_cross(q, kv[..., :d], kpm, False, H)}
    _hold("cross attention Lq=3 Lk=70", got, case)


@pytest.mark.parametrize("causal", [True, False])
@pytest.mark.parametrize("L", [5, 33])
def test_mhsa_fused_sequences_of_every_input_scale(pkg, L, causal):
    """ops.mhsa_fused, in-projection and attention in one kernel, on inputs of scale 0.03, 1.5 and 5.5 under a bias of 0.1.  At 0.03 the
    projected values are mostly bias: a projection that starts its accumulators from the bias and adds the d products to them one at a
    time (as the kernel did: 14.1 u here against a bar of 8.2 u) rounds every addition at the bias's magnitude and misses these rows."""
    case = SC.mhsa_case(L, causal)
    got = pkg.ops.mhsa_fused(case["x"].to(DEV), case["w"].to(DEV), case["b"].to(DEV), case["kpm"].to(DEV), SC.ATTN_H, causal=causal)
    _hold(f"mhsa_fused L={L} causal={int(causal)}", {"ctx": SC.head_rows(got)}, case)
