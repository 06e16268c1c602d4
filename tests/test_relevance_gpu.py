"""Attention relevance on the GPU: the gradient-weighted probabilities kernel and the rollout kernel alone against fp64 inside guard bands,
and Stlt.forward_relevance against the fp64 restatement (tests/relevance_restated.py, which tests/test_relevance_cpu.py holds to the goldens
and to the closed form) — every target form, the per-layer maps, exact zeros, the op-level recomposition, refusals, graph capture, and that
the call leaves no state behind.  Every test prints its worst figure (profiles/attention_relevance_bench.md records them)."""
import ctypes as C
import functools
import sys

import numpy as np
import pytest
import torch

import attention_restated as AR
import guard_arena as GA
import relevance_restated as R
from guard_arena import Out
from test_relevance_cpu import MAPS, WHOLE_PATH_CASES, _heads, _rel, reference

pytestmark = pytest.mark.gpu
DEV = "cuda"
EINVAL = -1
OP_CAP = 1e-5       # the project's op-level gradient bound (tests/test_layout_gradients_gpu.py)
ROLLOUT_CAP = 1e-5  # every term of the chain is non-negative: no cancellation
# Whole path: max(2e-4, 4 f).  2e-4 is the bound tests/test_layout_gradients_gpu.py already holds this same sweep's dctx chain to; f is the
# fp32 floor of the restatement, measured by tests/test_relevance_cpu.py::test_fp32_floor_of_the_whole_path (largest figure over its cases and
# over repeated runs: 3.45e-7, cfg2p/top1 relevance); the factor 4 because the GPU sums in another order than torch's CPU fp32.
FP32_FLOOR = 3.45e-7
CAP = max(2e-4, 4 * FP32_FLOOR)
LOGIT_TOL = 1e-4


def _report(what, value):
    print(f"\n[relevance] {what}: {value}", file=sys.stderr)


def _to(batch):
    return {k: (v.to(DEV) if isinstance(v, torch.Tensor) else v) for k, v in batch.items()}


@pytest.fixture(scope="module")
def arena():
    a = GA.Arena(64 << 20, DEV)
    yield a
    del a
    torch.cuda.empty_cache()


# ---- the gradient-weighted probabilities kernel alone ----------------------------------------------------------------------------------
def _op_case(S, L, H, dh, seed):
    """qkv and dctx uniform in [-1, 1]; about 30 % of the keys padded with key 0 kept — and, when there is more than one sequence, the last
    sequence fully masked"""
    qkv = GA.rand(S, L, 3 * H * dh, seed=seed)
    dctx = GA.rand(S, L, H * dh, seed=seed + 1)
    kpm = torch.rand(S, L, generator=torch.Generator().manual_seed(100 + seed)) < 0.3
    kpm[:, 0] = False
    if S > 1:
        kpm[S - 1, :] = True
    return qkv, dctx, kpm


def _op_specs(qkv, dctx, kpm):
    S, L, _ = qkv.shape
    return {"qkv": (qkv.reshape(S * L, -1), "in"), "dctx": (dctx.reshape(S * L, -1), "in"), "kpm": (kpm.to(torch.uint8), "extent", 0),
            "abar": (Out((S * L, L)), "out")}


def _op_call(lib, S, L, H, dh, causal):
    return lambda o: lib.stlt_attn_grad_probs(o.qkv.ptr, o.dctx.ptr, o.kpm.ptr, causal, S, L, H, dh, o.abar.ptr, GA.stream())


@pytest.mark.parametrize("causal", [0, 1])
@pytest.mark.parametrize("H,dh", [(2, 64), (3, 16), (2, 20)])
@pytest.mark.parametrize("L", [1, 7, 16, 17, 33, 64, 65, 256])
def test_attn_grad_probs_vs_fp64_inside_guard_bands(pkg, arena, L, H, dh, causal):
    """S = 1 and 5.  Plain call == arena call == second call bit for bit, no byte outside abar changes and every element of it is written
    (GA.three_ways); <= OP_CAP of max|ref| against the restated formula in fp64; masked entries exactly 0."""
    lib = pkg._lib.load()
    worst = 0.0
    for S in (1, 5):
        qkv, dctx, kpm = _op_case(S, L, H, dh, seed=1000 * L + 10 * dh + S)
        got = GA.three_ways(lib, arena, _op_specs(qkv, dctx, kpm), _op_call(lib, S, L, H, dh, causal), ["abar"])["abar"].view(S, L, L)
        ref = R.attn_grad_probs(qkv.double(), dctx.double(), kpm, bool(causal), H)
        assert torch.isfinite(got).all() and (got >= 0).all()
        assert (got[AR.masked_entries(kpm, bool(causal))] == 0).all()
        if S > 1:
            assert (got[S - 1] == 0).all()  # the fully masked sequence: zeros, written
        assert ref.abs().max().item() > 0
        worst = max(worst, _rel(got, ref))
        assert worst <= OP_CAP, (S, L, H, dh, causal, worst)
    _report(f"attn_grad_probs L={L} H={H} dh={dh} causal={causal} worst err / max|ref|", f"{worst:.2e}")


def test_attn_grad_probs_refusals_leave_the_output_untouched(pkg, arena):
    """One refusal per rule: STLT_EINVAL, the message names the cause, nothing is launched.  A four-byte displacement is refused on the
    16-byte path (dh % 4 == 0) and accepted, with the aligned call's bits, at dh = 25."""
    lib = pkg._lib.load()
    S, L, H, dh = 3, 7, 2, 64
    qkv, dctx, kpm = _op_case(S, L, H, dh, seed=5)
    specs = _op_specs(qkv, dctx, kpm)
    for operand in ("qkv", "dctx"):
        assert GA.misaligned(lib, arena, specs, _op_call(lib, S, L, H, dh, 0), ["abar"], operand=operand, mis=4, refused_as=operand) is None
    arena.reset()
    A = {k: arena.place(s[0], s[1], band=(s[2] if len(s) > 2 else None), name=k) for k, s in specs.items()}
    q, g, k, a = (A[n].ptr for n in ("qkv", "dctx", "kpm", "abar"))
    s = GA.stream()
    f = lib.stlt_attn_grad_probs
    for args, word in (((q, g, k, 0, S, 0, H, dh, a, s), "length"), ((q, g, k, 0, 1, 257, H, dh, a, s), "length"),
                       ((q, g, k, 0, S, L, H, 0, a, s), "head dim"), ((q, g, k, 0, S, L, H, 257, a, s), "head dim"),
                       ((q, g, k, 0, S, L, 0, dh, a, s), "head count"), ((q, g, k, 0, -1, L, H, dh, a, s), "sequence"),
                       ((None, g, k, 0, S, L, H, dh, a, s), "null"), ((q, None, k, 0, S, L, H, dh, a, s), "null"), ((q, g, None, 0, S, L, H, dh, a, s), "null"),
                       ((q, g, k, 0, S, L, H, dh, None, s), "null"), ((q, g, k, 0, S, L, H, dh, a + 2, s), "abar")):
        assert f(*args) == EINVAL and word in GA.last_error(lib), (word, GA.last_error(lib))
    arena.check(launched=False)
    # dh = 25: four-byte alignment is enough, and the displaced call gives the aligned call's bits
    S, L, H, dh = 3, 9, 4, 25
    qkv, dctx, kpm = _op_case(S, L, H, dh, seed=6)
    specs = _op_specs(qkv, dctx, kpm)
    want = pkg.ops.attn_grad_probs(qkv.to(DEV), dctx.to(DEV), kpm.to(DEV), True, H).cpu()
    for operand in ("qkv", "dctx", "abar"):
        got = GA.misaligned(lib, arena, specs, _op_call(lib, S, L, H, dh, 1), ["abar"], operand=operand, mis=4)
        assert torch.equal(got["abar"].view(S, L, L), want), operand
    assert _rel(want, R.attn_grad_probs(qkv.double(), dctx.double(), kpm, True, H)) <= OP_CAP


# ---- the rollout kernel alone ------------------------------------------------------------------------------------------------------------
def _chain(abar, S, L):
    R_ = np.broadcast_to(np.eye(L), (S, L, L)).copy()
    for a in abar:
        R_ = R_ + a @ R_
    return R_


@pytest.mark.parametrize("n_layers", [0, 1, 4])
@pytest.mark.parametrize("L", [1, 7, 33, 64, 65, 130])
def test_attn_rollout_vs_fp64_chain_inside_guard_bands(pkg, arena, L, n_layers):
    """S = 1 and 9, random non-negative maps in [0, 1) / L (row sums below 1, like head-averaged probabilities times a gradient of order 1):
    <= ROLLOUT_CAP of max|ref| against the numpy fp64 chain; plain == arena == second call, bands intact, every element written."""
    lib = pkg._lib.load()
    worst = 0.0
    for S in (1, 9):
        abar = torch.rand(max(n_layers, 1), S, L, L, generator=torch.Generator().manual_seed(7 * L + S + n_layers)) / L
        specs = {"abar": (abar.reshape(-1, L), "in"), "R": (Out((S * L, L)), "out")}
        call = lambda o: lib.stlt_attn_rollout(o.abar.ptr if n_layers else None, n_layers, S, L, o.R.ptr, GA.stream())  # noqa: E731
        got = GA.three_ways(lib, arena, specs, call, ["R"])["R"].view(S, L, L)
        ref = torch.from_numpy(_chain(abar[:n_layers].double().numpy(), S, L))
        worst = max(worst, _rel(got, ref))
        assert worst <= ROLLOUT_CAP, (S, L, n_layers, worst)
        if n_layers == 0:
            assert torch.equal(got, torch.eye(L).expand(S, L, L))
        assert torch.equal(pkg.ops.attn_rollout(abar[:n_layers].to(DEV)).cpu(), got)  # the wrapper: the same bits
    _report(f"attn_rollout L={L} layers={n_layers} worst err / max|ref|", f"{worst:.2e}")


def test_rollout_and_combine_refusals(pkg):
    lib = pkg._lib.load()
    s = GA.stream()
    abar = torch.zeros(2 * 3 * 7 * 7 + 4, device=DEV)
    out = torch.full((3 * 257 * 257,), 7.0, device=DEV)
    lengths = torch.tensor([1, 2, 3], device=DEV)
    f = lib.stlt_attn_rollout
    for args, word in (((abar.data_ptr(), 2, 3, 0, out.data_ptr(), s), "length"), ((abar.data_ptr(), 2, 3, 257, out.data_ptr(), s), "length"),
                       ((abar.data_ptr(), 65, 3, 7, out.data_ptr(), s), "layer count"), ((abar.data_ptr(), -1, 3, 7, out.data_ptr(), s), "layer count"),
                       ((None, 2, 3, 7, out.data_ptr(), s), "null"), ((abar.data_ptr(), 2, 3, 7, None, s), "null"),
                       ((abar.data_ptr() + 2, 2, 3, 7, out.data_ptr(), s), "abar"), ((abar.data_ptr(), 2, 3, 7, out.data_ptr() + 2, s), "R must")):
        assert f(*args) == EINVAL and word in GA.last_error(lib), (word, GA.last_error(lib))
    g = lib.stlt_relevance_combine
    rt, rs = abar.data_ptr(), abar.data_ptr()
    for args, word in (((None, rs, lengths.data_ptr(), 3, 2, 2, out.data_ptr(), s), "null"), ((rt, rs, None, 3, 2, 2, out.data_ptr(), s), "null"),
                       ((rt, rs, lengths.data_ptr(), 3, 0, 2, out.data_ptr(), s), "shape"), ((rt, rs, lengths.data_ptr(), 3, 2, 2, out.data_ptr() + 2, s), "rel"),
                       ((rt, rs, lengths.data_ptr() + 4, 3, 2, 2, out.data_ptr(), s), "lengths")):
        assert g(*args) == EINVAL and word in GA.last_error(lib), (word, GA.last_error(lib))
    torch.cuda.synchronize()
    assert (out == 7.0).all()


# ---- the whole path --------------------------------------------------------------------------------------------------------------------
def _model(pkg, name, sd):
    m = pkg.Stlt(pkg.StltModelConfig(**pkg.synth.model_kwargs(name)))
    m.load_state_dict(sd, strict=True)
    m.train(False)
    return m.to(DEV)


@functools.lru_cache(maxsize=None)
def _run(pkg, name, form):
    """(model, device batch, fp64 reference, forward_relevance's output with the per-layer maps) of a whole-path case, once"""
    sd, batch, gold, target, ref = reference(name, form)
    m = _model(pkg, name, sd)
    dev = _to(batch)
    out = m.forward_relevance(dev, None if target is None else target.to(DEV), return_layers=True)
    return m, dev, batch, gold, target, ref, out


@pytest.mark.parametrize("name,form", WHOLE_PATH_CASES)
def test_forward_relevance_vs_fp64_restatement(pkg, name, form):
    m, dev, batch, gold, target, ref, out = _run(pkg, name, form)
    B, T, N = batch["categories"].shape
    c = pkg.synth.CONFIGS[name]
    assert set(out) == {"stlt", "target", "relevance", "spatial_rollout", "temporal_rollout", "spatial_layers", "temporal_layers"}
    assert out["relevance"].shape == (B, T, N) and out["spatial_rollout"].shape == (B, T, N, N) and out["temporal_rollout"].shape == (B, T, T)
    assert out["spatial_layers"].shape == (c["num_spatial_layers"], B, T, N, N) and out["temporal_layers"].shape == (c["num_temporal_layers"], B, T, T)
    assert all(out[k].dtype == torch.float32 and torch.isfinite(out[k]).all() for k in MAPS + ("spatial_layers", "temporal_layers", "stlt"))
    # the logits: forward's, the restatement's and the golden's
    with torch.no_grad():
        e_fwd = (m(dev)["stlt"] - out["stlt"]).abs().max().item()
    e_ref = (out["stlt"].cpu().double() - ref["stlt"]).abs().max().item()
    assert e_fwd <= LOGIT_TOL and e_ref <= LOGIT_TOL and (out["stlt"].cpu() - gold).abs().max().item() <= LOGIT_TOL
    # the objective
    if form == "seed":
        assert out["target"] is not None and torch.equal(out["target"].cpu(), target)
    else:
        assert torch.equal(out["target"].cpu(), ref["target"])
    errs = {k: _rel(out[k], ref[k]) for k in MAPS + ("spatial_layers", "temporal_layers")}
    _report(f"forward_relevance {name}/{form} err / max|ref| (bound {CAP:.1e}); logits vs forward {e_fwd:.2e}, vs fp64 {e_ref:.2e}",
            ", ".join(f"{k} {v:.2e}" for k, v in errs.items()))
    assert all(v <= CAP for v in errs.values()), errs
    # exact zeros: masked entries of every layer's map, padded object slots and padded frames of the relevance
    m_sp = AR.masked_entries(batch["src_key_padding_mask_boxes"].reshape(B * T, N), False).reshape(B, T, N, N)
    m_tp = AR.masked_entries(batch["src_key_padding_mask_frames"], True)
    assert (out["spatial_layers"].cpu()[:, m_sp] == 0).all() and (out["temporal_layers"].cpu()[:, m_tp] == 0).all()
    pad = R.padded_entries(batch)
    assert pad.any() and (out["relevance"].cpu()[pad] == 0).all()
    # without return_layers: the same bits, no per-layer keys
    short = m.forward_relevance(dev, None if target is None else target.to(DEV))
    assert set(short) == {"stlt", "target"} | set(MAPS) and all(torch.equal(short[k], out[k]) for k in MAPS + ("stlt",))


@pytest.mark.parametrize("name,form", [("cfg1", "top1"), ("odd", "seed"), ("cfg2p", "top1")])
def test_layers_through_the_ops_reproduce_the_one_call_result(pkg, name, form):
    """The per-layer maps pushed through ops.attn_rollout and ops.relevance_combine: the one-call rollouts and relevance, bit for bit."""
    m, dev, batch, _, _, _, out = _run(pkg, name, form)
    r_sp = pkg.ops.attn_rollout(out["spatial_layers"])
    r_tp = pkg.ops.attn_rollout(out["temporal_layers"])
    assert torch.equal(r_sp, out["spatial_rollout"]) and torch.equal(r_tp, out["temporal_rollout"])
    assert torch.equal(pkg.ops.relevance_combine(r_tp, r_sp, dev["lengths"]), out["relevance"])


def test_forward_relevance_leaves_no_state_behind(pkg):
    """forward, forward_attention and forward_saliency give the same bits before and after a forward_relevance call; no parameter gets a
    .grad; two calls give the same bits."""
    sd, batch, _, _, _ = reference("cfg1", "top1")
    m = _model(pkg, "cfg1", sd)
    dev = _to(batch)

    def others():
        with torch.no_grad():
            return {"forward": m(dev), "attention": m.forward_attention(dev), "saliency": m.forward_saliency(dev)}

    before = others()
    first = m.forward_relevance(dev, return_layers=True)
    after = others()
    for call, outs in before.items():
        for k, v in outs.items():
            assert torch.equal(v, after[call][k]), (call, k)
    assert all(q.grad is None for q in m.parameters())
    second = m.forward_relevance(dev, return_layers=True)
    assert all(torch.equal(first[k], second[k]) for k in first)


def test_forward_relevance_refusals(pkg):
    sd, batch, _, _, _ = reference("cfg1", "top1")
    m = _model(pkg, "cfg1", sd)
    dev = _to(batch)
    with pytest.raises(pkg.StltHipError, match="CPU tensors"):
        m.forward_relevance(batch)
    m.backbone.skip_padding = True
    with pytest.raises(pkg.StltHipError, match="skip_padding"):
        m.forward_relevance(dev)
    m.backbone.skip_padding = False
    md = pkg.Stlt(pkg.StltModelConfig(**dict(pkg.synth.model_kwargs("cfg1"), hidden_dropout_prob=0.1))).to(DEV)
    md.train(True)
    with pytest.raises(pkg.StltHipError, match="training mode"):
        md.forward_relevance(dev)
    with pytest.raises(pkg.StltHipError, match="target"):
        m.forward_relevance(dev, target=torch.zeros(3, dtype=torch.int64, device=DEV))


def _c_step(pkg, m, dev):
    bb = m.backbone
    logits, step = bb._train_forward(dev, m.prediction_head, 0)
    return logits, step, m._logit_seed(logits, None, None)


def test_sweep_refusals_through_the_c_abi(pkg):
    """STLT_FLAG_SKIP_PADDING, dropout_p != 0, UPPER_ONLY / LOWER_ONLY, a NULL and a misaligned map: STLT_EINVAL, the maps untouched."""
    lib, L = pkg._lib.load(), pkg._lib
    sd, batch, _, _, _ = reference("odd", "top1")
    m = _model(pkg, "odd", sd)
    dev = _to(batch)
    bb = m.backbone
    logits, step, seed = _c_step(pkg, m, dev)
    good = bb._train_relevance(step, seed)
    outs = {k: torch.full_like(v, 7.0) for k, v in good.items()}
    B, T, N = step["shape"]
    p, _, _ = bb.c_params(m.prediction_head)
    d = m.config.hidden_size
    tape = bb._train_buf("tape", int(lib.stlt_train_tape_bytes(B, T, N, d, p.n_spatial, p.n_temporal)), dev["categories"].device)
    scratch = bb._train_buf("scratch", int(lib.stlt_train_scratch_bytes(B, T, N, d, p.n_categories)), dev["categories"].device)

    def call(flags=0, drop=0.0, null=None, off=None):
        ptr = {k: v.data_ptr() for k, v in outs.items()}
        if null:
            ptr[null] = None
        if off:
            ptr[off] += 2
        maps = L.RelevanceMaps(ptr["spatial_layers"], ptr["temporal_layers"], ptr["spatial_rollout"], ptr["temporal_rollout"], ptr["relevance"])
        rc = lib.stlt_train_backward_relevance(C.byref(p), C.byref(step["inp"]), tape.data_ptr(), tape.numel(), scratch.data_ptr(), scratch.numel(),
                                               seed.data_ptr(), drop, 0, flags, None, C.byref(maps), GA.stream())
        return rc, GA.last_error(lib)

    for kwargs, word in ((dict(flags=L.FLAG_SKIP_PADDING), "SKIP_PADDING"), (dict(drop=0.1), "dropout"), (dict(flags=L.FLAG_TRAIN_UPPER_ONLY), "UPPER_ONLY"),
                         (dict(flags=L.FLAG_TRAIN_LOWER_ONLY), "LOWER_ONLY"), (dict(null="relevance"), "null map"), (dict(null="spatial_layers"), "null map"),
                         (dict(off="temporal_rollout"), "rollout_temporal")):
        rc, msg = call(**kwargs)
        assert rc == EINVAL and word in msg, (kwargs, rc, msg)
    torch.cuda.synchronize()
    assert all((v == 7.0).all() for v in outs.values())
    rc, msg = call()
    assert rc == 0, msg
    torch.cuda.synchronize()
    assert all(torch.equal(outs[k], good[k]) for k in good)


def test_sweep_replays_from_a_graph(pkg):
    """One single-stream capture of the C call (stlt_train_backward_relevance on a recorded tape), replayed twice: the eager bits."""
    sd, batch, _, _, _ = reference("cfg1", "top1")
    m = _model(pkg, "cfg1", sd)
    dev = _to(batch)
    bb = m.backbone
    logits, step, seed = _c_step(pkg, m, dev)
    eager = {k: v.clone() for k, v in bb._train_relevance(step, seed).items()}  # also the warm-up
    static = {k: torch.empty_like(v) for k, v in eager.items()}
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        bb._train_relevance(step, seed, static)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        bb._train_relevance(step, seed, static)
    for _ in range(2):
        for v in static.values():
            v.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        assert all(torch.equal(static[k], eager[k]) for k in eager)
