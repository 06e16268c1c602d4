"""Attention maps on the GPU: the probabilities kernel alone against fp64 (tests/attention_restated.py, which tests/test_attention_cpu.py
holds to fixtures captured from the reference's own nn.MultiheadAttention modules), Stlt.forward_attention against the fp64 restatement, the
goldens' logits and those fixtures, edge masks, NULL outputs, refusals, guard bands, determinism and graph capture."""
import ctypes as C
import functools
import os

import numpy as np
import pytest
import torch

import attention_restated as R
import guard_arena as GA
from conftest import GOLDEN, golden_case
from guard_arena import Out

pytestmark = pytest.mark.gpu
DEV = "cuda"
TOL = 1e-4  # the project's north-star bound (tests/test_model_gpu.py, tests/test_prefix_gpu.py)
EINVAL = -1


def _rand(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(*shape, generator=g) * 2 - 1) * scale


def _to(batch):
    return {k: (v.to(DEV) if isinstance(v, torch.Tensor) else v) for k, v in batch.items()}


def _model(pkg, kwargs, sd=None, seed=5):
    m = pkg.Stlt(pkg.StltModelConfig(**kwargs))
    if sd is None:
        sd = pkg.synth.make_state_dict({k: tuple(v.shape) for k, v in m.state_dict().items()}, seed=seed)
    m.load_state_dict(sd, strict=True)
    m.train(False)
    return m.to(DEV), sd


# ---- the kernel alone ------------------------------------------------------------------------------------------------------------
def _kernel_case(S, L, H, dh, scale, seed):
    """inputs drawn like test_attn_core's: uniform in [-scale, scale], about 30 % of the keys masked, key 0 kept"""
    qkv = _rand(S, L, 3 * H * dh, seed=seed, scale=scale)
    kpm = torch.rand(S, L, generator=torch.Generator().manual_seed(100 + seed)) < 0.3
    kpm[:, 0] = False
    return qkv, kpm


SHAPES = ([(4, 64, L) for L in (1, 2, 7, 15, 16, 17, 33, 36, 48, 64)]  # DIAG with an odd number of sequences per block, the 16-boundaries, cfg4's 36, 16 NB + 1
          + [(4, 64, 65), (4, 64, 100)]                               # generic path at head dim 64
          + [(1, 64, 7), (1, 64, 33), (12, 64, 7), (12, 64, 33)]      # one head, many heads
          + [(4, 96, 7), (4, 96, 65), (4, 25, 7), (4, 25, 65)])       # other head dims: 16-byte and four-byte reads


@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("H,dh,L", SHAPES)
def test_attn_probs_vs_fp64(pkg, H, dh, L, causal):
    """S = 5.  Per head and head-averaged: <= 2e-5 max-abs (test_attn_core's bound), masked entries exactly 0, rows with a visible key sum
    to 1 within 1e-5 (each of a row's at most 100 terms here carries a relative rounding of 6e-8, and so does the shared 1 / sum: at most
    100 * 6e-8 = 6e-6 if they all fell the same way), everything finite, and the averaged output is the mean of the per-head output within 1e-6."""
    S = 5
    qkv, kpm = _kernel_case(S, L, H, dh, 1.5, L + dh + H)
    masked = R.masked_entries(kpm, causal)
    out = {}
    for per_head in (False, True):
        got = pkg.ops.attn_probs(qkv.to(DEV), kpm.to(DEV), causal, H, per_head=per_head).cpu()
        ref = R.attn_probs(qkv.double(), kpm, causal, H, per_head)
        assert got.shape == ref.shape == ((S, H, L, L) if per_head else (S, L, L)) and got.dtype == torch.float32
        assert torch.isfinite(got).all()
        err = (got.double() - ref).abs().max().item()
        print(f"attn_probs H={H} dh={dh} L={L} causal={causal} per_head={per_head}: max abs err {err:.3g}")
        assert err <= 2e-5
        m = masked[:, None].expand(S, H, L, L) if per_head else masked
        assert (got[m] == 0).all()
        rows = ~m.all(dim=-1)  # rows with at least one visible key (key 0 is kept and the diagonal is visible: all of them here)
        assert rows.all() and (got.sum(-1)[rows] - 1).abs().max().item() <= 1e-5
        out[per_head] = got
    assert (out[False] - out[True].mean(dim=1)).abs().max().item() <= 1e-6


@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("L", [7, 40])
def test_attn_probs_edge_masks(pkg, L, causal):
    """S = 4, H = 2, peaked rows (scale 6): a sequence with every key masked is an all-zero block, a sequence with only key 0 visible has
    column 0 == 1 exactly, and their neighbours — at L = 7 inside the same 16-row block — are what they are when those two are unmasked."""
    S, H, dh = 4, 2, 64
    qkv, _ = _kernel_case(S, L, H, dh, 6.0, 11 + L)
    free = torch.zeros(S, L, dtype=torch.bool)
    kpm = free.clone()
    kpm[1, :] = True
    kpm[2, 1:] = True
    for per_head in (False, True):
        got = pkg.ops.attn_probs(qkv.to(DEV), kpm.to(DEV), causal, H, per_head=per_head).cpu()
        base = pkg.ops.attn_probs(qkv.to(DEV), free.to(DEV), causal, H, per_head=per_head).cpu()
        ref = R.attn_probs(qkv.double(), kpm, causal, H, per_head)
        assert torch.isfinite(got).all() and (got.double() - ref).abs().max().item() <= TOL  # peaked: test_attn_core's bound for scale 6
        assert (got[1] == 0).all()
        assert (got[2][..., 0] == 1).all() and (got[2][..., 1:] == 0).all()
        assert torch.equal(got[0], base[0]) and torch.equal(got[3], base[3])
        assert not torch.equal(got[1], base[1])


# ---- the whole path ----------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _golden_reference(name):
    """(state dict, batch, golden logits, fp64 restatement) of a golden case — computed once, shared, never modified"""
    import importlib
    from conftest import PKG_NAME
    synth = importlib.import_module(PKG_NAME + ".synth")
    sd, batch, z, meta = golden_case(name)
    ref = R.forward_attention(sd, batch, synth.CONFIGS[name]["num_attention_heads"])
    return sd, batch, torch.from_numpy(z["logits"]), ref


FIXTURES = ("cfg1", "cfg2p", "heads", "odd")


@pytest.mark.parametrize("name", ["cfg1", "cfg2p", "refdef", "heads", "odd", "cfg4"])
def test_forward_attention_vs_fp64_restatement(pkg, name):
    """Maps and logits within TOL of the fp64 restatement for the goldens' weights and batches, the logits within TOL of the golden's, and
    for the four fixture configs the maps directly against the reference's own weights.  The maxima per config are printed
    (profiles/attention_maps_bench.md records them)."""
    sd, batch, gold, ref = _golden_reference(name)
    m, _ = _model(pkg, pkg.synth.model_kwargs(name), sd)
    out = m.forward_attention(_to(batch))
    got, sp, tp = out["stlt"].cpu(), out["spatial_attention"].cpu(), out["temporal_attention"].cpu()
    B, T, N = batch["categories"].shape
    c = pkg.synth.CONFIGS[name]
    assert got.shape == gold.shape and sp.shape == (c["num_spatial_layers"], B, T, N, N) and tp.shape == (c["num_temporal_layers"], B, T, T)
    assert sp.dtype == tp.dtype == got.dtype == torch.float32
    assert torch.isfinite(got).all() and torch.isfinite(sp).all() and torch.isfinite(tp).all()
    e_sp = (sp.double() - ref["spatial_attention"].mean(dim=3)).abs().max().item()
    e_tp = (tp.double() - ref["temporal_attention"].mean(dim=2)).abs().max().item()
    e_lg = (got.double() - ref["stlt"]).abs().max().item()
    e_gold = (got - gold).abs().max().item()
    print(f"forward_attention {name}: vs fp64 restatement: spatial {e_sp:.3g} temporal {e_tp:.3g} logits {e_lg:.3g}; logits vs golden {e_gold:.3g}")
    assert e_sp <= TOL and e_tp <= TOL and e_lg <= TOL
    assert e_gold <= TOL
    # exact zeros where masked, in every layer
    m_sp = R.masked_entries(batch["src_key_padding_mask_boxes"].reshape(B * T, N), False).reshape(B, T, N, N)
    m_tp = R.masked_entries(batch["src_key_padding_mask_frames"], True)
    assert (sp[:, m_sp] == 0).all() and (tp[:, m_tp] == 0).all()
    if name in FIXTURES:
        fx = np.load(os.path.join(GOLDEN, f"attention_{name}.npz"))
        f_sp = (sp - torch.from_numpy(fx["spatial"])).abs().max().item()
        f_tp = (tp - torch.from_numpy(fx["temporal"])).abs().max().item()
        print(f"forward_attention {name}: vs the reference fixture: spatial {f_sp:.3g} temporal {f_tp:.3g}")
        assert f_sp <= TOL and f_tp <= TOL
    # the ordinary forward on the same device: the same prediction to rounding
    with torch.no_grad():
        assert (m(_to(batch))["stlt"].cpu() - got).abs().max().item() <= TOL


@pytest.mark.parametrize("name", ["cfg1", "odd"])
def test_forward_attention_per_head(pkg, name):
    sd, batch, gold, ref = _golden_reference(name)
    m, _ = _model(pkg, pkg.synth.model_kwargs(name), sd)
    dev = _to(batch)
    out = m.forward_attention(dev, per_head=True)
    sp, tp = out["spatial_attention"].cpu(), out["temporal_attention"].cpu()
    assert sp.shape == ref["spatial_attention"].shape and tp.shape == ref["temporal_attention"].shape
    e_sp = (sp.double() - ref["spatial_attention"]).abs().max().item()
    e_tp = (tp.double() - ref["temporal_attention"]).abs().max().item()
    print(f"forward_attention {name} per head: spatial {e_sp:.3g} temporal {e_tp:.3g}")
    assert e_sp <= TOL and e_tp <= TOL
    assert (out["stlt"].cpu().double() - ref["stlt"]).abs().max().item() <= TOL
    avg = m.forward_attention(dev)
    assert torch.equal(avg["stlt"], out["stlt"])
    assert (avg["spatial_attention"].cpu() - sp.mean(dim=3)).abs().max().item() <= 1e-6
    assert (avg["temporal_attention"].cpu() - tp.mean(dim=2)).abs().max().item() <= 1e-6


def _c_call(pkg, m, batch):
    """The C-ABI arguments of stlt_forward_attention for a model and a device batch: (params, inputs, keep-alive, B, T, N, d, K)"""
    inp, keep, (B, T, N) = pkg.modelling.models._prep_inputs(batch, need_lengths=True)
    p, _, _ = m.backbone.c_params(m.prediction_head)
    return p, inp, keep, B, T, N, m.config.hidden_size, m.prediction_head.fc2.weight.shape[0]


def _aligned_ws(nbytes):
    ws = torch.empty(nbytes + 512, dtype=torch.uint8, device=DEV)
    return ws, ws.data_ptr() + (-ws.data_ptr() % 256)


@pytest.mark.parametrize("per_head", [0, 1])
def test_null_outputs_change_nothing_else(pkg, per_head):
    """attn_spatial or attn_temporal NULL through the C-ABI: the other output and the logits are the same bits."""
    lib = pkg._lib.load()
    c = pkg.synth.CONFIGS["cfg1"]
    m, _ = _model(pkg, pkg.synth.model_kwargs("cfg1"))
    batch = _to(pkg.synth.make_batch(3, c["T"], c["N"], seed=4))
    p, inp, keep, B, T, N, d, K = _c_call(pkg, m, batch)
    H, n_sp, n_tp = c["num_attention_heads"], c["num_spatial_layers"], c["num_temporal_layers"]
    need = int(lib.stlt_attention_workspace_bytes(B, T, N, d, K))
    ws, base = _aligned_ws(need)
    hs = H if per_head else 1

    def run(want_sp, want_tp):
        logits = torch.full((B, K), 7.0, device=DEV)
        sp = torch.full((n_sp, B, T, hs, N, N), 7.0, device=DEV)
        tp = torch.full((n_tp, B, hs, T, T), 7.0, device=DEV)
        rc = lib.stlt_forward_attention(C.byref(p), C.byref(inp), base, need, 0, per_head, logits.data_ptr(), sp.data_ptr() if want_sp else None,
                                        tp.data_ptr() if want_tp else None, GA.stream())
        assert rc == 0, GA.last_error(lib)
        torch.cuda.synchronize()
        return logits, sp, tp

    full = run(True, True)
    assert not (full[1] == 7.0).any() and not (full[2] == 7.0).any()
    no_sp, no_tp, none = run(False, True), run(True, False), run(False, False)
    assert (no_sp[1] == 7.0).all() and torch.equal(no_sp[2], full[2]) and torch.equal(no_sp[0], full[0])
    assert (no_tp[2] == 7.0).all() and torch.equal(no_tp[1], full[1]) and torch.equal(no_tp[0], full[0])
    assert torch.equal(none[0], full[0])


# ---- refusals ----------------------------------------------------------------------------------------------------------------------
def test_whole_path_refusals(pkg):
    lib = pkg._lib.load()
    c = pkg.synth.CONFIGS["cfg1"]
    m, _ = _model(pkg, pkg.synth.model_kwargs("cfg1"))
    batch = _to(pkg.synth.make_batch(2, c["T"], c["N"], seed=1))
    m.backbone.skip_padding = True
    with pytest.raises(pkg.StltHipError, match="skip_padding"):
        m.forward_attention(batch)
    m.backbone.skip_padding = False
    md, _ = _model(pkg, dict(pkg.synth.model_kwargs("cfg1"), hidden_dropout_prob=0.1))
    md.train(True)
    with pytest.raises(pkg.StltHipError, match="training mode"):
        md.forward_attention(batch)
    p, inp, keep, B, T, N, d, K = _c_call(pkg, m, batch)
    need = int(lib.stlt_attention_workspace_bytes(B, T, N, d, K))
    assert need > 0 and lib.stlt_attention_workspace_bytes(0, T, N, d, K) == 0
    ws, base = _aligned_ws(need)
    logits = torch.full((B, K), 7.0, device=DEV)
    sp = torch.full((c["num_spatial_layers"], B, T, N, N), 7.0, device=DEV)
    tp = torch.full((c["num_temporal_layers"], B, T, T), 7.0, device=DEV)
    call = lambda ptr, nbytes, flags: lib.stlt_forward_attention(C.byref(p), C.byref(inp), ptr, nbytes, flags, 0, logits.data_ptr(), sp.data_ptr(),  # noqa: E731
                                                                 tp.data_ptr(), GA.stream())
    assert call(base, need, pkg._lib.FLAG_SKIP_PADDING) == EINVAL and "SKIP_PADDING" in GA.last_error(lib)
    assert call(base, need - 1, 0) == EINVAL and "workspace" in GA.last_error(lib)  # one byte short
    assert call(base + 16, need, 0) == EINVAL and "256-byte aligned" in GA.last_error(lib)
    torch.cuda.synchronize()
    assert (logits == 7.0).all() and (sp == 7.0).all() and (tp == 7.0).all()
    # the elision flags are ignored: the same bits as without them
    assert call(base, need, pkg._lib.FLAG_LAST_ROW_ONLY_TEMPORAL | pkg._lib.FLAG_CLS_ONLY_LAST_SPATIAL) == 0, GA.last_error(lib)
    torch.cuda.synchronize()
    want = m.forward_attention(batch)
    assert torch.equal(logits, want["stlt"]) and torch.equal(sp, want["spatial_attention"]) and torch.equal(tp, want["temporal_attention"])


def test_kernel_refusals_and_four_byte_alignment(pkg):
    """L = 0, L = 1025, dh = 257 and a qkv 4 bytes off a 16-byte boundary at dh = 64: STLT_EINVAL, nothing launched, the output untouched.
    The same displacement at dh = 25 is accepted and correct.  Every buffer is large enough for the shape named, refused or not."""
    lib = pkg._lib.load()
    s = GA.stream()
    buf = torch.zeros(1025 * 3 * 257 + 64, device=DEV)
    kpm = torch.zeros(1025, dtype=torch.uint8, device=DEV)
    out = torch.full((1025 * 1025 + 8,), 7.0, device=DEV)
    assert buf.data_ptr() % 16 == 0
    f = lib.stlt_attn_probs_fwd
    assert f(buf.data_ptr(), kpm.data_ptr(), 0, 1, 0, 1, 64, 0, out.data_ptr(), s) == EINVAL and "length" in GA.last_error(lib)
    assert f(buf.data_ptr(), kpm.data_ptr(), 0, 1, 1025, 1, 64, 0, out.data_ptr(), s) == EINVAL and "length" in GA.last_error(lib)
    assert f(buf.data_ptr(), kpm.data_ptr(), 0, 1, 4, 1, 257, 0, out.data_ptr(), s) == EINVAL and "head dim" in GA.last_error(lib)
    for L in (7, 65):  # both kernels of head dim 64
        assert f(buf.data_ptr() + 4, kpm.data_ptr(), 0, 2, L, 2, 64, 0, out.data_ptr(), s) == EINVAL
        assert "qkv" in GA.last_error(lib) and "aligned" in GA.last_error(lib)
    assert f(buf.data_ptr(), kpm.data_ptr(), 0, 2, 7, 2, 64, 2, out.data_ptr(), s) == EINVAL  # per_head is 0 or 1
    torch.cuda.synchronize()
    assert (out == 7.0).all()
    for L in (7, 65):
        S, H, dh = 3, 4, 25
        qkv, mask = _kernel_case(S, L, H, dh, 1.5, 3 + L)
        n = qkv.numel()
        buf[1:1 + n].copy_(qkv.reshape(-1).to(DEV))
        k8 = mask.to(torch.uint8).to(DEV)
        probs = torch.full((S, H, L, L), 7.0, device=DEV)
        assert (buf.data_ptr() + 4) % 16 == 4
        rc = f(buf.data_ptr() + 4, k8.data_ptr(), 1, S, L, H, dh, 1, probs.data_ptr(), s)
        assert rc == 0, GA.last_error(lib)
        torch.cuda.synchronize()
        assert (probs.cpu().double() - R.attn_probs(qkv.double(), mask, True, H, True)).abs().max().item() <= 2e-5
        assert torch.equal(probs, pkg.ops.attn_probs(qkv.to(DEV), k8, True, H, per_head=True))  # the aligned call: the same bits


# ---- guard bands -------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def arena():
    a = GA.Arena(768 << 20, DEV)
    yield a
    del a
    torch.cuda.empty_cache()


@pytest.mark.parametrize("per_head", [0, 1])
@pytest.mark.parametrize("S,L", [(3, 7), (3, 33), (2, 65)])
def test_attn_probs_inside_guard_bands(pkg, arena, S, L, per_head):
    """No byte outside probs changes and every element of it is written (DIAG with a partly filled last block, FULL with a partly filled
    last key block, the generic kernel), per head and averaged, causal."""
    lib = pkg._lib.load()
    H, dh = 4, 64
    qkv, kpm = _kernel_case(S, L, H, dh, 1.5, 7 + L)
    kpm[S - 1, :] = True  # a fully masked sequence: its zeros are written, not skipped
    shape = (S * H * L, L) if per_head else (S * L, L)
    specs = {"qkv": (qkv, "in"), "kpm": (kpm.to(torch.uint8), "extent", 0), "probs": (Out(shape), "out")}
    call = lambda o: lib.stlt_attn_probs_fwd(o.qkv.ptr, o.kpm.ptr, 1, S, L, H, dh, per_head, o.probs.ptr, GA.stream())  # noqa: E731
    got = GA.three_ways(lib, arena, specs, call, ["probs"])["probs"]
    ref = R.attn_probs(qkv.double(), kpm, True, H, bool(per_head))
    assert (got.view(ref.shape).double() - ref).abs().max().item() <= 2e-5
    assert (got.view(ref.shape)[S - 1] == 0).all()


@pytest.mark.parametrize("per_head", [0, 1])
def test_forward_attention_inside_guard_bands(pkg, arena, per_head):
    """micro, B = 3: every input of the batch, the workspace (exactly stlt_attention_workspace_bytes), the logits and both maps are arena
    operands; every byte of the three outputs is written."""
    lib = pkg._lib.load()
    c = pkg.synth.CONFIGS["micro"]
    m, _ = _model(pkg, pkg.synth.model_kwargs("micro"))
    batch = pkg.synth.make_batch(3, c["T"], c["N"], seed=2, min_len=2)
    want = m.forward_attention(_to(batch), per_head=bool(per_head))
    B, T, N = batch["categories"].shape
    d, K, H = m.config.hidden_size, m.prediction_head.fc2.weight.shape[0], c["num_attention_heads"]
    n_sp, n_tp, hs = c["num_spatial_layers"], c["num_temporal_layers"], (H if per_head else 1)
    p, _, _ = m.backbone.c_params(m.prediction_head)
    need = int(lib.stlt_attention_workspace_bytes(B, T, N, d, K))
    specs = {"categories": (batch["categories"], "index", 0), "boxes": (batch["boxes"], "in"),
             "kpm_boxes": (batch["src_key_padding_mask_boxes"].to(torch.uint8), "extent", 1), "frame_types": (batch["frame_types"], "index", 0),
             "kpm_frames": (batch["src_key_padding_mask_frames"].to(torch.uint8), "extent", 1), "lengths": (batch["lengths"], "extent", 1),
             "workspace": (Out((need,), torch.uint8, must_write=False), "out"), "logits": (Out((B, K)), "out"),
             "spatial": (Out((n_sp * B * T * hs * N, N)), "out"), "temporal": (Out((n_tp * B * hs * T, T)), "out")}

    def call(o):
        inp = pkg._lib.Inputs()
        inp.B, inp.T, inp.N = B, T, N
        inp.categories, inp.boxes, inp.scores, inp.kpm_boxes = o.categories.ptr, o.boxes.ptr, None, o.kpm_boxes.ptr
        inp.frame_types, inp.kpm_frames, inp.lengths = o.frame_types.ptr, o.kpm_frames.ptr, o.lengths.ptr
        return lib.stlt_forward_attention(C.byref(p), C.byref(inp), o.workspace.ptr, need, 0, per_head, o.logits.ptr, o.spatial.ptr, o.temporal.ptr, GA.stream())

    got = GA.three_ways(lib, arena, specs, call, ["logits", "spatial", "temporal"])
    assert torch.equal(got["logits"], want["stlt"].cpu())
    assert torch.equal(got["spatial"].view(want["spatial_attention"].shape), want["spatial_attention"].cpu())
    assert torch.equal(got["temporal"].view(want["temporal_attention"].shape), want["temporal_attention"].cpu())


# ---- determinism and capture ---------------------------------------------------------------------------------------------------------
KEYS = ("stlt", "spatial_attention", "temporal_attention")


def test_forward_attention_is_deterministic_and_replays_from_a_graph(pkg):
    """Two eager calls on cfg1 are the same bits (the head average is summed in registers, no atomics), and one single-stream capture
    replayed twice gives the eager result both times."""
    sd, batch, gold, ref = _golden_reference("cfg1")
    m, _ = _model(pkg, pkg.synth.model_kwargs("cfg1"), sd)
    static = _to(batch)
    first = {k: v.clone() for k, v in m.forward_attention(static).items()}  # also the warm-up
    second = m.forward_attention(static)
    assert all(torch.equal(first[k], second[k]) for k in KEYS)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        m.forward_attention(static)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = m.forward_attention(static)
    for _ in range(2):
        for k in KEYS:
            captured[k].fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        assert all(torch.equal(captured[k], first[k]) for k in KEYS)
