"""Per-prefix logits on the GPU: the probe-attention kernel alone against fp64, Stlt.forward_prefixes against the fp64 two-stream
restatement (tests/prefix_restated.py, which tests/test_prefix_cpu.py holds to the oracle on truncated batches) and against the goldens,
edge shapes, refusals, guard bands, run_prefix_inference and graph capture."""
import ctypes as C
import functools
import pytest
import torch

import guard_arena as GA
import prefix_restated as R
from conftest import golden_case
from guard_arena import Out

pytestmark = pytest.mark.gpu
DEV = "cuda"
TOL = 1e-4  # the project's north-star bound on logits (tests/test_model_gpu.py)


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
def _probe_case(S, T, H, dh, scale, seed):
    d = H * dh
    qkv_f, qkv_p = _rand(S, T, 3 * d, seed=seed, scale=scale), _rand(S, T, 3 * d, seed=seed + 1000, scale=scale)
    kpm = torch.rand(S, T, generator=torch.Generator().manual_seed(100 + seed)) < 0.3
    kpm[:, 0] = False  # frame 0 is never masked
    return qkv_f, qkv_p, kpm


@pytest.mark.parametrize("dh,T", [(64, T) for T in (1, 2, 3, 16, 17, 33, 64, 65, 100, 256)] + [(96, 7), (96, 65), (25, 7), (25, 65)])
def test_probe_attention_vs_fp64(pkg, dh, T):
    """S = 5 clips, H = 4: one and several query blocks (32 probes each), one and several key tiles (64 keys), head dims on the 16-byte
    (64, 96: two channel groups) and the four-byte path (25); inputs drawn like test_attn_core's; 2e-5 max-abs, that test's bound."""
    S, H = 5, 4
    qkv_f, qkv_p, kpm = _probe_case(S, T, H, dh, 1.5, T + dh)
    got = pkg.ops.attn_prefix_probe(qkv_f.to(DEV), qkv_p.to(DEV), kpm.to(DEV), H).cpu()
    ref = R.probe_attention(qkv_f.double(), qkv_p.double(), kpm, H)
    assert got.shape == (S, T, H * dh) and torch.isfinite(got).all()
    err = (got.double() - ref).abs().max().item()
    print(f"probe attention dh={dh} T={T}: max abs err {err:.3g}")
    assert err <= 2e-5
    # probe 0 sees its own key only: its value row, to rounding (one ulp of the largest value)
    assert (got[:, 0] - qkv_p[:, 0, 2 * H * dh:]).abs().max().item() <= 2e-7


def test_probe_attention_peaked_with_a_fully_masked_first_key_tile(pkg):
    """Large logits (the online-softmax rescale across key tiles) at T = 70, and a clip whose first key tile (64 keys) is masked entirely."""
    S, T, H, dh = 4, 70, 2, 64
    qkv_f, qkv_p, _ = _probe_case(S, T, H, dh, 6.0, 5)
    kpm = torch.zeros(S, T, dtype=torch.bool)
    kpm[1, :] = True    # every frame key masked: each probe attends to itself only
    kpm[2, :64] = True  # first key tile fully masked
    got = pkg.ops.attn_prefix_probe(qkv_f.to(DEV), qkv_p.to(DEV), kpm.to(DEV), H).cpu()
    ref = R.probe_attention(qkv_f.double(), qkv_p.double(), kpm, H)
    assert torch.isfinite(got).all()
    err = (got.double() - ref).abs().max().item()
    print(f"probe attention peaked: max abs err {err:.3g}")
    assert err <= 1e-4
    assert (got[1] - qkv_p[1, :, 2 * H * dh:]).abs().max().item() <= 1e-6


# ---- the whole path ----------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _golden_reference(name):
    """(state dict, batch, golden logits, fp64 restatement, valid) of a golden case — computed once, shared, never modified"""
    sd, batch, z, meta = golden_case(name)
    H = importlib_synth().CONFIGS[name]["num_attention_heads"]
    ref, valid = R.forward_prefixes(sd, batch, H)
    return sd, batch, torch.from_numpy(z["logits"]), ref, valid


def importlib_synth():
    import importlib
    from conftest import PKG_NAME
    return importlib.import_module(PKG_NAME + ".synth")


@pytest.mark.parametrize("cls_only", [True, False])
@pytest.mark.parametrize("name", ["cfg1", "cfg2p", "refdef", "heads", "odd", "cfg4"])
def test_forward_prefixes_vs_fp64_restatement(pkg, name, cls_only):
    """Every valid entry within TOL of the fp64 restatement, for the goldens' weights and batches and both settings of the spatial elision.
    The maximum per config is printed (profiles/prefix_logits_bench.md records them); the ordinary forward sits at 1.4e-6 ... 3.1e-6."""
    sd, batch, gold, ref, valid = _golden_reference(name)
    m, _ = _model(pkg, pkg.synth.model_kwargs(name), sd)
    m.backbone.cls_only_last_spatial = cls_only
    out = m.forward_prefixes(_to(batch))
    got, got_valid = out["stlt"].cpu(), out["valid"].cpu()
    B, T = batch["categories"].shape[:2]
    assert got.shape == ref.shape == (B, T, gold.shape[1]) and got.dtype == torch.float32 and got_valid.dtype == torch.bool
    assert torch.equal(got_valid, valid) and torch.equal(valid, torch.arange(T)[None] < batch["lengths"][:, None])
    assert torch.isfinite(got).all()
    err = (got.double() - ref)[valid].abs().max().item()
    print(f"forward_prefixes {name} cls_only={cls_only}: max abs err over valid entries {err:.3g}")
    assert err <= TOL
    assert (got[~valid] == 0).all()  # exactly zero, never uninitialised
    # the full-clip prefix is the model's ordinary prediction
    last = got[torch.arange(B), batch["lengths"] - 1]
    assert (last - gold).abs().max().item() <= TOL
    if name == "cfg1":  # ... and every prefix directly against the oracle on the truncated batches
        want, _ = R.truncated_oracle(sd, batch, pkg.synth.CONFIGS[name]["num_attention_heads"], pkg.collate.prefix_batch)
        e2 = (got.double() - want)[valid].abs().max().item()
        print(f"forward_prefixes cfg1 cls_only={cls_only}: against the oracle on truncated batches {e2:.3g}")
        assert e2 <= TOL


def test_forward_prefixes_agrees_with_forward(pkg):
    """The last valid prefix against the model's own forward on the same device (not only the golden), and prefix t against forward on
    prefix_batch(batch, t) for the clips that have it."""
    sd, batch, gold, ref, valid = _golden_reference("cfg1")
    m, _ = _model(pkg, pkg.synth.model_kwargs("cfg1"), sd)
    dev = _to(batch)
    got = m.forward_prefixes(dev)["stlt"]
    B, T = valid.shape
    with torch.no_grad():
        full = m(dev)["stlt"]
        assert (got[torch.arange(B), dev["lengths"] - 1] - full).abs().max().item() <= TOL
        for t in (0, 1, T // 2):
            keep = valid[:, t].to(DEV)
            trunc = m(pkg.collate.prefix_batch(dev, t))["stlt"]
            assert (trunc[keep] - got[keep, t]).abs().max().item() <= TOL, t


TINY = dict(num_classes=11, unique_categories=None, hidden_size=128, num_attention_heads=2, num_spatial_layers=1, num_temporal_layers=2,
            hidden_dropout_prob=0.0)


def _edge_batches(synth):
    one = synth.make_batch(3, 2, 3, seed=2)
    # T = 2 with every length 1: the extract frame is frame 0, frame 1 is padding
    one["lengths"][:] = 1
    one["frame_types"][:, 0] = synth.DATASETS["something"]["extract"]
    one["frame_types"][:, 1] = 0
    one["categories"][:, :, 1:] = 0
    one["src_key_padding_mask_boxes"] = one["categories"] == 0
    one["src_key_padding_mask_frames"] = one["frame_types"] == 0
    return {"T=1": synth.make_batch(4, 1, 3, seed=1, min_len=1), "T=2, lengths 1": one, "B=1": synth.make_batch(1, 6, 4, seed=3),
            "N=1": synth.make_batch(3, 5, 1, seed=4, min_len=2), "T=65": synth.make_batch(2, 65, 3, seed=5, min_len=2)}


@pytest.mark.parametrize("case", ["T=1", "T=2, lengths 1", "B=1", "N=1", "T=65"])
def test_forward_prefixes_edge_shapes(pkg, case):
    m, sd = _model(pkg, dict(TINY, unique_categories=pkg.synth.DATASETS["something"]["unique_categories"]))
    batch = _edge_batches(pkg.synth)[case]
    ref, valid = R.forward_prefixes(sd, batch, TINY["num_attention_heads"])
    got = m.forward_prefixes(_to(batch))["stlt"].cpu()
    assert torch.isfinite(got).all() and got.shape == ref.shape
    err = (got.double() - ref)[valid].abs().max().item()
    print(f"forward_prefixes edge {case}: max abs err {err:.3g}")
    assert err <= TOL
    assert (got[~valid] == 0).all()


# ---- refusals ----------------------------------------------------------------------------------------------------------------------
def _c_call(pkg, m, batch):
    """The C-ABI arguments of stlt_forward_prefixes for a model and a device batch: (params, inputs, keep-alive, B, T, N, d, K)"""
    models = pkg.modelling.models
    inp, keep, (B, T, N) = models._prep_inputs(batch, need_lengths=True)
    p, _, _ = m.backbone.c_params(m.prediction_head)
    return p, inp, keep, B, T, N, m.config.hidden_size, m.prediction_head.fc2.weight.shape[0]


def test_refusals(pkg):
    lib = pkg._lib.load()
    c = pkg.synth.CONFIGS["cfg1"]
    m, _ = _model(pkg, pkg.synth.model_kwargs("cfg1"))
    batch = _to(pkg.synth.make_batch(2, c["T"], c["N"], seed=1))
    # skip_padding and live dropout: refused in Python before anything is prepared ...
    m.backbone.skip_padding = True
    with pytest.raises(pkg.StltHipError, match="skip_padding"):
        m.forward_prefixes(batch)
    m.backbone.skip_padding = False
    md, _ = _model(pkg, dict(pkg.synth.model_kwargs("cfg1"), hidden_dropout_prob=0.1))
    md.train(True)
    with pytest.raises(pkg.StltHipError, match="training mode"):
        md.forward_prefixes(batch)
    # ... and at the C-ABI: STLT_EINVAL, a message, nothing launched (the logits keep their sentinel)
    p, inp, keep, B, T, N, d, K = _c_call(pkg, m, batch)
    need = int(lib.stlt_prefix_workspace_bytes(B, T, N, d, K))
    assert need >= pkg.ops.workspace_bytes(B, T, N, d, K) > 0 and lib.stlt_prefix_workspace_bytes(0, T, N, d, K) == 0
    ws = torch.empty(need + 512, dtype=torch.uint8, device=DEV)
    base = ws.data_ptr() + (-ws.data_ptr() % 256)
    logits = torch.full((B, T, K), 7.0, device=DEV)
    s = GA.stream()
    call = lambda ptr, nbytes, flags: lib.stlt_forward_prefixes(C.byref(p), C.byref(inp), ptr, nbytes, flags, logits.data_ptr(), s)  # noqa: E731
    assert call(base, need, pkg._lib.FLAG_SKIP_PADDING) == -1 and "SKIP_PADDING" in GA.last_error(lib)
    assert call(base, need - 256, 0) == -2 and "workspace" in GA.last_error(lib)   # STLT_EWORKSPACE
    assert call(base + 16, need, 0) == -1 and "256-byte aligned" in GA.last_error(lib)
    torch.cuda.synchronize()
    assert (logits == 7.0).all()
    assert call(base, need, pkg._lib.FLAG_LAST_ROW_ONLY_TEMPORAL | pkg._lib.FLAG_CLS_ONLY_LAST_SPATIAL) == 0, GA.last_error(lib)  # ignored / honoured
    torch.cuda.synchronize()
    assert torch.equal(logits, m.forward_prefixes(batch)["stlt"])
    # an op-level pointer off 16 bytes
    S, Tq, H, dh = 2, 5, 2, 64
    buf = torch.zeros(3 * S * Tq * 3 * H * dh + 64, device=DEV)
    n = S * Tq * 3 * H * dh
    kpm = torch.zeros(S, Tq, dtype=torch.uint8, device=DEV)
    out = torch.full((S * Tq * H * dh + 8,), 7.0, device=DEV)
    good = (buf.data_ptr(), buf.data_ptr() + 4 * n, out.data_ptr())
    for i, name in enumerate(("qkv_frames", "qkv_probes", "ctx")):
        ptrs = list(good)
        ptrs[i] += 4
        rc = lib.stlt_attn_prefix_probe_fwd(ptrs[0], ptrs[1], kpm.data_ptr(), S, Tq, H, dh, ptrs[2], s)
        assert rc == -1 and name in GA.last_error(lib) and "aligned" in GA.last_error(lib)
    assert lib.stlt_attn_prefix_probe_fwd(good[0], good[1], kpm.data_ptr(), S, Tq, H, 257, good[2], s) == -1
    torch.cuda.synchronize()
    assert (out == 7.0).all()


# ---- guard bands -------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def arena():
    a = GA.Arena(768 << 20, DEV)
    yield a
    del a
    torch.cuda.empty_cache()


@pytest.mark.parametrize("dh,T", [(64, 33), (64, 65), (25, 7), (96, 65)])
def test_probe_attention_inside_guard_bands(pkg, arena, dh, T):
    lib = pkg._lib.load()
    S, H = 3, 2
    qkv_f, qkv_p, kpm = _probe_case(S, T, H, dh, 1.5, 7 + T)
    specs = {"qkv_f": (qkv_f, "in"), "qkv_p": (qkv_p, "in"), "kpm": (kpm.to(torch.uint8), "extent", 0), "ctx": (Out((S * T, H * dh)), "out")}
    call = lambda o: lib.stlt_attn_prefix_probe_fwd(o.qkv_f.ptr, o.qkv_p.ptr, o.kpm.ptr, S, T, H, dh, o.ctx.ptr, GA.stream())  # noqa: E731
    got = GA.three_ways(lib, arena, specs, call, ["ctx"])["ctx"].view(S, T, H * dh)
    ref = R.probe_attention(qkv_f.double(), qkv_p.double(), kpm, H)
    assert (got.double() - ref).abs().max().item() <= 2e-5


@pytest.mark.parametrize("cls_only", [True, False])
def test_forward_prefixes_inside_guard_bands(pkg, arena, cls_only):
    """cfg1, B = 3: every input of the batch, the workspace (exactly stlt_prefix_workspace_bytes) and the logits are arena operands."""
    lib = pkg._lib.load()
    c = pkg.synth.CONFIGS["cfg1"]
    m, _ = _model(pkg, pkg.synth.model_kwargs("cfg1"))
    m.backbone.cls_only_last_spatial = cls_only
    batch = pkg.synth.make_batch(3, c["T"], c["N"], seed=2, min_len=2)
    want = m.forward_prefixes(_to(batch))["stlt"]
    B, T, N = batch["categories"].shape
    d, K = m.config.hidden_size, m.prediction_head.fc2.weight.shape[0]
    p, _, _ = m.backbone.c_params(m.prediction_head)
    need = int(lib.stlt_prefix_workspace_bytes(B, T, N, d, K))
    specs = {"categories": (batch["categories"], "index", 0), "boxes": (batch["boxes"], "in"),
             "kpm_boxes": (batch["src_key_padding_mask_boxes"].to(torch.uint8), "extent", 1), "frame_types": (batch["frame_types"], "index", 0),
             "kpm_frames": (batch["src_key_padding_mask_frames"].to(torch.uint8), "extent", 1), "lengths": (batch["lengths"], "extent", 1),
             "workspace": (Out((need,), torch.uint8, must_write=False), "out"), "logits": (Out((B * T, K)), "out")}

    def call(o):
        inp = pkg._lib.Inputs()
        inp.B, inp.T, inp.N = B, T, N
        inp.categories, inp.boxes, inp.scores, inp.kpm_boxes = o.categories.ptr, o.boxes.ptr, None, o.kpm_boxes.ptr
        inp.frame_types, inp.kpm_frames, inp.lengths = o.frame_types.ptr, o.kpm_frames.ptr, o.lengths.ptr
        return lib.stlt_forward_prefixes(C.byref(p), C.byref(inp), o.workspace.ptr, need, m.backbone._flags(), o.logits.ptr, GA.stream())

    got = GA.three_ways(lib, arena, specs, call, ["logits"])["logits"]
    assert torch.equal(got.view(B, T, K), want.cpu())


# ---- run_prefix_inference ----------------------------------------------------------------------------------------------------------
def test_run_prefix_inference_counts(pkg):
    c = pkg.synth.CONFIGS["cfg1"]
    m, _ = _model(pkg, pkg.synth.model_kwargs("cfg1"))
    T, K = c["T"], c["num_classes"]
    batches = []
    for i, n in enumerate((6, 3)):
        b = pkg.synth.make_batch(n, T, c["N"], seed=50 + i, min_len=2)
        logits = m.forward_prefixes(_to(b))["stlt"].cpu()
        # labels chosen from the logits so that hits, top-5-only hits and misses all occur, differently per clip
        rank = torch.tensor([(0, 3, 9)[j % 3] for j in range(n)])
        order = logits[torch.arange(n), b["lengths"] - 1].argsort(dim=1, descending=True)
        b["labels"] = order[torch.arange(n), rank]
        batches.append(b)
    res = pkg.infer.run_prefix_inference(m, batches, DEV)
    assert set(res) == {"top1", "top5", "num_clips"} and all(v.shape == (T,) and v.dtype == torch.int64 for v in res.values())
    top1, top5, cnt = torch.zeros(T, dtype=torch.int64), torch.zeros(T, dtype=torch.int64), torch.zeros(T, dtype=torch.int64)
    last = torch.zeros(3, dtype=torch.int64)
    for b in batches:
        out = m.forward_prefixes(_to(b))
        logits, valid = out["stlt"].cpu(), out["valid"].cpu()
        # rank of the label: classes with a larger logit, or an equal one at a lower index (include/stlt_hip.h: stlt_eval_topk)
        lab = logits.gather(2, b["labels"][:, None, None].expand(-1, T, 1))
        idx = torch.arange(K)[None, None, :]
        rank = ((logits > lab) | ((logits == lab) & (idx < b["labels"][:, None, None]))).sum(-1)
        top1 += ((rank < 1) & valid).sum(0)
        top5 += ((rank < 5) & valid).sum(0)
        cnt += valid.sum(0)
        rl = rank[torch.arange(len(rank)), b["lengths"] - 1]
        last += torch.tensor([int((rl < 1).sum()), int((rl < 5).sum()), len(rl)])
    assert torch.equal(res["top1"], top1) and torch.equal(res["top5"], top5) and torch.equal(res["num_clips"], cnt)
    assert cnt[0] == 9 and cnt[-1] >= 2 and 0 < int(top1.sum()) < int(top5.sum()) < int(cnt.sum())
    # the last valid prefix of every clip is the ordinary forward: run_inference's totals
    whole = pkg.infer.run_inference(m, batches, DEV)
    assert whole["num_clips"] == int(last[2]) == 9
    assert whole["top1_accuracy"] == round(100.0 * int(last[0]) / 9, 2) and whole["top5_accuracy"] == round(100.0 * int(last[1]) / 9, 2)


# ---- capture -----------------------------------------------------------------------------------------------------------------------
def test_forward_prefixes_replays_from_a_graph(pkg):
    sd, batch, gold, ref, valid = _golden_reference("cfg1")
    m, _ = _model(pkg, pkg.synth.model_kwargs("cfg1"), sd)
    static = _to(batch)
    others = []
    for f in (0.5, 0.25):
        o = {k: v.clone() for k, v in static.items()}
        o["boxes"] = (o["boxes"] * f).contiguous()
        others.append(o)
    first = {k: v.clone() for k, v in static.items()}
    eager = [m.forward_prefixes(b)["stlt"].clone() for b in [static] + others]  # also the warm-up
    assert not torch.equal(eager[0], eager[1]) and not torch.equal(eager[1], eager[2])
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        m.forward_prefixes(static)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = m.forward_prefixes(static)["stlt"]
    for src, want in zip(others + [first], eager[1:] + eager[:1]):
        for k in static:
            static[k].copy_(src[k])
        captured.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(captured, want)
