"""Attention maps of the fusion models on the GPU: the cross-probabilities kernel alone against fp64 (tests/fusion_attention_restated.py,
which tests/test_fusion_attention_cpu.py holds to fixtures captured from the reference's own nn.MultiheadAttention modules),
forward_attention of CAF / CACNF / LCF against the fp64 restatement, those fixtures, the ordinary forward and Stlt.forward_attention, edge
masks, NULL sinks, refusals, guard bands, determinism and graph capture."""
import ctypes as C
import functools
import os

import numpy as np
import pytest
import torch

import attention_restated as R
import fusion_attention_restated as FR
import guard_arena as GA
from conftest import GOLDEN
from guard_arena import Out
from test_fusion_attention_cpu import EXTRA, fusion_case

pytestmark = pytest.mark.gpu
DEV = "cuda"
TOL = 1e-4  # the project's north-star bound (tests/test_attention_gpu.py)
EINVAL = -1
LOGITS = {"caf": ("caf",), "cacnf": ("stlt", "resnet3d", "caf", "ensemble"), "lcf": ("lcf",)}


def _rand(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(*shape, generator=g) * 2 - 1) * scale


def _to(batch):
    return {k: (v.to(DEV) if isinstance(v, torch.Tensor) else v) for k, v in batch.items()}


# ---- the kernel alone ------------------------------------------------------------------------------------------------------------
def _kernel_case(S, Lq, Lk, H, dh, scale, seed):
    """inputs drawn like test_attn_probs_vs_fp64's: uniform in [-scale, scale], about 30 % of the keys masked, key 0 kept.  The queries lie
    in the first d columns of a packed (S,Lq,3d) buffer, the keys in the first d columns of an (S,Lk,2d) buffer."""
    d = H * dh
    qbuf = _rand(S, Lq, 3 * d, seed=seed, scale=scale)
    kbuf = _rand(S, Lk, 2 * d, seed=seed + 1000, scale=scale)
    kpm = torch.rand(S, Lk, generator=torch.Generator().manual_seed(100 + seed)) < 0.3
    kpm[:, 0] = False
    return qbuf, kbuf, kpm


def _views(qbuf, kbuf, d):
    qd, kd = qbuf.to(DEV), kbuf.to(DEV)
    return qd[..., :d], kd[..., :d]  # row strides 3d and 2d


SHAPES = ([(4, 64, Lq, Lk, False) for Lq, Lk in ((1, 1), (7, 33), (33, 7), (16, 17), (17, 16), (33, 33), (17, 33), (33, 17), (65, 33), (33, 64), (33, 65),
                                                 (100, 40), (40, 100))]
          + [(1, 64, 17, 33, False), (12, 64, 17, 33, False)]                                    # one head, many heads
          + [(H, dh, Lq, Lk, False) for H, dh in ((4, 96), (4, 25)) for Lq, Lk in ((7, 33), (33, 65))]  # other head dims: 16-byte and four-byte reads
          + [(4, 64, 33, 33, True), (4, 64, 65, 65, True)])                                     # causal, both kernels


@pytest.mark.parametrize("H,dh,Lq,Lk,causal", SHAPES)
def test_attn_probs_cross_vs_fp64(pkg, H, dh, Lq, Lk, causal):
    """S = 5 (a partly filled workgroup).  Per head and head-averaged: <= 2e-5 max-abs (test_attn_probs_vs_fp64's bound), masked entries
    exactly 0, rows sum to 1 within 1e-5 (key 0 is kept: every row has a visible key), everything finite, and the averaged output is the
    mean of the per-head output within 1e-6."""
    S, d = 5, H * dh
    qbuf, kbuf, kpm = _kernel_case(S, Lq, Lk, H, dh, 1.5, Lq + 3 * Lk + dh + H)
    q, k = _views(qbuf, kbuf, d)
    assert q.stride(1) == 3 * d and k.stride(1) == 2 * d
    masked = FR.masked_entries(kpm, causal, S, Lq, Lk)
    out = {}
    for per_head in (False, True):
        got = pkg.ops.attn_probs_cross(q, k, kpm.to(DEV), causal, H, per_head=per_head).cpu()
        ref = FR.attn_probs_cross(qbuf[..., :d].double(), kbuf[..., :d].double(), kpm, causal, H, per_head)
        assert got.shape == ref.shape == ((S, H, Lq, Lk) if per_head else (S, Lq, Lk)) and got.dtype == torch.float32
        assert torch.isfinite(got).all()
        err = (got.double() - ref).abs().max().item()
        print(f"attn_probs_cross H={H} dh={dh} Lq={Lq} Lk={Lk} causal={causal} per_head={per_head}: max abs err {err:.3g}")
        assert err <= 2e-5
        m = masked[:, None].expand(S, H, Lq, Lk) if per_head else masked
        assert (got[m] == 0).all()
        assert (got.sum(-1) - 1).abs().max().item() <= 1e-5
        out[per_head] = got
    assert (out[False] - out[True].mean(dim=1)).abs().max().item() <= 1e-6


# (L, dh): 17 = two key blocks, the 17th row alone in its block; 65 = generic, the second key of a lane; dh 20 = generic, scalar reads
PACKED_VIEWS = [(7, 64), (16, 64), (17, 64), (33, 64), (64, 64), (65, 64), (33, 20)]


@pytest.mark.parametrize("L,dh,causal", [(L, dh, c) for c in (False, True) for L, dh in PACKED_VIEWS],
                         ids=[f"{L}{'' if dh == 64 else f'dh{dh}'}-{c}" for c in (False, True) for L, dh in PACKED_VIEWS])
def test_attn_probs_cross_on_one_packed_buffer_is_attn_probs(pkg, L, dh, causal):
    """q and k as views of one packed QKV buffer, Lq == Lk, against ops.attn_probs.  Above 16 tokens both entries run the same kernel on
    the same views (the sided MFMA kernel up to 64 tokens at head dim 64, the vector kernel elsewhere): equal bit for bit, S = 3 with
    some keys masked and the last sequence's keys all masked.  Up to 16 tokens the packed entry runs the diag form (several sequences to
    a 16-row block, S = 5 leaves the last block partial) against one sided block: within 1e-6."""
    same_kernel = L > 16
    S, H = (3 if same_kernel else 5), 4
    d = H * dh
    qkv = _rand(S, L, 3 * d, seed=L, scale=1.5).to(DEV)
    kpm = (torch.rand(S, L, generator=torch.Generator().manual_seed(L)) < 0.3)
    kpm[:, 0] = False
    if same_kernel:
        kpm[S - 1, :] = True
    for per_head in (False, True):
        a = pkg.ops.attn_probs_cross(qkv[..., :d], qkv[..., d:2 * d], kpm.to(DEV), causal, H, per_head=per_head)
        b = pkg.ops.attn_probs(qkv, kpm.to(DEV), causal, H, per_head=per_head)
        if same_kernel:
            assert torch.equal(a, b) and (a[S - 1] == 0).all() and a[0].abs().max().item() > 0
        else:
            assert (a - b).abs().max().item() <= 1e-6


@pytest.mark.parametrize("Lq,Lk", [(7, 40), (40, 7)])
def test_attn_probs_cross_edge_masks(pkg, Lq, Lk):
    """S = 4, H = 2, peaked rows (scale 6): a sequence with every key masked is an all-zero block, a sequence with only key 0 visible has
    column 0 == 1 exactly, and their neighbours are what they are when those two are unmasked."""
    S, H, dh = 4, 2, 64
    d = H * dh
    qbuf, kbuf, _ = _kernel_case(S, Lq, Lk, H, dh, 6.0, 11 + Lq)
    q, k = _views(qbuf, kbuf, d)
    free = torch.zeros(S, Lk, dtype=torch.bool)
    kpm = free.clone()
    kpm[1, :] = True
    kpm[2, 1:] = True
    for per_head in (False, True):
        got = pkg.ops.attn_probs_cross(q, k, kpm.to(DEV), False, H, per_head=per_head).cpu()
        base = pkg.ops.attn_probs_cross(q, k, free.to(DEV), False, H, per_head=per_head).cpu()
        ref = FR.attn_probs_cross(qbuf[..., :d].double(), kbuf[..., :d].double(), kpm, False, H, per_head)
        assert torch.isfinite(got).all() and (got.double() - ref).abs().max().item() <= TOL  # peaked: test_attn_probs_edge_masks' bound for scale 6
        assert (got[1] == 0).all()
        assert (got[2][..., 0] == 1).all() and (got[2][..., 1:] == 0).all()
        assert torch.equal(got[0], base[0]) and torch.equal(got[3], base[3])
        assert not torch.equal(got[1], base[1])


# ---- the whole path ----------------------------------------------------------------------------------------------------------------
def _model(pkg, model_name, kwargs, sd):
    m = pkg.models_factory[model_name](pkg.MultimodalModelConfig(**kwargs))
    m.load_state_dict(sd, strict=True)
    m.train(False)
    return m.to(DEV)


def _heads(m):
    """(fusion head, layout head, appearance head) as run_attention takes them"""
    if hasattr(m, "fusion_classifier"):
        return m.fusion_classifier, m.layout_classifier, m.appearance_classifier
    return m.classifier, None, None


@functools.lru_cache(maxsize=None)
def _cfg1_reference(model_name):
    """(state dict, batch, golden logits, fp64 restatement) of a cfg1 fusion golden — computed once, shared, never modified"""
    import importlib
    from conftest import PKG_NAME
    synth = importlib.import_module(PKG_NAME + ".synth")
    sd, batch, z = fusion_case(synth, model_name)
    return sd, batch, z, FR.forward_attention(model_name, sd, batch, synth.CONFIGS["cfg1"]["num_attention_heads"])


def _cfg1_kwargs(pkg):
    return dict(pkg.synth.model_kwargs("cfg1"), **EXTRA)


def _masks(batch, A):
    """{map name: bool mask, broadcastable behind the leading layer axes, of the entries that must be exactly 0}"""
    B, T, N = batch["categories"].shape
    kf = batch["src_key_padding_mask_frames"]
    causal = R.masked_entries(kf, True)
    return {"spatial_attention": R.masked_entries(batch["src_key_padding_mask_boxes"].reshape(B * T, N), False).reshape(B, T, N, N),
            "temporal_attention": causal, "fusion_layout_attention": causal, "appearance_to_layout": FR.masked_entries(kf, False, B, A, T)}


def _check_against(pkg, model_name, m, batch, ref, tag):
    """forward_attention within TOL of the restatement, shapes / dtypes as documented, exact zeros, per_head consistency, the ordinary
    forward.  -> (head-averaged outputs, per-head outputs) on the host"""
    dev = _to(batch)
    out = {k: v.cpu() for k, v in m.forward_attention(dev).items()}
    per = {k: v.cpu() for k, v in m.forward_attention(dev, per_head=True).items()}
    assert set(out) == set(per) == set(LOGITS[model_name]) | set(FR.MAP_KEYS)
    assert all(v.dtype == torch.float32 and torch.isfinite(v).all() for v in list(out.values()) + list(per.values()))
    avg = FR.head_mean(ref)
    worst = {}
    for k in FR.MAP_KEYS:
        assert tuple(out[k].shape) == tuple(avg[k].shape) and tuple(per[k].shape) == tuple(ref[k].shape), k
        if out[k].numel() == 0:
            continue
        worst[k] = max((out[k].double() - avg[k]).abs().max().item(), (per[k].double() - ref[k]).abs().max().item())
        assert (out[k] - per[k].mean(dim=-3)).abs().max().item() <= 1e-6, k
    for k in LOGITS[model_name]:
        worst[k] = (out[k].double() - ref[k]).abs().max().item()
        assert torch.equal(out[k], per[k]), k
    print(f"forward_attention {tag}: vs fp64 restatement: " + " ".join(f"{k} {v:.3g}" for k, v in worst.items()))
    assert all(v <= TOL for v in worst.values()), worst
    A = out["appearance_attention"].shape[-1]
    for k, msk in _masks(batch, A).items():
        assert msk.any()
        assert (out[k][..., msk] == 0).all(), k
        hm = msk.unsqueeze(-3).expand(*msk.shape[:-2], per[k].shape[-3], *msk.shape[-2:])
        assert (per[k][..., hm] == 0).all(), k
    with torch.no_grad():
        plain = m(dev)
    for k in LOGITS[model_name]:
        assert (plain[k].cpu() - out[k]).abs().max().item() <= TOL, k
    return out, per


@pytest.mark.parametrize("model_name", ["caf", "cacnf", "lcf"])
def test_forward_attention_cfg1(pkg, model_name):
    """cfg1 fixtures (3 clips, two of them with 2 and 8 padded frames): the restatement, the reference's own weights (caf, cacnf), the
    ordinary forward, and the layout maps bit for bit those of Stlt.forward_attention on the layout branch's weights."""
    sd, batch, z, ref = _cfg1_reference(model_name)
    m = _model(pkg, model_name, _cfg1_kwargs(pkg), sd)
    out, per = _check_against(pkg, model_name, m, batch, ref, f"{model_name} cfg1")
    c = pkg.synth.CONFIGS["cfg1"]
    B, T, N = batch["categories"].shape
    n_fu = 0 if model_name == "lcf" else 2
    assert out["spatial_attention"].shape == (c["num_spatial_layers"], B, T, N, N) and out["temporal_attention"].shape == (c["num_temporal_layers"], B, T, T)
    assert out["appearance_attention"].shape == (2, B, 33, 33) and out["layout_to_appearance"].shape == (n_fu, B, T, 33)
    assert out["appearance_to_layout"].shape == (n_fu, B, 33, T) and out["fusion_layout_attention"].shape == (n_fu, B, T, T)
    assert out["fusion_appearance_attention"].shape == (n_fu, 2, B, 33, 33) and per["fusion_appearance_attention"].shape == (n_fu, 2, B, 4, 33, 33)
    for k in LOGITS[model_name]:
        assert (out[k] - torch.from_numpy(z[k])).abs().max().item() <= TOL, k
    if model_name != "lcf":
        fx = np.load(os.path.join(GOLDEN, f"{model_name}_attention_cfg1.npz"))
        errs = {k: (out[k] - torch.from_numpy(fx[FR.FIXTURE_KEYS[k]])).abs().max().item() for k in FR.MAP_KEYS}
        print(f"forward_attention {model_name} cfg1: vs the reference fixture: " + " ".join(f"{k} {v:.3g}" for k, v in errs.items()))
        assert all(v <= TOL for v in errs.values()), errs
    # the same launches on the same data: an Stlt carrying the layout branch's weights
    stlt = pkg.Stlt(pkg.StltModelConfig(**pkg.synth.model_kwargs("cfg1")))
    pre = {"caf": "caf_backbone.", "cacnf": "backbone.", "lcf": ""}[model_name] + "layout_branch."
    ssd = pkg.synth.make_state_dict({k: tuple(v.shape) for k, v in stlt.state_dict().items()}, seed=3)
    ssd.update({"backbone." + k[len(pre):]: v for k, v in sd.items() if k.startswith(pre)})
    stlt.load_state_dict(ssd, strict=True)
    stlt.train(False).to(DEV)
    dev = _to(batch)
    for per_head, mine in ((False, out), (True, per)):
        want = stlt.forward_attention(dev, per_head=per_head)
        assert torch.equal(want["spatial_attention"].cpu(), mine["spatial_attention"])
        assert torch.equal(want["temporal_attention"].cpu(), mine["temporal_attention"])


@functools.lru_cache(maxsize=None)
def _full_width_state(seed=5):
    import importlib
    from conftest import PKG_NAME
    pkg = importlib.import_module(PKG_NAME)
    kw = dict(pkg.synth.model_kwargs("cfg2"), appearance_num_frames=32)
    m = pkg.CrossAttentionCentralNetFusion(pkg.MultimodalModelConfig(**kw))
    return kw, pkg.synth.make_state_dict({k: tuple(v.shape) for k, v in m.state_dict().items()}, seed=seed)


@pytest.mark.parametrize("name", ["cfg2", "refdef"])
def test_forward_attention_cacnf_full_width(pkg, name):
    """d = 768, 12 heads, the default 4 + 4 appearance / fusion layers, 2 clips, at cfg2's layout shapes (T = 32, N = 7) and the reference's
    defaults (T = 17, N = 5): cross maps of 32 / 17 frames against 33 tokens on the MFMA kernel.  Against the restatement."""
    c = pkg.synth.CONFIGS[name]
    kw, sd = _full_width_state()
    m = _model(pkg, "cacnf", kw, sd)
    batch = pkg.synth.make_batch(2, c["T"], c["N"], seed=8)
    batch["appearance_features"] = pkg.synth.make_appearance_features(2, seed=9)
    ref = FR.forward_attention("cacnf", sd, batch, c["num_attention_heads"])
    out, per = _check_against(pkg, "cacnf", m, batch, ref, f"cacnf {name} full width")
    assert out["layout_to_appearance"].shape == (4, 2, c["T"], 33) and per["appearance_to_layout"].shape == (4, 2, 12, 33, c["T"])


# ---- the C call: NULL sinks, refusals -----------------------------------------------------------------------------------------------
SINKS = ("spatial", "temporal", "appearance", "layout_to_appearance", "appearance_to_layout", "fusion_layout", "fusion_appearance")


def _aligned_ws(nbytes):
    ws = torch.empty(nbytes + 512, dtype=torch.uint8, device=DEV)
    return ws, ws.data_ptr() + (-ws.data_ptr() % 256)


class _CCall:
    """The C-ABI arguments of stlt_caf_forward_attention for CACNF at cfg1 and a device batch, and fresh outputs filled with 7"""

    def __init__(self, pkg, B=3, seed=4):
        self.pkg, self.lib = pkg, pkg._lib.load()
        c = pkg.synth.CONFIGS["cfg1"]
        kw = _cfg1_kwargs(pkg)
        m = pkg.CrossAttentionCentralNetFusion(pkg.MultimodalModelConfig(**kw))
        m.load_state_dict(pkg.synth.make_state_dict({k: tuple(v.shape) for k, v in m.state_dict().items()}, seed=5))
        self.m = m.train(False).to(DEV)
        batch = pkg.synth.make_batch(B, c["T"], c["N"], seed=seed)
        batch["appearance_features"] = pkg.synth.make_appearance_features(B, seed=seed + 1)
        self.batch = _to(batch)
        self.p, self.inp, self.keep, self.feats, (self.B, self.T, self.N, self.Cc, self.S, self.K) = self.m.backbone._native_args(self.batch, *_heads(self.m))
        self.H, self.A = c["num_attention_heads"], self.S + 1
        self.need = int(self.lib.stlt_caf_attention_workspace_bytes(self.B, self.T, self.N, kw["hidden_size"], self.Cc, self.S, self.K))
        self.ws, self.base = _aligned_ws(self.need)
        self.n_sp, self.n_tp = c["num_spatial_layers"], c["num_temporal_layers"]

    def shapes(self, per_head):
        B, T, N, A, hs = self.B, self.T, self.N, self.A, ((self.H,) if per_head else ())
        return dict(zip(SINKS, ((self.n_sp, B, T, *hs, N, N), (self.n_tp, B, *hs, T, T), (2, B, *hs, A, A), (2, B, *hs, T, A), (2, B, *hs, A, T), (2, B, *hs, T, T),
                                (2, 2, B, *hs, A, A))))

    def run(self, per_head=0, skip=(), flags=0, nbytes=None, base=None, expect=0):
        logits = [torch.full((self.B, self.K), 7.0, device=DEV) for _ in range(4)]
        maps = {k: torch.full(sh, 7.0, device=DEV) for k, sh in self.shapes(per_head == 1).items()}  # a refused per_head: the averaged shapes
        sinks = self.pkg._lib.CafAttentionMaps(*[(None if k in skip else maps[k].data_ptr()) for k in SINKS])
        rc = self.lib.stlt_caf_forward_attention(C.byref(self.p), C.byref(self.inp), self.feats.data_ptr(), self.base if base is None else base,
                                                 self.need if nbytes is None else nbytes, flags, per_head, logits[0].data_ptr(), logits[1].data_ptr(),
                                                 logits[2].data_ptr(), logits[3].data_ptr(), C.byref(sinks) if skip != "all" else None, GA.stream())
        assert rc == expect, GA.last_error(self.lib)
        torch.cuda.synchronize()
        return logits, maps


@pytest.mark.parametrize("per_head", [0, 1])
def test_null_sinks_change_nothing_else(pkg, per_head):
    """Each sink NULL in turn through the C-ABI: the other maps and the logits are the same bits, the skipped map is untouched.  All
    sinks NULL (and maps == NULL): the same logits, within TOL of stlt_caf_forward's."""
    cc = _CCall(pkg)
    full_logits, full = cc.run(per_head)
    assert all(not (v == 7.0).any() for v in full.values()) and all(not (v == 7.0).any() for v in full_logits)
    for k in SINKS:
        logits, maps = cc.run(per_head, skip=(k,))
        assert (maps[k] == 7.0).all(), k
        assert all(torch.equal(maps[o], full[o]) for o in SINKS if o != k), k
        assert all(torch.equal(a, b) for a, b in zip(logits, full_logits)), k
    for skip in (SINKS, "all"):
        logits, maps = cc.run(per_head, skip=skip)
        assert all((v == 7.0).all() for v in maps.values())
        assert all(torch.equal(a, b) for a, b in zip(logits, full_logits))
    plain = [torch.full((cc.B, cc.K), 7.0, device=DEV) for _ in range(4)]
    rc = cc.lib.stlt_caf_forward(C.byref(cc.p), C.byref(cc.inp), cc.feats.data_ptr(), cc.base, cc.need, *[t.data_ptr() for t in plain], GA.stream())
    assert rc == 0, GA.last_error(cc.lib)
    torch.cuda.synchronize()
    assert all((a - b).abs().max().item() <= TOL for a, b in zip(plain, full_logits))
    want = cc.m.forward_attention(cc.batch, per_head=bool(per_head))  # the Python call is this C call
    names = dict(zip(SINKS, FR.MAP_KEYS))
    assert all(torch.equal(want[names[k]], full[k]) for k in SINKS) and torch.equal(want["caf"], full_logits[0]) and torch.equal(want["ensemble"], full_logits[3])


def test_whole_path_refusals(pkg):
    """skip-padding, training mode with dropout, a CPU batch (Python); the skip-padding flag, a workspace one byte short, per_head outside
    {0, 1}, a misaligned workspace (C): STLT_EINVAL, nothing written."""
    cc = _CCall(pkg, B=2, seed=1)
    m, lib = cc.m, cc.lib
    m.backbone.layout_branch.skip_padding = True
    with pytest.raises(pkg.StltHipError, match="skip_padding"):
        m.forward_attention(cc.batch)
    m.backbone.layout_branch.skip_padding = False
    with pytest.raises(pkg.StltHipError, match="CPU"):
        m.forward_attention({k: v.cpu() for k, v in cc.batch.items()})
    for model_name in ("caf", "lcf"):
        md = pkg.models_factory[model_name](pkg.MultimodalModelConfig(**dict(_cfg1_kwargs(pkg), hidden_dropout_prob=0.1))).to(DEV)
        md.train(True)
        with pytest.raises(pkg.StltHipError, match="training mode"):
            md.forward_attention(cc.batch)
    assert lib.stlt_caf_attention_workspace_bytes(0, cc.T, cc.N, 256, cc.Cc, cc.S, cc.K) == 0
    for kwargs, word in ((dict(flags=pkg._lib.FLAG_SKIP_PADDING), "SKIP_PADDING"), (dict(nbytes=cc.need - 1), "workspace"), (dict(per_head=2), "per_head"),
                         (dict(per_head=-1), "per_head"), (dict(base=cc.base + 16), "256-byte aligned")):
        logits, maps = cc.run(expect=EINVAL, **kwargs)
        assert word in GA.last_error(lib), (word, GA.last_error(lib))
        assert all((v == 7.0).all() for v in maps.values()) and all((v == 7.0).all() for v in logits)
    # the elision flags are ignored: the same bits as without them
    a = cc.run(0, flags=pkg._lib.FLAG_LAST_ROW_ONLY_TEMPORAL | pkg._lib.FLAG_CLS_ONLY_LAST_SPATIAL)
    b = cc.run(0)
    assert all(torch.equal(x, y) for x, y in zip(a[0], b[0])) and all(torch.equal(a[1][k], b[1][k]) for k in SINKS)


def test_kernel_refusals(pkg):
    """causal with Lq != Lk, a q / k 4 bytes off a 16-byte boundary at head dim 64, ldq / ldk not a multiple of 4 there, lengths 0 and 1025,
    head dim 257, per_head 2, a stride below H * dh: STLT_EINVAL, nothing launched, the output untouched.  The displaced pointer and the odd
    stride are accepted and correct on the vector-ALU kernel (head dim 25).  Every buffer is large enough for the shape named."""
    lib = pkg._lib.load()
    s = GA.stream()
    qb = torch.zeros(64 * 1024, device=DEV)
    kb = torch.zeros(64 * 1024, device=DEV)
    kpm = torch.zeros(2048, dtype=torch.uint8, device=DEV)
    out = torch.full((64 * 1024,), 7.0, device=DEV)
    assert qb.data_ptr() % 16 == 0 and kb.data_ptr() % 16 == 0
    f = lib.stlt_attn_probs_cross_fwd
    q, k, m, o = qb.data_ptr(), kb.data_ptr(), kpm.data_ptr(), out.data_ptr()
    assert f(q, 128, k, 128, m, 1, 2, 7, 9, 2, 64, 0, o, s) == EINVAL and "causal" in GA.last_error(lib)
    for args in ((q + 4, 128, k, 128), (q, 128, k + 4, 128), (q, 130, k, 128), (q, 128, k, 134)):
        assert f(*args, m, 0, 2, 7, 9, 2, 64, 0, o, s) == EINVAL and "aligned" in GA.last_error(lib), args
    assert f(q, 128, k, 128, m, 0, 2, 0, 9, 2, 64, 0, o, s) == EINVAL and f(q, 128, k, 128, m, 0, 1, 7, 1025, 1, 4, 0, o, s) == EINVAL
    assert f(q, 257, k, 257, m, 0, 1, 4, 4, 1, 257, 0, o, s) == EINVAL and "head dim" in GA.last_error(lib)
    assert f(q, 128, k, 128, m, 0, 2, 7, 9, 2, 64, 2, o, s) == EINVAL and f(q, 64, k, 128, m, 0, 2, 7, 9, 2, 64, 0, o, s) == EINVAL
    assert f(None, 128, k, 128, m, 0, 2, 7, 9, 2, 64, 0, o, s) == EINVAL and f(q, 128, k, 128, None, 0, 2, 7, 9, 2, 64, 0, o, s) == EINVAL
    torch.cuda.synchronize()
    assert (out == 7.0).all()
    S, H, dh, Lq, Lk = 3, 4, 25, 9, 70
    d = H * dh
    qh, kh = _rand(S, Lq, d + 1, seed=1, scale=1.5), _rand(S, Lk, d + 3, seed=2, scale=1.5)  # odd strides
    mask = torch.rand(S, Lk, generator=torch.Generator().manual_seed(3)) < 0.3
    mask[:, 0] = False
    qb[1:1 + qh.numel()].copy_(qh.reshape(-1).to(DEV))
    kb[1:1 + kh.numel()].copy_(kh.reshape(-1).to(DEV))
    k8 = mask.to(torch.uint8).to(DEV)
    probs = torch.full((S, H, Lq, Lk), 7.0, device=DEV)
    rc = f(q + 4, d + 1, k + 4, d + 3, k8.data_ptr(), 0, S, Lq, Lk, H, dh, 1, probs.data_ptr(), s)
    assert rc == 0, GA.last_error(lib)
    torch.cuda.synchronize()
    assert (probs.cpu().double() - FR.attn_probs_cross(qh[..., :d].double(), kh[..., :d].double(), mask, False, H, True)).abs().max().item() <= 2e-5


# ---- guard bands -------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def arena():
    a = GA.Arena(768 << 20, DEV)
    yield a
    del a
    torch.cuda.empty_cache()


@pytest.mark.parametrize("per_head", [0, 1])
@pytest.mark.parametrize("S,Lq,Lk", [(3, 7, 33), (3, 33, 17), (2, 65, 33)])
def test_attn_probs_cross_inside_guard_bands(pkg, arena, S, Lq, Lk, per_head):
    """No byte outside probs changes and every element of it is written (a partly filled query block and key block on either side, Lq
    above 64), per head and averaged; q and k are read through their pitch (NaN in the columns behind H * dh)."""
    lib = pkg._lib.load()
    H, dh = 4, 64
    d = H * dh
    qbuf, kbuf, kpm = _kernel_case(S, Lq, Lk, H, dh, 1.5, 7 + Lq)
    kpm[S - 1, :] = True  # a fully masked sequence: its zeros are written, not skipped
    qp, kp = qbuf[..., :d + 4].clone(), kbuf[..., :d + 8].clone()
    qp[..., d:], kp[..., d:] = float("nan"), float("nan")
    shape = (S * H * Lq, Lk) if per_head else (S * Lq, Lk)
    specs = {"q": (qp.contiguous(), "in"), "k": (kp.contiguous(), "in"), "kpm": (kpm.to(torch.uint8), "extent", 0), "probs": (Out(shape), "out")}
    call = lambda o: lib.stlt_attn_probs_cross_fwd(o.q.ptr, d + 4, o.k.ptr, d + 8, o.kpm.ptr, 0, S, Lq, Lk, H, dh, per_head, o.probs.ptr, GA.stream())  # noqa: E731
    got = GA.three_ways(lib, arena, specs, call, ["probs"])["probs"]
    ref = FR.attn_probs_cross(qbuf[..., :d].double(), kbuf[..., :d].double(), kpm, False, H, bool(per_head))
    assert (got.view(ref.shape).double() - ref).abs().max().item() <= 2e-5
    assert (got.view(ref.shape)[S - 1] == 0).all()


@pytest.mark.parametrize("per_head", [0, 1])
def test_forward_attention_inside_guard_bands(pkg, arena, per_head):
    """CACNF at cfg1, B = 3: every input of the batch, the feature map, the workspace (exactly stlt_caf_attention_workspace_bytes), the four
    logits and the seven maps are arena operands; every byte of the eleven outputs is written."""
    cc = _CCall(pkg, B=3, seed=2)
    lib, B, T, N = cc.lib, cc.B, cc.T, cc.N
    host = {k: v.cpu() for k, v in cc.batch.items()}
    want = cc.m.forward_attention(cc.batch, per_head=bool(per_head))
    shapes = cc.shapes(per_head)
    specs = {"categories": (host["categories"], "index", 0), "boxes": (host["boxes"], "in"), "feats": (host["appearance_features"].contiguous(), "in"),
             "kpm_boxes": (host["src_key_padding_mask_boxes"].to(torch.uint8), "extent", 1), "frame_types": (host["frame_types"], "index", 0),
             "kpm_frames": (host["src_key_padding_mask_frames"].to(torch.uint8), "extent", 1), "lengths": (host["lengths"], "extent", 1),
             "workspace": (Out((cc.need,), torch.uint8, must_write=False), "out")}
    specs.update({f"logits{i}": (Out((B, cc.K)), "out") for i in range(4)})
    specs.update({k: (Out((int(np.prod(sh[:-1])), sh[-1])), "out") for k, sh in shapes.items()})

    def call(o):
        inp = pkg._lib.Inputs()
        inp.B, inp.T, inp.N = B, T, N
        inp.categories, inp.boxes, inp.scores, inp.kpm_boxes = o.categories.ptr, o.boxes.ptr, None, o.kpm_boxes.ptr
        inp.frame_types, inp.kpm_frames, inp.lengths = o.frame_types.ptr, o.kpm_frames.ptr, o.lengths.ptr
        sinks = pkg._lib.CafAttentionMaps(*[getattr(o, k).ptr for k in SINKS])
        return lib.stlt_caf_forward_attention(C.byref(cc.p), C.byref(inp), o.feats.ptr, o.workspace.ptr, cc.need, 0, per_head, o.logits0.ptr, o.logits1.ptr,
                                              o.logits2.ptr, o.logits3.ptr, C.byref(sinks), GA.stream())

    outs = [f"logits{i}" for i in range(4)] + list(SINKS)
    got = GA.three_ways(lib, arena, specs, call, outs)
    names = dict(zip(SINKS, FR.MAP_KEYS))
    for k in SINKS:
        assert torch.equal(got[k].view(shapes[k]), want[names[k]].cpu()), k
    for i, k in enumerate(("caf", "stlt", "resnet3d", "ensemble")):
        assert torch.equal(got[f"logits{i}"], want[k].cpu()), k


# ---- determinism and capture ---------------------------------------------------------------------------------------------------------
def test_forward_attention_is_deterministic_and_replays_from_a_graph(pkg):
    """Two eager calls on the cacnf cfg1 golden are the same bits (the head average is summed in registers, no atomics), and one
    single-stream capture replayed twice gives the eager result both times."""
    sd, batch, z, ref = _cfg1_reference("cacnf")
    m = _model(pkg, "cacnf", _cfg1_kwargs(pkg), sd)
    static = _to(batch)
    keys = LOGITS["cacnf"] + FR.MAP_KEYS
    first = {k: v.clone() for k, v in m.forward_attention(static).items()}  # also the warm-up
    second = m.forward_attention(static)
    assert all(torch.equal(first[k], second[k]) for k in keys)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        m.forward_attention(static)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = m.forward_attention(static)
    for _ in range(2):
        for k in keys:
            captured[k].fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        assert all(torch.equal(captured[k], first[k]) for k in keys)
