"""Pixel gradients on the GPU: the thin-input data gradient (stlt_conv3d_bwd_data_thin) against float64 autograd of F.conv3d inside the
guard arena; video.grad through the whole trunk (R3dTrunkFn, stlt_r3d_backward_inputs) against the float64 oracle with the video as a leaf,
with the bilinear identity <video.grad, video> = <stem_weight.grad, stem_weight> that ReLU flips cannot disturb; and forward_saliency of
the five video models against the autograd path of the same model.

Bounds.  Op level: the project's rule for a data gradient (test_r3d_train_gpu.test_conv3d_dgrad_against_float64),
4 · 2^-24 · sqrt(c_out · 343) · max|gradient of the absolute-valued problem|.  Whole trunk and CAF: test_r3d_train_gpu._bound(rel32) · max|g|,
rel32 the larger distance from float64 of two float32 oracle runs (plain, H and W exchanged).  The identity: 8x the float32 oracle's own
relative defect (the factor of _bound), relative to sum|video.grad · video|.  Fusion logits against `forward` (another schedule of the same
arithmetic): 1e-4, the bar of tests/test_layout_gradients_gpu.py; their layout gradients against the autograd path: its CAP of 2e-4.
Every test prints its figures."""
import ctypes
import sys

import pytest
import torch
import torch.nn.functional as F

import guard_arena as GA
from oracle import caf_oracle as CO
from oracle import r3d_oracle as RO
from test_r3d_train_gpu import _bound

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
EPS32 = 2.0 ** -24
CAP = 2e-4
WEIGHT_SEED = 4242


def _report(what, value):
    print(f"\n[pixel gradients] {what}: {value}", file=sys.stderr)


# ---------------------------------------------------------------------------------------------------------------- 1. op level
# (B, T, H, W, c_out), all 7x7x7, stride (1, 2, 2), pad 3, c_in = 3
THIN = {
    "odd_hw": (1, 5, 9, 11, 64),        # odd H and W: the four classes have different row counts
    "even_batch2": (2, 4, 8, 10, 64),   # even extents, batch stride
    "below_window": (1, 1, 2, 3, 64),   # every extent smaller than the tap window
    "cout24": (1, 3, 7, 6, 24),         # c_out other than 64 (a chunk zero-filled to 32 channels)
    "tiles": (1, 2, 33, 18, 64),        # 17 x 9 blocks: three 8-row tiles, the last with one row, and a partial 16-column tile
}
STRIDE, PAD = (1, 2, 2), (3, 3, 3)


@pytest.fixture(scope="module")
def arena():
    return GA.Arena(8 << 20)


def _thin_case(case):
    B, T, H, W, Co = THIN[case]
    g = torch.Generator().manual_seed(3100 + sorted(THIN).index(case))
    w = torch.randn(Co, 3, 7, 7, 7, generator=g) * (2.0 / (3 * 343)) ** 0.5
    scale = 0.5 + torch.rand(Co, generator=g)
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    dy = torch.randn(B, Co, T, Ho, Wo, generator=g)
    return (B, T, H, W, Co), w, scale, dy


def _ref64(shape, w, scale, dy, absval=False):
    B, T, H, W, Co = shape
    ws = w.double() * scale.double().view(-1, 1, 1, 1, 1)  # weights pre-multiplied by the per-c_out scale
    dyd = dy.double()
    if absval:
        ws, dyd = ws.abs(), dyd.abs()
    x = torch.zeros(B, 3, T, H, W, dtype=torch.float64, requires_grad=True)
    (dx,) = torch.autograd.grad(F.conv3d(x, ws, stride=STRIDE, padding=PAD), x, dyd)
    return dx


def _thin_specs(shape, w, scale, dy, layout):
    B, T, H, W, Co = shape
    dx = GA.Out((B, 3, T, H, W)) if layout else GA.Out((B, T, H, W, 4))
    return {"w": (w.contiguous(), "in"), "scale": (scale, "in"), "wt": (GA.Out((1792 * Co,)), "out"), "dy": (dy.permute(0, 2, 3, 4, 1).contiguous(), "in"),
            "dx": (dx, "out")}


@pytest.mark.parametrize("case", sorted(THIN))
def test_thin_dgrad_against_float64_inside_guard_bands(pkg, arena, case):
    shape, w, scale, dy = _thin_case(case)
    B, T, H, W, Co = shape
    lib = pkg._lib.load()
    d = pkg._lib.Conv3dDesc(B, T, H, W, 3, Co, 7, 7, 7, *STRIDE, *PAD)
    assert int(lib.stlt_conv3d_repack_dgrad_thin_floats(ctypes.byref(d))) == 1792 * Co

    def call(layout):
        def run(o):
            rc = lib.stlt_conv3d_repack_dgrad_thin(o.w.ptr, ctypes.byref(d), o.scale.ptr, o.wt.ptr, GA.stream())
            return rc or lib.stlt_conv3d_bwd_data_thin(ctypes.byref(d), o.dy.ptr, o.wt.ptr, o.dx.ptr, layout, GA.stream())
        return run

    # plain tensors, inside the arena, inside the arena again: bands untouched, every dx element written, the three runs bit-identical
    ndhwc = GA.three_ways(lib, arena, _thin_specs(shape, w, scale, dy, 0), call(0), ("dx", "wt"))
    ncdhw = GA.three_ways(lib, arena, _thin_specs(shape, w, scale, dy, 1), call(1), ("dx",))
    got = ncdhw["dx"].double()
    ref, mag = _ref64(shape, w, scale, dy), _ref64(shape, w, scale, dy, absval=True)
    tol = 4 * EPS32 * (Co * 343) ** 0.5 * mag.max().item()
    err = (got - ref).abs().max().item()
    _report(f"thin dgrad {case} {shape}: max|got - float64| / tol", f"{err:.3e} / {tol:.3e} = {err / tol:.3f}")
    assert err <= tol, (case, err, tol)
    # both layouts: the same bits on the three real channels, the padded channel stored as exactly 0
    assert torch.equal(ndhwc["dx"][..., :3].permute(0, 4, 1, 2, 3), ncdhw["dx"]), case
    assert torch.equal(ndhwc["dx"][..., 3], torch.zeros(B, T, H, W)), case
    # the thin copy: 3/4 of the columns and, of those, 49/64 of the (jh, jw) taps are real
    wt = ndhwc["wt"].view(7, 4, 4, Co // 4, 16, 4)
    assert torch.equal(wt[..., 3::4, :], torch.zeros_like(wt[..., 3::4, :]))
    assert int((wt != 0).sum()) == 7 * 49 * 3 * Co
    # dy 16 bytes into its slot is accepted (same bits); dy or the copy off a 16-byte boundary is refused and nothing is launched
    specs = _thin_specs(shape, w, scale, dy, 1)
    specs["wt"] = (ndhwc["wt"].contiguous(), "in")
    only = lambda o: lib.stlt_conv3d_bwd_data_thin(ctypes.byref(d), o.dy.ptr, o.wt.ptr, o.dx.ptr, 1, GA.stream())  # noqa: E731
    moved = GA.misaligned(lib, arena, specs, only, ("dx",), operand="dy", mis=16)
    assert torch.equal(moved["dx"], ncdhw["dx"]), case
    assert GA.misaligned(lib, arena, specs, only, ("dx",), operand="dy", mis=4, refused_as="dy") is None
    assert GA.misaligned(lib, arena, specs, only, ("dx",), operand="wt", mis=8, refused_as="w_dgrad_thin") is None


# ---------------------------------------------------------------------------------------------------------------- 2. whole trunk
TRUNK_SHAPES = [(1, 8, 64, 64),   # T = 1 at layer 4
                (2, 9, 49, 35)]   # stem output 25 x 18, odd extents below


def _app_cfg(pkg, frames, **extra):
    kw = pkg.synth.model_kwargs("cfg1")
    return pkg.AppearanceModelConfig(num_classes=kw["num_classes"], hidden_size=kw["hidden_size"], num_attention_heads=kw["num_attention_heads"],
                                     hidden_dropout_prob=0.0, appearance_num_frames=frames, train_trunk=True, **extra)


def _load(pkg, m, seed=WEIGHT_SEED):
    sd = pkg.synth.make_r3d_state_dict({k: tuple(v.shape) for k, v in m.state_dict().items()}, seed=seed)
    m.load_state_dict(sd, strict=True)
    return m.to(DEV), sd


@pytest.fixture(scope="module")
def trunk_model(pkg):
    m, sd = _load(pkg, pkg.Resnet3D(_app_cfg(pkg, 32)))
    return m.train(True), sd


def _features(m, v):
    return m._runner.run(m.resnet, v, features=True)[0]


def _pooled(m, v):
    return m._runner.run(m.resnet, v, features=False, pooled=True)[1]


def _oracle_video_grad(sd, video, dfeat, dpool, dtype, swap=False, with_stem=False):
    """d(<features, dfeat> + <pooled, dpool>)/d video by torch autograd through the oracle trunk in ``dtype``; ``swap``: the same problem
    with H and W exchanged (another float32 summation order), the result exchanged back."""
    sdd = {k: (v.to(dtype) if v.is_floating_point() else v) for k, v in sd.items()}
    v, df = video.to(dtype).clone(), dfeat.to(dtype)  # clones: .to() of the same dtype hands back the caller's own tensor
    if swap:
        sdd = {k: (t.transpose(-1, -2).contiguous() if t.dim() == 5 else t) for k, t in sdd.items()}
        v, df = v.transpose(-1, -2).contiguous(), df.transpose(-1, -2).contiguous()
    v.requires_grad_(True)
    stem = sdd["resnet.0.weight"].clone().requires_grad_(True)  # a private leaf: .to() of the same dtype hands back the fixture's own tensor
    sdd["resnet.0.weight"] = stem
    feats = RO.trunk_forward(sdd, v)
    loss = (feats * df).sum() + (feats.mean(dim=(2, 3, 4)) * dpool.to(dtype)).sum()
    gv, gw = torch.autograd.grad(loss, (v, stem))
    if swap:
        gv, gw = gv.transpose(-1, -2), gw.transpose(-1, -2)
    return (gv, gw.detach(), stem.detach().transpose(-1, -2) if swap else stem.detach()) if with_stem else gv


def _seeds(pkg, shape):
    B, T, H, W = shape
    r = pkg.modelling.resnet3d
    To, Ho, Wo = r._trunk_out(T), r._trunk_out(H, 2), r._trunk_out(W, 2)
    g = torch.Generator().manual_seed(900 + TRUNK_SHAPES.index(shape))
    # positive seeded gradients on both outputs, as test_r3d_shapes_gpu.test_trunk_weight_gradients_against_float64 forms them
    return torch.rand(B, 2048, To, Ho, Wo, generator=g), torch.rand(B, 2048, generator=g) * (To * Ho * Wo) ** 0.5


def _identity_defect(gv, v, gw, w):
    a, b = (gv.double() * v.double()).sum().item(), (gw.double() * w.double()).sum().item()
    return abs(a - b) / (gv.double() * v.double()).abs().sum().item()


@pytest.mark.parametrize("shape", TRUNK_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_trunk_video_gradient_against_float64(pkg, trunk_model, shape):
    m, sd = trunk_model
    video = pkg.synth.make_video(*shape, seed=700 + TRUNK_SHAPES.index(shape))
    dfeat, dpool = _seeds(pkg, shape)
    want = _oracle_video_grad(sd, video, dfeat, dpool, torch.float64)
    r32, gw32, w32 = _oracle_video_grad(sd, video, dfeat, dpool, torch.float32, with_stem=True)
    r32_t = _oracle_video_grad(sd, video, dfeat, dpool, torch.float32, swap=True)
    gmax = want.abs().max().item()
    rel32 = max((r32.double() - want).abs().max().item(), (r32_t.double() - want).abs().max().item()) / gmax
    bound = _bound(rel32)
    ws = [conv.weight for conv, _ in pkg.modelling.resnet3d.trunk_convs(m.resnet)]
    df, dp = dfeat.to(DEV), dpool.to(DEV)

    def passes(with_video, weights=True):
        v = video.to(DEV).requires_grad_(with_video)
        wanted = ([v] if with_video else []) + (ws if weights else [])
        gf = torch.autograd.grad(_features(m, v), wanted, df)
        gp = torch.autograd.grad(_pooled(m, v), wanted, dp)
        return v, gf, gp

    v, gf, gp = passes(True)
    got = (gf[0] + gp[0]).cpu().double()
    err = (got - want).abs().max().item() / gmax
    _report(f"trunk video.grad {shape}: err / max|g|, float32 oracle rel32, bound", f"{err:.3e}, {rel32:.3e}, {bound:.3e}")
    assert tuple(gf[0].shape) == tuple(video.shape)
    assert err <= bound, (shape, err, bound, rel32)
    # the identity no ReLU flip disturbs: on one pass, <video.grad, video> = <stem_weight.grad, stem_weight> (both are <G, BN-scaled conv(video)>)
    d_gpu = _identity_defect((gf[0] + gp[0]).cpu(), video, (gf[1] + gp[1]).cpu(), ws[0].detach().cpu())
    d_32 = _identity_defect(r32, video, gw32, w32)
    _report(f"trunk {shape}: identity defect GPU, float32 oracle, allowed", f"{d_gpu:.3e}, {d_32:.3e}, {8 * d_32:.3e}")
    assert d_gpu <= 8 * d_32, (shape, d_gpu, d_32)
    # asking for video.grad leaves the 53 weight gradients bit for bit as they are without it; two passes are bit-identical
    _, gf0, gp0 = passes(False)
    assert all(torch.equal(a, b) for a, b in zip(gf[1:], gf0)) and all(torch.equal(a, b) for a, b in zip(gp[1:], gp0)), "weight gradients moved"
    _, gf2, gp2 = passes(True)
    assert all(torch.equal(a, b) for a, b in zip(gf, gf2)) and all(torch.equal(a, b) for a, b in zip(gp, gp2)), "two passes differ"
    # a frozen trunk: the same video.grad bit for bit, from the input-only sweep (no weight-gradient launch in the recorder)
    m.resnet.requires_grad_(False)
    try:
        passes(True, weights=False)  # copies and buffers
        torch.cuda.synchronize()
        pkg.ops.prof_enable(True)
        try:
            pkg.ops.prof_launches()
            _, gff, gpf = passes(True, weights=False)
            torch.cuda.synchronize()
            launches = pkg.ops.prof_launches()
        finally:
            pkg.ops.prof_enable(False)
            pkg.ops.prof_collect()
    finally:
        for conv, _ in pkg.modelling.resnet3d.trunk_convs(m.resnet):
            conv.weight.requires_grad_(True)
    assert torch.equal(gff[0], gf[0]) and torch.equal(gpf[0], gp[0]), "frozen trunk: another video.grad"
    assert not [l["note"] for l in launches if "wgrad" in l["note"]], "the input-only sweep launched a weight gradient"
    assert sum(l["kernel"] == "conv_dgrad_thin" for l in launches) == 2 and any("conv3d_igemm_kernel<bwd>" in l["note"] for l in launches)


# ---------------------------------------------------------------------------------------------------------------- 3. models
VIDEO = (2, 16, 64, 64)   # trunk output (1, 2, 2): 4 appearance tokens
FRAMES = 4
SMALL = dict(num_spatial_layers=2, num_temporal_layers=1, num_appearance_layers=1, num_fusion_layers=1)


def _video(pkg, seed=801):
    return pkg.synth.make_video(*VIDEO, seed=seed).to(DEV)


def _recorded(pkg, fn):
    torch.cuda.synchronize()
    pkg.ops.prof_enable(True)
    try:
        pkg.ops.prof_launches()
        out = fn()
        torch.cuda.synchronize()
        launches = pkg.ops.prof_launches()
    finally:
        pkg.ops.prof_enable(False)
        pkg.ops.prof_collect()
    return out, launches


def _check_saliency(pkg, m, batch, names, grads, head=None, trunk=True, bitwise_trainable=True):
    """The checks every model shares.  batch: device tensors; grads: {output key: batch key} of the input gradients to compare.
    bitwise_trainable: the appearance gradient equals the autograd path's bit for bit with every parameter trainable (the video models).
    The block Functions of the fusion models' cross-modal layers run other kernels for an input gradient when weight and bias gradients are
    formed beside it (measured: 1.0e-6 of max|g| on CAF / CACNF, 0 on LCF, which has no such layer), so there the bitwise comparison is
    against the autograd path of the same model with its parameters frozen — the same launches — and the trainable path is held to CAP."""
    head_name = names[-1] if head is None else head
    kw = {} if head is None else {"head": head}
    with torch.no_grad():
        fwd = m(batch)
    assert all(q.grad is None for q in m.parameters())
    r, launches = _recorded(pkg, lambda: m.forward_saliency(batch, **kw))
    assert set(r) == set(names) | {"target"} | set(grads), sorted(r)
    assert all(q.grad is None for q in m.parameters()), "forward_saliency created a parameter gradient"
    for n in names:
        diff = (r[n] - fwd[n]).abs().max().item()
        _report(f"{type(m).__name__} {n}: max|forward_saliency - forward|", f"{diff:.3e}")
        assert diff <= 1e-4, (n, diff)
    assert not [l["note"] for l in launches if "wgrad" in l["note"]], "forward_saliency launched a trunk weight gradient"
    assert sum(l["kernel"] == "conv_dgrad_thin" for l in launches) == (1 if trunk else 0)
    if not trunk:
        assert not [l["note"] for l in launches if "conv3d" in l["note"] or "maxpool" in l["note"]], "a trunk launch without video_frames"
    assert r["target"].dtype == torch.int64 and torch.equal(r["target"], r[head_name].argmax(dim=1))
    # the three target forms: top-1, that class as int64, its one-hot row as a float seed
    onehot = F.one_hot(r["target"], r[head_name].shape[1]).float()
    by_index, by_seed = m.forward_saliency(batch, target=r["target"], **kw), m.forward_saliency(batch, target=onehot, **kw)
    assert by_seed["target"] is onehot
    for k in grads:
        assert torch.equal(by_index[k], r[k]) and torch.equal(by_seed[k], r[k]), k
    # the autograd path of the same model, every parameter trainable: this one does fill the parameters' .grad
    leaves = {bk: batch[bk].detach().clone().requires_grad_(True) for bk in grads.values()}
    out = m(dict(batch, **leaves))[head_name]
    out.gather(1, r["target"].view(-1, 1)).sum().backward()
    assert any(q.grad is not None for q in m.parameters())
    m.zero_grad(set_to_none=True)
    for k, bk in grads.items():
        g = leaves[bk].grad
        assert g is not None and tuple(r[k].shape) == tuple(batch[bk].shape), k
        diff = (r[k] - g).abs().max().item() / max(g.abs().max().item(), 1e-30)
        _report(f"{type(m).__name__} {k}: max|forward_saliency - autograd path| / max|autograd|", f"{diff:.3e}")
        if bk in ("video_frames", "appearance_features") and bitwise_trainable:
            assert torch.equal(r[k], g), (k, diff)
        else:
            assert diff <= CAP, (k, diff)
        assert g.abs().max().item() > 0, k
    if not bitwise_trainable:
        was = [(q, q.requires_grad) for q in m.parameters()]
        try:
            for q, _ in was:
                q.requires_grad_(False)
            leaves = {bk: batch[bk].detach().clone().requires_grad_(True) for bk in grads.values()}
            m(dict(batch, **leaves))[head_name].gather(1, r["target"].view(-1, 1)).sum().backward()
        finally:
            for q, flag in was:
                q.requires_grad_(flag)
        for k, bk in grads.items():
            assert torch.equal(r[k], leaves[bk].grad), f"{k}: forward_saliency differs from the frozen model's autograd path"
    return r


@pytest.mark.parametrize("name", ["resnet3d", "resnet3d-transformer"])
def test_video_models_forward_saliency(pkg, name):
    m, _ = _load(pkg, pkg.models_factory[name](_app_cfg(pkg, FRAMES, num_appearance_layers=2)))
    m.train(False)
    batch = {"video_frames": _video(pkg)}
    _check_saliency(pkg, m, batch, ("resnet3d",), {"video_frames_grad": "video_frames"})
    assert torch.equal(m.forward_saliency(batch)["video_frames_grad"], m.forward_saliency(batch)["video_frames_grad"])
    if name == "resnet3d-transformer":  # the appearance encoder's dropout is live in training mode (Resnet3D has none)
        m.train(True)
        with pytest.raises(pkg._lib.StltHipError, match="training mode with dropout"):
            m.forward_saliency(batch)
        m.train(False)
    with pytest.raises(pkg._lib.StltHipError, match="GPU"):
        m.forward_saliency({"video_frames": batch["video_frames"].cpu()})


def _fusion(pkg, name, dropout=0.0):
    kw = dict(pkg.synth.model_kwargs("cfg1"), **SMALL, appearance_num_frames=FRAMES, appearance_trunk=True, train_trunk=True)
    kw["hidden_dropout_prob"] = dropout
    m, sd = _load(pkg, pkg.models_factory[name](pkg.MultimodalModelConfig(**kw)))
    return m.train(False), sd, kw


def _fusion_batch(pkg, with_scores=True):
    B = VIDEO[0]
    batch = pkg.synth.make_batch(B, 16, 4, seed=1619, min_len=2, with_scores=with_scores)
    return {k: v.to(DEV) for k, v in batch.items()}, batch


@pytest.mark.parametrize("name", ["caf", "cacnf", "lcf"])
def test_fusion_models_forward_saliency(pkg, name):
    m, sd, kw = _fusion(pkg, name)
    dev, _ = _fusion_batch(pkg)
    names = m.logit_names
    lay = {"boxes_grad": "boxes", "scores_grad": "scores"}
    _check_saliency(pkg, m, dict(dev, video_frames=_video(pkg)), names, dict(lay, video_frames_grad="video_frames"), bitwise_trainable=False)
    # precomputed features instead of frames: their gradient, and no trunk launch
    feats = pkg.synth.make_appearance_features(VIDEO[0], seed=1620, grid=(1, 2, 2)).to(DEV)
    _check_saliency(pkg, m, dict(dev, appearance_features=feats), names, dict(lay, appearance_features_grad="appearance_features"), trunk=False,
                    bitwise_trainable=False)
    if name == "cacnf":  # another head than the default: the layout head never reads the video
        r = m.forward_saliency(dict(dev, video_frames=_video(pkg)), head="stlt")
        assert r["video_frames_grad"].abs().max().item() == 0 and r["boxes_grad"].abs().max().item() > 0
        with pytest.raises(pkg._lib.StltHipError, match="head must be one of"):
            m.forward_saliency(dict(dev, video_frames=_video(pkg)), head="lcf")
    m.train(True)
    with pytest.raises(pkg._lib.StltHipError, match="training mode with dropout"):
        m.forward_saliency(dict(dev, video_frames=_video(pkg)))


def test_caf_video_gradient_against_float64(pkg):
    m, sd, kw = _fusion(pkg, "caf")
    dev, host = _fusion_batch(pkg)
    video = pkg.synth.make_video(*VIDEO, seed=801)
    H = kw["num_attention_heads"]
    labels = torch.tensor([3, 100])
    pre = "caf_backbone.appearance_branch.resnet.resnet."

    def oracle(dtype, swap=False):
        cast = lambda t: t.to(dtype) if t.is_floating_point() else t  # noqa: E731
        sdd = {k: cast(v.detach()) for k, v in sd.items()}
        trunk = {k[len(pre) - len("resnet."):]: v for k, v in sdd.items() if k.startswith(pre)}
        v = video.to(dtype).clone()
        if swap:
            trunk = {k: (t.transpose(-1, -2).contiguous() if t.dim() == 5 else t) for k, t in trunk.items()}
            v = v.transpose(-1, -2).contiguous()
        v.requires_grad_(True)
        feats = RO.trunk_forward(trunk, v)
        if swap:
            feats = feats.transpose(-1, -2)
        b = {k: cast(t) for k, t in host.items()}
        b["appearance_features"] = feats
        logits = CO.caf_forward(sdd, b, H, dtype=dtype)["caf"]
        (g,) = torch.autograd.grad(logits.gather(1, labels.view(-1, 1)).sum(), v)
        return g.transpose(-1, -2) if swap else g

    want = oracle(torch.float64)
    gmax = want.abs().max().item()
    rel32 = max((oracle(torch.float32).double() - want).abs().max().item(), (oracle(torch.float32, swap=True).double() - want).abs().max().item()) / gmax
    bound = _bound(rel32)
    v = video.to(DEV).requires_grad_(True)
    m(dict(dev, video_frames=v))["caf"].gather(1, labels.to(DEV).view(-1, 1)).sum().backward()
    err = (v.grad.cpu().double() - want).abs().max().item() / gmax
    _report("CAF video.grad (autograd path) err / max|g|, float32 oracle rel32, bound", f"{err:.3e}, {rel32:.3e}, {bound:.3e}")
    assert err <= bound, (err, bound, rel32)
    sal = m.forward_saliency(dict(dev, video_frames=video.to(DEV)), target=labels.to(DEV))
    diff = (sal["video_frames_grad"] - v.grad).abs().max().item() / v.grad.abs().max().item()  # trainable path: other kernels (see _check_saliency)
    assert diff <= CAP, diff


def test_video_without_grad_runs_todays_launches(pkg, trunk_model):
    """A batch whose video does not require grad: the launches of the training pass are the parent's (stlt_r3d_train_forward, then
    stlt_r3d_backward: per conv a weight gradient and, but for the stem, a data gradient; no thin launch), and a frozen model under autograd
    runs the tapeless forward as before."""
    m, _ = trunk_model
    v = _video(pkg)
    ws = [conv.weight for conv, _ in pkg.modelling.resnet3d.trunk_convs(m.resnet)]
    labels = torch.tensor([1, 2], device=DEV)
    run = lambda: torch.autograd.grad(F.cross_entropy(m({"video_frames": v})["resnet3d"], labels), ws)  # noqa: E731
    base = run()
    grads, launches = _recorded(pkg, run)
    notes = [l["note"] for l in launches]
    assert all(torch.equal(a, b) for a, b in zip(base, grads))
    assert not any(l["kernel"] == "conv_dgrad_thin" for l in launches)
    assert sum("conv3d_wgrad_kernel" in n for n in notes) == 53 and sum("conv3d_wgrad_finish_kernel" in n for n in notes) == 53
    assert sum("maxpool3d_bwd_kernel" in n for n in notes) == 1 and sum("r3d_grad_in_kernel" in n for n in notes) == 1
    # the same pass with video.grad: the same 53 gradients, one more launch at the end
    vg = v.clone().requires_grad_(True)
    both, launches_v = _recorded(pkg, lambda: torch.autograd.grad(F.cross_entropy(m({"video_frames": vg})["resnet3d"], labels), [vg] + ws))
    assert all(torch.equal(a, b) for a, b in zip(base, both[1:]))
    extra = [l for l in launches_v if l["kernel"] == "conv_dgrad_thin"]
    assert len(extra) == 1 and len(launches_v) >= len(launches) + 1
    # frozen, grad enabled, no video grad: no tape
    m.resnet.requires_grad_(False)
    try:
        with torch.no_grad():
            want = m({"video_frames": v})["resnet3d"]
        out, launches_f = _recorded(pkg, lambda: m({"video_frames": v})["resnet3d"])
    finally:
        for w in ws:
            w.requires_grad_(True)
    assert torch.equal(out, want) and not any("argmax" in l["note"] for l in launches_f)
