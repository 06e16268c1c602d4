"""Class activation maps on the GPU.  Op level: stlt_cam_weights, stlt_cam_map and stlt_cam_upsample inside guard bands, three ways, with
offset and misaligned pointers, against tests/gradcam_restated.py in float64 within the worst case of the float32 sums; the refusals of
stlt_r3d_backward_layer.  End to end: Resnet3D.forward_gradcam against the classic CAM closed form at the last stage and against the fp64
oracle's autograd below it (the gradient at the stage as well), the bit-for-bit composition of every model's call from the public pieces,
the other outputs, the refusals and the perturbation runner."""
import ctypes
import sys

import numpy as np
import pytest
import torch

import gradcam_restated as R
import guard_arena as GA
import test_pixel_gradients_gpu as PG
from guard_arena import Out
from oracle import r3d_oracle as O
from test_r3d_train_gpu import _bound

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
EINVAL, EWORKSPACE = -1, -2
U = 2.0 ** -24
LAYOUTS = {"ndhwc": 0, "ncdhw": 1}
PS, CS = (1, 5, 33, 1000), (1, 12, 70, 256)  # 33 and 1000 cross the 32-position partition; 12 and 256 take the 16-byte path, 1 and 70 cannot
SHAPES = [(1, 8, 64, 64), (3, 9, 97, 75)]
_CACHE = {}


def _report(what, value):
    print(f"\n[gradcam] {what}: {value}", file=sys.stderr)


@pytest.fixture(scope="module")
def arena():
    return GA.Arena(48 << 20)


def _ag(B, P, C, layout, seed):
    """activations and gradients of (B, P, C) in `layout`, off the unit scale and with both signs"""
    g = torch.Generator().manual_seed(seed)
    shape = (B, P, C) if layout == "ndhwc" else (B, C, P)
    return torch.randn(shape, generator=g) * 3.0, torch.randn(shape, generator=g) * 0.01 + 0.002


# ------------------------------------------------------------------------------------------------------------------ 1. stlt_cam_weights
@pytest.mark.parametrize("layout", list(LAYOUTS))
@pytest.mark.parametrize("C", CS)
@pytest.mark.parametrize("P", PS)
def test_cam_weights_inside_guard_bands(pkg, arena, P, C, layout):
    lib = pkg._lib.load()
    B = 3
    _, g = _ag(B, P, C, layout, 100 + P + C)
    need = lib.stlt_cam_scratch_bytes(B, P, C)
    assert need == (B * -(-P // 32) * C * 4 if P > 32 else 0)
    specs = {"g": (g, "in"), "alpha": (Out((B, C)), "out"), "scratch": (Out((max(need // 4, 1),), must_write=False), "out")}

    def call(o):
        return lib.stlt_cam_weights(o.g.ptr, B, P, C, LAYOUTS[layout], o.alpha.ptr, o.scratch.ptr, need, GA.stream())

    want, bound = R.weights(g.numpy(), layout)
    got = {}
    for tag, mis in (("aligned", None), ("offset", {"g": 16, "alpha": 32}), ("misaligned", {"g": 4, "alpha": 12})):
        got[tag] = GA.three_ways(lib, arena, specs, call, ["alpha"], misalign=mis)["alpha"]  # three_ways: run to run bit for bit
        err = np.abs(got[tag].double().numpy() - want)
        _report(f"cam_weights {layout} P={P} C={C} {tag}: worst err / bound", f"{(err / np.maximum(bound, 1e-300)).max():.3g}")
        assert (err <= bound).all(), (tag, float((err / bound).max()))
    # one summation order per channel, whichever width the loads have
    assert torch.equal(got["aligned"], got["offset"]) and torch.equal(got["aligned"], got["misaligned"])
    # clip 1 alone gives the bits of clip 1 in the batch
    gd = g.to(DEV)
    assert torch.equal(pkg.ops.cam_weights(gd[1:2].contiguous(), layout)[0], pkg.ops.cam_weights(gd, layout)[1])
    assert torch.equal(pkg.ops.cam_weights(gd, layout).cpu(), got["aligned"])


def test_cam_weights_refusals(pkg, arena):
    lib = pkg._lib.load()
    g = torch.zeros(2, 40, 8, device=DEV)
    alpha, scratch = torch.empty(2, 8, device=DEV), torch.empty(2 * 2 * 8, device=DEV)
    assert lib.stlt_cam_weights(g.data_ptr(), 2, 40, 8, 0, alpha.data_ptr(), scratch.data_ptr(), scratch.numel() * 4 - 1, None) == EWORKSPACE
    assert lib.stlt_cam_weights(g.data_ptr(), 2, 40, 8, 0, alpha.data_ptr(), scratch.data_ptr() + 4, scratch.numel() * 4, None) == EWORKSPACE
    assert lib.stlt_cam_weights(g.data_ptr(), 2, 40, 8, 0, alpha.data_ptr(), None, 0, None) == EWORKSPACE
    assert lib.stlt_cam_weights(g.data_ptr() + 2, 2, 40, 8, 1, alpha.data_ptr(), None, 0, None) == EINVAL and "aligned" in GA.last_error(lib)
    assert lib.stlt_cam_weights(g.data_ptr(), 2, 40, 8, 3, alpha.data_ptr(), None, 0, None) == EINVAL and "layout" in GA.last_error(lib)
    assert lib.stlt_cam_weights(g.data_ptr(), 2, 40, 8, 1, alpha.data_ptr(), None, 0, None) == 0  # NCDHW needs no scratch
    with pytest.raises(pkg.StltHipError, match="layout"):
        pkg.ops.cam_weights(g, "nchw")


# ---------------------------------------------------------------------------------------------------------------------- 2. stlt_cam_map
@pytest.mark.parametrize("layout", list(LAYOUTS))
@pytest.mark.parametrize("per", [0, 1], ids=["gradcam", "hirescam"])
@pytest.mark.parametrize("C", CS)
@pytest.mark.parametrize("P", PS)
def test_cam_map_inside_guard_bands(pkg, arena, P, C, per, layout):
    lib = pkg._lib.load()
    B = 3
    a, g = _ag(B, P, C, layout, 300 + P + C)
    w = g if per else torch.randn(B, C, generator=torch.Generator().manual_seed(P + C)) * 0.02
    specs = {"a": (a, "in"), "w": (w, "in"), "cam": (Out((B, P)), "out")}
    res = {}
    for relu in (0, 1):
        def call(o):
            return lib.stlt_cam_map(o.a.ptr, o.w.ptr, per, B, P, C, LAYOUTS[layout], relu, o.cam.ptr, GA.stream())

        want, bound = R.cam_map(a.numpy(), w.numpy(), layout, bool(relu))
        for tag, mis in (("aligned", None), ("misaligned", {"a": 4, "w": 8, "cam": 12})):
            got = GA.three_ways(lib, arena, specs, call, ["cam"], misalign=mis)["cam"]
            err = np.abs(got.double().numpy() - want)
            _report(f"cam_map {layout} P={P} C={C} per_element={per} relu={relu} {tag}: worst err / bound", f"{(err / np.maximum(bound, 1e-300)).max():.3g}")
            assert (err <= bound).all(), (tag, relu, float((err / bound).max()))
            res[relu, tag] = got
    for tag in ("aligned", "misaligned"):
        raw, pos = res[0, tag], res[1, tag]
        assert P < 33 or (raw < 0).any()
        # the positive part: never negative, the signed value's bits where it is positive and +0 everywhere else
        assert not torch.signbit(pos).any()
        assert torch.equal(pos.view(torch.int32), torch.where(raw > 0, raw, torch.zeros_like(raw)).view(torch.int32))


def test_cam_map_refusals(pkg):
    lib = pkg._lib.load()
    a, w, cam = torch.zeros(2, 6, 8, device=DEV), torch.zeros(2, 8, device=DEV), torch.empty(2, 6, device=DEV)
    assert lib.stlt_cam_map(a.data_ptr(), w.data_ptr(), 0, 2, 6, 8, 0, 1, cam.data_ptr() + 2, None) == EINVAL and "aligned" in GA.last_error(lib)
    assert lib.stlt_cam_map(a.data_ptr(), None, 0, 2, 6, 8, 0, 1, cam.data_ptr(), None) == EINVAL and "null" in GA.last_error(lib)
    assert lib.stlt_cam_map(a.data_ptr(), w.data_ptr(), 0, 2, 0, 8, 0, 1, cam.data_ptr(), None) == EINVAL
    with pytest.raises(pkg.StltHipError, match="channel weights"):
        pkg.ops.cam_map(a, torch.zeros(2, 7, device=DEV))
    assert tuple(pkg.ops.cam_map(a.view(2, 1, 2, 3, 8), w).shape) == (2, 1, 2, 3) and tuple(pkg.ops.cam_map(a.view(2, 6, 2, 2, 2), torch.zeros(2, 6, device=DEV), "ncdhw").shape) == (2, 2, 2, 2)


# ----------------------------------------------------------------------------------------------------------------- 3. stlt_cam_upsample
@pytest.mark.parametrize("grid,size", [((1, 2, 3), (5, 4, 7)), ((2, 4, 4), (32, 112, 112))])
def test_cam_upsample_inside_guard_bands(pkg, arena, grid, size):
    """Against the float64 restatement within gradcam_restated.upsample_bound: per axis the source coordinate carries three float32
    roundings of numbers up to the grid's extent `in`, the lower weight one more, so a weight is off by at most (3 in + 1) 2^-24; the blend
    is continuous and piecewise linear in the coordinate, so that moves a blend of values up to M = max|cam| by (2 (3 in + 1) + 1) 2^-24 M
    per axis; each axis adds two products and a sum, 9 roundings over the three levels: (18 in + 18) 2^-24 M in all."""
    lib = pkg._lib.load()
    B = 2
    cam = torch.randn(B, *grid, generator=torch.Generator().manual_seed(7)) * 5.0
    specs = {"cam": (cam, "in"), "out": (Out((B,) + size), "out")}

    def call(o):
        return lib.stlt_cam_upsample(o.cam.ptr, B, *grid, *size, o.out.ptr, GA.stream())

    want, bound = R.upsample(cam.numpy(), size), R.upsample_bound(cam.numpy(), grid)
    for tag, mis in (("aligned", None), ("misaligned", {"cam": 4, "out": 12})):
        got = GA.three_ways(lib, arena, specs, call, ["out"], misalign=mis)["out"]
        err = float(np.abs(got.double().numpy() - want).max())
        _report(f"cam_upsample {grid} -> {size} {tag}: err / bound", f"{err / bound:.3g}")
        assert err <= bound
    assert torch.equal(pkg.ops.cam_upsample(cam.to(DEV), size).cpu(), got)


# ---------------------------------------------------------------------------------------------------------------------- the models
def _resnet3d(pkg):
    if "resnet3d" not in _CACHE:
        m, sd = PG._load(pkg, pkg.Resnet3D(PG._app_cfg(pkg, 32)))
        _CACHE["resnet3d"] = (m.train(False), sd)
    return _CACHE["resnet3d"]


def _target(B, K):
    return (torch.arange(B) * 7 + 3) % K


def _oracle(pkg, shape):
    """The oracle on `shape`, computed once: per stage 1..3 the activations and the gradient of the target logits with respect to the
    stage's output (autograd at the tensor after the stage's ReLU), in float64 and — the calibration of test_r3d_shapes_gpu — in two
    float32 runs in different summation orders, the plain one and the same problem with H and W exchanged (exact: every stride and pad
    of the trunk is equal in h and w).  Which near-zero ReLU mask inside a block float32 flips depends on the order, so one run can miss
    a flip that another float32 order (the kernels') makes."""
    key = ("oracle", shape)
    if key not in _CACHE:
        _, sd = _resnet3d(pkg)
        video = pkg.synth.make_video(*shape, seed=900 + shape[0])
        target = _target(shape[0], sd["classifier.weight"].shape[0])
        sd_t = {k: (v.transpose(-1, -2).contiguous() if v.dim() == 5 else v) for k, v in sd.items()}
        runs = {}
        for tag, dtype, weights, v in (("f64", torch.float64, sd, video), ("f32", torch.float32, sd, video), ("f32_t", torch.float32, sd_t, video.transpose(-1, -2).contiguous())):
            sdd = O._cast(weights, dtype)
            st = {}
            feats = O.trunk_forward(sdd, v.to(dtype).requires_grad_(True), stages=st)
            logits = feats.mean(dim=(2, 3, 4)) @ sdd["classifier.weight"].T + sdd["classifier.bias"]
            grads = torch.autograd.grad(logits[torch.arange(shape[0]), target].sum(), [st[f"layer{n}"] for n in (1, 2, 3)])
            back = (lambda t: t.transpose(-1, -2).contiguous()) if tag == "f32_t" else (lambda t: t)
            runs[tag] = {n: (back(st[f"layer{n}"].detach()), back(g)) for n, g in zip((1, 2, 3), grads)}
        _CACHE[key] = (video, target, runs)
    return _CACHE[key]


# ------------------------------------------------------------------------------------------------- 4. stlt_r3d_backward_layer, op level
def test_backward_layer_refusals(pkg):
    lib = pkg._lib.load()
    m, _ = _resnet3d(pkg)
    shape = SHAPES[0]
    video = pkg.synth.make_video(*shape, seed=5).to(DEV)
    tape = m._runner.run_tape(m.resnet, video, features=True)
    dfeat = torch.ones_like(tape.features)
    dims, off = pkg.ops.r3d_layer_geometry(*shape, 2)
    dlayer = torch.empty((shape[0],) + dims, device=DEV)
    ws = torch.empty(lib.stlt_r3d_backward_workspace_bytes(*shape), dtype=torch.uint8, device=DEV)
    dg = pkg._lib.R3dPointers(*[t.data_ptr() for t in tape.dgrad])

    def call(layer, out_ptr, ws_bytes):
        return lib.stlt_r3d_backward_layer(ctypes.byref(tape.params), dg, tape.tape.data_ptr(), tape.tape.numel(), *shape, dfeat.data_ptr(), None, layer, out_ptr,
                                           ws.data_ptr(), ws_bytes, GA.stream())

    for layer in (0, 4):
        assert call(layer, dlayer.data_ptr(), ws.numel()) == EINVAL and "layer" in GA.last_error(lib)
    assert call(2, dlayer.data_ptr(), ws.numel() - 1) == EWORKSPACE
    assert call(2, dlayer.data_ptr() + 4, ws.numel()) == EINVAL and "dlayer" in GA.last_error(lib) and "aligned" in GA.last_error(lib)
    assert call(2, None, ws.numel()) == EINVAL
    for layer in (0, 4):
        with pytest.raises(pkg.StltHipError, match="layer"):
            pkg.ops.r3d_backward_layer(tape.params, tape.dgrad, tape.tape, shape, layer, dfeatures=dfeat)
    with pytest.raises(pkg.StltHipError, match="exactly one"):
        pkg.ops.r3d_backward_layer(tape.params, tape.dgrad, tape.tape, shape, 2)
    # the tape's slot is the stage's output, and the stop leaves the sweep above it as it is: two calls, the same bits
    assert tuple(tape.stage(2).shape) == (shape[0],) + dims and tape.stage(2).data_ptr() == tape.tape.data_ptr() + off
    a = pkg.ops.r3d_backward_layer(tape.params, tape.dgrad, tape.tape, shape, 2, dfeatures=dfeat)
    assert torch.equal(a, tape.backward_layer(2, dfeatures=dfeat)) and a.abs().max().item() > 0


# ------------------------------------------------------------------------------------------------------------------------ 5. end to end
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_resnet3d_last_stage_is_the_cam_closed_form(pkg, shape):
    """cam = relu(sum_c W[t,c] A[b,c,p]) / P from the model's own features and classifier in float64.  The float32 path adds: the map's
    sum over C terms ((C + 1) u), the weights' sum of P equal terms and its division ((P + 1) u), the division dpooled / P and the
    classifier's input gradient of a one-hot seed (a few u): (C + P + 8) u sum_c|W A| / P."""
    m, _ = _resnet3d(pkg)
    B = shape[0]
    batch = {"video_frames": pkg.synth.make_video(*shape, seed=900 + B).to(DEV)}
    target = _target(B, m.classifier.weight.shape[0]).to(DEV)
    out = m.forward_gradcam(batch, target=target)
    A = m.forward_features(batch).double().cpu()
    Wt = m.classifier.weight.detach().double().cpu()[target.cpu()]  # (B, C)
    P, Cn = A[0, 0].numel(), A.shape[1]
    terms = Wt[:, :, None] * A.flatten(2)
    want = terms.sum(dim=1).relu() / P
    bound = (Cn + P + 8) * U * terms.abs().sum(dim=1) / P
    err = (out["cam"].flatten(1).double().cpu() - want).abs()
    _report(f"Resnet3D layer 4 closed form {shape}: worst err / bound", f"{(err / bound).max().item():.3g}")
    assert tuple(out["cam"].shape) == (B,) + tuple(A.shape[2:]) and out["cam"].dtype == torch.float32
    assert (err <= bound).all() and want.max().item() > 0
    assert torch.equal(out["target"], target) and torch.equal(out["resnet3d"], m(batch)["resnet3d"])
    assert torch.equal(out["cell_attribution"], out["cam"].flatten(1))
    if shape == SHAPES[1]:
        assert tuple(out["cell_attribution"].shape) == (3, 1 * 4 * 3)


@pytest.mark.parametrize("layer", [1, 2, 3])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_resnet3d_lower_stages_against_the_oracle(pkg, shape, layer):
    """The map and the gradient at the stage (ops.r3d_backward_layer) against the float64 oracle under the project's rule
    (test_r3d_train_gpu._bound with the reference distance of test_r3d_shapes_gpu: the larger of two float32 runs of the oracle in
    different summation orders).  Measured on an MI355X: (1, 8, 64, 64) — every error below 0.002 of the bound (5e-4); (3, 9, 97, 75) —
    at stages 1 and 2 one near-zero ReLU mask inside a block flips in float32, in the kernels as in the H/W-exchanged float32 oracle
    (both 1.48e-2 and 1.19e-2 of max|g| from float64, confined to one neighbourhood of one clip), so the gradient's bound there is the
    3 % cap and its error 0.49 and 0.40 of it; the maps there: float32 oracle at 6.3e-4 and 4.3e-4, error 0.125 of 8 x that; stage 3:
    0.0006 (gradient) and 0.002 (map) of 5e-4.  That a mask applied by mistake cannot pass (it moves the gradient by 80 % of its
    maximum and more) is asserted below."""
    m, _ = _resnet3d(pkg)
    video, target, runs = _oracle(pkg, shape)
    batch = {"video_frames": video.to(DEV)}
    out = m.forward_gradcam(batch, target=target.to(DEV), layer=layer)
    tape = m._runner.run_tape(m.resnet, batch["video_frames"], features=False, pooled=True)
    W = m.classifier.weight.detach()
    dlayer = tape.backward_layer(layer, dpooled=W[target.to(DEV)].contiguous())
    a64, g64 = runs["f64"][layer]
    zeros = (a64 == 0).double().mean().item()
    # the gradient at the stage, unmasked: NDHWC on the device, NCDHW in the oracle
    got_g = dlayer.permute(0, 4, 1, 2, 3).double().cpu()
    rel32 = max((runs[k][layer][1].double() - g64).abs().max().item() for k in ("f32", "f32_t")) / g64.abs().max().item()
    err = (got_g - g64).abs().max().item() / g64.abs().max().item()
    _report(f"dlayer {shape} layer {layer}: err / bound (float32 oracle at {rel32:.2e}; {100 * zeros:.0f} % of the stage is exactly 0)", f"{err / _bound(rel32):.3g}")
    assert err <= _bound(rel32), (err, _bound(rel32), rel32)
    assert (g64[a64 == 0] != 0).any(), "no zero of the stage carries a gradient: a mask applied by mistake would not show"
    masked = (torch.where(a64 == 0, torch.zeros_like(g64), g64) - g64).abs().max().item() / g64.abs().max().item()
    assert masked > _bound(rel32), "a ReLU mask applied by mistake would pass this bound"
    cams = {k: torch.from_numpy(R.gradcam(a.numpy(), g.numpy(), "ncdhw")) for k, (a, g) in ((k, runs[k][layer]) for k in ("f64", "f32", "f32_t"))}
    cams[64] = cams["f64"]
    rel32 = max((cams[k] - cams[64]).abs().max().item() for k in ("f32", "f32_t")) / cams[64].abs().max().item()
    err = (out["cam"].flatten(1).double().cpu() - cams[64]).abs().max().item() / cams[64].abs().max().item()
    _report(f"cam {shape} layer {layer}: err / bound (float32 oracle at {rel32:.2e})", f"{err / _bound(rel32):.3g}")
    assert err <= _bound(rel32), (err, _bound(rel32), rel32)
    assert tuple(out["cam"].shape) == (shape[0],) + tuple(a64.shape[2:]) and cams[64].max().item() > 0


def _fusion(pkg, name):
    if name not in _CACHE:
        _CACHE[name] = PG._fusion(pkg, name)[0]
    return _CACHE[name]


def _transformer(pkg):
    if "transformer" not in _CACHE:
        _CACHE["transformer"] = PG._load(pkg, pkg.models_factory["resnet3d-transformer"](PG._app_cfg(pkg, PG.FRAMES, num_appearance_layers=2)))[0].train(False)
    return _CACHE["transformer"]


def _compose_last_stage(pkg, m, feats, rest, target, **kw):
    g = m.forward_saliency(dict(rest, appearance_features=feats), target=target, **kw)["appearance_features_grad"]
    return pkg.ops.cam_map(feats, pkg.ops.cam_weights(g.contiguous(), "ncdhw"), "ncdhw")


def test_transformer_resnet_composes_from_the_public_pieces(pkg):
    m = _transformer(pkg)
    video = PG._video(pkg)
    target = _target(video.shape[0], m.classifier.weight.shape[0]).to(DEV)
    out = m.forward_gradcam({"video_frames": video}, target=target)
    with torch.no_grad():
        feats = m.resnet.forward_features({"video_frames": video})
    assert torch.equal(out["cam"], _compose_last_stage(pkg, m, feats, {}, target)) and out["cam"].abs().max().item() > 0
    assert torch.equal(out["resnet3d"], m({"video_frames": video})["resnet3d"]) and tuple(out["cell_attribution"].shape) == (video.shape[0], 4)
    with pytest.raises(pkg.StltHipError, match="training mode"):
        m.train(True).forward_gradcam({"video_frames": video})
    m.train(False)


@pytest.mark.parametrize("name,head", [("caf", None), ("lcf", None), ("cacnf", "stlt"), ("cacnf", "resnet3d"), ("cacnf", "caf"), ("cacnf", "ensemble")])
def test_fusion_models_compose_from_the_public_pieces(pkg, name, head):
    m = _fusion(pkg, name)
    lay, _ = PG._fusion_batch(pkg)
    B = PG.VIDEO[0]
    feats = pkg.synth.make_appearance_features(B, seed=1620, grid=(1, 2, 2)).to(DEV)
    target = _target(B, pkg.synth.model_kwargs("cfg1")["num_classes"]).to(DEV)
    kw = {} if head is None else {"head": head}
    # precomputed features: no trunk launch
    out = m.forward_gradcam(dict(lay, appearance_features=feats), target=target, **kw)
    assert torch.equal(out["cam"], _compose_last_stage(pkg, m, feats, lay, target, **kw))
    assert set(m.logit_names) <= set(out) and tuple(out["cam"].shape) == (B, 1, 2, 2) and torch.equal(out["cell_attribution"], out["cam"].flatten(1))
    if head == "stlt":
        assert out["cam"].abs().max().item() == 0  # this head does not read the appearance side
    else:
        assert out["cam"].abs().max().item() > 0
    # from frames: the trunk's features take their place
    video = PG._video(pkg)
    trunk = m.backbone.appearance_branch.resnet if name == "cacnf" else (m.caf_backbone if name == "caf" else m).appearance_branch.resnet
    out_v = m.forward_gradcam(dict(lay, video_frames=video), target=target, **kw)
    with torch.no_grad():
        feats_v = trunk.forward_features({"video_frames": video})
    assert torch.equal(out_v["cam"], _compose_last_stage(pkg, m, feats_v, lay, target, **kw))
    with pytest.raises(pkg.StltHipError, match="only `appearance_features`"):
        m.forward_gradcam(dict(lay, appearance_features=feats), layer=3)
    with pytest.raises(pkg.StltHipError, match="head must be one of"):
        m.forward_gradcam(dict(lay, appearance_features=feats), head="nope")


def test_cacnf_with_a_trunk_composes_at_a_lower_stage(pkg):
    m = _fusion(pkg, "cacnf")
    lay, _ = PG._fusion_batch(pkg)
    video = PG._video(pkg)
    shape = (video.shape[0],) + tuple(video.shape[2:])
    target = _target(shape[0], pkg.synth.model_kwargs("cfg1")["num_classes"]).to(DEV)
    out = m.forward_gradcam(dict(lay, video_frames=video), target=target, layer=2, head="caf")
    trunk = m.backbone.appearance_branch.resnet
    tape = trunk._runner.run_tape(trunk.resnet, video, features=True)
    g = m.forward_saliency(dict(lay, appearance_features=tape.features), target=target, head="caf")["appearance_features_grad"].contiguous()
    dims, off = pkg.ops.r3d_layer_geometry(*shape, 2)
    n = shape[0] * dims[0] * dims[1] * dims[2] * dims[3]
    a = tape.tape[off:off + 4 * n].view(torch.float32).view((shape[0],) + dims)
    dlayer = pkg.ops.r3d_backward_layer(tape.params, tape.dgrad, tape.tape, shape, 2, dfeatures=g)
    cam = pkg.ops.cam_map(a, pkg.ops.cam_weights(dlayer), "ndhwc")
    assert torch.equal(out["cam"], cam) and cam.abs().max().item() > 0 and tuple(cam.shape) == (shape[0],) + dims[:3]
    assert torch.equal(out["cell_attribution"], pkg.ops.cell_pool_sum(cam.view(shape[0], 1, *dims[:3]), (4, 4, 4)))
    with torch.no_grad():
        assert torch.equal(tape.features, trunk.forward_features({"video_frames": video}))


def test_the_other_outputs_and_invariants(pkg):
    m, _ = _resnet3d(pkg)
    shape = SHAPES[1]
    B = shape[0]
    batch = {"video_frames": pkg.synth.make_video(*shape, seed=900 + B).to(DEV)}
    target = _target(B, m.classifier.weight.shape[0]).to(DEV)
    flags = [(q, q.requires_grad) for q in m.parameters()]
    for layer in (4, 3):
        plain = m.forward_gradcam(batch, target=target, layer=layer)
        again = m.forward_gradcam(batch, target=target, layer=layer, upsample=True)
        assert all(torch.equal(plain[k], again[k]) for k in plain), "two calls differ"
        assert torch.equal(again["video_cam"], pkg.ops.cam_upsample(plain["cam"], shape[1:])) and tuple(again["video_cam"].shape) == shape
        raw = m.forward_gradcam(batch, target=target, layer=layer, relu=False)["cam"]
        assert (raw < 0).any() and torch.equal((raw - raw.clamp(max=0)).view(torch.int32), plain["cam"].view(torch.int32))
        # HiResCAM against the restatement, from the same activations and gradient the device used
        hires = m.forward_gradcam(batch, target=target, layer=layer, variant="hirescam")["cam"]
        tape = m._runner.run_tape(m.resnet, batch["video_frames"], features=True, pooled=True)
        dpooled = m._gradcam_head(None, tape.pooled, target, None)[3]  # the classifier's input gradient, as the call itself forms it
        if layer == 4:
            a, lay = tape.features, "ncdhw"
            g = (dpooled / a[0, 0].numel()).view(B, -1, 1, 1, 1).expand_as(a).contiguous()
        else:
            a, g, lay = tape.stage(layer), tape.backward_layer(layer, dpooled=dpooled), "ndhwc"
        want, bound = R.cam_map(a.cpu().numpy(), g.cpu().numpy(), lay, True)
        err = np.abs(hires.flatten(1).double().cpu().numpy() - want)
        _report(f"hirescam layer {layer} {shape}: worst err / bound", f"{(err / np.maximum(bound, 1e-300)).max():.3g}")
        assert (err <= bound).all() and want.max() > 0
        assert not torch.equal(hires, plain["cam"])
    assert tuple(plain["cell_attribution"].shape) == (B, 1 * 4 * 3)
    assert torch.equal(plain["cell_attribution"], pkg.ops.cell_pool_sum(plain["cam"].view(B, 1, *plain["cam"].shape[1:]), (2, 2, 2)))
    assert all(q.grad is None for q in m.parameters()) and all(q.requires_grad == r for q, r in flags)
    top1 = m.forward_gradcam(batch)  # no target: the top-1 class, picked on the device
    assert torch.equal(top1["target"], top1["resnet3d"].argmax(dim=1))


def test_refusals(pkg):
    m, _ = _resnet3d(pkg)
    E = pkg.StltHipError
    video = pkg.synth.make_video(1, 8, 64, 64, seed=3)
    with pytest.raises(E, match="layer"):
        m.forward_gradcam({"video_frames": video.to(DEV)}, layer=5)
    with pytest.raises(E, match="variant"):
        m.forward_gradcam({"video_frames": video.to(DEV)}, variant="scorecam")
    with pytest.raises(E, match="CPU"):
        m.forward_gradcam({"video_frames": video})
    with pytest.raises(E, match="target"):
        m.forward_gradcam({"video_frames": video.to(DEV)}, target=torch.zeros(2, dtype=torch.int64, device=DEV))
    with pytest.raises(E, match="video_frames"):
        m.forward_gradcam({"appearance_features": torch.zeros(1, 2048, 1, 2, 2, device=DEV)}, layer=3)
    assert not hasattr(pkg.Stlt, "forward_gradcam")


def test_the_perturbation_runner_takes_gradcam(pkg):
    m, _ = _resnet3d(pkg)
    batches = [{"video_frames": pkg.synth.make_video(2, 8, 64, 64, seed=s)} for s in (41, 42)]
    a = pkg.infer.run_perturbation_test(m, batches, method="gradcam", modality="appearance", steps=4)
    b = pkg.infer.run_perturbation_test(m, batches, method=lambda mod, bt: mod.forward_gradcam(bt)["cell_attribution"], modality="appearance", steps=4)
    assert a == b and a["descending"]["num_clips"] == 4 and len(a["descending"]["prob"]) == 5  # the same curves, number for number
    with pytest.raises(pkg.StltHipError, match="convolution"):
        pkg.infer.run_perturbation_test(m, batches, method="gradcam", modality="layout")
