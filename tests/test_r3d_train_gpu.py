"""Training the R3D-50 trunk on the GPU: the data / weight gradients of every trunk conv class against torch.autograd of a float64 CPU
convolution (with the fused epilogue and the accumulate flag), the max-pool backward exactly against torch, the whole trunk's weight
gradients against the reference's (tests/golden/r3d_train.npz, tools/gen_golden_r3d_train.py), two Trainer steps against the reference
loop, the refreshed weight copies after a fused optimiser step, the fusion models' trunk gradients, and per-forward tapes."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import GOLDEN

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
EPS32 = 2.0 ** -24


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _ndhwc(x_cpu, c_pad=None):
    x = x_cpu.permute(0, 2, 3, 4, 1)
    if c_pad is not None and c_pad > x.shape[-1]:
        x = F.pad(x, (0, c_pad - x.shape[-1]))
    return x.contiguous().to(DEV)


# (B, Cin, T, H, W, Cout, kernel, stride, pad, n_split): the trunk's conv classes at small sizes; the stem has a weight gradient only
CASES = {
    "stem_cin3": (1, 3, 5, 9, 11, 64, (7, 7, 7), (1, 2, 2), (3, 3, 3), 1),
    "3x3x3_s1": (2, 32, 4, 6, 5, 48, (3, 3, 3), (1, 1, 1), (1, 1, 1), 1),
    "3x3x3_s2_odd": (1, 32, 5, 7, 9, 40, (3, 3, 3), (2, 2, 2), (1, 1, 1), 1),
    "3x3x3_s2_even": (2, 16, 4, 6, 8, 24, (3, 3, 3), (2, 2, 2), (1, 1, 1), 1),
    "1x1x1_s1": (3, 64, 3, 5, 7, 96, (1, 1, 1), (1, 1, 1), (0, 0, 0), 1),
    "1x1x1_s2": (2, 64, 5, 7, 7, 128, (1, 1, 1), (2, 2, 2), (0, 0, 0), 1),
    "3x3x3_split3": (1, 128, 2, 4, 4, 64, (3, 3, 3), (1, 1, 1), (1, 1, 1), 3),
    "1x1x1_split_auto": (4, 256, 2, 4, 4, 512, (1, 1, 1), (1, 1, 1), (0, 0, 0), 0),
    # M = 65 536 (2048 m-slabs), one 64 x 64 wgrad tile: the automatic plan stops at WG_SPLIT_MAX = 256 splits of 8 slabs
    "with_wgsplit256_1x1x1": (4, 64, 16, 32, 32, 64, (1, 1, 1), (1, 1, 1), (0, 0, 0), 0),
    # 98 m-slabs: automatic wgrad plan of 11 splits (ten of 9 slabs, the last of 8); the dgrad plan splits 54 k-slabs 6 ways
    "with_wgsplit11_3x3x3": (2, 64, 8, 14, 14, 64, (3, 3, 3), (1, 1, 1), (1, 1, 1), 0),
    # explicit 7: wgrad 19 m-slabs (the last a partial one) as 6 x 3 + 1; dgrad 41 k-slabs as 6 x 6 + 5
    "with_split7_uneven_3x3x3": (1, 32, 6, 10, 10, 48, (3, 3, 3), (1, 1, 1), (1, 1, 1), 7),
    # layer 4's conv2 at B = 2: the automatic dgrad plan splits each parity class (up to 16 ways: 128 k-slabs of the 2x2x2-tap class)
    "with_split_auto_3x3x3_s2": (2, 512, 4, 7, 7, 512, (3, 3, 3), (2, 2, 2), (1, 1, 1), 0),
    # explicit 3 on a stride-2 dgrad with odd extents (classes of 2 to 16 k-slabs: 2 or 3 splits); wgrad 2 m-slabs, 2 splits
    "with_split3_3x3x3_s2": (1, 64, 6, 7, 5, 64, (3, 3, 3), (2, 2, 2), (1, 1, 1), 3),
    # Ti = 1 under stride 2: the four classes of odd t have no rows (layer 4's conv2 at T <= 8); explicit 3 splits the others
    "with_rowless_split3_3x3x3_s2_t1": (2, 64, 1, 6, 5, 64, (3, 3, 3), (2, 2, 2), (1, 1, 1), 3),
    # Hi = 1 under a 1x1x1 stride 2 (the downsample): classes without rows beside classes without taps; unsplit
    "with_rowless_1x1x1_s2_h1": (2, 64, 3, 1, 5, 128, (1, 1, 1), (2, 2, 2), (0, 0, 0), 0),
}
# (wgrad splits, dgrad splits) each case reaches, from the library's workspace queries (tests/test_r3d_plans_cpu.py): wgrad = bytes ÷ one
# c_out·K slab; dgrad at stride 1 = bytes ÷ one B·T·H·W·c_in slab; at stride 2 the classes differ, so 2 there means "some class splits"
PLANNED_SPLITS = {
    "3x3x3_split3": (1, 3),
    "with_wgsplit256_1x1x1": (256, 1),
    "with_wgsplit11_3x3x3": (11, 6),
    "with_split7_uneven_3x3x3": (7, 7),
    "with_split_auto_3x3x3_s2": (1, 2),
    "with_split3_3x3x3_s2": (2, 2),
    "with_rowless_split3_3x3x3_s2_t1": (1, 2),
    "with_rowless_1x1x1_s2_h1": (1, 1),
}


def _case(case):
    B, Ci, T, H, W, Co, k, s, p, n_split = CASES[case]
    g = _gen(2000 + sorted(CASES).index(case))
    x = torch.randn(B, Ci, T, H, W, generator=g)
    w = torch.randn(Co, Ci, *k, generator=g) * (2.0 / (Ci * k[0] * k[1] * k[2])) ** 0.5
    To, Ho, Wo = [(n + 2 * pp - kk) // ss + 1 for n, kk, ss, pp in zip((T, H, W), k, s, p)]
    dy = torch.randn(B, Co, To, Ho, Wo, generator=g)
    return (B, Ci, T, H, W, Co, k, s, p, n_split), g, x, w, dy


def _grads64(x, w, dy, s, p, absval=False):
    if absval:
        x, w, dy = x.abs(), w.abs(), dy.abs()
    xd, wd = x.double().requires_grad_(), w.double().requires_grad_()
    y = F.conv3d(xd, wd, stride=s, padding=p)
    return torch.autograd.grad(y, (xd, wd), dy.double())


@pytest.mark.parametrize("case", sorted(c for c in CASES if c != "stem_cin3"))  # the stem needs no data gradient (video_frames gets none)
def test_conv3d_dgrad_against_float64(pkg, case):
    (B, Ci, T, H, W, Co, k, s, p, n_split), g, x, w, dy = _case(case)
    lib = pkg._lib.load()
    scale_co = 0.5 + torch.rand(Co, generator=g)   # folded into the dgrad copy (the BN scale of the conv)
    scale_ci = 0.5 + torch.rand(Ci, generator=g)   # epilogue scale
    add = torch.randn(B, Ci, T, H, W, generator=g)
    mask = torch.randn(B, Ci, T, H, W, generator=g)
    d = pkg._lib.Conv3dDesc(B, T, H, W, Ci, Co, *k, *s, *p)
    wd = torch.empty(w.numel(), device=DEV)
    w_d, scale_co_d = w.to(DEV), scale_co.to(DEV)  # held: a temporary's memory could be reused before the launch reads it
    pkg._lib.check(lib.stlt_conv3d_repack_dgrad(w_d.data_ptr(), ctypes.byref(d), scale_co_d.data_ptr(), wd.data_ptr(), _stream()), "repack_dgrad")
    nbytes = int(lib.stlt_conv3d_bwd_data_workspace_bytes(ctypes.byref(d), n_split))
    ws = torch.empty(max(nbytes, 1), dtype=torch.uint8, device=DEV)
    dy_d, add_d, mask_d, sc_d = _ndhwc(dy), _ndhwc(add), _ndhwc(mask), scale_ci.to(DEV)

    def run(with_epilogue):
        dx = torch.full((B, T, H, W, Ci), float("nan"), device=DEV)
        args = (sc_d.data_ptr(), mask_d.data_ptr(), add_d.data_ptr()) if with_epilogue else (None, None, None)
        pkg._lib.check(lib.stlt_conv3d_bwd_data(ctypes.byref(d), dy_d.data_ptr(), wd.data_ptr(), *args, n_split, ws.data_ptr(), nbytes, dx.data_ptr(),
                                                _stream()), "stlt_conv3d_bwd_data")
        return dx.permute(0, 4, 1, 2, 3).cpu().double()

    ws_ = w * scale_co.view(-1, 1, 1, 1, 1)
    ref = _grads64(x, ws_, dy, s, p)[0]
    mag = _grads64(x, ws_, dy, s, p, absval=True)[0]
    K = Co * k[0] * k[1] * k[2]
    tol = 4 * EPS32 * K ** 0.5 * mag.max().item()
    got = run(False)
    assert (got - ref).abs().max().item() <= tol, (case, (got - ref).abs().max().item(), tol)
    ref_e = torch.where(mask.double() > 0, ref * scale_ci.double().view(1, -1, 1, 1, 1) + add.double(), torch.zeros_like(ref))
    got_e = run(True)
    tol_e = tol * scale_ci.max().item() + 4 * EPS32 * add.abs().max().item()
    assert (got_e - ref_e).abs().max().item() <= tol_e, (case, (got_e - ref_e).abs().max().item(), tol_e)
    assert torch.equal(got_e, run(True))  # a repeated launch is bit-identical
    # add == dx (the trunk's shortcut gradient): each element is read, then written, by one thread — bit for bit the out-of-place result
    dx = add_d.clone()
    pkg._lib.check(lib.stlt_conv3d_bwd_data(ctypes.byref(d), dy_d.data_ptr(), wd.data_ptr(), sc_d.data_ptr(), mask_d.data_ptr(), dx.data_ptr(), n_split,
                                            ws.data_ptr(), nbytes, dx.data_ptr(), _stream()), "stlt_conv3d_bwd_data (add == dx)")
    assert torch.equal(dx.permute(0, 4, 1, 2, 3).cpu().double(), got_e), case


@pytest.mark.parametrize("case", sorted(CASES))
def test_conv3d_wgrad_against_float64(pkg, case):
    (B, Ci, T, H, W, Co, k, s, p, n_split), g, x, w, dy = _case(case)
    lib = pkg._lib.load()
    c_pad = (Ci + 3) // 4 * 4
    scale = 0.5 + torch.rand(Co, generator=g)
    init = torch.randn(Co, Ci, *k, generator=g)
    d = pkg._lib.Conv3dDesc(B, T, H, W, c_pad, Co, *k, *s, *p)
    nbytes = int(lib.stlt_conv3d_bwd_weight_workspace_bytes(ctypes.byref(d), n_split))
    ws = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
    x_d, dy_d, sc_d = _ndhwc(x, c_pad), _ndhwc(dy), scale.to(DEV)

    def run(accumulate):
        dw = init.to(DEV) if accumulate else torch.full((Co, Ci, *k), float("nan"), device=DEV)
        pkg._lib.check(lib.stlt_conv3d_bwd_weight(ctypes.byref(d), x_d.data_ptr(), dy_d.data_ptr(), sc_d.data_ptr(), Ci, int(accumulate), n_split,
                                                  ws.data_ptr(), nbytes, dw.data_ptr(), _stream()), "stlt_conv3d_bwd_weight")
        return dw.cpu().double()

    sc = scale.double().view(-1, 1, 1, 1, 1)
    ref = _grads64(x, w, dy, s, p)[1] * sc
    mag = _grads64(x, w, dy, s, p, absval=True)[1] * sc
    M = dy[0, 0].numel() * B
    tol = 4 * EPS32 * M ** 0.5 * mag.max().item()
    got = run(False)
    assert (got - ref).abs().max().item() <= tol, (case, (got - ref).abs().max().item(), tol)
    got_acc = run(True)
    ref_acc = ref + init.double()
    assert (got_acc - ref_acc).abs().max().item() <= tol + 4 * EPS32 * init.abs().max().item(), case
    assert torch.equal(got_acc, run(True))


def test_maxpool_backward_exact(pkg):
    lib = pkg._lib.load()
    g = _gen(77)
    for (B, C, T, H, W) in ((2, 8, 7, 9, 10), (1, 64, 6, 12, 12), (3, 4, 1, 2, 3)):
        x = (torch.randint(-3, 4, (B, C, T, H, W), generator=g).float() / 4).relu()  # dyadic, many ties (zeros above all)
        xr = x.clone().requires_grad_()
        y_ref = F.max_pool3d(xr, kernel_size=3, stride=2, padding=1)
        dy = torch.randint(-64, 64, y_ref.shape, generator=g).float() / 64
        (dx_ref,) = torch.autograd.grad(y_ref, xr, dy)
        xn = _ndhwc(x)
        y = torch.empty(y_ref.permute(0, 2, 3, 4, 1).shape, device=DEV)
        am = torch.empty(y.shape, dtype=torch.uint8, device=DEV)
        pkg._lib.check(lib.stlt_maxpool3d_ndhwc_train(xn.data_ptr(), B, T, H, W, C, y.data_ptr(), am.data_ptr(), _stream()), "maxpool_train")
        assert torch.equal(y.permute(0, 4, 1, 2, 3).cpu(), y_ref.detach())
        dy_d = _ndhwc(dy)
        for mask in (None, xn):
            dx = torch.empty_like(xn)
            pkg._lib.check(lib.stlt_maxpool3d_ndhwc_bwd(dy_d.data_ptr(), am.data_ptr(), B, T, H, W, C, None if mask is None else mask.data_ptr(),
                                                        dx.data_ptr(), _stream()), "maxpool_bwd")
            want = dx_ref if mask is None else torch.where(x > 0, dx_ref, torch.zeros_like(dx_ref))
            assert torch.equal(dx.permute(0, 4, 1, 2, 3).cpu(), want)


# ---- the whole trunk against the reference ----
def _golden():
    return np.load(os.path.join(GOLDEN, "r3d_train.npz")), json.load(open(os.path.join(GOLDEN, "r3d_schema.json")))


def _app_kwargs(pkg, **extra):
    kw = pkg.synth.model_kwargs("cfg1")
    return dict(num_classes=kw["num_classes"], hidden_size=kw["hidden_size"], num_attention_heads=kw["num_attention_heads"], hidden_dropout_prob=0.0,
                appearance_num_frames=32, **extra)


def _loaded(pkg, model, meta):
    sd = pkg.synth.make_r3d_state_dict({k: tuple(v.shape) for k, v in model.state_dict().items()}, seed=meta["weight_seed"])
    model.load_state_dict(sd, strict=True)
    return model.to(DEV)


@pytest.fixture(scope="module")
def video(pkg):
    _, meta = _golden()
    return pkg.synth.make_video(meta["clips"], seed=meta["video_seed"]).to(DEV)


def _conv_weights(m):
    return [p for n, p in m.named_parameters() if p.dim() == 5 and ".resnet." in "." + n and "projector" not in n]


def _trunk_grads(m, video, labels):
    out = m({"video_frames": video})["resnet3d"]
    ws = _conv_weights(m)
    return torch.autograd.grad(F.cross_entropy(out, labels), ws)


def _bound(ref_rel):
    """5e-4 where the fp32 reference is within 1e-4 of the fp64 run (most convs); elsewhere 8x the reference's own distance, capped at 3 %."""
    return 5e-4 if ref_rel <= 1e-4 else min(3e-2, 8 * ref_rel)


def _check_against_golden(gold, tag, grads):
    """Per conv: max error over the sampled entries <= _bound(reference distance) · max|golden|, and the Frobenius norm's relative error
    <= _bound(reference norm distance).  Through 50 ReLUs an fp32 run flips a few near-zero masks, differently for every summation
    order: on some convs the fp32 reference itself is up to ~1 % of max|g| away from fp64, so a flat 1e-4 would fail the reference
    too.  Where the reference is tight, the bound is a fixed 5e-4, so a local bug in any conv shows."""
    assert len(grads) == 53
    bad = []
    for i, gr in enumerate(grads):
        gmax = float(gold[f"{tag}_gmax"][i])
        bound, bound_norm = _bound(float(gold[f"{tag}_f32_rel"][i])), _bound(float(gold[f"{tag}_f32_norm_rel"][i]))
        idx = torch.from_numpy(gold[f"{tag}_g{i}_idx"].astype(np.int64))
        got = gr.reshape(-1).cpu().double()[idx]
        err = (got - torch.from_numpy(gold[f"{tag}_g{i}_val"]).double()).abs().max().item() / gmax
        norm = float(gold[f"{tag}_norm"][i])
        err_norm = abs(gr.double().norm().item() - norm) / norm
        if err > bound or err_norm > bound_norm:
            bad.append((i, err, bound, err_norm, bound_norm))
    tight = int(np.sum(gold[f"{tag}_f32_rel"] <= 1e-4))
    assert not bad, (tag, f"{tight} of 53 convs tight", bad)


def test_resnet3d_trunk_gradients_against_golden(pkg, video):
    gold, meta = _golden()
    m = _loaded(pkg, pkg.Resnet3D(pkg.AppearanceModelConfig(**_app_kwargs(pkg, train_trunk=True))), meta).train(True)
    labels = torch.from_numpy(gold["labels"]).to(DEV)
    out = m({"video_frames": video})["resnet3d"]
    loss = F.cross_entropy(out, labels)
    assert abs(loss.item() - float(gold["res_loss"])) <= 2e-5
    ws = _conv_weights(m) + [m.classifier.weight, m.classifier.bias]
    grads = torch.autograd.grad(loss, ws)
    _check_against_golden(gold, "res", grads[:53])
    assert (grads[54].cpu() - torch.from_numpy(gold["res_cls_bias"])).abs().max().item() <= 1e-5
    idx = torch.from_numpy(gold["res_cls_w_idx"].astype(np.int64))
    want = torch.from_numpy(gold["res_cls_w_val"])
    assert (grads[53].reshape(-1).cpu()[idx] - want).abs().max().item() <= 1e-4 * max(1.0, want.abs().max().item())
    again = _trunk_grads(m, video, labels)
    assert all(torch.equal(a, b) for a, b in zip(grads[:53], again)), "two backward passes differ"


def test_transformer_resnet_trunk_gradients_against_golden(pkg, video):
    gold, meta = _golden()
    m = _loaded(pkg, pkg.TransformerResnet(pkg.AppearanceModelConfig(**_app_kwargs(pkg, train_trunk=True))), meta).train(False)
    labels = torch.from_numpy(gold["labels"]).to(DEV)
    grads = _trunk_grads(m, video, labels)
    _check_against_golden(gold, "tr", grads)
    assert all(torch.equal(a, b) for a, b in zip(grads, _trunk_grads(m, video, labels)))


def test_two_trainer_steps_match_reference_loop(pkg, video):
    gold, meta = _golden()
    m = _loaded(pkg, pkg.Resnet3D(pkg.AppearanceModelConfig(**_app_kwargs(pkg, train_trunk=True))), meta)
    tr = pkg.train.Trainer(m, "something", learning_rate=5e-5, weight_decay=1e-3, clip_val=5.0, warmup_steps=2, total_steps=10)
    params = dict(m.named_parameters())
    batch = {"video_frames": video, "labels": torch.from_numpy(gold["labels"]).to(DEV)}
    for s in range(2):
        out = tr.step(batch)
        assert abs(float(out["loss"]) - float(gold["step_loss"][s])) <= 2e-5, s
        assert abs(float(out["grad_norm"]) - float(gold["step_grad_norm"][s])) <= 2e-4 * float(gold["step_grad_norm"][s]), s
        for j, k in enumerate(gold["step_watch"]):
            got = params[str(k)].detach().reshape(-1)[:64].cpu().numpy()
            assert np.abs(got - gold[f"step{s}_w{j}"]).max() <= 2.5e-5, (s, str(k))


def test_no_stale_weight_copies_after_a_fused_step(pkg, video):
    gold, meta = _golden()
    m = _loaded(pkg, pkg.Resnet3D(pkg.AppearanceModelConfig(**_app_kwargs(pkg, train_trunk=True))), meta)
    tr = pkg.train.Trainer(m, "something", learning_rate=1e-3, warmup_steps=0, total_steps=10)
    batch = {"video_frames": video, "labels": torch.from_numpy(gold["labels"]).to(DEV)}
    with torch.no_grad():
        before = m.forward_features(batch)
    tr.step(batch)
    with torch.no_grad():
        after = m.forward_features(batch)
    fresh = pkg.Resnet3D(pkg.AppearanceModelConfig(**_app_kwargs(pkg)))
    fresh.load_state_dict(m.state_dict(), strict=True)
    fresh.to(DEV).train(False)
    with torch.no_grad():
        want = fresh.forward_features(batch)
    assert not torch.equal(before, after)
    assert torch.equal(after, want)


def _fusion(pkg, name, meta, train_trunk=True):
    cfg = pkg.MultimodalModelConfig(**dict(pkg.synth.model_kwargs("cfg1"), appearance_num_frames=32, num_appearance_layers=2, num_fusion_layers=2,
                                           appearance_trunk=True, train_trunk=train_trunk))
    return _loaded(pkg, pkg.models_factory[name](cfg), meta)


def _fusion_batch(pkg, meta, video):
    c = pkg.synth.CONFIGS[meta["config"]]
    batch = {k: v.to(DEV) for k, v in pkg.synth.make_batch(meta["clips"], c["T"], c["N"], seed=meta["batch_seed"]).items()}
    batch["video_frames"] = video
    batch["labels"] = torch.arange(meta["clips"], device=DEV)
    return batch


@pytest.mark.parametrize("name", ["cacnf", "lcf"])
def test_fusion_models_train_the_trunk(pkg, video, name):
    _, meta = _golden()
    m = _fusion(pkg, name, meta)
    batch = _fusion_batch(pkg, meta, video)
    trunk = [t for t in m.modules() if isinstance(t, pkg.Resnet3D)][0]
    convs = [c.weight for c in trunk.modules() if isinstance(c, torch.nn.Conv3d)]
    tr = pkg.train.Trainer(m, "something", learning_rate=5e-5, warmup_steps=0, total_steps=10)
    out = tr.step(batch)
    assert np.isfinite(float(out["loss"]))
    for i, w in enumerate(convs):
        g = w.grad  # a view of the trainer's flat gradient buffer
        assert g is not None and tr.bound.owns(w) and torch.isfinite(g).all() and g.abs().max().item() > 0, i
    # eval mode, grad enabled: training the trunk leaves the rest of the backward bit for bit as with a frozen trunk
    m = _fusion(pkg, name, meta).train(False)

    def grads():
        m.zero_grad(set_to_none=True)
        outs = m(batch)
        sum(F.cross_entropy(v, batch["labels"]) for v in outs.values()).backward()
        return {n: p.grad.clone() for n, p in m.named_parameters() if p.grad is not None and ".resnet." not in n}

    g_on = grads()
    trunk = [t for t in m.modules() if isinstance(t, pkg.Resnet3D)][0]
    trunk.resnet.requires_grad_(False)
    g_off = grads()
    assert g_on and set(g_on) == set(g_off)
    for n in g_on:
        assert torch.equal(g_on[n], g_off[n]), n


def test_each_forward_owns_its_tape(pkg, video):
    gold, meta = _golden()
    m = _loaded(pkg, pkg.Resnet3D(pkg.AppearanceModelConfig(**_app_kwargs(pkg, train_trunk=True))), meta).train(True)
    labels = torch.from_numpy(gold["labels"]).to(DEV)
    v2 = pkg.synth.make_video(meta["clips"], seed=99).to(DEV)
    ws = _conv_weights(m)
    one = torch.autograd.grad(F.cross_entropy(m({"video_frames": video})["resnet3d"], labels), ws)
    two = torch.autograd.grad(F.cross_entropy(m({"video_frames": v2})["resnet3d"], labels), ws)
    l1 = F.cross_entropy(m({"video_frames": video})["resnet3d"], labels)
    l2 = F.cross_entropy(m({"video_frames": v2})["resnet3d"], labels)
    g2 = torch.autograd.grad(l2, ws)
    g1 = torch.autograd.grad(l1, ws)
    assert all(torch.equal(a, b) for a, b in zip(one, g1))
    assert all(torch.equal(a, b) for a, b in zip(two, g2))
    assert not torch.equal(one[0], two[0])
    # a weight changed between a forward and its backward (and a forward after it re-made the shared copies) is refused, as torch
    # refuses a saved tensor modified in place
    l1 = F.cross_entropy(m({"video_frames": video})["resnet3d"], labels)
    with torch.no_grad():
        ws[5].mul_(1.5)
    m({"video_frames": v2})
    with pytest.raises(pkg.StltHipError, match="changed between this forward and its backward"):
        torch.autograd.grad(l1, ws)
