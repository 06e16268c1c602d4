"""R3D-50 trunk on the GPU: the implicit-GEMM Conv3d (+ BatchNorm, residual, ReLU) against a float64 CPU convolution over the trunk's
five convolution classes and odd shapes, the pooling and layout kernels against torch CPU, the whole trunk and the three models built on it
against the reference goldens (tools/gen_golden_r3d.py), determinism, and the training rule (frozen trunk only)."""
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


def _golden():
    return np.load(os.path.join(GOLDEN, "r3d.npz")), json.load(open(os.path.join(GOLDEN, "r3d_schema.json")))


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _to_ndhwc(pkg, x_cpu, c_pad):
    B, C, T, H, W = x_cpu.shape
    x = x_cpu.to(DEV)
    y = torch.empty(B, T, H, W, c_pad, device=DEV)
    pkg._lib.check(pkg._lib.load().stlt_ncdhw_to_ndhwc(x.data_ptr(), B, C, T, H, W, c_pad, y.data_ptr(), _stream()), "stlt_ncdhw_to_ndhwc")
    return y


def _repack(pkg, w_cpu, c_pad):
    co, ci, kt, kh, kw = w_cpu.shape
    w = w_cpu.to(DEV)
    out = torch.empty(co, kt, kh, kw, c_pad, device=DEV)
    pkg._lib.check(pkg._lib.load().stlt_conv3d_repack(w.data_ptr(), co, ci, kt, kh, kw, c_pad, out.data_ptr(), _stream()), "stlt_conv3d_repack")
    return out


def _conv(pkg, x_ndhwc, w_packed, c_out, k, s, p, bn=None, res=None, relu=True, n_split=1):
    lib = pkg._lib.load()
    B, T, H, W, C = x_ndhwc.shape
    d = pkg._lib.Conv3dDesc(B, T, H, W, C, c_out, *k, *s, *p)
    To, Ho, Wo = [(n + 2 * pp - kk) // ss + 1 for n, kk, ss, pp in zip((T, H, W), k, s, p)]
    y = torch.empty(B, To, Ho, Wo, c_out, device=DEV)
    nbytes = int(lib.stlt_conv3d_workspace_bytes(ctypes.byref(d), n_split))
    ws = torch.empty(max(nbytes, 1), dtype=torch.uint8, device=DEV)
    bnp = [t.data_ptr() for t in bn] if bn is not None else [None] * 4
    pkg._lib.check(lib.stlt_conv3d_fwd(ctypes.byref(d), x_ndhwc.data_ptr(), w_packed.data_ptr(), *bnp, 1e-5, None if res is None else res.data_ptr(),
                                       int(relu), n_split, ws.data_ptr(), nbytes, y.data_ptr(), _stream()), "stlt_conv3d_fwd")
    return y


# (B, Cin, T, H, W, Cout, kernel, stride, pad, residual, relu, n_split): the five classes of the trunk at small sizes, and odd shapes
CASES = {
    "stem_cin3": (1, 3, 9, 13, 13, 64, (7, 7, 7), (1, 2, 2), (3, 3, 3), False, True, 1),
    "cin4_3x3x3": (2, 4, 5, 6, 7, 40, (3, 3, 3), (1, 1, 1), (1, 1, 1), False, True, 1),
    "3x3x3_s1_odd_cout": (2, 64, 4, 7, 7, 96, (3, 3, 3), (1, 1, 1), (1, 1, 1), False, True, 1),
    "3x3x3_s2_odd_spatial": (1, 32, 5, 7, 9, 72, (3, 3, 3), (2, 2, 2), (1, 1, 1), False, True, 1),
    "1x1x1_s1_residual": (3, 128, 3, 5, 7, 200, (1, 1, 1), (1, 1, 1), (0, 0, 0), True, True, 1),
    "1x1x1_s2_downsample": (2, 64, 5, 7, 7, 256, (1, 1, 1), (2, 2, 2), (0, 0, 0), False, False, 1),
    "3x3x3_split3": (1, 256, 2, 4, 4, 130, (3, 3, 3), (1, 1, 1), (1, 1, 1), True, True, 3),
    "1x1x1_split_auto": (4, 512, 2, 4, 4, 512, (1, 1, 1), (1, 1, 1), (0, 0, 0), False, True, 0),
    # layer 4's conv2 at B = 2 (M = 64, 432 k-slabs), with BN and a residual: the automatic plan's 54 splits of 8 slabs
    "with_split54_3x3x3_s2_residual": (2, 512, 4, 7, 7, 512, (3, 3, 3), (2, 2, 2), (1, 1, 1), True, True, 0),
    # 108 k-slabs in an explicit 5 splits: four of 22 slabs, the last of 20
    "with_split5_uneven_3x3x3": (1, 128, 3, 4, 5, 96, (3, 3, 3), (1, 1, 1), (1, 1, 1), True, False, 5),
}
# the split count each splitting case reaches (stlt_conv3d_workspace_bytes ÷ one M·c_out slab: tests/test_r3d_plans_cpu.py)
PLANNED_SPLITS = {"3x3x3_split3": 3, "1x1x1_split_auto": 2, "with_split54_3x3x3_s2_residual": 54, "with_split5_uneven_3x3x3": 5}


@pytest.mark.parametrize("case", sorted(CASES))
def test_conv3d_against_float64(pkg, case):
    B, Ci, T, H, W, Co, k, s, p, with_res, relu, n_split = CASES[case]
    g = _gen(1000 + sorted(CASES).index(case))
    x = torch.randn(B, Ci, T, H, W, generator=g).relu_() if Ci > 4 else torch.randn(B, Ci, T, H, W, generator=g)
    fan = Ci * k[0] * k[1] * k[2]
    w = torch.randn(Co, Ci, *k, generator=g) * (2.0 / fan) ** 0.5
    bn = [1 + 0.2 * torch.randn(Co, generator=g), 0.1 * torch.randn(Co, generator=g), 0.1 * torch.randn(Co, generator=g),
          0.5 + torch.rand(Co, generator=g)]
    c_pad = (Ci + 3) // 4 * 4
    ref = F.conv3d(x.double(), w.double(), stride=s, padding=p)
    mag = F.conv3d(x.double().abs(), w.double().abs(), stride=s, padding=p)
    scale = bn[0].double() / torch.sqrt(bn[3].double() + 1e-5)
    ref = ref * scale.view(1, -1, 1, 1, 1) + (bn[1].double() - bn[2].double() * scale).view(1, -1, 1, 1, 1)
    res = torch.randn(ref.shape, generator=g) if with_res else None
    if with_res:
        ref = ref + res.double()
    if relu:
        ref = ref.relu()
    res_dev = None if res is None else res.permute(0, 2, 3, 4, 1).contiguous().to(DEV)
    y = _conv(pkg, _to_ndhwc(pkg, x, c_pad), _repack(pkg, w, c_pad), Co, k, s, p, bn=[t.to(DEV) for t in bn], res=res_dev, relu=relu, n_split=n_split)
    got = y.permute(0, 4, 1, 2, 3).cpu().double()
    assert got.shape == ref.shape
    K = fan
    tol = 4 * EPS32 * K ** 0.5 * (mag * scale.abs().view(1, -1, 1, 1, 1)).max().item() + 4 * EPS32 * ref.abs().max().item()
    err = (got - ref).abs().max().item()
    assert err <= tol, (case, err, tol)
    # deterministic: a second launch is bit-identical
    y2 = _conv(pkg, _to_ndhwc(pkg, x, c_pad), _repack(pkg, w, c_pad), Co, k, s, p, bn=[t.to(DEV) for t in bn], res=res_dev, relu=relu, n_split=n_split)
    assert torch.equal(y, y2)


def test_conv3d_argument_checks(pkg):
    lib = pkg._lib.load()
    x = torch.zeros(1, 2, 2, 2, 3, device=DEV)
    w = torch.zeros(8, 1, 1, 1, 3, device=DEV)
    y = torch.zeros(1, 2, 2, 2, 8, device=DEV)
    d = pkg._lib.Conv3dDesc(1, 2, 2, 2, 3, 8, 1, 1, 1, 1, 1, 1, 0, 0, 0)  # c_in not a multiple of 4
    assert lib.stlt_conv3d_fwd(ctypes.byref(d), x.data_ptr(), w.data_ptr(), None, None, None, None, 1e-5, None, 1, 1, None, 0, y.data_ptr(), _stream()) == -1
    assert b"multiple of 4" in lib.stlt_last_error()
    d = pkg._lib.Conv3dDesc(1, 2, 2, 2, 4, 8, 3, 3, 3, 1, 1, 1, 1, 1, 1)
    assert lib.stlt_conv3d_fwd(ctypes.byref(d), x.data_ptr(), w.data_ptr(), None, None, None, None, 1e-5, None, 1, 4, None, 0, y.data_ptr(), _stream()) == -2


def test_pooling_and_layout_kernels_exact(pkg):
    lib = pkg._lib.load()
    g = _gen(5)
    # dyadic values (multiples of 1/64, small): every summation order gives the same float, so the average pool can be exact too
    for (B, C, T, H, W) in ((2, 64, 7, 9, 10), (1, 8, 32, 56, 56), (3, 4, 1, 2, 3)):
        x = torch.randint(-512, 512, (B, C, T, H, W), generator=g).float() / 64
        xn = _to_ndhwc(pkg, x, C)
        assert torch.equal(xn.cpu(), x.permute(0, 2, 3, 4, 1))
        ref = F.max_pool3d(x, kernel_size=3, stride=2, padding=1)
        y = torch.empty(ref.permute(0, 2, 3, 4, 1).shape, device=DEV)
        pkg._lib.check(lib.stlt_maxpool3d_ndhwc(xn.data_ptr(), B, T, H, W, C, y.data_ptr(), _stream()), "maxpool")
        assert torch.equal(y.permute(0, 4, 1, 2, 3).cpu(), ref)
        P = T * H * W
        avg = torch.empty(B, C, device=DEV)
        pkg._lib.check(lib.stlt_avgpool_ndhwc(xn.data_ptr(), B, P, C, avg.data_ptr(), _stream()), "avgpool")
        if P in (1, 2, 4, 8, 16, 32, 64):  # exact division
            assert torch.equal(avg.cpu(), F.adaptive_avg_pool3d(x, (1, 1, 1)).flatten(1))
        back = torch.empty(B, C, P, device=DEV)
        pkg._lib.check(lib.stlt_ndhwc_to_ncdhw(xn.data_ptr(), B, P, C, back.data_ptr(), _stream()), "ndhwc_to_ncdhw")
        assert torch.equal(back.cpu(), x.flatten(2))
    # the trunk's own average pool: 32 positions
    x = torch.randint(-512, 512, (2, 2048, 2, 4, 4), generator=g).float() / 64
    xn = x.permute(0, 2, 3, 4, 1).contiguous().to(DEV)
    avg = torch.empty(2, 2048, device=DEV)
    pkg._lib.check(lib.stlt_avgpool_ndhwc(xn.data_ptr(), 2, 32, 2048, avg.data_ptr(), _stream()), "avgpool")
    assert torch.equal(avg.cpu(), F.adaptive_avg_pool3d(x, (1, 1, 1)).flatten(1))


def _app_kwargs(pkg):
    kw = pkg.synth.model_kwargs("cfg1")
    return dict(num_classes=kw["num_classes"], hidden_size=kw["hidden_size"], num_attention_heads=kw["num_attention_heads"], hidden_dropout_prob=0.0,
                appearance_num_frames=32)


def _loaded(pkg, model, meta):
    sd = pkg.synth.make_r3d_state_dict({k: tuple(v.shape) for k, v in model.state_dict().items()}, seed=meta["weight_seed"])
    model.load_state_dict(sd, strict=True)
    return model.to(DEV).train(False)


@pytest.fixture(scope="module")
def video(pkg):
    _, meta = _golden()
    return pkg.synth.make_video(meta["clips"], seed=meta["video_seed"]).to(DEV)


def test_trunk_features_against_float64_golden(pkg, video):
    gold, meta = _golden()
    m = _loaded(pkg, pkg.Resnet3D(pkg.AppearanceModelConfig(**_app_kwargs(pkg))), meta)
    with torch.no_grad():
        f1 = m.forward_features({"video_frames": video})
        f2 = m.forward_features({"video_frames": video})
    ref = torch.from_numpy(gold["features_f64"]).double()  # the fp64 run, rounded to fp32 for storage (2e-6 at most)
    bound = 1e-4 * ref.abs().max().item()
    err = (f1.cpu().double() - ref).abs().max().item()
    ref32 = float(gold["features_f32_maxdiff"])  # max|fp32 reference - fp64 run|
    assert ref32 <= bound, f"the fp32 reference itself misses the bound: {ref32} > {bound}"
    assert err <= bound, f"max|trunk - fp64| = {err} > {bound} (fp32 reference: {ref32})"
    assert torch.equal(f1, f2), "two trunk forwards differ"


def test_resnet3d_and_transformer_logits(pkg, video):
    gold, meta = _golden()
    r = _loaded(pkg, pkg.Resnet3D(pkg.AppearanceModelConfig(**_app_kwargs(pkg))), meta)
    t = _loaded(pkg, pkg.TransformerResnet(pkg.AppearanceModelConfig(**_app_kwargs(pkg))), meta)
    with torch.no_grad():
        lr = r({"video_frames": video})["resnet3d"].cpu()
        lt = t({"video_frames": video})["resnet3d"].cpu()
    assert (lr - torch.from_numpy(gold["resnet3d_logits"])).abs().max().item() <= 1e-4
    assert (lt - torch.from_numpy(gold["transformer_logits"])).abs().max().item() <= 1e-4


def _cacnf(pkg, meta):
    cfg = pkg.MultimodalModelConfig(**dict(pkg.synth.model_kwargs("cfg1"), appearance_num_frames=32, num_appearance_layers=2, num_fusion_layers=2,
                                           appearance_trunk=True))
    return _loaded(pkg, pkg.CrossAttentionCentralNetFusion(cfg), meta)


def _layout_batch(pkg, meta, video):
    c = pkg.synth.CONFIGS[meta["config"]]
    batch = {k: v.to(DEV) for k, v in pkg.synth.make_batch(meta["clips"], c["T"], c["N"], seed=meta["batch_seed"]).items()}
    batch["video_frames"] = video
    return batch


def test_cacnf_from_video_frames(pkg, video):
    gold, meta = _golden()
    m = _cacnf(pkg, meta)
    batch = _layout_batch(pkg, meta, video)
    with torch.no_grad():
        out = m(batch)
        feats = m.backbone.appearance_branch.resnet.forward_features(batch)
        pre = m({k: v for k, v in batch.items() if k != "video_frames"} | {"appearance_features": feats})
    for k in ("stlt", "resnet3d", "caf", "ensemble"):
        err = (out[k].cpu() - torch.from_numpy(gold[f"cacnf_{k}"])).abs().max().item()
        assert err <= 1e-4, (k, err)
        assert torch.equal(out[k], pre[k]), k  # from video == from the trunk's own features


def test_training_rule(pkg, video):
    _, meta = _golden()
    m = _cacnf(pkg, meta)
    batch = _layout_batch(pkg, meta, video)
    batch["labels"] = torch.arange(meta["clips"], device=DEV)
    with pytest.raises(pkg.StltHipError, match=r"appearance_branch\.resnet.*requires_grad_\(False\)"):
        m(batch)
    trunk = m.backbone.appearance_branch.resnet
    trunk.requires_grad_(False)
    # eval mode: the appearance encoder's fixed dropout (0.1) is off, so the two steps draw no random masks and must agree bit for bit
    m.train(False)

    def grads(b):
        m.zero_grad(set_to_none=True)
        out = m(b)
        loss = sum(F.cross_entropy(out[k], b["labels"]) for k in ("stlt", "resnet3d", "caf"))
        loss.backward()
        return {n: p.grad.clone() for n, p in m.named_parameters() if p.grad is not None}

    g_video = grads(batch)
    with torch.no_grad():
        feats = trunk.forward_features(batch)
    g_feat = grads({k: v for k, v in batch.items() if k != "video_frames"} | {"appearance_features": feats})
    assert g_video and set(g_video) == set(g_feat) and not any(".resnet." in n for n in g_video)
    for n in g_video:
        assert torch.equal(g_video[n], g_feat[n]), n
