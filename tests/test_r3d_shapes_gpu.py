"""The whole R3D-50 trunk across shapes and batches against the float64 CPU oracle (oracle/r3d_oracle.py), which is pinned to the
reference at the golden shape by tests/test_r3d_oracle_cpu.py.  The split plans of every conv depend on (B, T, H, W), so each shape runs
other summation orders and other parity classes than the golden (2, 32, 112, 112) (tests/test_r3d_plans_cpu.py asserts what the
sweep reaches).  Weights: synth.make_r3d_state_dict; video: synth.make_video(B, T, H, W, seed).

At every shape: features and pooled features within 1e-4 · max|oracle float64| (the golden test's bar); the training forward
(stlt_r3d_train_forward, under R3dTrunkFn) bit for bit the inference forward (stlt_r3d_forward); two runs bit-identical.
Weight gradients (through R3dTrunkFn, seeded gradients on the feature map and on the pooled features) per conv against float64 by the
golden test's rule (test_r3d_train_gpu._bound): 5e-4 · max|g| where float32 runs of the oracle at the same shape are within 1e-4 of
float64, otherwise 8x their largest distance, capped at 3 % (a float32 run flips a few near-zero ReLU masks: its distance is what
float32 itself gets wrong at that conv)."""
import pytest
import torch

from oracle import r3d_oracle as O
from test_r3d_train_gpu import _bound

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
WEIGHT_SEED = 4242
FWD_REL = 1e-4
# (B, T, H, W): "grad" = forward and weight gradients, "fwd" = forward only
SHAPES = {
    (1, 16, 112, 112): "grad",  # 16 frames: To = 1
    (3, 9, 97, 75): "grad",     # non-square; odd extents under the stride-2 convs: (5, 25, 19), (3, 13, 10), (2, 7, 5)
    (1, 8, 64, 64): "grad",     # Ti = 1 at layer 4's stride-2 convs: parity classes without rows
    (8, 32, 112, 112): "grad",  # wgrad plans up to ~240 splits
    (2, 16, 224, 224): "fwd",   # 224 pixels
    (16, 32, 112, 112): "fwd",  # the benchmarks' batch
}
BIG = (64, 32, 112, 112)  # checked against four 16-clip runs of the same clips (GPU only); WG_SPLIT_MAX-sized plans
GRAD_SHAPES = [s for s, kind in SHAPES.items() if kind == "grad"]


def _seed(shape):
    return 500 + list(SHAPES).index(shape)


@pytest.fixture(scope="module")
def model(pkg):
    kw = pkg.synth.model_kwargs("cfg1")
    cfg = pkg.AppearanceModelConfig(num_classes=kw["num_classes"], hidden_size=kw["hidden_size"], num_attention_heads=kw["num_attention_heads"],
                                    hidden_dropout_prob=0.0, appearance_num_frames=32, train_trunk=True)
    m = pkg.Resnet3D(cfg)
    sd = pkg.synth.make_r3d_state_dict({k: tuple(v.shape) for k, v in m.state_dict().items()}, seed=WEIGHT_SEED)
    m.load_state_dict(sd, strict=True)
    return m.to(DEV).train(True), sd


def _features(m, v):
    return m._runner.run(m.resnet, v, features=True)[0]


def _pooled(m, v):
    return m._runner.run(m.resnet, v, features=False, pooled=True)[1]


def _rel_err(got, want):
    return (got.detach().cpu().double() - want).abs().max().item() / want.abs().max().item()


@pytest.mark.parametrize("shape", list(SHAPES), ids=lambda s: "x".join(map(str, s)))
def test_trunk_forward_against_float64(pkg, model, shape):
    m, sd = model
    video = pkg.synth.make_video(*shape, seed=_seed(shape))
    ref = O.forward(sd, video, torch.float64)
    v = video.to(DEV)
    with torch.no_grad():
        f1, p1 = _features(m, v), _pooled(m, v)
        f2, p2 = _features(m, v), _pooled(m, v)
    assert f1.shape == ref["features"].shape and p1.shape == ref["pooled"].shape
    ef, ep = _rel_err(f1, ref["features"]), _rel_err(p1, ref["pooled"])
    print(f"[r3d sweep] forward {shape}: features err/bound {ef / FWD_REL:.3f}, pooled err/bound {ep / FWD_REL:.3f}")
    assert ef <= FWD_REL and ep <= FWD_REL, (shape, ef, ep)
    assert torch.equal(f1, f2) and torch.equal(p1, p2), "two trunk forwards differ"
    # the training forward (R3dTrunkFn: stlt_r3d_train_forward, which records the tape) is bit for bit the inference forward
    ft, pt = _features(m, v), _pooled(m, v)
    assert ft.requires_grad and pt.requires_grad
    assert torch.equal(ft.detach(), f1) and torch.equal(pt.detach(), p1), "training forward differs from the inference forward"


@pytest.mark.parametrize("shape", GRAD_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_trunk_weight_gradients_against_float64(pkg, model, shape):
    m, sd = model
    B, T, H, W = shape
    video = pkg.synth.make_video(*shape, seed=_seed(shape))
    g = torch.Generator().manual_seed(_seed(shape))
    To, Ho, Wo = pkg.modelling.resnet3d._trunk_out(T), pkg.modelling.resnet3d._trunk_out(H, 2), pkg.modelling.resnet3d._trunk_out(W, 2)
    # positive seeded gradients on both outputs (the pooled one scaled so its share is as large as the map's): with random signs the
    # weight gradients cancel down to where a float32 run's ReLU mask flips dominate on most convs, and every bound would be loose
    dfeat = torch.rand(B, 2048, To, Ho, Wo, generator=g)
    dpool = torch.rand(B, 2048, generator=g) * (To * Ho * Wo) ** 0.5
    r64 = O.weight_grads(sd, video, torch.float64, dfeatures=dfeat, dpooled=dpool)["grads"]
    # float32 calibration: two runs in different summation orders, the plain one and the same problem with H and W exchanged (exact:
    # every stride and pad of the trunk is equal in h and w); which near-zero ReLU masks float32 flips depends on the order, so one
    # run can miss a flip that another float32 order (the kernels') makes
    r32 = O.weight_grads(sd, video, torch.float32, dfeatures=dfeat, dpooled=dpool)["grads"]
    sd_t = {k: (v.transpose(-1, -2).contiguous() if v.dim() == 5 else v) for k, v in sd.items()}
    r32_t = O.weight_grads(sd_t, video.transpose(-1, -2).contiguous(), torch.float32, dfeatures=dfeat.transpose(-1, -2).contiguous(),
                           dpooled=dpool)["grads"]
    ws = [conv.weight for conv, _ in pkg.modelling.resnet3d.trunk_convs(m.resnet)]
    v, df, dp = video.to(DEV), dfeat.to(DEV), dpool.to(DEV)
    g_feat = torch.autograd.grad(_features(m, v), ws, df)
    g_pool = torch.autograd.grad(_pooled(m, v), ws, dp)
    assert all(torch.equal(a, b) for a, b in zip(g_feat, torch.autograd.grad(_features(m, v), ws, df))), "two backward passes differ"
    bad, tight, worst = [], 0, 0.0
    for i, (a, b, want, ref32, ref32_t) in enumerate(zip(g_feat, g_pool, r64, r32, r32_t)):
        gmax = want.abs().max().item()
        rel32 = max((ref32.double() - want).abs().max().item(), (ref32_t.transpose(-1, -2).double() - want).abs().max().item()) / gmax
        bound = _bound(rel32)
        err = ((a + b).cpu().double() - want).abs().max().item() / gmax
        tight += rel32 <= 1e-4
        worst = max(worst, err / bound)
        if err > bound:
            bad.append((i, err, bound, rel32))
    print(f"[r3d sweep] wgrad {shape}: {tight} of 53 convs tight, worst err/bound {worst:.3f}")
    assert not bad, (shape, f"{tight} of 53 convs tight", bad)


def test_batch64_against_four_batches_of_16(pkg, model):
    """B = 64 runs other split plans than B = 16; both are within FWD_REL · max|oracle| of the oracle (checked at 16 clips above),
    so they may differ by the sum of the two bounds (max|oracle| taken as the 16-clip run's max, FWD_REL from it)."""
    m, _ = model
    v = pkg.synth.make_video(*BIG, seed=_seed((16, 32, 112, 112))).to(DEV)  # its first 16 clips are those checked against the oracle
    with torch.no_grad():
        f, p = _features(m, v), _pooled(m, v)
        assert torch.equal(f, _features(m, v)), "two trunk forwards differ"
        worst = 0.0
        for c in range(4):
            sl = slice(16 * c, 16 * (c + 1))
            f16, p16 = _features(m, v[sl]), _pooled(m, v[sl])
            for got, want in ((f[sl], f16), (p[sl], p16)):
                r = (got - want).abs().max().item() / (2 * FWD_REL * want.abs().max().item())
                worst = max(worst, r)
                assert r <= 1, (c, r)
    print(f"[r3d sweep] forward {BIG} vs 4 x 16 clips: err/bound {worst:.3f}")
    ft = _features(m, v)
    assert torch.equal(ft.detach(), f), "training forward differs from the inference forward"
