"""Grad-CAM, host side: the names in the header, the ctypes table, the ops wrappers and the export map; the refusals that need no GPU; the
NumPy restatement (tests/gradcam_restated.py) against torch autograd on a toy network — the unmasked-gradient convention and both variants
— and against F.interpolate; stlt_r3d_layer_geometry against the oracle's stage shapes, the ceil chain and the tape.  No GPU."""
import fnmatch
import inspect
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import gradcam_restated as R
from conftest import ROOT
from oracle import r3d_oracle as O
from test_r3d_shapes_gpu import SHAPES

NAMES = ("stlt_cam_scratch_bytes", "stlt_cam_weights", "stlt_cam_map", "stlt_cam_upsample", "stlt_r3d_layer_geometry", "stlt_r3d_backward_layer")
WRAPPERS = ("cam_weights", "cam_map", "cam_upsample", "r3d_layer_geometry", "r3d_backward_layer")
CHANNELS = {1: 256, 2: 512, 3: 1024, 4: 2048}


def test_the_names_are_declared_bound_wrapped_and_exported(pkg):
    header = open(os.path.join(ROOT, "include", "stlt_hip.h")).read()
    export_map = open(os.path.join(ROOT, "revisiting-spatial-temporal-layouts_amd", "csrc", "exports.map")).read()
    patterns = re.search(r"global:([^;]*);", export_map).group(1).split()
    lib = pkg._lib.load()
    flat = re.sub(r"\s+", " ", header)
    for name in NAMES:
        m = re.search(rf"\b(?:int|size_t) {name}\(([^)]*)\);", flat)
        assert m, f"{name} is not declared in include/stlt_hip.h"
        assert name in pkg._lib.SIGNATURES, f"{name} has no ctypes signature"
        n_args = len([a for a in m.group(1).split(",") if a.strip() and a.strip() != "void"])
        assert len(pkg._lib.SIGNATURES[name][1]) == n_args, f"{name}: the header declares {n_args} arguments, _lib.py binds {len(pkg._lib.SIGNATURES[name][1])}"
        assert any(fnmatch.fnmatchcase(name, pat) for pat in patterns), f"{name} is not a global of csrc/exports.map"
        assert hasattr(lib, name)
    for w in WRAPPERS:
        assert callable(getattr(pkg.ops, w)) and "include/stlt_hip.h" in inspect.getdoc(getattr(pkg.ops, w)), w
    for macro, value in (("STLT_CAM_NDHWC", pkg._lib.CAM_LAYOUTS["ndhwc"]), ("STLT_CAM_NCDHW", pkg._lib.CAM_LAYOUTS["ncdhw"]), ("STLT_CAM_CHUNK", pkg._lib.CAM_CHUNK)):
        assert re.search(rf"#define {macro}\s+{value}\b", header), macro
    assert "gradcam.hip" in __import__(pkg.__name__ + ".build", fromlist=["SOURCES"]).SOURCES
    # host arithmetic: one partial per chunk of positions, none when one chunk holds them all or the shape is refused
    ch = pkg._lib.CAM_CHUNK
    assert lib.stlt_cam_scratch_bytes(3, ch, 7) == 0 and lib.stlt_cam_scratch_bytes(3, ch + 1, 7) == 3 * 2 * 7 * 4
    assert lib.stlt_cam_scratch_bytes(3, 0, 7) == 0 and lib.stlt_cam_scratch_bytes(2, 1 << 20, 1 << 12) == 0
    for key in ("resnet3d", "resnet3d-transformer", "caf", "cacnf", "lcf"):
        assert callable(getattr(pkg.models_factory[key], "forward_gradcam")), key
    assert not hasattr(pkg.Stlt, "forward_gradcam")
    assert "gradcam" in pkg.infer._PERTURB_METHODS


def test_refusals_without_a_gpu(pkg):
    cfg = pkg.AppearanceModelConfig(num_classes=5, hidden_size=64, num_attention_heads=4, hidden_dropout_prob=0.0, appearance_num_frames=32)
    m = pkg.Resnet3D(cfg).train(False)
    batch = {"video_frames": torch.zeros(1, 3, 8, 64, 64)}
    with pytest.raises(pkg.StltHipError, match="CPU"):
        m.forward_gradcam(batch)
    for bad in (0, 5, -1, 2.0, True):
        with pytest.raises(pkg.StltHipError, match="layer"):
            m.forward_gradcam(batch, layer=bad)
    with pytest.raises(pkg.StltHipError, match="variant"):
        m.forward_gradcam(batch, variant="gradcam++")
    with pytest.raises(pkg.StltHipError, match="video_frames"):
        m.forward_gradcam({})
    with pytest.raises(pkg.StltHipError, match="convolution"):
        pkg.infer.run_perturbation_test(m, [batch], method="gradcam", modality="layout")
    with pytest.raises(pkg.StltHipError, match="convolution"):
        pkg.infer.attribution_scores(m, batch, "gradcam")
    lib = pkg._lib.load()
    for call in (lambda: lib.stlt_cam_weights(None, 2, 8, 4, 0, 16, None, 0, None),           # NULL g
                 lambda: lib.stlt_cam_weights(16, 2, 0, 4, 0, 16, None, 0, None),             # P < 1
                 lambda: lib.stlt_cam_weights(16, 2, 8, 0, 1, 16, None, 0, None),             # C < 1
                 lambda: lib.stlt_cam_weights(16, 2, 8, 4, 2, 16, None, 0, None),             # an unknown layout
                 lambda: lib.stlt_cam_weights(18, 2, 8, 4, 1, 16, None, 0, None),             # g off its 4 bytes
                 lambda: lib.stlt_cam_weights(16, 2, 1 << 20, 1 << 12, 0, 16, None, 0, None),  # 2^31 elements and more
                 lambda: lib.stlt_cam_map(16, None, 0, 2, 8, 4, 0, 1, 16, None),              # NULL w
                 lambda: lib.stlt_cam_map(16, 16, 0, -1, 8, 4, 0, 1, 16, None),               # B < 0
                 lambda: lib.stlt_cam_map(16, 16, 1, 2, 8, 4, 7, 1, 16, None),                # an unknown layout
                 lambda: lib.stlt_cam_map(16, 16, 1, 2, 8, 4, 1, 1, 17, None),                # cam off its 4 bytes
                 lambda: lib.stlt_cam_upsample(None, 1, 2, 2, 2, 4, 4, 4, 16, None),          # NULL cam
                 lambda: lib.stlt_cam_upsample(16, 1, 0, 2, 2, 4, 4, 4, 16, None),            # an empty grid
                 lambda: lib.stlt_cam_upsample(16, 1, 2, 2, 2, 4, 0, 4, 16, None),            # an empty output
                 lambda: lib.stlt_cam_upsample(16, 64, 2, 2, 2, 1024, 1024, 1024, 16, None)):  # 2^31 elements and more
        assert call() == -1
        assert lib.stlt_last_error().decode().startswith("stlt_cam_")
    assert lib.stlt_cam_weights(16, 2, 33, 4, 0, 16, None, 0, None) == -2 and "scratch" in lib.stlt_last_error().decode()  # two chunks, no scratch
    assert lib.stlt_cam_weights(None, 0, 8, 4, 0, None, None, 0, None) == 0  # an empty batch
    for layer in (0, 4, -3):
        assert lib.stlt_r3d_backward_layer(None, None, None, 0, 1, 8, 64, 64, None, None, layer, 16, None, 0, None) == -1
        assert "layer" in lib.stlt_last_error().decode()
    assert lib.stlt_r3d_backward_layer(None, None, None, 0, 1, 8, 64, 64, None, None, 2, 24, None, 0, None) == -1  # dlayer off its 16 bytes
    assert "dlayer" in lib.stlt_last_error().decode() and "aligned" in lib.stlt_last_error().decode()
    for layer in (0, 5):
        with pytest.raises(pkg.StltHipError, match="layer"):
            pkg.ops.r3d_layer_geometry(1, 8, 64, 64, layer)


@pytest.mark.parametrize("variant", ["gradcam", "hirescam"])
@pytest.mark.parametrize("relu", [True, False])
def test_restated_gradcam_equals_autograd_on_a_toy_network(variant, relu):
    """conv - ReLU (the tapped stage output) - conv - ReLU - average pool - linear in float64: the gradient the map is made from is the one
    autograd gives at the tensor AFTER the first ReLU, zeros of that ReLU's output included (no mask of the tapped output is applied)."""
    g = torch.Generator().manual_seed(11)
    x = torch.randn(2, 3, 4, 6, 5, generator=g, dtype=torch.float64)
    w1, w2 = torch.randn(7, 3, 3, 3, 3, generator=g, dtype=torch.float64) * 0.3, torch.randn(6, 7, 3, 3, 3, generator=g, dtype=torch.float64) * 0.3
    wc = torch.randn(4, 6, generator=g, dtype=torch.float64)
    target = torch.tensor([1, 3])
    a = F.conv3d(x, w1, padding=1).relu().detach().requires_grad_(True)
    logits = F.conv3d(a, w2, stride=2, padding=1).relu().mean(dim=(2, 3, 4)) @ wc.T
    (grad,) = torch.autograd.grad(logits[torch.arange(2), target].sum(), a)
    dead = a.detach() == 0
    assert dead.any() and (grad[dead] != 0).any(), "the case must hold zeros of the tapped ReLU that carry a gradient"
    if variant == "gradcam":
        want = (grad.mean(dim=(2, 3, 4), keepdim=True) * a.detach()).sum(dim=1)
    else:
        want = (grad * a.detach()).sum(dim=1)
    want = (want.relu() if relu else want).flatten(1).numpy()
    got = R.gradcam(a.detach().numpy(), grad.numpy(), "ncdhw", variant, relu)
    assert np.abs(got - want).max() <= 1e-13 * np.abs(want).max()
    # the same numbers from the other layout
    nd = lambda t: t.permute(0, 2, 3, 4, 1).contiguous().numpy()  # noqa: E731
    assert np.abs(R.gradcam(nd(a.detach()), nd(grad), "ndhwc", variant, relu) - want).max() <= 1e-13 * np.abs(want).max()
    # a masked gradient, the mistake this convention rules out, is a different map
    masked = R.gradcam(a.detach().numpy(), (grad * ~dead).numpy(), "ncdhw", variant, relu)
    if variant == "gradcam":
        assert np.abs(masked - want).max() > 1e-6 * np.abs(want).max()


@pytest.mark.parametrize("grid,size", [((1, 2, 3), (5, 4, 7)), ((2, 4, 4), (32, 112, 112))])
def test_restated_upsample_equals_interpolate(grid, size):
    cam = torch.randn(2, *grid, generator=torch.Generator().manual_seed(3), dtype=torch.float64)
    want = F.interpolate(cam[:, None], size=size, mode="trilinear", align_corners=False)[:, 0].numpy()
    got = R.upsample(cam.numpy(), size)
    assert got.shape == want.shape and np.abs(got - want).max() <= 1e-13 * np.abs(want).max()


def test_restated_cell_pool():
    cam = np.random.default_rng(5).standard_normal((2, 3, 7, 5))
    got = R.pool_cells(cam, (2, 2, 2))
    assert got.shape == (2, 2 * 4 * 3) and np.allclose(got.sum(axis=1), cam.reshape(2, -1).sum(axis=1))
    assert np.isclose(got[0, 0], cam[0, :2, :2, :2].sum()) and np.isclose(got[1, -1], cam[1, 2:, 6:, 4:].sum())


@pytest.mark.parametrize("shape", [(1, 8, 64, 64), (3, 9, 97, 75)], ids=lambda s: "x".join(map(str, s)))
def test_layer_geometry_equals_the_oracle_stage_shapes(pkg, shape):
    m = pkg.Resnet3D(pkg.AppearanceModelConfig(num_classes=5, hidden_size=64, num_attention_heads=4, hidden_dropout_prob=0.0, appearance_num_frames=32))
    sd = pkg.synth.make_r3d_state_dict({k: tuple(v.shape) for k, v in m.state_dict().items()}, seed=1)
    stages = O.forward(sd, pkg.synth.make_video(*shape, seed=2), torch.float32, with_stages=True)["stages"]
    for layer in (1, 2, 3, 4):
        (t, h, w, c), _ = pkg.ops.r3d_layer_geometry(*shape, layer)
        assert (shape[0], c, t, h, w) == tuple(stages[f"layer{layer}"].shape), layer


@pytest.mark.parametrize("shape", list(SHAPES), ids=lambda s: "x".join(map(str, s)))
def test_layer_geometry_is_the_ceil_chain_inside_the_tape(pkg, shape):
    lib = pkg._lib.load()
    B, T, H, W = shape
    half = lambda n: -(-n // 2)  # noqa: E731
    t, h, w = half(T), half(half(H)), half(half(W))  # the stem (stride 1, 2, 2), then the max-pool
    tape = lib.stlt_r3d_tape_bytes(*shape)
    seen = []
    for layer in (1, 2, 3, 4):
        if layer > 1:
            t, h, w = half(t), half(h), half(w)
        dims, off = pkg.ops.r3d_layer_geometry(*shape, layer)
        assert dims == (t, h, w, CHANNELS[layer]), (layer, dims)
        assert off % 256 == 0 and 0 < off and off + B * t * h * w * CHANNELS[layer] * 4 <= tape, (layer, off, tape)
        seen.append(off)
    assert seen == sorted(set(seen))
    assert dims[:3] == tuple(pkg.modelling.resnet3d._trunk_out(n, s) for n, s in ((T, 1), (H, 2), (W, 2)))


@pytest.mark.parametrize("shape", [(0, 8, 64, 64), (1, 0, 64, 64), (-1, 8, 64, 64), (1, 8, 64, 5000), (1 << 21, 8, 64, 64), (1, 8, 0, 64)])
def test_layer_geometry_fails_where_the_tape_is_empty(pkg, shape):
    lib = pkg._lib.load()
    assert lib.stlt_r3d_tape_bytes(*shape) == 0
    with pytest.raises(pkg.StltHipError, match="stlt_r3d_layer_geometry"):
        pkg.ops.r3d_layer_geometry(*shape, 2)
    assert lib.stlt_r3d_tape_bytes(1, 1, 1, 1) > 0 and pkg.ops.r3d_layer_geometry(1, 1, 1, 1, 4)[0] == (1, 1, 1, 2048)
