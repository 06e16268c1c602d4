"""Device video collater on the GPU: the golden fixture (Pillow's own crops, tools/gen_golden_video.py) through DeviceVideoCollater bit for
bit in evaluation and in training, randomized batches against the numpy restatement (tests/pil_restated.py), determinism, and the end to
end runs: Resnet3D and CACNF (appearance_trunk=True) fed by the collaters against the same models fed the expected batch."""
import json
import math
import os

import numpy as np
import pytest
import torch

import pil_restated as R
from conftest import GOLDEN

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _fixture():
    return np.load(os.path.join(GOLDEN, "video_prep.npz")), json.load(open(os.path.join(GOLDEN, "video_prep_schema.json")))


def _case(meta, name):
    return next(c for c in meta["cases"] if c["name"] == name)


def _frames(z, case):
    return [z[f"{case['name']}/src{i}"] if stored else R.pattern_clip(case["T"], h, w)
            for i, ((h, w), stored) in enumerate(zip(case["sizes"], case["stored_frames"]))]


def _samples(frames):
    return [{"frames": f, "labels": torch.tensor(i % 7), "video_id": f"v{i}"} for i, f in enumerate(frames)]


def _expected(z, case):
    return torch.from_numpy(R.video_frames(z[f"{case['name']}/crops"]))


def _params(video, p):
    if not p["train"]:
        return video.ClipParams(p["rh"], p["rw"], p["top"], p["left"])
    return video.ClipParams(p["rh"], p["rw"], p["top"], p["left"], True, tuple(p["order"]), p["b"], p["c"], p["s"], p["hue"])


@pytest.mark.parametrize("name", ["eval32", "train32", "axis32", "big112_eval", "big112_train"])
def test_fixture_bit_exact(pkg, name):
    video = pkg.video
    z, meta = _fixture()
    case = _case(meta, name)
    col = video.DeviceVideoCollater(case["S"], train=case["train"], device=DEV)
    samples = _samples(_frames(z, case))
    if case["explicit_resize"]:
        out = col(samples, [_params(video, p) for p in case["params"]])
    else:  # the collater draws: from torch's global RNG after the case's seed, as the reference would
        if case["train"]:
            torch.manual_seed(case["seed"])
        out = col(samples)
    got = out["video_frames"]
    assert got.is_cuda and got.dtype == torch.float32 and got.is_contiguous()
    want = _expected(z, case)
    assert got.shape == want.shape
    diff = (got.cpu() - want).abs().max().item()
    assert torch.equal(got.cpu(), want), f"{name}: max diff {diff}"
    assert out["video_id"] == [s["video_id"] for s in samples]
    assert torch.equal(out["labels"].cpu(), torch.stack([s["labels"] for s in samples]))


def _random_batch(rng, S, T, B):
    t = math.floor(1.15 * S)
    frames = []
    for _ in range(B):
        kind = int(rng.integers(0, 4))
        if kind == 0:
            h, w = t, int(rng.integers(t, 3 * t))  # short side == target
        elif kind == 1:
            h, w = int(rng.integers(max(8, S // 2), t)), int(rng.integers(max(8, S // 2), 2 * t))  # upscale on the short side
        else:
            h, w = int(rng.integers(t, 4 * t)), int(rng.integers(t, 4 * t))
        if rng.random() < 0.5:
            h, w = w, h
        frames.append(rng.integers(0, 256, (T, h, w, 3), dtype=np.uint8))
    return frames


@pytest.mark.parametrize("seed", range(6))
def test_random_batches_against_restatement(pkg, seed):
    video = pkg.video
    rng = np.random.default_rng(1000 + seed)
    S = (32, 112)[seed % 2]
    T = int(rng.integers(1, 33)) if S == 32 else int(rng.integers(1, 5))
    B = int(rng.integers(1, 9)) if S == 32 else int(rng.integers(1, 4))
    train = seed % 3 != 0
    frames = _random_batch(rng, S, T, B)
    col = video.DeviceVideoCollater(S, train=train, device=DEV, generator=torch.Generator().manual_seed(seed))
    params = col.params(_samples(frames))
    if seed == 5:  # explicit sizes with one axis kept
        params = [video.ClipParams(f.shape[1] if f.shape[1] >= S else S + 3, max(S, f.shape[2] // 2 + 1), 0, 0, True, (1, 3, 0, 2), 1.2, 0.8, 1.1,
                                   -0.07) for f in frames]
    got = col(_samples(frames), params)["video_frames"].cpu()
    crops = np.stack([R.clip_crops(f, dict(rh=p.rh, rw=p.rw, top=p.top, left=p.left, train=p.train, order=p.order, b=p.brightness,
                                           c=p.contrast, s=p.saturation, shift=p.hue_shift), S) for f, p in zip(frames, params)])
    want = torch.from_numpy(R.video_frames(crops))
    assert torch.equal(got, want), f"max diff {(got - want).abs().max().item()}"


def test_same_seed_same_bits(pkg):
    video = pkg.video
    rng = np.random.default_rng(77)
    frames = _random_batch(rng, 112, 4, 3)
    runs = []
    for _ in range(2):
        col = video.DeviceVideoCollater(112, train=True, device=DEV, generator=torch.Generator().manual_seed(5))
        runs.append(col(_samples(frames))["video_frames"].cpu())
    assert torch.equal(runs[0], runs[1])
    other = video.DeviceVideoCollater(112, train=True, device=DEV, generator=torch.Generator().manual_seed(6))(_samples(frames))["video_frames"]
    assert not torch.equal(runs[0], other.cpu())


def _r3d(pkg, cls, cfg_cls, **extra):
    # 8 frames of 112 x 112 leave 1 x 4 x 4 trunk positions: the appearance branch's position table is sized by appearance_num_frames
    kw = pkg.synth.model_kwargs("cfg1")
    base = dict(num_classes=kw["num_classes"], hidden_size=kw["hidden_size"], num_attention_heads=kw["num_attention_heads"], hidden_dropout_prob=0.0,
                appearance_num_frames=16)
    cfg = cfg_cls(**base) if not extra else cfg_cls(**dict(kw, appearance_num_frames=16, **extra))
    m = cls(cfg)
    sd = pkg.synth.make_r3d_state_dict({k: tuple(v.shape) for k, v in m.state_dict().items()}, seed=4242)
    m.load_state_dict(sd, strict=True)
    return m.to(DEV).train(False)


def test_resnet3d_from_the_collater_matches_the_expected_batch(pkg):
    z, meta = _fixture()
    case = _case(meta, "big112_eval")  # T = 8, S = 112
    out = pkg.video.DeviceVideoCollater(112, device=DEV)(_samples(_frames(z, case)))
    m = _r3d(pkg, pkg.Resnet3D, pkg.AppearanceModelConfig)
    with torch.no_grad():
        a = m({"video_frames": out["video_frames"]})["resnet3d"]
        b = m({"video_frames": _expected(z, case).to(DEV)})["resnet3d"]
    assert torch.isfinite(a).all() and torch.equal(a, b)


def test_multimodal_collater_feeds_cacnf(pkg):
    z, meta = _fixture()
    case = _case(meta, "big112_eval")
    frames = _frames(z, case) * 2  # B = 2
    layout = pkg.synth.make_video_samples("something", 2, pkg.synth.CONFIGS["cfg1"]["N"], seed=3)
    samples = [{"layout": lay, "appearance": app} for lay, app in zip(layout, _samples(frames))]
    batch = pkg.video.DeviceMultimodalCollater("something", 112, train=False, device=DEV)(samples)
    host = pkg.collate.DeviceCollater("something", DEV)(layout)  # the layout half as DeviceCollater alone makes it
    host["video_frames"] = _expected(z, case).repeat(2, 1, 1, 1, 1).to(DEV)
    for k in ("categories", "boxes", "frame_types", "src_key_padding_mask_boxes", "src_key_padding_mask_frames", "lengths"):
        assert torch.equal(batch[k], host[k]), k
    assert torch.equal(batch["video_frames"], host["video_frames"])
    assert torch.equal(batch["labels"].cpu(), torch.stack([s["appearance"]["labels"] for s in samples]))  # appearance keys last
    m = _r3d(pkg, pkg.CrossAttentionCentralNetFusion, pkg.MultimodalModelConfig, num_appearance_layers=2, num_fusion_layers=2, appearance_trunk=True)
    with torch.no_grad():
        got = m(batch)
        want = m(host)
    for k in ("stlt", "resnet3d", "caf", "ensemble"):
        assert torch.isfinite(got[k]).all() and torch.equal(got[k], want[k]), k
