"""Device frame store and the appearance / multimodal datasets on the GPU.  Everything is integer or table arithmetic the video collater
already matches to Pillow, so every comparison is torch.equal: the stored frames against the numpy restatement of Pillow's resize
(tests/pil_restated.py) for the sources of tests/golden/video_prep.npz and for random sizes; batches from the store against Pillow's own
crops (video_prep.npz) and against DeviceVideoCollater.prep on the same frames and parameters, with repeated frame indices and mixed
resident / spilled clips; encoded input; two shuffled training epochs of DeviceMultimodalDataset.loader() against the fixture's draws
(tests/golden/frame_data.npz); Resnet3D and CACNF logits, a Trainer step and inference passes from the loaders; a captured graph."""
import io
import itertools
import json
import math
import os
import types

import numpy as np
import pytest
import torch

import layout_restated as LR
import pil_restated as R
from conftest import GOLDEN

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def fd(pkg):
    return pkg.frame_data


def _video_fixture():
    return np.load(os.path.join(GOLDEN, "video_prep.npz")), json.load(open(os.path.join(GOLDEN, "video_prep_schema.json")))


def _frame_fixture():
    return np.load(os.path.join(GOLDEN, "frame_data.npz")), json.load(open(os.path.join(GOLDEN, "frame_data_schema.json")))


def _case(meta, name):
    return next(c for c in meta["cases"] if c["name"] == name)


def _clips(z, case):
    return [z[f"{case['name']}/src{i}"] if stored else R.pattern_clip(case["T"], h, w)
            for i, ((h, w), stored) in enumerate(zip(case["sizes"], case["stored_frames"]))]


def _source(clips):
    """source[video_id][str(frame)] over a list of (n, h, w, 3) uint8 arrays."""
    return {f"v{i}": {str(j): c[j] for j in range(len(c))} for i, c in enumerate(clips)}, [f"v{i}" for i in range(len(clips))]


def _params(video, p):
    if not p["train"]:
        return video.ClipParams(p["rh"], p["rw"], p["top"], p["left"])
    return video.ClipParams(p["rh"], p["rw"], p["top"], p["left"], True, tuple(p["order"]), p["b"], p["c"], p["s"], p["hue"])


def _check_stored(store, clips):
    for i, c in enumerate(clips):
        rh, rw = R.resized_size(c.shape[1], c.shape[2], store.target)
        want = torch.from_numpy(np.stack([R.resize(f, rh, rw) for f in c]))
        got = store.frames(i).cpu()
        assert got.shape == want.shape and torch.equal(got, want), (i, c.shape)


@pytest.mark.parametrize("name", ["eval32", "train32", "axis32", "big112_eval", "big112_train"])
def test_stored_frames_equal_the_restated_resize_on_the_fixture_sources(fd, name):
    z, meta = _video_fixture()
    case = _case(meta, name)
    clips = _clips(z, case)
    store = fd.DeviceFrameStore(*_source(clips), spatial_size=case["S"], device=DEV)
    _check_stored(store, clips)
    assert store.nbytes == sum(int(store.frames(i).numel()) for i in range(len(clips)))


def _random_clips(rng, S, counts):
    """Both orientations; short side equal to the target, below it (upscaled) and above it."""
    t = math.floor(1.15 * S)
    clips = []
    for i, n in enumerate(counts):
        kind = i % 4
        if kind == 0:
            h, w = t, int(rng.integers(t, 3 * t))  # short side == target: stored as it is
        elif kind == 1:
            h, w = int(rng.integers(max(8, S // 2), t)), int(rng.integers(max(8, S // 2), 2 * t))  # smaller than the target
        elif kind == 2:
            h, w = t, t
        else:
            h, w = int(rng.integers(t + 1, 4 * t)), int(rng.integers(t + 1, 4 * t))
        if rng.random() < 0.5:
            h, w = w, h
        clips.append(rng.integers(0, 256, (int(n), h, w, 3), dtype=np.uint8))
    return clips


@pytest.mark.parametrize("seed,S", [(0, 32), (1, 32), (2, 112), (3, 17)])
def test_stored_frames_equal_the_restated_resize_on_random_sizes(fd, seed, S):
    rng = np.random.default_rng(500 + seed)
    clips = _random_clips(rng, S, rng.integers(1, 6 if S < 112 else 3, size=12 if S < 112 else 8))
    store = fd.DeviceFrameStore(*_source(clips), spatial_size=S, device=DEV)
    _check_stored(store, clips)


@pytest.mark.parametrize("name", ["eval32", "train32", "big112_eval", "big112_train"])
def test_fixture_batches_equal_pillows_crops(fd, pkg, name):
    video = pkg.video
    z, meta = _video_fixture()
    case = _case(meta, name)
    clips = _clips(z, case)
    store = fd.DeviceFrameStore(*_source(clips), spatial_size=case["S"], device=DEV)
    v = list(range(len(clips)))
    fi = np.tile(np.arange(case["T"]), (len(clips), 1))
    want = torch.from_numpy(R.video_frames(z[f"{name}/crops"]))
    params = [_params(video, p) for p in case["params"]]
    got = store.gather(v, fi, params)
    assert got.is_cuda and got.dtype == torch.float32 and got.is_contiguous() and got.shape == want.shape
    assert torch.equal(got.cpu(), want), f"{name}: max diff {(got.cpu() - want).abs().max().item()}"
    if case["train"]:  # the store draws what the reference would after the case's seed
        torch.manual_seed(case["seed"])
        drawn = store.clip_params(v, True)
        assert [(p.rh, p.rw, p.top, p.left, p.order) for p in drawn] == [(p.rh, p.rw, p.top, p.left, p.order) for p in params]
        assert torch.equal(store.gather(v, fi, drawn).cpu(), want)
    else:  # no parameters: the centre crop
        assert torch.equal(store.gather(v, fi).cpu(), want)


def test_parameters_for_another_resize_are_refused(fd, pkg):
    """axis32 resizes to sizes Resize(floor(1.15 S)) does not give; the store holds the reference's resize only."""
    z, meta = _video_fixture()
    case = _case(meta, "axis32")
    clips = _clips(z, case)
    store = fd.DeviceFrameStore(*_source(clips), spatial_size=case["S"], device=DEV)
    with pytest.raises(pkg.StltHipError, match="the store holds"):
        store.gather([0, 1, 2], np.tile(np.arange(case["T"]), (3, 1)), [_params(pkg.video, p) for p in case["params"]])


@pytest.mark.parametrize("seed", range(6))
def test_random_batches_equal_the_video_collater(fd, pkg, seed):
    video = pkg.video
    rng = np.random.default_rng(900 + seed)
    S = (32, 112, 32, 23)[seed % 4]
    train = seed % 2 == 1
    T = int(rng.integers(3, 17)) if S < 112 else 4
    counts = rng.integers(1, 3 * T, size=10 if S < 112 else 6)
    counts[1] = 3  # a 3-frame video: repeated indices
    clips = _random_clips(rng, S, counts)
    source, ids = _source(clips)
    full = fd.DeviceFrameStore(source, ids, spatial_size=S, device=DEV)
    cut = fd.DeviceFrameStore(source, ids, spatial_size=S, device=DEV, capacity_bytes=int(full.video_bytes[:len(ids) // 2].sum()) + 5)
    assert cut.resident(0) and not cut.resident(len(ids) - 1) and cut.nbytes < full.nbytes == full.total_bytes
    v = np.concatenate([[1, len(ids) - 1, 0], rng.integers(0, len(ids), size=5)])
    np.random.seed(seed)
    fi = np.asarray([fd.appearance_indices(T, int(counts[i]), train) for i in v])
    assert len(set(fi[0].tolist())) < T  # the 3-frame video repeats frames
    params = full.clip_params(v, train, torch.Generator().manual_seed(seed))
    col = video.DeviceVideoCollater(S, train=train, device=DEV)
    want = col.prep([torch.from_numpy(clips[i][fi[b]]) for b, i in enumerate(v)], params)
    for store in (full, cut):
        got = store.gather(v, fi, params if train else None)
        assert torch.equal(got, want), f"max diff {(got - want).abs().max().item()}"
        if not train:
            assert torch.equal(store.gather(v, fi, params), want)
    assert {cut.resident(int(i)) for i in v} == {True, False}  # the batch mixed resident and spilled clips
    with pytest.raises(IndexError):
        full.gather([1], np.asarray([[0, 3]]))


def test_encoded_frames_ingest_like_decoded_ones(fd):
    Image = pytest.importorskip("PIL.Image")
    rng = np.random.default_rng(7)
    smooth = R.pattern_clip(3, 60, 81)
    noisy = rng.integers(0, 256, (3, 47, 40, 3), dtype=np.uint8)

    def encode(frame, fmt):
        b = io.BytesIO()
        Image.fromarray(frame, "RGB").save(b, fmt, **({"quality": 90} if fmt == "JPEG" else {}))
        return b.getvalue()

    for fmt in ("PNG", "JPEG"):
        enc = {"a": {str(j): encode(f, fmt) for j, f in enumerate(smooth)},
               "b": {str(j): np.frombuffer(encode(f, fmt), np.uint8) for j, f in enumerate(noisy)}}  # bytes, and bytes as an HDF5 file gives them
        dec = {k: {j: np.asarray(Image.open(io.BytesIO(bytes(f)))) for j, f in fr.items()} for k, fr in enc.items()}
        if fmt == "PNG":
            assert np.array_equal(dec["a"]["1"], smooth[1]) and np.array_equal(dec["b"]["2"], noisy[2])
        a = fd.DeviceFrameStore(enc, ["a", "b"], spatial_size=32, device=DEV)
        b = fd.DeviceFrameStore(dec, ["a", "b"], spatial_size=32, device=DEV)
        for i in range(2):
            assert torch.equal(a.frames(i), b.frames(i))
        fi = np.asarray([[0, 2, 1], [1, 1, 0]])
        assert torch.equal(a.gather([0, 1], fi), b.gather([0, 1], fi))
    with pytest.raises(ValueError, match="mode"):
        grey = io.BytesIO()
        Image.fromarray(smooth[0, :, :, 0], "L").save(grey, "PNG")
        fd.DeviceFrameStore({"g": {"0": grey.getvalue()}}, ["g"], spatial_size=32, device=DEV).ingest()


def _epoch_setup(pkg, tmp_path, train, S=32, T_app=None, frame_hw=(40, 52), seed=31):
    z, meta = _frame_fixture()
    e = meta["epoch"]
    p, digest = pkg.synth.write_layout_annotations(str(tmp_path), e["dataset"], e["n_videos"], e["annotation_seed"])
    assert digest == e["digest"]
    cfg = types.SimpleNamespace(dataset_name=e["dataset"], dataset_path=p["annotations"], labels_path=p["labels"], videoid2size_path=p["sizes"],
                                videos_path="", train=train, layout_num_frames=e["layout_num_frames"],
                                appearance_num_frames=T_app or e["appearance_num_frames"], spatial_size=S, score_threshold=0.5, max_num_objects=7)
    ids = [v["id"] for v in json.load(open(p["annotations"]))]
    rng = np.random.default_rng(seed)
    clips = [rng.integers(0, 256, (int(n), *frame_hw, 3), dtype=np.uint8) for n in z["epoch/frame_counts"]]
    return z, e, cfg, p, ids, clips, {vid: {str(j): c[j] for j in range(len(c))} for vid, c in zip(ids, clips)}


def test_multimodal_loader_epochs_equal_the_fixture_draws(fd, pkg, tmp_path):
    video = pkg.video
    z, e, cfg, _, ids, clips, source = _epoch_setup(pkg, tmp_path, True)
    S, B = cfg.spatial_size, e["batch_size"]
    total = fd.DeviceFrameStore(source, ids, spatial_size=S, device="cpu").total_bytes
    ds = fd.DeviceMultimodalDataset(cfg, source, device=DEV, capacity_bytes=total // 2, generator=torch.Generator().manual_seed(99))
    store = ds.appearance_dataset.store
    assert 0 < store.nbytes <= total // 2 and not store.resident(len(ids) - 1)
    lay = pkg.layout_data.DeviceStltDataset(cfg, device=DEV)
    col = video.DeviceVideoCollater(S, train=True, device=DEV)
    twin = torch.Generator().manual_seed(99)  # the clip parameters, drawn per clip in batch order
    torch.manual_seed(e["epoch_seed"])
    np.random.seed(e["epoch_seed"])
    loader = ds.loader(B, shuffle=True, real_counts=True)
    batches = [b for _ in range(e["epochs"]) for b in loader]
    assert len(batches) == e["epochs"] * len(loader) == len(z["epoch/order"]) // B
    assert np.random.random_sample() == z["epoch/probe"][0]
    for k, batch in enumerate(batches):
        rows = slice(k * B, (k + 1) * B)
        v = z["epoch/order"][rows]
        assert batch["video_id"] == [ids[i] for i in v]
        want = lay.collate(v, real_counts=True, sampled=(np.maximum(z["epoch/layout"][rows], 0), z["epoch/layout_count"][rows]))
        layout_keys = [k_ for k_ in want if k_ not in ("video_id", "labels")]
        assert list(batch) == list(want) + ["video_frames"]  # the layout batch, the appearance keys merged last
        for key in layout_keys:
            if isinstance(want[key], torch.Tensor):
                assert torch.equal(batch[key], want[key]), (k, key)
            else:
                assert batch[key] == want[key], (k, key)
        assert torch.equal(batch["labels"].cpu(), torch.from_numpy(lay.video_label[v]))
        params = [video.draw_clip_params(40, 52, S, True, twin) for _ in v]
        frames = [torch.from_numpy(clips[i][z["epoch/appearance"][rows][b]]) for b, i in enumerate(v)]
        assert torch.equal(batch["video_frames"], col.prep(frames, params)), k


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


def test_models_run_from_the_loaders(fd, pkg, tmp_path):
    """Resnet3D and CACNF (appearance_trunk=True) logits from store batches are those of the matching DeviceMultimodalCollater batch,
    bit for bit; one Trainer step and one inference pass per loader."""
    video, ld = pkg.video, pkg.layout_data
    z, e, cfg, p, ids, clips, source = _epoch_setup(pkg, tmp_path, False, S=112, T_app=8, frame_hw=(130, 171))
    ds = fd.DeviceMultimodalDataset(cfg, source, device=DEV)
    restated = LR.Restated(*LR.load_annotations("something", p), "something", cfg.layout_num_frames, False, 0.5, ld.CATEGORY2ID["something"],
                           ld.FRAME2TYPE["something"])
    idx = [3, 17, 0, 25]
    batch = ds.collate(idx)
    fi = ds.appearance_dataset.sample_indices(idx)
    samples = [{"layout": {k: torch.as_tensor(v_) for k, v_ in restated.item(i).items() if k != "video_id"},
                "appearance": {"frames": clips[i][fi[b]], "labels": torch.tensor(int(ds.appearance_dataset.video_label[i])), "video_id": ids[i]}}
               for b, i in enumerate(idx)]
    host = video.DeviceMultimodalCollater("something", 112, train=False, device=DEV)(samples)
    tensors = {k for k, t in host.items() if isinstance(t, torch.Tensor)}
    assert tensors == {k for k, t in batch.items() if isinstance(t, torch.Tensor)} and batch["video_id"] == host["video_id"]
    for k in tensors:
        assert torch.equal(batch[k], host[k]), k
    r3d = _r3d(pkg, pkg.Resnet3D, pkg.AppearanceModelConfig)
    cacnf = _r3d(pkg, pkg.CrossAttentionCentralNetFusion, pkg.MultimodalModelConfig, num_appearance_layers=2, num_fusion_layers=2, appearance_trunk=True)
    app_batch = ds.appearance_dataset.collate(idx)
    assert list(app_batch) == ["video_id", "video_frames", "labels"] and torch.equal(app_batch["video_frames"], host["video_frames"])
    with torch.no_grad():
        a, b = r3d(app_batch)["resnet3d"], r3d({"video_frames": host["video_frames"]})["resnet3d"]
        assert torch.isfinite(a).all() and torch.equal(a, b)
        got, want = cacnf(batch), cacnf(host)
        for k in ("stlt", "resnet3d", "caf", "ensemble"):
            assert torch.isfinite(got[k]).all() and torch.equal(got[k], want[k]), k
    # inference passes from both loaders, two batches of four clips each
    out = pkg.infer.run_inference(r3d, itertools.islice(ds.appearance_dataset.loader(4), 2), DEV, forward=lambda b_: r3d(b_)["resnet3d"])
    assert out["num_clips"] == 8
    out = pkg.infer.run_inference(cacnf, itertools.islice(ds.loader(4, real_counts=True), 2), DEV, forward=lambda b_: cacnf(b_)["caf"])
    assert out["num_clips"] == 8
    # one optimisation step from the training loader
    train_cfg = types.SimpleNamespace(**dict(vars(cfg), train=True))
    train_ds = fd.DeviceMultimodalDataset(train_cfg, source, device=DEV, generator=torch.Generator().manual_seed(1))
    torch.manual_seed(0)
    np.random.seed(0)
    first = next(iter(train_ds.loader(4, shuffle=True, drop_last=True)))
    trainable = _r3d(pkg, pkg.CrossAttentionCentralNetFusion, pkg.MultimodalModelConfig, num_appearance_layers=2, num_fusion_layers=2, appearance_trunk=True,
                     train_trunk=True)
    trainer = pkg.train.Trainer(trainable, "something", learning_rate=1e-4, warmup_steps=0, total_steps=4)
    step = trainer.step(first)
    assert np.isfinite(float(step["loss"])) and float(step["grad_norm"]) > 0


def test_captured_graph_replays_the_batch(fd):
    rng = np.random.default_rng(3)
    clips = _random_clips(rng, 32, [9, 4, 12, 6])
    store = fd.DeviceFrameStore(*_source(clips), spatial_size=32, device=DEV)
    v = [2, 0, 3, 1, 2]
    fi = np.asarray([[0, 2, 4, 6], [8, 8, 1, 0], [5, 3, 1, 0], [0, 1, 2, 3], [11, 9, 7, 5]])
    want = store.gather(v, fi)  # warm-up: the store and the pinned blocks exist before the capture
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        store.gather(v, fi)
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        got = store.gather(v, fi)
    got.zero_()
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(got, want)
    other = store.gather([1, 1], np.asarray([[0, 1, 2, 3], [3, 2, 1, 0]]))  # the ring keeps serving eager batches; the graph keeps its block
    got.zero_()
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(got, want) and other.shape == (2, 3, 4, 32, 32)
