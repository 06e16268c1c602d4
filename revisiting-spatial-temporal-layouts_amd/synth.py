"""Seeded synthetic layouts and deterministic closed-form weights.

Everything the GPU box needs to rebuild the exact inputs and weights the golden
fixtures under ``tests/golden/`` were captured with: no ``torch.manual_seed``
module init (that depends on torch version / constructor order), only
splitmix64 over (name-hash, element index), computed in numpy uint64.

Input contract follows the reference collater
(``src/modelling/datasets.py:52-125,239-288``):

* slot 0 of every frame (padded frames too) is the CLS object: category =
  ``cls`` id, box ``[0,0,1,1]``, score 1.0;
* real frames are a prefix, the last real frame is the "extract" frame with
  only the CLS object, padded frames have frame type 0;
* padded object slots: category 0, box zeros, score 0;
* ``src_key_padding_mask_boxes = categories == 0``,
  ``src_key_padding_mask_frames = frame_types == 0``, ``lengths`` = real
  frames (incl. extract).
"""
from __future__ import annotations

from typing import Dict, Optional

import numpy as np
import torch

_MASK64 = (1 << 64) - 1

# dataset vocabularies (src/modelling/configs.py:40-89)
DATASETS = {
    # name: (unique_categories, cls_id, first_object_id, regular, empty, extract)
    "something": dict(unique_categories=4, cls=3, obj_ids=(1, 2), regular=2, empty=3, extract=4),
    "action_genome": dict(unique_categories=38, cls=1, obj_ids=tuple(range(2, 38)), regular=1, empty=3, extract=2),
}


def fnv1a64(text: str) -> int:
    h = 0xCBF29CE484222325
    for b in text.encode("utf-8"):
        h ^= b
        h = (h * 0x100000001B3) & _MASK64
    return h


def splitmix64(x: np.ndarray) -> np.ndarray:
    """Vectorised splitmix64 finaliser over a uint64 array (wrapping arithmetic)."""
    with np.errstate(over="ignore"):
        z = x + np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return z ^ (z >> np.uint64(31))


def uniform01(key: int, n: int) -> np.ndarray:
    """n float64 in [0,1): element i = splitmix64(splitmix64(key) + i) >> 11 * 2^-53."""
    with np.errstate(over="ignore"):
        base = splitmix64(np.array([key & _MASK64], dtype=np.uint64))[0]
        idx = np.arange(n, dtype=np.uint64) + base
    z = splitmix64(idx)
    return (z >> np.uint64(11)).astype(np.float64) * (1.0 / 9007199254740992.0)


def _sym(key: int, shape, bound: float) -> torch.Tensor:
    n = int(np.prod(shape))
    u = uniform01(key, n)
    return torch.from_numpy(((2.0 * u - 1.0) * bound).astype(np.float32).reshape(shape))


def make_state_dict(shapes: Dict[str, tuple], seed: int = 1234, gain: float = 1.0) -> Dict[str, torch.Tensor]:
    """Deterministic fp32 weights for every key of a Stlt / StltBackbone state dict.

    ``shapes`` maps state-dict key -> shape (take it from ``module.state_dict()``).
    Bounds are torch-like (1/sqrt(fan_in) for matrices) so activations have
    realistic magnitudes and the softmaxes are not uniform; ``gain`` scales the
    attention in-projections to sharpen (gain>1) the attention distributions.
    """
    out: Dict[str, torch.Tensor] = {}
    for name, shape in shapes.items():
        shape = tuple(shape)
        key = fnv1a64(name) ^ (seed * 0x9E3779B97F4A7C15 & _MASK64)
        if name.endswith("position_ids"):
            out[name] = torch.arange(shape[-1], dtype=torch.int64).expand(shape).clone()
            continue
        leaf = name.rsplit(".", 1)[-1]
        parent = name.rsplit(".", 2)[-2] if name.count(".") >= 1 else ""
        if leaf in ("cls_token", "pos_embed"):
            out[name] = _sym(key, shape, 0.5)
            continue
        if parent in ("norm1", "norm2", "layer_norm", "ln"):
            if leaf == "weight":
                out[name] = 1.0 + _sym(key, shape, 0.1)
            else:
                out[name] = _sym(key, shape, 0.05)
        elif parent in ("category_embeddings", "position_embeddings", "frame_type_embedding"):
            out[name] = _sym(key, shape, 1.0)
        elif leaf == "in_proj_weight":
            out[name] = _sym(key, shape, gain * (6.0 / (shape[0] + shape[1])) ** 0.5 * 1.5)
        elif leaf in ("in_proj_bias",) or leaf == "bias":
            out[name] = _sym(key, shape, 0.05)
        elif leaf == "weight" and len(shape) in (2, 5):  # Linear, or the 1x1x1 Conv3d projector
            out[name] = _sym(key, shape, 1.0 / (shape[1] ** 0.5))
        else:
            raise KeyError(f"no init rule for {name} {shape}")
    return out


def make_batch(
    B: int,
    T: int,
    N: int,
    dataset: str = "something",
    seed: int = 0,
    dense: bool = False,
    with_scores: Optional[bool] = None,
    min_len: Optional[int] = None,
) -> Dict[str, torch.Tensor]:
    """Seeded collater-shaped batch (SURVEY.md §8d 'Synthetic inputs').

    ``T`` includes the extract frame, ``N`` includes the CLS slot.  Clip 0 always
    has ``length == T``.  ``dense=True`` makes every clip full length and every
    object slot real.
    """
    ds = DATASETS[dataset]
    if with_scores is None:
        with_scores = dataset == "action_genome"
    rng = np.random.Generator(np.random.PCG64(seed))
    cats = np.zeros((B, T, N), dtype=np.int64)
    boxes = np.zeros((B, T, N, 4), dtype=np.float32)
    scores = np.zeros((B, T, N), dtype=np.float32)
    ftypes = np.zeros((B, T), dtype=np.int64)
    lengths = np.zeros((B,), dtype=np.int64)
    lo = max(2, (T + 1) // 2) if min_len is None else max(2, min_len)
    lo = min(lo, T)
    obj_ids = np.asarray(ds["obj_ids"], dtype=np.int64)
    for b in range(B):
        ln = T if (dense or b == 0) else int(rng.integers(lo, T + 1))
        lengths[b] = ln
        # CLS slot in every frame, padded frames included (datasets.py:247-264)
        cats[b, :, 0] = ds["cls"]
        boxes[b, :, 0] = (0.0, 0.0, 1.0, 1.0)
        scores[b, :, 0] = 1.0
        for t in range(ln - 1):
            k = (N - 1) if dense else int(rng.integers(0, N))
            if k > 0:
                cats[b, t, 1 : k + 1] = obj_ids[rng.integers(0, len(obj_ids), size=k)]
                xy = np.sort(rng.random((k, 2, 2), dtype=np.float64), axis=1)  # [k,(lo,hi),(x,y)]
                boxes[b, t, 1 : k + 1, 0] = xy[:, 0, 0]
                boxes[b, t, 1 : k + 1, 1] = xy[:, 0, 1]
                boxes[b, t, 1 : k + 1, 2] = xy[:, 1, 0]
                boxes[b, t, 1 : k + 1, 3] = xy[:, 1, 1]
                scores[b, t, 1 : k + 1] = 0.5 + 0.5 * rng.random(k)
                ftypes[b, t] = ds["regular"]
            else:
                ftypes[b, t] = ds["empty"]
        ftypes[b, ln - 1] = ds["extract"]
    batch = {
        "categories": torch.from_numpy(cats),
        "boxes": torch.from_numpy(boxes),
        "frame_types": torch.from_numpy(ftypes),
        "lengths": torch.from_numpy(lengths),
        "src_key_padding_mask_boxes": torch.from_numpy(cats == 0),
        "src_key_padding_mask_frames": torch.from_numpy(ftypes == 0),
    }
    if with_scores:
        batch["scores"] = torch.from_numpy(scores)
    return batch


def make_video_samples(dataset: str, n_videos: int, N: int, seed: int):
    """Seeded per-video dicts shaped like ``StltDataset.__getitem__`` output (reference datasets.py:52-125): variable
    frame counts, fixed N object slots, last frame = extract.  Input of the collater (device or reference)."""
    rng = np.random.Generator(np.random.PCG64(seed))
    out = []
    for i in range(n_videos):
        n_frames = int(rng.integers(2, 9))
        b = make_batch(1, n_frames, N, dataset=dataset, seed=seed * 100 + i, with_scores=True, min_len=n_frames)
        label = torch.tensor(int(rng.integers(0, 174))) if dataset == "something" else torch.from_numpy(rng.random(157).astype(np.float32))
        out.append({"video_id": f"vid{i}", "categories": b["categories"][0], "boxes": b["boxes"][0], "scores": b["scores"][0],
                    "frame_types": b["frame_types"][0], "lengths": torch.tensor(n_frames), "labels": label})
    return out


# Named shape configurations (BASELINE.json "configs")
CONFIGS = {
    "micro": dict(T=5, N=3, hidden_size=32, num_attention_heads=4, num_spatial_layers=1, num_temporal_layers=1,
                  num_classes=7, dataset="something"),
    # the smallest model the checkpoint round-trip fixture trains on the GPU box (tools/make_ckpt_fixture.py: 58 KB of weights; head dim 8)
    "nano": dict(T=9, N=3, hidden_size=16, num_attention_heads=2, num_spatial_layers=1, num_temporal_layers=1,
                 num_classes=7, dataset="something"),
    "cfg1": dict(T=16, N=4, hidden_size=256, num_attention_heads=4, num_spatial_layers=4, num_temporal_layers=8,
                 num_classes=174, dataset="something"),
    "cfg2": dict(T=32, N=7, hidden_size=768, num_attention_heads=12, num_spatial_layers=4, num_temporal_layers=8,
                 num_classes=174, dataset="something"),
    "cfg2p": dict(T=33, N=8, hidden_size=768, num_attention_heads=12, num_spatial_layers=4, num_temporal_layers=8,
                  num_classes=174, dataset="something"),
    # the reference's defaults: layout_num_frames 16 (+ 1 extract frame), 4 object slots (+ CLS) — utils/parser.py:62-66, datasets.py:97-113
    "refdef": dict(T=17, N=5, hidden_size=768, num_attention_heads=12, num_spatial_layers=4, num_temporal_layers=8,
                   num_classes=174, dataset="something"),
    # a head dim other than 64 (96): the reference takes any hidden_size % num_attention_heads == 0 (configs.py:92-111)
    "heads": dict(T=9, N=6, hidden_size=384, num_attention_heads=4, num_spatial_layers=2, num_temporal_layers=3,
                  num_classes=174, dataset="something"),
    # a hidden size that is not a multiple of 32 (head dim 25)
    "odd": dict(T=7, N=4, hidden_size=100, num_attention_heads=4, num_spatial_layers=2, num_temporal_layers=2,
                num_classes=174, dataset="something"),
    "cfg4": dict(T=64, N=36, hidden_size=768, num_attention_heads=12, num_spatial_layers=4, num_temporal_layers=8,
                 num_classes=157, dataset="action_genome"),
}


def model_kwargs(name: str) -> dict:
    c = CONFIGS[name]
    return dict(
        num_classes=c["num_classes"],
        unique_categories=DATASETS[c["dataset"]]["unique_categories"],
        hidden_size=c["hidden_size"],
        num_attention_heads=c["num_attention_heads"],
        num_spatial_layers=c["num_spatial_layers"],
        num_temporal_layers=c["num_temporal_layers"],
        hidden_dropout_prob=0.0,
    )


# The small learnable task of the epoch-shell fixture (tools/gen_golden_fit.py -> tests/golden/fit_micro.npz): the label of a clip is a
# function of its number of real frames, which the temporal tower sees through the frame types and positions.
FIT_TASK = dict(config="micro", T=9, N=3, clips_per_batch=16, train_batches=2, val_batches=2, epochs=6, warmup_epochs=1, lr=6e-3,
                weight_decay=1e-3, clip_val=5.0, weight_seed=77)


def fit_batch(split: str, epoch: int, index: int) -> Dict[str, torch.Tensor]:
    """Batch `index` of `epoch` of the fit task's train split (a fresh shuffle per epoch, as a DataLoader(shuffle=True) gives) or of
    its fixed validation split, with labels."""
    t = FIT_TASK
    seed = 40000 + 100 * epoch + index if split == "train" else 90000 + index
    b = make_batch(t["clips_per_batch"], t["T"], t["N"], seed=seed)
    b["labels"] = (b["lengths"] - 2) % CONFIGS[t["config"]]["num_classes"]
    return b


def make_appearance_features(B: int, seed: int = 0, channels: int = 2048, grid=(2, 4, 4)) -> torch.Tensor:
    """Stand-in for the R3D-50 feature map of Resnet3D.forward_features (reference models.py:221-222):
    (B, 2048, *grid) — (2, 4, 4) by default, S = prod(grid) appearance tokens — non-negative like a post-ReLU map."""
    grid = tuple(int(g) for g in grid)
    u = uniform01(fnv1a64("appearance_features") ^ (seed * 0x9E3779B97F4A7C15 & _MASK64), B * channels * int(np.prod(grid)))
    return torch.from_numpy((u * 1.5).astype(np.float32).reshape(B, channels, *grid))


def make_r3d_state_dict(shapes: Dict[str, tuple], seed: int = 1234) -> Dict[str, torch.Tensor]:
    """Deterministic fp32 values for a model whose keys include an R3D-50 trunk (keys containing ``resnet.<digit>``): Conv3d weights
    He-uniform over their fan-in (activations stay O(1) through the ReLUs), BatchNorm with non-trivial gamma / beta / running mean,
    a positive running variance and num_batches_tracked = 0.  Every other key goes through ``make_state_dict``."""
    import re

    trunk = re.compile(r"(^|\.)resnet\.\d")
    out: Dict[str, torch.Tensor] = {}
    rest = {}
    for name, shape in shapes.items():
        shape = tuple(shape)
        if not trunk.search(name):
            rest[name] = shape
            continue
        key = fnv1a64("r3d:" + name) ^ (seed * 0x9E3779B97F4A7C15 & _MASK64)
        leaf = name.rsplit(".", 1)[-1]
        if leaf == "num_batches_tracked":
            out[name] = torch.zeros(shape, dtype=torch.int64)
        elif len(shape) == 5:
            fan_in = shape[1] * shape[2] * shape[3] * shape[4]
            out[name] = _sym(key, shape, (6.0 / fan_in) ** 0.5)
        elif leaf == "weight":
            out[name] = 0.75 + _sym(key, shape, 0.25)
        elif leaf == "bias":
            out[name] = _sym(key, shape, 0.1)
        elif leaf == "running_mean":
            out[name] = _sym(key, shape, 0.1)
        elif leaf == "running_var":
            out[name] = torch.from_numpy((0.6 + 0.8 * uniform01(key, int(np.prod(shape)))).astype(np.float32).reshape(shape))
        else:
            raise KeyError(f"no init rule for {name} {shape}")
    other = make_state_dict(rest, seed=seed)
    return {k: (out[k] if k in out else other[k]) for k in shapes}


def make_video(B: int, T: int = 32, H: int = 112, W: int = 112, seed: int = 0) -> torch.Tensor:
    """Stand-in for ``video_frames`` (reference datasets.py:198-206): (B, 3, T, H, W) fp32, normalised-pixel-like values in [-1.5, 1.5)."""
    u = uniform01(fnv1a64("video_frames") ^ (seed * 0x9E3779B97F4A7C15 & _MASK64), B * 3 * T * H * W)
    return torch.from_numpy(((2.0 * u - 1.0) * 1.5).astype(np.float32).reshape(B, 3, T, H, W))


def flops_per_clip(T: int, N: int, d: int, n_sp: int, n_tp: int, classes: int) -> float:
    """Algorithmic dense forward FLOPs per clip."""
    return (
        n_sp * (24.0 * T * N * d * d + 4.0 * T * N * N * d)
        + n_tp * (24.0 * T * d * d + 4.0 * T * T * d)
        + 2.0 * d * d
        + 2.0 * d * classes
    )


# Templates of the seeded "something" annotation sets: some carry the bracketed placeholders the reference strips before its label
# lookup (datasets.py:131), so a lookup that forgot the stripping fails on them.
LAYOUT_TEMPLATES = ("Putting [something] on [something]", "Pushing [something] from left to right", "Holding [something]",
                    "Dropping [something] into [something]", "Opening [something]", "Turning the camera left while filming [something]",
                    "Pretending to pick [something] up", "Moving [part] of [something]", "Showing that [something] is empty",
                    "Poking a stack of [something] without the stack collapsing")
LAYOUT_EDGE_FRAMES = (0, 1, 15, 16, 17, 300)  # videos of 0, 1, T - 1, T, T + 1 and many frames at the reference's T = 16


def make_layout_annotations(dataset: str, n_videos: int, seed: int, max_frames: int = 40, max_objects: int = 5):
    """Seeded annotation set in the reference's file formats (what StltDataset reads, src/modelling/datasets.py:31-47):
    -> (videos, labels, videoid2size), the contents of dataset_path, labels_path and videoid2size_path.

    videos: [{"id", "frames": [{"frame_objects": [{"category", "score", "x1", "y1", "x2", "y2"}, ...]}, ...], "template" (something) or
    "actions" (action_genome)}].  The first videos have 0, 1, 15, 16, 17 and 300 frames; the rest 0..max_frames.  Boxes include
    x1 > x2 / y1 > y2, negative, zero-width, out-of-frame, fractional and very large coordinates; frames include empty
    `frame_objects`, frames whose objects all score below 0.5, and scores exactly 0.5; one video is 1 x 2 pixels."""
    from .layout_data import CATEGORY2ID  # the reference's vocabularies (configs.py:25-90)

    rng = np.random.Generator(np.random.PCG64(seed))
    names = [c for c in CATEGORY2ID[dataset] if c not in ("pad", "cls")]
    n_classes = 174 if dataset == "something" else 157
    if dataset == "something":
        ids = rng.permutation(n_classes)[: len(LAYOUT_TEMPLATES)]
        labels = {t.replace("[", "").replace("]", ""): str(int(i)) for t, i in zip(LAYOUT_TEMPLATES, ids)}
    else:
        labels = {f"c{i:03d}": f"action {i}" for i in range(n_classes)}

    def coord(size):
        kind = rng.integers(0, 10)
        if kind == 0:
            return int(rng.integers(-40, 0))  # negative
        if kind == 1:
            return int(size + rng.integers(0, 60))  # at or past the frame's edge
        if kind == 2:
            return float(np.round(rng.uniform(-1.0, size + 1.0), 2))  # fractional (int() truncates toward zero)
        if kind == 3 and rng.integers(0, 4) == 0:
            return int(rng.integers(1 << 31, 1 << 40))  # beyond int32
        return int(rng.integers(0, size))

    def frame_objects(w, h):
        kind = rng.integers(0, 8)
        if kind == 0:
            return []
        k = int(rng.integers(1, max_objects + 1))
        out = []
        for _ in range(k):
            s = rng.random()
            if kind == 1:
                score = float(s * 0.5)  # every object below the threshold
            elif rng.integers(0, 6) == 0:
                score = 0.5  # exactly the threshold: kept (datasets.py:42, 72 compare with <)
            else:
                score = float(np.round(s, 4))
            x1, y1, x2, y2 = coord(w), coord(h), coord(w), coord(h)
            if rng.integers(0, 8) == 0:
                x2 = x1  # zero width
            if rng.integers(0, 8) == 0:
                y2 = y1
            out.append({"category": names[int(rng.integers(0, len(names)))], "score": score, "x1": x1, "y1": y1, "x2": x2, "y2": y2})
        return out

    videos, sizes = [], {}
    for i in range(n_videos):
        vid = f"{dataset[:2]}{seed}_{i:05d}"
        n = LAYOUT_EDGE_FRAMES[i] if i < len(LAYOUT_EDGE_FRAMES) else int(rng.integers(0, max_frames + 1))
        w, h = (1, 2) if i == len(LAYOUT_EDGE_FRAMES) else (int(rng.integers(64, 641)), int(rng.integers(64, 481)))
        sizes[vid] = [w, h]
        v = {"id": vid, "frames": [{"frame_objects": frame_objects(w, h)} for _ in range(n)]}
        if dataset == "something":
            v["template"] = LAYOUT_TEMPLATES[int(rng.integers(0, len(LAYOUT_TEMPLATES)))]
        else:
            v["actions"] = [f"c{int(a):03d}" for a in rng.choice(n_classes, size=int(rng.integers(0, 5)), replace=False)]
        videos.append(v)
    return videos, labels, sizes


def write_layout_annotations(directory: str, dataset: str, n_videos: int, seed: int, **kw):
    """make_layout_annotations written as the reference's three files under `directory` ->
    ({"annotations", "labels", "sizes"}: paths, sha256 hex digest of the three files' bytes)."""
    import hashlib
    import json
    import os

    h = hashlib.sha256()
    paths = {}
    for k, obj in zip(("annotations", "labels", "sizes"), make_layout_annotations(dataset, n_videos, seed, **kw)):
        paths[k] = os.path.join(directory, f"layout_{dataset}_{seed}_{k}.json")
        data = json.dumps(obj, separators=(",", ":")).encode()
        h.update(data)
        with open(paths[k], "wb") as f:
            f.write(data)
    return paths, h.hexdigest()
