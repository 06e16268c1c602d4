"""Device-side counterpart of the reference's layout dataset: ``StltDataset`` (src/modelling/datasets.py:31-137, with
``fix_box`` / ``get_test_layout_indices`` / ``sample_train_layout_indices`` from src/utils/data_utils.py:33-56,205-231) and
``StltCollater`` (datasets.py:239-288) in one object.

``DeviceStltDataset(config, device)`` reads the three annotation files once into flat host tables (per video: frame offsets,
size, label; per frame: kept-object offsets and whether ``frame_objects`` was empty; per kept object: category, score and the
raw box), uploads them once and runs ``fix_box`` + the division by ``(w, h, w, h)`` over every kept object in one kernel
(csrc/layout_data.hip).  ``collate(indices)`` then builds the reference's padded batch for those videos on the device with one
copy of a small pinned index block and one kernel launch: ``StltCollater(cfg)([StltDataset(cfg)[i] for i in indices])``, bit
for bit.  ``loader(...)`` iterates it the way ``DataLoader(StltDataset, batch_size, shuffle, collate_fn=StltCollater)`` does.

Frame indices are made on the host with the reference's expressions, vectorised over the batch.  In training every sample
with frames takes the first branch of sample_train_layout_indices, whose ``np.random.uniform(0, avg, size=T)`` is
``avg * random_sample(T)``: one ``np.random.random_sample`` call per batch, in sample order, gives the same stream, so after the
same ``np.random.seed`` the frames equal the reference's (its DataLoader with ``num_workers=0``).  A video without frames
takes the last branch (no draws) and has only the extract frame.
"""
from __future__ import annotations

import ctypes as C
import json
import re
from typing import Dict, List, Optional, Sequence

import numpy as np
import torch

from . import _lib as L

# the reference's vocabularies (src/modelling/configs.py:25-90)
_AG_OBJECTS = ("chair", "book", "medicine", "vacuum", "food", "groceries", "floor", "mirror", "closet/cabinet", "doorway",
               "paper/notebook", "picture", "phone/camera", "sofa/couch", "sandwich", "cup/glass/bottle", "towel", "box", "blanket",
               "television", "bag", "refrigerator", "table", "light", "broom", "shoe", "doorknob", "bed", "window", "shelf", "door",
               "pillow", "laptop", "dish", "clothes", "person")
CATEGORY2ID = {
    "something": {"pad": 0, "hand": 1, "object": 2, "cls": 3},
    "action_genome": {"pad": 0, "cls": 1, **{c: i + 2 for i, c in enumerate(_AG_OBJECTS)}},
}
FRAME2TYPE = {
    "something": {"pad": 0, "start": 1, "regular": 2, "empty": 3, "extract": 4},
    "action_genome": {"pad": 0, "regular": 1, "extract": 2, "empty": 3},
}
BOX_SATURATION = 1 << 30  # raw coordinates are stored as min(max(int(b), 0), 2^30): fix_box maps anything >= the frame size alike
MAX_VIDEO_SIDE = 1 << 24  # every clamped coordinate converts to float32 exactly
RING = 4  # pinned index blocks in flight


def layout_test_indices(T: int, n: np.ndarray):
    """get_test_layout_indices (data_utils.py:48-56) for every video of a batch: n (B,) frame counts -> (idx (B, T) int64, count (B,)).
    Row b holds int(tick / 2.0 + tick * x) for x < T when n > T (tick = n * 1.0 / T), else arange(n)."""
    n = np.asarray(n, dtype=np.int64)
    x = np.arange(T, dtype=np.int64)
    tick = (n * 1.0 / T)[:, None]
    spread = (tick / 2.0 + tick * x).astype(np.int64)  # float64 as the reference's Python floats; int() truncates (values >= 0)
    idx = np.where((n > T)[:, None], spread, np.broadcast_to(x, (len(n), T)))
    return idx, np.minimum(n, T)


def layout_train_indices(T: int, n: np.ndarray, uniforms: Optional[np.ndarray] = None):
    """sample_train_layout_indices (data_utils.py:33-45) for every video of a batch: -> (idx (B, T) int64, count (B,)).
    Videos with frames take the first branch, floor(i * avg + uniform(0, avg)) with avg = n * 1.0 / T; their T uniforms come, in
    sample order, from ONE np.random.random_sample call (or `uniforms`, (#videos with frames, T)).  Videos without frames draw nothing
    and sample no frame.  IndexError when a floor reaches n (the reference's frames[index] would raise)."""
    n = np.asarray(n, dtype=np.int64)
    idx = np.zeros((len(n), T), np.int64)
    live = n > 0
    k = int(live.sum())
    if k:
        u = np.random.random_sample(k * T).reshape(k, T) if uniforms is None else np.asarray(uniforms, np.float64).reshape(k, T)
        avg = (n[live] * 1.0 / T)[:, None]
        offsets = np.floor(np.multiply(np.arange(T), avg) + avg * u)
        if (offsets >= n[live][:, None]).any():
            raise IndexError("list index out of range (a sampled layout frame index reached the video's frame count)")
        idx[live] = offsets.astype(np.int64)
    return idx, np.where(live, T, 0)


def _identity(batch):
    return batch


class _Loader:
    """Re-iterable over collated batches; batch indices come from a real DataLoader over range(len) so torch's RNG is consumed as the
    reference's DataLoader consumes it."""

    def __init__(self, ds: "DeviceStltDataset", batch_size: int, shuffle: bool, drop_last: bool, generator, real_counts: bool):
        self.ds = ds
        self.real_counts = real_counts
        self.index_loader = torch.utils.data.DataLoader(range(len(ds)), batch_size=batch_size, shuffle=shuffle, drop_last=drop_last,
                                                        generator=generator, collate_fn=_identity, num_workers=0)

    def __len__(self):
        return len(self.index_loader)

    def __iter__(self):
        for idx in self.index_loader:
            yield self.ds.collate(idx, real_counts=self.real_counts)


class DeviceStltDataset:
    def __init__(self, config, device="cuda"):
        self.config = config
        self.dataset_name = config.dataset_name
        if self.dataset_name not in CATEGORY2ID:
            raise AssertionError(f"{self.dataset_name} does not exist!")
        self.category2id = dict(CATEGORY2ID[self.dataset_name])
        self.frame2type = dict(FRAME2TYPE[self.dataset_name])
        self.device = torch.device(device)
        self.T = int(config.layout_num_frames)
        if self.T <= 0:
            raise ValueError(f"layout_num_frames must be positive, got {self.T}")
        self.train = bool(config.train)
        with open(config.dataset_path) as f:
            videos = json.load(f)
        with open(config.labels_path) as f:
            self.labels = json.load(f)
        with open(config.videoid2size_path) as f:
            videoid2size = json.load(f)
        self._parse(videos, videoid2size, float(config.score_threshold))
        config.max_num_objects = self.max_num_objects  # datasets.py:36-46
        self.N = self.max_num_objects + 1
        self._dev = None  # device tables (upload())
        self._ring = [None] * RING
        self._next = 0
        self._captured = []  # index blocks a captured graph reads at replay

    # ---- host tables ----
    def _parse(self, videos, videoid2size, threshold: float):
        c2i = self.category2id
        something = self.dataset_name == "something"
        V = len(videos)
        self.video_ids = [v["id"] for v in videos]
        vframes = np.zeros(V + 1, np.int64)
        sizes = np.zeros((V, 2), np.int32)
        label = np.zeros(V, np.int64)
        act_off = np.zeros(V + 1, np.int64)
        actions: List[int] = []
        fobj, fempty, fnz = [0], [], []
        cats: List[int] = []
        scores: List[float] = []
        boxes: List[int] = []
        obj_video: List[int] = []
        sat = BOX_SATURATION
        for vi, v in enumerate(videos):
            size = videoid2size[v["id"]]  # KeyError like the reference
            if len(size) != 2 or not all(isinstance(s, int) and not isinstance(s, bool) for s in size):
                raise ValueError(f"video {v['id']}: size {size!r} is not two integers")
            w, h = size
            if not (1 <= w <= MAX_VIDEO_SIDE and 1 <= h <= MAX_VIDEO_SIDE):
                raise ValueError(f"video {v['id']}: size {size!r} outside [1, 2^24]")
            sizes[vi] = (w, h)
            for fr in v["frames"]:
                objs = fr["frame_objects"]
                fempty.append(len(objs) == 0)
                nz = 0
                for o in objs:
                    if o["score"] < threshold:  # datasets.py:72 (Python floats: float64)
                        continue
                    cid = c2i[o["category"]]  # KeyError like datasets.py:84
                    cats.append(cid)
                    nz += cid != 0
                    scores.append(o["score"])
                    boxes.extend(min(max(int(o[k]), 0), sat) for k in ("x1", "y1", "x2", "y2"))
                    obj_video.append(vi)
                fobj.append(len(cats))
                fnz.append(nz)
            vframes[vi + 1] = len(fempty)
            if something:
                label[vi] = int(self.labels[re.sub(r"[\[\]]", "", v["template"])])  # datasets.py:129-132
            else:
                acts = [int(a[1:]) for a in v["actions"]]  # datasets.py:133-136
                C_ = len(self.labels)
                bad = [a for a in acts if not 0 <= a < C_]
                if bad:
                    raise IndexError(f"video {v['id']}: action index {bad[0]} out of range for {C_} classes")
                actions.extend(acts)
                act_off[vi + 1] = len(actions)
        self.video_frames = vframes
        self.video_size = sizes
        self.frame_objects = np.asarray(fobj, np.int64)
        self.frame_empty = np.asarray(fempty, np.uint8)
        self.frame_tokens = np.asarray(fnz, np.int64)  # kept objects with a non-zero category (what the box mask leaves unmasked)
        self.object_category = np.asarray(cats, np.int32)
        self.object_score = np.asarray(scores, np.float64).astype(np.float32)
        self.object_box_raw = np.asarray(boxes, np.int32).reshape(-1, 4)
        self.object_size = sizes[np.asarray(obj_video, np.int64)] if obj_video else np.zeros((0, 2), np.int32)
        self.n_classes = 0 if something else len(self.labels)
        self.video_label = label
        self.video_actions = act_off
        self.actions = np.asarray(actions, np.int32)
        counts = np.diff(self.frame_objects)
        self.max_num_objects = int(counts.max()) if len(counts) else -1
        if self.max_num_objects < 0:
            raise ValueError("the annotation set has no frames: the reference's max_num_objects would stay -1")

    def __len__(self):
        return len(self.video_ids)

    def num_frames(self, indices) -> np.ndarray:
        v = np.asarray(indices, np.int64)
        return self.video_frames[v + 1] - self.video_frames[v]

    def sample_indices(self, indices, uniforms: Optional[np.ndarray] = None):
        """-> (frame indices (B, T) int64, sampled counts (B,) int64) for the videos `indices`, as __getitem__ picks them (training
        draws from numpy's global RNG, see the module docstring)."""
        n = self.num_frames(indices)
        if self.train:
            return layout_train_indices(self.T, n, uniforms)
        return layout_test_indices(self.T, n)

    def host_labels(self, indices) -> np.ndarray:
        v = np.asarray(indices, np.int64)
        if not self.n_classes:
            return self.video_label[v].copy()
        out = np.zeros((len(v), self.n_classes), np.float32)
        for b, vi in enumerate(v):
            out[b, self.actions[self.video_actions[vi]:self.video_actions[vi + 1]]] = 1.0
        return out

    def host_real_counts(self, indices, frames: np.ndarray, counts: np.ndarray) -> Dict[str, int]:
        """collate.real_counts of the batch, from the host tables: every real frame (sampled + extract) has its CLS token, sampled
        frames add their kept objects of non-zero category."""
        v = np.asarray(indices, np.int64)
        gf = self.video_frames[v][:, None] + frames
        live = np.arange(frames.shape[1])[None, :] < counts[:, None]
        n_frames = int(counts.sum()) + len(v)
        return {"num_real_tokens": n_frames + int(self.frame_tokens[gf[live]].sum()), "num_real_frames": n_frames}

    # ---- device ----
    def upload(self):
        """Copies the tables to the device once and runs the box kernel (fix_box + normalisation) over every kept object."""
        if self._dev is not None:
            return self._dev
        lib = L.load()
        dev = self.device
        # every table holds at least one element (an empty tensor has no address); the launcher bounds reads by the true counts
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a if len(a) else np.zeros((1,) + a.shape[1:], a.dtype))).to(dev)  # noqa: E731
        K = len(self.object_category)
        d = {
            "video_frames": t(self.video_frames), "frame_objects": t(self.frame_objects), "frame_empty": t(self.frame_empty),
            "object_category": t(self.object_category), "object_score": t(self.object_score),
            "object_box": torch.empty(max(K, 1), 4, dtype=torch.float32, device=dev),
            "video_label": t(self.video_label), "video_actions": t(self.video_actions), "actions": t(self.actions),
        }
        raw, size = t(self.object_box_raw), t(self.object_size)  # freed after the launch: the allocator reuses them in stream order
        with torch.cuda.device(dev):
            L.check(lib.stlt_layout_boxes_fwd(raw.data_ptr(), size.data_ptr(), K, d["object_box"].data_ptr(),
                                              torch.cuda.current_stream().cuda_stream), "stlt_layout_boxes_fwd")
        tab = L.LayoutTable()
        tab.n_videos, tab.n_frames, tab.n_objects, tab.n_actions = len(self), len(self.frame_empty), K, len(self.actions)
        tab.n_classes, tab.cls_id = self.n_classes, self.category2id["cls"]
        tab.type_regular, tab.type_empty, tab.type_extract = self.frame2type["regular"], self.frame2type["empty"], self.frame2type["extract"]
        self._host_actions = self.actions if len(self.actions) else np.zeros(1, np.int32)
        tab.video_frames_host, tab.frame_objects_host = self.video_frames.ctypes.data, self.frame_objects.ctypes.data
        tab.video_actions_host, tab.actions_host = self.video_actions.ctypes.data, self._host_actions.ctypes.data
        for k, v in d.items():
            setattr(tab, k, v.data_ptr())
        self._dev = d
        self._table = tab
        return d

    def device_bytes(self) -> int:
        """Bytes of the resident device tables."""
        self.upload()
        return sum(v.numel() * v.element_size() for v in self._dev.values())

    def _slot(self, n_ints: int, capturing: bool):
        """A pinned index block and its device twin.  Eager calls take the ring's blocks in turn and wait for the event of the copy
        that last read the block (RING batches ago: in practice never a wait).  A call under graph capture takes an allocated block
        without waiting (torch.cuda.graph synchronises before it captures) and hands it to the graph, which reads it at every replay."""
        order = [(self._next + j) % RING for j in range(RING)]
        if capturing:
            i = next((j for j in order if self._ring[j] is not None and self._ring[j][0].numel() >= n_ints), None)
            if i is None:
                raise L.StltHipError("DeviceStltDataset.collate: run a batch of this size once before capturing one (pinned blocks are "
                                     "allocated outside the capture)")
        else:
            i = order[0]
        self._next = (i + 1) % RING
        s = self._ring[i]
        if capturing:
            self._captured.append(s)
            self._ring[i] = None
            return s
        if s is not None and s[2] is not None:
            s[2].synchronize()
        if s is None or s[0].numel() < n_ints:
            cap = max(n_ints, 1024)
            s = [torch.empty(cap, dtype=torch.int32, pin_memory=True), torch.empty(cap, dtype=torch.int32, device=self.device), None]
            self._ring[i] = s
        return s

    def collate(self, indices, real_counts: bool = False, sampled=None) -> Dict[str, object]:
        """StltCollater(cfg)([StltDataset(cfg)[i] for i in indices]) on the device (see the module docstring).  `sampled`: (frame
        indices (B, T), sampled counts (B,)) the caller drew already, in sample_indices' form (frame_data.DeviceMultimodalDataset draws
        them sample by sample, interleaved with the appearance indices); the default draws them here, one call per batch."""
        v = np.asarray([int(i) for i in indices], np.int64)
        B = len(v)
        if B == 0:
            raise L.StltHipError("DeviceStltDataset.collate: empty batch")
        if (v < 0).any() or (v >= len(self)).any():
            raise IndexError(f"video index out of range for {len(self)} videos")
        if sampled is None:
            frames, counts = self.sample_indices(v)
        else:
            frames, counts = np.asarray(sampled[0], np.int64), np.asarray(sampled[1], np.int64)
            if frames.shape != (B, self.T) or counts.shape != (B,):
                raise L.StltHipError(f"DeviceStltDataset.collate: sampled indices {frames.shape} / counts {counts.shape} for {B} clips of {self.T} frames")
        self.upload()
        lib = L.load()
        dev, T, N = self.device, self.T, self.N
        Lf = int(counts.max()) + 1
        n_ints = B * (2 + T)
        capturing = torch.cuda.is_current_stream_capturing()
        slot = self._slot(n_ints, capturing)
        host = slot[0].numpy()
        host[:B] = v
        host[B:2 * B] = counts
        host[2 * B:n_ints] = frames.reshape(-1)
        keep_scores = self.dataset_name == "action_genome"  # datasets.py:253-260
        out = {
            "categories": torch.empty(B, Lf, N, dtype=torch.int64, device=dev),
            "boxes": torch.empty(B, Lf, N, 4, dtype=torch.float32, device=dev),
            "frame_types": torch.empty(B, Lf, dtype=torch.int64, device=dev),
            "lengths": torch.empty(B, dtype=torch.int64, device=dev),
            "labels": (torch.empty(B, self.n_classes, dtype=torch.float32, device=dev) if self.n_classes
                       else torch.empty(B, dtype=torch.int64, device=dev)),
            "src_key_padding_mask_boxes": torch.empty(B, Lf, N, dtype=torch.bool, device=dev),
            "src_key_padding_mask_frames": torch.empty(B, Lf, dtype=torch.bool, device=dev),
        }
        if keep_scores:
            out["scores"] = torch.empty(B, Lf, N, dtype=torch.float32, device=dev)
        with torch.cuda.device(dev):
            stream = torch.cuda.current_stream()
            L.check(lib.stlt_layout_batch_fwd(C.byref(self._table), slot[0].data_ptr(), slot[1].data_ptr(), B, T, Lf, N,
                                              out["categories"].data_ptr(), out["boxes"].data_ptr(),
                                              out["scores"].data_ptr() if keep_scores else None, out["frame_types"].data_ptr(),
                                              out["src_key_padding_mask_boxes"].data_ptr(), out["src_key_padding_mask_frames"].data_ptr(),
                                              out["lengths"].data_ptr(), out["labels"].data_ptr(), stream.cuda_stream),
                    "stlt_layout_batch_fwd")
            if not capturing:
                slot[2] = torch.cuda.Event()
                slot[2].record(stream)
        out["video_id"] = [self.video_ids[i] for i in v]
        if real_counts:
            out.update(self.host_real_counts(v, frames, counts))
        return out

    def loader(self, batch_size: int, shuffle: bool = False, drop_last: bool = False, generator: Optional[torch.Generator] = None,
               real_counts: bool = False) -> _Loader:
        """DataLoader(StltDataset, batch_size, shuffle, drop_last, collate_fn=StltCollater, num_workers=0) on the device."""
        return _Loader(self, batch_size, shuffle, drop_last, generator, real_counts)
