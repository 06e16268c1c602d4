"""Device-side counterpart of the reference's appearance and multimodal datasets: ``AppearanceDataset`` + ``AppearanceCollater``
(src/modelling/datasets.py:139-208, 291-300) and ``MultimodalDataset`` + ``MultiModalCollater`` (datasets.py:211-229, 303-319), with
``sample_appearance_indices`` (src/utils/data_utils.py:59-90).

The reference resizes each frame on its own, before any random transform (datasets.py:172-177), and Pillow's result is an 8-bit
image: the resized frame is a constant of the dataset.  ``DeviceFrameStore`` decodes every frame once on the host, resizes it on the
device (csrc/frame_store.hip: Pillow's two 8-bit passes from the tables ``video.resample_table`` builds) and keeps the result as one
packed uint8 device buffer.  A batch is then one launch over byte offsets into that buffer: crop + normalisation table in evaluation,
``VideoColorJitter`` + crop + table in training, the values ``video.DeviceVideoCollater`` gives for the same frames and parameters,
bit for bit, without the per-batch packing, upload and resampling.  Videos that do not fit under ``capacity_bytes`` are not resident:
the sampled frames of their clips are decoded and resized per batch into a spill area the same launch reads.

``source[video_id]`` maps ``str(frame_index)`` to one frame, either encoded bytes Pillow can open (what the reference's HDF5 file
holds, datasets.py:174) or a decoded (H, W, 3) uint8 array; ``len(source[video_id])`` is the video's frame count (datasets.py:167).
An open ``h5py.File`` has this shape.

Random draws follow the reference's ``__getitem__`` order.  numpy's global RNG: per sample the layout indices, then the appearance
indices.  torch's RNG (or ``generator``): per clip in batch order ``video.draw_clip_params``.  The two are separate streams, so after the
same ``np.random.seed`` / ``torch.manual_seed`` the batches equal the reference's DataLoader with ``num_workers=0``.
"""
from __future__ import annotations

import ctypes as C
import io
import json
import math
import re
import time
from typing import Dict, List, Optional, Sequence

import numpy as np
import torch

from . import _lib as L
from . import layout_data as LD
from . import video as V

SAMPLE_RATE = 2  # sample_appearance_indices' default, the only value the reference uses
RING = 4  # pinned descriptor blocks in flight
CLIP_DTYPE = np.dtype([("rh", "<i4"), ("rw", "<i4"), ("top", "<i4"), ("left", "<i4"), ("jitter", "<i4"), ("order", "<i4", (4,)),
                       ("brightness", "<f4"), ("contrast", "<f4"), ("saturation", "<f4"), ("hue_shift", "<i4"), ("reserved", "<i4")])
assert CLIP_DTYPE.itemsize == C.sizeof(L.FramesClip)  # stlt_frames_clip


def appearance_indices(num_frames_wanted: int, num_video_frames: int, train: bool, sample_rate: int = SAMPLE_RATE) -> List[int]:
    """sample_appearance_indices (data_utils.py:59-90): the reference's calls on numpy's global RNG, in its order."""
    k, n = int(num_frames_wanted), int(num_video_frames)
    d = k * sample_rate
    if n > d:
        offset = np.random.randint(0, n - d) if train else (n - d) // 2
        frames = list(range(offset, offset + d, sample_rate))
    else:
        if train and not n - 2 < k:
            pos = np.sort(np.random.choice(list(range(n - 2)), k, replace=False))
        else:  # fewer frames than wanted, or evaluation
            pos = np.linspace(0, n - 2, k)
        frames = [round(p) for p in pos]
    return [int(max(x, 0)) for x in frames]  # n = 1 gives negative positions


def decode_frame(frame) -> np.ndarray:
    """One frame of a source -> (H, W, 3) uint8.  Encoded bytes go through Pillow as in datasets.py:174; the reference converts no
    modes, so anything but 8-bit RGB is an error."""
    if getattr(frame, "ndim", 0) >= 2:
        a = np.asarray(frame)
        if a.dtype != np.uint8 or a.ndim != 3 or a.shape[2] != 3:
            raise ValueError(f"a decoded frame must be (H, W, 3) uint8, got {a.shape} {a.dtype}")
        return a
    from PIL import Image
    raw = frame if isinstance(frame, (bytes, bytearray, memoryview)) else np.array(frame)
    img = Image.open(io.BytesIO(raw))
    if img.mode != "RGB":
        raise ValueError(f"frame mode {img.mode!r}: only 8-bit RGB frames are supported (the reference converts no modes)")
    return np.asarray(img)


def _frame_size(frame):
    if getattr(frame, "ndim", 0) >= 2:
        return decode_frame(frame).shape[:2]
    from PIL import Image
    raw = frame if isinstance(frame, (bytes, bytearray, memoryview)) else np.array(frame)
    w, h = Image.open(io.BytesIO(raw)).size  # the header alone
    return h, w


def _pad16(n: int) -> int:
    return max(16, (int(n) + 15) & ~15)


class DeviceFrameStore:
    """Resized frames of `video_ids` as one packed uint8 device buffer plus host tables (per video: first-frame byte offset, frame
    count, source and resized size).  `capacity_bytes` bounds the buffer: videos are made resident in the order given until the next
    one does not fit; the default keeps everything resident."""

    def __init__(self, source, video_ids: Sequence[str], spatial_size: int = 112, device="cuda", capacity_bytes: Optional[int] = None):
        self.source = source
        self.video_ids = list(video_ids)
        self.S = int(spatial_size)
        if self.S <= 0:
            raise ValueError(f"spatial_size must be positive, got {self.S}")
        self.target = math.floor(self.S * 1.15)
        self.device = torch.device(device)
        n_videos = len(self.video_ids)
        self.frame_count = np.zeros(n_videos, np.int64)
        self.source_size = np.zeros((n_videos, 2), np.int64)  # (h, w) of frame 0: the reference takes the crop window from it
        self.size = np.zeros((n_videos, 2), np.int64)  # (rh, rw)
        for i, vid in enumerate(self.video_ids):
            frames = source[vid]  # KeyError like the reference
            self.frame_count[i] = len(frames)
            if self.frame_count[i] <= 0:
                raise ValueError(f"video {vid}: no frames")
            self.source_size[i] = _frame_size(frames["0"])
            self.size[i] = V.resized_size(int(self.source_size[i, 0]), int(self.source_size[i, 1]), self.target)
        self.frame_bytes = self.size[:, 0] * self.size[:, 1] * 3
        self.video_bytes = self.frame_count * self.frame_bytes
        self.total_bytes = int(self.video_bytes.sum())
        if capacity_bytes is not None and capacity_bytes < 0:
            raise ValueError("capacity_bytes must not be negative")
        self.capacity_bytes = None if capacity_bytes is None else int(capacity_bytes)
        cap = self.total_bytes if capacity_bytes is None else int(capacity_bytes)
        self.video_offset = np.full(n_videos, -1, np.int64)  # byte offset of the video's first frame; -1: not resident
        used = 0
        for i in range(n_videos):
            if used + self.video_bytes[i] > cap:
                break
            self.video_offset[i] = used
            used += int(self.video_bytes[i])
        self.nbytes = used
        centre = [V.center_crop_offsets(int(rh), int(rw), self.S) for rh, rw in self.size]
        self.center = np.asarray(centre, np.int64).reshape(n_videos, 2)
        self.stats = {"frames": 0, "decode_s": 0.0}  # host decoding, ingest and spills together
        self._buf = None
        self._lut = None
        self._ring = [None] * RING
        self._next = 0
        self._captured = []  # descriptor blocks a captured graph reads at replay

    def __len__(self):
        return len(self.video_ids)

    def resident(self, video_index: int) -> bool:
        return bool(self.video_offset[int(video_index)] >= 0)

    # ---- ingest ----
    def _decode(self, video_index: int, frame_indices) -> torch.Tensor:
        """Decoded frames of one video as a pinned (n, h, w, 3) uint8 tensor; every frame must have the size of frame 0."""
        vid = self.video_ids[video_index]
        h, w = (int(x) for x in self.source_size[video_index])
        t0 = time.perf_counter()
        frames = self.source[vid]
        pin = self.device.type == "cuda"
        out = torch.empty(len(frame_indices), h, w, 3, dtype=torch.uint8, pin_memory=pin)
        host = out.numpy()
        for j, fi in enumerate(frame_indices):
            a = decode_frame(frames[str(int(fi))])
            if a.shape != (h, w, 3):
                raise ValueError(f"video {vid}: frame {int(fi)} is {a.shape[0]} x {a.shape[1]}, frame 0 is {h} x {w} (all frames of a video "
                                 "must share one size: the crop window comes from frame 0)")
            host[j] = a
        self.stats["frames"] += len(frame_indices)
        self.stats["decode_s"] += time.perf_counter() - t0
        return out

    def _resize_into(self, buf: torch.Tensor, offset: int, video_index: int, frames: torch.Tensor):
        lib = L.load()
        n, h, w, _ = frames.shape
        rh, rw = (int(x) for x in self.size[video_index])
        src = frames.to(self.device, non_blocking=True)
        kx, tx = V.resample_table(w, rw) if w != rw else (0, None)
        ky, ty = V.resample_table(h, rh) if h != rh else (0, None)
        ws_bytes = lib.stlt_frames_resize_workspace_bytes(n, h, w, rh, rw, kx, ky)
        if ws_bytes == 0:
            raise L.StltHipError(f"DeviceFrameStore: unsupported frames ({n} x {h} x {w} -> {rh} x {rw})")
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=self.device)
        with torch.cuda.device(self.device):
            L.check(lib.stlt_frames_resize_fwd(src.data_ptr(), n, h, w, rh, rw, tx.ctypes.data if tx is not None else None, kx,
                                               ty.ctypes.data if ty is not None else None, ky, buf.data_ptr(), buf.numel(), int(offset),
                                               ws.data_ptr(), ws_bytes, torch.cuda.current_stream().cuda_stream), "stlt_frames_resize_fwd")

    def ingest(self):
        """Decodes and resizes every resident video once (one upload and one resize per video)."""
        if self._buf is not None:
            return self._buf
        if self.device.type != "cuda":
            raise L.StltHipError("DeviceFrameStore: frames live on a GPU; device='cpu' gives the host tables only")
        try:
            buf = torch.empty(_pad16(self.nbytes), dtype=torch.uint8, device=self.device)  # padded: rows are read as whole dwords
        except torch.OutOfMemoryError as e:
            raise MemoryError(f"DeviceFrameStore: {self.nbytes} bytes of resized frames do not fit on {self.device}; pass capacity_bytes "
                              "to keep only the first videos resident") from e
        for i in np.flatnonzero(self.video_offset >= 0):
            self._resize_into(buf, int(self.video_offset[i]), int(i), self._decode(int(i), range(int(self.frame_count[i]))))
        self._lut = V.normalize_table().to(self.device)
        self._buf = buf
        return buf

    def frames(self, video_index: int) -> torch.Tensor:
        """The stored (n, rh, rw, 3) uint8 frames of a resident video (a view of the buffer)."""
        buf = self.ingest()
        i = int(video_index)
        if not self.resident(i):
            raise KeyError(f"video {self.video_ids[i]} is not resident")
        rh, rw = (int(x) for x in self.size[i])
        return buf[int(self.video_offset[i]):int(self.video_offset[i] + self.video_bytes[i])].view(int(self.frame_count[i]), rh, rw, 3)

    # ---- batches ----
    def clip_params(self, video_indices, train: bool, generator: Optional[torch.Generator] = None) -> List[V.ClipParams]:
        """One clip's parameters per video, drawn as the reference draws them, in batch order (video.draw_clip_params)."""
        return [V.draw_clip_params(int(self.source_size[i, 0]), int(self.source_size[i, 1]), self.S, train, generator)
                for i in np.asarray(video_indices, np.int64)]

    def _slot(self, nbytes: int, capturing: bool):
        """A pinned descriptor block and its device twin, as DeviceStltDataset._slot: eager calls take the ring's blocks in turn and
        wait for the event of the copy that last read the block; a call under graph capture takes an allocated block without waiting
        and hands it to the graph, which reads it at every replay."""
        order = [(self._next + j) % RING for j in range(RING)]
        if capturing:
            i = next((j for j in order if self._ring[j] is not None and self._ring[j][0].numel() >= nbytes), None)
            if i is None:
                raise L.StltHipError("DeviceFrameStore.gather: run a batch of this size once before capturing one (pinned blocks are "
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
        if s is None or s[0].numel() < nbytes:
            cap = max(nbytes, 4096)
            s = [torch.empty(cap, dtype=torch.uint8, pin_memory=True), torch.empty(cap, dtype=torch.uint8, device=self.device), None]
            self._ring[i] = s
        return s

    def gather(self, video_indices, frame_indices, params: Optional[Sequence[V.ClipParams]] = None) -> torch.Tensor:
        """video_frames (B, 3, T, S, S) float32 for clips of frames `frame_indices` (B, T) of videos `video_indices`.  `params` holds one
        ClipParams per clip (clip_params); None is evaluation: the centre crop."""
        v = np.asarray([int(i) for i in video_indices], np.int64)
        fi = np.asarray(frame_indices, np.int64)
        B = len(v)
        if B == 0 or fi.ndim != 2 or fi.shape[0] != B or fi.shape[1] == 0:
            raise L.StltHipError(f"DeviceFrameStore.gather: {B} clips need a (B, T) array of frame indices with T > 0, got {fi.shape}")
        if (v < 0).any() or (v >= len(self)).any():
            raise IndexError(f"video index out of range for {len(self)} videos")
        if (fi < 0).any() or (fi >= self.frame_count[v][:, None]).any():
            raise IndexError("frame index outside its video")
        if params is not None and len(params) != B:
            raise L.StltHipError("DeviceFrameStore.gather: one ClipParams per clip")
        T = fi.shape[1]
        lib = L.load()
        buf = self.ingest()
        dev, S = self.device, self.S
        capturing = torch.cuda.is_current_stream_capturing()
        fb = self.frame_bytes[v]
        offsets = self.video_offset[v][:, None] + fi * fb[:, None]
        spilled = np.flatnonzero(self.video_offset[v] < 0)
        spill = None
        if len(spilled):
            if capturing:
                raise L.StltHipError("DeviceFrameStore.gather: a clip of a video that is not resident cannot be captured (it is decoded per batch)")
            picks = [np.unique(fi[b], return_inverse=True) for b in spilled]
            starts = np.concatenate([[0], np.cumsum([len(u) * fb[b] for (u, _), b in zip(picks, spilled)])]).astype(np.int64)
            spill = torch.empty(_pad16(starts[-1]), dtype=torch.uint8, device=dev)  # at most B * T frame slots
            for (u, inv), b, start in zip(picks, spilled, starts[:-1]):
                self._resize_into(spill, int(start), int(v[b]), self._decode(int(v[b]), u))
                offsets[b] = buf.numel() + start + inv.reshape(-1) * fb[b]
        clips = np.zeros(B, CLIP_DTYPE)
        clips["rh"], clips["rw"] = self.size[v, 0], self.size[v, 1]
        if params is None:
            clips["top"], clips["left"] = self.center[v, 0], self.center[v, 1]
        else:
            for b, p in enumerate(params):
                if (p.rh, p.rw) != (int(self.size[v[b], 0]), int(self.size[v[b], 1])):
                    raise L.StltHipError(f"DeviceFrameStore.gather: clip {b}: parameters for {p.rh} x {p.rw} frames, the store holds "
                                         f"{int(self.size[v[b], 0])} x {int(self.size[v[b], 1])}")
                c = clips[b]
                c["top"], c["left"], c["jitter"] = p.top, p.left, int(p.train)
                if p.train:
                    c["order"] = p.order
                    c["brightness"], c["contrast"], c["saturation"], c["hue_shift"] = p.brightness, p.contrast, p.saturation, p.hue_shift
        jitter = bool(clips["jitter"].any())
        nbytes = lib.stlt_frames_batch_block_bytes(B, T)
        if nbytes == 0:
            raise L.StltHipError(f"DeviceFrameStore.gather: unsupported batch (B={B}, T={T})")
        slot = self._slot(nbytes, capturing)
        host = slot[0].numpy()
        host[:B * T * 8] = np.ascontiguousarray(offsets).view(np.uint8).reshape(-1)
        host[B * T * 8:nbytes] = clips.view(np.uint8)
        sums = torch.empty(B * T, dtype=torch.int64, device=dev) if jitter else None
        out = torch.empty(B, 3, T, S, S, dtype=torch.float32, device=dev)
        with torch.cuda.device(dev):
            stream = torch.cuda.current_stream()
            L.check(lib.stlt_frames_batch_fwd(buf.data_ptr(), buf.numel(), spill.data_ptr() if spill is not None else None,
                                              spill.numel() if spill is not None else 0, slot[0].data_ptr(), slot[1].data_ptr(),
                                              self._lut.data_ptr(), B, T, S, sums.data_ptr() if jitter else None, out.data_ptr(),
                                              stream.cuda_stream), "stlt_frames_batch_fwd")
            if not capturing:
                slot[2] = torch.cuda.Event()
                slot[2].record(stream)
        return out


def _template_label(labels: Dict[str, object], video: dict) -> int:
    return int(labels[re.sub(r"[\[\]]", "", video["template"])])  # datasets.py:200-202


class DeviceAppearanceDataset:
    """AppearanceDataset + AppearanceCollater on the device.  config: dataset_name ("something": the reference's label expression reads
    the video's template), dataset_path, labels_path, appearance_num_frames, spatial_size, train."""

    def __init__(self, config, source, device="cuda", capacity_bytes: Optional[int] = None, generator: Optional[torch.Generator] = None,
                 layout: Optional[LD.DeviceStltDataset] = None):
        self.config = config
        if config.dataset_name != "something":
            raise ValueError(f"dataset {config.dataset_name!r}: the reference's AppearanceDataset labels a video by its template "
                             "(datasets.py:200-202), which only 'something' annotations carry")
        if layout is None:
            with open(config.dataset_path) as f:
                videos = json.load(f)
            with open(config.labels_path) as f:
                self.labels = json.load(f)
            self.video_ids = [v["id"] for v in videos]
            self.video_label = np.asarray([_template_label(self.labels, v) for v in videos], np.int64).reshape(len(videos))
        else:  # MultimodalDataset hands the layout dataset's annotation list on (datasets.py:213-216): same videos, same expression
            self.labels, self.video_ids, self.video_label = layout.labels, layout.video_ids, layout.video_label
        self.device = torch.device(device)
        self.T = int(config.appearance_num_frames)
        if self.T <= 0:
            raise ValueError(f"appearance_num_frames must be positive, got {self.T}")
        self.train = bool(config.train)
        self.generator = generator
        self.store = DeviceFrameStore(source, self.video_ids, int(config.spatial_size), device, capacity_bytes)
        self._eval_indices = {}

    def __len__(self):
        return len(self.video_ids)

    def _videos(self, indices) -> np.ndarray:
        v = np.asarray([int(i) for i in indices], np.int64)
        if len(v) == 0:
            raise L.StltHipError(f"{type(self).__name__}.collate: empty batch")
        if (v < 0).any() or (v >= len(self)).any():
            raise IndexError(f"video index out of range for {len(self)} videos")
        return v

    def sample_indices(self, indices) -> np.ndarray:
        """(B, T) frame indices as __getitem__ picks them, sample by sample (training draws from numpy's global RNG)."""
        counts = self.store.frame_count[np.asarray(indices, np.int64)].tolist()
        if self.train:
            rows = [appearance_indices(self.T, n, True) for n in counts]
        else:  # evaluation draws nothing: one list per frame count
            for n in set(counts) - set(self._eval_indices):
                self._eval_indices[n] = appearance_indices(self.T, n, False)
            rows = [self._eval_indices[n] for n in counts]
        return np.asarray(rows, np.int64).reshape(len(counts), self.T)

    def collate(self, indices, real_counts: bool = False, frame_indices=None) -> Dict[str, object]:
        """AppearanceCollater(cfg)([AppearanceDataset(cfg)[i] for i in indices]) on the device.  `frame_indices` (B, T): indices the
        caller drew already (the multimodal dataset draws them interleaved with the layout ones)."""
        v = self._videos(indices)
        fi = self.sample_indices(v) if frame_indices is None else frame_indices
        params = self.store.clip_params(v, True, self.generator) if self.train else None
        frames = self.store.gather(v, fi, params)
        labels = torch.from_numpy(self.video_label[v]).to(self.device, non_blocking=True)
        return {"video_id": [self.video_ids[i] for i in v], "video_frames": frames, "labels": labels}

    def loader(self, batch_size: int, shuffle: bool = False, drop_last: bool = False, generator: Optional[torch.Generator] = None):
        """DataLoader(AppearanceDataset, batch_size, shuffle, drop_last, collate_fn=AppearanceCollater, num_workers=0) on the device."""
        return LD._Loader(self, batch_size, shuffle, drop_last, generator, False)


class DeviceMultimodalDataset:
    """MultimodalDataset + MultiModalCollater on the device: a DeviceStltDataset and a DeviceAppearanceDataset over one annotation
    list.  A batch is the layout batch with the appearance keys merged last, so `labels` and `video_id` are the appearance ones."""

    def __init__(self, config, source, device="cuda", capacity_bytes: Optional[int] = None, generator: Optional[torch.Generator] = None):
        self.config = config
        self.layout_dataset = LD.DeviceStltDataset(config, device)
        self.appearance_dataset = DeviceAppearanceDataset(config, source, device, capacity_bytes, generator, layout=self.layout_dataset)
        self.labels = self.layout_dataset.labels  # datasets.py:217-219
        self.device = torch.device(device)

    def __len__(self):
        return len(self.layout_dataset)

    def sample_indices(self, indices):
        """-> ((layout frame indices (B, T), counts (B,)), appearance frame indices (B, Ta)), drawn from numpy's global RNG sample by
        sample in the order of MultimodalDataset.__getitem__ (datasets.py:224-229): the layout indices, then the appearance ones."""
        lay, app = self.layout_dataset, self.appearance_dataset
        v = np.asarray(indices, np.int64)
        n = lay.num_frames(v)
        uniforms, frames = [], []
        for b, i in enumerate(v):
            if lay.train and n[b] > 0:  # sample_train_layout_indices' one draw (layout_data.layout_train_indices)
                uniforms.append(np.random.random_sample(lay.T))
            frames.append(appearance_indices(app.T, int(app.store.frame_count[i]), app.train))
        if lay.train:
            sampled = LD.layout_train_indices(lay.T, n, np.stack(uniforms) if uniforms else None)
        else:
            sampled = LD.layout_test_indices(lay.T, n)
        return sampled, np.asarray(frames, np.int64).reshape(len(v), app.T)

    def collate(self, indices, real_counts: bool = False) -> Dict[str, object]:
        """MultiModalCollater(cfg)([MultimodalDataset(cfg)[i] for i in indices]) on the device."""
        v = self.appearance_dataset._videos(indices)
        sampled, frames = self.sample_indices(v)
        layout = self.layout_dataset.collate(v, real_counts=real_counts, sampled=sampled)
        appearance = self.appearance_dataset.collate(v, frame_indices=frames)
        return {**layout, **appearance}

    def loader(self, batch_size: int, shuffle: bool = False, drop_last: bool = False, generator: Optional[torch.Generator] = None,
               real_counts: bool = False):
        """DataLoader(MultimodalDataset, batch_size, shuffle, drop_last, collate_fn=MultiModalCollater, num_workers=0) on the device."""
        return LD._Loader(self, batch_size, shuffle, drop_last, generator, real_counts)
