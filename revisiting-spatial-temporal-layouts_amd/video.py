"""Device-side counterpart of the reference's appearance pipeline: the per-frame transforms of ``AppearanceDataset.__getitem__``
(src/modelling/datasets.py:163-208) and ``AppearanceCollater`` (datasets.py:291-300).

``DeviceVideoCollater(spatial_size, train, device)(samples)`` takes the list of per-clip dicts an appearance dataset produces when it
stops before its transforms — ``frames`` (T, H, W, 3) uint8 (the decoded frames at the indices ``sample_appearance_indices`` chose),
``labels``, ``video_id`` — and returns ``{"video_frames": (B, 3, T, S, S) float32, "labels", "video_id"}`` on the device.  The values
are the reference's bit for bit: Resize(floor(1.15 S)) with Pillow's antialiased 8-bit bilinear resampling, in training
VideoColorJitter (src/utils/data_utils.py:110-137) and RandomCrop, in evaluation center_crop, then ToTensor + Normalize(0.5, 0.5) —
all of it in csrc/video.hip.  Only the random draws and the resample coefficient tables are made on the host.

The draws follow torchvision 0.11.2 in the reference's order, per clip in batch order: ``ColorJitter.get_params`` (``torch.randperm(4)``,
then four ``uniform_`` draws: brightness, contrast, saturation, hue) and ``RandomCrop.get_params`` (``torch.randint`` for top, then left).
They come from torch's global RNG unless a ``generator`` is given, so after the same ``torch.manual_seed`` the augmentations equal the
reference's when its DataLoader runs with ``num_workers=0`` (with workers each worker has its own torch seed; frame-index sampling uses
numpy's RNG and stays with the caller).  The Pillow arithmetic restated here is checked against Pillow 12.2; the reference pins
Pillow 8.4, and that the two agree for these calls is assumed, not checked.
"""
from __future__ import annotations

import ctypes as C
import functools
import math
from dataclasses import dataclass
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib as L
from .collate import DeviceCollater

PRECISION_BITS = 22  # Pillow's fixed-point weights for 8-bit images (libImaging/Resample.c)
BRIGHTNESS = CONTRAST = SATURATION = (0.75, 1.25)  # VideoColorJitter (data_utils.py:110-122)
HUE = (-0.1, 0.1)


@dataclass
class ClipParams:
    """Everything one clip's transforms depend on.  order / brightness / contrast / saturation / hue_factor matter in training only."""
    rh: int
    rw: int
    top: int
    left: int
    train: bool = False
    order: Tuple[int, int, int, int] = (0, 1, 2, 3)
    brightness: float = 1.0
    contrast: float = 1.0
    saturation: float = 1.0
    hue_factor: float = 0.0

    @property
    def hue_shift(self) -> int:
        return hue_shift(self.hue_factor)


def hue_shift(hue_factor: float) -> int:
    """F_pil.adjust_hue adds np.uint8(hue_factor * 255) to H; under numpy 1.21 on x86 that truncates toward zero and wraps mod 256."""
    return int(math.trunc(hue_factor * 255.0)) % 256


def resized_size(h: int, w: int, target: int) -> Tuple[int, int]:
    """torchvision 0.11.2 F_pil.resize with an int size -> (new_h, new_w).  A short side already equal to the target leaves the frame
    as it is (no resampling)."""
    short, long = (w, h) if w <= h else (h, w)
    if short == target:
        return h, w
    new_short, new_long = target, int(target * long / short)
    new_w, new_h = (new_short, new_long) if w <= h else (new_long, new_short)
    return new_h, new_w


def center_crop_offsets(rh: int, rw: int, S: int) -> Tuple[int, int]:
    """TF.center_crop's origin (Python's round: half to even)."""
    return int(round((rh - S) / 2.0)), int(round((rw - S) / 2.0))


def draw_clip_params(h: int, w: int, S: int, train: bool, generator: Optional[torch.Generator] = None) -> ClipParams:
    """One clip's parameters for (h, w) source frames, drawn as the reference draws them (see the module docstring)."""
    target = math.floor(S * 1.15)
    rh, rw = resized_size(h, w, target)  # both sides >= target >= S
    if not train:
        top, left = center_crop_offsets(rh, rw, S)
        return ClipParams(rh, rw, top, left)
    fn_idx = torch.randperm(4, generator=generator)
    b, c, s, hf = (float(torch.empty(1).uniform_(lo, hi, generator=generator)) for lo, hi in (BRIGHTNESS, CONTRAST, SATURATION, HUE))
    if rh == S and rw == S:
        top = left = 0
    else:
        top = int(torch.randint(0, rh - S + 1, size=(1,), generator=generator).item())
        left = int(torch.randint(0, rw - S + 1, size=(1,), generator=generator).item())
    return ClipParams(rh, rw, top, left, True, tuple(int(i) for i in fn_idx.tolist()), b, c, s, hf)


@functools.lru_cache(maxsize=256)
def resample_table(in_size: int, out_size: int) -> Tuple[int, np.ndarray]:
    """Pillow's precompute_coeffs + normalize_coeffs_8bpc (bilinear, whole axis), float64 in its operation order -> (ksize, int32 array of
    out_size (first, count) pairs followed by out_size x ksize weights with 22 fraction bits): the layout csrc/video.hip reads."""
    scale = filterscale = float(in_size) / out_size
    if filterscale < 1.0:
        filterscale = 1.0
    support = 1.0 * filterscale
    ksize = int(math.ceil(support)) * 2 + 1
    bounds = np.zeros((out_size, 2), np.int32)
    coeffs = np.zeros((out_size, ksize), np.int32)
    ss = 1.0 / filterscale
    one = float(1 << PRECISION_BITS)
    for xx in range(out_size):
        center = 0.0 + (xx + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        n = min(int(center + support + 0.5), in_size) - xmin
        ws = []
        ww = 0.0
        for x in range(n):
            t = abs((x + xmin - center + 0.5) * ss)
            wt = 1.0 - t if t < 1.0 else 0.0
            ws.append(wt)
            ww += wt
        for x in range(n):
            wt = ws[x] / ww if ww != 0.0 else ws[x]
            coeffs[xx, x] = int(-0.5 + wt * one) if wt < 0 else int(0.5 + wt * one)
        bounds[xx] = (xmin, n)
    table = np.concatenate([bounds.ravel(), coeffs.ravel()]).astype(np.int32)
    table.flags.writeable = False
    return ksize, table


@functools.lru_cache(maxsize=1)
def normalize_table() -> torch.Tensor:
    """ToTensor + Normalize(0.5, 0.5) of every uint8 value, in the reference's op order (float32: div 255, sub 0.5, div 0.5)."""
    x = torch.arange(256, dtype=torch.uint8).to(torch.float32).div(255)
    return x.sub_(torch.tensor([0.5])).div_(torch.tensor([0.5])).contiguous()


def _frames_u8(x) -> torch.Tensor:
    t = x if isinstance(x, torch.Tensor) else torch.as_tensor(np.asarray(x))
    if t.dtype != torch.uint8 or t.dim() != 4 or t.shape[-1] != 3:
        raise L.StltHipError(f"frames must be uint8 (T, H, W, 3), got {tuple(t.shape)} {t.dtype}")
    return t.cpu().contiguous()


class DeviceVideoCollater:
    def __init__(self, spatial_size: int = 112, train: bool = False, device="cuda", generator: Optional[torch.Generator] = None):
        self.S = int(spatial_size)
        self.train = bool(train)
        self.device = torch.device(device)
        self.generator = generator
        self._inflight = None  # pinned descriptor/table memory of the last call and the event after which it may be reused

    def params(self, samples: Sequence[Dict[str, object]]) -> List[ClipParams]:
        """Draws the batch's parameters (consumes the RNG exactly as the reference's __getitem__ calls do, in batch order)."""
        out = []
        for s in samples:
            shape = np.shape(s["frames"]) if not isinstance(s["frames"], torch.Tensor) else tuple(s["frames"].shape)
            out.append(draw_clip_params(int(shape[1]), int(shape[2]), self.S, self.train, self.generator))
        return out

    def __call__(self, samples: List[Dict[str, object]], params: Optional[Sequence[ClipParams]] = None) -> Dict[str, object]:
        if not samples:
            raise L.StltHipError("DeviceVideoCollater: empty batch")
        frames = [_frames_u8(s["frames"]) for s in samples]
        if params is None:
            params = self.params(samples)
        out = {"video_frames": self.prep(frames, params)}
        out["labels"] = torch.stack([torch.as_tensor(s["labels"]) for s in samples]).to(self.device)
        out["video_id"] = [s.get("video_id") for s in samples]
        return out

    def prep(self, frames: Sequence[torch.Tensor], params: Sequence[ClipParams]) -> torch.Tensor:
        """(T, H, W, 3) uint8 host clips + their parameters -> video_frames (B, 3, T, S, S) float32 on the device."""
        lib = L.load()
        dev, S, B = self.device, self.S, len(frames)
        if len(params) != B:
            raise L.StltHipError("DeviceVideoCollater: one ClipParams per clip")
        T = int(frames[0].shape[0])
        if any(int(f.shape[0]) != T for f in frames):
            raise L.StltHipError(f"DeviceVideoCollater: every clip of a batch needs the same number of frames, got {[int(f.shape[0]) for f in frames]}")
        # tables: one per distinct (in, out) axis pair of the batch
        tables, tab_off, n_table = [], {}, 0

        def table(n_in, n_out):
            nonlocal n_table
            if n_in == n_out:
                return -1, 0
            key = (n_in, n_out)
            if key not in tab_off:
                k, t = resample_table(n_in, n_out)
                tab_off[key] = (n_table, k)
                tables.append(t)
                n_table += t.size
            return tab_off[key]

        clips = (L.VideoClip * B)()
        off = 0
        for i, (f, p) in enumerate(zip(frames, params)):
            _, h, w, _ = f.shape
            d = clips[i]
            d.src_offset, d.h, d.w, d.rh, d.rw, d.top, d.left = off, h, w, p.rh, p.rw, p.top, p.left
            d.tab_x, d.ksize_x = table(int(w), int(p.rw))
            d.tab_y, d.ksize_y = table(int(h), int(p.rh))
            d.jitter = int(p.train)
            if p.train:
                d.order[:] = list(p.order)
                d.brightness, d.contrast, d.saturation, d.hue_shift = p.brightness, p.contrast, p.saturation, p.hue_shift
            off += f.numel()
        # frames: one pinned buffer, one copy
        packed = torch.empty(off, dtype=torch.uint8, pin_memory=True)
        pos = 0
        for f in frames:
            packed[pos:pos + f.numel()].copy_(f.view(-1))
            pos += f.numel()
        frames_d = packed.to(dev, non_blocking=True)
        # descriptors, tables and the normalisation table: pinned host memory the launcher checks, then copies
        n_clip_bytes = C.sizeof(clips)
        meta = torch.empty(n_clip_bytes + 4 * n_table + 4 * 256, dtype=torch.uint8, pin_memory=True)
        mv = meta.numpy()
        C.memmove(meta.data_ptr(), C.addressof(clips), n_clip_bytes)
        if n_table:
            mv[n_clip_bytes:n_clip_bytes + 4 * n_table] = np.concatenate(tables).view(np.uint8)
        mv[n_clip_bytes + 4 * n_table:] = normalize_table().numpy().view(np.uint8)
        base = meta.data_ptr()
        ws_bytes = lib.stlt_video_prep_workspace_bytes(B, T, n_table)
        if ws_bytes == 0:
            raise L.StltHipError(f"DeviceVideoCollater: unsupported batch (B={B}, T={T})")
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
        out = torch.empty(B, 3, T, S, S, dtype=torch.float32, device=dev)
        if self._inflight is not None:
            self._inflight[1].synchronize()
        with torch.cuda.device(dev):
            stream = torch.cuda.current_stream()
            L.check(lib.stlt_video_prep_fwd(frames_d.data_ptr(), off, C.cast(base, C.POINTER(L.VideoClip)), base + n_clip_bytes, n_table,
                                            base + n_clip_bytes + 4 * n_table, B, T, S, out.data_ptr(), ws.data_ptr(), ws_bytes,
                                            stream.cuda_stream), "stlt_video_prep_fwd")
            ev = torch.cuda.Event()
            ev.record(stream)
        self._inflight = (meta, ev)
        return out


class DeviceMultimodalCollater:
    """MultiModalCollater (datasets.py:303-318) on the device: DeviceCollater on the "layout" dicts, DeviceVideoCollater on the
    "appearance" dicts, merged into one batch (the appearance keys last, as in the reference).  Its output feeds CAF, CACNF or LCF with
    appearance_trunk=True."""

    def __init__(self, dataset_name: str = "something", spatial_size: int = 112, train: bool = False, device="cuda",
                 generator: Optional[torch.Generator] = None):
        self.layout = DeviceCollater(dataset_name, device)
        self.appearance = DeviceVideoCollater(spatial_size, train, device, generator)

    def __call__(self, samples: List[Dict[str, Dict[str, object]]], params: Optional[Sequence[ClipParams]] = None) -> Dict[str, object]:
        layout = self.layout([s["layout"] for s in samples])
        appearance = self.appearance([s["appearance"] for s in samples], params)
        return {**layout, **appearance}
