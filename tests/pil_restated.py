"""numpy-only restatement of the Pillow / torchvision (0.11.2, PIL path) arithmetic behind the reference's clip transforms
(AppearanceDataset.__getitem__: Resize, VideoColorJitter, RandomCrop / center_crop, ToTensor + Normalize).  It computes exactly what
csrc/video.hip computes, operation for operation, and the not-gpu tests check it against the installed Pillow: it is the arbiter the
device collater is measured by, and it needs no Pillow itself (the GPU tests use it on machines without one).

Types follow Pillow's C: the resample coefficients are float64 rounded to int32 with 22 fraction bits; Image.blend runs in float32;
RGB -> HSV and HSV -> RGB mix float32 variables with float64 literals (libImaging/Convert.c, rgb2hsv_row / hsv2rgb)."""
from __future__ import annotations

import math

import numpy as np

PRECISION_BITS = 22  # 32 - 8 - 2 (libImaging/Resample.c)


# ----------------------------------------------------------------------------------------------------------------------- resample
def resample_table(in_size: int, out_size: int):
    """PIL's precompute_coeffs + normalize_coeffs_8bpc for the bilinear filter over the whole axis -> (ksize, bounds (out, 2) int32 of
    (xmin, count), coeffs (out, ksize) int32).  float64 throughout, in Pillow's operation order."""
    scale = filterscale = float(in_size) / out_size
    if filterscale < 1.0:
        filterscale = 1.0
    support = 1.0 * filterscale
    ksize = int(math.ceil(support)) * 2 + 1
    bounds = np.zeros((out_size, 2), np.int32)
    coeffs = np.zeros((out_size, ksize), np.int32)
    ss = 1.0 / filterscale
    for xx in range(out_size):
        center = 0.0 + (xx + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        xmax = min(int(center + support + 0.5), in_size) - xmin
        k = []
        ww = 0.0
        for x in range(xmax):
            t = abs((x + xmin - center + 0.5) * ss)
            w = 1.0 - t if t < 1.0 else 0.0
            k.append(w)
            ww += w
        for x in range(xmax):
            w = k[x] / ww if ww != 0.0 else k[x]
            coeffs[xx, x] = int(-0.5 + w * (1 << PRECISION_BITS)) if w < 0 else int(0.5 + w * (1 << PRECISION_BITS))
        bounds[xx] = (xmin, xmax)
    return ksize, bounds, coeffs


def _pass(img: np.ndarray, axis: int, out_size: int) -> np.ndarray:
    """One 8-bit pass along `axis` (1 = horizontal, 0 = vertical) of an (H, W, C) uint8 image."""
    _, bounds, coeffs = resample_table(img.shape[axis], out_size)
    src = np.moveaxis(img, axis, 0).astype(np.int64)
    out = np.empty((out_size,) + src.shape[1:], np.int64)
    for i in range(out_size):
        xmin, n = bounds[i]
        acc = np.full(src.shape[1:], 1 << (PRECISION_BITS - 1), np.int64)
        for x in range(n):
            acc += src[xmin + x] * int(coeffs[i, x])
        out[i] = acc
    out = np.where(out >= (1 << PRECISION_BITS << 8), 255, np.where(out <= 0, 0, out >> PRECISION_BITS))
    return np.moveaxis(out.astype(np.uint8), 0, axis)


def resize(img: np.ndarray, out_h: int, out_w: int) -> np.ndarray:
    """Image.resize((out_w, out_h), BILINEAR) of an (H, W, 3) uint8 array: horizontal pass first, each pass only on an axis whose size
    changes (ImagingResampleInner)."""
    if img.shape[1] != out_w:
        img = _pass(img, 1, out_w)
    if img.shape[0] != out_h:
        img = _pass(img, 0, out_h)
    return np.ascontiguousarray(img)


# ----------------------------------------------------------------------------------------------------------------------- colour
def luma(img: np.ndarray) -> np.ndarray:
    """convert("L"): (r*19595 + g*38470 + b*7471 + 0x8000) >> 16."""
    x = img.astype(np.int64)
    return ((x[..., 0] * 19595 + x[..., 1] * 38470 + x[..., 2] * 7471 + 0x8000) >> 16).astype(np.uint8)


def blend(degenerate, img: np.ndarray, factor: float) -> np.ndarray:
    """Image.blend(degenerate, img, factor): float32 in1 + alpha * (in2 - in1), clipped, truncated."""
    a = np.float32(factor)
    in1 = np.asarray(degenerate).astype(np.int32)
    in2 = img.astype(np.int32)
    t = in1.astype(np.float32) + a * (in2 - in1).astype(np.float32)
    t = np.broadcast_to(t, img.shape)
    return np.where(t <= 0, 0, np.where(t >= 255, 255, np.trunc(np.clip(t, 0, 255)))).astype(np.uint8)


def brightness(img, f):
    return blend(0, img, f)


def contrast_mean(img) -> int:
    """ImageEnhance.Contrast's degenerate level: int(ImageStat mean of the L image + 0.5), the mean a float64 sum / count."""
    lum = luma(img)
    return int(float(int(lum.astype(np.int64).sum())) / lum.size + 0.5)


def contrast(img, f, mean=None):
    m = contrast_mean(img) if mean is None else mean
    return blend(m, img, f)


def saturation(img, f):
    return blend(luma(img)[..., None], img, f)


def rgb_to_hsv(img: np.ndarray) -> np.ndarray:
    """rgb2hsv_row: float32 variables, float64 literals."""
    f32, f64 = np.float32, np.float64
    r, g, b = (img[..., i].astype(np.int32) for i in range(3))
    maxc = np.maximum(r, np.maximum(g, b))
    minc = np.minimum(r, np.minimum(g, b))
    same = maxc == minc
    cr = (maxc - minc).astype(f32)
    cr_safe = np.where(same, f32(1), cr)
    mx_safe = np.where(maxc == 0, 1, maxc).astype(f32)
    s = cr / mx_safe
    rc = (maxc - r).astype(f32) / cr_safe
    gc = (maxc - g).astype(f32) / cr_safe
    bc = (maxc - b).astype(f32) / cr_safe
    h = np.where(r == maxc, (bc - gc).astype(f64),
                 np.where(g == maxc, (f64(2.0) + rc.astype(f64)) - bc.astype(f64),
                          (f64(4.0) + gc.astype(f64)) - rc.astype(f64))).astype(f32)
    h = np.fmod(h.astype(f64) / 6.0 + 1.0, 1.0).astype(f32)
    uh = np.clip((h.astype(f64) * 255.0).astype(np.int64), 0, 255)
    us = np.clip((s.astype(f64) * 255.0).astype(np.int64), 0, 255)
    out = np.stack([np.where(same, 0, uh), np.where(same, 0, us), maxc], -1)
    return out.astype(np.uint8)


def _round_half_away(x: np.ndarray) -> np.ndarray:  # C round() of a non-negative double
    fl = np.floor(x)
    return (fl + ((x - fl) >= 0.5)).astype(np.int64)


def hsv_to_rgb(hsv: np.ndarray) -> np.ndarray:
    """hsv2rgb: i = floor(h*6.0/255.0) and the remainder in float64, f and fs stored as float32, fs*f a float32 product."""
    f32, f64 = np.float32, np.float64
    h, s, v = (hsv[..., i].astype(np.int32) for i in range(3))
    h6 = h.astype(f32).astype(f64) * 6.0 / 255.0
    i = np.floor(h6).astype(np.int64)
    f = (h6 - i.astype(f32).astype(f64)).astype(f32)
    fs = (s.astype(f32).astype(f64) / 255.0).astype(f32)
    vf = v.astype(f32).astype(f64)
    p = np.clip(_round_half_away(vf * (1.0 - fs.astype(f64))), 0, 255)
    q = np.clip(_round_half_away(vf * (1.0 - (fs * f).astype(f64))), 0, 255)
    t = np.clip(_round_half_away(vf * (1.0 - fs.astype(f64) * (1.0 - f.astype(f64)))), 0, 255)
    sel = i % 6
    cand = [(v, t, p), (q, v, p), (p, v, t), (p, q, v), (t, p, v), (v, p, q)]
    out = np.zeros(hsv.shape[:-1] + (3,), np.int64)
    for k, (a, b, c) in enumerate(cand):
        m = sel == k
        out[..., 0] = np.where(m, a, out[..., 0])
        out[..., 1] = np.where(m, b, out[..., 1])
        out[..., 2] = np.where(m, c, out[..., 2])
    grey = (s == 0)[..., None]
    return np.where(grey, v[..., None], out).astype(np.uint8)


def hue_shift(hue_factor: float) -> int:
    """np.uint8(hue_factor * 255) under numpy 1.21 on x86: truncate toward zero, then mod 256."""
    return int(math.trunc(hue_factor * 255.0)) % 256


def hue(img, shift: int):
    hsv = rgb_to_hsv(img)
    hsv[..., 0] = ((hsv[..., 0].astype(np.int32) + shift) % 256).astype(np.uint8)
    return hsv_to_rgb(hsv)


# ----------------------------------------------------------------------------------------------------------------------- clip chain
def resized_size(h: int, w: int, target: int):
    """torchvision 0.11.2 F_pil.resize with an int size -> (new_h, new_w); the short side equal to the target leaves the image as is."""
    short, long = (w, h) if w <= h else (h, w)
    if short == target:
        return h, w
    new_short, new_long = target, int(target * long / short)
    new_w, new_h = (new_short, new_long) if w <= h else (new_long, new_short)
    return new_h, new_w


def center_crop_offsets(rh: int, rw: int, S: int):
    return int(round((rh - S) / 2.0)), int(round((rw - S) / 2.0))


def apply_jitter(img, order, b, c, s, shift):
    for fn in order:
        if fn == 0:
            img = brightness(img, b)
        elif fn == 1:
            img = contrast(img, c)
        elif fn == 2:
            img = saturation(img, s)
        else:
            img = hue(img, shift)
    return img


def clip_crops(frames: np.ndarray, p: dict, S: int) -> np.ndarray:
    """(T, H, W, 3) uint8 + one clip's parameters (keys rh, rw, top, left, and when p["train"]: order, b, c, s, shift) -> the (T, S, S, 3)
    uint8 crops the reference feeds to ToTensor."""
    out = []
    for fr in frames:
        img = resize(np.asarray(fr, np.uint8), p["rh"], p["rw"])
        if p.get("train"):
            img = apply_jitter(img, p["order"], p["b"], p["c"], p["s"], p["shift"])
        out.append(img[p["top"]:p["top"] + S, p["left"]:p["left"] + S])
    return np.stack(out)


def normalize_table() -> np.ndarray:
    """ToTensor + Normalize(0.5, 0.5) of each uint8 value as the reference computes it (float32 div 255, then (x - 0.5) / 0.5)."""
    x = np.arange(256, dtype=np.float32) / np.float32(255)
    return ((x - np.float32(0.5)) / np.float32(0.5)).astype(np.float32)


def video_frames(crops: np.ndarray) -> np.ndarray:
    """(B, T, S, S, 3) uint8 crops -> (B, 3, T, S, S) float32 video_frames."""
    return np.ascontiguousarray(normalize_table()[crops].transpose(0, 4, 1, 2, 3))


def pattern_clip(T: int, H: int, W: int) -> np.ndarray:
    """The closed-form (T, H, W, 3) uint8 source of the large fixture clip (not stored): smooth ramps, a product term and a per-frame,
    per-channel offset, so that every resample tap and every jitter op sees varied values."""
    t, y, x, c = np.meshgrid(np.arange(T), np.arange(H), np.arange(W), np.arange(3), indexing="ij")
    v = x * 3 + y * 5 + ((x * y) >> 4) + ((x ^ y) & 31) * 2 + c * 85 + t * 29
    return (v & 255).astype(np.uint8)
