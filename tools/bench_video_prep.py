#!/usr/bin/env python3
"""Device video collater at the trunk's training shape: B = 64 clips x T = 32 frames from 240 x 427 sources, S = 112, in training and in
evaluation.  Measures (i) the kernels alone (stlt_video_prep_fwd on frames already on the device) against the HBM bound of source bytes
read + output bytes written at 6.3 TB/s, (ii) packing the clips into pinned host memory and the host -> device copy, (iii) the whole
DeviceVideoCollater.__call__, and (iv) beside them the reference's PIL chain per frame (Resize, VideoColorJitter in training, crop, ToTensor,
Normalize, stack) on the host with 16 worker threads.  Prints one JSON line; --out writes it to a file too."""
import argparse
import concurrent.futures
import importlib
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
pkg = importlib.import_module("revisiting-spatial-temporal-layouts_amd")
V = pkg.video
HBM = 6.3e12  # measured copy bandwidth of the MI355X (bytes/s)


def events(fn, n, warmup=3):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / n * 1e3  # us


def wall(fn, n, warmup=2):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t = time.perf_counter()
    for _ in range(n):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) / n * 1e6  # us


def pil_chain(frames, params, S, threads):
    """The reference's __getitem__ transforms on the host (torchvision 0.11.2's PIL calls), one clip per task."""
    from PIL import Image, ImageEnhance

    norm = lambda a: torch.from_numpy(np.array(a)).permute(2, 0, 1).float().div(255).sub_(0.5).div_(0.5)  # noqa: E731

    def clip(args):
        f, p = args
        out = []
        for fr in f:
            img = Image.fromarray(fr, "RGB")
            if (p.rh, p.rw) != fr.shape[:2]:
                img = img.resize((p.rw, p.rh), Image.BILINEAR)
            if p.train:
                for fn in p.order:
                    if fn == 0:
                        img = ImageEnhance.Brightness(img).enhance(p.brightness)
                    elif fn == 1:
                        img = ImageEnhance.Contrast(img).enhance(p.contrast)
                    elif fn == 2:
                        img = ImageEnhance.Color(img).enhance(p.saturation)
                    else:
                        h, s, v = img.convert("HSV").split()
                        nh = (np.array(h, dtype=np.uint8) + np.uint8(p.hue_shift)).astype(np.uint8)
                        img = Image.merge("HSV", (Image.fromarray(nh, "L"), s, v)).convert("RGB")
            out.append(norm(img.crop((p.left, p.top, p.left + S, p.top + S))))
        return torch.stack(out).transpose(0, 1)

    intra = torch.get_num_threads()
    torch.set_num_threads(1)  # one intra-op thread per worker, as in a DataLoader worker: 16 x 16 threads would oversubscribe
    try:
        with concurrent.futures.ThreadPoolExecutor(threads) as ex:
            return torch.stack(list(ex.map(clip, zip(frames, params))))
    finally:
        torch.set_num_threads(intra)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=64)
    ap.add_argument("--T", type=int, default=32)
    ap.add_argument("--H", type=int, default=240)
    ap.add_argument("--W", type=int, default=427)
    ap.add_argument("--S", type=int, default=112)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lib = pkg._lib.load()
    B, T, H, W, S = a.B, a.T, a.H, a.W, a.S
    g = torch.Generator().manual_seed(0)
    frames = [torch.randint(0, 256, (T, H, W, 3), dtype=torch.uint8, generator=g) for _ in range(B)]
    src_bytes = B * T * H * W * 3
    out_bytes = B * 3 * T * S * S * 4
    bound_us = (src_bytes + out_bytes) / HBM * 1e6
    res = {"B": B, "T": T, "H": H, "W": W, "S": S, "src_MB": src_bytes / 1e6, "out_MB": out_bytes / 1e6, "hbm_bound_us": bound_us,
           "device": torch.cuda.get_device_name(0)}
    packed = torch.cat([f.view(-1) for f in frames]).pin_memory()
    frames_d = packed.to("cuda")
    torch.cuda.synchronize()
    res["h2d_copy_us"] = events(lambda: frames_d.copy_(packed, non_blocking=True), a.iters)
    res["h2d_GBps"] = src_bytes / res["h2d_copy_us"] / 1e3
    pin = torch.empty_like(packed).pin_memory()

    def pack():
        pos = 0
        for f in frames:
            pin[pos:pos + f.numel()].copy_(f.view(-1))
            pos += f.numel()
    t = time.perf_counter()
    for _ in range(3):
        pack()
    res["pack_pinned_us"] = (time.perf_counter() - t) / 3 * 1e6
    for mode in ("eval", "train"):
        train = mode == "train"
        col = V.DeviceVideoCollater(S, train=train, device="cuda", generator=torch.Generator().manual_seed(1))
        samples = [{"frames": f, "labels": torch.tensor(0), "video_id": i} for i, f in enumerate(frames)]
        params = col.params(samples)
        # the kernels alone: the same launch DeviceVideoCollater.prep makes, on frames already on the device
        tabs, offs, n = [], {}, 0
        clips = (pkg._lib.VideoClip * B)()
        for i, p in enumerate(params):
            d = clips[i]
            d.src_offset, d.h, d.w, d.rh, d.rw, d.top, d.left = i * T * H * W * 3, H, W, p.rh, p.rw, p.top, p.left
            for axis, (nin, nout) in (("x", (W, p.rw)), ("y", (H, p.rh))):
                if nin == nout:
                    setattr(d, "tab_" + axis, -1)
                    continue
                if (nin, nout) not in offs:
                    k, tb = V.resample_table(nin, nout)
                    offs[(nin, nout)] = (n, k)
                    tabs.append(tb)
                    n += tb.size
                setattr(d, "tab_" + axis, offs[(nin, nout)][0])
                setattr(d, "ksize_" + axis, offs[(nin, nout)][1])
            d.jitter = int(train)
            if train:
                d.order[:] = list(p.order)
                d.brightness, d.contrast, d.saturation, d.hue_shift = p.brightness, p.contrast, p.saturation, p.hue_shift
        tables = np.concatenate(tabs).astype(np.int32)
        lut = V.normalize_table().numpy()
        ws_bytes = lib.stlt_video_prep_workspace_bytes(B, T, n)
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device="cuda")
        out = torch.empty(B, 3, T, S, S, device="cuda")

        def launch():
            pkg._lib.check(lib.stlt_video_prep_fwd(frames_d.data_ptr(), src_bytes, clips, tables.ctypes.data, n, lut.ctypes.data, B, T, S,
                                                   out.data_ptr(), ws.data_ptr(), ws_bytes, torch.cuda.current_stream().cuda_stream), "prep")
        us = events(launch, a.iters)
        ref = col(samples, params)["video_frames"]
        torch.cuda.synchronize()
        assert torch.equal(ref, out), "bench launch differs from the collater"
        r = {"kernels_us": us, "fraction_of_hbm_bound": bound_us / us, "frames_per_s_kernels": B * T / us * 1e6}
        r["collater_call_us"] = wall(lambda: col(samples, params), max(3, a.iters // 4))
        r["frames_per_s_collater"] = B * T / r["collater_call_us"] * 1e6
        try:
            np_frames = [f.numpy() for f in frames]
            t = time.perf_counter()
            host = pil_chain(np_frames, params, S, a.threads)
            r["pil_chain_us"] = (time.perf_counter() - t) * 1e6
            r["frames_per_s_pil_16_threads"] = B * T / r["pil_chain_us"] * 1e6
            r["pil_chain_equals_device"] = bool(torch.equal(host, ref.cpu()))
        except ImportError as e:
            r["pil_chain_us"] = None
            r["pil_note"] = f"Pillow not importable here: {e}"
        res[mode] = r
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
