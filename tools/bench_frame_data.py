#!/usr/bin/env python3
"""Device frame store at the shape of profiles/video_prep_bench.md: 64 clips x 32 frames from 240 x 427 sources, S = 112, all in one
process on the same clips.  Measures (i) the parent path, the whole DeviceVideoCollater.__call__ on the decoded clips, (ii)
DeviceAppearanceDataset.collate() from a fully resident store, whole call and kernels alone, in evaluation and in training, (iii) the
same with half of the clips spilled, (iv) ingest: frames/s, split into host decoding and the rest (upload + device resize), the resize
kernels alone, and store.nbytes.  The kernels are held against their byte bounds at 6.3 TB/s.  Prints one JSON line; --out writes it
to a file, --md writes the table as markdown."""
import argparse
import importlib
import io
import json
import os
import sys
import tempfile
import time
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
pkg = importlib.import_module("revisiting-spatial-temporal-layouts_amd")
V, FD = pkg.video, pkg.frame_data
HBM = 6.3e12  # measured copy bandwidth of the MI355X (bytes/s)
AIM = 0.5


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


def relaunch(store, B, T, jitter):
    """The launch the last gather() made, again, on its descriptor block: the kernels (and the copy of the block) alone."""
    lib = pkg._lib.load()
    slot = store._ring[(store._next - 1) % len(store._ring)]
    buf = store._buf
    sums = torch.empty(B * T, dtype=torch.int64, device=store.device)
    out = torch.empty(B, 3, T, store.S, store.S, device=store.device)

    def launch():
        pkg._lib.check(lib.stlt_frames_batch_fwd(buf.data_ptr(), buf.numel(), None, 0, slot[0].data_ptr(), slot[1].data_ptr(), store._lut.data_ptr(),
                                                 B, T, store.S, sums.data_ptr() if jitter else None, out.data_ptr(),
                                                 torch.cuda.current_stream().cuda_stream), "stlt_frames_batch_fwd")
    return launch, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=64)
    ap.add_argument("--T", type=int, default=32)
    ap.add_argument("--H", type=int, default=240)
    ap.add_argument("--W", type=int, default=427)
    ap.add_argument("--S", type=int, default=112)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--out", default=None)
    ap.add_argument("--md", default=None)
    a = ap.parse_args()
    B, T, H, W, S = a.B, a.T, a.H, a.W, a.S
    dev = "cuda"
    rng = np.random.default_rng(0)
    # smooth frames with noise on top, so that the JPEG sizes are those of video frames rather than of noise
    y, x = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    base = np.stack([(x * 255 // W), (y * 255 // H), ((x + y) * 255 // (W + H))], -1)
    raw = [np.clip(base[None] + rng.integers(-24, 25, (T, H, W, 3)) + rng.integers(-40, 41, (T, 1, 1, 3)), 0, 255).astype(np.uint8) for _ in range(B)]
    tmp = tempfile.TemporaryDirectory()
    p, _ = pkg.synth.write_layout_annotations(tmp.name, "something", B, 5)
    ids = [v["id"] for v in json.load(open(p["annotations"]))]
    try:
        from PIL import Image

        def enc(f):
            b = io.BytesIO()
            Image.fromarray(f, "RGB").save(b, "JPEG", quality=90)
            return b.getvalue()
        source = {vid: {str(j): enc(f) for j, f in enumerate(c)} for vid, c in zip(ids, raw)}
        clips = [np.stack([np.asarray(Image.open(io.BytesIO(source[vid][str(j)]))) for j in range(T)]) for vid in ids]
        encoded = "JPEG quality 90, %.1f KB per frame" % (sum(len(f) for fr in source.values() for f in fr.values()) / (B * T) / 1e3)
    except ImportError:
        source = {vid: {str(j): f for j, f in enumerate(c)} for vid, c in zip(ids, raw)}
        clips, encoded = raw, "decoded arrays (Pillow not importable): the decoding share is a copy"
    del raw

    def config(train):
        return types.SimpleNamespace(dataset_name="something", dataset_path=p["annotations"], labels_path=p["labels"], videoid2size_path=p["sizes"],
                                     train=train, appearance_num_frames=T, spatial_size=S)

    rh, rw = V.resized_size(H, W, int(S * 1.15))
    out_bytes = B * 3 * T * S * S * 4
    res = {"B": B, "T": T, "H": H, "W": W, "S": S, "resized": [rh, rw], "source": encoded, "device": torch.cuda.get_device_name(0),
           "bound_eval_us": (B * T * S * S * 3 + out_bytes) / HBM * 1e6, "bound_train_us": (B * T * rh * rw * 3 + out_bytes) / HBM * 1e6,
           "bound_train_two_reads_us": (2 * B * T * rh * rw * 3 + out_bytes) / HBM * 1e6}
    # ---- ingest ----
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    store = FD.DeviceAppearanceDataset(config(False), source, dev).store
    store.ingest()
    torch.cuda.synchronize()
    total = time.perf_counter() - t0
    frames_d = torch.from_numpy(clips[0]).to(dev)

    def resize_one():
        store._resize_into(store._buf, 0, 0, frames_d)
    resize_us = events(resize_one, 5, warmup=1)  # includes the device-to-device hand-over of the source, not its upload
    res["ingest"] = {"frames": B * T, "seconds": total, "frames_per_s": B * T / total, "decode_s": store.stats["decode_s"],
                     "upload_and_resize_s": total - store.stats["decode_s"], "resize_kernels_us_per_video": resize_us,
                     "resize_frames_per_s_kernels": T / resize_us * 1e6, "nbytes": store.nbytes, "source_bytes": B * T * H * W * 3}
    # ---- batches ----
    idx = list(range(B))
    half_cap = int(store.video_bytes[:B // 2].sum())
    for mode in ("eval", "train"):
        train = mode == "train"
        ds = FD.DeviceAppearanceDataset(config(train), source, dev, generator=torch.Generator().manual_seed(1))
        ds.store._buf, ds.store._lut = store._buf, store._lut  # the same resident frames: one ingest serves both modes
        np.random.seed(0)
        fi = ds.sample_indices(idx)
        params = ds.store.clip_params(idx, train, torch.Generator().manual_seed(2))
        samples = [{"frames": torch.from_numpy(clips[b][fi[b]]), "labels": torch.tensor(0), "video_id": ids[b]} for b in idx]
        col = V.DeviceVideoCollater(S, train=train, device=dev, generator=torch.Generator().manual_seed(1))
        want = col(samples, params)["video_frames"]
        got = ds.store.gather(idx, fi, params)
        launch, out = relaunch(ds.store, B, T, train)
        launch()
        torch.cuda.synchronize()
        assert torch.equal(got, want) and torch.equal(out, want), "the store's batch differs from the collater's"
        r = {"parent_call_us": wall(lambda: col(samples), max(3, a.iters // 4))}
        r["kernels_us"] = events(launch, a.iters)
        bound = res["bound_eval_us"] if not train else res["bound_train_us"]
        r["fraction_of_bound"] = bound / r["kernels_us"]
        if train:
            r["fraction_of_bound_two_reads"] = res["bound_train_two_reads_us"] / r["kernels_us"]
        r["gather_us"] = wall(lambda: ds.store.gather(idx, fi, params), a.iters)
        r["collate_us"] = wall(lambda: ds.collate(idx), a.iters)
        r["speedup_collate_vs_parent"] = r["parent_call_us"] / r["collate_us"]
        cut = FD.DeviceAppearanceDataset(config(train), source, dev, capacity_bytes=half_cap, generator=torch.Generator().manual_seed(1))
        cut.store.ingest()
        assert sum(cut.store.resident(i) for i in idx) == B // 2
        assert torch.equal(cut.store.gather(idx, fi, params), want)
        before = cut.store.stats["decode_s"]
        n_spill = max(2, a.iters // 5)
        r["collate_half_spilled_us"] = wall(lambda: cut.collate(idx), n_spill, warmup=1)
        r["half_spilled_decode_us"] = (cut.store.stats["decode_s"] - before) / (n_spill + 1) * 1e6
        del cut
        res[mode] = r
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    if a.md:
        with open(a.md, "w") as f:
            f.write(markdown(res))


def markdown(res):
    e, t, g = res["eval"], res["train"], res["ingest"]
    met = lambda x: "met" if x >= AIM else "missed"  # noqa: E731
    ms = lambda us: f"{us / 1e3:.2f} ms"  # noqa: E731
    slow = [m for m in ("eval", "train") if res[m]["speedup_collate_vs_parent"] < 3.0]
    lines = [
        "# Device frame store at the trunk's training shape",
        "",
        f"`tools/bench_frame_data.py` on one {res['device']}: B = {res['B']} clips, T = {res['T']} frames each, {res['H']} x {res['W']} sources "
        f"({res['source']}), S = {res['S']} (resized to {res['resized'][0]} x {res['resized'][1]}), one process, the same clips on every row.  "
        "Event timing for the kernels, wall clock for whole calls.  Every number below is from that run.",
        "",
        f"Bounds at 6.3 TB/s: evaluation reads the crops and writes the output, **{res['bound_eval_us']:.1f} us**; training reads the whole "
        f"resized frames and writes the output, **{res['bound_train_us']:.1f} us** ({res['bound_train_two_reads_us']:.1f} us if the second "
        "pass over the frames misses the caches).",
        "",
        "| step | evaluation | training |",
        "|---|---|---|",
        f"| parent path: whole `DeviceVideoCollater.__call__` | {ms(e['parent_call_us'])} | {ms(t['parent_call_us'])} |",
        f"| `collate()`, every clip resident, whole call | {ms(e['collate_us'])} | {ms(t['collate_us'])} |",
        f"| speed-up over the parent call | **{e['speedup_collate_vs_parent']:.1f} x** | **{t['speedup_collate_vs_parent']:.1f} x** |",
        f"| `store.gather()` alone (indices and parameters given) | {ms(e['gather_us'])} | {ms(t['gather_us'])} |",
        f"| kernels alone (`stlt_frames_batch_fwd`) | {e['kernels_us']:.1f} us | {t['kernels_us']:.1f} us |",
        f"| fraction of the bound (aim {AIM}) | **{e['fraction_of_bound']:.2f}** ({met(e['fraction_of_bound'])}) | "
        f"**{t['fraction_of_bound']:.2f}** ({met(t['fraction_of_bound'])}; {t['fraction_of_bound_two_reads']:.2f} against two reads) |",
        f"| `collate()`, half of the clips spilled, whole call | {ms(e['collate_half_spilled_us'])} | {ms(t['collate_half_spilled_us'])} |",
        f"| of that, decoding the spilled frames on the host | {ms(e['half_spilled_decode_us'])} | {ms(t['half_spilled_decode_us'])} |",
        "",
        f"Ingest of {g['frames']} frames: {g['seconds']:.2f} s, **{g['frames_per_s']:.0f} frames/s**; host decoding {g['decode_s']:.2f} s, upload and "
        f"device resize {g['upload_and_resize_s']:.2f} s.  The resize kernels alone take {g['resize_kernels_us_per_video']:.0f} us per video of "
        f"{res['T']} frames ({g['resize_frames_per_s_kernels'] / 1e6:.2f} M frames/s).  `store.nbytes` = {g['nbytes'] / 1e6:.1f} MB for "
        f"{g['source_bytes'] / 1e6:.1f} MB of decoded source.",
        "",
    ]
    if slow:
        lines += [f"**Something is wrong:** the resident `collate()` is less than 3 x faster than the parent call in {', '.join(slow)}; the store "
                  "removes the packing and the upload, which are 19.0 of the parent's 19.2 - 21.0 ms.", ""]
    else:
        lines += ["The resident `collate()` is at least 3 x faster than the parent call measured beside it in both modes, as removing the packing "
                  "and the upload (19.0 of the parent's 19.2 - 21.0 ms in `profiles/video_prep_bench.md`) predicts.", ""]
    return "\n".join(lines)


if __name__ == "__main__":
    main()
