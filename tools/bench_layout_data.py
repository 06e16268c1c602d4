#!/usr/bin/env python3
"""Device layout dataset benchmark (profiles/layout_data_bench.md): on a seeded synthetic annotation set of --videos videos
(synth.make_layout_annotations), for the refdef layout (something, T = 16 + 1, N = 5) and action_genome (N = 9), at B = 64 and 1024:

  table     one-time build: JSON parse into the host tables, then upload + the box kernel (synchronised)
  bytes     resident device bytes per kept object (all tables / objects)
  wall      per collate(indices) call, steady state: wall time of K back-to-back calls (one sync at the end) / K
  host      the host part of a call (frame indices, packing, checks, launch): time until collate returns
  device    the stream time of a call (index copy + kernel), from events around it with the stream held busy until it is enqueued
  restated  tests/layout_restated.py (numpy, per sample) on the same batches, same process

--reference SRC times the reference's StltDataset + StltCollater on the same files instead, SRC being the reference's src/ directory
(CPU only; its modules for the appearance path are inert MagicMocks, as in tools/gen_golden_layout_dataset.py).
One JSON line per (dataset, B) on stdout."""
import argparse
import importlib
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
PKG = "revisiting-spatial-temporal-layouts_amd"
SETS = {"something": 4, "action_genome": 8}  # max objects per frame: N = 5 (refdef) and 9


def write_set(dataset, n_videos, d):
    synth = importlib.import_module(PKG + ".synth")
    import layout_restated as R
    p, _ = synth.write_layout_annotations(d, dataset, n_videos, 2024, max_frames=48, max_objects=SETS[dataset])
    return p, R.load_annotations(dataset, p)


def bench_device(dataset, p, data, batches, iters, train):
    import torch
    ld = importlib.import_module(PKG + ".layout_data")
    import layout_restated as R
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    ds = ld.DeviceStltDataset(R.config(dataset, train, p), device="cuda")
    t1 = time.perf_counter()
    ds.upload()
    torch.cuda.synchronize()
    t2 = time.perf_counter()
    rng = np.random.default_rng(0)
    out = []
    for B in batches:
        idx = [rng.integers(0, len(ds), size=B).tolist() for _ in range(iters)]
        for i in idx[:3]:
            ds.collate(i)
        torch.cuda.synchronize()
        # wall: back to back, one sync
        w0 = time.perf_counter()
        for i in idx:
            ds.collate(i)
        torch.cuda.synchronize()
        wall = (time.perf_counter() - w0) / iters
        # host part and device part of each call: a spin kernel ahead of the first event keeps the stream busy until the call has
        # been enqueued, so the events bracket the copy and the kernel alone
        host, dev = [], []
        for i in idx:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda._sleep(20_000_000)
            e0.record()
            h0 = time.perf_counter()
            ds.collate(i)
            host.append(time.perf_counter() - h0)
            e1.record()
            e1.synchronize()
            dev.append(e0.elapsed_time(e1) / 1e3)
        r = R.Restated(*data, dataset, 16, train, 0.5, ld.CATEGORY2ID[dataset], ld.FRAME2TYPE[dataset])
        n_r = max(1, min(5, 4096 // B))
        r0 = time.perf_counter()
        for i in idx[:n_r]:
            r.collate(i)
        restated = (time.perf_counter() - r0) / n_r
        out.append(dict(dataset=dataset, B=B, T=ds.T + 1, N=ds.N, train=train, videos=len(ds), objects=int(len(ds.object_category)),
                        parse_s=round(t1 - t0, 3), upload_s=round(t2 - t1, 4), bytes_per_object=round(ds.device_bytes() / max(1, len(ds.object_category)), 2),
                        wall_ms=round(wall * 1e3, 4), host_ms=round(float(np.median(host)) * 1e3, 4), device_ms=round(float(np.median(dev)) * 1e3, 4),
                        restated_ms=round(restated * 1e3, 2), device=torch.cuda.get_device_name(0)))
    return out


def bench_reference(src, dataset, p, batches, train):
    from unittest.mock import MagicMock
    sys.path.insert(0, src)
    for name in ("h5py", "ffmpeg", "torchvision", "torchvision.transforms", "torchvision.transforms.functional", "PIL", "PIL.Image", "natsort"):
        sys.modules.setdefault(name, MagicMock())
    from modelling.configs import DataConfig
    from modelling.datasets import StltCollater, StltDataset
    cfg = DataConfig(dataset_name=dataset, dataset_path=p["annotations"], labels_path=p["labels"], videoid2size_path=p["sizes"], videos_path="",
                     train=train, layout_num_frames=16, score_threshold=0.5)
    t0 = time.perf_counter()
    ds = StltDataset(cfg)
    t1 = time.perf_counter()
    col = StltCollater(cfg)
    rng = np.random.default_rng(0)
    out = []
    for B in batches:
        n = max(1, min(5, 4096 // B))
        idx = [rng.integers(0, len(ds), size=B).tolist() for _ in range(n)]
        r0 = time.perf_counter()
        for i in idx:
            col([ds[j] for j in i])
        out.append(dict(dataset=dataset, B=B, train=train, reference_ms=round((time.perf_counter() - r0) / n * 1e3, 2), reference_init_s=round(t1 - t0, 3)))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--videos", type=int, default=20000)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--batches", default="64,1024")
    ap.add_argument("--modes", default="eval,train", help="eval (test-mode indices), train (sampled indices) or both")
    ap.add_argument("--reference", metavar="SRC", help="time the reference (its src/ directory) instead")
    a = ap.parse_args()
    batches = [int(b) for b in a.batches.split(",")]
    with tempfile.TemporaryDirectory() as d:
        for dataset in SETS:
            g0 = time.perf_counter()
            p, data = write_set(dataset, a.videos, d)
            gen = time.perf_counter() - g0
            for mode in a.modes.split(","):
                train = mode == "train"
                rows = bench_reference(a.reference, dataset, p, batches, train) if a.reference else bench_device(dataset, p, data, batches, a.iters, train)
                for r in rows:
                    print(json.dumps(dict(r, generate_s=round(gen, 2))), flush=True)


if __name__ == "__main__":
    main()
