#!/usr/bin/env python3
"""The frame store's training launch at 64 clips x 32 frames of 240 x 427 (S = 112, random-noise frames), timed with one jitter order for all
clips: how much of the launch is VideoColorJitter's arithmetic, and how much of that the hue op (profiles/frame_data_bench.md)."""
import importlib
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import bench_frame_data as BF  # noqa: E402

pkg = importlib.import_module("revisiting-spatial-temporal-layouts_amd")
V, FD = pkg.video, pkg.frame_data
B, T, H, W, S = 64, 32, 240, 427, 112
rng = np.random.default_rng(0)
one = rng.integers(0, 256, (T, H, W, 3), dtype=np.uint8)
ids = [f"v{i}" for i in range(B)]
source = {vid: {str(j): np.roll(one[j], i, axis=1) for j in range(T)} for i, vid in enumerate(ids)}
store = FD.DeviceFrameStore(source, ids, S, "cuda")
store.ingest()
idx = list(range(B))
fi = np.tile(np.arange(T), (B, 1))
rh, rw = (int(x) for x in store.size[0])
for name, order in (("contrast first, hue last", (1, 0, 2, 3)), ("hue first, contrast last", (3, 0, 2, 1)), ("contrast second after brightness", (0, 1, 3, 2)),
                    ("contrast second after hue", (3, 1, 0, 2))):
    params = [V.ClipParams(rh, rw, 5, 40, True, order, 1.1, 0.9, 1.2, 0.05) for _ in idx]
    store.gather(idx, fi, params)
    launch, _ = BF.relaunch(store, B, T, True)
    print(f"{name}: {BF.events(launch, 10):.1f} us", flush=True)
store.gather(idx, fi)
launch, _ = BF.relaunch(store, B, T, False)
print(f"evaluation: {BF.events(launch, 10):.1f} us", flush=True)
