#!/usr/bin/env python3
"""Layout-gradient benchmark (profiles/layout_gradients_bench.md).  Seeded synthetic inputs, closed-form weights; one JSON line per case.

1. The input-gradient kernel (stlt_embed_bwd_inputs) against its HBM bound, rows * d * 4 bytes read once at 8 TB/s (the 20 bytes written per
   token are counted too), d = 768, with and without scores, at the token counts of the model cases below:

  us, event_us    one launch: the median over windows of back-to-back calls, and the library's recorder (one event pair around each launch)
  hbm_frac        bound / time for either

2. Stlt.forward_saliency against the model's ordinary forward and against a training forward + full backward of the same batch
   (autograd path, every parameter trainable), padded schedule and skip_padding, cfg2 at 64 and 1024 clips and T = 17 x N = 5 at 64 clips:

  forward_ms, saliency_ms, train_ms, saliency_over_forward, saliency_over_train, and the matrix-core FLOPs each enqueues
  (ops.prof_take_gemm_flops) with their ratio.

Every time is the median over --repeats windows of device-event time around --iters back-to-back calls, after --warmup calls of the same
shape; the windows of the sides of a comparison alternate.  Needs a GPU: there is no fallback."""
import argparse
import importlib
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PKG = "revisiting-spatial-temporal-layouts_amd"
HBM_BYTES_PER_S = 8e12
MODEL_CASES = (("cfg2", 64), ("cfg2", 1024), ("refdef", 64))  # refdef: T = 17 frames of N = 5 slots


def alternating_ms(fns, torch, warmup, iters, repeats):
    """{name: median ms per call}: the windows of the functions alternate, so drift of the machine hits them alike"""
    for fn in fns.values():
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    out = {k: [] for k in fns}
    for _ in range(repeats):
        for k, fn in fns.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(iters):
                fn()
            e1.record()
            e1.synchronize()
            out[k].append(e0.elapsed_time(e1) / iters)
    return {k: statistics.median(v) for k, v in out.items()}, {k: [round(min(v), 4), round(max(v), 4)] for k, v in out.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--skip-model", action="store_true")
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_saliency.py needs a GPU")
    pkg = importlib.import_module(PKG)
    dev_name = torch.cuda.get_device_name(0)
    d = 768
    g = torch.Generator().manual_seed(1)
    box_w, score_w = torch.rand(d, 4, generator=g).to("cuda"), torch.rand(d, 1, generator=g).to("cuda")
    for name, B in MODEL_CASES:
        c = pkg.synth.CONFIGS[name]
        rows = B * c["T"] * c["N"]
        d_pre = (torch.rand(rows, d, generator=g) * 2 - 1).to("cuda")
        fns = {"boxes": lambda: pkg.ops.embed_bwd_inputs(d_pre, box_w), "boxes_scores": lambda: pkg.ops.embed_bwd_inputs(d_pre, box_w, score_w)}
        med, rng = alternating_ms(fns, torch, a.warmup, a.iters, a.repeats)
        pkg.ops.prof_enable(True)
        pkg.ops.prof_launches()
        for _ in range(a.iters):
            for fn in fns.values():
                fn()
        torch.cuda.synchronize()
        recs = [r["us"] for r in pkg.ops.prof_launches() if r["kernel"] == "embed_bwd"]
        pkg.ops.prof_enable(False)
        assert len(recs) == 2 * a.iters, len(recs)
        ev = {"boxes": statistics.median(recs[0::2]), "boxes_scores": statistics.median(recs[1::2])}
        bound_us = {"boxes": rows * (4.0 * d + 16) / HBM_BYTES_PER_S * 1e6, "boxes_scores": rows * (4.0 * d + 20) / HBM_BYTES_PER_S * 1e6}
        print(json.dumps(dict(part="kernel", rows=rows, d=d, like=f"{name} x {B} clips", bound_us={k: round(v, 2) for k, v in bound_us.items()},
                              us={k: round(v * 1e3, 2) for k, v in med.items()}, event_us={k: round(v, 2) for k, v in ev.items()},
                              hbm_frac={k: round(bound_us[k] / (med[k] * 1e3), 3) for k in med}, hbm_frac_event={k: round(bound_us[k] / ev[k], 3) for k in ev},
                              ranges_ms=rng, device=dev_name)), flush=True)
        del d_pre
    if a.skip_model:
        return
    for name, B in MODEL_CASES:
        c = pkg.synth.CONFIGS[name]
        m = pkg.Stlt(pkg.StltModelConfig(**pkg.synth.model_kwargs(name)))
        m.load_state_dict(pkg.synth.make_state_dict({k: tuple(v.shape) for k, v in m.state_dict().items()}, seed=1234))
        m = m.train(False).to("cuda")
        host = pkg.synth.make_batch(B, c["T"], c["N"], dataset=c["dataset"], seed=3)
        batch = dict({k: v.to("cuda") for k, v in host.items()}, **pkg.collate.real_counts(host))
        labels = torch.randint(0, c["num_classes"], (B,), generator=torch.Generator().manual_seed(5)).to("cuda")

        def forward():
            with torch.no_grad():
                return m(batch)["stlt"]

        def train():
            m.zero_grad(set_to_none=True)
            torch.nn.functional.cross_entropy(m(batch)["stlt"], labels).backward()

        for skip in (False, True):
            m.backbone.skip_padding = skip
            fns = {"forward": forward, "saliency": lambda: m.forward_saliency(batch), "train": train}
            it = max(2, a.iters // (5 if B == 64 else 25))
            med, rng = alternating_ms(fns, torch, max(2, a.warmup // 2), it, a.repeats)
            flops = {}
            pkg.ops.prof_enable(True)
            for k, fn in fns.items():
                pkg.ops.prof_take_gemm_flops()
                fn()
                torch.cuda.synchronize()
                flops[k] = pkg.ops.prof_take_gemm_flops()
            pkg.ops.prof_enable(False)
            pkg.ops.prof_launches()
            print(json.dumps(dict(part="model", config=name, clips=B, T=c["T"], N=c["N"], skip_padding=skip, forward_ms=round(med["forward"], 4),
                                  saliency_ms=round(med["saliency"], 4), train_ms=round(med["train"], 4),
                                  saliency_over_forward=round(med["saliency"] / med["forward"], 3), saliency_over_train=round(med["saliency"] / med["train"], 3),
                                  gemm_gflop={k: round(v / 1e9, 2) for k, v in flops.items()}, gemm_flop_saliency_over_train=round(flops["saliency"] / flops["train"], 3),
                                  ranges_ms=rng, device=dev_name)), flush=True)
        del m, batch
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
