#!/usr/bin/env python3
"""Pixel-gradient benchmark (profiles/pixel_gradients_bench.md).  Seeded synthetic inputs, closed-form weights; one JSON line per case,
at 16 and 64 clips of 32 x 112 x 112 (--clips).

1. The thin data-gradient launch alone (stlt_conv3d_bwd_data_thin, the stem's geometry, NCDHW and NDHWC) against its matrix-pipe bound:
   the formulation's FLOPs — every 2x2 block a row of 16 columns over a 112·c_out contraction, zero taps and the padded channel included,
   whole 8 x 16 tiles — at 157.3 TFLOP/s.  useful_share = the FLOPs of the taps and channels that exist / the formulation's.

  us, event_us    one launch: the median over windows of back-to-back calls, and the library's recorder (one event pair around each launch)
  pipe_frac       bound / time

2. The trunk's reverse sweep on one tape: stlt_r3d_backward (the parent's entry point: 53 weight gradients), stlt_r3d_backward_inputs with
   dvideo only (the input-only sweep), and with weights plus video; ratios against stlt_r3d_backward.

3. Resnet3D.forward_saliency against Resnet3D.forward (no_grad) of the same batch.

Every time is the median over --repeats windows of device-event time around --iters back-to-back calls, after --warmup calls of the same
shape; the windows of the sides of a comparison alternate.  Needs a GPU: there is no fallback."""
import argparse
import ctypes as C
import importlib
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PKG = "revisiting-spatial-temporal-layouts_amd"
PIPE_FLOPS = 157.3e12
T, H, W = 32, 112, 112


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
    ap.add_argument("--clips", type=int, nargs="+", default=[16, 64])
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=5)
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_pixel_saliency.py needs a GPU")
    pkg = importlib.import_module(PKG)
    L, lib = pkg._lib, pkg._lib.load()
    dev_name = torch.cuda.get_device_name(0)
    stream = lambda: torch.cuda.current_stream().cuda_stream  # noqa: E731
    g = torch.Generator().manual_seed(1)
    kw = pkg.synth.model_kwargs("cfg1")
    cfg = pkg.AppearanceModelConfig(num_classes=kw["num_classes"], hidden_size=kw["hidden_size"], num_attention_heads=kw["num_attention_heads"],
                                    hidden_dropout_prob=0.0, appearance_num_frames=32, train_trunk=True)
    m = pkg.Resnet3D(cfg)
    m.load_state_dict(pkg.synth.make_r3d_state_dict({k: tuple(v.shape) for k, v in m.state_dict().items()}, seed=4242), strict=True)
    m = m.to("cuda").train(False)
    ws = [conv.weight for conv, _ in pkg.modelling.resnet3d.trunk_convs(m.resnet)]
    w_stem = torch.randn(64, 3, 7, 7, 7, generator=g).to("cuda")
    for B in a.clips:
        # ---- 1. the launch alone
        d = L.Conv3dDesc(B, T, H, W, 3, 64, 7, 7, 7, 1, 2, 2, 3, 3, 3)
        Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
        dy = torch.randn(B, T, Ho, Wo, 64, device="cuda")
        wt = torch.empty(int(lib.stlt_conv3d_repack_dgrad_thin_floats(C.byref(d))), device="cuda")
        L.check(lib.stlt_conv3d_repack_dgrad_thin(w_stem.data_ptr(), C.byref(d), None, wt.data_ptr(), stream()), "repack")
        dx = {"ncdhw": torch.empty(B, 3, T, H, W, device="cuda"), "ndhwc": torch.empty(B, T, H, W, 4, device="cuda")}
        code = {"ncdhw": L.DX_NCDHW, "ndhwc": L.DX_NDHWC}
        fns = {k: (lambda k=k: L.check(lib.stlt_conv3d_bwd_data_thin(C.byref(d), dy.data_ptr(), wt.data_ptr(), dx[k].data_ptr(), code[k], stream()), k))
               for k in dx}
        med, rng = alternating_ms(fns, torch, a.warmup, a.iters, a.repeats)
        pkg.ops.prof_enable(True)
        pkg.ops.prof_launches()
        for _ in range(a.iters):
            for fn in fns.values():
                fn()
        torch.cuda.synchronize()
        recs = [r for r in pkg.ops.prof_launches() if r["kernel"] == "conv_dgrad_thin"]
        pkg.ops.prof_enable(False)
        assert len(recs) == 2 * a.iters, len(recs)
        ev = {"ncdhw": statistics.median(r["us"] for r in recs[0::2]), "ndhwc": statistics.median(r["us"] for r in recs[1::2])}
        flops = recs[0]["flops"]                                   # the formulation's, whole tiles (the launcher's own count)
        useful = 2.0 * B * T * Ho * Wo * 7 * 49 * 3 * 64           # interior count: 7 x 49 taps x 3 channels x 64 c_out per 2x2 block
        bound_us = flops / PIPE_FLOPS * 1e6
        print(json.dumps(dict(part="kernel", clips=B, note=recs[0]["note"], gflop=round(flops / 1e9, 1), useful_share=round(useful / flops, 3),
                              useful_share_of_whole_blocks=round(49 / 64 * 3 / 4, 3), bound_us=round(bound_us, 1),
                              us={k: round(v * 1e3, 1) for k, v in med.items()}, event_us={k: round(v, 1) for k, v in ev.items()},
                              pipe_frac={k: round(bound_us / (v * 1e3), 3) for k, v in med.items()}, ranges_ms=rng, device=dev_name)), flush=True)
        del dy, dx, wt
        torch.cuda.empty_cache()
        # ---- 2. the sweeps on one tape
        video = pkg.synth.make_video(B, T, H, W, seed=3).to("cuda").requires_grad_(True)
        pooled = m._runner.run(m.resnet, video, features=False, pooled=True)[1]
        ctx = pooled.grad_fn  # R3dTrunkFn's context: the tape, the parameter table and the dgrad copies of this forward
        dpool = torch.rand(B, 2048, generator=g).to("cuda")
        dws = [torch.empty_like(w) for w in ws]
        dw_ptrs = L.R3dPointers(*[t.data_ptr() for t in dws])
        dgrad = L.R3dPointers(*[t.data_ptr() for t in ctx.dgrad])
        dvideo = torch.empty(B, 3, T, H, W, device="cuda")
        wsb = torch.empty(int(lib.stlt_r3d_backward_inputs_workspace_bytes(B, T, H, W)), dtype=torch.uint8, device="cuda")
        head = (C.byref(ctx.params), dgrad, ctx.tape.data_ptr(), ctx.tape.numel(), B, T, H, W, None, dpool.data_ptr())
        tail = (wsb.data_ptr(), wsb.numel())
        fns = {"backward": lambda: L.check(lib.stlt_r3d_backward(*head, dw_ptrs, 0, *tail, stream()), "stlt_r3d_backward"),
               "inputs_video_only": lambda: L.check(lib.stlt_r3d_backward_inputs(*head, None, 0, dvideo.data_ptr(), *tail, stream()), "inputs"),
               "inputs_weights_and_video": lambda: L.check(lib.stlt_r3d_backward_inputs(*head, dw_ptrs, 0, dvideo.data_ptr(), *tail, stream()), "inputs")}
        med, rng = alternating_ms(fns, torch, 1, max(1, a.iters // 2), a.repeats)
        print(json.dumps(dict(part="sweep", clips=B, ms={k: round(v, 3) for k, v in med.items()},
                              video_only_over_backward=round(med["inputs_video_only"] / med["backward"], 3),
                              weights_and_video_over_backward=round(med["inputs_weights_and_video"] / med["backward"], 3), ranges_ms=rng, device=dev_name)),
              flush=True)
        del pooled, ctx, dws, dvideo, wsb, head, tail, fns
        torch.cuda.empty_cache()
        # ---- 3. the model
        batch = {"video_frames": video.detach()}

        def forward():
            with torch.no_grad():
                return m(batch)["resnet3d"]

        fns = {"forward": forward, "saliency": lambda: m.forward_saliency(batch)}
        med, rng = alternating_ms(fns, torch, 1, max(1, a.iters // 2), a.repeats)
        print(json.dumps(dict(part="model", model="Resnet3D", clips=B, forward_ms=round(med["forward"], 3), saliency_ms=round(med["saliency"], 3),
                              saliency_over_forward=round(med["saliency"] / med["forward"], 3), ranges_ms=rng, device=dev_name)), flush=True)
        del video, batch
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
