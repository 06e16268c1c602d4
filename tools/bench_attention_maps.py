#!/usr/bin/env python3
"""Attention-map benchmark (profiles/attention_maps_bench.md).  Seeded synthetic inputs, closed-form weights; one JSON line per case.

1. The probabilities launch against the attention core, on the same packed QKV buffer in the same process:

  core_us         one stlt_attn_core_fwd launch (ops.attn_core)
  probs_us        one stlt_attn_probs_fwd launch, head-averaged (ops.attn_probs); probs_over_core = probs_us / core_us
  probs_ph_us     the same per head (H times the output)
  probs_hbm_frac  the launch's HBM bound over probs_us: the bytes the algorithm moves (q and k read, probs written, the mask) at 8 TB/s
  *_event_us      the same launches timed by the library's recorder (one event pair around each launch, stlt_prof_launches), the three
                  launches alternating; small launches sit at the launch floor in the back-to-back windows, so both are given

  shapes: cfg2 spatial (S = B*32 frames of 7 objects) and cfg2 temporal (B clips of 32 frames) at B = 64 and 1024, refdef temporal (17 frames),
  cfg4 spatial (36 objects), 12 heads of 64 channels.

2. Stlt.forward_attention against the model's ordinary forward on the dense schedule (cls_only_last_spatial and last_row_only_temporal
   off, the fused MHSA kernel off: the launch sequence forward_attention extends by one launch per layer), cfg2 at 64 and 1024 clips:

  dense_forward_ms, attention_ms, ratio = attention_ms / dense_forward_ms, and default_forward_ms (both elisions on) for scale.
  The fused kernel is switched off for the whole process (STLT_FUSED_MHSA=0 is read once), so default_forward_ms here is the default
  schedule without it.

Every figure is the median over --repeats windows of device-event time around --iters back-to-back calls, after --warmup calls of the
same shape; the windows of the two sides of a comparison alternate.  Needs a GPU: there is no fallback."""
import argparse
import importlib
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
os.environ["STLT_FUSED_MHSA"] = "0"  # before the library loads: the dense pair everywhere (part 2's baseline)
PKG = "revisiting-spatial-temporal-layouts_amd"
HBM_BYTES_PER_S = 8e12
KERNEL_CASES = (("cfg2 spatial", 32, 7, False), ("cfg2 temporal", 1, 32, True), ("refdef temporal", 1, 17, True), ("cfg4 spatial", 64, 36, False))
KERNEL_CLIPS = {"cfg2 spatial": (64, 1024), "cfg2 temporal": (64, 1024), "refdef temporal": (1024,), "cfg4 spatial": (64,)}


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
        raise SystemExit("bench_attention_maps.py needs a GPU")
    pkg = importlib.import_module(PKG)
    H, dh = 12, 64
    d = H * dh
    for name, seqs_per_clip, L, causal in KERNEL_CASES:
        for B in KERNEL_CLIPS[name]:
            S = B * seqs_per_clip
            g = torch.Generator().manual_seed(1)
            qkv = ((torch.rand(S, L, 3 * d, generator=g) * 2 - 1) * 1.5).to("cuda")
            kpm = torch.rand(S, L, generator=g) < 0.3
            kpm[:, 0] = False
            kpm = kpm.to(torch.uint8).to("cuda")
            fns = {"core": lambda: pkg.ops.attn_core(qkv, kpm, causal, H), "probs": lambda: pkg.ops.attn_probs(qkv, kpm, causal, H),
                   "probs_ph": lambda: pkg.ops.attn_probs(qkv, kpm, causal, H, per_head=True)}
            med, rng = alternating_ms(fns, torch, a.warmup, a.iters, a.repeats)
            # the library's own recorder: one event pair around every launch (stlt_prof_launches), the three launches alternating
            pkg.ops.prof_enable(True)
            pkg.ops.prof_launches()
            for _ in range(a.iters):
                for fn in fns.values():
                    fn()
            torch.cuda.synchronize()
            recs = pkg.ops.prof_launches()
            pkg.ops.prof_enable(False)
            ev = {"core": [r["us"] for r in recs if r["kernel"] in ("attn_spatial", "attn_temporal")],
                  "probs": [r["us"] for r in recs if r["kernel"] == "attn_probs" and "per_head=0" in r["note"]],
                  "probs_ph": [r["us"] for r in recs if r["kernel"] == "attn_probs" and "per_head=1" in r["note"]]}
            assert all(len(v) == a.iters for v in ev.values()), {k: len(v) for k, v in ev.items()}
            ev = {k: statistics.median(v) for k, v in ev.items()}
            qk = 2.0 * S * L * d * 4 + S * L
            bytes_avg, bytes_ph = qk + 4.0 * S * L * L, qk + 4.0 * S * L * L * H
            print(json.dumps(dict(part="kernel", shape=name, clips=B, S=S, L=L, H=H, dh=dh, causal=causal, core_us=round(med["core"] * 1e3, 2),
                                  probs_us=round(med["probs"] * 1e3, 2), probs_ph_us=round(med["probs_ph"] * 1e3, 2),
                                  core_event_us=round(ev["core"], 2), probs_event_us=round(ev["probs"], 2), probs_ph_event_us=round(ev["probs_ph"], 2),
                                  probs_over_core_event=round(ev["probs"] / ev["core"], 3), probs_hbm_frac_event=round(bytes_avg / HBM_BYTES_PER_S * 1e6 / ev["probs"], 3),
                                  probs_ph_hbm_frac_event=round(bytes_ph / HBM_BYTES_PER_S * 1e6 / ev["probs_ph"], 3),
                                  probs_over_core=round(med["probs"] / med["core"], 3), probs_ph_over_core=round(med["probs_ph"] / med["core"], 3),
                                  probs_bytes=int(bytes_avg), probs_hbm_frac=round(bytes_avg / HBM_BYTES_PER_S * 1e3 / med["probs"], 3),
                                  probs_ph_bytes=int(bytes_ph), probs_ph_hbm_frac=round(bytes_ph / HBM_BYTES_PER_S * 1e3 / med["probs_ph"], 3),
                                  ranges_ms=rng, device=torch.cuda.get_device_name(0))), flush=True)
            del qkv, kpm
    if a.skip_model:
        return
    c = pkg.synth.CONFIGS["cfg2"]
    m = pkg.Stlt(pkg.StltModelConfig(**pkg.synth.model_kwargs("cfg2")))
    m.load_state_dict(pkg.synth.make_state_dict({k: tuple(v.shape) for k, v in m.state_dict().items()}, seed=1234))
    m = m.train(False).to("cuda")
    bb = m.backbone
    for B in (64, 1024):
        batch = {k: v.to("cuda") for k, v in pkg.synth.make_batch(B, c["T"], c["N"], dataset=c["dataset"], seed=3).items()}

        def forward(dense):
            bb.cls_only_last_spatial = bb.last_row_only_temporal = not dense
            return m(batch)["stlt"]

        with torch.no_grad():
            fns = {"dense_forward": lambda: forward(True), "attention": lambda: m.forward_attention(batch),
                   "attention_ph": lambda: m.forward_attention(batch, per_head=True), "default_forward": lambda: forward(False)}
            med, rng = alternating_ms(fns, torch, max(2, a.warmup // 2), max(2, a.iters // (5 if B == 64 else 25)), a.repeats)
            err = (m.forward_attention(batch)["stlt"] - forward(True)).abs().max().item()
        print(json.dumps(dict(part="model", config="cfg2", clips=B, dense_forward_ms=round(med["dense_forward"], 4), attention_ms=round(med["attention"], 4),
                              ratio=round(med["attention"] / med["dense_forward"], 3), attention_per_head_ms=round(med["attention_ph"], 4),
                              ratio_per_head=round(med["attention_ph"] / med["dense_forward"], 3), default_forward_ms=round(med["default_forward"], 4),
                              ranges_ms=rng, logits_vs_dense_forward_max_abs=err, device=torch.cuda.get_device_name(0))), flush=True)
        del batch
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
