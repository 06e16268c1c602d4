#!/usr/bin/env python3
"""Per-prefix logits benchmark (profiles/prefix_logits_bench.md): Stlt.forward_prefixes against the ordinary forward and against the
naive route, at cfg2 x {64, 1024} clips and refdef x 64 clips (seeded synthetic batches, closed-form weights).  Per case, one JSON line:

  forward_ms      Stlt.forward on the batch (both exact elisions on, as the model's defaults)
  prefixes_ms     Stlt.forward_prefixes on the same batch; ratio = prefixes_ms / forward_ms
  naive_ms        T Stlt.forward calls on collate.prefix_batch(batch, t), t = 0 .. T-1 (the batches are cut outside the timed window)
  probe_us        one stlt_attn_prefix_probe_fwd launch alone at the case's shape (B clips, T frames, 12 heads of 64 channels)
  probe_hbm_frac  its HBM bound over probe_us: bytes the algorithm moves (frame K / V, probe q / k / v, ctx: 6 * B*T*d*4) at 8 TB/s

--launches adds, per case, the library recorder's event time per kernel class (stlt_prof_collect) of one forward and one forward_prefixes
call, in a pass of its own after the timings (the recorder's two events per launch overstate the sums): which launches carry the
difference.

Every figure is the median over --repeats windows of device-event time around --iters back-to-back calls, after --warmup calls of the
same shape.  Needs a GPU: there is no fallback."""
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
CASES = (("cfg2", 64), ("cfg2", 1024), ("refdef", 64))


def timed_ms(fn, torch, warmup, iters, repeats):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(iters):
            fn()
        e1.record()
        e1.synchronize()
        out.append(e0.elapsed_time(e1) / iters)
    return statistics.median(out), min(out), max(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--launches", action="store_true", help="per-kernel-class recorder times of forward and forward_prefixes")
    ap.add_argument("--cases", default=",".join(f"{n}:{b}" for n, b in CASES))
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_prefix.py needs a GPU")
    pkg = importlib.import_module(PKG)
    for case in a.cases.split(","):
        name, B = case.split(":")
        B = int(B)
        c = pkg.synth.CONFIGS[name]
        T, N, d, H = c["T"], c["N"], c["hidden_size"], c["num_attention_heads"]
        m = pkg.Stlt(pkg.StltModelConfig(**pkg.synth.model_kwargs(name)))
        m.load_state_dict(pkg.synth.make_state_dict({k: tuple(v.shape) for k, v in m.state_dict().items()}, seed=1234))
        m = m.train(False).to("cuda")
        batch = {k: v.to("cuda") for k, v in pkg.synth.make_batch(B, T, N, dataset=c["dataset"], seed=3).items()}
        cuts = [pkg.collate.prefix_batch(batch, t) for t in range(T)]
        with torch.no_grad():
            fwd = timed_ms(lambda: m(batch), torch, a.warmup, a.iters, a.repeats)
            pre = timed_ms(lambda: m.forward_prefixes(batch), torch, a.warmup, a.iters, a.repeats)

            def naive():
                for cb in cuts:
                    m(cb)

            nai = timed_ms(naive, torch, 1, max(1, a.iters // 5), a.repeats)
            # agreement at the size that is timed: the full-clip prefix against the forward
            out = m.forward_prefixes(batch)["stlt"]
            err = (out[torch.arange(B, device="cuda"), batch["lengths"] - 1] - m(batch)["stlt"]).abs().max().item()
        g = torch.Generator().manual_seed(1)
        qf = ((torch.rand(B, T, 3 * d, generator=g) * 2 - 1) * 1.5).to("cuda")
        qp = ((torch.rand(B, T, 3 * d, generator=g) * 2 - 1) * 1.5).to("cuda")
        kpm = batch["src_key_padding_mask_frames"]
        probe = timed_ms(lambda: pkg.ops.attn_prefix_probe(qf, qp, kpm, H), torch, a.warmup, a.iters * 4, a.repeats)
        probe_bytes = 6.0 * B * T * d * 4 + B * T
        bound_us = probe_bytes / HBM_BYTES_PER_S * 1e6
        print(json.dumps(dict(config=name, clips=B, T=T, N=N, forward_ms=round(fwd[0], 4), forward_ms_range=[round(fwd[1], 4), round(fwd[2], 4)],
                              prefixes_ms=round(pre[0], 4), prefixes_ms_range=[round(pre[1], 4), round(pre[2], 4)], ratio=round(pre[0] / fwd[0], 3),
                              naive_ms=round(nai[0], 3), naive_over_prefixes=round(nai[0] / pre[0], 2), probe_us=round(probe[0] * 1e3, 2),
                              probe_bytes=int(probe_bytes), probe_hbm_bound_us=round(bound_us, 2), probe_hbm_frac=round(bound_us / (probe[0] * 1e3), 3),
                              full_prefix_vs_forward_max_abs=err, device=torch.cuda.get_device_name(0))), flush=True)
        if a.launches:
            rec = {}
            for what, fn in (("forward", lambda: m(batch)), ("prefixes", lambda: m.forward_prefixes(batch))):
                torch.cuda.synchronize()
                pkg.ops.prof_enable(True)
                pkg.ops.prof_collect()
                with torch.no_grad():
                    for _ in range(a.iters):
                        fn()
                torch.cuda.synchronize()
                got = pkg.ops.prof_collect()
                pkg.ops.prof_enable(False)
                rec[what] = {k: [round(ms / a.iters, 4), int(n // a.iters)] for k, (ms, n) in got.items() if n}
            print(json.dumps(dict(config=name, clips=B, launches_ms_and_count=rec)), flush=True)
        del m, batch, cuts, qf, qp
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
