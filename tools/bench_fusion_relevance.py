#!/usr/bin/env python3
"""Fusion-model attention-relevance benchmark (profiles/fusion_relevance_bench.md).  Seeded synthetic inputs, closed-form weights; one JSON
line per case.

  --build   (no GPU needed) build the two A/B variants of the library into build/variants/: the cross grad-probs launcher sending every
            shape to the vector-ALU kernel (csrc/attn_grad_probs.hip with -DSTLT_GRAD_PROBS_CROSS_NO_MFMA), and sending every MFMA
            shape to the MFMA kernel however few its work units (-DSTLT_GRAD_PROBS_CROSS_ALL_MFMA); run it before the measurement.

1. part "kernel": the cross grad-probs launch (stlt_attn_grad_probs_cross) against the cross-attention backward (stlt_attn_bwd) on the same
   buffers — queries and dctx (S,Lq,d), packed keys / values (S,Lk,2d), 12 heads of 64 channels, about 30 % of the keys masked — at the
   fusion blocks' shapes in both directions, T = 16, 32, 64 against A = 33, and the self blocks (T,T) causal and (33,33), at 64 clips:
   grad_probs_us (the library as routed), attn_bwd_us, and generic_us / mfma_us / mfma_over_generic from the variant libraries when they
   have been built — the figures the launcher's routing rule rests on.
2. part "joint": stlt_attn_rollout_joint and stlt_relevance_combine_joint at T = 16, 32, 64, A = 33, 4 fusion layers, 64 clips, in us.
3. part "model": forward_relevance against forward_saliency of the same model (the comparable existing call), CAF / CACNF / LCF at cfg2's
   layout shapes (d = 768, 12 heads, T = 32, N = 7, 33 appearance tokens), 64 clips, their windows alternating, ms per call.
4. part "launches": inside one forward_relevance call, the library's recorder: every grad-probs launch of the fusion blocks and the
   appearance encoder next to the attention-backward launch it precedes, the rollouts and the read-out, in us (medians over recorded calls).

Every time in parts 1-3 is the median over --repeats windows of device-event time around --iters back-to-back calls, after --warmup calls
of the same shape.  Needs a GPU: there is no fallback."""
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
VARIANTS = {"generic": ("grad_probs_cross_generic", "-DSTLT_GRAD_PROBS_CROSS_NO_MFMA=1"), "mfma": ("grad_probs_cross_all_mfma", "-DSTLT_GRAD_PROBS_CROSS_ALL_MFMA=1")}
# (Lq, Lk, causal): layout -> appearance, appearance -> layout, layout_attn, and the appearance self blocks
SHAPES = ((16, 33, 0), (33, 16, 0), (32, 33, 0), (33, 32, 0), (64, 33, 0), (33, 64, 0), (16, 16, 1), (32, 32, 1), (64, 64, 1), (33, 33, 0))
CLIPS = 64


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


def launch_table(pkg, torch, call, iters):
    """Per-launch medians (us) of one forward_relevance call: [(grad-probs note, its us, the us of the attention backward behind it)], and
    the rollouts and read-outs"""
    pkg.ops.prof_enable(True)
    pkg.ops.prof_launches()
    runs = []
    for _ in range(iters):
        call()
        torch.cuda.synchronize()
        recs = pkg.ops.prof_launches()
        pairs, extra = [], []
        for i, r in enumerate(recs):
            if r["kernel"] == "attn_probs" and r["note"].startswith("attn_grad_probs"):
                nxt = next((q for q in recs[i + 1:] if q["kernel"] in ("attn_bwd", "attn_probs")), None)
                pairs.append((r["note"], r["us"], nxt["us"] if nxt is not None and nxt["kernel"] == "attn_bwd" else None))
            elif r["kernel"] == "misc" and r["note"].startswith(("attn_rollout", "relevance_combine")):
                extra.append((r["note"], r["us"]))
        runs.append((pairs, extra))
    pkg.ops.prof_enable(False)
    pairs0, extra0 = runs[0]
    med = lambda vals: None if any(v is None for v in vals) else round(statistics.median(vals), 2)  # noqa: E731
    table = [dict(launch=note, grad_probs_us=med([r[0][i][1] for r in runs]), attn_bwd_us=med([r[0][i][2] for r in runs])) for i, (note, _, _) in enumerate(pairs0)]
    tail = [dict(launch=note, us=med([r[1][i][1] for r in runs])) for i, (note, _) in enumerate(extra0)]
    return table, tail, round(sum(t["grad_probs_us"] for t in table) + sum(t["us"] for t in tail), 2)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--build", action="store_true")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--skip-model", action="store_true")
    a = ap.parse_args()
    if a.build:
        builder = importlib.import_module(PKG + ".build")
        for tag, flag in VARIANTS.values():
            print(builder.variant(tag, {"attn_grad_probs.hip": [flag]}))
        return
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_fusion_relevance.py needs a GPU")
    pkg = importlib.import_module(PKG)
    lib = pkg._lib.load()
    dev_name = torch.cuda.get_device_name(0)
    stream = lambda: torch.cuda.current_stream().cuda_stream  # noqa: E731
    variants = {}
    for name, (tag, _) in VARIANTS.items():
        path = os.path.join(ROOT, "build", "variants", f"libstlt_hip_{tag}.so")
        if os.path.exists(path):
            variants[name] = C.CDLL(path).stlt_attn_grad_probs_cross
            variants[name].restype, variants[name].argtypes = pkg._lib.SIGNATURES["stlt_attn_grad_probs_cross"]
    H, dh, S = 12, 64, CLIPS
    d = H * dh
    for Lq, Lk, causal in SHAPES:
        g = torch.Generator().manual_seed(1)
        q, dctx = (((torch.rand(S, Lq, d, generator=g) * 2 - 1) * 1.5).to("cuda") for _ in range(2))
        kv = ((torch.rand(S, Lk, 2 * d, generator=g) * 2 - 1) * 1.5).to("cuda")
        kpm = torch.rand(S, Lk, generator=g) < 0.3
        kpm[:, 0] = False
        kpm = kpm.to(torch.uint8).to("cuda")
        abar, outs = torch.empty(S, Lq, Lk, device="cuda"), {name: torch.empty(S, Lq, Lk, device="cuda") for name in variants}
        dq, dkv = torch.empty_like(q), torch.empty_like(kv)

        def grad_probs(f, out):
            rc = f(q.data_ptr(), d, kv.data_ptr(), kv.data_ptr() + 4 * d, 2 * d, dctx.data_ptr(), kpm.data_ptr(), causal, S, Lq, Lk, H, dh, out.data_ptr(), stream())
            assert rc == 0, lib.stlt_last_error()

        def attn_bwd():
            rc = lib.stlt_attn_bwd(q.data_ptr(), d, kv.data_ptr(), kv.data_ptr() + 4 * d, 2 * d, dctx.data_ptr(), kpm.data_ptr(), causal, S, Lq, Lk, H, dh, 0.0, 0, 0,
                                   dq.data_ptr(), d, dkv.data_ptr(), dkv.data_ptr() + 4 * d, 2 * d, stream())
            assert rc == 0, lib.stlt_last_error()

        fns = {"grad_probs": lambda: grad_probs(lib.stlt_attn_grad_probs_cross, abar), "attn_bwd": attn_bwd}
        for name in variants:
            fns[name] = (lambda name: lambda: grad_probs(variants[name], outs[name]))(name)
        med, rng = alternating_ms(fns, torch, a.warmup, a.iters, a.repeats)
        rec = dict(part="kernel", Lq=Lq, Lk=Lk, causal=causal, clips=S, H=H, dh=dh, units=S * ((Lq + 15) // 16), grad_probs_us=round(med["grad_probs"] * 1e3, 2),
                   attn_bwd_us=round(med["attn_bwd"] * 1e3, 2), grad_probs_over_attn_bwd=round(med["grad_probs"] / med["attn_bwd"], 3))
        for name in variants:
            rec[name + "_us"] = round(med[name] * 1e3, 2)
        if len(variants) == 2:
            rec.update(mfma_over_generic=round(med["mfma"] / med["generic"], 3), routed_to="mfma" if torch.equal(abar, outs["mfma"]) else "generic",
                       mfma_vs_generic_max_abs=(outs["mfma"] - outs["generic"]).abs().max().item())
        rec.update(ranges_ms=rng, device=dev_name)
        print(json.dumps(rec), flush=True)
    A, n = 33, 4
    for T in (16, 32, 64):
        g = torch.Generator().manual_seed(2)
        J = T + A
        rnd = lambda *s: (torch.rand(*s, generator=g) / J).to("cuda")  # noqa: E731
        maps = (rnd(n, S, T, A), rnd(n, S, A, T), rnd(n, S, T, T), rnd(n, 2, S, A, A))
        r_tp, r_app, r_sp = rnd(S, T, T), rnd(S, A, A), rnd(S, T, 7, 7)
        lengths = torch.full((S,), T, dtype=torch.int64, device="cuda")
        R = pkg.ops.attn_rollout_joint(r_tp, r_app, *maps)
        fns = {"rollout_joint": lambda: pkg.ops.attn_rollout_joint(r_tp, r_app, *maps), "combine_joint": lambda: pkg.ops.relevance_combine_joint(R, r_sp, lengths, 1.0, 1.0)}
        med, rng = alternating_ms(fns, torch, a.warmup, a.iters, a.repeats)
        print(json.dumps(dict(part="joint", T=T, A=A, layers=n, clips=S, rollout_joint_us=round(med["rollout_joint"] * 1e3, 2),
                              combine_joint_us=round(med["combine_joint"] * 1e3, 2), ranges_ms=rng, note="wrapper calls: each allocates its outputs", device=dev_name)), flush=True)
    if a.skip_model:
        return
    c = pkg.synth.CONFIGS["cfg2"]
    for name in ("caf", "cacnf", "lcf"):
        m = pkg.models_factory[name](pkg.MultimodalModelConfig(**dict(pkg.synth.model_kwargs("cfg2"), appearance_num_frames=32)))
        m.load_state_dict(pkg.synth.make_state_dict({k: tuple(v.shape) for k, v in m.state_dict().items()}, seed=1234))
        m = m.train(False).to("cuda")
        batch = pkg.synth.make_batch(S, c["T"], c["N"], dataset=c["dataset"], seed=3)
        batch["appearance_features"] = pkg.synth.make_appearance_features(S, seed=4)
        batch = {k: v.to("cuda") for k, v in batch.items()}
        fns = {"saliency": lambda: m.forward_saliency(batch), "relevance": lambda: m.forward_relevance(batch)}
        it = max(2, a.iters // 10)
        med, rng = alternating_ms(fns, torch, max(2, a.warmup // 2), it, a.repeats)
        print(json.dumps(dict(part="model", model=name, config="cfg2", clips=S, T=c["T"], N=c["N"], saliency_ms=round(med["saliency"], 4),
                              relevance_ms=round(med["relevance"], 4), relevance_over_saliency=round(med["relevance"] / med["saliency"], 3), ranges_ms=rng, iters=it,
                              repeats=a.repeats, device=dev_name)), flush=True)
        table, tail, new_us = launch_table(pkg, torch, fns["relevance"], max(3, it // 2))
        print(json.dumps(dict(part="launches", model=name, config="cfg2", clips=S, blocks=table, rollouts_and_read_out=tail, new_launches_us=new_us)), flush=True)
        del m, batch
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
