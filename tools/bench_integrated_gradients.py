#!/usr/bin/env python3
"""Benchmark of integrated gradients; writes profiles/integrated_gradients_bench.md (and one JSON line per part).  Seeded synthetic inputs
and weights.  Nothing here is asserted anywhere: these are the numbers nobody had measured.

1. part "kernels": device events around --iters back-to-back calls, medians of alternating windows after a warm-up.
   stlt_ig_path_dense on 16 clips of 3 x 32 x 112 x 112 at steps = 10 (all 11 steps in one call) beside stlt_perturb_apply_cells on the same
   video and step count — the same read-once, write-every-step pattern at equal bytes written — and beside the torch construction of the same
   path; stlt_ig_path on the cfg2 layout at 64 clips and steps = 16; stlt_ig_reduce and stlt_ig_delta on the video's shape.  Each as a
   fraction of the HBM bound of its own traffic (6.3 TB/s achievable: MI355X_MICROARCH.md).
2. part "call": forward_integrated_gradients at steps = 16 — Stlt cfg2 at 64 clips (all 17 steps in one pass) and Resnet3D at 16 clips (one
   step per pass) — beside the same work done the way the tree before this one could: torch interpolation, forward_saliency per pass, a
   torch accumulation; and, with the library's recorder on, the microseconds of the new launches inside the call.
3. part "completeness": |delta| of the fp64 oracle and of the GPU at steps 4, 16 and 64 on cfg1 (4 clips, zero baseline, top-1 target).

Needs a GPU: there is no fallback."""
import argparse
import importlib
import json
import os
import statistics
import sys

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = "revisiting-spatial-temporal-layouts_amd"
HBM_BYTES_PER_S = 6.3e12
CELL = (16, 32, 32)
NEW = ("ig_path", "ig_path_dense", "ig_reduce", "ig_delta", "cell_pool_sum")


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


def recorded_us(pkg, torch, call):
    """{launch: us summed inside one call, count} of the new launches"""
    pkg.ops.prof_enable(True)
    pkg.ops.prof_launches()
    call()
    torch.cuda.synchronize()
    seen = {k: [0.0, 0] for k in NEW}
    for r in pkg.ops.prof_launches():
        for k in NEW:
            if r["kernel"] == "misc" and r["note"].startswith(k + " "):
                seen[k][0] += r["us"]
                seen[k][1] += 1
    pkg.ops.prof_enable(False)
    pkg.ops.prof_collect()
    return {k: [round(v[0], 2), v[1]] for k, v in seen.items()}


def torch_way(m, batch, moved, target, steps, per, torch):
    """The same quadrature without the new launches: torch interpolation, forward_saliency per pass, a torch accumulation"""
    B = target.shape[0]
    acc = {k: torch.zeros_like(batch[k]) for k in moved}
    hi = steps
    while hi >= 0:
        lo = max(hi - per + 1, 0)
        n = hi - lo + 1
        s = torch.arange(lo, hi + 1, device=target.device, dtype=torch.float32)
        part = {k: (v.repeat((n,) + (1,) * (v.dim() - 1)) if isinstance(v, torch.Tensor) else v) for k, v in batch.items()}
        for k in moved:
            x = batch[k]
            part[k] = ((s / steps).view((n,) + (1,) * x.dim()) * x[None]).reshape((n * B,) + tuple(x.shape[1:]))
        out = m.forward_saliency(part, target=target.repeat(n))
        w = torch.where((s == 0) | (s == steps), 0.5 / steps, 1.0 / steps)
        for k in moved:
            g = out[k + "_grad"]
            acc[k] += (w.view((n,) + (1,) * batch[k].dim()) * g.view((n, B) + tuple(g.shape[1:]))).sum(dim=0)
        hi = lo - 1
    return {k: batch[k] * acc[k] for k in moved}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--parts", default="kernels,call,completeness")
    ap.add_argument("--out", default=os.path.join(HERE, "profiles", "integrated_gradients_bench.md"))
    a = ap.parse_args()
    sys.path.insert(0, HERE)
    sys.path.insert(0, os.path.join(HERE, "tests"))
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_integrated_gradients.py needs a GPU")
    pkg = importlib.import_module(PKG)
    ops = pkg.ops
    dev_name = torch.cuda.get_device_name(0)
    parts = a.parts.split(",")
    lines = []

    def emit(**row):
        print(json.dumps(row), flush=True)
        lines.append(row)

    if "kernels" in parts:
        B, steps = 16, 10
        S = steps + 1
        video = pkg.synth.make_video(B, seed=17).to("cuda")
        grid = pkg.collate.appearance_cells({"video_frames": video})[2]
        C = grid[0] * grid[1] * grid[2]
        rank, n_cand = ops.perturb_rank_cells(torch.rand(B, C, generator=torch.Generator().manual_seed(5)).to("cuda"), True)
        out = torch.empty((S * B,) + tuple(video.shape[1:]), device="cuda")
        alphas = (torch.arange(S, device="cuda", dtype=torch.float32) / steps).view(S, 1, 1, 1, 1, 1)
        fns = {"ig_path_dense": lambda: ops.ig_path_dense(video, steps, 0, steps, out=out),
               "apply_cells": lambda: ops.perturb_apply_cells(video, CELL, rank, n_cand, steps, 0, steps, 0.0, out=out),
               "path_torch": lambda: (alphas * video[None]).view(out.shape)}
        med, rng = alternating_ms(fns, torch, a.warmup, a.iters, a.repeats)
        nbytes = (1 + S) * video.numel() * 4
        bound = nbytes / HBM_BYTES_PER_S * 1e3
        emit(part="kernels", what="dense", clips=B, steps=steps, video=list(video.shape[2:]), bytes=nbytes, hbm_bound_ms=round(bound, 4),
             **{n + "_ms": round(v, 4) for n, v in med.items()}, ranges_ms=rng, ig_path_dense_fraction=round(bound / med["ig_path_dense"], 3),
             apply_cells_fraction=round(bound / med["apply_cells"], 3), device=dev_name)
        del out
        grads = torch.randn((3 * B,) + tuple(video.shape[1:]), device="cuda")
        acc, attr = torch.empty_like(video), torch.empty_like(video)
        seed, lx, lx0 = (torch.randn(B, 174, device="cuda") for _ in range(3))
        scratch = torch.empty(B * 1024, device="cuda")
        fns = {"ig_reduce": lambda: ops.ig_reduce(grads, acc, steps, 0, 2, begin=True, finish=True, x=video, attr=attr),
               "ig_delta": lambda: ops.ig_delta([attr], seed, lx, lx0, scratch=scratch), "cell_pool_sum": lambda: ops.cell_pool_sum(attr, CELL)}
        med, rng = alternating_ms(fns, torch, a.warmup, a.iters, a.repeats)
        one = video.numel() * 4
        emit(part="kernels", what="reduce", clips=B, steps_in_call=3, **{n + "_ms": round(v, 4) for n, v in med.items()}, ranges_ms=rng,
             ig_reduce_fraction=round(6 * one / HBM_BYTES_PER_S * 1e3 / med["ig_reduce"], 3), ig_delta_fraction=round(one / HBM_BYTES_PER_S * 1e3 / med["ig_delta"], 3),
             cell_pool_sum_fraction=round(one / HBM_BYTES_PER_S * 1e3 / med["cell_pool_sum"], 3), device=dev_name)
        del grads, acc, attr, video
        torch.cuda.empty_cache()
        c = pkg.synth.CONFIGS["cfg2"]
        Bl, st = 64, 16
        layout = {k: v.to("cuda") for k, v in pkg.synth.make_batch(Bl, c["T"], c["N"], seed=21, with_scores=True).items()}
        med, rng = alternating_ms({"ig_path": lambda: ops.ig_path(layout, st, 0, st)}, torch, a.warmup, a.iters, a.repeats)
        slots = Bl * c["T"] * c["N"]
        nbytes = slots * (8 + 16 + 4 + 1) * (1 + st + 1)
        emit(part="kernels", what="layout", clips=Bl, steps=st, T=c["T"], N=c["N"], bytes=nbytes, ig_path_ms=round(med["ig_path"], 4), ranges_ms=rng,
             hbm_bound_ms=round(nbytes / HBM_BYTES_PER_S * 1e3, 5), ig_path_fraction=round(nbytes / HBM_BYTES_PER_S * 1e3 / med["ig_path"], 4),
             note="includes the wrapper's seven output allocations", device=dev_name)
    if "call" in parts:
        steps = 16
        c = pkg.synth.CONFIGS["cfg2"]
        m = pkg.Stlt(pkg.StltModelConfig(**pkg.synth.model_kwargs("cfg2")))
        m.load_state_dict(pkg.synth.make_state_dict({k: tuple(v.shape) for k, v in m.state_dict().items()}, seed=31, gain=1.5))
        m.train(False).to("cuda")
        batch = {k: v.to("cuda") for k, v in pkg.synth.make_batch(64, c["T"], c["N"], seed=21, with_scores=True).items()}
        cases = [("Stlt cfg2", m, batch, ("boxes", "scores"), 64, steps + 1)]
        kw = pkg.synth.model_kwargs("cfg1")
        r3 = pkg.Resnet3D(pkg.AppearanceModelConfig(num_classes=kw["num_classes"], hidden_size=kw["hidden_size"], num_attention_heads=kw["num_attention_heads"],
                                                    hidden_dropout_prob=0.0, appearance_num_frames=4))
        r3.load_state_dict(pkg.synth.make_r3d_state_dict({k: tuple(v.shape) for k, v in r3.state_dict().items()}, seed=4242), strict=True)
        r3.train(False).to("cuda")
        cases.append(("Resnet3D", r3, {"video_frames": pkg.synth.make_video(16, seed=17).to("cuda")}, ("video_frames",), 16, 1))
        for name, model, b, moved, clips, per in cases:
            tgt = model.forward_integrated_gradients(b, steps=steps, steps_per_pass=per)["target"]
            fns = {"call": lambda: model.forward_integrated_gradients(b, target=tgt, steps=steps, steps_per_pass=per),
                   "torch_way": lambda: torch_way(model, b, moved, tgt, steps, per, torch)}
            ours, theirs = fns["call"](), fns["torch_way"]()
            agree = max(((ours[k + "_attribution"] - theirs[k]).abs().max() / theirs[k].abs().max()).item() for k in moved)
            us = recorded_us(pkg, torch, fns["call"])
            med, rng = alternating_ms(fns, torch, 1, 2 if name == "Resnet3D" else a.iters, a.repeats if name != "Resnet3D" else 3)
            emit(part="call", model=name, clips=clips, steps=steps, steps_per_pass=per, call_ms=round(med["call"], 3), torch_way_ms=round(med["torch_way"], 3), ranges_ms=rng,
                 torch_way_over_call=round(med["torch_way"] / med["call"], 3), new_launches_us=us, new_launches_total_us=round(sum(v[0] for v in us.values()), 2),
                 share_of_call=round(sum(v[0] for v in us.values()) / 1e3 / med["call"], 5), max_rel_diff_to_torch_way=float(f"{agree:.3g}"), device=dev_name)
        del r3, cases
        torch.cuda.empty_cache()
    if "completeness" in parts:
        import ig_cases as IC
        import ig_restated as R
        name, B = IC.CASES[0]
        c, sd, batch = IC.layout_case(name, B)
        m = pkg.Stlt(pkg.StltModelConfig(**pkg.synth.model_kwargs(name)))
        m.load_state_dict(sd)
        m.train(False).to("cuda")
        dev = {k: v.to("cuda") for k, v in batch.items()}
        for steps in (4, 16, 64):
            r = m.forward_integrated_gradients(dev, steps=steps)
            seed = torch.nn.functional.one_hot(r["target"].cpu(), c["num_classes"]).double()
            ref = R.stlt_ig(sd, batch, c["num_attention_heads"], seed, steps)
            gap = (seed * (ref["logits_x"] - ref["logits_x0"])).sum(dim=1)
            emit(part="completeness", config=name, clips=B, steps=steps, gpu_abs_delta=[float(f"{v:.4g}") for v in r["delta"].abs().tolist()],
                 oracle_abs_delta=[float(f"{v:.4g}") for v in ref["delta"].abs().tolist()], logit_gap=[float(f"{v:.4g}") for v in gap.tolist()], device=dev_name)
    write_markdown(a.out, lines, dev_name)


def write_markdown(path, rows, dev_name):
    out = ["# Integrated gradients: measurements", "",
           f"Written by `tools/bench_integrated_gradients.py` on {dev_name}.  Seeded inputs and weights; device-event times, medians of alternating windows.  "
           "Nothing here is asserted by a test.", ""]
    for r in (r for r in rows if r["part"] == "kernels" and r["what"] == "dense"):
        T, H, W = r["video"]
        out += [f"## The path kernels ({r['clips']} clips of 3 x {T} x {H} x {W}, steps = {r['steps']}: all {r['steps'] + 1} steps in one call)", "",
                "| launch | median ms | min .. max ms | fraction of the HBM bound |", "|---|---|---|---|"]
        for n, frac in (("ig_path_dense", r["ig_path_dense_fraction"]), ("apply_cells", r["apply_cells_fraction"]), ("path_torch", None)):
            out.append(f"| {n} | {r[n + '_ms']} | {r['ranges_ms'][n][0]} .. {r['ranges_ms'][n][1]} | {'' if frac is None else f'{100 * frac:.0f} %'} |")
        out += ["", f"Both kernels move {r['bytes'] / 1e6:.0f} MB (the input read once, {r['steps'] + 1} steps written; HBM bound at 6.3 TB/s: {r['hbm_bound_ms']} ms).  "
                "`apply_cells` is stlt_perturb_apply_cells on the same video and step count; `path_torch` is one broadcast multiply writing the same batch "
                "(zero baseline).", ""]
    for r in (r for r in rows if r["part"] == "kernels" and r["what"] == "layout"):
        out += [f"`stlt_ig_path` on the cfg2 layout ({r['clips']} clips, T = {r['T']}, N = {r['N']}, steps = {r['steps']}, through `ops.ig_path`, which also allocates the seven "
                f"outputs): {r['ig_path_ms']} ms for {r['bytes'] / 1e6:.1f} MB — {100 * r['ig_path_fraction']:.1f} % of the HBM bound ({r['hbm_bound_ms']} ms): at this size the call "
                "is launch and allocation time, not bandwidth.", ""]
    for r in (r for r in rows if r["part"] == "kernels" and r["what"] == "reduce"):
        out += [f"## The reduction kernels ({r['clips']} clips of the same video)", "", "| launch | median ms | min .. max ms | fraction of the HBM bound |", "|---|---|---|---|"]
        for n in ("ig_reduce", "ig_delta", "cell_pool_sum"):
            out.append(f"| {n} | {r[n + '_ms']} | {r['ranges_ms'][n][0]} .. {r['ranges_ms'][n][1]} | {100 * r[n + '_fraction']:.0f} % |")
        out += ["", f"`ig_reduce`: {r['steps_in_call']} steps in one finishing call (three gradient reads, the input read, acc and attr written: six tensors' worth); "
                "`ig_delta` and `cell_pool_sum` read the attribution once.", ""]
    call_rows = [r for r in rows if r["part"] == "call"]
    if call_rows:
        out += ["## The whole call at steps = 16", "",
                "| model | clips | steps per pass | forward_integrated_gradients ms | torch way ms | torch way / call | new launches us (count) | share of the call |",
                "|---|---|---|---|---|---|---|---|"]
        for r in call_rows:
            new = ", ".join(f"{k} {v[0]} ({v[1]})" for k, v in r["new_launches_us"].items() if v[1])
            out.append(f"| {r['model']} | {r['clips']} | {r['steps_per_pass']} | {r['call_ms']} | {r['torch_way_ms']} | {r['torch_way_over_call']} | {new} | "
                       f"{100 * r['share_of_call']:.2f} % |")
        out += ["", "The torch way is what the tree before this one could do: torch interpolation, `forward_saliency` per pass, a torch accumulation (same passes, same target; "
                "largest relative difference of the attributions: " + ", ".join(f"{r['model']} {r['max_rel_diff_to_torch_way']}" for r in call_rows) + ").", ""]
    comp = [r for r in rows if r["part"] == "completeness"]
    if comp:
        out += [f"## Completeness on {comp[0]['config']} ({comp[0]['clips']} clips, zero baseline, top-1 target)", "",
                "| steps | GPU abs(delta) per clip | fp64 oracle abs(delta) per clip | logit(x) - logit(x0) per clip |", "|---|---|---|---|"]
        for r in comp:
            out.append(f"| {r['steps']} | {r['gpu_abs_delta']} | {r['oracle_abs_delta']} | {r['logit_gap']} |")
        out.append("")
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "w") as f:
        f.write("\n".join(out))


if __name__ == "__main__":
    main()
