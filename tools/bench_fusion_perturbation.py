#!/usr/bin/env python3
"""Benchmark of the appearance side of the perturbation test; writes profiles/fusion_perturbation_bench.md (and one JSON line per part).
Seeded synthetic inputs and weights (synth.make_video, synth.make_r3d_state_dict).  At the reference's sizes: video 32 x 112 x 112,
16 clips, 10 steps.

1. part "kernels": the three launches alone, device events around --iters back-to-back calls, median over --repeats windows after a
   warm-up: stlt_perturb_rank_cells; stlt_perturb_apply_cells for all S = steps+1 steps in one call, beside a plain torch construction of
   the same S*B clips (a gathered cell mask and torch.where — it uses torch alone, so it is what the parent commit's tree could do), the
   windows alternating, and as a fraction of the HBM bound of its own traffic (B*X floats read, S*B*X written, 6.3 TB/s achievable:
   MI355X_MICROARCH.md); stlt_cell_pool_abs on a gradient of the video's shape.  The two constructions are compared bit for bit first.
2. part "model": TransformerResnet.forward_perturbed and CACNF.forward_perturbed (modality "appearance", one step per pass: S forwards on
   16 clips) with the library's recorder on: the microseconds of the new launches inside the call, and in a second, unrecorded run the
   call's device time; their ratio is the share.
3. part "areas": infer.run_perturbation_test, 4 clips, for relevance / saliency / attention / random and every modality of CACNF and the
   appearance side of TransformerResnet.  The weights are seeded, not trained (no fusion checkpoint fixture exists): the areas show that
   the instrument runs end to end and say nothing about the faithfulness of any map.

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


def recorded_us(pkg, torch, call, iters, prefixes):
    """{prefix: median us of the launches whose note starts with it, summed inside one call}"""
    pkg.ops.prof_enable(True)
    pkg.ops.prof_launches()
    runs = {k: [] for k in prefixes}
    for _ in range(iters):
        call()
        torch.cuda.synchronize()
        seen = {k: 0.0 for k in prefixes}
        for r in pkg.ops.prof_launches():
            for k in prefixes:
                if r["kernel"] == "misc" and r["note"].startswith(k + " "):
                    seen[k] += r["us"]
        for k in prefixes:
            runs[k].append(seen[k])
    pkg.ops.prof_enable(False)
    return {k: round(statistics.median(v), 2) for k, v in runs.items()}


def build_models(pkg, torch, frames):
    kw = pkg.synth.model_kwargs("cfg1")
    app = dict(num_classes=kw["num_classes"], hidden_size=kw["hidden_size"], num_attention_heads=kw["num_attention_heads"], hidden_dropout_prob=0.0,
               appearance_num_frames=frames)
    tr = pkg.TransformerResnet(pkg.AppearanceModelConfig(**app))
    mm = pkg.CrossAttentionCentralNetFusion(pkg.MultimodalModelConfig(**dict(kw, appearance_num_frames=frames, num_appearance_layers=2, num_fusion_layers=2,
                                                                             appearance_trunk=True)))
    for m in (tr, mm):
        m.load_state_dict(pkg.synth.make_r3d_state_dict({k: tuple(v.shape) for k, v in m.state_dict().items()}, seed=4242), strict=True)
        m.train(False).to("cuda")
    return {"TransformerResnet": tr, "CACNF": mm}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--clips", type=int, default=16)
    ap.add_argument("--area-clips", type=int, default=4)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--parts", default="kernels,model,areas")
    ap.add_argument("--out", default=os.path.join(HERE, "profiles", "fusion_perturbation_bench.md"))
    a = ap.parse_args()
    sys.path.insert(0, HERE)
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_fusion_perturbation.py needs a GPU")
    pkg = importlib.import_module(PKG)
    dev_name = torch.cuda.get_device_name(0)
    parts = a.parts.split(",")
    B, steps = a.clips, a.steps
    S = steps + 1
    video = pkg.synth.make_video(B, seed=17).to("cuda")
    _, _, T, H, W = video.shape
    grid = pkg.collate.appearance_cells({"video_frames": video})[2]
    C = grid[0] * grid[1] * grid[2]
    scores = torch.rand(B, C, generator=torch.Generator().manual_seed(5)).to("cuda")
    lines = []

    def emit(**row):
        print(json.dumps(row), flush=True)
        lines.append(row)

    if "kernels" in parts:
        rank, n_cand = pkg.ops.perturb_rank_cells(scores, True)
        out = torch.empty(S * B, 3, T, H, W, device="cuda")
        removed = torch.empty(S, B, dtype=torch.int32, device="cuda")
        idx = pkg.collate.cell_index((T, H, W), CELL).to("cuda")
        k = (torch.arange(S, device="cuda")[:, None] * n_cand.long()[None, :]) // steps
        zero = torch.zeros((), device="cuda")

        def with_torch():
            gone = rank.long()[None] < k[:, :, None]
            return torch.where(gone[:, :, idx][:, :, None], zero, video[None]).view(S * B, 3, T, H, W)

        kernel = lambda: pkg.ops.perturb_apply_cells(video, CELL, rank, n_cand, steps, 0, steps, 0.0, removed=removed, out=out)  # noqa: E731
        kernel()
        assert torch.equal(out.view(torch.int32), with_torch().view(torch.int32)), "the kernel and the torch construction differ"
        grad = torch.randn_like(video)
        fns = {"rank_cells": lambda: pkg.ops.perturb_rank_cells(scores, True), "apply_cells": kernel, "apply_torch": with_torch,
               "cell_pool_abs": lambda: pkg.ops.cell_pool_abs(grad, CELL)}
        med, rng = alternating_ms(fns, torch, a.warmup, a.iters, a.repeats)
        nbytes = (1 + S) * video.numel() * 4
        bound_ms = nbytes / HBM_BYTES_PER_S * 1e3
        emit(part="kernels", clips=B, steps=steps, video=[T, H, W], cells=C, **{f"{n}_ms": round(v, 4) for n, v in med.items()}, ranges_ms=rng, apply_bytes=nbytes,
             apply_hbm_bound_ms=round(bound_ms, 4), apply_fraction_of_hbm_bound=round(bound_ms / med["apply_cells"], 3),
             pool_fraction_of_hbm_bound=round(video.numel() * 4 / HBM_BYTES_PER_S * 1e3 / med["cell_pool_abs"], 3),
             torch_over_kernel=round(med["apply_torch"] / med["apply_cells"], 2), iters=a.iters, repeats=a.repeats, device=dev_name)
        del out, grad
        torch.cuda.empty_cache()
    models = build_models(pkg, torch, C) if ("model" in parts or "areas" in parts) else {}
    c = pkg.synth.CONFIGS["cfg1"]
    if "model" in parts:
        layout = {k: v.to("cuda") for k, v in pkg.synth.make_batch(B, c["T"], c["N"], seed=21).items()}
        for name, m in models.items():
            batch = dict(layout, video_frames=video) if name == "CACNF" else {"video_frames": video}
            run = lambda: m.forward_perturbed(batch, scores, steps=steps, steps_per_pass=1)  # noqa: E731
            for _ in range(a.warmup):
                run()
            us = recorded_us(pkg, torch, run, 3, ("perturb_rank_cells", "perturb_apply_cells", "perturb_curve"))
            med, rng = alternating_ms({"forward_perturbed": run}, torch, 1, 3, a.repeats)
            total = med["forward_perturbed"]
            emit(part="model", model=name, clips=B, steps=steps, steps_per_pass=1, **{n + "_us": v for n, v in us.items()}, new_launches_us=round(sum(us.values()), 2),
                 forward_perturbed_ms=round(total, 3), ranges_ms=rng, share_of_forward_perturbed=round(sum(us.values()) / 1e3 / total, 5), device=dev_name)
    if "areas" in parts:
        Ba = a.area_clips
        layout = {k: v.to("cuda") for k, v in pkg.synth.make_batch(Ba, c["T"], c["N"], seed=21).items()}
        for name, m in models.items():
            batch = dict(layout, video_frames=video[:Ba]) if name == "CACNF" else {"video_frames": video[:Ba]}
            for modality in (("appearance", "layout", "both") if name == "CACNF" else ("appearance",)):
                for method in ("relevance", "saliency", "attention", "random"):
                    res = pkg.infer.run_perturbation_test(m, [batch], method=method, steps=steps, modality=modality)
                    emit(part="areas", model=name, weights="seeded", modality=modality, method=method, steps=steps, clips=res["descending"]["num_clips"],
                         **{f"{o}_{q}": round(res[o][q], 4) for o in ("descending", "ascending") for q in ("auc_prob", "auc_accuracy")})
    write_markdown(a.out, lines, dev_name)


def write_markdown(path, rows, dev_name):
    out = ["# Appearance-side perturbation test: measurements", "",
           f"Written by `tools/bench_fusion_perturbation.py` on {dev_name}.  Seeded inputs and weights; device-event times, medians of alternating windows.", ""]
    for r in (r for r in rows if r["part"] == "kernels"):
        T, H, W = r["video"]
        out += [f"## The three launches alone ({r['clips']} clips of 3 x {T} x {H} x {W}, {r['cells']} cells, {r['steps']} steps)", "",
                "| launch | median ms | min .. max ms |", "|---|---|---|"]
        for n in ("rank_cells", "apply_cells", "apply_torch", "cell_pool_abs"):
            out.append(f"| {n} | {r[n + '_ms']} | {r['ranges_ms'][n][0]} .. {r['ranges_ms'][n][1]} |")
        out += ["", f"`apply_cells` moves {r['apply_bytes'] / 1e6:.0f} MB (the input read once, {r['steps'] + 1} steps written): the HBM bound at 6.3 TB/s is "
                f"{r['apply_hbm_bound_ms']} ms, the kernel reaches {100 * r['apply_fraction_of_hbm_bound']:.0f} % of it.  `apply_torch` is the same batch from a gathered "
                f"cell mask and `torch.where` (bit-identical output): {r['torch_over_kernel']} x the kernel's time.  `cell_pool_abs` reads the gradient once: "
                f"{100 * r['pool_fraction_of_hbm_bound']:.0f} % of its HBM bound.", ""]
    model_rows = [r for r in rows if r["part"] == "model"]
    if model_rows:
        out += ["## Inside forward_perturbed (modality appearance, one step per pass)", "",
                "| model | rank_cells us | apply_cells us (all passes) | curve us | forward_perturbed ms | share of the new launches |", "|---|---|---|---|---|---|"]
        for r in model_rows:
            out.append(f"| {r['model']} | {r['perturb_rank_cells_us']} | {r['perturb_apply_cells_us']} | {r['perturb_curve_us']} | {r['forward_perturbed_ms']} | "
                       f"{100 * r['share_of_forward_perturbed']:.2f} % |")
        out.append("")
    area_rows = [r for r in rows if r["part"] == "areas"]
    if area_rows:
        out += ["## Areas under the curves (seeded weights)", "",
                "The weights are seeded, not trained: these areas show the instrument running end to end and say nothing about the faithfulness of any map.", "",
                "| model | modality | method | descending auc_prob | ascending auc_prob | descending auc_accuracy | ascending auc_accuracy |", "|---|---|---|---|---|---|---|"]
        for r in area_rows:
            out.append(f"| {r['model']} | {r['modality']} | {r['method']} | {r['descending_auc_prob']} | {r['ascending_auc_prob']} | {r['descending_auc_accuracy']} | "
                       f"{r['ascending_auc_accuracy']} |")
        out.append("")
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "w") as f:
        f.write("\n".join(out))


if __name__ == "__main__":
    main()
