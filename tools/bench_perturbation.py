#!/usr/bin/env python3
"""Perturbation-test benchmark (profiles/perturbation_bench.md).  Seeded synthetic inputs, closed-form weights; one JSON line per part.

At cfg2, 64 clips, steps = 10, both orders:

1. part "launches": inside Stlt.forward_perturbed, the library's recorder (one event pair around each launch): the stlt_perturb_rank,
   stlt_perturb_apply and stlt_perturb_curve launches in us, median over --iters recorded calls, and their sum.
2. part "model": the whole forward_perturbed beside `forward` alone on the same S*B perturbed clips (collate.perturb_batch made once, outside
   the timed window), in the same run, their windows alternating: what the three launches (and the curve's torch epilogue) add on top of
   the forwards.  Median over --repeats windows of device-event time around --iters back-to-back calls, after --warmup calls.
3. part "areas": for the trained checkpoint fixture tests/golden/ckpt_trained_nano.npz on its validation batches, the areas under the
   probability and accuracy curves of infer.run_perturbation_test for the four methods (relevance, saliency, attention, random), both
   orders.  An illustration on a toy task, not a test.

Needs a GPU: there is no fallback."""
import argparse
import importlib
import json
import os
import statistics
import sys

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = "revisiting-spatial-temporal-layouts_amd"


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


def launch_us(pkg, torch, call, iters):
    """{rank, apply, curve: median us of the launch inside one call}"""
    pkg.ops.prof_enable(True)
    pkg.ops.prof_launches()
    runs = {"perturb_rank": [], "perturb_apply": [], "perturb_curve": []}
    for _ in range(iters):
        call()
        torch.cuda.synchronize()
        seen = {k: 0.0 for k in runs}
        for r in pkg.ops.prof_launches():
            for k in runs:
                if r["kernel"] == "misc" and r["note"].startswith(k):
                    seen[k] += r["us"]
        for k in runs:
            runs[k].append(seen[k])
    pkg.ops.prof_enable(False)
    return {k: round(statistics.median(v), 2) for k, v in runs.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--config", default="cfg2")
    ap.add_argument("--clips", type=int, default=64)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--parts", default="launches,model,areas")
    a = ap.parse_args()
    sys.path.insert(0, HERE)
    import numpy as np
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_perturbation.py needs a GPU")
    pkg = importlib.import_module(PKG)
    dev_name = torch.cuda.get_device_name(0)
    parts = a.parts.split(",")
    if "launches" in parts or "model" in parts:
        name, B, steps = a.config, a.clips, a.steps
        c = pkg.synth.CONFIGS[name]
        m = pkg.Stlt(pkg.StltModelConfig(**pkg.synth.model_kwargs(name)))
        m.load_state_dict(pkg.synth.make_state_dict({k: tuple(v.shape) for k, v in m.state_dict().items()}, seed=1234))
        m = m.train(False).to("cuda")
        batch = {k: v.to("cuda") for k, v in pkg.synth.make_batch(B, c["T"], c["N"], dataset=c["dataset"], seed=3).items()}
        scores = torch.rand(B, c["T"], c["N"], generator=torch.Generator().manual_seed(5)).to("cuda")
        for order in ("descending", "ascending"):
            run = lambda: m.forward_perturbed(batch, scores, steps=steps, order=order, dataset_name=c["dataset"])  # noqa: E731
            if "launches" in parts:
                run()
                us = launch_us(pkg, torch, run, max(3, a.iters))
                print(json.dumps(dict(part="launches", config=name, clips=B, steps=steps, order=order, **{k + "_us": v for k, v in us.items()},
                                      sum_us=round(sum(us.values()), 2), device=dev_name)), flush=True)
            if "model" in parts:
                pb = pkg.collate.perturb_batch(batch, scores, steps=steps, order=order, dataset_name=c["dataset"])
                with torch.no_grad():
                    fns = {"forward_perturbed": run, "forward_alone": lambda: m(pb)}
                    med, rng = alternating_ms(fns, torch, a.warmup, a.iters, a.repeats)
                print(json.dumps(dict(part="model", config=name, clips=B, steps=steps, order=order, perturbed_clips=(steps + 1) * B,
                                      forward_perturbed_ms=round(med["forward_perturbed"], 4), forward_alone_ms=round(med["forward_alone"], 4),
                                      difference_ms=round(med["forward_perturbed"] - med["forward_alone"], 4), ranges_ms=rng, iters=a.iters, repeats=a.repeats,
                                      device=dev_name)), flush=True)
        del m, batch
        torch.cuda.empty_cache()
    if "areas" in parts:
        z = np.load(os.path.join(HERE, "tests", "golden", "ckpt_trained_nano.npz"))
        sd = {k: torch.from_numpy(z[k]) for k in z.files if not k.startswith("__")}
        m = pkg.Stlt(pkg.StltModelConfig(**pkg.synth.model_kwargs("nano")))
        m.load_state_dict(sd, strict=True)
        m = m.train(False).to("cuda")
        val = [pkg.synth.fit_batch("val", 0, i) for i in range(pkg.synth.FIT_TASK["val_batches"])]
        for method in ("relevance", "saliency", "attention", "random"):
            res = pkg.infer.run_perturbation_test(m, val, method=method, steps=a.steps, target="top1")
            print(json.dumps(dict(part="areas", model="ckpt_trained_nano", method=method, steps=a.steps, clips=res["descending"]["num_clips"],
                                  **{f"{o}_{k}": round(res[o][k], 4) for o in ("descending", "ascending") for k in ("auc_prob", "auc_accuracy")})), flush=True)


if __name__ == "__main__":
    main()
