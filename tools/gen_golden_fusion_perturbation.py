#!/usr/bin/env python3
"""Generate the appearance-side perturbation fixtures tests/golden/fusion_perturbation_<model>.npz by importing the REFERENCE.

Run on the CPU, next to a checkout of the reference (first argument: its src/ directory; default a `reference` checkout beside this
repository).  The reference never travels to the GPU tests:

    PYTHONDONTWRITEBYTECODE=1 python tools/gen_golden_fusion_perturbation.py [reference/src]

For the reference's ``Resnet3D``, ``TransformerResnet`` and ``CrossAttentionCentralNetFusion`` (weights from synth.make_r3d_state_dict, the
video from synth.make_video, the layout from synth.make_batch — all rebuilt from the seeds in the schema, none stored) this builds the
perturbed batches with the restatements (tests/fusion_perturbation_restated.py for the video cells, tests/perturbation_restated.py for the
layout) from seeded scores that hold ties and both zeros, and runs the reference on every step's batch.  A deleted cell holds 0.0 —
mid-grey after the reference's Normalize(0.5, 0.5) (datasets.py:151) — so every batch is one the reference could have been handed.

The video is (2, 3, 32, 32, 64): the trunk's strides (16, 32, 32) give the grid 2 x 1 x 2 = 4 appearance tokens = ``appearance_num_frames``;
the tool asserts that the reference's own feature map has that many positions.  Stored per model and case (modality_order): ``logits_*``
(S,B,K) float32 per logit name, ``removed_*`` (S,B) and ``margin_*`` (S,B) float64 — the distance between the target's logit (the top-1
class of step 0, last logit name) and the best other class on a float64 run of the reference; plus ``scores_cells`` (B,C) and, for CACNF,
``scores_layout`` (B,T,N).  The tool asserts that everything is finite and that at most 5 % of a model's (step, clip) entries have a
margin below 1e-3 — the only entries the ``hit`` comparison of the GPU test may skip — and records the share in the schema.  Fixtures
are numeric arrays and a JSON of seeds, sizes and key shapes; no reference source text is written anywhere.
"""
import copy
import importlib
import json
import os
import sys
import tempfile
import warnings

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
synth = importlib.import_module("revisiting-spatial-temporal-layouts_amd.synth")
import fusion_perturbation_restated as FR  # noqa: E402
import perturbation_restated as R  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")
REFERENCE = sys.argv[1] if len(sys.argv) > 1 else os.path.join(os.path.dirname(ROOT), "reference", "src")

CLIPS, STEPS = 2, 3
VIDEO = dict(T=32, H=32, W=64)  # grid 2 x 1 x 2
APPEARANCE_NUM_FRAMES = 4
WEIGHT_SEED, VIDEO_SEED, BATCH_SEED, SCORE_SEED = 4242, 17, 21, 20261020
MARGIN, CAP = 1e-3, 0.05
CONFIG = "cfg1"
CASES = {"resnet3d": [("appearance", o) for o in FR.ORDERS], "transformer": [("appearance", o) for o in FR.ORDERS],
         "cacnf": [("appearance", o) for o in FR.ORDERS] + [("both", o) for o in FR.ORDERS]}


def fixture_scores(B, C, T, N):
    """Seeded scores on a coarse grid (ties), some of them -0.0 and +0.0: (B,C) for the cells, (B,T,N) for the layout"""
    rng = np.random.Generator(np.random.PCG64(SCORE_SEED))
    cells = (np.round(rng.random((B, C)) * 3) / 3).astype(np.float32)
    cells[rng.random((B, C)) < 0.15] = -0.0
    lay = (np.round(rng.random((B, T, N)) * 8) / 8).astype(np.float32)
    lay[rng.random((B, T, N)) < 0.1] = -0.0
    return cells, lay


def schema(sd):
    return {k: {"shape": list(v.shape), "dtype": str(v.dtype).replace("torch.", "")} for k, v in sd.items()}


def main():
    sys.path.insert(0, REFERENCE)
    sys.dont_write_bytecode = True
    warnings.filterwarnings("ignore")
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    from modelling import models as RM
    from modelling.configs import AppearanceModelConfig, MultimodalModelConfig
    from modelling.resnets3d import generate_model

    tmp = tempfile.mkdtemp()
    ck = os.path.join(tmp, "r3d_random.pt")
    torch.save({"state_dict": generate_model(model_depth=50, n_classes=1139).state_dict()}, ck)
    c = synth.CONFIGS[CONFIG]
    kw = synth.model_kwargs(CONFIG)
    app_kw = dict(num_classes=kw["num_classes"], hidden_size=kw["hidden_size"], num_attention_heads=kw["num_attention_heads"],
                  hidden_dropout_prob=0.0, appearance_num_frames=APPEARANCE_NUM_FRAMES, resnet_model_path=ck)
    video = synth.make_video(CLIPS, seed=VIDEO_SEED, **VIDEO)
    shape = tuple(video.shape[2:])
    grid = FR.grid(shape, FR.VIDEO_CELL)
    C = grid[0] * grid[1] * grid[2]
    layout = synth.make_batch(CLIPS, c["T"], c["N"], seed=BATCH_SEED)
    nb = {k: v.numpy() for k, v in layout.items()}
    cells, lay = fixture_scores(CLIPS, C, c["T"], c["N"])
    empty = synth.DATASETS[c["dataset"]]["empty"]
    models = {
        "resnet3d": RM.Resnet3D(AppearanceModelConfig(**app_kw)),
        "transformer": RM.TransformerResnet(AppearanceModelConfig(**app_kw)),
        "cacnf": RM.CrossAttentionCentralNetFusion(MultimodalModelConfig(**dict(kw, appearance_num_frames=APPEARANCE_NUM_FRAMES, resnet_model_path=ck,
                                                                                num_appearance_layers=2, num_fusion_layers=2))),
    }
    meta = {"clips": CLIPS, "steps": STEPS, "video": VIDEO, "grid": list(grid), "appearance_num_frames": APPEARANCE_NUM_FRAMES, "weight_seed": WEIGHT_SEED,
            "video_seed": VIDEO_SEED, "batch_seed": BATCH_SEED, "score_seed": SCORE_SEED, "config": CONFIG, "cacnf_num_appearance_layers": 2,
            "cacnf_num_fusion_layers": 2, "margin": MARGIN, "cap": CAP, "clip_index": list(range(CLIPS)), "models": {}}
    S = STEPS + 1
    for name, model in models.items():
        sd = synth.make_r3d_state_dict({k: tuple(v.shape) for k, v in model.state_dict().items()}, seed=WEIGHT_SEED)
        model.load_state_dict(sd, strict=True)
        model.train(False)
        model64 = copy.deepcopy(model).double()
        with torch.no_grad():  # the grid against the reference's own trunk: as many positions as appearance tokens
            trunk = model if name == "resnet3d" else (model.resnet if name == "transformer" else model.backbone.appearance_branch.resnet)
            feats = trunk.forward_features({"video_frames": video})
            assert tuple(feats.shape[2:]) == grid and C == APPEARANCE_NUM_FRAMES, (tuple(feats.shape), grid)
        out = {"scores_cells": cells}
        if name == "cacnf":
            out["scores_layout"] = lay
        low = total = 0
        for modality, order in CASES[name]:
            tag = f"{modality}_{order}"
            rank, n_cand = FR.rank_cells(torch.from_numpy(cells), order == "descending")
            vids, removed = FR.apply_cells(video, FR.VIDEO_CELL, rank, n_cand, STEPS, 0, STEPS, 0.0)
            out[f"removed_{tag}"] = removed.numpy()
            if modality == "both":
                lrank, ln = R.rank(lay, nb["src_key_padding_mask_boxes"], nb["lengths"], "object", order == "descending")
                pert = R.apply(nb, lrank, ln, STEPS, 0, STEPS, empty)
                out[f"removed_layout_{tag}"] = pert.pop("removed")
                out[f"n_candidates_layout_{tag}"] = ln
            logits, logits64 = {}, {}
            with torch.no_grad():
                for s in range(S):  # one run per step at the fixture's batch size
                    step = {"video_frames": vids[s * CLIPS:(s + 1) * CLIPS]}
                    if name == "cacnf":
                        src = {k: torch.from_numpy(np.ascontiguousarray(v[s * CLIPS:(s + 1) * CLIPS])) for k, v in pert.items()} if modality == "both" else layout
                        step.update(src)
                    for k, v in model(step).items():
                        logits.setdefault(k, []).append(v.float().numpy())
                    step64 = {k: (v.double() if v.is_floating_point() else v) for k, v in step.items()}
                    for k, v in model64(step64).items():
                        logits64.setdefault(k, []).append(v.numpy())
            for k in logits:
                arr = np.stack(logits[k])
                assert np.isfinite(arr).all(), f"{name} {tag}: NaN / inf in the reference's logits"
                out[f"logits_{k}_{tag}"] = arr
            head = "ensemble" if "ensemble" in logits else list(logits)[-1]  # the native models' last logit name
            l64 = np.stack(logits64[head])
            target = R.curve(l64)[2]
            margin = R.margin(l64, target)
            out[f"margin_{tag}"] = margin
            low += int((margin < MARGIN).sum())
            total += margin.size
        assert low <= CAP * total, f"{name}: {low} of {total} (step, clip) entries have a top-two margin below {MARGIN}"
        path = os.path.join(GOLDEN, f"fusion_perturbation_{name}.npz")
        np.savez_compressed(path, **out)
        meta["models"][name] = {"keys": schema(model.state_dict()), "cases": [f"{m}_{o}" for m, o in CASES[name]], "logit_names": list(logits),
                                "low_margin_share": low / total, "low_margin": low, "entries": total}
        print(f"{name}: {CLIPS} clips, {S} steps, {len(CASES[name])} cases, {low}/{total} margins below {MARGIN} -> {os.path.getsize(path)} bytes")
    with open(os.path.join(GOLDEN, "fusion_perturbation_schema.json"), "w") as f:
        json.dump(meta, f)


if __name__ == "__main__":
    main()
