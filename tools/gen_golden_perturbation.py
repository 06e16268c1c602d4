#!/usr/bin/env python3
"""Generate the perturbation-test fixtures tests/golden/perturbation_<cfg>.npz by importing the REFERENCE.

Run in the build container only (the reference never travels to the GPU box):

    PYTHONDONTWRITEBYTECODE=1 python tools/gen_golden_perturbation.py --reference /root/reference

For each config this builds the reference ``Stlt`` with the golden's weights and batch exactly as ``tools/gen_golden.py`` does, builds the
perturbed batches of both orders and both units with the NumPy restatement (tests/perturbation_restated.py) from seeded scores that hold
ties and both zeros, and runs the reference on every step's batch — a deleted slot is a slot without a detection as the reference's own
dataset and collater make it (datasets.py:64-69, 88-93, 274-278), so each is a batch the reference could have been handed.  Every step runs
at the golden's batch size, so that step 0 repeats the existing golden's run; the clips CLIPS[cfg] of it are stored (``clip_index``).  Stored per config:
``scores_object`` (B,T,N), ``scores_frame`` (B,T), and per order / unit ``rank``, ``removed`` (S,B), the perturbed ``categories``, ``kpm_boxes``
and ``frame_types`` (S*B clips, step-major), the reference's ``logits`` (S,B,K) float32 and ``margin`` (S,B) float64: the distance between
the target's logit (the top-1 class of step 0) and the best other class on the reference run in float64.  The tool asserts that step 0
equals the existing golden's logits bit for bit, that everything is finite, that at least one frame per config turns ``empty``, and that at
most 5 % of the (step, clip) entries have a margin below 1e-3 (the only entries the ``hit`` comparison of the GPU test may skip).
Fixtures are numeric arrays only; no reference source text is written anywhere.
"""
import argparse
import copy
import importlib
import os
import sys
import warnings

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
pkg = importlib.import_module("revisiting-spatial-temporal-layouts_amd.synth")
import perturbation_restated as R  # noqa: E402
from gen_golden import GOLDEN_BATCH, INPUT_SEED, WEIGHT_SEED  # noqa: E402

CLIPS = {"micro": (0, 1, 2, 3), "cfg1": (0, 1, 2, 3), "odd": (0, 2, 3, 4), "cfg4": (0, 1)}  # clips of the run that are stored
# odd: clip 1 of the golden batch is left out.  Its two best classes lie 3.0e-4 apart on the untouched clip (float64 reference), so its step 0
# alone would put 4 of the 96 (step, clip) entries under the margin, in every order and unit, whatever the scores are.
STEPS = {"micro": 5, "cfg1": 5, "odd": 5, "cfg4": 3}
SCORE_SEED = 20261020
MARGIN = 1e-3


def fixture_scores(name, B, T, N):
    """Seeded scores on a grid of eighths (blocks of ties), some of them -0.0 and +0.0: (B,T,N) for the objects, (B,T) for the frames"""
    rng = np.random.Generator(np.random.PCG64(SCORE_SEED + sum(map(ord, name))))
    obj = (np.round(rng.random((B, T, N)) * 8) / 8).astype(np.float32)
    frm = (np.round(rng.random((B, T)) * 4) / 4).astype(np.float32)
    obj[rng.random((B, T, N)) < 0.1] = -0.0
    frm[rng.random((B, T)) < 0.1] = -0.0
    return obj, frm


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default="/root/reference")
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden"))
    ap.add_argument("--configs", nargs="*", default=list(CLIPS))
    args = ap.parse_args()
    sys.path.insert(0, os.path.join(args.reference, "src"))
    sys.dont_write_bytecode = True
    warnings.filterwarnings("ignore")
    from modelling.configs import StltModelConfig  # reference
    from modelling.models import Stlt  # reference

    torch.set_num_threads(8)
    for name in args.configs:
        c = pkg.CONFIGS[name]
        ds = pkg.DATASETS[c["dataset"]]
        sel = np.array(CLIPS[name])
        B_run, B, steps = max(GOLDEN_BATCH[name], int(sel.max()) + 1), len(sel), STEPS[name]
        S = steps + 1
        model = Stlt(StltModelConfig(**pkg.model_kwargs(name)))
        sd = pkg.make_state_dict({k: tuple(v.shape) for k, v in model.state_dict().items()}, seed=WEIGHT_SEED)
        model.load_state_dict(sd, strict=True)
        model.train(False)
        model64 = copy.deepcopy(model).double()
        batch = pkg.make_batch(B_run, c["T"], c["N"], dataset=c["dataset"], seed=INPUT_SEED)
        T, N = batch["categories"].shape[1:]
        nb = {k: v.numpy() for k, v in batch.items()}
        gold = np.load(os.path.join(args.out, f"{name}.npz"))
        obj, frm = fixture_scores(name, B_run, T, N)
        out = {"scores_object": obj[sel], "scores_frame": frm[sel], "batch_clips": np.array([B_run]), "clip_index": sel, "steps": np.array([steps])}
        turned_empty, low, total = 0, 0, 0
        for unit in R.UNITS:
            sc = obj if unit == "object" else frm
            for order in R.ORDERS:
                rank, n_cand = R.rank(sc, nb["src_key_padding_mask_boxes"], nb["lengths"], unit, order == "descending")
                pert = R.apply(nb, rank, n_cand, steps, 0, steps, ds["empty"])
                logits, logits64 = [], []
                with torch.no_grad():
                    for s in range(S):  # one run per step at the golden's batch size: step 0 is the golden's own run
                        step = {k: torch.from_numpy(np.ascontiguousarray(v[s * B_run:(s + 1) * B_run])) for k, v in pert.items() if k != "removed"}
                        logits.append(model(step)["stlt"].float().numpy())
                        step["boxes"] = step["boxes"].double()
                        if "scores" in step:
                            step["scores"] = step["scores"].double()
                        logits64.append(model64(step)["stlt"].numpy())
                logits, logits64 = np.stack(logits), np.stack(logits64)
                n_gold = gold["logits"].shape[0]
                assert np.array_equal(logits[0, :n_gold], gold["logits"]), f"{name}: step 0 differs from the existing golden's logits"
                assert np.isfinite(logits).all() and np.isfinite(logits64).all(), f"{name}: NaN / inf in the reference's logits"
                target = R.curve(logits64[:, sel])[2]
                margin = R.margin(logits64[:, sel], target)
                low += int((margin < MARGIN).sum())
                total += margin.size
                clip = lambda v: v.reshape(S, B_run, *v.shape[1:])[:, sel].reshape(S * B, *v.shape[1:])  # noqa: E731
                turned_empty += int(((clip(pert["frame_types"]) == ds["empty"]) & (np.concatenate([nb["frame_types"][sel]] * S) != ds["empty"])).sum())
                tag = f"{order}_{unit}"
                out[f"rank_{tag}"] = rank[sel]
                out[f"n_candidates_{tag}"] = n_cand[sel]
                out[f"removed_{tag}"] = pert["removed"][:, sel]
                out[f"categories_{tag}"] = clip(pert["categories"])
                out[f"kpm_boxes_{tag}"] = clip(pert["src_key_padding_mask_boxes"])
                out[f"frame_types_{tag}"] = clip(pert["frame_types"])
                out[f"logits_{tag}"] = logits[:, sel]
                out[f"margin_{tag}"] = margin
        assert turned_empty > 0, f"{name}: no frame turns empty"
        assert low <= 0.05 * total, f"{name}: {low} of {total} (step, clip) entries have a top-two margin below {MARGIN}"
        path = os.path.join(args.out, f"perturbation_{name}.npz")
        np.savez_compressed(path, **out)
        print(f"{name}: {B} of {B_run} clips, {S} steps, {turned_empty} frames turn empty, {low}/{total} margins below {MARGIN} -> {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
