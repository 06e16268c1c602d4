"""The perturbation-test fixtures (tests/golden/perturbation_<cfg>.npz, tools/gen_golden_perturbation.py) rebuilt into what the CPU and GPU
tests compare against: the weights and the clips from the goldens' seeds, the stored scores, and per order / unit the expected rank, removal
counts, perturbed batch and the reference's logits.  Loaded once per config, shared, never modified.

The fixtures store a chosen subset of the clips the reference ran (``clip_index``; the batch is rebuilt whole from the seeds and cut to it).
For micro, cfg1 and cfg4 that is simply the first clips.  For ``odd`` it is clips 0, 2, 3, 4 of the golden batch: on the untouched clip 1
the reference's two best classes lie 3.0e-4 apart (float64 run), so its step 0 alone would put 4 of the 96 (step, clip) entries under the
1e-3 margin below which ``hit`` cannot be compared, in every order and unit and whatever the scores are — with any other near-tie that breaks
the generator's cap of 5 %.  The clip was left out for that reason, by the reference's own margins and before any run of the package; the
cap and its assertion stand as they are in tools/gen_golden_perturbation.py."""
import functools
import importlib
import os

import numpy as np
import torch

import perturbation_restated as R
from conftest import GOLDEN, PKG_NAME, golden_case

CONFIGS = ("micro", "cfg1", "odd", "cfg4")
COMBOS = [(order, unit) for unit in R.UNITS for order in R.ORDERS]
BATCH_KEYS = ("categories", "boxes", "scores", "src_key_padding_mask_boxes", "frame_types", "src_key_padding_mask_frames", "lengths")


@functools.lru_cache(maxsize=None)
def fixture(name):
    """-> dict: sd, batch (the stored clips, CPU tensors), steps, dataset, heads, scores {unit: tensor}, and z: the fixture's arrays"""
    synth = importlib.import_module(PKG_NAME + ".synth")
    z = np.load(os.path.join(GOLDEN, f"perturbation_{name}.npz"))
    sd, _, _, meta = golden_case(name)
    c = synth.CONFIGS[name]
    full = synth.make_batch(int(z["batch_clips"][0]), c["T"], c["N"], dataset=c["dataset"], seed=meta["input_seed"])
    sel = torch.from_numpy(z["clip_index"])
    batch = {k: v[sel].contiguous() for k, v in full.items()}
    return {"sd": sd, "batch": batch, "steps": int(z["steps"][0]), "dataset": c["dataset"], "heads": c["num_attention_heads"],
            "scores": {"object": torch.from_numpy(z["scores_object"]), "frame": torch.from_numpy(z["scores_frame"])}, "z": z}


def expected_batch(fx, order, unit):
    """The perturbed batch the fixture stores for (order, unit), all steps, step-major: categories, kpm_boxes and frame_types as stored,
    boxes / scores from the rule (zero where the stored mask turned True), the rest tiled."""
    z, batch, tag = fx["z"], fx["batch"], f"{order}_{unit}"
    S = fx["steps"] + 1
    out = {"categories": torch.from_numpy(z[f"categories_{tag}"]), "src_key_padding_mask_boxes": torch.from_numpy(z[f"kpm_boxes_{tag}"]),
           "frame_types": torch.from_numpy(z[f"frame_types_{tag}"])}
    tile = lambda t: t.repeat((S,) + (1,) * (t.dim() - 1))  # noqa: E731
    gone = out["src_key_padding_mask_boxes"] & ~tile(batch["src_key_padding_mask_boxes"])
    out["boxes"] = torch.where(gone[..., None], torch.zeros(()), tile(batch["boxes"]))
    if "scores" in batch:
        out["scores"] = torch.where(gone, torch.zeros(()), tile(batch["scores"]))
    out["src_key_padding_mask_frames"], out["lengths"] = tile(batch["src_key_padding_mask_frames"]), tile(batch["lengths"])
    return out


def same_bits(a, b):
    """equal as stored: floats are compared as the integers they are kept as (so -0.0 != +0.0 and NaN == NaN)"""
    a, b = a.detach().cpu().contiguous(), b.detach().cpu().contiguous()
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if a.dtype == torch.float32:
        a, b = a.view(torch.int32), b.view(torch.int32)
    return bool(torch.equal(a, b))
