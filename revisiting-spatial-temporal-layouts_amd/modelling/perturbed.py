"""``forward_perturbed`` of the video and fusion models: the perturbation test of Chefer, Gur and Wolf (2021) on the appearance side, the
layout side, or both.  One routine serves Resnet3D, TransformerResnet, CrossAttentionFusion, CrossAttentionCentralNetFusion and
LateConcatenationFusion: rank (stlt_perturb_rank_cells / stlt_perturb_rank), delete for a rising k (stlt_perturb_apply_cells /
stlt_perturb_apply), the model's ordinary ``forward`` on every reduced batch, one launch for the curves (stlt_perturb_curve).  Nothing is
read back; the whole call is capturable once the model's workspaces have their size.

What an appearance token's deletion means is written down at ``collate.perturb_cells``: the reference's appearance encoder takes no
key-padding mask (src/modelling/models.py:269), so the stride block of the token — its cell — is set to ``fill`` in the video.
"""
from __future__ import annotations

from typing import Dict, Optional

import torch

from .. import _lib as L
from .. import ops

MODALITIES = ("appearance", "layout", "both")
_LAYOUT_KEYS = tuple(k for k, _, _ in ops.PERTURB_KEYS)


def _tile(v: torch.Tensor, n: int) -> torch.Tensor:
    return v.repeat((n,) + (1,) * (v.dim() - 1))


@torch.no_grad()
def forward_perturbed(model, batch: Dict[str, torch.Tensor], scores, steps: int = 10, order: str = "descending", modality: str = "appearance",
                      unit: str = "object", target=None, head: Optional[str] = None, steps_per_pass: Optional[int] = None, fill: float = 0.0,
                      dataset_name: str = "something", activation: str = "softmax", dropout_live: bool = False, modalities=MODALITIES, has_trunk: bool = True) -> Dict[str, torch.Tensor]:
    """See CrossAttentionFusion.forward_perturbed.  ``modalities``: what this model accepts; ``dropout_live``: the model's own answer;
    ``has_trunk``: a fusion model built with ``appearance_trunk=True``."""
    from .. import collate
    who = "forward_perturbed"
    if dropout_live:
        raise L.StltHipError(f"{who} is an inference call: the model is in training mode with dropout > 0 (call model.train(False))")
    if modality not in MODALITIES:
        raise L.StltHipError(f"{who}: modality: expected one of {MODALITIES}, got {modality!r}")
    if modality not in modalities:
        raise L.StltHipError(f"{who}: this model has the appearance side only: modality must be 'appearance', got {modality!r}")
    descending = collate._perturb_args(order, unit)
    steps = int(steps)
    if steps < 1:
        raise L.StltHipError(f"{who}: steps must be >= 1, got {steps}")
    S = steps + 1
    per = S if steps_per_pass is None else int(steps_per_pass)
    if per < 1:
        raise L.StltHipError(f"{who}: steps_per_pass must be >= 1, got {steps_per_pass}")
    names = tuple(model.logit_names)
    head = names[-1] if head is None else head
    if head not in names:
        raise L.StltHipError(f"{who}: head must be one of {names}, got {head!r}")
    do_app, do_lay = modality in ("appearance", "both"), modality in ("layout", "both")
    if modality == "both":
        if not isinstance(scores, dict) or set(scores) != {"layout", "appearance"}:
            raise L.StltHipError(f'{who}: modality "both" takes scores = {{"layout": ..., "appearance": ...}}, got {type(scores).__name__}')
        sc_lay, sc_app = scores["layout"], scores["appearance"]
    else:
        sc_lay, sc_app = (scores, None) if do_lay else (None, scores)
    fusion = "layout" in modalities
    if fusion and "appearance_features" in batch:  # the fusion models read the features when a batch carries both: so does the deletion
        batch = {k: v for k, v in batch.items() if k != "video_frames"}
    if fusion and "appearance_features" not in batch and "video_frames" in batch and not has_trunk:
        raise L.StltHipError("the batch needs `appearance_features` (or `video_frames` with MultimodalModelConfig(appearance_trunk=True))")
    if not fusion and "video_frames" not in batch:
        raise L.StltHipError(f"{who}: the batch needs `video_frames`")
    app_key, cell, grid = collate.appearance_cells(batch)
    tensors = [batch[app_key]] + ([batch["categories"]] if fusion else []) + [s for s in (sc_lay, sc_app) if s is not None]
    if not all(isinstance(t, torch.Tensor) and t.is_cuda for t in tensors):
        raise L.StltHipError(f"{who} runs on the GPU: the batch or the scores hold CPU tensors (move the model and the batch to a cuda device)")
    x = ops._chk(batch[app_key].contiguous(), torch.float32, app_key)
    device, B = x.device, x.shape[0]
    if target is not None and (not isinstance(target, torch.Tensor) or target.dtype != torch.int64 or tuple(target.shape) != (B,) or target.device != device):
        raise L.StltHipError(f"{who}: target is None or an int64 ({B},) tensor on the batch's device")
    core = {k: batch[k].contiguous() for k in _LAYOUT_KEYS if k in batch} if fusion else {}
    counts = {k: batch[k] for k in ("num_real_tokens", "num_real_frames") if k in batch} if fusion else {}
    if any(isinstance(v, torch.Tensor) and v.is_cuda for v in counts.values()):
        raise L.StltHipError("num_real_tokens / num_real_frames must be host integers (a device tensor would have to be read back, which is what they are there to avoid)")
    counts = {k: int(v) for k, v in counts.items()}
    removed = {}
    if do_app:
        n_cells = grid[0] * grid[1] * grid[2]
        max_items = L.load().stlt_perturb_max_items()
        if n_cells > max_items:
            raise L.StltHipError(f"{who}: {n_cells} cells exceed the {max_items} a clip is ranked with (STLT_EINVAL)")
        rank_app, n_app = ops.perturb_rank_cells(collate.cell_scores(sc_app, B, n_cells), descending)
        removed["appearance"] = torch.empty(S, B, device=device, dtype=torch.int32)
    if do_lay:
        rank_lay, n_lay = ops.perturb_rank(sc_lay.to(torch.float32).contiguous(), core["src_key_padding_mask_boxes"], core["lengths"], unit, descending)
        removed["layout"] = torch.empty(S, B, device=device, dtype=torch.int32)
        empty_type = collate.DATASETS[dataset_name]["empty"]
    logits = None
    for s0 in range(0, S, per):
        s1 = min(s0 + per, S) - 1
        n = s1 - s0 + 1
        if do_lay:
            part = ops.perturb_apply(core, rank_lay, n_lay, steps, s0, s1, empty_type, removed=removed["layout"])
            part.pop("removed")
        else:
            part = {k: _tile(v, n) for k, v in core.items()}
        part.update({k: v * n for k, v in counts.items()})
        if do_app:
            part[app_key], _ = ops.perturb_apply_cells(x, cell, rank_app, n_app, steps, s0, s1, fill, removed=removed["appearance"][s0:s1 + 1])
        else:
            part[app_key] = _tile(x, n)
        out = model.forward(part)
        if logits is None:
            logits = {k: torch.empty(S, B, out[k].shape[-1], device=device, dtype=torch.float32) for k in names}
        for k in names:
            logits[k][s0:s1 + 1].copy_(out[k].view(n, B, -1))
    prob, hit, tgt = ops.perturb_curve(logits[head], target, activation)
    result = dict(logits)
    result.update(prob=prob, hit=hit, auc=(prob.sum(0) - 0.5 * (prob[0] + prob[-1])) / steps, target=tgt)
    if modality == "both":
        result.update(removed_layout=removed["layout"], n_candidates_layout=n_lay, removed_appearance=removed["appearance"], n_candidates_appearance=n_app)
    elif do_app:
        result.update(removed=removed["appearance"], n_candidates=n_app)
    else:
        result.update(removed=removed["layout"], n_candidates=n_lay)
    return result
