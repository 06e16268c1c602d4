"""The Python shell of the explanation calls — ``forward_attention``, ``forward_saliency``, ``forward_relevance``, ``forward_perturbed`` and
``forward_prefixes`` — written once for Stlt, Resnet3D, TransformerResnet, CrossAttentionFusion, CrossAttentionCentralNetFusion and
LateConcatenationFusion: the refusals of an inference call (``require_inference``), the target of a saliency / relevance pass and its seed
(``parse_target``, ``logit_seed``, ``saliency_seed``), the choice of a head (``pick_head``), and the perturbation test of Chefer, Gur and
Wolf (2021) on the layout side, the appearance side, or both (``forward_perturbed``): rank (stlt_perturb_rank / stlt_perturb_rank_cells),
delete for a rising k (stlt_perturb_apply / stlt_perturb_apply_cells), the model's ordinary forward on every reduced batch, one launch for
the curves (stlt_perturb_curve).  Nothing is read back; the whole call is capturable once the model's workspaces have their size.

What an appearance token's deletion means is written down at ``collate.perturb_cells``: the reference's appearance encoder takes no
key-padding mask (src/modelling/models.py:269), so the stride block of the token — its cell — is set to ``fill`` in the video.
"""
from __future__ import annotations

from typing import Callable, Dict, Optional

import torch

from .. import _lib as L
from .. import collate, ops

MODALITIES = ("appearance", "layout", "both")
_LAYOUT_KEYS = tuple(k for k, _, _ in ops.PERTURB_KEYS)


def require_inference(who: str, *, dropout_live: bool = False, skip_padding: bool = False, skip_padding_attr: str = "backbone", tensors=(),
                      holder: str = "the batch holds") -> None:
    """The three refusals of an inference call ``who``, in this order: live dropout (the model's own answer), ``skip_padding`` on the
    backbone the call would run the padded schedule on (``skip_padding_attr`` names it for the message), a CPU tensor among ``tensors``.
    A call that checks them in another order calls twice."""
    if dropout_live:
        raise L.StltHipError(f"{who} is an inference call: the model is in training mode with dropout > 0 (call model.train(False))")
    if skip_padding:
        raise L.StltHipError(f"{who} runs the padded schedule: skip_padding is not supported (STLT_EINVAL); set {skip_padding_attr}.skip_padding = False")
    if not all(isinstance(t, torch.Tensor) and t.is_cuda for t in tensors):
        raise L.StltHipError(f"{who} runs on the GPU: {holder} CPU tensors (move the model and the batch to a cuda device)")


def parse_target(who: str, target, B: int, K: int, device):
    """The three forms of a saliency / relevance target -> (int64 classes or None, float seed or None); both None: top-1."""
    if isinstance(target, torch.Tensor) and target.is_floating_point():
        if tuple(target.shape) != (B, K) or target.device != device:
            raise L.StltHipError(f"{who}: a float target is the (B, num_classes) = ({B}, {K}) seed on the batch's device, got {tuple(target.shape)} on {target.device}")
        return None, target.detach().to(torch.float32).contiguous()
    if target is not None:
        if not isinstance(target, torch.Tensor) or target.dtype != torch.int64 or tuple(target.shape) != (B,) or target.device != device:
            raise L.StltHipError(f"{who}: target is None, an int64 ({B},) tensor or a float ({B}, {K}) tensor on the batch's device")
        return target.contiguous(), None
    return None, None


def logit_seed(logits: torch.Tensor, tgt, seed) -> torch.Tensor:
    """d(objective)/d(logits) of a saliency / relevance pass: the caller's float seed, or stlt_saliency_seed's one-hot rows"""
    if seed is None:
        seed = torch.empty_like(logits)
        with torch.cuda.device(logits.device):
            L.check(L.load().stlt_saliency_seed(logits.data_ptr(), None if tgt is None else tgt.data_ptr(), logits.shape[0], logits.shape[1], seed.data_ptr(),
                                                torch.cuda.current_stream().cuda_stream), "stlt_saliency_seed")
    return seed


def saliency_seed(logits: torch.Tensor, target, who: str = "forward_saliency"):
    """``target`` of a saliency / relevance call (None: top-1; int64 (B,): that class; float (B, K): the seed itself) -> (seed (B, K), target
    as returned: the one-hot rows' classes — the kernel's pick, lowest index on ties, still on the device — when none was given)."""
    tgt, seed = parse_target(who, target, logits.shape[0], logits.shape[1], logits.device)
    seed = logit_seed(logits.detach().contiguous(), tgt, seed)
    return seed, (seed.argmax(dim=1) if target is None else target)


def pick_head(who: str, names, head: Optional[str]) -> str:
    """``head`` of a call on a model with several logits: one of ``names``, default the last"""
    head = names[-1] if head is None else head
    if head not in names:
        raise L.StltHipError(f"{who}: head must be one of {names}, got {head!r}")
    return head


def _tile(v: torch.Tensor, n: int) -> torch.Tensor:
    return v.repeat((n,) + (1,) * (v.dim() - 1))


@torch.no_grad()
def forward_perturbed(model, batch: Dict[str, torch.Tensor], scores, steps: int = 10, order: str = "descending", modality: str = "appearance",
                      unit: str = "object", target=None, head: Optional[str] = None, steps_per_pass: Optional[int] = None, fill: float = 0.0,
                      dataset_name: str = "something", activation: str = "softmax", dropout_live: bool = False, modalities=MODALITIES, has_trunk: bool = True,
                      run_pass: Optional[Callable] = None) -> Dict[str, torch.Tensor]:
    """See CrossAttentionFusion.forward_perturbed and Stlt.forward_perturbed.  ``modalities``: what this model accepts (its
    ``perturb_modalities``); ``dropout_live``: the model's own answer; ``has_trunk``: a fusion model built with ``appearance_trunk=True``;
    ``run_pass(part, s0, s1, logits)``: runs the model on the reduced batch of steps s0 .. s1 and puts each head's logits into rows
    s0 .. s1 of ``logits`` = {name: (S,B,K)} (None before the first pass: the runner allocates it), returning the dict.  The default is the
    model's ``forward`` and one copy per head; Stlt has its native call write the rows in place."""
    who = "forward_perturbed"
    require_inference(who, dropout_live=dropout_live)
    if modality not in MODALITIES:
        raise L.StltHipError(f"{who}: modality: expected one of {MODALITIES}, got {modality!r}")
    if modality not in modalities:
        raise L.StltHipError(f"{who}: this model has the appearance side only: modality must be 'appearance', got {modality!r}")
    descending = collate._perturb_args(order, unit)
    steps, _, _ = collate._step_range(steps, None, who)
    S = steps + 1
    per = S if steps_per_pass is None else int(steps_per_pass)
    if per < 1:
        raise L.StltHipError(f"{who}: steps_per_pass must be >= 1, got {steps_per_pass}")
    names = tuple(model.logit_names)
    head = pick_head(who, names, head)
    do_app, do_lay = modality in ("appearance", "both"), modality in ("layout", "both")
    if modality == "both":
        if not isinstance(scores, dict) or set(scores) != {"layout", "appearance"}:
            raise L.StltHipError(f'{who}: modality "both" takes scores = {{"layout": ..., "appearance": ...}}, got {type(scores).__name__}')
        sc_lay, sc_app = scores["layout"], scores["appearance"]
    else:
        sc_lay, sc_app = (scores, None) if do_lay else (None, scores)
    has_lay, has_app = "layout" in modalities, "appearance" in modalities  # what the model reads, deleted from or not
    app_key = None
    if has_app:
        if has_lay and "appearance_features" in batch:  # the fusion models read the features when a batch carries both: so does the deletion
            batch = {k: v for k, v in batch.items() if k != "video_frames"}
        if has_lay and "appearance_features" not in batch and "video_frames" in batch and not has_trunk:
            raise L.StltHipError("the batch needs `appearance_features` (or `video_frames` with MultimodalModelConfig(appearance_trunk=True))")
        if not has_lay and "video_frames" not in batch:
            raise L.StltHipError(f"{who}: the batch needs `video_frames`")
        app_key, cell, grid = collate.appearance_cells(batch)
    tensors = ([batch[app_key]] if has_app else []) + ([batch["categories"]] if has_lay else []) + [s for s in (sc_lay, sc_app) if s is not None]
    require_inference(who, tensors=tensors, holder="the batch or the scores hold")
    x = ops._chk(batch[app_key].contiguous(), torch.float32, app_key) if has_app else None
    first = x if has_app else batch["categories"]
    device, B = first.device, first.shape[0]
    if target is not None and (not isinstance(target, torch.Tensor) or target.dtype != torch.int64 or tuple(target.shape) != (B,) or target.device != device):
        raise L.StltHipError(f"{who}: target is None or an int64 ({B},) tensor on the batch's device")
    core = {k: batch[k].contiguous() for k in _LAYOUT_KEYS if k in batch} if has_lay else {}
    counts = {k: batch[k] for k in ("num_real_tokens", "num_real_frames") if k in batch} if has_lay else {}
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

    def forward_and_copy(part, s0, s1, logits):
        out = model.forward(part)
        if logits is None:
            logits = {k: torch.empty(S, B, out[k].shape[-1], device=device, dtype=torch.float32) for k in names}
        for k in names:
            logits[k][s0:s1 + 1].copy_(out[k].view(s1 - s0 + 1, B, -1))
        return logits

    run_pass = forward_and_copy if run_pass is None else run_pass
    logits = None
    for s0 in range(0, S, per):
        s1 = min(s0 + per, S) - 1
        n = s1 - s0 + 1
        # the two `removed` conventions of ops (both public): perturb_apply takes the whole (S,B) buffer and writes its rows s0 .. s1,
        # perturb_apply_cells takes the (n,B) rows themselves
        if do_lay:
            part = ops.perturb_apply(core, rank_lay, n_lay, steps, s0, s1, empty_type, removed=removed["layout"])
            part.pop("removed")
        else:
            part = {k: _tile(v, n) for k, v in core.items()}
        part.update({k: v * n for k, v in counts.items()})
        if do_app:
            part[app_key], _ = ops.perturb_apply_cells(x, cell, rank_app, n_app, steps, s0, s1, fill, removed=removed["appearance"][s0:s1 + 1])
        elif has_app:
            part[app_key] = _tile(x, n)
        logits = run_pass(part, s0, s1, logits)
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
