"""The Python shell of the explanation calls — ``forward_attention``, ``forward_saliency``, ``forward_relevance``, ``forward_perturbed``,
``forward_integrated_gradients`` and ``forward_prefixes`` — written once for Stlt, Resnet3D, TransformerResnet, CrossAttentionFusion, CrossAttentionCentralNetFusion and
LateConcatenationFusion: the refusals of an inference call (``require_inference``), the target of a saliency / relevance pass and its seed
(``parse_target``, ``logit_seed``, ``saliency_seed``), the choice of a head (``pick_head``), and the perturbation test of Chefer, Gur and
Wolf (2021) on the layout side, the appearance side, or both (``forward_perturbed``): rank (stlt_perturb_rank / stlt_perturb_rank_cells),
delete for a rising k (stlt_perturb_apply / stlt_perturb_apply_cells), the model's ordinary forward on every reduced batch, one launch for
the curves (stlt_perturb_curve).  Nothing is read back; the whole call is capturable once the model's workspaces have their size.
``forward_integrated_gradients`` (Sundararajan, Taly, Yan 2017) is the same kind of shell around each model's own ``forward_saliency``:
the path batches of a pass in one launch per input (stlt_ig_path / stlt_ig_path_dense), the model's sweep on them, the quadrature in a
fixed order (stlt_ig_reduce), the completeness gap on the device (stlt_ig_delta).
``forward_gradcam`` (Selvaraju et al. 2017; HiResCAM: Draelos and Carin 2020) is the shell of the class activation maps at a stage of the
R3D-50 trunk for the five models that read appearance: the model's layers above the trunk give the gradient at the feature map, the
sweep stopped at the stage (stlt_r3d_backward_layer) carries it down, stlt_cam_weights and stlt_cam_map reduce it with the activations.

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


class InputRowSeed:
    """The target of a ``forward_saliency`` call on a step-major pass of ``forward_integrated_gradients`` whose last ``B`` rows are the
    unperturbed input: every row is seeded with the top-1 class of its own clip's input row (stlt_saliency_seed on those rows, tiled), so
    the class comes from logits the pass itself produces and nothing is read back."""

    def __init__(self, B: int):
        self.B = int(B)

    def resolve(self, logits: torch.Tensor) -> torch.Tensor:
        return _tile(logit_seed(logits[logits.shape[0] - self.B:].contiguous(), None, None), logits.shape[0] // self.B)


def parse_target(who: str, target, B: int, K: int, device):
    """The three forms of a saliency / relevance target -> (int64 classes or None, float seed or None); both None: top-1."""
    if isinstance(target, InputRowSeed):
        return None, target
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
    if isinstance(seed, InputRowSeed):
        return seed.resolve(logits)
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


IG_BASELINE_KEYS = ("boxes", "scores", "video_frames", "appearance_features")


@torch.no_grad()
def forward_integrated_gradients(model, batch: Dict[str, torch.Tensor], target=None, steps: int = 16, baseline=None, steps_per_pass: Optional[int] = None,
                                 head: Optional[str] = None, modality: Optional[str] = None, dropout_live: bool = False, modalities=MODALITIES,
                                 has_trunk: bool = True, num_classes: Optional[int] = None, takes_head: bool = False) -> Dict[str, torch.Tensor]:
    """See Stlt.forward_integrated_gradients and CrossAttentionFusion.forward_integrated_gradients.  ``modalities``: what this model reads
    (its ``perturb_modalities``); ``dropout_live``: the model's own answer; ``has_trunk``: a fusion model built with
    ``appearance_trunk=True``; ``num_classes``: the width of the logits when the model knows it before a forward (a float target is then
    checked against it here); ``takes_head``: the model's ``forward_saliency`` takes ``head``.
    Per pass of at most ``steps_per_pass`` steps, from the input end of the path downwards: one path launch per moved input, the model's
    own ``forward_saliency`` on the pass's (n*B)-clip batch with the target tiled, one stlt_ig_reduce per moved input.  Within a pass the
    steps are added in ascending s; the passes themselves run from the highest steps to the lowest, so the order of the sum is a function
    of ``steps`` and ``steps_per_pass`` alone and two calls give the same bits."""
    who = "forward_integrated_gradients"
    require_inference(who, dropout_live=dropout_live)
    has_lay, has_app = "layout" in modalities, "appearance" in modalities
    if modality is None:
        modality = "both" if has_lay and has_app else ("layout" if has_lay else "appearance")
    if modality not in MODALITIES:
        raise L.StltHipError(f"{who}: modality: expected one of {MODALITIES}, got {modality!r}")
    if modality not in modalities:
        raise L.StltHipError(f"{who}: this model reads the {'layout' if has_lay else 'appearance'} side only: modality {modality!r} is not one of {tuple(modalities)}")
    if isinstance(steps, bool) or not isinstance(steps, int) or steps < 1 or steps >= 1 << 23:
        raise L.StltHipError(f"{who}: steps must be an integer >= 1 (and below 2^23), got {steps!r}")
    S = steps + 1
    per = S if steps_per_pass is None else steps_per_pass
    if isinstance(per, bool) or not isinstance(per, int) or per < 1:
        raise L.StltHipError(f"{who}: steps_per_pass must be an integer >= 1, got {steps_per_pass!r}")
    per = min(per, S)
    if per > L.IG_MAX_STEPS:
        raise L.StltHipError(f"{who}: one pass holds at most {L.IG_MAX_STEPS} steps, got {per} (set steps_per_pass)")
    names = tuple(model.logit_names)
    head = pick_head(who, names, head) if takes_head else names[-1]
    do_app, do_lay = modality in ("appearance", "both"), modality in ("layout", "both")
    app_key = None
    if has_app:
        app_key = "appearance_features" if has_lay and "appearance_features" in batch else "video_frames"
        if app_key not in batch:
            raise L.StltHipError("the batch needs `appearance_features` (or `video_frames` with MultimodalModelConfig(appearance_trunk=True))" if has_lay
                                 else f"{who}: the batch needs `video_frames`")
        if has_lay and app_key == "video_frames" and not has_trunk:
            raise L.StltHipError("the batch needs `appearance_features` (or `video_frames` with MultimodalModelConfig(appearance_trunk=True))")
    require_inference(who, tensors=([batch[app_key]] if has_app else []) + ([batch["categories"]] if has_lay else []))
    first_t = batch["categories"] if has_lay else batch[app_key]
    device, B = first_t.device, first_t.shape[0]
    core = {k: batch[k].contiguous() for k in _LAYOUT_KEYS if k in batch} if has_lay else {}
    counts = {k: batch[k] for k in ("num_real_tokens", "num_real_frames") if k in batch} if has_lay else {}
    if any(isinstance(v, torch.Tensor) and v.is_cuda for v in counts.values()):
        raise L.StltHipError("num_real_tokens / num_real_frames must be host integers (a device tensor would have to be read back, which is what they are there to avoid)")
    counts = {k: int(v) for k, v in counts.items()}
    x_app = ops._chk(batch[app_key].contiguous(), torch.float32, app_key) if has_app else None
    moved = {}  # key -> the input the path moves, in the order the attributions are summed in
    if do_lay:
        moved["boxes"] = ops._chk(core["boxes"], torch.float32, "boxes")
        if "scores" in core:
            moved["scores"] = ops._chk(core["scores"], torch.float32, "scores")
    if do_app:
        moved[app_key] = x_app
    if baseline is None:
        baseline = {}
    if not isinstance(baseline, dict):
        raise L.StltHipError(f"{who}: baseline is None or a dict with any of {IG_BASELINE_KEYS}, got {type(baseline).__name__}")
    for k, v in baseline.items():
        if k not in IG_BASELINE_KEYS:
            raise L.StltHipError(f"{who}: baseline: unknown key {k!r} (expected any of {IG_BASELINE_KEYS})")
        if k not in moved:
            raise L.StltHipError(f"{who}: baseline[{k!r}]: modality {modality!r} does not move `{k}` on this batch (it moves {tuple(moved)})")
        x = moved[k]
        if not isinstance(v, torch.Tensor) or tuple(v.shape) != tuple(x.shape) or v.dtype != x.dtype or v.device != x.device:
            raise L.StltHipError(f"{who}: baseline[{k!r}] must have the input's shape, dtype and device — {tuple(x.shape)}, {x.dtype}, {x.device} — got "
                                 f"{(tuple(v.shape), v.dtype, v.device) if isinstance(v, torch.Tensor) else type(v).__name__}")
    base = {k: (baseline[k].contiguous() if k in baseline else None) for k in moved}
    # a bad target is refused here, before a tape is overwritten; the width of a float seed is checked where the model knows it
    if isinstance(target, torch.Tensor) and target.is_floating_point():
        if target.dim() != 2 or target.shape[0] != B or target.device != device or (num_classes is not None and target.shape[1] != num_classes):
            raise L.StltHipError(f"{who}: a float target is the (B, num_classes) = ({B}, {num_classes if num_classes is not None else 'K'}) seed on the batch's device, "
                                 f"got {tuple(target.shape)} on {target.device}")
        tgt, seed = None, target.detach().to(torch.float32).contiguous()
    elif target is not None:
        tgt, seed = parse_target(who, target, B, 0, device)
    else:
        tgt, seed = None, None
    kw = {"head": head} if takes_head else {}
    acc = {k: torch.empty_like(v) for k, v in moved.items()}
    attr, obj, x_logits, out = {}, None, None, None
    hi = steps
    while hi >= 0:
        lo = max(hi - per + 1, 0)
        n = hi - lo + 1
        if do_lay:
            part = ops.ig_path(core, steps, lo, hi, base["boxes"], base.get("scores"))
        else:
            part = {k: _tile(v, n) for k, v in core.items()}
        part.update({k: v * n for k, v in counts.items()})
        if do_app:
            part[app_key] = ops.ig_path_dense(x_app, steps, lo, hi, base[app_key])
        elif has_app:
            part[app_key] = _tile(x_app, n)
        if seed is not None:
            t_arg = _tile(seed, n)
        elif tgt is not None:
            t_arg = _tile(tgt, n)
        else:
            t_arg = InputRowSeed(B)  # the first pass ends with the input's rows: their top-1 seeds every step
        out = model.forward_saliency(part, target=t_arg, **kw)
        if x_logits is None:
            x_logits = {k: out[k][(n - 1) * B:].contiguous() for k in names}
            seed_bk = seed if seed is not None else logit_seed(x_logits[head], tgt, None)
            if tgt is None and seed is None:
                tgt = seed_bk.argmax(dim=1)  # the one-hot row's only 1, still on the device; the later passes are seeded with it
        finish = lo == 0
        for k in (["scores"] if "scores" in moved else []) + [k for k in moved if k != "scores"]:  # the score term is ready when the boxes are grouped
            g = out[k + "_grad"].contiguous()
            if not finish:
                ops.ig_reduce(g, acc[k], steps, lo, hi, begin=hi == steps)
            elif k == "boxes":
                attr[k], obj = ops.ig_reduce(g, acc[k], steps, lo, hi, begin=hi == steps, finish=True, x=moved[k], baseline=base[k], group=4, extra=attr.get("scores"))
            else:
                attr[k], _ = ops.ig_reduce(g, acc[k], steps, lo, hi, begin=hi == steps, finish=True, x=moved[k], baseline=base[k])
        hi = lo - 1
    base_logits = out[head][:B].contiguous()
    result = dict(x_logits)
    result.update(baseline_logits=base_logits, target=target if target is not None else tgt)
    result["delta"] = ops.ig_delta([attr[k] for k in moved], seed_bk, x_logits[head], base_logits)
    for k in moved:
        result[k + "_attribution"] = attr[k]
    if do_lay:
        result["object_attribution"] = obj
    if do_app:
        _, cell, _ = collate.appearance_cells({app_key: x_app})
        result["cell_attribution"] = ops.cell_pool_sum(attr[app_key], cell)
    return result


GRADCAM_VARIANTS = ("gradcam", "hirescam")


@torch.no_grad()
def forward_gradcam(model, batch: Dict[str, torch.Tensor], target=None, layer: int = 4, variant: str = "gradcam", relu: bool = True, upsample: bool = False,
                    head: Optional[str] = None, dropout_live: bool = False, trunk=None, head_gradient: Optional[Callable] = None, takes_head: bool = False,
                    takes_features: bool = False, pooled_head: bool = False) -> Dict[str, torch.Tensor]:
    """See Resnet3D.forward_gradcam.  ``trunk``: (TrunkRunner, the trunk's nn.Sequential) or None (a fusion model without
    ``appearance_trunk``); ``head_gradient(features, pooled, target, head)``: the model's part — its layers above the trunk on the feature
    map as a leaf -> ({name: logits}, target as returned, d logit / d features (B, 2048, gt, gh, gw) or None, d logit / d pooled (B, 2048) or
    None; exactly one of the two); ``takes_head``: the model has several logits; ``takes_features``: the model reads precomputed
    ``appearance_features`` when the batch carries them; ``pooled_head``: the model's head reads the average-pooled features (Resnet3D);
    ``dropout_live``: the model's own answer.
    The last stage: the plain trunk forward (or the batch's features), the head's gradient, stlt_cam_weights and stlt_cam_map in NCDHW.
    A stage below: the tape forward, the head's gradient, stlt_r3d_backward_layer, then the two launches in NDHWC on the tape's slot."""
    who = "forward_gradcam"
    if isinstance(layer, bool) or not isinstance(layer, int) or not 1 <= layer <= 4:
        raise L.StltHipError(f"{who}: layer is a stage of the trunk, 1 to 4, got {layer!r}")
    if variant not in GRADCAM_VARIANTS:
        raise L.StltHipError(f"{who}: variant: expected one of {GRADCAM_VARIANTS}, got {variant!r}")
    require_inference(who, dropout_live=dropout_live)
    names = tuple(model.logit_names)
    head = pick_head(who, names, head) if takes_head else names[-1]
    from_features = takes_features and "appearance_features" in batch
    if from_features and layer < 4:
        raise L.StltHipError(f"{who}: layer {layer} lies inside the trunk: the batch carries only `appearance_features`, the trunk's output; it needs "
                             f"`video_frames` (and MultimodalModelConfig(appearance_trunk=True)); layer 4 works on the features")
    if not from_features and ("video_frames" not in batch or trunk is None):
        raise L.StltHipError("the batch needs `appearance_features` (or `video_frames` with MultimodalModelConfig(appearance_trunk=True))" if takes_features
                             else f"{who}: the batch needs `video_frames`")
    app_key = "appearance_features" if from_features else "video_frames"
    require_inference(who, tensors=(batch[app_key],))
    x = ops._chk(batch[app_key].contiguous(), torch.float32, app_key)
    if x.dim() != 5:
        raise L.StltHipError(f"{app_key} must have five dimensions, got {tuple(x.shape)}")
    if upsample and from_features:
        raise L.StltHipError(f"{who}: upsample lays the map over `video_frames`, which this batch does not carry")
    B = x.shape[0]
    want_pooled = pooled_head
    tape = None
    if from_features:
        feats, pooled = x, None
    elif layer == 4:
        feats, pooled = trunk[0].run(trunk[1], x, features=True, pooled=want_pooled)
    else:
        tape = trunk[0].run_tape(trunk[1], x, features=not want_pooled, pooled=want_pooled)
        feats, pooled = tape.features, tape.pooled
    logits, target, dfeatures, dpooled = head_gradient(feats, pooled, target, head)
    if layer == 4:
        a, layout = feats, "ncdhw"
        if dfeatures is None:  # the pooled features' gradient, spread as the average pool spreads it: dpooled / P at every position
            P = feats[0, 0].numel()
            dfeatures = (dpooled / P).view(B, -1, 1, 1, 1).expand_as(feats).contiguous()
        g = dfeatures.contiguous()
    else:
        a, layout = tape.stage(layer), "ndhwc"
        g = tape.backward_layer(layer, dfeatures=None if dfeatures is None else dfeatures.contiguous(), dpooled=dpooled)
    cam = ops.cam_map(a, ops.cam_weights(g, layout) if variant == "gradcam" else g, layout, relu=relu)
    result = {k: logits[k] for k in names}
    result.update(target=target, cam=cam)
    if layer == 4:
        result["cell_attribution"] = cam.flatten(1)
    else:
        result["cell_attribution"] = ops.cell_pool_sum(cam.view(B, 1, *cam.shape[1:]), (1 << (4 - layer),) * 3)
    if upsample:
        result["video_cam"] = ops.cam_upsample(cam, x.shape[2:])
    return result
