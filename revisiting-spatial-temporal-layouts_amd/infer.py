"""Inference loop for the STLT path: the counterpart of the reference's `inference()` (src/inference.py:15-85).

Step semantics reproduced: eval mode, no_grad, per batch `move_batch_to_device` -> `model(batch)` -> evaluator
update; here every rank runs its own shard of each batch and the top-1/top-5 counters (reference
src/utils/evaluation.py:21-34 keeps two integer counters per logit head) are summed over ranks at the end.  The
counters stay on the device: the reference's per-batch `.cpu()` synchronisation (evaluation.py:25-30) is gone.
"""
from __future__ import annotations

import itertools
from typing import Callable, Dict, Iterable, Optional

import torch

from . import dist as D
from ._lib import StltHipError


def topk_counts(logits: torch.Tensor, labels: torch.Tensor, ks=(1, 5)) -> torch.Tensor:
    """Number of rows whose label is among the k largest logits, for each k. -> int64 tensor (len(ks),)
    Device logits with the reference's ks = (1, 5) go through the library's counting kernel (include/stlt_hip.h:
    stlt_eval_topk, no torch kernels); anything else — CPU tensors in the not-gpu tests, other ks — takes the torch form."""
    if logits.is_cuda and tuple(ks) == (1, 5) and logits.dim() == 2 and logits.shape[0] > 0:
        from . import _lib as L
        lib = L.load()
        x = logits if (logits.dtype == torch.float32 and logits.stride(-1) == 1) else logits.float().contiguous()
        y = labels.to(device=logits.device, dtype=torch.int64).contiguous()
        counts = torch.zeros(2, dtype=torch.int64, device=logits.device)
        with torch.cuda.device(logits.device):
            L.check(lib.stlt_eval_topk(x.data_ptr(), x.stride(0), y.data_ptr(), x.shape[0], x.shape[1], counts.data_ptr(),
                                       torch.cuda.current_stream().cuda_stream), "stlt_eval_topk")
        return counts
    kmax = min(max(ks), logits.shape[1])
    top = logits.topk(kmax, dim=1).indices  # (n, kmax)
    hit = top == labels.view(-1, 1)
    return torch.stack([hit[:, : min(k, kmax)].any(dim=1).sum() for k in ks]).to(torch.int64)


@torch.no_grad()
def run_inference(model, batches: Iterable[Dict[str, torch.Tensor]], device, rank: int = 0, world: int = 1,
                  forward: Optional[Callable] = None, collect_logits: bool = False) -> Dict[str, object]:
    """Evaluate `model` over an iterable of collated batches (each holding `labels`), sharding every batch over ranks.

    `forward` defaults to `model(batch)["stlt"]`; tests on CPU pass a stand-in.  Returns top-1 / top-5 accuracy in
    percent (rounded as the reference logs them, inference.py:83-84), the clip count and optionally all logits.
    """
    if hasattr(model, "train"):
        model.train(False)
    counts = torch.zeros(3, dtype=torch.int64, device=device)  # top1, top5, n
    kept = []
    for batch in batches:
        n_total = D.batch_size(batch)
        mine = D.shard_batch(batch, rank, world)
        mine = {k: (v.to(device) if isinstance(v, torch.Tensor) else v) for k, v in mine.items()}
        if D.batch_size(mine) > 0:
            logits = forward(mine) if forward is not None else model(mine)["stlt"]
            c = topk_counts(logits, mine["labels"])
            counts[:2] += c
            counts[2] += logits.shape[0]
        else:
            logits = torch.zeros(0, 1, device=device)
        if collect_logits:
            width = torch.tensor([logits.shape[1] if logits.shape[0] else 0], device=device)
            if world > 1:
                torch.distributed.all_reduce(width, op=torch.distributed.ReduceOp.MAX)
            if logits.shape[0] == 0:
                logits = torch.zeros(0, int(width.item()), device=device)
            kept.append(D.gather_rows(logits.float(), n_total, world).cpu())
    D.all_reduce_sum_(counts, world)
    n = max(int(counts[2].item()), 1)
    out = {"top1_accuracy": round(100.0 * counts[0].item() / n, 2), "top5_accuracy": round(100.0 * counts[1].item() / n, 2),
           "num_clips": int(counts[2].item())}
    if collect_logits:
        out["logits"] = torch.cat(kept, dim=0) if kept else torch.zeros(0, 0)
    return out


@torch.no_grad()
def run_prefix_inference(model, batches: Iterable[Dict[str, torch.Tensor]], device, rank: int = 0, world: int = 1) -> Dict[str, torch.Tensor]:
    """Accuracy against the number of observed frames: `model.forward_prefixes` over an iterable of collated batches (each holding `labels`),
    every batch sharded over the ranks as in `run_inference`.  Returns {"top1", "top5", "num_clips"}: int64 tensors of length T (the longest
    batch's), entry t counting the clips that have a prefix of t observed frames (t < lengths) and those of them whose label is among the
    1 / 5 largest logits after t frames.  The counters stay on the device while the batches run: one `stlt_eval_topk` launch per t on the
    strided view logits[:, t] (row pitch T * num_classes), the labels of clips without that prefix set to -1 (the kernel ignores
    out-of-range labels); the counts are summed over the ranks at the end."""
    from . import _lib as L
    lib = L.load()
    if hasattr(model, "train"):
        model.train(False)
    counts = torch.zeros(0, 3, dtype=torch.int64, device=device)  # per t: top1, top5, clips
    for batch in batches:
        mine = D.shard_batch(batch, rank, world)
        mine = {k: (v.to(device) if isinstance(v, torch.Tensor) else v) for k, v in mine.items()}
        T = int(batch["categories"].shape[1])
        if T > counts.shape[0]:
            counts = torch.cat([counts, torch.zeros(T - counts.shape[0], 3, dtype=torch.int64, device=device)])
        if D.batch_size(mine) == 0:
            continue
        out = model.forward_prefixes(mine)
        logits, valid = out["stlt"], out["valid"]
        B, _, K = logits.shape
        labels = torch.where(valid.t(), mine["labels"].to(torch.int64)[None, :], torch.full((), -1, dtype=torch.int64, device=device)).contiguous()  # (T,B)
        part = torch.zeros(T, 3, dtype=torch.int64, device=device)
        with torch.cuda.device(logits.device):
            stream = torch.cuda.current_stream().cuda_stream
            for t in range(T):
                L.check(lib.stlt_eval_topk(logits.data_ptr() + 4 * t * K, T * K, labels.data_ptr() + 8 * t * B, B, K, part.data_ptr() + 24 * t, stream),
                        "stlt_eval_topk")
        part[:, 2] = valid.sum(0)  # the kernel's two counters of row t sit in part[t, 0:2]
        counts[:T] += part
    if world > 1:  # every rank sees the same batches, so the same T
        D.all_reduce_sum_(counts, world)
    counts = counts.cpu()
    return {"top1": counts[:, 0].clone(), "top5": counts[:, 1].clone(), "num_clips": counts[:, 2].clone()}


def perturb_curve(logits: torch.Tensor, target: Optional[torch.Tensor] = None, activation: str = "softmax"):
    """The curves of the perturbation test from logits (S,B,K): -> (prob (S,B) float32 — the target class's softmax probability, or its
    sigmoid; hit (S,B) bool — no class beats the target (a larger logit, or an equal logit at a lower index), or for sigmoid its logit is
    positive; target (B,) int64 — as given, or the arg-max of each clip's step-0 row, first maximum on ties).  A target outside [0, K)
    gives prob 0 and hit False.  Device logits go through the library (include/stlt_hip.h: stlt_perturb_curve); CPU logits take the
    torch form (the not-gpu tests, stand-in models)."""
    if logits.is_cuda:
        from . import ops
        x = logits if logits.dtype == torch.float32 else logits.float()
        if x.stride(-1) != 1 or x.stride(0) != x.shape[1] * x.stride(1):
            x = x.contiguous()
        return ops.perturb_curve(x, None if target is None else target.to(device=logits.device, dtype=torch.int64).contiguous(), activation)
    if activation not in ("softmax", "sigmoid"):
        raise StltHipError(f"activation: expected 'softmax' or 'sigmoid', got {activation!r}")
    x = logits.float()
    S, B, K = x.shape
    if target is None:
        top = x[0].max(dim=1, keepdim=True).values
        target = (x[0] == top).to(torch.int64).argmax(dim=1)  # the first maximum
    target = target.to(torch.int64)
    valid = (target >= 0) & (target < K)
    idx = target.clamp(0, K - 1)[None, :, None].expand(S, B, 1)
    xt = x.gather(2, idx)  # (S,B,1)
    if activation == "sigmoid":
        prob, hit = torch.sigmoid(xt[..., 0]), xt[..., 0] > 0
    else:
        prob = torch.softmax(x, dim=2).gather(2, idx)[..., 0]
        cls = torch.arange(K)[None, None, :]
        hit = ~((x > xt) | ((x == xt) & (cls < idx))).any(dim=2)
    return torch.where(valid[None], prob, torch.zeros(())), hit & valid[None], target


_PERTURB_METHODS = ("relevance", "saliency", "attention", "random", "integrated_gradients", "gradcam")


@torch.no_grad()
def _appearance_cls_attention(model, batch: Dict[str, torch.Tensor]) -> torch.Tensor:
    """What the CLS token of the appearance side attends to, (B,C): the fusion models' last fusion layer's appearance self-attention
    (forward_attention: fusion_appearance_attention[-1, 0]; LCF has no fusion layer: appearance_attention[-1]); TransformerResnet — which
    has no forward_attention — its last encoder layer's probabilities (ops.attn_probs on that layer's packed projections)."""
    from . import ops
    if hasattr(model, "forward_attention"):
        out = model.forward_attention(batch)
        fa = out["fusion_appearance_attention"]
        return (fa[-1, 0] if fa.shape[0] else out["appearance_attention"][-1])[:, 0, 1:]
    from .modelling import fusion as F
    H = model.config.num_attention_heads
    x = F._appearance_embed(model, model.resnet._runner.run(model.resnet.resnet, batch["video_frames"], name="….resnet.resnet")[0])
    layers = list(model.transformer.layers)
    x = F._appearance_layers(model, x, H, 0.0, len(layers) - 1)
    sa = layers[-1].self_attn
    qkv = ops.LinearFn.apply(x.contiguous(), sa.in_proj_weight, sa.in_proj_bias)
    kpm = torch.zeros(x.shape[0], x.shape[1], dtype=torch.uint8, device=x.device)
    return ops.attn_probs(qkv.contiguous(), kpm, False, H)[:, 0, 1:]


def appearance_attribution_scores(model, batch: Dict[str, torch.Tensor], method, generator: Optional[torch.Generator] = None, head: Optional[str] = None) -> torch.Tensor:
    """One (B,C) score per video cell (or feature column) from `method`, the appearance counterpart of attribution_scores: "relevance" —
    forward_relevance's appearance_relevance[:, 1:]; "saliency" — |video_frames_grad| (or |appearance_features_grad|) summed over each
    cell and all channels (stlt_cell_pool_abs); "integrated_gradients" — forward_integrated_gradients' cell_attribution, signed (stlt_cell_pool_sum);
    "gradcam" — forward_gradcam's cell_attribution (Grad-CAM at the trunk's last stage, whose positions are the cells);
    "attention" — the CLS row of the last appearance self-attention
    (_appearance_cls_attention); "random" — uniform numbers from `generator`; or a callable (model, batch) -> scores.  `head` goes to the
    fusion models' forward_relevance / forward_saliency.  Resnet3D has neither attention nor relevance and refuses the two."""
    from . import collate, ops
    if callable(method):
        return method(model, batch)
    kw = {} if head is None else {"head": head}
    if method in ("relevance", "attention") and not hasattr(model, "forward_relevance"):
        raise StltHipError(f"method {method!r}: {type(model).__name__} has no attention and no relevance; it takes 'saliency', 'random' or a callable")
    if method == "relevance":
        return model.forward_relevance(batch, **kw)["appearance_relevance"][:, 1:]
    if method == "attention":
        return _appearance_cls_attention(model, batch)
    key, cell, grid = collate.appearance_cells({k: v for k, v in batch.items() if k != "video_frames"} if "appearance_features" in batch and hasattr(model, "forward_attention")
                                               else batch)
    if method == "saliency":
        return ops.cell_pool_abs(model.forward_saliency(batch, **kw)[key + "_grad"].contiguous(), cell)
    if method == "integrated_gradients":
        side = {"modality": "appearance"} if "layout" in getattr(model, "perturb_modalities", ()) else {}
        return model.forward_integrated_gradients(batch, **kw, **side)["cell_attribution"]
    if method == "gradcam":
        return model.forward_gradcam(batch, **kw)["cell_attribution"]
    if method == "random":
        return torch.rand((batch[key].shape[0], grid[0] * grid[1] * grid[2]), generator=generator, device=batch[key].device, dtype=torch.float32)
    raise StltHipError(f"method: expected one of {_PERTURB_METHODS} or a callable (model, batch) -> scores, got {method!r}")


def attribution_scores(model, batch: Dict[str, torch.Tensor], method, generator: Optional[torch.Generator] = None, head: Optional[str] = None) -> torch.Tensor:
    """One (B,T,N) score per object slot from `method`: "relevance" — forward_relevance's map; "saliency" — |boxes_grad| summed over the four
    coordinates, plus |scores_grad| when the batch has scores; "integrated_gradients" — forward_integrated_gradients' signed
    object_attribution (zero baseline, 16 steps); "attention" — the last layers' raw attention joined like the relevance,
    temporal_attention[-1][b, lengths[b]-1, t] * spatial_attention[-1][b,t,0,n]; "random" — uniform numbers from `generator`; or a callable
    (model, batch) -> scores.  `head` (the fusion models): the logits the relevance and the saliency are taken from.  "gradcam" is refused:
    the layout side has no convolution."""
    if callable(method):
        return method(model, batch)
    kw = {} if head is None else {"head": head}
    if method == "relevance":
        return model.forward_relevance(batch, **kw)["relevance"]
    if method == "saliency":
        out = model.forward_saliency(batch, **kw)
        s = out["boxes_grad"].abs().sum(-1)
        return s + out["scores_grad"].abs() if "scores_grad" in out else s
    if method == "integrated_gradients":
        side = {"modality": "layout"} if "appearance" in getattr(model, "perturb_modalities", ()) else {}
        return model.forward_integrated_gradients(batch, **kw, **side)["object_attribution"]
    if method == "gradcam":
        raise StltHipError("method 'gradcam': a class activation map lives on the positions of the convolutional trunk, the video's cells; the layout side has no "
                           "convolution (use modality='appearance')")
    if method == "attention":
        out = model.forward_attention(batch)
        B = batch["categories"].shape[0]
        rows = torch.arange(B, device=batch["lengths"].device)
        return out["temporal_attention"][-1][rows, batch["lengths"] - 1][:, :, None] * out["spatial_attention"][-1][:, :, 0, :]
    if method == "random":
        cats = batch["categories"]
        return torch.rand(tuple(cats.shape), generator=generator, device=cats.device, dtype=torch.float32)
    raise StltHipError(f"method: expected one of {_PERTURB_METHODS} or a callable (model, batch) -> scores, got {method!r}")


@torch.no_grad()
def run_perturbation_test(model, batches: Iterable[Dict[str, torch.Tensor]], method="relevance", steps: int = 10,
                          orders=("descending", "ascending"), unit: str = "object", target: str = "top1", rank: int = 0, world: int = 1,
                          forward: Optional[Callable] = None, activation: str = "softmax", dataset_name: str = "something", seed: int = 0,
                          device=None, modality: str = "layout", head: Optional[str] = None, fill: float = 0.0) -> Dict[str, object]:
    """The perturbation test of Chefer, Gur and Wolf (2021) over an iterable of collated batches, every batch sharded over the ranks as in
    `run_inference`.  Per clip: rank the real object tokens (unit "frame": the frames, scored by the sum of their objects n >= 1) by the
    map `method` gives (attribution_scores), delete the first k of them for k rising over `steps` steps — the highest-scored first for
    order "descending", the lowest first for "ascending" —, run the model on every reduced batch, and follow the target class: "top1" —
    the model's own prediction on the untouched clip —, or "label" — batch["labels"].
    `forward` defaults to `model.forward_perturbed`; with a callable (batch) -> (n, K) logits the reduced batches come from
    `collate.perturb_batch` and the curves from `perturb_curve`, which serves any model (the fusion models on precomputed features, a
    stand-in on the CPU).  Which modalities `model.forward_perturbed` deletes from, and so which keywords it is called with, is the
    model's `perturb_modalities`: ("layout",) — `unit` and `dataset_name` —, ("appearance",) — `modality` and `fill` —, or all three —
    both sets and `head`; a model object without the attribute is taken for a layout-only one, as Stlt is (it is called with `unit` and
    `dataset_name` and refused any other modality).  The sums stay on the device while the batches run — fp64 probability and int64 hit
    per step, the clip count — and are all-reduced once at the end.  `device`: where the batches are moved to and the sums are kept (default: the device of the
    model's parameters; a model without parameters: wherever the first batch lies).  `seed` seeds the "random" method's device generator.
    -> {"fractions": [s / steps], order: {"prob": mean target probability per step, "accuracy": share of clips whose target is still the
    prediction per step, "auc_prob", "auc_accuracy": the trapezoid areas over the fractions, "num_clips"}}.  A faithful map makes the
    descending curves fall fast (small areas) and keeps the ascending ones flat (large areas).
    `modality` "layout" (the default) is the above.  "appearance" deletes video cells — or feature columns of `appearance_features` — instead
    (collate.perturb_cells; scores from appearance_attribution_scores, pixels set to `fill`) and serves Resnet3D, TransformerResnet and the
    fusion models through their forward_perturbed; "both" (the fusion models) ranks each modality on its own by the same method and
    removes the same fraction of each per step; a callable method then returns {"layout": ..., "appearance": ...}.  `head`: the logits
    the maps and the curves are read from (the fusion models; default the last of `logit_names`).  With `forward=` the reduced batches of
    "appearance" come from collate.perturb_cells, those of "both" from perturb_batch followed by perturb_cells on the same step."""
    from . import collate
    if modality not in ("layout", "appearance", "both"):
        raise StltHipError(f"modality: expected 'layout', 'appearance' or 'both', got {modality!r}")
    if target not in ("top1", "label"):
        raise StltHipError(f"target: expected 'top1' or 'label', got {target!r}")
    if not callable(method) and method not in _PERTURB_METHODS:
        raise StltHipError(f"method: expected one of {_PERTURB_METHODS} or a callable (model, batch) -> scores, got {method!r}")
    if method == "gradcam" and modality != "appearance":
        raise StltHipError(f"method 'gradcam' with modality {modality!r}: a class activation map lives on the positions of the convolutional trunk, the video's "
                           f"cells; the layout side has no convolution (use modality='appearance')")
    orders = tuple(orders)
    for o in orders:
        collate._perturb_args(o, unit)
    steps, _, _ = collate._step_range(steps)
    if hasattr(model, "train"):
        model.train(False)
    if forward is None:
        sides = getattr(model, "perturb_modalities", ("layout",))
        if modality != "layout" and "appearance" not in sides:
            raise StltHipError(f"modality {modality!r}: {type(model).__name__}.forward_perturbed deletes layout tokens only")
        if modality != "appearance" and "layout" not in sides:
            raise StltHipError(f"modality {modality!r}: {type(model).__name__} has the appearance side only")
    S = steps + 1
    if device is None and isinstance(model, torch.nn.Module):
        device = next((q.device for q in model.parameters()), None)
    batches = iter(batches)
    first = next(batches, None)
    if device is None:
        device = next((v.device for v in first.values() if isinstance(v, torch.Tensor)), "cpu") if first is not None else "cpu"
    device = torch.device(device)
    gen = torch.Generator(device=device).manual_seed(seed + rank) if method == "random" else None
    prob_sum = torch.zeros(len(orders), S, dtype=torch.float64, device=device)
    hit_sum = torch.zeros(len(orders), S, dtype=torch.int64, device=device)
    n_clips = torch.zeros(1, dtype=torch.int64, device=device)
    for batch in itertools.chain(() if first is None else (first,), batches):
        mine = D.shard_batch(batch, rank, world)
        mine = {k: (v.to(device) if isinstance(v, torch.Tensor) else v) for k, v in mine.items()}
        B = D.batch_size(mine)
        if B == 0:
            continue
        if callable(method) and modality == "both":
            both = method(model, mine)
            lay, app = both["layout"].to(torch.float32), both["appearance"].to(torch.float32)
        else:
            lay = attribution_scores(model, mine, method, gen, head).to(torch.float32) if modality != "appearance" else None
            app = appearance_attribution_scores(model, mine, method, gen, head).to(torch.float32) if modality != "layout" else None
        if unit == "frame" and lay is not None:
            lay = lay[:, :, 1:].sum(dim=2)
        scores = {"layout": lay.contiguous(), "appearance": app.contiguous()} if modality == "both" else (lay if modality == "layout" else app).contiguous()
        tgt = mine["labels"].to(torch.int64) if target == "label" else None
        for i, order in enumerate(orders):
            if forward is None:
                kw = dict(steps=steps, order=order, target=tgt, activation=activation)
                if "layout" in sides:
                    kw.update(unit=unit, dataset_name=dataset_name)
                if "appearance" in sides:
                    kw.update(modality=modality, fill=fill)
                if "both" in sides:
                    kw.update(head=head)
                out = model.forward_perturbed(mine, scores, **kw)
                prob, hit = out["prob"], out["hit"]
            else:
                pb = mine
                if modality != "appearance":
                    pb = collate.perturb_batch(pb, lay, steps=steps, order=order, unit=unit, dataset_name=dataset_name)
                if modality != "layout":
                    if modality == "both":  # step s of the layout meets step s of the appearance: the cells of each step's own clips
                        cells = collate.perturb_cells(mine, app, steps=steps, order=order, fill=fill)
                        key = collate.appearance_cells(mine)[0]
                        pb = dict(pb, **{key: cells[key]})
                    else:
                        pb = collate.perturb_cells(pb, app, steps=steps, order=order, fill=fill)
                logits = forward(pb)
                prob, hit, _ = perturb_curve(logits.reshape(S, B, -1), tgt, activation)
            prob_sum[i] += prob.sum(dim=1, dtype=torch.float64)
            hit_sum[i] += hit.sum(dim=1)
        n_clips += B
    packed = torch.cat([prob_sum.reshape(-1), hit_sum.reshape(-1).double(), n_clips.double()])  # counts are exact in fp64 below 2^53
    D.all_reduce_sum_(packed, world)
    packed = packed.cpu()
    n = int(packed[-1].item())
    fractions = [s / steps for s in range(S)]
    result: Dict[str, object] = {"fractions": fractions}
    trapezoid = lambda c: float((c.sum() - 0.5 * (c[0] + c[-1])) / steps)  # noqa: E731
    for i, order in enumerate(orders):
        p = packed[i * S:(i + 1) * S] / max(n, 1)
        a = packed[(len(orders) + i) * S:(len(orders) + i + 1) * S] / max(n, 1)
        result[order] = {"prob": p.tolist(), "accuracy": a.tolist(), "auc_prob": trapezoid(p), "auc_accuracy": trapezoid(a), "num_clips": n}
    return result
