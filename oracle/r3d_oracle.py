"""CPU oracle for the R3D-50 trunk (reference src/modelling/resnets3d.py:58-214, ``generate_model(50)`` minus avgpool / fc, as
models.py:198-228 uses it).  TEST INFRASTRUCTURE ONLY: nothing in the package imports this file.

A plain-tensor restatement over a state dict under the package's keys (``resnet.0.weight``, ``resnet.4.0.conv1.weight``, ...):

  stem     Conv3d 7x7x7, stride (1, 2, 2), pad 3, no bias -> eval BatchNorm (eps 1e-5) -> ReLU -> MaxPool3d(3, stride 2, pad 1)
  layer1-4 Bottleneck blocks (3, 4, 6, 3), planes (64, 128, 256, 512): conv1 1x1x1 -> bn -> relu -> conv2 3x3x3 (stride 2 in the
           first block of layers 2-4, pad 1) -> bn -> relu -> conv3 1x1x1 (x4 channels) -> bn, + shortcut, relu; the first block of
           every layer has the type-B shortcut (Conv3d 1x1x1 with the block's stride -> bn)

BatchNorm always has eval semantics (Resnet3D.train keeps it so), which makes every clip independent: weight gradients are summed
over clips computed one at a time, about 2 GB per 32 x 112 x 112 clip in float64.
"""
from __future__ import annotations

from typing import Dict, List, Optional

import torch
import torch.nn.functional as F

BLOCKS = (3, 4, 6, 3)
PLANES = (64, 128, 256, 512)
BN_EPS = 1e-5
STAGES = ("stem", "layer1", "layer2", "layer3", "layer4")


def conv_prefixes(prefix: str = "resnet.") -> List[str]:
    """The 53 (conv, BatchNorm) key prefixes in state-dict order: stem, then per block conv1, conv2, conv3, [downsample]."""
    out = [(prefix + "0.", prefix + "1.")]
    for L, n in enumerate(BLOCKS):
        for b in range(n):
            blk = f"{prefix}{L + 4}.{b}."
            out += [(blk + "conv1.", blk + "bn1."), (blk + "conv2.", blk + "bn2."), (blk + "conv3.", blk + "bn3.")]
            if b == 0:
                out.append((blk + "downsample.0.", blk + "downsample.1."))
    return out


def conv_weight_keys(prefix: str = "resnet.") -> List[str]:
    return [c + "weight" for c, _ in conv_prefixes(prefix)]


def _bn(sd, p, x):
    return F.batch_norm(x, sd[p + "running_mean"], sd[p + "running_var"], sd[p + "weight"], sd[p + "bias"], training=False, eps=BN_EPS)


def trunk_forward(sd: Dict[str, torch.Tensor], video: torch.Tensor, prefix: str = "resnet.", stages: Optional[dict] = None) -> torch.Tensor:
    """video (B, 3, T, H, W) in sd's dtype -> features (B, 2048, To, Ho, Wo); ``stages``: filled with the five stage outputs."""
    x = F.conv3d(video, sd[prefix + "0.weight"], stride=(1, 2, 2), padding=3)
    x = F.max_pool3d(_bn(sd, prefix + "1.", x).relu(), kernel_size=3, stride=2, padding=1)
    if stages is not None:
        stages["stem"] = x
    for L, n in enumerate(BLOCKS):
        for b in range(n):
            blk = f"{prefix}{L + 4}.{b}."
            s = 2 if (L > 0 and b == 0) else 1
            y = _bn(sd, blk + "bn1.", F.conv3d(x, sd[blk + "conv1.weight"])).relu()
            y = _bn(sd, blk + "bn2.", F.conv3d(y, sd[blk + "conv2.weight"], stride=s, padding=1)).relu()
            y = _bn(sd, blk + "bn3.", F.conv3d(y, sd[blk + "conv3.weight"]))
            short = _bn(sd, blk + "downsample.1.", F.conv3d(x, sd[blk + "downsample.0.weight"], stride=s)) if b == 0 else x
            x = (y + short).relu()
        if stages is not None:
            stages[f"layer{L + 1}"] = x
    return x


def _cast(sd, dtype):
    return {k: (v.to(dtype) if v.is_floating_point() else v) for k, v in sd.items()}


def forward(sd: Dict[str, torch.Tensor], video: torch.Tensor, dtype=torch.float64, prefix: str = "resnet.", with_stages: bool = False,
            chunk: int = 4) -> dict:
    """-> {"features": (B, 2048, To, Ho, Wo), "pooled": (B, 2048)[, "stages": {name: (B, C, t, h, w)}]}, run in ``dtype``, ``chunk``
    clips at a time (no autograd)."""
    sdd = _cast(sd, dtype)
    feats, stages = [], {n: [] for n in STAGES}
    with torch.no_grad():
        for c in range(0, video.shape[0], chunk):
            st = {} if with_stages else None
            feats.append(trunk_forward(sdd, video[c:c + chunk].to(dtype), prefix, st))
            if with_stages:
                for n in STAGES:
                    stages[n].append(st[n])
    f = torch.cat(feats)
    out = {"features": f, "pooled": f.mean(dim=(2, 3, 4))}
    if with_stages:
        out["stages"] = {n: torch.cat(v) for n, v in stages.items()}
    return out


def weight_grads(sd: Dict[str, torch.Tensor], video: torch.Tensor, dtype=torch.float64, prefix: str = "resnet.",
                 dfeatures: Optional[torch.Tensor] = None, dpooled: Optional[torch.Tensor] = None, labels: Optional[torch.Tensor] = None,
                 classifier: str = "classifier.") -> dict:
    """Gradients of the 53 conv weights (state-dict order) of
        L = <features, dfeatures> + <pooled, dpooled> + cross_entropy(classifier(pooled), labels)   (each term only when given;
    the cross entropy is the batch mean, as nn.CrossEntropyLoss / the reference's Criterion("something") with one head)
    by torch autograd, one clip at a time, summed in clip order.  -> {"grads": [53 tensors], and with labels: "loss",
    "classifier.weight", "classifier.bias" (their gradients)}."""
    sdd = _cast(sd, dtype)
    keys = conv_weight_keys(prefix)
    B = video.shape[0]
    with_ce = labels is not None
    leaves = keys + ([classifier + "weight", classifier + "bias"] if with_ce else [])
    total = [torch.zeros_like(sdd[k]) for k in leaves]
    loss_sum = 0.0
    for b in range(B):
        params = {k: sdd[k].detach().clone().requires_grad_() for k in leaves}
        f = trunk_forward({**sdd, **params}, video[b:b + 1].to(dtype), prefix)
        pooled = f.mean(dim=(2, 3, 4))
        loss = f.new_zeros(())
        if dfeatures is not None:
            loss = loss + (f * dfeatures[b:b + 1].to(dtype)).sum()
        if dpooled is not None:
            loss = loss + (pooled * dpooled[b:b + 1].to(dtype)).sum()
        if with_ce:
            logits = F.linear(pooled, params[classifier + "weight"], params[classifier + "bias"])
            ce = F.cross_entropy(logits, labels[b:b + 1], reduction="sum") / B
            loss = loss + ce
            loss_sum += ce.item()
        grads = torch.autograd.grad(loss, [params[k] for k in leaves], allow_unused=True)
        for t, g in zip(total, grads):
            if g is not None:
                t += g
        del params, f, pooled, loss, grads
    out = {"grads": total[:len(keys)]}
    if with_ce:
        out["loss"] = loss_sum
        out[classifier + "weight"], out[classifier + "bias"] = total[len(keys):]
    return out
