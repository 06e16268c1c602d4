"""Drop-in ``CrossAttentionFusion`` (CAF), ``CrossAttentionCentralNetFusion`` (CACNF) and ``LateConcatenationFusion`` (LCF)
on PRECOMPUTED appearance features (reference src/modelling/models.py:230-271, 286-322, 328-549; BASELINE config 5).

Differences from the reference, by design of the scope:
  * by default the R3D-50 trunk is not part of the model: the batch carries ``appearance_features`` (B, 2048, 2, 4, 4) — what
    ``Resnet3D.forward_features`` returns — instead of ``video_frames``, and the state dict has every reference key EXCEPT
    ``…appearance_branch.resnet.*`` (load reference checkpoints with ``strict=False``).  ``MultimodalModelConfig(appearance_trunk=True)``
    adds the trunk (``modelling/resnet3d.py``) with the reference's 320 ``…resnet.*`` keys in their place (reference checkpoints then load
    with ``strict=True``); a batch with ``video_frames`` and no ``appearance_features`` runs it natively.  A frozen trunk runs without a
    tape and feeds the training composition below; a trainable one under autograd needs ``train_trunk=True`` (then its conv weights
    train through ``resnet3d.R3dTrunkFn``), else it is an error.  A batch whose ``video_frames`` (or ``appearance_features``) requires
    grad takes the differentiable composition as well, frozen model or not, and gets its gradient (the trunk through its tape path);
    ``forward_saliency`` is that composition as an inference call with the inputs as the only gradient targets;
  * inference is one native call (``stlt_caf_forward``).  Training — with autograd enabled and trainable parameters —
    composes the same arithmetic from the op-level autograd Functions of ``ops.py`` (native forward AND backward kernels
    per op: linear, attention, add+LayerNorm, GELU, the two embedding kernels); a frozen layout branch runs through the
    native forward without a tape, a trainable one through ``StltBackbone.forward_train``.  Dropout (reference
    models.py:333,341,350,358,368,376 and the appearance encoder's fixed 0.1) is the native counter-based mask everywhere
    (``ops.dropout`` at the post-attention / feed-forward sites, inside the attention kernel on the probabilities); the
    appearance encoder's ReLU runs in its product's epilogue.
As for STLT, the modules only hold parameters.
"""
from __future__ import annotations

import ctypes as C
from typing import Dict

import torch
from torch import nn

from .. import _lib as L
from .. import ops
from . import explain
from .configs import MultimodalModelConfig
from .models import (ClassificationHead, StltBackbone, _dev_ptr, _EncoderLayerParams, _EncoderStack, _layout_requires_grad, _prep_inputs, _SelfAttnParams,
                     _Workspace)
from .resnet3d import Resnet3D, inputs_only, video_saliency


class _AttnBlock(nn.Module):
    """SelfAttentionLayer / CrossAttentionLayer parameters: ``attn`` (MultiheadAttention) + ``ln`` (models.py:345-382)."""

    def __init__(self, config):
        super().__init__()
        self.attn = _SelfAttnParams(config.hidden_size)
        self.ln = nn.LayerNorm(config.hidden_size, eps=config.layer_norm_eps)

    def c_struct(self):
        ts = (self.attn.in_proj_weight, self.attn.in_proj_bias, self.attn.out_proj.weight, self.attn.out_proj.bias,
              self.ln.weight, self.ln.bias)
        return L.AttnBlockParams(*[_dev_ptr(t) for t in ts])


class FeedforwardModule(nn.Module):
    def __init__(self, config):
        super().__init__()
        self.linear1 = nn.Linear(config.hidden_size, config.hidden_size * 4)
        self.linear2 = nn.Linear(config.hidden_size * 4, config.hidden_size)
        self.ln = nn.LayerNorm(config.hidden_size, eps=config.layer_norm_eps)

    def c_struct(self):
        ts = (self.linear1.weight, self.linear1.bias, self.linear2.weight, self.linear2.bias, self.ln.weight, self.ln.bias)
        return L.FfnBlockParams(*[_dev_ptr(t) for t in ts])


class CrossModalModule(nn.Module):
    def __init__(self, config):
        super().__init__()
        self.cross_attn = _AttnBlock(config)
        self.layout_attn = _AttnBlock(config)
        self.layout_ffn = FeedforwardModule(config)
        self.appearance_attn = _AttnBlock(config)
        self.appearance_ffn = _AttnBlock(config)  # a SelfAttentionLayer in the reference (models.py:401)

    def c_struct(self):
        return L.CrossModalParams(self.cross_attn.c_struct(), self.layout_attn.c_struct(), self.appearance_attn.c_struct(),
                                  self.appearance_ffn.c_struct(), self.layout_ffn.c_struct())


class TransformerResnetFeatures(nn.Module):
    """``TransformerResnet`` (models.py:230-252): projector, CLS token, position table, ReLU encoder — and, with
    ``config.appearance_trunk``, the R3D-50 trunk as ``resnet`` (a native ``Resnet3D``, at the reference's key position)."""

    def __init__(self, config):
        super().__init__()
        d = config.hidden_size
        if getattr(config, "appearance_trunk", False):
            self.resnet = Resnet3D(config)
        self.projector = nn.Conv3d(2048, d, kernel_size=(1, 1, 1))
        self.transformer = _EncoderStack(_EncoderLayerParams(d), config.num_appearance_layers)
        self.cls_token = nn.Parameter(torch.zeros(1, 1, d))
        self.pos_embed = nn.Parameter(torch.zeros(config.appearance_num_frames + 1, 1, d))
        self.classifier = nn.Linear(d, config.num_classes)  # unused by CAF/CACNF, present in reference checkpoints


def _appearance_tokens(ab, feats, H: int, p: float):
    """projector, CLS token, position table and the ReLU encoder layers of TransformerResnet.forward_features (models.py:257-271) on the
    trunk's feature map (B, 2048, ...), batch-major (B, S+1, d), on the op-level native Functions."""
    return _appearance_layers(ab, _appearance_embed(ab, feats), H, p)


def _appearance_embed(ab, feats):
    """the encoder's input: projector, CLS token in front, position table (models.py:257-266) -> (B, S+1, d)"""
    B, Cc = feats.shape[0], feats.shape[1]
    d = ab.projector.weight.shape[0]
    x = ops.LinearFn.apply(feats.flatten(2).transpose(1, 2).contiguous(), ab.projector.weight.view(d, Cc), ab.projector.bias)
    return torch.cat((ab.cls_token.view(1, 1, d).expand(B, -1, -1), x), dim=1) + ab.pos_embed.view(1, -1, d)


def _appearance_layers(ab, x, H: int, p: float, n_layers=None):
    """the ReLU encoder layers (models.py:239-246, 267-271) on (B, S+1, d); ``n_layers``: the first so many only (default: all)"""
    for l in list(ab.transformer.layers)[:n_layers]:  # nn.TransformerEncoderLayer defaults: ReLU, post-norm, eps 1e-5, dropout 0.1
        sa = l.self_attn
        x = ops.AttnBlockFn.apply(x, None, None, False, H, 1e-5, p, sa.in_proj_weight, sa.in_proj_bias, sa.out_proj.weight, sa.out_proj.bias,
                                  l.norm1.weight, l.norm1.bias)
        x = ops.FfnBlockFn.apply(x, 1e-5, L.ACT_RELU, True, p, l.linear1.weight, l.linear1.bias, l.linear2.weight, l.linear2.bias,
                                 l.norm2.weight, l.norm2.bias)
    return x


def _appearance_requires_grad(batch: Dict[str, torch.Tensor]) -> bool:
    """The batch's video_frames or appearance_features are autograd leaves (or results) that want a gradient."""
    return any(isinstance(batch.get(k), torch.Tensor) and batch[k].requires_grad for k in ("video_frames", "appearance_features"))


def _trunk_path(owner: nn.Module, trunk: nn.Module) -> str:
    """the attribute path of the trunk's parameters for the error message (e.g. ``model.backbone.appearance_branch.resnet.resnet``)"""
    for name, m in owner.named_modules():
        if m is trunk:
            return f"….{name}.resnet" if name else "….resnet"
    return "….resnet"


class TransformerResnet(nn.Module):
    """``TransformerResnet`` (models.py:230-283) on ``video_frames``: the native R3D-50 trunk, then the projector, CLS token, position table
    and ReLU encoder on the native op-level Functions; ``forward(batch) -> {"resnet3d": classifier(CLS state)}``."""

    def __init__(self, config):
        super().__init__()
        d = config.hidden_size
        self.config = config
        self.resnet = Resnet3D(config)
        self.projector = nn.Conv3d(2048, d, kernel_size=(1, 1, 1))
        self.transformer = _EncoderStack(_EncoderLayerParams(d), config.num_appearance_layers)
        self.cls_token = nn.Parameter(torch.zeros(1, 1, d))
        self.pos_embed = nn.Parameter(torch.zeros(config.appearance_num_frames + 1, 1, d))
        self.classifier = nn.Linear(d, config.num_classes)
        self.logit_names = ("resnet3d",)

    perturb_modalities = ("appearance",)  # what forward_perturbed deletes from (infer.run_perturbation_test reads this)

    def forward_features(self, batch: Dict[str, torch.Tensor]) -> torch.Tensor:
        """(S+1, B, d), sequence-first like the reference's (models.py:271)"""
        feats = self.resnet._runner.run(self.resnet.resnet, batch["video_frames"], name="….resnet.resnet")[0]
        return _appearance_tokens(self, feats, self.config.num_attention_heads, 0.1 if self.training else 0.0).transpose(0, 1)

    def forward(self, batch: Dict[str, torch.Tensor]) -> Dict[str, torch.Tensor]:
        feats = self.resnet._runner.run(self.resnet.resnet, batch["video_frames"], name="….resnet.resnet")[0]
        x = _appearance_tokens(self, feats, self.config.num_attention_heads, 0.1 if self.training else 0.0)
        return {"resnet3d": ops.LinearFn.apply(x[:, 0].contiguous(), self.classifier.weight, self.classifier.bias)}

    def forward_saliency(self, batch: Dict[str, torch.Tensor], target=None) -> Dict[str, torch.Tensor]:
        """As Resnet3D.forward_saliency: {"resnet3d": logits, "target", "video_frames_grad": (B, 3, T, H, W)} from the input-only sweep of
        the op-level Functions and the trunk (no weight-gradient product, no parameter's ``.grad`` touched).  Inference call: training mode
        keeps the appearance encoder's dropout live and is refused."""
        if "video_frames" not in batch and "appearance_features" in batch:
            return self._feature_saliency(batch, target)
        return video_saliency(self, batch, target, "resnet3d", dropout_live=self.training)

    def _feature_saliency(self, batch: Dict[str, torch.Tensor], target, who: str = "forward_saliency") -> Dict[str, torch.Tensor]:
        """forward_saliency on a batch that carries the trunk's feature map as ``appearance_features`` (B, 2048, gt, gh, gw) instead of
        ``video_frames``: the layers above the trunk on the features as a leaf, input-only -> {"resnet3d", "target",
        "appearance_features_grad"}.  No trunk launch (forward_gradcam's head gradient)."""
        feats = batch["appearance_features"]
        explain.require_inference(who, dropout_live=self.training, tensors=(feats,))
        leaf = ops._chk(feats.contiguous(), torch.float32, "appearance_features").detach().requires_grad_(True)
        with inputs_only(self), torch.enable_grad():
            x = _appearance_tokens(self, leaf, self.config.num_attention_heads, 0.0)
            logits = ops.LinearFn.apply(x[:, 0].contiguous(), self.classifier.weight, self.classifier.bias)
            seed, target = explain.saliency_seed(logits, target, who)
            (g,) = torch.autograd.grad(logits, leaf, seed)
        return {"resnet3d": logits.detach(), "target": target, "appearance_features_grad": g}

    def _gradcam_head(self, feats, pooled, target, head):
        out = self.forward_saliency({"appearance_features": feats}, target=target)
        return {"resnet3d": out["resnet3d"]}, out["target"], out["appearance_features_grad"], None

    def forward_gradcam(self, batch: Dict[str, torch.Tensor], target=None, layer: int = 4, variant: str = "gradcam", relu: bool = True,
                        upsample: bool = False) -> Dict[str, torch.Tensor]:
        """As Resnet3D.forward_gradcam, the gradient at the feature map being ``appearance_features_grad`` of this model's own
        ``forward_saliency`` on the trunk's features as a leaf (the projector, the encoder and the classifier, input-only).  Training
        mode keeps the encoder's dropout live and is refused."""
        return explain.forward_gradcam(self, batch, target=target, layer=layer, variant=variant, relu=relu, upsample=upsample, dropout_live=self.training,
                                       trunk=(self.resnet._runner, self.resnet.resnet), head_gradient=self._gradcam_head)

    def forward_relevance(self, batch: Dict[str, torch.Tensor], target=None, return_layers: bool = False) -> Dict[str, torch.Tensor]:
        """The logits and the relevance of every appearance token for one raw logit per clip (the machinery of
        CrossAttentionFusion.forward_relevance on the appearance encoder alone): {"resnet3d": logits, "target", "appearance_rollout"
        (B,A,A), "appearance_relevance" (B,A) = appearance_rollout[:, 0, :] (the classifier reads the CLS token)}, with ``return_layers``
        also "appearance_layers" (n_app,B,A,A).  The trunk runs without a tape: relevance stops at the appearance tokens."""
        video = batch["video_frames"]
        explain.require_inference("forward_relevance", dropout_live=self.training, tensors=(video,))
        with torch.no_grad():
            x0 = _appearance_embed(self, self.resnet._runner.run(self.resnet.resnet, video, name="….resnet.resnet")[0])
        B, A = x0.shape[0], x0.shape[1]
        layers = torch.zeros(len(self.transformer.layers), B, A, A, device=x0.device, dtype=torch.float32)
        leaf = x0.detach().requires_grad_(True)
        with inputs_only(self), torch.enable_grad():
            with ops.RelevanceRecorder(list(layers)):
                x = _appearance_layers(self, leaf, self.config.num_attention_heads, 0.0)
                logits = ops.LinearFn.apply(x[:, 0].contiguous(), self.classifier.weight, self.classifier.bias)
            seed, target = explain.saliency_seed(logits, target, "forward_relevance")
            torch.autograd.grad(logits, leaf, seed)
        rollout = ops.attn_rollout(layers)
        out = {"resnet3d": logits.detach(), "target": target, "appearance_rollout": rollout, "appearance_relevance": rollout[:, 0, :].contiguous()}
        if return_layers:
            out["appearance_layers"] = layers
        return out

    def forward_perturbed(self, batch: Dict[str, torch.Tensor], scores: torch.Tensor, steps: int = 10, order: str = "descending", modality: str = "appearance",
                          target=None, steps_per_pass=None, fill: float = 0.0, activation: str = "softmax") -> Dict[str, torch.Tensor]:
        """As Resnet3D.forward_perturbed: the deletion test of a per-cell map (``appearance_relevance[:, 1:]``, pooled |video_frames_grad|,
        an attention row) on ``video_frames``; ``scores`` (B,A) lose their CLS column.  Training mode keeps the encoder's dropout live and
        is refused."""
        return explain.forward_perturbed(self, batch, scores, steps=steps, order=order, modality=modality, target=target, steps_per_pass=steps_per_pass, fill=fill,
                                         activation=activation, dropout_live=self.training, modalities=self.perturb_modalities)

    def forward_integrated_gradients(self, batch: Dict[str, torch.Tensor], target=None, steps: int = 16, baseline=None, steps_per_pass=None) -> Dict[str, torch.Tensor]:
        """As Resnet3D.forward_integrated_gradients, every pass being this model's own ``forward_saliency``.  Training mode keeps the
        encoder's dropout live and is refused."""
        return explain.forward_integrated_gradients(self, batch, target=target, steps=steps, baseline=baseline, steps_per_pass=steps_per_pass,
                                                    dropout_live=self.training, modalities=self.perturb_modalities, num_classes=self.classifier.weight.shape[0])

    def no_weight_decay(self):
        return {"pos_embed", "cls_token"}


class FusionHead(nn.Module):
    def __init__(self, config):
        super().__init__()
        self.fc1 = nn.Linear(config.hidden_size * 2, config.hidden_size)
        self.layer_norm = nn.LayerNorm(config.hidden_size, eps=config.layer_norm_eps)
        self.fc2 = nn.Linear(config.hidden_size, config.num_classes)


def _head_struct(h) -> "L.HeadParams":
    if h is None:
        return L.HeadParams()
    return L.HeadParams(*[_dev_ptr(t) for t in (h.fc1.weight, h.fc1.bias, h.layer_norm.weight, h.layer_norm.bias,
                                                h.fc2.weight, h.fc2.bias)])


class CrossAttentionFusionBackbone(nn.Module):
    def __init__(self, config: MultimodalModelConfig):
        super().__init__()
        self.config = config
        self.layout_branch = StltBackbone(config.stlt_config)
        self.appearance_branch = TransformerResnetFeatures(config)
        self.mm_fusion = nn.ModuleList([CrossModalModule(config) for _ in range(config.num_fusion_layers)])
        self._ws = _Workspace()

    def __getstate__(self):
        state = self.__dict__.copy()
        state["_ws"] = _Workspace()
        return state

    # ---- training path: op-level autograd over native kernels -------------------------------------------------
    @staticmethod
    def _lin(x, lin):
        return ops.LinearFn.apply(x, lin.weight, lin.bias)

    def _attn_block(self, blk: _AttnBlock, x, ctx, kpm, causal, p_drop):
        """SelfAttentionLayer (ctx is x) / CrossAttentionLayer, models.py:345-382: LN(dropout(MHA(x, ctx, ctx)) + x) — one native
        call each way (ops.AttnBlockFn)."""
        return ops.AttnBlockFn.apply(x, None if ctx is x else ctx, kpm, causal, self.config.num_attention_heads, self.config.layer_norm_eps,
                                     p_drop if self.training else 0.0, blk.attn.in_proj_weight, blk.attn.in_proj_bias, blk.attn.out_proj.weight,
                                     blk.attn.out_proj.bias, blk.ln.weight, blk.ln.bias)

    def _appearance_train(self, feats):
        """TransformerResnet.forward_features from the feature map on (models.py:257-271), batch-major (B, S+1, d)."""
        return _appearance_tokens(self.appearance_branch, feats, self.config.num_attention_heads, 0.1 if self.training else 0.0)

    def _features(self, batch: Dict[str, torch.Tensor]) -> torch.Tensor:
        """The appearance branch's input: ``appearance_features`` when the batch carries them, else (``appearance_trunk`` on) the native
        trunk on ``video_frames``, without a tape."""
        if "appearance_features" in batch:
            return ops._chk(batch["appearance_features"].contiguous(), torch.float32, "appearance_features")
        trunk = getattr(self.appearance_branch, "resnet", None)
        if trunk is None or "video_frames" not in batch:
            raise L.StltHipError("the batch needs `appearance_features` (or `video_frames` with MultimodalModelConfig(appearance_trunk=True))")
        return trunk._runner.run(trunk.resnet, batch["video_frames"], name=_trunk_path(self, trunk))[0]

    def _head_train(self, h, x):
        eps = self.config.layer_norm_eps
        z = ops.GeluFn.apply(self._lin(x.contiguous(), h.fc1))
        z = ops.AddLayerNormFn.apply(z, None, h.layer_norm.weight, h.layer_norm.bias, eps)
        return self._lin(z, h.fc2)

    def run_train(self, batch: Dict[str, torch.Tensor], fusion_head, layout_head=None, appearance_head=None):
        """Differentiable forward (see the module docstring).  -> same tuple as run()."""
        feats = self._features(batch)
        if any(q.requires_grad for q in self.layout_branch.parameters()) or _layout_requires_grad(batch):
            Lh = self.layout_branch.forward_train(batch)  # (B,T,d) with its autograd graph (op-level composition); boxes / scores get their gradients here
        else:  # frozen (load_backbone_path + freeze_backbone): one native call, no tape
            was_training = self.layout_branch.training
            self.layout_branch.train(False)
            with torch.no_grad():
                Lh = self.layout_branch.forward_batch_major(batch)
            self.layout_branch.train(was_training)
        return self._fuse_train(batch, Lh, self._appearance_train(feats), fusion_head, layout_head, appearance_head)

    def _fuse_train(self, batch, Lh, Ah, fusion_head, layout_head=None, appearance_head=None):
        """run_train from the two branches' states on: Lh (B,T,d) layout frames, Ah (B,A,d) appearance tokens -> the fusion layers and the heads"""
        B, d = Lh.shape[0], Lh.shape[2]
        # row lengths - 1 of every clip (models.py:455-459) as a gather: its backward is one scatter-add, where advanced indexing
        # (Lh[arange(B), last]) sorts the indices and runs six launches.  Only a NEGATIVE row wraps around, as indexing wraps it; a row beyond
        # the last frame stays out of range and the gather's bounds check fails loudly, as the reference's indexing raises IndexError
        last = batch["lengths"].to(Lh.device) - 1
        last = torch.where(last < 0, last + Lh.shape[1], last).view(B, 1, 1).expand(B, 1, d)
        lay_state, app_state = Lh.gather(1, last).squeeze(1), Ah[:, 0]
        kpm = batch["src_key_padding_mask_frames"]
        p = self.config.hidden_dropout_prob
        eps = self.config.layer_norm_eps
        for m in self.mm_fusion:  # CrossModalModule.forward, models.py:403-431
            la = self._attn_block(m.cross_attn, Lh, Ah, None, False, p)
            aa = self._attn_block(m.cross_attn, Ah, Lh, kpm, False, p)
            la = self._attn_block(m.layout_attn, la, la, kpm, True, p)
            aa = self._attn_block(m.appearance_attn, aa, aa, None, False, p)
            ff = m.layout_ffn
            Lh = ops.FfnBlockFn.apply(la, eps, L.ACT_GELU, False, p if self.training else 0.0, ff.linear1.weight, ff.linear1.bias, ff.linear2.weight,
                                      ff.linear2.bias, ff.ln.weight, ff.ln.bias)
            Ah = self._attn_block(m.appearance_ffn, aa, aa, None, False, p)
        fused = torch.cat((Lh.gather(1, last).squeeze(1), Ah[:, 0]), dim=-1)
        caf = self._head_train(fusion_head, fused)
        if layout_head is None:
            return (caf,)
        stlt = self._head_train(layout_head, lay_state)
        res = self._head_train(appearance_head, app_state)
        return caf, stlt, res, (stlt + res + caf) / 3

    def run(self, batch: Dict[str, torch.Tensor], fusion_head, layout_head=None, appearance_head=None):
        """-> (logits_caf, logits_stlt | None, logits_resnet3d | None, logits_ensemble | None)"""
        heads = [h for h in (fusion_head, layout_head, appearance_head) if h is not None]
        if torch.is_grad_enabled() and any(q.requires_grad for mod in [self] + heads for q in mod.parameters()):
            return self.run_train(batch, fusion_head, layout_head, appearance_head)
        if torch.is_grad_enabled() and _appearance_requires_grad(batch):  # pixel (or feature) gradients of a frozen model
            return self.run_train(batch, fusion_head, layout_head, appearance_head)
        if self.training and self.config.hidden_dropout_prob > 0:
            # train mode without grad: nn.Dropout is still live in the reference (models.py:334,351,376): the training
            # composition runs (its Functions just execute their forward kernels under no_grad)
            return self.run_train(batch, fusion_head, layout_head, appearance_head)
        lib = L.load()
        p, inp, keep, feats, (B, T, N, Cc, S, K) = self._native_args(batch, fusion_head, layout_head, appearance_head)
        device = feats.device
        nbytes = int(lib.stlt_caf_workspace_bytes(B, T, N, self.config.hidden_size, Cc, S, K))
        ws = self._ws.get(nbytes, device)
        outs = [torch.empty(B, K, device=device, dtype=torch.float32) for _ in range(4 if layout_head is not None else 1)]
        ptrs = [o.data_ptr() for o in outs] + [None] * (4 - len(outs))
        with torch.cuda.device(device):
            # layout_branch.skip_padding (as on a stand-alone StltBackbone): the layout branch on the real tokens / frames only
            flags = L.FLAG_SKIP_PADDING if self.layout_branch.skip_padding else 0
            L.check(lib.stlt_caf_forward_flags(C.byref(p), C.byref(inp), feats.data_ptr(), ws.data_ptr(), ws.numel(), flags, ptrs[0],
                                               ptrs[1], ptrs[2], ptrs[3], torch.cuda.current_stream().cuda_stream), "stlt_caf_forward")
        return outs

    def _dropout_live(self, appearance_encoder: bool = True) -> bool:
        """Would a forward in this mode draw a dropout mask?  Two rules stand side by side and are left as they are here.  run_saliency,
        run_relevance and run_perturbed (``appearance_encoder=True``) count the appearance encoder's fixed 0.1 dropout (models.py:239-246)
        next to ``hidden_dropout_prob``: any training-mode model with an appearance layer is refused.  run_attention
        (``appearance_encoder=False``) asks about ``hidden_dropout_prob`` alone, as ``run`` does when it picks the native call: in
        training mode with ``hidden_dropout_prob == 0`` it runs the inference kernels, which draw no mask.  Whether run_attention should
        refuse that case too is open; changing it changes what a model refuses."""
        return self.training and (self.config.hidden_dropout_prob > 0 or (appearance_encoder and len(self.appearance_branch.transformer.layers) > 0))

    @staticmethod
    def _named_logits(names, outs) -> Dict[str, torch.Tensor]:
        """run()'s tuple under the model's ``logit_names``: (caf,) as it is, (caf, stlt, res, ens) as ("stlt", "resnet3d", "caf", "ensemble")"""
        return dict(zip(names, (outs[1], outs[2], outs[0], outs[3]) if len(outs) == 4 else outs))

    def run_saliency(self, owner: nn.Module, names, batch: Dict[str, torch.Tensor], target, head, fusion_head, layout_head=None, appearance_head=None):
        """forward_saliency of the fusion models: run_train on private leaves of the batch's inputs — boxes, scores (when present) and
        video_frames or appearance_features — with every parameter of ``owner`` frozen (``inputs_only``), then one backward from the seeded
        head ``head`` of ``names`` to those leaves.  -> the dict forward_saliency returns."""
        explain.require_inference("forward_saliency", dropout_live=self._dropout_live(), tensors=(batch["categories"],))
        head = explain.pick_head("forward_saliency", names, head)
        app = "appearance_features" if "appearance_features" in batch else "video_frames"
        if app not in batch:
            raise L.StltHipError("the batch needs `appearance_features` (or `video_frames` with MultimodalModelConfig(appearance_trunk=True))")
        keys = ["boxes"] + (["scores"] if "scores" in batch else []) + [app]
        leaves = {k: batch[k].detach().requires_grad_(True) for k in keys}
        with inputs_only(owner), torch.enable_grad():
            outs = self.run_train(dict(batch, **leaves), fusion_head, layout_head, appearance_head)
            logits = self._named_logits(names, outs)
            seed, target = explain.saliency_seed(logits[head], target)
            grads = torch.autograd.grad(logits[head], [leaves[k] for k in keys], seed, allow_unused=True)
        out = {k: v.detach() for k, v in logits.items()}
        out["target"] = target
        for k, g in zip(keys, grads):
            out[k + "_grad"] = g if g is not None else torch.zeros_like(leaves[k])  # a head that does not read the input (CACNF's "stlt" and the video)
        return out

    RELEVANCE_WEIGHTS = {"stlt": (1.0, 0.0), "resnet3d": (0.0, 1.0)}  # (layout read-out row, appearance CLS row); every fused head: (1, 1)

    def run_relevance(self, owner: nn.Module, names, batch: Dict[str, torch.Tensor], target, head, return_layers: bool, fusion_head, layout_head=None,
                      appearance_head=None):
        """forward_relevance of the fusion models (include/stlt_hip.h: the attention relevance of the fusion models).  The layout branch runs
        on its native tape (stlt_train_forward with STLT_FLAG_TRAIN_BACKBONE, frozen or not); the appearance encoder, the fusion blocks and
        the heads on the op-level Functions over private leaves with every parameter of ``owner`` frozen and a recorder, so that each
        attention block's backward (stlt_attn_block_bwd_relevance) leaves its gradient-weighted map; one autograd.grad from the seeded head
        to the two leaves; the layout sweep (stlt_train_backward_relevance) from the layout leaf's gradient; then the appearance rollout,
        the joint rollout and the read-out.  -> the dict forward_relevance returns."""
        who = "forward_relevance"
        lb, ab = self.layout_branch, self.appearance_branch
        explain.require_inference(who, dropout_live=self._dropout_live(), tensors=(batch["categories"],))
        explain.require_inference(who, skip_padding=lb.skip_padding, skip_padding_attr="layout_branch")  # this call refuses CPU tensors first
        head = explain.pick_head(who, names, head)
        if "appearance_features" not in batch and "video_frames" not in batch:
            raise L.StltHipError("the batch needs `appearance_features` (or `video_frames` with MultimodalModelConfig(appearance_trunk=True))")
        H = self.config.num_attention_heads
        was_training = lb.training
        lb.train(False)
        try:
            with torch.no_grad():  # the trunk (when the batch carries video_frames) runs without a tape: relevance stops at the appearance tokens
                Lh, step = lb._train_forward(batch, None, L.FLAG_TRAIN_BACKBONE, stale=f"{who}: the layout branch ran another forward before the sweep")
                x0 = _appearance_embed(ab, self._features(batch))
        finally:
            lb.train(was_training)
        device = Lh.device
        B, T, A = Lh.shape[0], Lh.shape[1], x0.shape[1]
        n_app, n_fu = len(ab.transformer.layers), len(self.mm_fusion)
        zeros = lambda *shape: torch.zeros(*shape, device=device, dtype=torch.float32)  # noqa: E731  (a block the head never reaches keeps its zeros)
        layers = {"appearance_layers": zeros(n_app, B, A, A), "layout_to_appearance_layers": zeros(n_fu, B, T, A),
                  "appearance_to_layout_layers": zeros(n_fu, B, A, T), "fusion_layout_layers": zeros(n_fu, B, T, T),
                  "fusion_appearance_layers": zeros(n_fu, 2, B, A, A)}
        slots = list(layers["appearance_layers"])
        for l in range(n_fu):  # the order of _fuse_train's attention blocks (CrossModalModule.forward, models.py:403-431)
            slots += [layers["layout_to_appearance_layers"][l], layers["appearance_to_layout_layers"][l], layers["fusion_layout_layers"][l],
                      layers["fusion_appearance_layers"][l, 0], layers["fusion_appearance_layers"][l, 1]]
        lay_leaf, app_leaf = Lh.detach().requires_grad_(True), x0.detach().requires_grad_(True)
        with inputs_only(owner), torch.enable_grad():
            with ops.RelevanceRecorder(slots):
                outs = self._fuse_train(batch, lay_leaf, _appearance_layers(ab, app_leaf, H, 0.0), fusion_head, layout_head, appearance_head)
            logits = self._named_logits(names, outs)
            seed, target = explain.saliency_seed(logits[head], target, who)
            d_lay, _ = torch.autograd.grad(logits[head], [lay_leaf, app_leaf], seed, allow_unused=True)
        with torch.no_grad():
            maps = lb._train_relevance(step, torch.zeros_like(Lh) if d_lay is None else d_lay)  # (CACNF's "resnet3d" never reads the layout)
            app_rollout = ops.attn_rollout(layers["appearance_layers"])
            R = ops.attn_rollout_joint(maps["temporal_rollout"], app_rollout, layers["layout_to_appearance_layers"], layers["appearance_to_layout_layers"],
                                       layers["fusion_layout_layers"], layers["fusion_appearance_layers"])
            rel, frame_rel, app_rel = ops.relevance_combine_joint(R, maps["spatial_rollout"], batch["lengths"].to(device).contiguous(),
                                                                  *self.RELEVANCE_WEIGHTS.get(head, (1.0, 1.0)))
        out = {k: v.detach() for k, v in logits.items()}
        out.update(target=target, relevance=rel, frame_relevance=frame_rel, appearance_relevance=app_rel, fusion_rollout=R,
                   spatial_rollout=maps["spatial_rollout"], temporal_rollout=maps["temporal_rollout"], appearance_rollout=app_rollout)
        if return_layers:
            out.update(spatial_layers=maps["spatial_layers"], temporal_layers=maps["temporal_layers"], **layers)
        return out

    def run_perturbed(self, owner: nn.Module, batch, scores, **kw):
        """forward_perturbed of the fusion models (modelling/explain.py) with this backbone's answers: is dropout live, is there a trunk"""
        return explain.forward_perturbed(owner, batch, scores, dropout_live=self._dropout_live(), has_trunk=getattr(self.appearance_branch, "resnet", None) is not None, **kw)

    def run_integrated_gradients(self, owner: nn.Module, batch, **kw):
        """forward_integrated_gradients of the fusion models (modelling/explain.py) with this backbone's answers, as run_perturbed gives them"""
        return explain.forward_integrated_gradients(owner, batch, dropout_live=self._dropout_live(), modalities=explain.MODALITIES, takes_head=True,
                                                    has_trunk=getattr(self.appearance_branch, "resnet", None) is not None, **kw)

    def run_gradcam(self, owner: nn.Module, batch, **kw):
        """forward_gradcam of the fusion models (modelling/explain.py) with this backbone's answers: is dropout live, where is the trunk;
        the gradient at the feature map is ``appearance_features_grad`` of the owner's own ``forward_saliency`` on the batch with the
        features in place of the video"""
        trunk = getattr(self.appearance_branch, "resnet", None)
        rest = {k: v for k, v in batch.items() if k not in ("video_frames", "appearance_features")}

        def head_gradient(feats, pooled, target, head):
            out = owner.forward_saliency(dict(rest, appearance_features=feats), target=target, head=head)
            return {k: out[k] for k in owner.logit_names}, out["target"], out["appearance_features_grad"], None

        return explain.forward_gradcam(owner, batch, dropout_live=self._dropout_live(), trunk=None if trunk is None else (trunk._runner, trunk.resnet),
                                       head_gradient=head_gradient, takes_head=True, takes_features=True, **kw)

    def _native_args(self, batch, fusion_head, layout_head, appearance_head):
        """Marshal a batch and the parameters for the whole-path native calls (stlt_caf_forward_flags, stlt_caf_forward_attention):
        -> (stlt_caf_params, stlt_inputs, keep-alive, feature map, (B, T, N, feature channels, appearance tokens, classes))"""
        inp, keep, (B, T, N) = _prep_inputs(batch, need_lengths=True)
        feats = self._features(batch)
        ab = self.appearance_branch
        Cc = ab.projector.weight.shape[1]
        S = ab.pos_embed.shape[0] - 1
        if feats.shape[0] != B or feats.shape[1] != Cc or feats[0, 0].numel() != S:
            raise L.StltHipError(f"appearance_features must be (B, {Cc}, ...{S} positions), got {tuple(feats.shape)}")
        K = fusion_head.fc2.weight.shape[0]
        lay, sp, tp = self.layout_branch._build_struct(None, _dev_ptr)
        lay.n_classes = K
        app = (L.LayerParams * max(1, len(ab.transformer.layers)))(*[l.c_struct() for l in ab.transformer.layers])
        fus = (L.CrossModalParams * max(1, len(self.mm_fusion)))(*[m.c_struct() for m in self.mm_fusion])
        p = L.CafParams()
        p.layout = lay
        p.feat_channels, p.app_tokens = Cc, S
        p.proj_w, p.proj_b = _dev_ptr(ab.projector.weight), _dev_ptr(ab.projector.bias)
        p.cls_token, p.pos_embed = _dev_ptr(ab.cls_token), _dev_ptr(ab.pos_embed)
        p.n_app_layers, p.app_layers = len(ab.transformer.layers), app
        p.n_fusion, p.fusion = len(self.mm_fusion), fus
        p.fusion_head, p.layout_head, p.appearance_head = _head_struct(fusion_head), _head_struct(layout_head), _head_struct(appearance_head)
        return p, inp, (keep, sp, tp, app, fus), feats, (B, T, N, Cc, S, K)

    MAP_NAMES = ("spatial_attention", "temporal_attention", "appearance_attention", "layout_to_appearance", "appearance_to_layout",
                 "fusion_layout_attention", "fusion_appearance_attention")

    def run_attention(self, batch: Dict[str, torch.Tensor], per_head: bool, fusion_head, layout_head=None, appearance_head=None):
        """The native forward with every attention map (include/stlt_hip.h: stlt_caf_forward_attention), beside run().
        -> (logits as run() returns them, {map name: tensor} in the order of MAP_NAMES).  Inference only, dense padded schedule."""
        explain.require_inference("forward_attention", dropout_live=self._dropout_live(appearance_encoder=False), skip_padding=self.layout_branch.skip_padding,
                                  skip_padding_attr="layout_branch", tensors=(batch["categories"],))
        lib = L.load()
        p, inp, keep, feats, (B, T, N, Cc, S, K) = self._native_args(batch, fusion_head, layout_head, appearance_head)
        device = feats.device
        cfg = self.config
        H, A = cfg.num_attention_heads, S + 1
        n_sp, n_tp = len(self.layout_branch.frames_embeddings.layout_embedding.transformer.layers), len(self.layout_branch.transformer.layers)
        n_app, n_fu = len(self.appearance_branch.transformer.layers), len(self.mm_fusion)
        hs = (H,) if per_head else ()
        shapes = ((n_sp, B, T, *hs, N, N), (n_tp, B, *hs, T, T), (n_app, B, *hs, A, A), (n_fu, B, *hs, T, A), (n_fu, B, *hs, A, T),
                  (n_fu, B, *hs, T, T), (n_fu, 2, B, *hs, A, A))
        maps = [torch.empty(sh, device=device, dtype=torch.float32) for sh in shapes]
        sinks = L.CafAttentionMaps(*[(m.data_ptr() if m.numel() else None) for m in maps])
        ws = self._ws.get(int(lib.stlt_caf_attention_workspace_bytes(B, T, N, cfg.hidden_size, Cc, S, K)), device)
        outs = [torch.empty(B, K, device=device, dtype=torch.float32) for _ in range(4 if layout_head is not None else 1)]
        ptrs = [o.data_ptr() for o in outs] + [None] * (4 - len(outs))
        with torch.cuda.device(device):
            L.check(lib.stlt_caf_forward_attention(C.byref(p), C.byref(inp), feats.data_ptr(), ws.data_ptr(), ws.numel(), 0, int(bool(per_head)), ptrs[0],
                                                   ptrs[1], ptrs[2], ptrs[3], C.byref(sinks), torch.cuda.current_stream().cuda_stream),
                    "stlt_caf_forward_attention")
        return outs, dict(zip(self.MAP_NAMES, maps))


class CrossAttentionFusion(nn.Module):
    """CAF (models.py:486-498): ``forward(batch) -> {"caf": (B, num_classes)}``."""

    perturb_modalities = explain.MODALITIES  # what forward_perturbed deletes from (infer.run_perturbation_test reads this)

    def __init__(self, config: MultimodalModelConfig):
        super().__init__()
        self.caf_backbone = CrossAttentionFusionBackbone(config)
        self.classifier = FusionHead(config)
        self.logit_names = ("caf",)

    def forward(self, batch: Dict[str, torch.Tensor]):
        (caf,) = self.caf_backbone.run(batch, self.classifier)
        return {"caf": caf}

    @torch.no_grad()
    def forward_attention(self, batch: Dict[str, torch.Tensor], per_head: bool = False) -> Dict[str, torch.Tensor]:
        """The model's logits and the attention probabilities of every attention layer in one native pass (include/stlt_hip.h:
        stlt_caf_forward_attention): what the reference's nn.MultiheadAttention modules return with need_weights=True and its layers throw away.
        -> the logits under `logit_names`, and float32 maps averaged over the heads (A = appearance tokens + 1, token 0 the CLS token):
          spatial_attention (n_spatial,B,T,N,N), temporal_attention (n_temporal,B,T,T): the layout branch, as Stlt.forward_attention;
          appearance_attention (n_appearance,B,A,A): the appearance encoder;
          layout_to_appearance (n_fusion,B,T,A): which appearance token each layout frame attends to (models.py:411-414);
          appearance_to_layout (n_fusion,B,A,T): which layout frame each appearance token attends to, padded frames masked (415-419);
          fusion_layout_attention (n_fusion,B,T,T): layout_attn, causal + padding; fusion_appearance_attention (n_fusion,2,B,A,A):
          [:, 0] appearance_attn, [:, 1] appearance_ffn (a self-attention layer in the reference).
        With `per_head` the head axis H is inserted before the last two dimensions.  Index [..., i, j] is how much query i attends to key j;
        masked keys are exactly 0.  `layout_to_appearance[-1][b, lengths[b]-1]` is what clip b's read-out frame attends to in the video.
        Inference only, dense padded schedule: the logits equal `forward`'s to fp32 rounding, not bit for bit."""
        (caf,), maps = self.caf_backbone.run_attention(batch, per_head, self.classifier)
        return {"caf": caf, **maps}

    def forward_saliency(self, batch: Dict[str, torch.Tensor], target=None, head=None) -> Dict[str, torch.Tensor]:
        """The model's logits and the gradient of one raw logit per clip of head ``head`` (one of ``logit_names``; default the last) with
        respect to every input, in one pass: -> the logits under ``logit_names``, "target", "boxes_grad" (B, T, N, 4), "scores_grad"
        (B, T, N) when the batch has scores, and "video_frames_grad" (B, 3, T, H, W) (``appearance_trunk=True`` and ``video_frames``) or
        "appearance_features_grad" (the batch carries precomputed features; no trunk launch).  ``target`` as in Stlt.forward_saliency.
        Built on the op-level Functions with the inputs as the only gradient targets: no weight-gradient product, no parameter's
        ``.grad`` touched.  Inference call: training mode with live dropout is refused."""
        return self.caf_backbone.run_saliency(self, self.logit_names, batch, target, head, self.classifier)

    def forward_relevance(self, batch: Dict[str, torch.Tensor], target=None, head=None, return_layers: bool = False) -> Dict[str, torch.Tensor]:
        """The model's logits and how much of one raw logit per clip of head ``head`` (one of ``logit_names``; default the last) came through
        each layout frame, each object and each appearance token: gradient-weighted attention rollout (Chefer, Gur, Wolf 2021, the bi-modal
        rule without its row normalisation) over the T layout frames and A = appearance tokens + 1 (token 0 the CLS token) as one stacked
        token set of J = T + A, joint index t = frame t, T + a = appearance token a.  Every attention block contributes
        abar = mean over the heads of max(P * dLogit/dP, 0); the layout branch and the appearance encoder roll up on their own
        (R_l = R_{l-1} + abar_l R_{l-1}), the fusion layers continue from blockdiag(temporal_rollout, appearance_rollout) with three steps
        each (both cross-attention directions at once; layout_attn and appearance_attn; appearance_ffn), and the read-out row is
        R[b, lengths[b]-1] for the layout state plus R[b, T] for the appearance CLS state (head "stlt": the first only, "resnet3d": the second).
        ``target`` as in forward_saliency.
        -> the logits under ``logit_names``, "target", "relevance" (B,T,N) = frame_relevance x spatial_rollout[b,t,0,n], "frame_relevance"
        (B,T), "appearance_relevance" (B,A), "fusion_rollout" (B,J,J), "spatial_rollout" (B,T,N,N), "temporal_rollout" (B,T,T),
        "appearance_rollout" (B,A,A); with ``return_layers`` also "spatial_layers", "temporal_layers", "appearance_layers" (n_app,B,A,A),
        "layout_to_appearance_layers" (n_fusion,B,T,A), "appearance_to_layout_layers" (n_fusion,B,A,T), "fusion_layout_layers"
        (n_fusion,B,T,T), "fusion_appearance_layers" (n_fusion,2,B,A,A).  Entries of padded frames and padded object slots are exactly 0;
        the map of a block the head does not read is exactly 0.  With ``video_frames`` the trunk runs without a tape: relevance stops at the
        appearance tokens.  Inference call, padded schedule, N, T, A <= 256: no parameter's ``.grad`` is touched, two calls give the same bits."""
        return self.caf_backbone.run_relevance(self, self.logit_names, batch, target, head, return_layers, self.classifier)

    def forward_perturbed(self, batch: Dict[str, torch.Tensor], scores, steps: int = 10, order: str = "descending", modality: str = "appearance",
                          unit: str = "object", target=None, head=None, steps_per_pass=None, fill: float = 0.0, dataset_name: str = "something",
                          activation: str = "softmax") -> Dict[str, torch.Tensor]:
        """The perturbation test of an attribution map on this model (Chefer, Gur, Wolf 2021), on either modality or on both.
        modality "appearance": ``scores`` is (B,C) — one per cell of ``video_frames``, or per feature column of ``appearance_features``
        when the batch carries those (collate.perturb_cells says what a cell is and why the feature form is the weaker test) — or (B,A)
        token scores such as ``appearance_relevance``, whose CLS column is dropped; the cells are ranked (stlt_perturb_rank_cells), the
        first k = floor(s * C / steps) are set to ``fill`` for s = 0 .. steps (stlt_perturb_apply_cells), the layout is untouched.
        modality "layout": ``scores`` (B,T,N) for unit "object", (B,T) for "frame", exactly Stlt.forward_perturbed's deletion
        (stlt_perturb_rank / stlt_perturb_apply), the video untouched.  modality "both": ``scores`` = {"layout": ..., "appearance": ...};
        each modality is ranked on its own and step s removes the same fraction s / steps of each.  The ordinary ``forward`` runs on
        every reduced batch (``steps_per_pass`` steps per pass; default all S = steps+1 in one pass, which equals
        ``model(collate.perturb_cells(...))`` bit for bit), and one launch reads the curves off the logits of ``head`` (one of
        ``logit_names``; default the last).  -> the (S,B,K) logits under every logit name, "prob" (S,B), "hit" (S,B) bool, "auc" (B,),
        "target" (B,), "removed" (S,B) int32 and "n_candidates" (B,) — for "both": "removed_layout", "removed_appearance",
        "n_candidates_layout", "n_candidates_appearance".  ``target``, ``dataset_name`` and ``activation`` as in Stlt.forward_perturbed.
        ``layout_branch.skip_padding`` is honoured as ``forward`` honours it.  Inference only: refuses live dropout, CPU tensors, and
        ``video_frames`` without ``appearance_trunk=True``."""
        return self.caf_backbone.run_perturbed(self, batch, scores, steps=steps, order=order, modality=modality, unit=unit, target=target, head=head,
                                          steps_per_pass=steps_per_pass, fill=fill, dataset_name=dataset_name, activation=activation)

    def forward_gradcam(self, batch: Dict[str, torch.Tensor], target=None, layer: int = 4, variant: str = "gradcam", relu: bool = True, upsample: bool = False,
                        head=None) -> Dict[str, torch.Tensor]:
        """Grad-CAM / HiResCAM of one raw logit per clip of head ``head`` (one of ``logit_names``; default the last) at stage ``layer`` of
        the appearance trunk: Resnet3D.forward_gradcam, the gradient at the feature map being ``appearance_features_grad`` of this
        model's own ``forward_saliency`` on the features as a leaf.  ``layer=4`` works on the batch's ``appearance_features`` (no trunk
        launch) or on ``video_frames`` with ``appearance_trunk=True``; a stage below needs ``video_frames`` and the trunk, and a batch
        with only ``appearance_features`` is refused.  -> the logits under ``logit_names``, "target", "cam" (B, gt, gh, gw),
        "cell_attribution" (B, C), with ``upsample`` "video_cam" (B, T, H, W)."""
        return self.caf_backbone.run_gradcam(self, batch, target=target, layer=layer, variant=variant, relu=relu, upsample=upsample, head=head)

    def forward_integrated_gradients(self, batch: Dict[str, torch.Tensor], target=None, steps: int = 16, baseline=None, steps_per_pass=None, head=None,
                                     modality: str = "both") -> Dict[str, torch.Tensor]:
        """Integrated gradients (Sundararajan, Taly, Yan 2017) of one raw logit per clip of head ``head`` (one of ``logit_names``; default
        the last): Stlt.forward_integrated_gradients on either modality or on both.  ``modality`` says which inputs move along the path —
        "layout": boxes and scores; "appearance": ``appearance_features`` when the batch carries them, else ``video_frames``; "both" —; the
        others stay at the input and get no attribution key.  ``baseline``: None or a dict with any of "boxes" / "scores" /
        "video_frames" / "appearance_features" (the moved ones), each of the input's shape, dtype and device; a missing one is all zeros,
        for the video the dataset mean after Normalize(0.5, 0.5).  -> the logits at the input under ``logit_names``, "baseline_logits"
        (B,K) of ``head``, "target", "delta" (B,) over every moved input together, "<key>_attribution" per moved input,
        "object_attribution" (B,T,N) for the layout and "cell_attribution" (B,C) — the signed sum per cell of collate.appearance_cells
        (stlt_cell_pool_sum) — for the appearance side.  Every pass is this model's own ``forward_saliency`` on the path batch."""
        return self.caf_backbone.run_integrated_gradients(self, batch, target=target, steps=steps, baseline=baseline, steps_per_pass=steps_per_pass, head=head,
                                               modality=modality)


class CrossAttentionCentralNetFusion(nn.Module):
    """CACNF (models.py:501-549): ``forward(batch) -> {"stlt", "resnet3d", "caf", "ensemble"}``."""

    perturb_modalities = explain.MODALITIES  # what forward_perturbed deletes from (infer.run_perturbation_test reads this)

    def __init__(self, config: MultimodalModelConfig):
        super().__init__()
        self.config = config
        self.backbone = CrossAttentionFusionBackbone(config)
        self.layout_classifier = ClassificationHead(config)
        self.appearance_classifier = ClassificationHead(config)
        self.fusion_classifier = FusionHead(config)
        self.logit_names = ("stlt", "resnet3d", "caf", "ensemble")

    def forward(self, batch: Dict[str, torch.Tensor]):
        return self.backbone._named_logits(self.logit_names, self.backbone.run(batch, self.fusion_classifier, self.layout_classifier, self.appearance_classifier))

    @torch.no_grad()
    def forward_attention(self, batch: Dict[str, torch.Tensor], per_head: bool = False) -> Dict[str, torch.Tensor]:
        """As CrossAttentionFusion.forward_attention, with this model's four logits (include/stlt_hip.h: stlt_caf_forward_attention)."""
        outs, maps = self.backbone.run_attention(batch, per_head, self.fusion_classifier, self.layout_classifier, self.appearance_classifier)
        return {**self.backbone._named_logits(self.logit_names, outs), **maps}

    def forward_saliency(self, batch: Dict[str, torch.Tensor], target=None, head=None) -> Dict[str, torch.Tensor]:
        """As CrossAttentionFusion.forward_saliency with this model's four heads; an input the chosen head does not read gets zeros."""
        return self.backbone.run_saliency(self, self.logit_names, batch, target, head, self.fusion_classifier, self.layout_classifier,
                                          self.appearance_classifier)

    def forward_relevance(self, batch: Dict[str, torch.Tensor], target=None, head=None, return_layers: bool = False) -> Dict[str, torch.Tensor]:
        """As CrossAttentionFusion.forward_relevance with this model's four heads: "stlt" reads the layout branch alone and "resnet3d" the
        appearance encoder alone (every fusion map exactly 0), "caf" and "ensemble" both."""
        return self.backbone.run_relevance(self, self.logit_names, batch, target, head, return_layers, self.fusion_classifier, self.layout_classifier,
                                           self.appearance_classifier)

    def forward_perturbed(self, batch: Dict[str, torch.Tensor], scores, steps: int = 10, order: str = "descending", modality: str = "appearance",
                          unit: str = "object", target=None, head=None, steps_per_pass=None, fill: float = 0.0, dataset_name: str = "something",
                          activation: str = "softmax") -> Dict[str, torch.Tensor]:
        """As CrossAttentionFusion.forward_perturbed with this model's four heads (``head`` default "ensemble")."""
        return self.backbone.run_perturbed(self, batch, scores, steps=steps, order=order, modality=modality, unit=unit, target=target, head=head,
                                          steps_per_pass=steps_per_pass, fill=fill, dataset_name=dataset_name, activation=activation)

    def forward_gradcam(self, batch: Dict[str, torch.Tensor], target=None, layer: int = 4, variant: str = "gradcam", relu: bool = True, upsample: bool = False,
                        head=None) -> Dict[str, torch.Tensor]:
        """As CrossAttentionFusion.forward_gradcam with this model's four heads (``head`` default "ensemble"); a head that does not read the
        appearance side ("stlt") gives a zero gradient and a zero map."""
        return self.backbone.run_gradcam(self, batch, target=target, layer=layer, variant=variant, relu=relu, upsample=upsample, head=head)

    def forward_integrated_gradients(self, batch: Dict[str, torch.Tensor], target=None, steps: int = 16, baseline=None, steps_per_pass=None, head=None,
                                     modality: str = "both") -> Dict[str, torch.Tensor]:
        """As CrossAttentionFusion.forward_integrated_gradients with this model's four heads (``head`` default "ensemble"); an input the chosen head does not read gets zeros."""
        return self.backbone.run_integrated_gradients(self, batch, target=target, steps=steps, baseline=baseline, steps_per_pass=steps_per_pass, head=head,
                                               modality=modality)


class LateConcatenationFusion(nn.Module):
    """LCF (reference models.py:296-322): ``forward(batch) -> {"lcf": (B, num_classes)}`` — the FusionHead on the layout
    state at ``lengths-1`` concatenated with the appearance branch's CLS state.  That is the fusion backbone with zero
    cross-modal layers, so it runs through the same native entry point (``stlt_caf_forward``, ``n_fusion = 0``) and the same
    op-level training composition.  State-dict keys are the reference's (``layout_branch.*``, ``appearance_branch.*``,
    ``classifier.*``) minus ``…resnet.*``: the helper that owns the launch logic shares these modules without being
    registered as a child."""

    perturb_modalities = explain.MODALITIES  # what forward_perturbed deletes from (infer.run_perturbation_test reads this)

    def __init__(self, config: MultimodalModelConfig):
        super().__init__()
        self.config = config
        self.layout_branch = StltBackbone(config.stlt_config)
        self.appearance_branch = TransformerResnetFeatures(config)
        self.classifier = FusionHead(config)
        self.logit_names = ("lcf",)
        object.__setattr__(self, "_runner", self._make_runner())

    def _make_runner(self):
        r = CrossAttentionFusionBackbone.__new__(CrossAttentionFusionBackbone)
        nn.Module.__init__(r)
        r.config = self.config
        r.layout_branch, r.appearance_branch = self.layout_branch, self.appearance_branch  # shared, not copied
        r.mm_fusion = nn.ModuleList([])
        r._ws = _Workspace()
        return r

    def __getstate__(self):
        state = self.__dict__.copy()
        state.pop("_runner", None)
        return state

    def __setstate__(self, state):
        self.__dict__.update(state)
        object.__setattr__(self, "_runner", self._make_runner())

    def train(self, mode: bool = True):
        super().train(mode)
        self._runner.training = mode  # the runner is not a child: keep its mode flag (dropout switch) in step
        return self

    def forward(self, batch: Dict[str, torch.Tensor]):
        (lcf,) = self._runner.run(batch, self.classifier)
        return {"lcf": lcf}

    @torch.no_grad()
    def forward_attention(self, batch: Dict[str, torch.Tensor], per_head: bool = False) -> Dict[str, torch.Tensor]:
        """As CrossAttentionFusion.forward_attention; LCF has no cross-modal layers, so its four fusion maps have a leading dimension of 0."""
        (lcf,), maps = self._runner.run_attention(batch, per_head, self.classifier)
        return {"lcf": lcf, **maps}

    def forward_saliency(self, batch: Dict[str, torch.Tensor], target=None, head=None) -> Dict[str, torch.Tensor]:
        """As CrossAttentionFusion.forward_saliency."""
        return self._runner.run_saliency(self, self.logit_names, batch, target, head, self.classifier)

    def forward_relevance(self, batch: Dict[str, torch.Tensor], target=None, head=None, return_layers: bool = False) -> Dict[str, torch.Tensor]:
        """As CrossAttentionFusion.forward_relevance; LCF has no cross-modal layers, so "fusion_rollout" is the block-diagonal of the two
        branches' rollouts and the four fusion maps have a leading dimension of 0."""
        return self._runner.run_relevance(self, self.logit_names, batch, target, head, return_layers, self.classifier)

    def forward_perturbed(self, batch: Dict[str, torch.Tensor], scores, steps: int = 10, order: str = "descending", modality: str = "appearance",
                          unit: str = "object", target=None, head=None, steps_per_pass=None, fill: float = 0.0, dataset_name: str = "something",
                          activation: str = "softmax") -> Dict[str, torch.Tensor]:
        """As CrossAttentionFusion.forward_perturbed."""
        return self._runner.run_perturbed(self, batch, scores, steps=steps, order=order, modality=modality, unit=unit, target=target, head=head,
                                          steps_per_pass=steps_per_pass, fill=fill, dataset_name=dataset_name, activation=activation)

    def forward_gradcam(self, batch: Dict[str, torch.Tensor], target=None, layer: int = 4, variant: str = "gradcam", relu: bool = True, upsample: bool = False,
                        head=None) -> Dict[str, torch.Tensor]:
        """As CrossAttentionFusion.forward_gradcam."""
        return self._runner.run_gradcam(self, batch, target=target, layer=layer, variant=variant, relu=relu, upsample=upsample, head=head)

    def forward_integrated_gradients(self, batch: Dict[str, torch.Tensor], target=None, steps: int = 16, baseline=None, steps_per_pass=None, head=None,
                                     modality: str = "both") -> Dict[str, torch.Tensor]:
        """As CrossAttentionFusion.forward_integrated_gradients."""
        return self._runner.run_integrated_gradients(self, batch, target=target, steps=steps, baseline=baseline, steps_per_pass=steps_per_pass, head=head,
                                               modality=modality)


from .models import models_factory  # noqa: E402

models_factory["caf"] = CrossAttentionFusion
models_factory["cacnf"] = CrossAttentionCentralNetFusion
models_factory["lcf"] = LateConcatenationFusion
models_factory["resnet3d"] = Resnet3D
models_factory["resnet3d-transformer"] = TransformerResnet
