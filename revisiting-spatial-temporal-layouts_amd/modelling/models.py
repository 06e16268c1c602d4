"""Drop-in ``StltBackbone`` / ``Stlt`` for the reference's ``src/modelling/models.py:16-195``.

Same constructor (``StltModelConfig``), same ``forward(batch: Dict[str, Tensor])`` signature and return
values, same 174 state-dict keys (168 for the backbone) — but the modules below only *store* parameters
(``nn.Parameter`` holders with torch's default initialisation).  All arithmetic runs in hand-written HIP
kernels for gfx950 through the C-ABI of ``libstlt_hip.so``; no ``torch.nn`` forward is ever called and
there is no CPU fallback (CPU tensors raise ``StltHipError``).
"""
from __future__ import annotations

import copy
import ctypes as C
import math
from typing import Dict, List, Optional

import torch
from torch import nn

from .. import _lib as L
from .. import ops
from . import explain
from .configs import StltModelConfig, model_configs_factory  # noqa: F401  (re-exported like the reference)

_ENC_EPS = 1e-5  # nn.TransformerEncoderLayer default; config.layer_norm_eps is not forwarded (models.py:46-52,118-124)


class _SelfAttnParams(nn.Module):
    """Parameter holder with nn.MultiheadAttention's names/shapes/init: in_proj_weight (3d,d) rows [q;k;v]."""

    def __init__(self, d: int):
        super().__init__()
        self.in_proj_weight = nn.Parameter(torch.empty(3 * d, d))
        self.in_proj_bias = nn.Parameter(torch.zeros(3 * d))
        self.out_proj = nn.Linear(d, d)
        nn.init.xavier_uniform_(self.in_proj_weight)
        nn.init.zeros_(self.out_proj.bias)


class _EncoderLayerParams(nn.Module):
    """Parameter holder with nn.TransformerEncoderLayer's 12 tensors (post-norm, gelu, dim_feedforward=4d)."""

    def __init__(self, d: int):
        super().__init__()
        self.self_attn = _SelfAttnParams(d)
        self.linear1 = nn.Linear(d, 4 * d)
        self.linear2 = nn.Linear(4 * d, d)
        self.norm1 = nn.LayerNorm(d, eps=_ENC_EPS)
        self.norm2 = nn.LayerNorm(d, eps=_ENC_EPS)

    def c_struct(self) -> L.LayerParams:
        sa = self.self_attn
        ts = (sa.in_proj_weight, sa.in_proj_bias, sa.out_proj.weight, sa.out_proj.bias, self.linear1.weight,
              self.linear1.bias, self.linear2.weight, self.linear2.bias, self.norm1.weight, self.norm1.bias,
              self.norm2.weight, self.norm2.bias)
        return L.LayerParams(*[_dev_ptr(t) for t in ts])


class _EncoderStack(nn.Module):
    """``nn.TransformerEncoder``'s container: ``layers`` are deep copies of one layer (same initial weights)."""

    def __init__(self, layer: _EncoderLayerParams, num_layers: int):
        super().__init__()
        self.layers = nn.ModuleList([copy.deepcopy(layer) for _ in range(num_layers)])


def _dev_ptr(t: torch.Tensor) -> int:
    if not t.is_cuda:
        raise L.StltHipError("STLT parameters must be on a GPU (`model.to('cuda')`): the hot path has no CPU fallback")
    if t.dtype != torch.float32 or not t.is_contiguous():
        raise L.StltHipError("STLT parameters must be contiguous float32")
    return t.data_ptr()


class CategoryBoxEmbeddings(nn.Module):
    """Parameters of reference models.py:16-27; forward = ``stlt_embed_fwd`` (K1)."""

    def __init__(self, config: StltModelConfig):
        super().__init__()
        self.category_embeddings = nn.Embedding(config.unique_categories, config.hidden_size, padding_idx=0)
        self.box_embedding = nn.Linear(4, config.hidden_size)
        self.score_embeddings = nn.Linear(1, config.hidden_size)
        self.layer_norm = nn.LayerNorm(config.hidden_size, eps=config.layer_norm_eps)
        self.eps = config.layer_norm_eps

    def forward(self, batch: Dict[str, torch.Tensor]) -> torch.Tensor:
        scores = batch["scores"].contiguous() if "scores" in batch else None
        return ops.embed(batch["categories"].contiguous(), batch["boxes"].contiguous(), scores,
                         self.category_embeddings.weight, self.box_embedding.weight, self.box_embedding.bias,
                         self.score_embeddings.weight, self.score_embeddings.bias, self.layer_norm.weight,
                         self.layer_norm.bias, self.eps)


class SpatialTransformer(nn.Module):
    """Parameters of reference models.py:42-55 (incl. the never-used ``encoder_layer`` the state dict carries)."""

    def __init__(self, config: StltModelConfig):
        super().__init__()
        self.category_box_embeddings = CategoryBoxEmbeddings(config)
        self.encoder_layer = _EncoderLayerParams(config.hidden_size)
        self.transformer = _EncoderStack(self.encoder_layer, config.num_spatial_layers)


class FramesEmbeddings(nn.Module):
    """Parameters of reference models.py:84-96."""

    def __init__(self, config: StltModelConfig):
        super().__init__()
        self.layout_embedding = SpatialTransformer(config)
        self.position_embeddings = nn.Embedding(config.layout_num_frames, config.hidden_size)
        self.frame_type_embedding = nn.Embedding(5, config.hidden_size, padding_idx=0)
        self.layer_norm = nn.LayerNorm(config.hidden_size, eps=config.layer_norm_eps)
        self.register_buffer("position_ids", torch.arange(config.layout_num_frames).expand((1, -1)))


class ClassificationHead(nn.Module):
    """Parameters of reference models.py:155-160; forward = fc2(LN(gelu(fc1(h)))) on the HIP kernels."""

    def __init__(self, config: StltModelConfig):
        super().__init__()
        self.fc1 = nn.Linear(config.hidden_size, config.hidden_size)
        self.layer_norm = nn.LayerNorm(config.hidden_size, eps=config.layer_norm_eps)
        self.fc2 = nn.Linear(config.hidden_size, config.num_classes)
        self.eps = config.layer_norm_eps

    def forward(self, hidden_state: torch.Tensor) -> torch.Tensor:
        h = ops.linear(hidden_state.contiguous(), self.fc1.weight, self.fc1.bias, act=L.ACT_GELU)
        h = ops.add_layernorm(h, None, self.layer_norm.weight, self.layer_norm.bias, self.eps)
        return ops.linear(h, self.fc2.weight, self.fc2.bias)


class _Workspace:
    """Grow-only scratch buffer per device, reused across forwards (the C-ABI never allocates)."""

    def __init__(self):
        self.buf: Optional[torch.Tensor] = None

    def get(self, nbytes: int, device) -> torch.Tensor:
        if self.buf is None or self.buf.device != device or self.buf.numel() < nbytes:
            self.buf = None
            self.buf = torch.empty(nbytes, dtype=torch.uint8, device=device)
        return self.buf


def _prep_inputs(batch: Dict[str, torch.Tensor], need_lengths: bool):
    """Validate the collated batch (reference src/modelling/datasets.py:243-288) and build the C struct."""
    cats = batch["categories"]
    if cats.dim() != 3:
        raise L.StltHipError(f"categories must be (B,T,N), got {tuple(cats.shape)}")
    B, T, N = cats.shape
    keep = []  # keep converted tensors alive until the launch is enqueued

    def take(t, dtype, name, shape):
        if tuple(t.shape) != shape:
            raise L.StltHipError(f"{name}: expected shape {shape}, got {tuple(t.shape)}")
        if dtype == torch.uint8:
            t = ops._mask_u8(t, name)
        else:
            t = ops._chk(t.contiguous(), dtype, name)
        keep.append(t)
        return t.data_ptr()

    inp = L.Inputs()
    inp.B, inp.T, inp.N = B, T, N
    inp.categories = take(cats, torch.int64, "categories", (B, T, N))
    inp.boxes = take(batch["boxes"], torch.float32, "boxes", (B, T, N, 4))
    inp.scores = take(batch["scores"], torch.float32, "scores", (B, T, N)) if "scores" in batch else None
    inp.kpm_boxes = take(batch["src_key_padding_mask_boxes"], torch.uint8, "src_key_padding_mask_boxes", (B, T, N))
    inp.frame_types = take(batch["frame_types"], torch.int64, "frame_types", (B, T))
    inp.kpm_frames = take(batch["src_key_padding_mask_frames"], torch.uint8, "src_key_padding_mask_frames", (B, T))
    inp.lengths = take(batch["lengths"], torch.int64, "lengths", (B,)) if need_lengths else None
    # optional: the batch's real rows, counted where the masks were made (collate.real_counts on the host).  With them a skip-padding
    # forward / training step reads nothing back from the device (include/stlt_hip.h: stlt_inputs.n_real_tokens)
    if "num_real_tokens" in batch or "num_real_frames" in batch:
        counts = []
        for key in ("num_real_tokens", "num_real_frames"):
            v = batch.get(key)
            if isinstance(v, torch.Tensor):
                if v.is_cuda:
                    raise L.StltHipError(f"{key} must be a host integer (a device tensor would have to be read back, which is what it is there to avoid)")
                v = int(v)
            if not isinstance(v, int) or v <= 0:
                raise L.StltHipError("num_real_tokens and num_real_frames come together, as positive host integers")
            counts.append(v)
        inp.n_real_tokens, inp.n_real_frames = counts
    return inp, keep, (B, T, N)


def _layout_requires_grad(batch: Dict[str, torch.Tensor]) -> bool:
    """The batch's boxes or scores are autograd leaves (or results) that want a gradient, as they may be in the reference."""
    return any(isinstance(batch.get(k), torch.Tensor) and batch[k].requires_grad for k in ("boxes", "scores"))


def _layout_grad_buffers(ctx_needs, batch, shape, device):
    """(d_boxes, d_scores) output buffers of stlt_train_backward_inputs for the gradients autograd asks for, (None, None) when it asks for
    neither.  The native call writes d_scores only beside d_boxes, so a scores-only request still allocates both."""
    B, T, N = shape
    want_b, want_s = bool(ctx_needs[0]), bool(ctx_needs[1]) and "scores" in batch
    if not (want_b or want_s):
        return None, None
    d_boxes = torch.empty(B, T, N, 4, device=device, dtype=torch.float32)
    d_scores = torch.empty(B, T, N, device=device, dtype=torch.float32) if want_s else None
    return d_boxes, d_scores


def _flat_grad_layout(params):
    """[(parameter, offset, numel)] of one flat fp32 gradient buffer and its length: offsets rounded up to 4 floats so each tensor stays
    16-byte aligned (the gaps stay zero)."""
    layout, off = [], 0
    for q in params:
        layout.append((q, off, q.numel()))
        off += (q.numel() + 3) // 4 * 4
    return layout, off


class StltBackbone(nn.Module):
    """Drop-in for reference ``StltBackbone`` (models.py:114-152): ``forward(batch) -> (T, B, d)``."""

    def __init__(self, config: StltModelConfig):
        super().__init__()
        if config.hidden_size % config.num_attention_heads != 0:
            raise AssertionError("embed_dim must be divisible by num_heads")
        self.config = config
        self.frames_embeddings = FramesEmbeddings(config)
        self.transformer = _EncoderStack(_EncoderLayerParams(config.hidden_size), config.num_temporal_layers)
        self.cls_only_last_spatial = True  # exact: only token 0 of the last spatial layer is read (models.py:79)
        self.last_row_only_temporal = True  # exact, Stlt.forward only: the head reads one row per clip (models.py:189-192)
        # Stlt.forward (inference and training), off by default: compute the real tokens / frames of the padded batch only.
        # Same logits (a padded row is masked as a key and never read); needs collater-shaped masks and costs one
        # stream synchronisation per call (include/stlt_hip.h: STLT_FLAG_SKIP_PADDING).
        self.skip_padding = False
        self._cache = None
        self._ws = _Workspace()

    def __getstate__(self):  # ctypes tables / scratch are rebuilt lazily; keep deepcopy / pickling working
        state = self.__dict__.copy()
        state["_cache"] = None
        state["_ws"] = _Workspace()
        state.pop("_train_bufs", None)
        state.pop("_flat_grad_buf", None)
        state.pop("_grad_table", None)
        return state

    @classmethod
    def from_pretrained(cls, config: StltModelConfig):
        model = cls(config)
        model.load_state_dict(torch.load(config.load_backbone_path, map_location="cpu"))
        return model

    # ---- parameter table for the C-ABI -------------------------------------------------------------
    def _apply(self, fn, *a, **kw):
        self._cache = None  # .to()/.cuda()/.float() move parameter storage
        self.__dict__.pop("_grad_table", None)
        return super()._apply(fn, *a, **kw)

    def _sentinel(self):
        """Identity of every parameter's storage: the cached C table holds raw device pointers, so rebinding any
        parameter (`p.data = …`, an EMA / SWA swap, pruning, replacing a Parameter) must rebuild it."""
        return tuple(q.data_ptr() for q in self.parameters())

    def _build_struct(self, head: Optional["ClassificationHead"], ptr):
        """Fill a stlt_params table; `ptr(tensor)` yields the device pointer to store for that parameter (its data
        for the forward tables, its gradient buffer — or None — for the backward's gradient table)."""
        cfg = self.config
        fe = self.frames_embeddings
        le = fe.layout_embedding
        cbe = le.category_box_embeddings

        def layer_struct(l):
            sa = l.self_attn
            ts = (sa.in_proj_weight, sa.in_proj_bias, sa.out_proj.weight, sa.out_proj.bias, l.linear1.weight,
                  l.linear1.bias, l.linear2.weight, l.linear2.bias, l.norm1.weight, l.norm1.bias, l.norm2.weight,
                  l.norm2.bias)
            return L.LayerParams(*[ptr(t) for t in ts])

        sp = (L.LayerParams * max(1, len(le.transformer.layers)))(*[layer_struct(l) for l in le.transformer.layers])
        tp = (L.LayerParams * max(1, len(self.transformer.layers)))(*[layer_struct(l) for l in self.transformer.layers])
        p = L.Params()
        p.d, p.H = cfg.hidden_size, cfg.num_attention_heads
        p.n_categories = cbe.category_embeddings.weight.shape[0]
        p.n_spatial, p.n_temporal = len(le.transformer.layers), len(self.transformer.layers)
        p.n_classes = 0 if head is None else head.fc2.weight.shape[0]
        p.n_positions = fe.position_embeddings.weight.shape[0]
        p.ln_eps = cfg.layer_norm_eps
        for name, t in (("cat_emb", cbe.category_embeddings.weight), ("box_w", cbe.box_embedding.weight),
                        ("box_b", cbe.box_embedding.bias), ("score_w", cbe.score_embeddings.weight),
                        ("score_b", cbe.score_embeddings.bias), ("emb_ln_w", cbe.layer_norm.weight),
                        ("emb_ln_b", cbe.layer_norm.bias), ("pos_emb", fe.position_embeddings.weight),
                        ("type_emb", fe.frame_type_embedding.weight), ("frames_ln_w", fe.layer_norm.weight),
                        ("frames_ln_b", fe.layer_norm.bias)):
            setattr(p, name, ptr(t))
        p.spatial, p.temporal = sp, tp
        if head is not None:
            for name, t in (("fc1_w", head.fc1.weight), ("fc1_b", head.fc1.bias), ("head_ln_w", head.layer_norm.weight),
                            ("head_ln_b", head.layer_norm.bias), ("fc2_w", head.fc2.weight), ("fc2_b", head.fc2.bias)):
                setattr(p, name, ptr(t))
        return p, sp, tp  # keep the layer arrays alive with the struct

    def c_params(self, head: Optional["ClassificationHead"] = None):
        key = (self._sentinel(), None if head is None else tuple(q.data_ptr() for q in head.parameters()))
        if self._cache is not None and self._cache[0] == key:
            return self._cache[1]
        self._cache = (key, self._build_struct(head, _dev_ptr))
        return self._cache[1]

    def _train_buf(self, name: str, nbytes: int, device) -> torch.Tensor:
        """Tape / scratch of the training step, allocated zero-filled and reused while the byte size matches.  Two batch
        shapes can round to the same size with different row layouts; the library does not rely on what an earlier step
        left behind: every step it clears the rows its weight-gradient products read beyond the row count (train.hip)."""
        bufs = self.__dict__.setdefault("_train_bufs", {})
        cur = bufs.get(name)
        if cur is None or cur.device != device or cur.numel() != nbytes:
            bufs[name] = cur = torch.zeros(nbytes, dtype=torch.uint8, device=device)
        return cur

    def _unused_param_ids(self, has_scores: bool):
        """ids of the parameters the forward never uses (they get no gradient, like in the reference: the dead `encoder_layer` copy, and
        `score_embeddings` when the batch has no scores — SURVEY.md §5)."""
        le = self.frames_embeddings.layout_embedding
        skip = {id(q) for q in le.encoder_layer.parameters()}
        if not has_scores:
            skip |= {id(q) for q in le.category_box_embeddings.score_embeddings.parameters()}
        return skip

    # ---- the native training step (csrc/train.hip), its two halves: what _StltTrainFn, _BackboneTrainFn and forward_saliency run ----
    def _train_forward(self, batch, head: Optional["ClassificationHead"], flags: int, seed_override=None, stale: str = ""):
        """stlt_train_forward into the backbone's one tape -> (output, step): the (B, num_classes) logits with a head, the (B,T,d) backbone
        output without one (flags: FLAG_TRAIN_BACKBONE); `step` is what `_train_backward` needs to run on that tape.  `stale`: what the
        backward says when a later forward has overwritten the tape."""
        lib = L.load()
        inp, keep, (B, T, N) = _prep_inputs(batch, need_lengths=True)
        device = batch["categories"].device
        p, _, _ = self.c_params(head)
        d = self.config.hidden_size
        tape = self._train_buf("tape", int(lib.stlt_train_tape_bytes(B, T, N, d, p.n_spatial, p.n_temporal)), device)
        # one tape per backbone: every forward overwrites it and takes a new generation number, and the backward refuses to run on a
        # tape that is no longer its own
        self._tape_gen = gen = getattr(self, "_tape_gen", 0) + 1
        out = torch.empty((B, T, d) if head is None else (B, head.fc2.weight.shape[0]), device=device, dtype=torch.float32)
        # train-mode dropout (reference default hidden_dropout_prob = 0.1): counter-based masks from one seed per
        # forward, drawn from torch's CPU generator (so torch.manual_seed makes runs repeatable)
        drop_p = float(self.config.hidden_dropout_prob) if self.training else 0.0
        seed = int(torch.randint(0, 2 ** 62, (1,)).item()) if drop_p > 0 else 0
        seed = seed_override or seed
        with torch.cuda.device(device):
            L.check(lib.stlt_train_forward(C.byref(p), C.byref(inp), tape.data_ptr(), tape.numel(), out.data_ptr(), drop_p, seed, flags,
                                           torch.cuda.current_stream().cuda_stream), "stlt_train_forward")
        # (the input table and the tensors it points into stay with the step, for the backward)
        return out, dict(gen=gen, stale=stale, inp=inp, keep=keep, shape=(B, T, N), device=device, head=head, drop=(drop_p, seed), flags=flags)

    def _check_tape(self, step):
        if getattr(self, "_tape_gen", 0) != step["gen"]:
            raise L.StltHipError(step["stale"])

    def _train_backward(self, step, g, dout, ctx_handle, d_boxes=None, d_scores=None, extra_flags: int = 0):
        """The reverse sweep of `step` from the seed `dout` into the gradient table `g` (and the layout gradients, when given):
        stlt_train_backward_inputs, which with neither layout gradient is stlt_train_backward.  (The autograd backwards also call
        `_check_tape` first thing, so that a refused backward has not touched a gradient buffer.)"""
        self._check_tape(step)
        lib = L.load()
        (B, T, N), device, d = step["shape"], step["device"], self.config.hidden_size
        p, _, _ = self.c_params(step["head"])
        tape = self._train_buf("tape", int(lib.stlt_train_tape_bytes(B, T, N, d, p.n_spatial, p.n_temporal)), device)
        scratch = self._train_buf("scratch", int(lib.stlt_train_scratch_bytes(B, T, N, d, p.n_categories)), device)
        dl = dout.contiguous().float()
        with torch.cuda.device(device):
            L.check(lib.stlt_train_backward_inputs(
                C.byref(p), C.byref(g), C.byref(step["inp"]), tape.data_ptr(), tape.numel(), scratch.data_ptr(), scratch.numel(), dl.data_ptr(),
                step["drop"][0], step["drop"][1], step["flags"] | extra_flags, ctx_handle, None if d_boxes is None else d_boxes.data_ptr(),
                None if d_scores is None else d_scores.data_ptr(), torch.cuda.current_stream().cuda_stream), "stlt_train_backward_inputs")

    def _train_relevance(self, step, dout, out=None):
        """stlt_train_backward_relevance on the tape of `step` from the seed `dout` -> the five maps (`out`: maps of an earlier call to
        write into again, e.g. under graph capture).  No gradient table, no context: the input-only sweep has no side stream.  On a tape
        of FLAG_TRAIN_BACKBONE (the fusion models' layout branch) `dout` is the (B,T,d) gradient of the backbone's output and there is no
        "relevance": the fusion model reads the rollouts out itself (ops.relevance_combine_joint)."""
        self._check_tape(step)
        lib = L.load()
        (B, T, N), device, d = step["shape"], step["device"], self.config.hidden_size
        p, _, _ = self.c_params(step["head"])
        tape = self._train_buf("tape", int(lib.stlt_train_tape_bytes(B, T, N, d, p.n_spatial, p.n_temporal)), device)
        scratch = self._train_buf("scratch", int(lib.stlt_train_scratch_bytes(B, T, N, d, p.n_categories)), device)
        dl = dout.contiguous().float()
        if out is None:
            new = lambda *shape: torch.empty(*shape, device=device, dtype=torch.float32)  # noqa: E731
            out = {"spatial_layers": new(p.n_spatial, B, T, N, N), "temporal_layers": new(p.n_temporal, B, T, T), "spatial_rollout": new(B, T, N, N),
                   "temporal_rollout": new(B, T, T)}
            if not step["flags"] & L.FLAG_TRAIN_BACKBONE:
                out["relevance"] = new(B, T, N)
        ptr = lambda t: t.data_ptr() if t is not None and t.numel() else None  # noqa: E731
        maps = L.RelevanceMaps(ptr(out["spatial_layers"]), ptr(out["temporal_layers"]), ptr(out["spatial_rollout"]), ptr(out["temporal_rollout"]),
                               ptr(out.get("relevance")))
        with torch.cuda.device(device):
            L.check(lib.stlt_train_backward_relevance(
                C.byref(p), C.byref(step["inp"]), tape.data_ptr(), tape.numel(), scratch.data_ptr(), scratch.numel(), dl.data_ptr(), step["drop"][0],
                step["drop"][1], step["flags"], None, C.byref(maps), torch.cuda.current_stream().cuda_stream), "stlt_train_backward_relevance")
        return out

    def _flags(self) -> int:
        return ((L.FLAG_CLS_ONLY_LAST_SPATIAL if self.cls_only_last_spatial else 0)
                | (L.FLAG_LAST_ROW_ONLY_TEMPORAL if self.last_row_only_temporal else 0)
                | (L.FLAG_SKIP_PADDING if self.skip_padding else 0))

    def _dropout_live(self) -> bool:
        """nn.Dropout is active whenever the module is in training mode, grad or no grad (models.py:27,37,93,109): such
        forwards take the training kernels (counter-based masks), not the inference schedule."""
        return self.training and self.config.hidden_dropout_prob > 0

    # ---- differentiable forward, composed from the op-level autograd Functions of ops.py ----------------------------
    def _encoder_layer_train(self, l: _EncoderLayerParams, x: torch.Tensor, kpm, causal: bool) -> torch.Tensor:
        """nn.TransformerEncoderLayer as configured at models.py:46-52,118-124 (post-norm, GELU, eps 1e-5) as two native
        block calls each way (attention half, feed-forward half; ops.AttnBlockFn / ops.FfnBlockFn), dropout with the native
        counter-based masks at the reference's four sites."""
        p, H = self.config.hidden_dropout_prob if self.training else 0.0, self.config.num_attention_heads
        sa = l.self_attn
        x = ops.AttnBlockFn.apply(x, None, kpm, causal, H, _ENC_EPS, p, sa.in_proj_weight, sa.in_proj_bias, sa.out_proj.weight, sa.out_proj.bias,
                                  l.norm1.weight, l.norm1.bias)
        return ops.FfnBlockFn.apply(x, _ENC_EPS, L.ACT_GELU, True, p, l.linear1.weight, l.linear1.bias, l.linear2.weight, l.linear2.bias,
                                    l.norm2.weight, l.norm2.bias)

    def forward_train(self, batch: Dict[str, torch.Tensor]) -> torch.Tensor:
        """(B,T,d) backbone output with an autograd graph: what a model that consumes EVERY row of the backbone (the fusion
        models) trains through.  `Stlt` itself trains through the single native reverse sweep instead (`_StltTrainFn`).
        Layouts of at most 256 frames / 256 object slots (the op-level attention backward streams keys above 64)."""
        if not self.skip_padding and "lengths" in batch:
            # one native tape forward / reverse sweep (csrc/train.hip with STLT_FLAG_TRAIN_BACKBONE): the last spatial layer
            # runs its out-proj / norms / FFN on the CLS rows only, weight gradients go out layer by layer in grouped launches
            return _BackboneTrainFn.apply(self, batch, batch["boxes"], batch.get("scores"), *tuple(self.parameters()))
        fe = self.frames_embeddings
        le = fe.layout_embedding
        cbe = le.category_box_embeddings
        cats = batch["categories"]
        B, T, N = cats.shape
        eps, p = self.config.layer_norm_eps, self.config.hidden_dropout_prob
        x = ops.EmbedFn.apply(cats, batch["boxes"], batch.get("scores"), cbe.category_embeddings.weight, cbe.box_embedding.weight,
                              cbe.box_embedding.bias, cbe.score_embeddings.weight, cbe.score_embeddings.bias, cbe.layer_norm.weight,
                              cbe.layer_norm.bias, eps)
        x = ops.dropout(x, p, self.training).view(B * T, N, -1)
        kpm_boxes = batch["src_key_padding_mask_boxes"].reshape(B * T, N)
        for l in le.transformer.layers:
            x = self._encoder_layer_train(l, x, kpm_boxes, False)
        cls_rows = x[:, 0].reshape(B, T, -1)  # models.py:79
        g = ops.FramesEmbedFn.apply(cls_rows, batch["frame_types"], fe.position_embeddings.weight, fe.frame_type_embedding.weight,
                                    fe.layer_norm.weight, fe.layer_norm.bias, eps)
        g = ops.dropout(g, p, self.training)
        kpm_frames = batch["src_key_padding_mask_frames"]
        for l in self.transformer.layers:
            g = self._encoder_layer_train(l, g, kpm_frames, True)
        return g

    def forward_batch_major(self, batch: Dict[str, torch.Tensor]) -> torch.Tensor:
        """HIP forward, batch-major (B,T,d) result (the layout the kernels compute in)."""
        if (torch.is_grad_enabled() and (any(q.requires_grad for q in self.parameters()) or _layout_requires_grad(batch))) or self._dropout_live():
            return self.forward_train(batch)  # under no_grad the op-level Functions just run their forward kernels
        out, = self._whole_path("stlt_backbone_forward", batch, None, ops.workspace_bytes, self._flags(),
                                lambda B, T, N, K, new: (new(B, T, self.config.hidden_size),))
        return out

    def _whole_path(self, entry: str, batch: Dict[str, torch.Tensor], head: Optional["ClassificationHead"], size_fn, flags: int, make_outputs, before=()):
        """Marshal a batch and make one whole-path native call: `entry`(params, inputs, workspace, bytes, flags, *before, *outputs, stream).
        `make_outputs(B, T, N, K, new)` allocates the call's float32 outputs with `new(*shape)`; they are returned as a tuple (an empty one
        — a tower without layers — reaches the library as NULL).  `head`: the prediction head whose logits the call produces (None: the
        backbone alone, which needs no lengths)."""
        lib = L.load()
        inp, keep, (B, T, N) = _prep_inputs(batch, need_lengths=head is not None)
        device = batch["categories"].device
        p, _, _ = self.c_params(head)
        K = head.fc2.weight.shape[0] if head is not None else 0
        ws = self._ws.get(size_fn(B, T, N, self.config.hidden_size, K), device)
        outs = make_outputs(B, T, N, K, lambda *shape: torch.empty(*shape, device=device, dtype=torch.float32))
        with torch.cuda.device(device):
            L.check(getattr(lib, entry)(C.byref(p), C.byref(inp), ws.data_ptr(), ws.numel(), flags, *before,
                                        *(o.data_ptr() if o.numel() else None for o in outs), torch.cuda.current_stream().cuda_stream), entry)
        return outs

    def forward(self, batch: Dict[str, torch.Tensor]) -> torch.Tensor:
        # [Num. frames, Batch size, Hidden size] like the reference (a transposed view of the batch-major result)
        return self.forward_batch_major(batch).transpose(0, 1)


class Stlt(nn.Module):
    """Drop-in for reference ``Stlt`` (models.py:166-195): ``forward(batch) -> {"stlt": (B, num_classes)}``."""

    def __init__(self, config: StltModelConfig):
        super().__init__()
        self.config = config
        if config.load_backbone_path is not None:
            self.backbone = StltBackbone.from_pretrained(config)
            if config.freeze_backbone:
                for param in self.backbone.parameters():
                    param.requires_grad = False
        else:
            self.backbone = StltBackbone(config)
        self.prediction_head = ClassificationHead(config)
        self.logit_names = ("stlt",)

    perturb_modalities = ("layout",)  # what forward_perturbed deletes from (infer.run_perturbation_test reads this)

    def _own_context(self):
        """The module's own training context (include/stlt_hip.h: stlt_ctx), made at the first autograd backward that runs outside a
        Trainer step: it owns the side stream of that sweep's weight-gradient products.  Not a parameter, not in the state dict."""
        c = self.__dict__.get("_ctx_own")
        if c is None or c.handle is None:
            c = self.__dict__["_ctx_own"] = ops.TrainContext()
        return c

    def train(self, mode: bool = True):
        super().train(mode)
        if self.config.load_backbone_path and self.config.freeze_backbone:
            self.backbone.train(False)
        return self  # the reference returns None here; returning self is a superset

    def _grad_params(self, has_scores: bool):
        """ids of the parameters the forward actually uses (StltBackbone._unused_param_ids names the others)."""
        return {id(q) for q in self.parameters()} - self.backbone._unused_param_ids(has_scores)

    def forward(self, batch: Dict[str, torch.Tensor]) -> Dict[str, torch.Tensor]:
        bb = self.backbone
        grad_path = torch.is_grad_enabled() and (any(q.requires_grad for q in self.parameters()) or _layout_requires_grad(batch))
        if grad_path or bb._dropout_live():
            # train mode without grad (a validation pass that forgot model.train(False), MC-dropout): the reference still
            # applies its dropouts, so the training forward runs here too — same kernels, the tape is just not kept
            params = tuple(self.parameters())
            logits = _StltTrainFn.apply(self, batch, batch["boxes"], batch.get("scores"), *params)
            return {k: v for k, v in zip(self.logit_names, (logits,))}
        logits = bb._whole_path("stlt_forward", batch, self.prediction_head, ops.workspace_bytes, bb._flags(),
                                lambda B, T, N, K, new: (new(B, K),), before=(None,))  # no (B,T,d) backbone output
        return {k: v for k, v in zip(self.logit_names, logits)}


    @torch.no_grad()
    def forward_prefixes(self, batch: Dict[str, torch.Tensor]) -> Dict[str, torch.Tensor]:
        """The model's logits after every number of observed frames, in one pass (include/stlt_hip.h: stlt_forward_prefixes).
        -> {"stlt": (B, T, num_classes) float32, "valid": (B, T) bool}.  `valid[b, t] = t < lengths[b]`; for valid entries `stlt[b, t]` is
        what `forward` returns for `collate.prefix_batch(batch, t)` — frames 0 .. t-1 of the clip followed by its own extract frame — so
        `stlt[b, lengths[b]-1]` is the ordinary forward's logits; invalid entries are 0.  Inference only, padded schedule."""
        bb = self.backbone
        explain.require_inference("forward_prefixes", dropout_live=bb._dropout_live(), skip_padding=bb.skip_padding)
        logits, = bb._whole_path("stlt_forward_prefixes", batch, self.prediction_head, ops.prefix_workspace_bytes, bb._flags(),
                                 lambda B, T, N, K, new: (new(B, T, K),))
        valid = torch.arange(logits.shape[1], device=logits.device)[None, :] < batch["lengths"].to(logits.device)[:, None]
        return {"stlt": logits, "valid": valid}


    @torch.no_grad()
    def forward_attention(self, batch: Dict[str, torch.Tensor], per_head: bool = False) -> Dict[str, torch.Tensor]:
        """The model's logits and every layer's attention probabilities in one pass (include/stlt_hip.h: stlt_forward_attention): what
        the reference's nn.MultiheadAttention layers return with need_weights=True.
        -> {"stlt": (B, num_classes), "spatial_attention": (n_spatial, B, T, N, N), "temporal_attention": (n_temporal, B, T, T)} float32,
        averaged over the heads; with `per_head` the maps are (n_spatial, B, T, H, N, N) and (n_temporal, B, H, T, T).  Index [layer, ..., i, j]
        is how much query i attends to key j; masked keys are exactly 0.
        `spatial_attention[-1][:, :, 0, :]` is what each frame's CLS token attends to among the frame's objects;
        `temporal_attention[-1][b, lengths[b]-1]` is what clip b's read-out (extract) token attends to among its frames.
        Rows of padded tokens hold the reference's values for them: mask them with the batch's `src_key_padding_mask_boxes` /
        `src_key_padding_mask_frames`.  Inference only, dense padded schedule: every layer runs on every row as the unfused pair, so the
        logits equal `forward`'s to fp32 rounding, not bit for bit."""
        bb = self.backbone
        explain.require_inference("forward_attention", dropout_live=bb._dropout_live(), skip_padding=bb.skip_padding, tensors=(batch["categories"],))
        H, n_sp, n_tp = self.config.num_attention_heads, self.config.num_spatial_layers, self.config.num_temporal_layers
        def maps(B, T, N, K, new):
            return (new(B, K), new((n_sp, B, T, H, N, N) if per_head else (n_sp, B, T, N, N)), new((n_tp, B, H, T, T) if per_head else (n_tp, B, T, T)))
        outs = bb._whole_path("stlt_forward_attention", batch, self.prediction_head, ops.attention_workspace_bytes, 0, maps, before=(int(bool(per_head)),))
        return dict(zip(("stlt", "spatial_attention", "temporal_attention"), outs))

    _logit_seed = staticmethod(explain.logit_seed)  # the seed of a saliency / relevance pass under its earlier name (tests/test_relevance_gpu.py calls it)

    @torch.no_grad()
    def forward_saliency(self, batch: Dict[str, torch.Tensor], target=None) -> Dict[str, torch.Tensor]:
        """The model's logits and the gradient of one raw logit per clip with respect to the layout, in one pass: which object's
        position (and detection score) the prediction depends on.  What the reference gives for `boxes.requires_grad_()` followed by
        `logits[b, target[b]].backward()` (models.py:29-39, 166-195), without autograd: stlt_train_forward with dropout 0,
        stlt_saliency_seed, then stlt_train_backward_inputs with a gradient table of NULLs — the input-only sweep (no weight-gradient
        product, no parameter reduction, no side stream).
        -> {"stlt": (B, num_classes) float32 logits, "target": the selected classes, "boxes_grad": (B, T, N, 4) float32,
            "scores_grad": (B, T, N) float32 — only when the batch has scores}.
        `target`: None — each clip's top-1 class ("target" is then the (B,) int64 device tensor of those classes); an int64 (B,) tensor —
        that class per clip; a float (B, num_classes) tensor — used as the seed d(objective)/d(logits) itself (a multi-hot row for Action
        Genome, or any weighting), returned as given.  The gradients are of the raw logit, not of a loss.  Entries of padded object slots
        and of padded frames are exactly 0.  Works with `backbone.skip_padding` on and off; reads nothing back from the device (with
        skip_padding: when the batch carries num_real_tokens / num_real_frames).  Inference only: touches no parameter's .grad.  It runs
        on the backbone's one activation tape, so an autograd backward still pending from an earlier forward refuses to run afterwards."""
        bb = self.backbone
        explain.require_inference("forward_saliency", dropout_live=bb._dropout_live(), tensors=(batch["categories"],))
        device = batch["categories"].device
        head = self.prediction_head
        B = batch["categories"].shape[0]
        tgt, seed = explain.parse_target("forward_saliency", target, B, head.fc2.weight.shape[0], device)  # a bad target is refused before the tape is overwritten
        # (dropout is off here, so the forward draws no seed; the tape is overwritten: a pending backward of an earlier forward will refuse)
        logits, step = bb._train_forward(batch, head, L.FLAG_SKIP_PADDING if bb.skip_padding else 0)
        _, T, N = step["shape"]
        g, gsp, gtp = bb._build_struct(head, lambda t: None)
        new = lambda *shape: torch.empty(*shape, device=device, dtype=torch.float32)  # noqa: E731
        d_boxes = new(B, T, N, 4)
        d_scores = new(B, T, N) if "scores" in batch else None
        seed = explain.logit_seed(logits, tgt, seed)
        bb._train_backward(step, g, seed, None, d_boxes, d_scores)
        if target is None:
            target = seed.argmax(dim=1)  # the one-hot row's only 1: the class the kernel picked (lowest index on ties), still on the device
        out = {"stlt": logits, "target": target, "boxes_grad": d_boxes}
        if d_scores is not None:
            out["scores_grad"] = d_scores
        return out

    @torch.no_grad()
    def forward_relevance(self, batch: Dict[str, torch.Tensor], target=None, return_layers: bool = False) -> Dict[str, torch.Tensor]:
        """The model's logits and the relevance of every object of every frame for one logit per clip, in one pass: which object, in which
        frame, the prediction rests on.  Gradient-weighted attention rollout (Chefer, Gur, Wolf 2021): each layer's attention probabilities
        are weighted by the gradient of the target logit with respect to them, the positive part is averaged over the heads
        (stlt_attn_grad_probs), and the layers are rolled up through the residual connections, R_l = R_{l-1} + abar_l·R_{l-1}
        (stlt_attn_rollout); the relevance joins the two towers, relevance[b,t,n] = temporal_rollout[b, lengths[b]-1, t] *
        spatial_rollout[b,t,0,n] (stlt_relevance_combine).  On the reference this takes need_weights=True, hooks and retain_grad on every
        layer and a Python loop; here it is stlt_train_forward with dropout 0, stlt_saliency_seed and stlt_train_backward_relevance: the
        input-only sweep with one extra launch per layer.
        -> {"stlt": (B, num_classes) float32 logits, "target": the selected classes, "relevance": (B, T, N), "spatial_rollout": (B, T, N, N),
            "temporal_rollout": (B, T, T)}; with `return_layers` also the per-layer maps "spatial_layers": (n_spatial, B, T, N, N) and
            "temporal_layers": (n_temporal, B, T, T).
        `target` as in forward_saliency: None — each clip's top-1 class; an int64 (B,) tensor; a float (B, num_classes) seed.  Entries of
        padded object slots and of padded frames of "relevance" are exactly 0.  Padded schedule only (N, T <= 256).  Inference only: touches
        no parameter's .grad.  Like forward_saliency it runs on the backbone's one activation tape, so an autograd backward still pending
        from an earlier forward refuses to run afterwards."""
        bb = self.backbone
        explain.require_inference("forward_relevance", dropout_live=bb._dropout_live(), skip_padding=bb.skip_padding, tensors=(batch["categories"],))
        cats = batch["categories"]
        tgt, seed = explain.parse_target("forward_relevance", target, cats.shape[0], self.prediction_head.fc2.weight.shape[0], cats.device)
        logits, step = bb._train_forward(batch, self.prediction_head, 0)
        seed = explain.logit_seed(logits, tgt, seed)
        maps = bb._train_relevance(step, seed)
        if target is None:
            target = seed.argmax(dim=1)
        out = {"stlt": logits, "target": target, "relevance": maps["relevance"], "spatial_rollout": maps["spatial_rollout"],
               "temporal_rollout": maps["temporal_rollout"]}
        if return_layers:
            out["spatial_layers"], out["temporal_layers"] = maps["spatial_layers"], maps["temporal_layers"]
        return out

    @torch.no_grad()
    def forward_perturbed(self, batch: Dict[str, torch.Tensor], scores: torch.Tensor, steps: int = 10, order: str = "descending", unit: str = "object",
                          target=None, steps_per_pass: Optional[int] = None, dataset_name: str = "something", activation: str = "softmax") -> Dict[str, torch.Tensor]:
        """The perturbation test of an attribution map on this model (Chefer, Gur, Wolf 2021): the clips' object tokens (unit "object",
        scores (B,T,N)) or frames (unit "frame", scores (B,T)) are ranked by `scores` (include/stlt_hip.h: stlt_perturb_rank), the first
        k = floor(s * n_candidates / steps) of the removal order are deleted for s = 0 .. steps (stlt_perturb_apply — a deleted slot is a
        slot without a detection as the reference's dataset and collater make it, datasets.py:64-69, 88-93, 274-278), the ordinary
        `forward` runs on every reduced batch, and one launch reads the curves off the logits (stlt_perturb_curve).  order "descending"
        deletes the highest-scored first (a faithful map makes the target's probability fall fast), "ascending" the lowest-scored first
        (it should stay flat).  -> {"stlt": (S,B,K) float32 logits with S = steps+1, "prob": (S,B) the target class's softmax probability,
        "hit": (S,B) bool — the target is still the prediction, "auc": (B,) the trapezoid of prob over the steps divided by `steps`,
        "target": (B,) int64, "removed": (S,B) int32 — k per step and clip, "n_candidates": (B,) int32}.
        `target`: None — each clip's top-1 class on the unperturbed batch (step 0) — or an int64 (B,) tensor.  steps_per_pass: how many
        steps one forward holds (default: all S, one forward on S*B clips; 1: S forwards on B clips).  Works with `backbone.skip_padding` on
        and off; num_real_tokens / num_real_frames of the batch are carried as upper bounds (no read-back).  `dataset_name` names the frame
        type "empty"; activation "sigmoid" (Action Genome's multi-label head) makes prob the target's sigmoid and hit "its logit is positive".
        Inference only: refuses live dropout and CPU tensors, as forward_saliency does."""
        bb, head = self.backbone, self.prediction_head
        # this call refuses CPU tensors ahead of its argument checks (the shared routine: behind them), and scores that are not float32 and
        # contiguous, as ops.perturb_rank does (the shared routine converts what the fusion models are handed): both stay as they were
        explain.require_inference("forward_perturbed", dropout_live=bb._dropout_live(), tensors=(batch["categories"], scores), holder="the batch or the scores hold")
        scores = ops._chk(scores, torch.float32, "scores")
        K = head.fc2.weight.shape[0]

        def run_pass(part, s0, s1, logits):
            """stlt_forward writes the pass's logits straight into rows s0 .. s1 of the (S,B,K) result: no copy launch"""
            if logits is None:
                logits = {"stlt": torch.empty(int(steps) + 1, batch["categories"].shape[0], K, device=batch["categories"].device, dtype=torch.float32)}
            bb._whole_path("stlt_forward", part, head, ops.workspace_bytes, bb._flags(), lambda *a: (logits["stlt"][s0:s1 + 1].view(-1, K),), before=(None,))
            return logits

        return explain.forward_perturbed(self, batch, scores, steps=steps, order=order, modality="layout", unit=unit, target=target,
                                         steps_per_pass=steps_per_pass, dataset_name=dataset_name, activation=activation, modalities=self.perturb_modalities,
                                         run_pass=run_pass)

    def forward_integrated_gradients(self, batch: Dict[str, torch.Tensor], target=None, steps: int = 16, baseline=None,
                                     steps_per_pass: Optional[int] = None) -> Dict[str, torch.Tensor]:
        """Integrated gradients (Sundararajan, Taly, Yan 2017) of one raw logit per clip with respect to the layout: the signed, complete
        member of the gradient family.  attr = (x - x0) * the integral of d logit / d x along the straight path from a baseline x0 to the
        input x, by the trapezoid rule on S = steps + 1 points (include/stlt_hip.h spells out the fp32 arithmetic); the attributions sum
        to logit(x) - logit(x0) up to the quadrature's error, which "delta" reports per clip.  What the reference needs S copies, a loop
        of requires_grad_ / backward and a torch accumulation for is here: stlt_ig_path (all the path batches of a pass in one launch),
        ``forward_saliency`` on them (the tape forward and the input-only sweep), stlt_ig_reduce (the quadrature, fixed order), and one
        stlt_ig_delta at the end.  Nothing is read back.
        ``target`` as in forward_saliency: None — each clip's top-1 class at the unperturbed input, taken from the logits of step
        ``steps`` that this very call computes; an int64 (B,) tensor; a float (B, num_classes) seed.  ``baseline``: None — all zeros — or a
        dict with "boxes" and / or "scores", each of the input's shape, dtype and device.  ``steps_per_pass``: how many of the S steps one
        tape forward and sweep hold (default: all).  Passes start at the input end of the path; inside a pass the steps are added in
        ascending s, so the order of the sum — and every bit of the result — is a function of (steps, steps_per_pass) alone.
        -> {"stlt": (B,K) logits at the input, "baseline_logits": (B,K), "target", "delta": (B,) = sum of the attributions -
        seed . (logits - baseline_logits), "boxes_attribution": (B,T,N,4), "scores_attribution": (B,T,N) when the batch has scores,
        "object_attribution": (B,T,N) = the four box terms plus the score term}.  Entries of padded object slots and frames are exactly
        0.  Refuses what forward_saliency refuses (live dropout, CPU tensors), and bad ``steps``, baselines and targets, all before the
        tape is overwritten.  Works with ``backbone.skip_padding`` on and off; touches no parameter's .grad."""
        return explain.forward_integrated_gradients(self, batch, target=target, steps=steps, baseline=baseline, steps_per_pass=steps_per_pass,
                                                    dropout_live=self.backbone._dropout_live(), modalities=self.perturb_modalities,
                                                    num_classes=self.prediction_head.fc2.weight.shape[0])


class _StltTrainFn(torch.autograd.Function):
    """Autograd shell of the native training step: forward = stlt_train_forward (records the tape), backward =
    stlt_train_backward (the reverse sweep in HIP).  The parameters are passed as inputs only so that autograd
    routes their gradients, and so are the batch's boxes and scores (the reference's layout inputs are ordinary autograd leaves; the
    sweep produces their gradients through stlt_train_backward_inputs when they are asked for); all arithmetic happens behind the C-ABI."""

    @staticmethod
    def forward(ctx, model, batch, boxes, scores, *params):
        bb = model.backbone
        flags = L.FLAG_SKIP_PADDING if bb.skip_padding else 0  # the other two flags are inference-only elisions
        logits, ctx.step = bb._train_forward(
            batch, model.prediction_head, flags, getattr(model, "_dropout_seed_override", None),
            "Stlt backward: the activation tape was overwritten by a later grad-enabled forward of the same "
            "model (one tape per backbone): run each forward's backward before the next forward, or wrap "
            "forwards that need no gradient in torch.no_grad()")
        ctx.model, ctx.batch, ctx.params = model, batch, params
        return logits

    @staticmethod
    def backward(ctx, dlogits):
        model, batch = ctx.model, ctx.batch
        bb = model.backbone
        bb._check_tape(ctx.step)
        device = dlogits.device
        used = model._grad_params("scores" in batch)
        # every gradient lives in one flat buffer: what a data-parallel run all-reduces and what train.FusedAdamW consumes
        layout, off = _flat_grad_layout(prm for prm in ctx.params if prm.requires_grad and id(prm) in used)
        # The fused trainer consumes the buffer before the next backward, so it is kept per backbone and cleared, not
        # re-allocated (344 MB at d = 768).  Otherwise the views below become the parameters' .grad tensors and outlive
        # this call: a fresh buffer every time.
        reuse = bool(getattr(model, "_flat_grads_only", False))
        flat = bb.__dict__.get("_flat_grad_buf") if reuse else None
        if flat is not None and flat.device == device and flat.numel() == off:
            flat.zero_()
        else:
            flat = torch.zeros(off, device=device, dtype=torch.float32)
            if reuse:
                bb.__dict__["_flat_grad_buf"] = flat
        views = {id(q): flat[o: o + n].view_as(q) for q, o, n in layout}
        g, gsp, gtp = bb._build_struct(model.prediction_head, lambda t: views[id(t)].data_ptr() if id(t) in views else None)
        model._last_flat_grad = flat  # one contiguous buffer: what a data-parallel wrapper all-reduces
        model._flat_layout = layout
        # the training context the sweep names: the trainer's while its step runs this backward (its transposed weight copies, its side
        # stream), else one the module owns for the side stream of plain autograd backwards
        tctx = getattr(model, "_train_context", None) or model._own_context()
        d_boxes, d_scores = _layout_grad_buffers(ctx.needs_input_grad[2:4], batch, ctx.step["shape"], device)

        def run(extra_flags):
            lower = extra_flags != L.FLAG_TRAIN_UPPER_ONLY  # the upper half never reaches the embedding
            bb._train_backward(ctx.step, g, dlogits, tctx.handle, d_boxes if lower else None, d_scores if lower else None, extra_flags)

        sync = getattr(model, "_grad_sync", None)  # data-parallel hook: sync(flat, lo, hi) may start reducing flat[lo:hi]
        with torch.cuda.device(device):
            if sync is None:
                run(0)
            else:
                # the temporal tower and the head come last in parameter order and first in the reverse sweep: their
                # gradients are final after the upper half, and can travel while the lower half computes
                upper = {id(q) for q in model.backbone.transformer.parameters()} | {id(q) for q in model.prediction_head.parameters()}
                split = min((o for q, o, n in layout if id(q) in upper), default=off)
                assert all((id(q) in upper) == (o >= split) for q, o, n in layout), "temporal tower + head must be the tail of the flat buffer"
                run(L.FLAG_TRAIN_UPPER_ONLY)
                sync(flat, split, off)
                run(L.FLAG_TRAIN_LOWER_ONLY)
                sync(flat, 0, split)
        d_boxes_out = d_boxes if ctx.needs_input_grad[2] else None
        if reuse:  # train.FusedAdamW reads the flat buffer: skip the per-parameter .grad copies
            return (None, None, d_boxes_out, d_scores) + tuple(None for _ in ctx.params)
        return (None, None, d_boxes_out, d_scores) + tuple(views.get(id(prm)) for prm in ctx.params)


class _BackboneTrainFn(torch.autograd.Function):
    """The backbone alone under autograd, for models that consume EVERY row of its output (the fusion models' layout branch,
    models.py:446-483): the same native tape forward / reverse sweep as `_StltTrainFn` with STLT_FLAG_TRAIN_BACKBONE — no
    prediction head, every temporal layer on every frame, the (B,T,d) output's gradient as the sweep's seed."""

    @staticmethod
    def forward(ctx, bb, batch, boxes, scores, *params):
        out, ctx.step = bb._train_forward(
            batch, None, L.FLAG_TRAIN_BACKBONE, None,
            "StltBackbone backward: the activation tape was overwritten by a later grad-enabled forward of the same "
            "backbone (one tape per backbone): run each forward's backward before the next forward")
        ctx.bb, ctx.batch, ctx.params = bb, batch, params
        return out

    @staticmethod
    def backward(ctx, dout):
        bb, batch = ctx.bb, ctx.batch
        bb._check_tape(ctx.step)
        device = dout.device
        # inside a Trainer step, parameters whose .grad is bound to the trainer's flat buffer are accumulated into in place (no
        # temporary, autograd gets None for them); the others — and every parameter outside a Trainer step, e.g. under
        # torch.autograd.grad() — get views of a fresh zero buffer that autograd accumulates / returns.  The gradient table of a
        # fully bound backbone is the same every step (fixed views of one flat buffer): it is kept with the backbone.
        b0 = next((getattr(q, "_stlt_bound", None) for q in ctx.params if q.requires_grad), None)
        key = (id(b0), "scores" in batch, tuple(q.requires_grad for q in ctx.params)) if (b0 is not None and b0.accumulating) else None
        cached = bb.__dict__.get("_grad_table")
        views = {}
        if key is not None and cached is not None and cached[0] == key and cached[1] is b0:
            g, gsp, gtp, touched = cached[2]
            b0._touched.update(touched)
        else:
            skip = bb._unused_param_ids("scores" in batch)
            want = [prm for prm in ctx.params if prm.requires_grad and id(prm) not in skip]
            direct = {}
            for q in want:
                bound = getattr(q, "_stlt_bound", None)
                view = bound.view_of(q) if bound is not None else None
                if view is not None:
                    bound.touch(q)
                    direct[id(q)] = view
            layout, off = _flat_grad_layout(q for q in want if id(q) not in direct)
            flat = torch.zeros(off, device=device, dtype=torch.float32) if off else None
            views = {id(q): flat[o: o + n].view_as(q) for q, o, n in layout}
            target = lambda t: direct[id(t)].data_ptr() if id(t) in direct else (views[id(t)].data_ptr() if id(t) in views else None)  # noqa: E731
            g, gsp, gtp = bb._build_struct(None, target)
            if key is not None and not layout and all(getattr(q, "_stlt_bound", None) is b0 for q in want):
                bb.__dict__["_grad_table"] = (key, b0, (g, gsp, gtp, frozenset(direct)))
        d_boxes, d_scores = _layout_grad_buffers(ctx.needs_input_grad[2:4], batch, ctx.step["shape"], device)
        bb._train_backward(ctx.step, g, dout, ops._ctx_handle(ops.context_of(ctx.params)), d_boxes, d_scores)
        return (None, None, d_boxes if ctx.needs_input_grad[2] else None, d_scores) + tuple(views.get(id(prm)) for prm in ctx.params)


models_factory = {"stlt": Stlt}  # "caf" / "cacnf" are added by modelling/fusion.py at package import
