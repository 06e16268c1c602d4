"""Drop-in ``Resnet3D`` (reference src/modelling/models.py:198-228): the R3D-50 trunk of ``generate_model(50)``
(src/modelling/resnets3d.py:93-214) minus ``avgpool`` / ``fc``, run natively on ``video_frames`` (B, 3, T, H, W).

The modules only hold parameters, under the reference's names and in its order (``resnet.0`` stem conv, ``resnet.1`` its
BatchNorm, ``resnet.4`` .. ``resnet.7`` the four layers of Bottleneck blocks, then ``classifier``).  The forward is one call of
``stlt_r3d_forward`` (csrc/r3d.hip): channels-last implicit-GEMM convolutions on the f32 MFMA with BatchNorm, residual and ReLU in
their epilogues.  BatchNorm always has eval semantics, as ``Resnet3D.train`` keeps it (models.py:215-219).

Training the trunk is opt-in (``train_trunk=True`` in the model's config).  With it on, a grad-enabled forward with trainable conv
weights runs ``R3dTrunkFn``: ``stlt_r3d_train_forward`` records a tape (its own, from torch's allocator, held by the autograd context)
and ``stlt_r3d_backward`` writes the 53 conv weight gradients — straight into a Trainer's flat gradient buffer inside its step
(``ops.grad_targets``).  The packed weight copies are then re-made by one batched repack whenever the weights may have changed: a
parameter's storage or ``_version`` moved, or the fused optimiser (which writes through raw pointers and leaves ``_version`` alone)
stepped since (``ops.raw_param_writes``).  With it off (the default) nothing changes: with autograd on, a
trainable trunk parameter is an error that names the fix (``….resnet.requires_grad_(False)``); a frozen trunk runs without a tape and
its consumers train on its output.

Pixel gradients: a grad-enabled forward whose ``video_frames`` requires grad takes the tape path as well, with a trainable trunk
(``train_trunk``) and with a frozen one, and ``R3dTrunkFn.backward`` returns ``video_frames.grad`` from ``stlt_r3d_backward_inputs`` (the
stem's thin data gradient, written in the video's own layout); with no conv weight to train the sweep is input-only (no weight-gradient
launch).  ``forward_saliency`` is that sweep as an inference call: the logits and ∂ logit / ∂ video_frames in one pass.
"""
from __future__ import annotations

import contextlib
import ctypes as C
from typing import Dict, List, Optional, Tuple

import torch
from torch import nn

from .. import _lib as L
from .. import ops
from . import explain
from .models import _dev_ptr, _Workspace

BLOCKS = (3, 4, 6, 3)
PLANES = (64, 128, 256, 512)
BN_EPS = 1e-5
FEATURE_CHANNELS = 2048


class Bottleneck(nn.Module):
    """resnets3d.py:58-91: conv1 (1x1x1), conv2 (3x3x3, stride), conv3 (1x1x1, x4), BatchNorm3d after each, shortcut type B."""

    expansion = 4

    def __init__(self, in_planes: int, planes: int, stride: int = 1, downsample: bool = False):
        super().__init__()
        self.conv1 = nn.Conv3d(in_planes, planes, kernel_size=1, bias=False)
        self.bn1 = nn.BatchNorm3d(planes)
        self.conv2 = nn.Conv3d(planes, planes, kernel_size=3, stride=stride, padding=1, bias=False)
        self.bn2 = nn.BatchNorm3d(planes)
        self.conv3 = nn.Conv3d(planes, planes * 4, kernel_size=1, bias=False)
        self.bn3 = nn.BatchNorm3d(planes * 4)
        self.relu = nn.ReLU(inplace=True)
        if downsample:
            self.downsample = nn.Sequential(nn.Conv3d(in_planes, planes * 4, kernel_size=1, stride=stride, bias=False), nn.BatchNorm3d(planes * 4))
        else:
            self.downsample = None


def make_trunk() -> nn.Sequential:
    """``nn.Sequential(*list(generate_model(50).children())[:-2])`` as a parameter holder (same keys, shapes and init)."""
    layers: List[nn.Module] = [nn.Conv3d(3, 64, kernel_size=(7, 7, 7), stride=(1, 2, 2), padding=(3, 3, 3), bias=False), nn.BatchNorm3d(64),
                               nn.ReLU(inplace=True), nn.MaxPool3d(kernel_size=3, stride=2, padding=1)]
    in_planes = 64
    for i, (n, planes) in enumerate(zip(BLOCKS, PLANES)):
        stride = 1 if i == 0 else 2
        blocks = []
        for b in range(n):
            blocks.append(Bottleneck(in_planes, planes, stride if b == 0 else 1, downsample=(b == 0)))
            in_planes = planes * 4
        layers.append(nn.Sequential(*blocks))
    trunk = nn.Sequential(*layers)
    for m in trunk.modules():  # resnets3d.py:150-156
        if isinstance(m, nn.Conv3d):
            nn.init.kaiming_normal_(m.weight, mode="fan_out", nonlinearity="relu")
        elif isinstance(m, nn.BatchNorm3d):
            nn.init.constant_(m.weight, 1)
            nn.init.constant_(m.bias, 0)
    return trunk


def trunk_convs(trunk: nn.Sequential) -> List[Tuple[nn.Conv3d, nn.BatchNorm3d]]:
    """The 53 (conv, BatchNorm) pairs in state-dict order: stem, then per block conv1, conv2, conv3, [downsample]."""
    out = [(trunk[0], trunk[1])]
    for layer in trunk[4:8]:
        for blk in layer:
            out += [(blk.conv1, blk.bn1), (blk.conv2, blk.bn2), (blk.conv3, blk.bn3)]
            if blk.downsample is not None:
                out.append((blk.downsample[0], blk.downsample[1]))
    return out


def load_full_resnet_state(trunk: nn.Sequential, path: str) -> None:
    """Resnet3D's constructor (models.py:201-206): ``torch.load(path)["state_dict"]`` holds the keys of the full ResNet (conv1, bn1,
    layer1..4, fc); avgpool / fc are dropped by child index, so conv1 -> 0, bn1 -> 1, layerN -> N + 3."""
    sd = torch.load(path, map_location="cpu")["state_dict"]
    rename = {"conv1": "0", "bn1": "1", "layer1": "4", "layer2": "5", "layer3": "6", "layer4": "7"}
    mapped, rest = {}, []
    for k, v in sd.items():
        head, _, tail = k.partition(".")
        if head in rename:
            mapped[f"{rename[head]}.{tail}"] = v
        else:
            rest.append(k)
    if sorted(rest) != ["fc.bias", "fc.weight"]:
        raise RuntimeError(f"{path}: expected the state dict of a full R3D-50 (conv1, bn1, layer1-4, fc); unexpected keys {sorted(rest)[:8]}")
    trunk.load_state_dict(mapped, strict=True)


class TrunkRunner:
    """Launch state of one trunk: packed weight copies (re-made when a parameter's storage or ``_version`` changes) and the workspace.
    Held outside the module's parameters and buffers, so it never reaches a state dict; copies and pickles start empty.
    ``train_trunk``: a trainable trunk under autograd runs R3dTrunkFn; its forward and dgrad copies are re-made by one batched launch
    whenever the weights may have changed (``_weights_key``).  A video that requires grad runs R3dTrunkFn too, frozen trunk or not: the
    same copies, plus the stem's thin data-gradient copy (``stlt_conv3d_repack_dgrad_thin``) under the same key."""

    def __init__(self, train_trunk: bool = False):
        self.packed: Dict[int, Tuple[Tuple, torch.Tensor]] = {}
        self.ws = _Workspace()
        self.bws = _Workspace()
        self.train_trunk = train_trunk
        self.copies = None  # (device, forward copies, dgrad copies) of the trainable trunk: stlt_r3d_repack_all's destinations
        self.copies_key = None  # _weights_key of the weights the copies were made from
        self.thin_key = None  # ... and of those the stem's thin copy (dgrad copies [0]) was made from; made only when a video wants its gradient

    @staticmethod
    def _weights_key(pairs, device):
        """What the copies depend on: every conv weight and BN scale (storage, _version) and the raw-pointer writes of the fused optimiser."""
        return (device, ops.raw_param_writes(),
                tuple((t.data_ptr(), t._version) for conv, bn in pairs for t in (conv.weight, bn.weight, bn.running_var)))

    def _refresh(self, trunk: nn.Sequential, p, device, thin: bool = False) -> None:
        """Point p at the forward copies, re-made first (stlt_r3d_repack_all: every forward copy and every BN-scaled dgrad copy, one
        launch) when the weights may have changed since they were made.  ``thin``: also the stem's thin data-gradient copy."""
        pairs = trunk_convs(trunk)
        key = self._weights_key(pairs, device)
        if self.copies is None or self.copies[0] != device:
            fwd, dgr = [], []
            for i, (conv, _) in enumerate(pairs):
                co, ci, kt, kh, kw = conv.weight.shape
                fwd.append(torch.empty(co, kt, kh, kw, (ci + 3) // 4 * 4, device=device, dtype=torch.float32))
                dgr.append(torch.empty(conv.weight.numel() if i else THIN_FLOATS, device=device, dtype=torch.float32))
            self.copies = (device, fwd, dgr)
            self.copies_key = self.thin_key = None
        _, fwd, dgr = self.copies
        if key != self.copies_key:
            ws = L.R3dPointers(*[_dev_ptr(conv.weight) for conv, _ in pairs])
            L.check(L.load().stlt_r3d_repack_all(ws, C.byref(p), L.R3dPointers(*[t.data_ptr() for t in fwd]),
                                                 L.R3dPointers(*[t.data_ptr() for t in dgr]), torch.cuda.current_stream().cuda_stream),
                    "stlt_r3d_repack_all")
            self.copies_key = key
            self.packed.clear()  # the per-conv cache would be stale after an in-place optimiser step
        if thin and key != self.thin_key:
            conv, bn = pairs[0]
            scale = (bn.weight.detach() / torch.sqrt(bn.running_var + BN_EPS)).contiguous()  # the stem's BN scale, folded into the copy
            L.check(L.load().stlt_conv3d_repack_dgrad_thin(_dev_ptr(conv.weight), C.byref(stem_desc(1, 1, 1, 1)), scale.data_ptr(), dgr[0].data_ptr(),
                                                           torch.cuda.current_stream().cuda_stream), "stlt_conv3d_repack_dgrad_thin")
            self.thin_key = key
        for i, t in enumerate(fwd):
            p.conv[i].w = t.data_ptr()

    def _packed_weight(self, i: int, w: torch.Tensor) -> torch.Tensor:
        key = (w.data_ptr(), w._version, w.device, tuple(w.shape))
        hit = self.packed.get(i)
        if hit is not None and hit[0] == key:
            return hit[1]
        co, ci, kt, kh, kw = w.shape
        cpad = (ci + 3) // 4 * 4
        out = torch.empty(co, kt, kh, kw, cpad, device=w.device, dtype=torch.float32)
        L.check(L.load().stlt_conv3d_repack(_dev_ptr(w), co, ci, kt, kh, kw, cpad, out.data_ptr(), torch.cuda.current_stream().cuda_stream),
                "stlt_conv3d_repack")
        self.packed[i] = (key, out)
        return out

    def run(self, trunk: nn.Sequential, video: torch.Tensor, features: bool = True, pooled: bool = False, name: str = "resnet"):
        """-> (features (B, 2048, To, Ho, Wo) | None, pooled (B, 2048) | None); an autograd tape with ``train_trunk`` on and a trainable
        trunk, or whenever the video requires grad."""
        trainable = any(p.requires_grad for p in trunk.parameters())
        video_grad = torch.is_grad_enabled() and isinstance(video, torch.Tensor) and video.requires_grad
        with_grad = (torch.is_grad_enabled() and trainable) or video_grad
        if torch.is_grad_enabled() and trainable and not self.train_trunk:
            raise L.StltHipError(
                f"the R3D-50 trunk ({name}) has trainable parameters, but Conv3d backward is not built: freeze it with "
                f"`{name}.requires_grad_(False)` (training then goes on through the layers after it), or run under torch.no_grad() "
                f"(or train it: train_trunk=True in the model config)")
        if with_grad and features == pooled:
            raise L.StltHipError("a trained trunk forward returns either the feature map or the pooled features, not both")
        video = ops._chk(video, torch.float32, "video_frames")
        if video.dim() != 5 or video.shape[1] != 3:
            raise L.StltHipError(f"video_frames must be (B, 3, T, H, W), got {tuple(video.shape)}")
        B, _, T, H, W = video.shape
        lib = L.load()
        device = video.device
        p = L.R3dParams()
        p.bn_eps = BN_EPS
        with torch.cuda.device(device):
            stream = torch.cuda.current_stream().cuda_stream
            refresh = (self.train_trunk and trainable) or video_grad  # the tape path reads the batched copies (the dgrad ones among them)
            for i, (conv, bn) in enumerate(trunk_convs(trunk)):
                if abs(bn.eps - BN_EPS) > 0:
                    raise L.StltHipError(f"BatchNorm3d eps must be {BN_EPS} (resnets3d.py), got {bn.eps}")
                pw = None if refresh else self._packed_weight(i, conv.weight).data_ptr()
                p.conv[i] = L.R3dConv(pw, _dev_ptr(bn.weight), _dev_ptr(bn.bias), _dev_ptr(bn.running_mean), _dev_ptr(bn.running_var))
            if refresh:
                self._refresh(trunk, p, device, thin=video_grad)
            nbytes = int(lib.stlt_r3d_workspace_bytes(B, T, H, W))
            if nbytes == 0:
                raise L.StltHipError(f"video_frames {tuple(video.shape)}: no trunk for this shape")
            ws = self.ws.get(nbytes, device)
            if with_grad:
                out = R3dTrunkFn.apply(self, p, video, bool(pooled), *[conv.weight for conv, _ in trunk_convs(trunk)])
                return (None, out) if pooled else (out, None)
            To, Ho, Wo = _trunk_out(T), _trunk_out(H, 2), _trunk_out(W, 2)
            feats = torch.empty(B, FEATURE_CHANNELS, To, Ho, Wo, device=device, dtype=torch.float32) if features else None
            pool = torch.empty(B, FEATURE_CHANNELS, device=device, dtype=torch.float32) if pooled else None
            L.check(lib.stlt_r3d_forward(C.byref(p), video.data_ptr(), B, T, H, W, ws.data_ptr(), ws.numel(), None if feats is None else feats.data_ptr(),
                                         None if pool is None else pool.data_ptr(), stream), "stlt_r3d_forward")
        return feats, pool

    def run_tape(self, trunk: nn.Sequential, video: torch.Tensor, features: bool = True, pooled: bool = False) -> "TrunkTape":
        """The tape forward outside autograd (stlt_r3d_train_forward; the features and the pooled features are bit for bit those of
        ``run``), for a call that reads a stage's output off the tape and sends a gradient down to it (``forward_gradcam`` below the last
        stage: ops.r3d_tape_stage, ops.r3d_backward_layer).  Frozen or trainable trunk alike: nothing here forms a weight gradient."""
        video = ops._chk(video, torch.float32, "video_frames")
        if video.dim() != 5 or video.shape[1] != 3:
            raise L.StltHipError(f"video_frames must be (B, 3, T, H, W), got {tuple(video.shape)}")
        if not features and not pooled:
            raise L.StltHipError("run_tape: ask for the feature map, the pooled features or both")
        B, _, T, H, W = video.shape
        lib = L.load()
        device = video.device
        p = L.R3dParams()
        p.bn_eps = BN_EPS
        with torch.cuda.device(device), torch.no_grad():
            for i, (conv, bn) in enumerate(trunk_convs(trunk)):
                if abs(bn.eps - BN_EPS) > 0:
                    raise L.StltHipError(f"BatchNorm3d eps must be {BN_EPS} (resnets3d.py), got {bn.eps}")
                p.conv[i] = L.R3dConv(None, _dev_ptr(bn.weight), _dev_ptr(bn.bias), _dev_ptr(bn.running_mean), _dev_ptr(bn.running_var))
            self._refresh(trunk, p, device)
            nbytes = int(lib.stlt_r3d_tape_bytes(B, T, H, W))
            if nbytes == 0:
                raise L.StltHipError(f"video_frames {tuple(video.shape)}: no trunk for this shape")
            tape = torch.empty(nbytes, dtype=torch.uint8, device=device)
            ws = self.ws.get(int(lib.stlt_r3d_workspace_bytes(B, T, H, W)), device)
            To, Ho, Wo = _trunk_out(T), _trunk_out(H, 2), _trunk_out(W, 2)
            feats = torch.empty(B, FEATURE_CHANNELS, To, Ho, Wo, device=device, dtype=torch.float32) if features else None
            pool = torch.empty(B, FEATURE_CHANNELS, device=device, dtype=torch.float32) if pooled else None
            L.check(lib.stlt_r3d_train_forward(C.byref(p), video.data_ptr(), B, T, H, W, ws.data_ptr(), ws.numel(), tape.data_ptr(), tape.numel(),
                                               None if feats is None else feats.data_ptr(), None if pool is None else pool.data_ptr(),
                                               torch.cuda.current_stream().cuda_stream), "stlt_r3d_train_forward")
        return TrunkTape(self, L.R3dParams.from_buffer_copy(p), tape, (B, T, H, W), list(self.copies[2]), feats, pool)


class TrunkTape:
    """One tape forward of the trunk (TrunkRunner.run_tape): ``features`` / ``pooled`` as asked for, the ``tape``, the ``params`` and the
    data-gradient copies ``dgrad`` it was made with, ``shape`` = (B, T, H, W).  ``stage(layer)``: that stage's output (B, t, h, w, c) NDHWC,
    a view of the tape; ``backward_layer(layer, dfeatures=, dpooled=)``: the gradient there (ops.r3d_backward_layer) in the runner's
    backward workspace."""

    def __init__(self, runner, params, tape, shape, dgrad, features, pooled):
        self.runner, self.params, self.tape, self.shape, self.dgrad, self.features, self.pooled = runner, params, tape, shape, dgrad, features, pooled

    def stage(self, layer: int) -> torch.Tensor:
        return ops.r3d_tape_stage(self.tape, self.shape, layer)

    def backward_layer(self, layer: int, dfeatures: Optional[torch.Tensor] = None, dpooled: Optional[torch.Tensor] = None) -> torch.Tensor:
        ws = self.runner.bws.get(int(L.load().stlt_r3d_backward_workspace_bytes(*self.shape)), self.tape.device)
        return ops.r3d_backward_layer(self.params, self.dgrad, self.tape, self.shape, layer, dfeatures=dfeatures, dpooled=dpooled, workspace=ws)


class R3dTrunkFn(torch.autograd.Function):
    """The trunk with a tape: forward = stlt_r3d_train_forward (the features or the pooled features, bit for bit those of
    stlt_r3d_forward), backward = stlt_r3d_backward into the 53 conv weights' gradients (in place into a Trainer's flat buffer inside
    its step, fresh tensors anywhere else: ops.grad_targets).  Each call owns its tape.  When video_frames requires grad the backward is
    stlt_r3d_backward_inputs: the same sweep, then the stem's thin data gradient into video_frames.grad (B, 3, T, H, W); with no conv
    weight asking for a gradient it is the input-only sweep (dweight NULL: no weight-gradient launch)."""

    @staticmethod
    def forward(ctx, runner, p, video, pooled, *weights):
        lib = L.load()
        B, _, T, H, W = video.shape
        device = video.device
        stream = torch.cuda.current_stream().cuda_stream
        tape = torch.empty(int(lib.stlt_r3d_tape_bytes(B, T, H, W)), dtype=torch.uint8, device=device)
        ws = runner.ws.get(int(lib.stlt_r3d_workspace_bytes(B, T, H, W)), device)
        if pooled:
            out = torch.empty(B, FEATURE_CHANNELS, device=device, dtype=torch.float32)
        else:
            out = torch.empty(B, FEATURE_CHANNELS, _trunk_out(T), _trunk_out(H, 2), _trunk_out(W, 2), device=device, dtype=torch.float32)
        L.check(lib.stlt_r3d_train_forward(C.byref(p), video.data_ptr(), B, T, H, W, ws.data_ptr(), ws.numel(), tape.data_ptr(), tape.numel(),
                                           None if pooled else out.data_ptr(), out.data_ptr() if pooled else None, stream), "stlt_r3d_train_forward")
        ctx.runner, ctx.params, ctx.tape, ctx.shape, ctx.pooled = runner, L.R3dParams.from_buffer_copy(p), tape, (B, T, H, W), pooled
        # the dgrad copies are the runner's, shared by every forward and re-made when the weights change: the backward checks that they
        # still come from the weights this forward saw (a changed weight between a forward and its backward is an error, as in torch)
        ctx.dgrad, ctx.copies_key = list(runner.copies[2]), runner.copies_key
        ctx.weights = weights  # the parameters themselves: grad_targets looks at their Trainer binding
        return out

    @staticmethod
    def backward(ctx, dout):
        lib = L.load()
        B, T, H, W = ctx.shape
        if ctx.tape is None:
            raise L.StltHipError("R3dTrunkFn: the tape of this forward was already consumed by a backward (retain_graph is not supported)")
        if ctx.runner.copies_key != ctx.copies_key or ctx.runner.copies[2][0] is not ctx.dgrad[0]:
            raise L.StltHipError("R3dTrunkFn: the trunk's weights changed between this forward and its backward (an optimiser step or a load in "
                                 "between); run the backward before changing the weights")
        dout = dout.contiguous()
        want_video, want_weights = ctx.needs_input_grad[2], any(ctx.needs_input_grad[4:])
        if not want_video and not want_weights:
            ctx.tape = None
            return (None,) * (4 + len(ctx.weights))
        grads, dw_ptrs = (None,) * len(ctx.weights), None
        if want_weights:
            targets, grads = ops.grad_targets(ctx.weights, ctx.needs_input_grad[4:])
            dws = [t if t is not None else torch.empty_like(w) for t, w in zip(targets, ctx.weights)]  # frozen convs: a scratch target
            dw_ptrs = L.R3dPointers(*[t.data_ptr() for t in dws])
        dgrad = L.R3dPointers(*[t.data_ptr() for t in ctx.dgrad])
        dfeat, dpool = (None, dout.data_ptr()) if ctx.pooled else (dout.data_ptr(), None)
        stream = torch.cuda.current_stream().cuda_stream
        dvideo = None
        if want_video:
            if ctx.runner.thin_key != ctx.copies_key:
                raise L.StltHipError("R3dTrunkFn: the stem's thin data-gradient copy does not belong to this forward's weights")
            dvideo = torch.empty(B, 3, T, H, W, device=dout.device, dtype=torch.float32)
            ws = ctx.runner.bws.get(int(lib.stlt_r3d_backward_inputs_workspace_bytes(B, T, H, W)), dout.device)
            L.check(lib.stlt_r3d_backward_inputs(C.byref(ctx.params), dgrad, ctx.tape.data_ptr(), ctx.tape.numel(), B, T, H, W, dfeat, dpool, dw_ptrs, 1,
                                                 dvideo.data_ptr(), ws.data_ptr(), ws.numel(), stream), "stlt_r3d_backward_inputs")
        else:
            ws = ctx.runner.bws.get(int(lib.stlt_r3d_backward_workspace_bytes(B, T, H, W)), dout.device)
            L.check(lib.stlt_r3d_backward(C.byref(ctx.params), dgrad, ctx.tape.data_ptr(), ctx.tape.numel(), B, T, H, W, dfeat, dpool, dw_ptrs, 1,
                                          ws.data_ptr(), ws.numel(), stream), "stlt_r3d_backward")
        ctx.tape = None
        return (None, None, dvideo, None, *grads)


def stem_desc(B: int, T: int, H: int, W: int) -> "L.Conv3dDesc":
    """The stem as the thin data gradient's descriptor (real input channels: 3)."""
    return L.Conv3dDesc(B, T, H, W, 3, 64, 7, 7, 7, 1, 2, 2, 3, 3, 3)


THIN_FLOATS = 1792 * 64  # stlt_conv3d_repack_dgrad_thin_floats of the stem: [jt 7][jh 4][jw 4][co / 4][column 16][4]


@contextlib.contextmanager
def inputs_only(module: nn.Module):
    """Every parameter of ``module`` frozen for the duration, then as it was: the native Functions form a weight gradient only for a
    parameter that requires grad, so a backward inside reaches the inputs alone (no weight-gradient product, no ``.grad`` touched)."""
    was = [(q, q.requires_grad) for q in module.parameters()]
    for q, _ in was:
        q.requires_grad_(False)
    try:
        yield
    finally:
        for q, r in was:
            q.requires_grad_(r)


def video_saliency(model: nn.Module, batch: Dict[str, torch.Tensor], target, name: str, dropout_live: bool = False) -> Dict[str, torch.Tensor]:
    """forward_saliency of a video-only model: its forward on a private leaf of ``video_frames`` with every parameter frozen
    (``inputs_only``), the seed, and the input-only sweep.  ``dropout_live``: the model's own answer."""
    video = batch["video_frames"]
    explain.require_inference("forward_saliency", dropout_live=dropout_live, tensors=(video,))
    leaf = video.detach().requires_grad_(True)
    with inputs_only(model), torch.enable_grad():
        logits = model.forward(dict(batch, video_frames=leaf))[name]
        seed, target = explain.saliency_seed(logits, target)
        (dvideo,) = torch.autograd.grad(logits, leaf, seed)
    return {name: logits.detach(), "target": target, "video_frames_grad": dvideo}


def _trunk_out(n: int, stem_stride: int = 1) -> int:
    """A temporal (stem_stride 1) or spatial (2) extent through the stem, the max-pool and the three stride-2 layers."""
    n = (n + 6 - 7) // stem_stride + 1
    for _ in range(4):
        n = (n + 2 - 3) // 2 + 1
    return n


class Resnet3D(nn.Module):
    """``forward_features(batch)`` -> (B, 2048, 2, 4, 4) from ``batch["video_frames"]``; ``forward(batch)`` -> ``{"resnet3d": logits}``."""

    def __init__(self, config):
        super().__init__()
        self.resnet = make_trunk()
        if getattr(config, "resnet_model_path", None):
            load_full_resnet_state(self.resnet, config.resnet_model_path)
        for m in self.resnet.modules():  # models.py:207-211: BatchNorm affine parameters frozen
            if isinstance(m, nn.BatchNorm3d):
                m.weight.requires_grad = False
                m.bias.requires_grad = False
        if config.num_classes > 0:
            self.avgpool = nn.AdaptiveAvgPool3d((1, 1, 1))  # parameter-free; the native trunk pools (stlt_avgpool_ndhwc)
            self.classifier = nn.Linear(FEATURE_CHANNELS, config.num_classes)
        self.logit_names = ("resnet3d",)
        self.trunk_name = "resnet"
        self.train_trunk = bool(getattr(config, "train_trunk", False))
        object.__setattr__(self, "_runner", TrunkRunner(self.train_trunk))

    perturb_modalities = ("appearance",)  # what forward_perturbed deletes from (infer.run_perturbation_test reads this)

    def __getstate__(self):
        state = self.__dict__.copy()
        state.pop("_runner", None)
        return state

    def __setstate__(self, state):
        self.__dict__.update(state)
        object.__setattr__(self, "_runner", TrunkRunner(self.__dict__.get("train_trunk", False)))

    def train(self, mode: bool = True):
        super().train(mode)
        for m in self.resnet.modules():  # models.py:213-219
            if isinstance(m, nn.BatchNorm3d):
                m.train(False)
        return self

    def forward_features(self, batch: Dict[str, torch.Tensor]) -> torch.Tensor:
        feats, _ = self._runner.run(self.resnet, batch["video_frames"], features=True, name=self.trunk_name)
        return feats

    def forward(self, batch: Dict[str, torch.Tensor]) -> Dict[str, torch.Tensor]:
        _, pooled = self._runner.run(self.resnet, batch["video_frames"], features=False, pooled=True, name=self.trunk_name)
        return {"resnet3d": ops.LinearFn.apply(pooled, self.classifier.weight, self.classifier.bias)}

    def forward_saliency(self, batch: Dict[str, torch.Tensor], target=None) -> Dict[str, torch.Tensor]:
        """The model's logits and the gradient of one raw logit per clip with respect to the pixels, in one pass: what the reference gives
        for ``video_frames.requires_grad_()`` followed by ``logits[b, target[b]].backward()``.  The trunk's tape forward, stlt_saliency_seed,
        then stlt_r3d_backward_inputs with dweight NULL — the input-only sweep: no weight-gradient launch, no parameter's ``.grad`` touched,
        whether or not the parameters are trainable (``train_trunk`` is not needed).
        -> {"resnet3d": (B, num_classes) logits, "target": the selected classes, "video_frames_grad": (B, 3, T, H, W) float32}.
        ``target`` as in Stlt.forward_saliency: None (each clip's top-1 class), an int64 (B,) tensor, or a float (B, num_classes) seed.
        Inference call; this model has no dropout, so there is none to refuse."""
        return video_saliency(self, batch, target, "resnet3d")

    def forward_perturbed(self, batch: Dict[str, torch.Tensor], scores: torch.Tensor, steps: int = 10, order: str = "descending", modality: str = "appearance",
                          target=None, steps_per_pass: Optional[int] = None, fill: float = 0.0, activation: str = "softmax") -> Dict[str, torch.Tensor]:
        """The perturbation test of a per-cell map on this model, as CrossAttentionFusion.forward_perturbed with the appearance side alone
        (``modality`` is "appearance"; this model reads no layout): the cells of ``video_frames`` — collate.perturb_cells says what a cell
        is — are ranked by ``scores`` (B,C) (or (B,C+1), first column dropped), the first k = floor(s * C / steps) are set to ``fill`` for
        s = 0 .. steps, and ``forward`` runs on every reduced video.  -> {"resnet3d": (S,B,K), "prob", "hit", "auc", "target", "removed",
        "n_candidates"}."""
        return explain.forward_perturbed(self, batch, scores, steps=steps, order=order, modality=modality, target=target, steps_per_pass=steps_per_pass, fill=fill,
                                         activation=activation, modalities=self.perturb_modalities)  # no dropout in this model: never live

    def forward_integrated_gradients(self, batch: Dict[str, torch.Tensor], target=None, steps: int = 16, baseline=None, steps_per_pass=None) -> Dict[str, torch.Tensor]:
        """Integrated gradients of one raw logit per clip with respect to the pixels: Stlt.forward_integrated_gradients with
        ``video_frames`` as the moved input (stlt_ig_path_dense builds the path).  ``baseline``: None — all zeros, the dataset mean after
        Normalize(0.5, 0.5) — or {"video_frames": a tensor of the input's shape, dtype and device}.
        -> {"resnet3d": (B,K) logits at the input, "baseline_logits", "target", "delta" (B,), "video_frames_attribution" (B,3,T,H,W),
        "cell_attribution" (B,C): the signed sum per cell of collate.appearance_cells (stlt_cell_pool_sum)}.  Every pass is
        ``forward_saliency`` on the path batch: ``steps_per_pass`` bounds the clips one tape holds."""
        return explain.forward_integrated_gradients(self, batch, target=target, steps=steps, baseline=baseline, steps_per_pass=steps_per_pass,
                                                    modalities=self.perturb_modalities, num_classes=self.classifier.weight.shape[0])

    def _gradcam_head(self, feats, pooled, target, head):
        """forward_gradcam's part of this model: the classifier on the pooled features as a leaf -> its input gradient"""
        leaf = pooled.detach().requires_grad_(True)
        with inputs_only(self), torch.enable_grad():
            logits = ops.LinearFn.apply(leaf, self.classifier.weight, self.classifier.bias)
            seed, target = explain.saliency_seed(logits, target, "forward_gradcam")
            (dpooled,) = torch.autograd.grad(logits, leaf, seed)
        return {"resnet3d": logits.detach()}, target, None, dpooled

    def forward_gradcam(self, batch: Dict[str, torch.Tensor], target=None, layer: int = 4, variant: str = "gradcam", relu: bool = True,
                        upsample: bool = False) -> Dict[str, torch.Tensor]:
        """Grad-CAM (Selvaraju et al., ICCV 2017) of one raw logit per clip at the output of stage ``layer`` (1 to 4) of the trunk: the
        stage's activations summed over the channels, weighted by the logit's gradient with respect to them — by its mean over the
        positions (``variant="gradcam"``) or element by element (``"hirescam"``, Draelos and Carin 2020) — and, with ``relu``, the
        positive part.  The gradient is the one a hook on ``layerN``'s output sees in the reference's trunk (after the stage's ReLU).
        -> {"resnet3d": (B, num_classes) logits, "target", "cam": (B, gt, gh, gw) float32, raw, not normalised, "cell_attribution": (B, C) on
        the grid of collate.appearance_cells — ``cam`` flattened at the last stage, below it the sum over the 2^(4 - layer) cube of positions
        of each cell (stlt_cell_pool_sum) —, with ``upsample`` "video_cam": (B, T, H, W), the trilinear resize of ``cam`` onto the video}.
        ``layer=4`` needs no tape and no trunk backward: the plain trunk forward, the classifier's input gradient spread as the average
        pool spreads it (dpooled / P), stlt_cam_weights and stlt_cam_map.  Below it: the tape forward, stlt_r3d_backward_layer — the
        input-only sweep stopped at the stage — and the two launches on the tape's slot.  ``target`` as in ``forward_saliency``.  Nothing
        is read back; no parameter's ``.grad`` is touched (``train_trunk`` is not needed).  Inference call; this model has no dropout."""
        return explain.forward_gradcam(self, batch, target=target, layer=layer, variant=variant, relu=relu, upsample=upsample,
                                       trunk=(self._runner, self.resnet), head_gradient=self._gradcam_head, pooled_head=True)
