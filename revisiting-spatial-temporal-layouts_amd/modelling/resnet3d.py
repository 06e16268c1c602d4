"""Drop-in ``Resnet3D`` (reference src/modelling/models.py:198-228): the R3D-50 trunk of ``generate_model(50)``
(src/modelling/resnets3d.py:93-214) minus ``avgpool`` / ``fc``, run natively on ``video_frames`` (B, 3, T, H, W).

The modules only hold parameters, under the reference's names and in its order (``resnet.0`` stem conv, ``resnet.1`` its
BatchNorm, ``resnet.4`` .. ``resnet.7`` the four layers of Bottleneck blocks, then ``classifier``).  The forward is one call of
``stlt_r3d_forward`` (csrc/r3d.hip): channels-last implicit-GEMM convolutions on the f32 MFMA with BatchNorm, residual and ReLU in
their epilogues.  BatchNorm always has eval semantics, as ``Resnet3D.train`` keeps it (models.py:215-219).

The trunk has no backward here (Conv3d backward is not built): with autograd on, a trainable trunk parameter is an error that names
the fix (``….resnet.requires_grad_(False)``); a frozen trunk runs without a tape and its consumers train on its output.
"""
from __future__ import annotations

import ctypes as C
from typing import Dict, List, Tuple

import torch
from torch import nn

from .. import _lib as L
from .. import ops
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
    Held outside the module's parameters and buffers, so it never reaches a state dict; copies and pickles start empty."""

    def __init__(self):
        self.packed: Dict[int, Tuple[Tuple, torch.Tensor]] = {}
        self.ws = _Workspace()

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
        """-> (features (B, 2048, To, Ho, Wo) | None, pooled (B, 2048) | None); no autograd tape."""
        if torch.is_grad_enabled() and any(p.requires_grad for p in trunk.parameters()):
            raise L.StltHipError(
                f"the R3D-50 trunk ({name}) has trainable parameters, but Conv3d backward is not built: freeze it with "
                f"`{name}.requires_grad_(False)` (training then goes on through the layers after it), or run under torch.no_grad()")
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
            for i, (conv, bn) in enumerate(trunk_convs(trunk)):
                if abs(bn.eps - BN_EPS) > 0:
                    raise L.StltHipError(f"BatchNorm3d eps must be {BN_EPS} (resnets3d.py), got {bn.eps}")
                pw = self._packed_weight(i, conv.weight)
                p.conv[i] = L.R3dConv(pw.data_ptr(), _dev_ptr(bn.weight), _dev_ptr(bn.bias), _dev_ptr(bn.running_mean), _dev_ptr(bn.running_var))
            nbytes = int(lib.stlt_r3d_workspace_bytes(B, T, H, W))
            if nbytes == 0:
                raise L.StltHipError(f"video_frames {tuple(video.shape)}: no trunk for this shape")
            ws = self.ws.get(nbytes, device)
            To, Ho, Wo = _trunk_out(T), _trunk_out(H, 2), _trunk_out(W, 2)
            feats = torch.empty(B, FEATURE_CHANNELS, To, Ho, Wo, device=device, dtype=torch.float32) if features else None
            pool = torch.empty(B, FEATURE_CHANNELS, device=device, dtype=torch.float32) if pooled else None
            L.check(lib.stlt_r3d_forward(C.byref(p), video.data_ptr(), B, T, H, W, ws.data_ptr(), ws.numel(), None if feats is None else feats.data_ptr(),
                                         None if pool is None else pool.data_ptr(), stream), "stlt_r3d_forward")
        return feats, pool


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
        object.__setattr__(self, "_runner", TrunkRunner())

    def __getstate__(self):
        state = self.__dict__.copy()
        state.pop("_runner", None)
        return state

    def __setstate__(self, state):
        self.__dict__.update(state)
        object.__setattr__(self, "_runner", TrunkRunner())

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
