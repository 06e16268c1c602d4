"""Training the R3D-50 trunk, CPU side: the `train_trunk` switch on the configs and the six factories, the old error with the switch
off, the tape / workspace sizes as host arithmetic, the argument checks of the backward entry points (no GPU needed: they fail before
any launch), and the weight-decay grouping of a trainable trunk."""
import ctypes

import pytest
import torch


def _app_kwargs(pkg, **extra):
    kw = pkg.synth.model_kwargs("cfg1")
    return dict(num_classes=kw["num_classes"], hidden_size=kw["hidden_size"], num_attention_heads=kw["num_attention_heads"],
                hidden_dropout_prob=0.0, appearance_num_frames=32, **extra)


def _mm_kwargs(pkg, **extra):
    return dict(pkg.synth.model_kwargs("cfg1"), appearance_num_frames=32, num_appearance_layers=2, num_fusion_layers=2, **extra)


def test_switch_on_configs_and_factories(pkg):
    assert pkg.AppearanceModelConfig(**_app_kwargs(pkg)).train_trunk is False
    assert pkg.MultimodalModelConfig(**_mm_kwargs(pkg)).train_trunk is False
    assert pkg.AppearanceModelConfig(**_app_kwargs(pkg, train_trunk=True)).train_trunk is True
    assert pkg.MultimodalModelConfig(**_mm_kwargs(pkg, train_trunk=True)).train_trunk is True
    for name in ("resnet3d", "resnet3d-transformer", "lcf", "caf", "cacnf"):
        cfg_cls = pkg.model_configs_factory[name]
        kw = _app_kwargs(pkg, train_trunk=True) if cfg_cls is pkg.AppearanceModelConfig else _mm_kwargs(pkg, appearance_trunk=True, train_trunk=True)
        m = pkg.models_factory[name](cfg_cls(**kw))
        trunks = [t for t in m.modules() if isinstance(t, pkg.Resnet3D)]
        assert len(trunks) == 1 and trunks[0].train_trunk and trunks[0]._runner.train_trunk, name
        off = pkg.models_factory[name](cfg_cls(**{k: v for k, v in kw.items() if k != "train_trunk"}))
        assert not [t for t in off.modules() if isinstance(t, pkg.Resnet3D)][0]._runner.train_trunk, name
    # stlt has no trunk: the switch is accepted and ignored
    pkg.models_factory["stlt"](pkg.model_configs_factory["stlt"](**dict(pkg.synth.model_kwargs("cfg1"), train_trunk=True)))


def test_switch_off_keeps_the_error(pkg):
    m = pkg.Resnet3D(pkg.AppearanceModelConfig(**_app_kwargs(pkg)))
    with pytest.raises(pkg.StltHipError, match=r"resnet\) has trainable parameters, but Conv3d backward is not built: freeze it with "
                                               r"`resnet\.requires_grad_\(False\)`.*train_trunk=True"):
        m.forward_features({"video_frames": torch.zeros(1, 3, 32, 112, 112)})
    # switch on: past the training rule, the CPU tensor is what is refused
    on = pkg.Resnet3D(pkg.AppearanceModelConfig(**_app_kwargs(pkg, train_trunk=True)))
    with pytest.raises(pkg.StltHipError, match="expected a GPU tensor"):
        on.forward_features({"video_frames": torch.zeros(1, 3, 32, 112, 112)})


def test_tape_and_workspaces_are_host_arithmetic(pkg):
    lib = pkg._lib.load()
    for fn in (lib.stlt_r3d_tape_bytes, lib.stlt_r3d_backward_workspace_bytes):
        sizes = [int(fn(B, 32, 112, 112)) for B in (0, 1, 2, 4, 16, 64)]
        assert sizes[0] == 0 and all(a < b for a, b in zip(sizes, sizes[1:])), sizes
    # ~123 MB of tape per 32 x 112 x 112 clip (the stem's padded input, stem, max-pool + argmax, three activations per block)
    assert 110e6 < lib.stlt_r3d_tape_bytes(1, 32, 112, 112) < 135e6
    d = pkg._lib.Conv3dDesc(4, 4, 7, 7, 256, 512, 3, 3, 3, 1, 1, 1, 1, 1, 1)
    assert lib.stlt_conv3d_bwd_data_workspace_bytes(d, 1) == 0
    assert lib.stlt_conv3d_bwd_data_workspace_bytes(d, 3) == 3 * 4 * 4 * 7 * 7 * 256 * 4
    # wgrad: always its (c_out, K) slabs, one per split of the contraction over M
    assert lib.stlt_conv3d_bwd_weight_workspace_bytes(d, 1) == 512 * 27 * 256 * 4
    assert lib.stlt_conv3d_bwd_weight_workspace_bytes(d, 2) == 2 * 512 * 27 * 256 * 4
    bad = pkg._lib.Conv3dDesc(4, 4, 7, 7, 6, 512, 3, 3, 3, 1, 1, 1, 1, 1, 1)
    assert lib.stlt_conv3d_bwd_weight_workspace_bytes(bad, 0) == 0


def test_backward_argument_checks_without_a_gpu(pkg):
    lib = pkg._lib.load()
    fake = ctypes.c_void_p(4096)  # never dereferenced: every call below fails in its host checks
    d = pkg._lib.Conv3dDesc(1, 2, 2, 2, 6, 8, 1, 1, 1, 1, 1, 1, 0, 0, 0)  # c_in not a multiple of 4
    assert lib.stlt_conv3d_bwd_data(ctypes.byref(d), fake, fake, None, None, None, 1, None, 0, fake, None) == -1
    assert b"multiple of 4" in lib.stlt_last_error()
    assert lib.stlt_conv3d_bwd_weight(ctypes.byref(d), fake, fake, None, 6, 0, 1, fake, 1 << 20, fake, None) == -1
    assert b"multiple of 4" in lib.stlt_last_error()
    d = pkg._lib.Conv3dDesc(1, 4, 4, 4, 8, 8, 3, 3, 3, 1, 1, 1, 1, 1, 1)
    assert lib.stlt_conv3d_bwd_data(ctypes.byref(d), None, fake, None, None, None, 1, None, 0, fake, None) == -1
    assert b"null pointer" in lib.stlt_last_error()
    assert lib.stlt_conv3d_bwd_weight(ctypes.byref(d), fake, fake, None, 8, 0, 1, None, 0, fake, None) == -2  # workspace too small
    assert lib.stlt_conv3d_bwd_weight(ctypes.byref(d), fake, fake, None, 9, 0, 1, fake, 1 << 20, fake, None) == -1  # c_in_w > c_in
    assert lib.stlt_maxpool3d_ndhwc_bwd(None, fake, 1, 4, 4, 4, 8, None, fake, None) == -1
    assert lib.stlt_maxpool3d_ndhwc_train(fake, 1, 0, 4, 4, 8, fake, fake, None) == -1
    p = pkg._lib.R3dParams()
    ptrs = pkg._lib.R3dPointers(*([4096] * 53))
    assert lib.stlt_r3d_backward(ctypes.byref(p), ptrs, fake, 1 << 30, 1, 32, 112, 112, fake, None, ptrs, 1, fake, 1 << 30, None) == -1
    assert b"null weight" in lib.stlt_last_error()
    for i in range(53):
        p.conv[i] = pkg._lib.R3dConv(4096, 4096, 4096, 4096, 4096)
    tape = int(lib.stlt_r3d_tape_bytes(1, 32, 112, 112))
    ws = int(lib.stlt_r3d_backward_workspace_bytes(1, 32, 112, 112))
    assert lib.stlt_r3d_backward(ctypes.byref(p), ptrs, fake, tape, 1, 32, 112, 112, fake, fake, ptrs, 1, fake, ws, None) == -1  # both dfeatures and dpooled
    assert lib.stlt_r3d_backward(ctypes.byref(p), ptrs, fake, tape - 1, 1, 32, 112, 112, fake, None, ptrs, 1, fake, ws, None) == -2
    assert lib.stlt_r3d_backward(ctypes.byref(p), ptrs, fake, tape, 1, 32, 112, 112, fake, None, ptrs, 1, fake, ws - 1, None) == -2
    assert lib.stlt_r3d_train_forward(ctypes.byref(p), fake, 1, 32, 112, 112, fake, 1 << 40, fake, tape - 1, fake, None, None) == -2
    assert lib.stlt_r3d_repack_all(None, ctypes.byref(p), ptrs, ptrs, None) == -1
    odd = pkg._lib.R3dPointers(*([4104] * 53))  # 8-byte aligned only
    assert lib.stlt_r3d_repack_all(ptrs, ctypes.byref(p), odd, ptrs, None) == -1
    assert b"16-byte aligned" in lib.stlt_last_error()


def test_weight_decay_groups_with_the_switch_on(pkg):
    m = pkg.Resnet3D(pkg.AppearanceModelConfig(**_app_kwargs(pkg, train_trunk=True)))
    groups = pkg.train.add_weight_decay(m, 1e-3)
    decay = {id(p) for g in groups if g["weight_decay"] > 0 for p in g["params"]}
    convs = [c.weight for c in m.modules() if isinstance(c, torch.nn.Conv3d)]
    assert len(convs) == 53 and all(id(w) in decay for w in convs)
    bns = [p for b in m.modules() if isinstance(b, torch.nn.BatchNorm3d) for p in b.parameters()]
    listed = {id(p) for g in groups for p in g["params"]}
    assert bns and not any(p.requires_grad or id(p) in listed for p in bns)
