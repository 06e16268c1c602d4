"""R3D-50 trunk models on CPU: state-dict schemas equal the reference's (tests/golden/*r3d*_schema.json, captured by
tools/gen_golden_r3d.py), reference-shaped checkpoints load, the factories know the reference's six names, the trunk workspace is
host arithmetic, and the fusion models' key lists are unchanged with the trunk switch off."""
import json
import os

import pytest
import torch

from conftest import GOLDEN


def _schema(name):
    return json.load(open(os.path.join(GOLDEN, name)))


def _app_kwargs(pkg, **extra):
    kw = pkg.synth.model_kwargs("cfg1")
    return dict(num_classes=kw["num_classes"], hidden_size=kw["hidden_size"], num_attention_heads=kw["num_attention_heads"],
                hidden_dropout_prob=0.0, appearance_num_frames=32, **extra)


def _mm_config(pkg, **extra):
    return pkg.MultimodalModelConfig(**dict(pkg.synth.model_kwargs("cfg1"), appearance_num_frames=32, num_appearance_layers=2, num_fusion_layers=2,
                                            **extra))


def _check_schema(sd, meta):
    assert list(sd) == list(meta["keys"])  # same keys, same order
    for k, v in sd.items():
        assert list(v.shape) == meta["keys"][k]["shape"], k
        assert str(v.dtype).replace("torch.", "") == meta["keys"][k]["dtype"], k


def test_resnet3d_schema_matches_reference(pkg):
    meta = _schema("r3d_schema.json")
    m = pkg.Resnet3D(pkg.AppearanceModelConfig(**_app_kwargs(pkg)))
    _check_schema(m.state_dict(), meta)
    assert len(meta["keys"]) == 320 and sum(1 for k in meta["keys"] if k.startswith("resnet.")) == 318
    # BatchNorm affine parameters frozen, conv weights trainable (models.py:207-211); BatchNorm stays in eval mode
    bns = [b for b in m.modules() if isinstance(b, torch.nn.BatchNorm3d)]
    convs = [c for c in m.modules() if isinstance(c, torch.nn.Conv3d)]
    assert len(bns) == len(convs) == 53
    assert not any(p.requires_grad for b in bns for p in b.parameters()) and all(c.weight.requires_grad for c in convs)
    m.train(True)
    assert all(not b.training for b in m.modules() if isinstance(b, torch.nn.BatchNorm3d))


def test_transformer_resnet_schema_matches_reference(pkg):
    meta = _schema("r3d_transformer_schema.json")
    m = pkg.TransformerResnet(pkg.AppearanceModelConfig(**_app_kwargs(pkg)))
    _check_schema(m.state_dict(), meta)
    assert len(meta["keys"]) == 374


def test_cacnf_with_trunk_schema_matches_reference(pkg):
    meta = _schema("cacnf_trunk_cfg1_schema.json")
    m = pkg.CrossAttentionCentralNetFusion(_mm_config(pkg, appearance_trunk=True))
    _check_schema(m.state_dict(), meta)
    sd = pkg.synth.make_r3d_state_dict({k: tuple(v["shape"]) for k, v in meta["keys"].items()}, seed=meta["weight_seed"])
    m.load_state_dict(sd, strict=True)
    assert sum(1 for k in m.state_dict() if ".appearance_branch.resnet." in k) == 320


@pytest.mark.parametrize("name", ["caf", "cacnf", "lcf"])
def test_switch_off_keeps_fusion_keys(pkg, name):
    """appearance_trunk defaults to off: the state dict is the one of the precomputed-feature models, key for key"""
    meta = json.load(open(os.path.join(GOLDEN, f"{name}_cfg1_schema.json")))
    m = pkg.models_factory[name](_mm_config(pkg))
    assert list(m.state_dict()) == list(meta["keys"])
    on = pkg.models_factory[name](_mm_config(pkg, appearance_trunk=True))
    assert len(on.state_dict()) == len(meta["keys"]) + 320 and not _mm_config(pkg).appearance_trunk
    # the reference model's key count (recorded with these goldens by tools/gen_golden_caf.py)
    assert len(on.state_dict()) == meta["n_reference_keys"]


def test_factories_know_the_reference_names(pkg):
    names = {"stlt", "resnet3d", "resnet3d-transformer", "lcf", "caf", "cacnf"}
    assert set(pkg.models_factory) == names and set(pkg.model_configs_factory) == names
    assert pkg.models_factory["resnet3d"] is pkg.Resnet3D and pkg.models_factory["resnet3d-transformer"] is pkg.TransformerResnet
    assert pkg.model_configs_factory["resnet3d"] is pkg.AppearanceModelConfig
    assert pkg.model_configs_factory["lcf"] is pkg.MultimodalModelConfig


def test_reference_state_dict_and_checkpoint_file_load(pkg, tmp_path):
    meta = _schema("r3d_schema.json")
    sd = pkg.synth.make_r3d_state_dict({k: tuple(v["shape"]) for k, v in meta["keys"].items()}, seed=meta["weight_seed"])
    m = pkg.Resnet3D(pkg.AppearanceModelConfig(**_app_kwargs(pkg)))
    m.load_state_dict(sd, strict=True)
    # a full-ResNet checkpoint as the reference's constructor reads it: {"state_dict": conv1 / bn1 / layer1-4 / fc}
    names = {"0": "conv1", "1": "bn1", "4": "layer1", "5": "layer2", "6": "layer3", "7": "layer4"}
    full = {}
    for k, v in sd.items():
        if k.startswith("resnet."):
            head, _, tail = k[len("resnet."):].partition(".")
            full[f"{names[head]}.{tail}"] = v
    full["fc.weight"], full["fc.bias"] = torch.zeros(1139, 2048), torch.zeros(1139)
    path = str(tmp_path / "r3d50.pth")
    torch.save({"state_dict": full}, path)
    m2 = pkg.Resnet3D(pkg.AppearanceModelConfig(**_app_kwargs(pkg, resnet_model_path=path)))
    for k, v in m2.resnet.state_dict().items():
        assert torch.equal(v, sd["resnet." + k]), k
    # ... and the fusion models read it with the switch on
    mm = pkg.CrossAttentionFusion(_mm_config(pkg, appearance_trunk=True, resnet_model_path=path))
    assert torch.equal(mm.caf_backbone.appearance_branch.resnet.resnet[7][2].conv3.weight, sd["resnet.7.2.conv3.weight"])
    del full["fc.bias"]
    torch.save({"state_dict": full}, path)
    with pytest.raises(RuntimeError):
        pkg.Resnet3D(pkg.AppearanceModelConfig(**_app_kwargs(pkg, resnet_model_path=path)))


def test_r3d_workspace_is_host_arithmetic(pkg):
    lib = pkg._lib.load()
    sizes = [int(lib.stlt_r3d_workspace_bytes(B, 32, 112, 112)) for B in (0, 1, 2, 4, 16, 64)]
    assert sizes[0] == 0
    assert all(a < b for a, b in zip(sizes, sizes[1:])), sizes
    # the op-level conv's split workspace: 0 for an unsplit launch, slabs of M x c_out floats otherwise
    d = pkg._lib.Conv3dDesc(4, 4, 7, 7, 1024, 512, 3, 3, 3, 1, 1, 1, 1, 1, 1)
    assert lib.stlt_conv3d_workspace_bytes(d, 1) == 0
    assert lib.stlt_conv3d_workspace_bytes(d, 3) == 3 * 4 * 4 * 7 * 7 * 512 * 4


def test_trunk_refuses_cpu_tensors(pkg):
    m = pkg.Resnet3D(pkg.AppearanceModelConfig(**_app_kwargs(pkg)))
    with torch.no_grad(), pytest.raises(pkg.StltHipError):
        m.forward_features({"video_frames": torch.zeros(1, 3, 32, 112, 112)})
    # autograd on with a trainable trunk: an error naming the fix, before anything runs
    with pytest.raises(pkg.StltHipError, match=r"requires_grad_\(False\)"):
        m.forward_features({"video_frames": torch.zeros(1, 3, 32, 112, 112)})
