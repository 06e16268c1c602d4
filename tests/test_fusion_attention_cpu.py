"""Attention maps of the fusion models, host side: the fp64 restatement (tests/fusion_attention_restated.py) against the fixtures captured
from the reference's own nn.MultiheadAttention modules (tools/gen_golden_fusion_attention.py), exact zeros where keys are masked, the CPU
refusal of forward_attention and the three names in the header, the ctypes table and the export map.  No GPU."""
import fnmatch
import functools
import json
import os
import re

import numpy as np
import pytest
import torch

import fusion_attention_restated as FR
from conftest import GOLDEN, ROOT

NAMES = ("stlt_attn_probs_cross_fwd", "stlt_caf_attention_workspace_bytes", "stlt_caf_forward_attention")
EXTRA = dict(appearance_num_frames=32, num_appearance_layers=2, num_fusion_layers=2)


def fusion_case(synth, model_name):
    """(state dict, batch, golden logits) of tests/golden/<model>_cfg1.npz, as tests/test_caf.py builds them"""
    z = np.load(os.path.join(GOLDEN, f"{model_name}_cfg1.npz"))
    meta = json.load(open(os.path.join(GOLDEN, f"{model_name}_cfg1_schema.json")))
    c = synth.CONFIGS["cfg1"]
    sd = synth.make_state_dict({k: tuple(v) for k, v in meta["keys"].items()}, seed=meta["weight_seed"])
    batch = synth.make_batch(meta["batch"], c["T"], c["N"], seed=meta["input_seed"])
    batch["appearance_features"] = synth.make_appearance_features(meta["batch"], seed=meta["feature_seed"])
    return sd, batch, z


@functools.lru_cache(maxsize=None)
def _case(synth, model_name):
    """(batch, golden logits, fixture, fp64 restatement) — computed once, shared, never modified"""
    sd, batch, z = fusion_case(synth, model_name)
    fx = np.load(os.path.join(GOLDEN, f"{model_name}_attention_cfg1.npz"))
    ref = FR.forward_attention(model_name, sd, batch, synth.CONFIGS["cfg1"]["num_attention_heads"])
    return batch, z, fx, ref


@pytest.mark.parametrize("model_name", ["caf", "cacnf"])
def test_restatement_matches_the_reference_fixture(pkg, model_name):
    """Maps <= 5e-5 max-abs, logits <= 2e-5: the bounds of tests/test_attention_cpu.py for the same comparison (the fixture is the
    reference's fp32)."""
    batch, z, fx, ref = _case(pkg.synth, model_name)
    assert set(fx.files) == set(FR.FIXTURE_KEYS.values()) | set(z.files) and all(fx[k].dtype == np.float32 for k in fx.files)
    assert all(np.array_equal(fx[k], z[k]) for k in z.files)  # the fixture's run is the golden's run
    avg = FR.head_mean(ref)
    for k in FR.MAP_KEYS:
        want = torch.from_numpy(fx[FR.FIXTURE_KEYS[k]]).double()
        assert tuple(avg[k].shape) == tuple(want.shape), k
        err = (avg[k] - want).abs().max().item()
        print(f"{model_name}: restatement vs reference fixture: {k} {err:.3g}")
        assert err <= 5e-5, k
        assert (ref[k].sum(-1) - 1).abs().max().item() <= 1e-9, k  # every row here has a visible key
    for k in z.files:
        err = (ref[k] - torch.from_numpy(z[k]).double()).abs().max().item()
        print(f"{model_name}: restatement vs reference fixture: logits {k} {err:.3g}")
        assert err <= 2e-5, k


@pytest.mark.parametrize("model_name", ["caf", "cacnf"])
def test_masked_entries_are_exactly_zero_in_fixture_and_restatement(pkg, model_name):
    batch, _, fx, ref = _case(pkg.synth, model_name)
    B, T, _ = batch["categories"].shape
    kpm = batch["src_key_padding_mask_frames"]
    A = fx["appearance"].shape[-1]
    H = ref["appearance_to_layout"].shape[2]
    m_a2l = FR.masked_entries(kpm, False, B, A, T)
    m_lay = FR.masked_entries(kpm, True, B, T, T)
    assert m_a2l.any() and m_lay.any() and int(kpm.sum(1).max()) >= 8  # clips with padded frames
    assert (torch.from_numpy(fx["appearance_to_layout"])[:, m_a2l] == 0).all() and (torch.from_numpy(fx["fusion_layout"])[:, m_lay] == 0).all()
    assert (ref["appearance_to_layout"][:, m_a2l[:, None].expand(B, H, A, T)] == 0).all()
    assert (ref["fusion_layout_attention"][:, m_lay[:, None].expand(B, H, T, T)] == 0).all()
    assert (ref["layout_to_appearance"] > 0).all() and (ref["fusion_appearance_attention"] > 0).all()  # no mask there


def test_lcf_restatement_has_no_fusion_maps(pkg):
    sd, batch, z = fusion_case(pkg.synth, "lcf")
    ref = FR.forward_attention("lcf", sd, batch, pkg.synth.CONFIGS["cfg1"]["num_attention_heads"])
    assert (ref["lcf"] - torch.from_numpy(z["lcf"]).double()).abs().max().item() <= 2e-5
    assert all(ref[k].shape[0] == 0 for k in FR.MAP_KEYS[3:]) and ref["appearance_attention"].shape[0] == 2


def test_cross_probs_restatement_on_edge_masks():
    """every key masked: zeros; only key 0 unmasked: column 0 is exactly 1; the head average is the mean of the per-head maps; with q and k
    of one packed buffer it is tests/attention_restated.py's attn_probs"""
    import attention_restated as R
    g = torch.Generator().manual_seed(3)
    S, Lq, Lk, H, dh = 3, 5, 7, 2, 8
    q = torch.randn(S, Lq, H * dh, generator=g, dtype=torch.float64)
    k = torch.randn(S, Lk, H * dh, generator=g, dtype=torch.float64)
    kpm = torch.zeros(S, Lk, dtype=torch.bool)
    kpm[0, :] = True
    kpm[1, 1:] = True
    p = FR.attn_probs_cross(q, k, kpm, False, H, per_head=True)
    assert p.shape == (S, H, Lq, Lk) and (p[0] == 0).all() and (p[1, :, :, 0] == 1).all() and (p[1, :, :, 1:] == 0).all()
    assert (p[2].sum(-1) - 1).abs().max().item() <= 1e-12
    assert torch.equal(FR.attn_probs_cross(q, k, kpm, False, H), p.mean(1))
    qkv = torch.randn(S, Lk, 3 * H * dh, generator=g, dtype=torch.float64)
    for causal in (False, True):
        assert torch.equal(FR.attn_probs_cross(qkv[..., :H * dh], qkv[..., H * dh:2 * H * dh], kpm, causal, H, True), R.attn_probs(qkv, kpm, causal, H, True))


@pytest.mark.parametrize("model_name", ["caf", "cacnf", "lcf"])
def test_forward_attention_refuses_cpu_tensors(pkg, model_name):
    m = pkg.models_factory[model_name](pkg.MultimodalModelConfig(**dict(pkg.synth.model_kwargs("cfg1"), **EXTRA)))
    m.train(False)
    c = pkg.synth.CONFIGS["cfg1"]
    batch = pkg.synth.make_batch(2, c["T"], c["N"], seed=1)
    batch["appearance_features"] = pkg.synth.make_appearance_features(2, seed=2)
    with pytest.raises(pkg.StltHipError, match="CPU"):
        m.forward_attention(batch)
    with pytest.raises(pkg.StltHipError):
        m.forward_attention(batch, per_head=True)


def test_the_three_names_are_declared_bound_and_exported(pkg):
    header = open(os.path.join(ROOT, "include", "stlt_hip.h")).read()
    declared = set(re.findall(r"\b(stlt_[a-z0-9_]+)\s*\(", header))
    export_map = open(os.path.join(ROOT, "revisiting-spatial-temporal-layouts_amd", "csrc", "exports.map")).read()
    patterns = re.search(r"global:([^;]*);", export_map).group(1).split()
    lib = pkg._lib.load()
    for name in NAMES:
        assert name in declared, f"{name} is not declared in include/stlt_hip.h"
        assert name in pkg._lib.SIGNATURES, f"{name} has no ctypes signature"
        assert any(fnmatch.fnmatchcase(name, pat) for pat in patterns), f"{name} is not a global of csrc/exports.map"
        assert hasattr(lib, name)
    assert "models.py:362-382" in header and "models.py:353-388" in header  # the reference lines the three calls extend
    assert "stlt_caf_attention_maps" in header and len(pkg._lib.CafAttentionMaps._fields_) == 7
    assert lib.stlt_version() == 111
    # workspace sizing is host arithmetic: the fusion forward's buffers
    args = (8, 32, 7, 768, 2048, 32, 174)
    assert lib.stlt_caf_attention_workspace_bytes(*args) == lib.stlt_caf_workspace_bytes(*args) > 0
    assert lib.stlt_caf_attention_workspace_bytes(0, 32, 7, 768, 2048, 32, 174) == 0
    # refusals of the kernel's launcher are host arithmetic too: nothing is launched, no GPU is needed
    EINVAL = -1
    f = lib.stlt_attn_probs_cross_fwd
    assert f(None, 64, None, 64, None, 0, 1, 4, 4, 1, 64, 0, None, None) == EINVAL
    assert f(16, 64, 16, 64, 16, 1, 1, 4, 5, 1, 64, 0, 16, None) == EINVAL and b"causal" in lib.stlt_last_error()
    assert f(16, 64, 16, 64, 16, 0, 1, 4, 1025, 1, 64, 0, 16, None) == EINVAL and f(16, 64, 16, 64, 16, 0, 1, 4, 4, 1, 257, 0, 16, None) == EINVAL
    assert f(16, 64, 16, 64, 16, 0, 1, 4, 4, 1, 64, 2, 16, None) == EINVAL and b"per_head" in lib.stlt_last_error()
    assert f(20, 64, 16, 64, 16, 0, 1, 4, 4, 1, 64, 0, 16, None) == EINVAL and b"aligned" in lib.stlt_last_error()
    assert f(16, 66, 16, 64, 16, 0, 1, 4, 4, 1, 64, 0, 16, None) == EINVAL and f(16, 32, 16, 64, 16, 0, 1, 4, 4, 1, 64, 0, 16, None) == EINVAL
