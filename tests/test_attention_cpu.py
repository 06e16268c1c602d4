"""Attention maps, host side: the fp64 restatement (tests/attention_restated.py) against the fixtures captured from the reference's own
nn.MultiheadAttention modules (tools/gen_golden_attention.py), its row sums and exact zeros, the CPU refusal of Stlt.forward_attention and
the three names in the header, the ctypes table and the export map.  No GPU."""
import fnmatch
import functools
import os
import re

import numpy as np
import pytest
import torch

import attention_restated as R
from conftest import GOLDEN, ROOT, golden_case

FIXTURES = ["cfg1", "cfg2p", "heads", "odd"]
NAMES = ("stlt_attn_probs_fwd", "stlt_attention_workspace_bytes", "stlt_forward_attention")


@functools.lru_cache(maxsize=None)
def _case(pkg_synth, name):
    """(batch, golden logits, fixture, fp64 restatement) — computed once, shared, never modified"""
    sd, batch, z, meta = golden_case(name)
    fx = np.load(os.path.join(GOLDEN, f"attention_{name}.npz"))
    ref = R.forward_attention(sd, batch, pkg_synth.CONFIGS[name]["num_attention_heads"])
    return batch, z["logits"], fx, ref


@pytest.mark.parametrize("name", FIXTURES)
def test_restatement_matches_the_reference_fixture(pkg, name):
    """Maps <= 5e-5 max-abs (the bound tests/test_oracle_golden.py applies to layer taps: the fixture is the reference's fp32), logits <= 2e-5."""
    batch, gold_logits, fx, ref = _case(pkg.synth, name)
    assert set(fx.files) == {"spatial", "temporal", "logits"} and all(fx[k].dtype == np.float32 for k in fx.files)
    assert np.array_equal(fx["logits"], gold_logits)  # the fixture's run is the golden's run
    sp, tp = ref["spatial_attention"].mean(dim=3), ref["temporal_attention"].mean(dim=2)
    assert tuple(sp.shape) == fx["spatial"].shape and tuple(tp.shape) == fx["temporal"].shape
    e_sp = (sp - torch.from_numpy(fx["spatial"]).double()).abs().max().item()
    e_tp = (tp - torch.from_numpy(fx["temporal"]).double()).abs().max().item()
    e_lg = (ref["stlt"] - torch.from_numpy(fx["logits"]).double()).abs().max().item()
    print(f"{name}: restatement vs reference fixture: spatial {e_sp:.3g} temporal {e_tp:.3g} logits {e_lg:.3g}")
    assert e_sp <= 5e-5 and e_tp <= 5e-5
    assert e_lg <= 2e-5


@pytest.mark.parametrize("name", FIXTURES)
def test_restatement_rows_sum_to_one_and_masked_entries_are_zero(pkg, name):
    batch, _, fx, ref = _case(pkg.synth, name)
    B, T, N = batch["categories"].shape
    m_sp = R.masked_entries(batch["src_key_padding_mask_boxes"].reshape(B * T, N), False).reshape(B, T, N, N)
    m_tp = R.masked_entries(batch["src_key_padding_mask_frames"], True)
    sp, tp = ref["spatial_attention"], ref["temporal_attention"]
    assert sp.dtype == torch.float64 and (sp.sum(-1) - 1).abs().max().item() <= 1e-9 and (tp.sum(-1) - 1).abs().max().item() <= 1e-9
    assert (sp[:, m_sp[:, :, None].expand(B, T, sp.shape[3], N, N)] == 0).all() and (tp[:, m_tp[:, None].expand(B, tp.shape[2], T, T)] == 0).all()
    assert m_sp.any() and m_tp.any() and (sp > 0).any()
    # the reference's own weights are zero in the same places
    assert (torch.from_numpy(fx["spatial"])[:, m_sp] == 0).all() and (torch.from_numpy(fx["temporal"])[:, m_tp] == 0).all()


def test_attn_probs_restatement_on_edge_masks():
    """every key masked: zeros; only key 0 unmasked: column 0 is exactly 1; the head average is the mean of the per-head maps"""
    g = torch.Generator().manual_seed(3)
    S, L, H, dh = 3, 7, 2, 8
    qkv = torch.randn(S, L, 3 * H * dh, generator=g, dtype=torch.float64)
    kpm = torch.zeros(S, L, dtype=torch.bool)
    kpm[0, :] = True
    kpm[1, 1:] = True
    for causal in (False, True):
        p = R.attn_probs(qkv, kpm, causal, H, per_head=True)
        assert p.shape == (S, H, L, L) and (p[0] == 0).all() and (p[1, :, :, 0] == 1).all() and (p[1, :, :, 1:] == 0).all()
        assert (p[2].sum(-1) - 1).abs().max().item() <= 1e-12
        assert torch.equal(R.attn_probs(qkv, kpm, causal, H), p.mean(1))
        assert (p.transpose(1, 0)[:, R.masked_entries(kpm, causal)] == 0).all()


def test_forward_attention_refuses_cpu_tensors(pkg):
    m = pkg.Stlt(pkg.StltModelConfig(**pkg.synth.model_kwargs("micro")))
    m.train(False)
    c = pkg.synth.CONFIGS["micro"]
    batch = pkg.synth.make_batch(2, c["T"], c["N"], seed=1)
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
    assert "models.py:46-55,118-128" in header  # the reference lines the three calls extend
    assert re.search(r"#define STLT_K_ATTN_PROBS\s+15\b", header) and pkg._lib.K_NAMES[15] == "attn_probs"
    assert lib.stlt_version() == 111
    # workspace sizing is host arithmetic: the dense forward's buffers
    assert pkg.ops.attention_workspace_bytes(8, 32, 7, 768, 174) == pkg.ops.workspace_bytes(8, 32, 7, 768, 174) > 0
    assert pkg.ops.attention_workspace_bytes(0, 32, 7, 768, 174) == 0
