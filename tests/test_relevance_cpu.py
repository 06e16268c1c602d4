"""Attention relevance without a GPU: the fp64 restatement the GPU tests hold the library to (tests/relevance_restated.py) against the goldens'
logits, its autograd G_h against the closed form the kernel computes, the exact zeros that follow from the masks, the C-ABI's declarations,
and the fp32 floor of the whole path — the restatement evaluated in fp32 against fp64 on every case tests/test_relevance_gpu.py uses, from
which that test's bound is made."""
import functools
import importlib
import os
import re
import sys

import pytest
import torch

import attention_restated as AR
import relevance_restated as R
from conftest import PKG_NAME, ROOT, golden_case

# the whole-path cases of tests/test_relevance_gpu.py: (golden case, target form)
WHOLE_PATH_CASES = [("cfg1", "top1"), ("cfg1", "classes"), ("cfg1", "seed"), ("odd", "top1"), ("odd", "seed"), ("heads", "top1"), ("heads", "classes"),
                    ("cfg2p", "top1")]
MAPS = ("relevance", "spatial_rollout", "temporal_rollout")


def _rel(got, ref):  # tests/test_layout_gradients_gpu.py's measure
    return (got.detach().cpu().double() - ref).abs().max().item() / max(ref.abs().max().item(), 1e-30)


def _heads(name):
    return importlib.import_module(PKG_NAME + ".synth").CONFIGS[name]["num_attention_heads"]


def make_target(form, B, K):
    """the target argument of a whole-path case (shared with the GPU test): None, seeded int64 classes, or a seeded multi-hot float seed"""
    if form == "top1":
        return None
    if form == "classes":
        return torch.randint(0, K, (B,), generator=torch.Generator().manual_seed(11))
    seed = (torch.rand(B, K, generator=torch.Generator().manual_seed(9)) < 0.03).float()
    seed[:, 1] = 1.0  # never an empty row
    return seed


@functools.lru_cache(maxsize=None)
def reference(name, form):
    """(state dict, batch, golden logits, target, fp64 relevance) of a whole-path case — computed once, shared, never modified.  For "top1"
    the fp64 run picks the classes; they are returned as the explicit target so that a lower precision is held to the same objective."""
    sd, batch, z, _ = golden_case(name)
    gold = torch.from_numpy(z["logits"])
    target = make_target(form, *gold.shape)
    ref = R.relevance(sd, batch, _heads(name), target)
    return sd, batch, gold, target, ref


@pytest.mark.parametrize("name", ["cfg1", "odd", "heads"])
def test_restatement_logits_equal_the_goldens(name):
    sd, batch, gold, _, ref = reference(name, "top1")
    err = (ref["stlt"] - gold.double()).abs().max().item()
    print(f"\n[relevance] {name}: restated fp64 logits vs golden: {err:.3g}", file=sys.stderr)
    assert ref["stlt"].shape == gold.shape and err <= 1e-4


@pytest.mark.parametrize("name", ["cfg1", "odd", "heads"])
def test_autograd_gradient_equals_the_closed_form(name):
    """G_h by autograd wrt P_h equals dctx_h · V_h^T with dctx by autograd wrt ctx_h = P_h @ V_h: two derivations of one quantity, to 1e-10
    (absolute, and relative to the largest entry)."""
    sd, batch, _, _, _ = reference(name, "top1")
    logits, spatial, temporal = R.forward(sd, batch, _heads(name))
    seed, _ = R.seed_of(logits, None)
    nodes = spatial + temporal
    G = R.grad_probs(logits, seed, nodes)
    dctx = torch.autograd.grad((logits * seed).sum(), [c for _, _, c in nodes], retain_graph=True)
    worst = 0.0
    for (P, V, _), g, dc in zip(nodes, G, dctx):
        closed = dc @ V.detach().transpose(-1, -2)
        assert g.shape == closed.shape == P.shape
        err = (g - closed).abs().max().item()
        worst = max(worst, err)
        assert err <= 1e-10 and _rel(g, closed) <= 1e-10, (name, err)
    assert any(g.abs().max().item() > 0 for g in G)
    print(f"\n[relevance] {name}: autograd G vs dctx·V^T, worst abs {worst:.3g}", file=sys.stderr)


@pytest.mark.parametrize("name,form", [("cfg1", "top1"), ("odd", "seed"), ("heads", "classes")])
def test_masked_entries_and_padded_relevance_are_exactly_zero(name, form):
    sd, batch, _, _, ref = reference(name, form)
    B, T, N = batch["categories"].shape
    m_sp = AR.masked_entries(batch["src_key_padding_mask_boxes"].reshape(B * T, N), False).reshape(B, T, N, N)
    m_tp = AR.masked_entries(batch["src_key_padding_mask_frames"], True)
    assert ref["spatial_layers"].shape[1:] == (B, T, N, N) and ref["temporal_layers"].shape[1:] == (B, T, T)
    assert (ref["spatial_layers"][:, m_sp] == 0).all() and (ref["temporal_layers"][:, m_tp] == 0).all()
    pad = R.padded_entries(batch)
    assert pad.any() and (ref["relevance"][pad] == 0).all()
    assert (ref["relevance"] >= 0).all() and ref["relevance"][~pad].max().item() > 0
    # the last layer of a tower is read at the CLS rows / at frame lengths-1 only: no other row of its map carries a gradient
    assert (ref["spatial_layers"][-1][:, :, 1:, :] == 0).all()
    last = torch.zeros(B, T, dtype=torch.bool)
    last[torch.arange(B), batch["lengths"] - 1] = True
    assert (ref["temporal_layers"][-1][~last] == 0).all()


def test_header_declares_the_entry_points_and_each_has_a_signature(pkg):
    header = open(os.path.join(ROOT, "include", "stlt_hip.h")).read()
    for name in ("stlt_attn_grad_probs", "stlt_attn_rollout", "stlt_relevance_combine", "stlt_train_backward_relevance"):
        assert re.search(rf"\bint {name}\s*\(", header), f"{name} is not declared in include/stlt_hip.h"
        assert name in pkg._lib.SIGNATURES, f"{name} has no ctypes signature"
    assert re.search(r"\}\s*stlt_relevance_maps;", header)
    assert [f for f, _ in pkg._lib.RelevanceMaps._fields_] == ["abar_spatial", "abar_temporal", "rollout_spatial", "rollout_temporal", "relevance"]
    # no new profiling id: the new launches are recorded under attn_probs and misc
    assert re.search(r"#define STLT_K_COUNT\s+17\b", header) and len(pkg._lib.K_NAMES) == 17
    for api in ("forward_relevance",):
        assert callable(getattr(pkg.Stlt, api))
    for op in ("attn_grad_probs", "attn_rollout", "relevance_combine"):
        assert callable(getattr(pkg.ops, op))


@pytest.mark.parametrize("name,form", WHOLE_PATH_CASES)
def test_fp32_floor_of_the_whole_path(name, form):
    """The restatement in fp32 against itself in fp64, same objective: max|fp32 - fp64| / max|fp64| of rel and of both rollouts.  The largest
    value over all cases is the `f` of tests/test_relevance_gpu.py's bound max(2e-4, 4 f), kept there as FP32_FLOOR.  torch's fp32 CPU
    products are threaded and their sums change order from run to run (2.3e-7 ... 3.5e-7 for the worst case seen), so what is asserted is
    that no case leaves the band the bound grants a different summation order, 4 f — the GPU's allowance, nothing wider."""
    gpu_test = importlib.import_module("test_relevance_gpu")
    sd, batch, _, target, ref = reference(name, form)
    low = R.relevance(sd, batch, _heads(name), target if target is not None else ref["target"], dtype=torch.float32)
    worst = 0.0
    for k in MAPS:
        assert low[k].dtype == torch.float32
        e = _rel(low[k], ref[k])
        worst = max(worst, e)
        print(f"\n[relevance] fp32 floor {name}/{form} {k}: {e:.3g}", file=sys.stderr)
    assert worst <= 4 * gpu_test.FP32_FLOOR <= gpu_test.CAP, (name, form, worst)
