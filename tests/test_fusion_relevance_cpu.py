"""Attention relevance of the fusion models without a GPU: the fp64 restatement the GPU tests hold the library to
(tests/fusion_relevance_restated.py) against tests/fusion_attention_restated.py's logits and probabilities, its autograd G_h against the
closed form the kernels compute, the quadrant-wise joint chain against the dense one, the exact zeros that follow from the masks and from
what a head reads, the C-ABI's declarations, the CPU refusal, and the fp32 floor of the whole path — the restatement evaluated in fp32
against fp64 on every case tests/test_fusion_relevance_gpu.py uses, from which that test's bound is made."""
import fnmatch
import functools
import importlib
import os
import re
import sys

import pytest
import torch

import fusion_attention_restated as FR
import fusion_relevance_restated as XR
import relevance_restated as R
from conftest import ROOT
from test_fusion_attention_cpu import EXTRA, fusion_case
from test_relevance_cpu import _rel, make_target

NAMES = ("stlt_attn_grad_probs_cross", "stlt_attn_rollout_joint", "stlt_relevance_combine_joint", "stlt_attn_block_bwd_relevance")
# the whole-path cases of tests/test_fusion_relevance_gpu.py: (model, head, target form), all at the cfg1 fixtures (B = 3, lengths 16 / 14 / 8)
WHOLE_PATH_CASES = [("caf", "caf", "top1"), ("caf", "caf", "classes"), ("caf", "caf", "seed"), ("lcf", "lcf", "top1"), ("lcf", "lcf", "seed"),
                    ("cacnf", "stlt", "top1"), ("cacnf", "resnet3d", "classes"), ("cacnf", "caf", "seed"), ("cacnf", "ensemble", "top1")]
LAYOUT_MAPS = ("spatial_layers", "temporal_layers")
FUSION_MAPS = XR.LAYER_KEYS[3:]


def reached(model_name, head):
    """the per-layer maps whose blocks the head reads (every other map is exactly 0: autograd never visits it)"""
    if head == "stlt":
        return LAYOUT_MAPS
    if head == "resnet3d":
        return ("appearance_layers",)
    return XR.LAYER_KEYS[:3] + (FUSION_MAPS if model_name != "lcf" else ())


def _H(synth):
    return synth.CONFIGS["cfg1"]["num_attention_heads"]


def _synth():
    from conftest import PKG_NAME
    return importlib.import_module(PKG_NAME + ".synth")


@functools.lru_cache(maxsize=None)
def reference(model_name, head, form):
    """(state dict, batch, golden logits file, target, fp64 relevance) of a whole-path case — computed once, shared, never modified.  For
    "top1" the fp64 run picks the classes; a lower precision is held to the same objective through ref["target"]."""
    synth = _synth()
    sd, batch, z = fusion_case(synth, model_name)
    B, K = z[head].shape
    target = make_target(form, B, K)
    ref = XR.relevance(model_name, sd, batch, _H(synth), head, target)
    return sd, batch, z, target, ref


def differenced(k, t):
    """a rollout minus its identity, so that the unit diagonal cannot hide an error; every other output as it is"""
    if k not in XR.ROLLOUT_KEYS:
        return t
    return t - torch.eye(t.shape[-1], dtype=t.dtype, device=t.device)


@pytest.mark.parametrize("model_name", ["caf", "cacnf", "lcf"])
def test_restatement_equals_the_attention_restatement(pkg, model_name):
    """logits and head-mean probabilities of the differentiable forward == tests/fusion_attention_restated.forward_attention, <= 1e-12 in fp64"""
    sd, batch, _ = fusion_case(pkg.synth, model_name)
    want = FR.forward_attention(model_name, sd, batch, _H(pkg.synth))
    logits, nodes = XR.forward(model_name, sd, batch, _H(pkg.synth))
    for k, v in logits.items():
        assert (v.detach() - want[k]).abs().max().item() <= 1e-12, k
    B, T, N = batch["categories"].shape
    mean = lambda ns: [P.detach().mean(dim=1) for P, _, _ in ns]  # noqa: E731
    got = {"spatial_attention": [p.reshape(B, T, N, N) for p in mean(nodes["spatial"])], "temporal_attention": mean(nodes["temporal"]),
           "appearance_attention": mean(nodes["appearance"]), "layout_to_appearance": mean(nodes["l2a"]), "appearance_to_layout": mean(nodes["a2l"]),
           "fusion_layout_attention": mean(nodes["f_layout"]),
           "fusion_appearance_attention": [torch.stack(p) for p in zip(mean(nodes["f_app0"]), mean(nodes["f_app1"]))]}
    avg = FR.head_mean(want)
    for k in FR.MAP_KEYS:
        assert len(got[k]) == avg[k].shape[0], k
        for l, p in enumerate(got[k]):
            assert (p - avg[k][l]).abs().max().item() <= 1e-12, (k, l)


@pytest.mark.parametrize("model_name,head", [("caf", "caf"), ("cacnf", "ensemble"), ("cacnf", "stlt"), ("lcf", "lcf")])
def test_autograd_gradient_equals_the_closed_form(pkg, model_name, head):
    """G_h by autograd wrt P_h equals dctx_h · V_h^T with dctx by autograd wrt ctx_h = P_h @ V_h, for every block the head reads (<= 1e-10)"""
    sd, batch, _ = fusion_case(pkg.synth, model_name)
    logits, nodes = XR.forward(model_name, sd, batch, _H(pkg.synth))
    seed, _ = R.seed_of(logits[head], None)
    G = XR.grad_probs(logits[head], seed, nodes)
    worst, n_read = 0.0, 0
    for kind, ns in nodes.items():
        dctx = torch.autograd.grad((logits[head] * seed).sum(), [c for _, _, c in ns], retain_graph=True, allow_unused=True) if ns else ()
        for (P, V, _), g, dc in zip(ns, G[kind], dctx):
            if dc is None:
                assert (g == 0).all(), kind
                continue
            n_read += 1
            closed = dc @ V.detach().transpose(-1, -2)
            assert g.shape == closed.shape == P.shape
            worst = max(worst, (g - closed).abs().max().item())
            assert (g - closed).abs().max().item() <= 1e-10 and _rel(g, closed) <= 1e-10, (model_name, kind)
    assert n_read > 0
    print(f"\n[fusion relevance] {model_name}/{head}: autograd G vs dctx·V^T over {n_read} blocks, worst abs {worst:.3g}", file=sys.stderr)


def test_closed_form_of_one_block_equals_autograd():
    """fusion_relevance_restated.attn_grad_probs_cross (what the kernel tests compare with) against autograd through ctx = P @ V, cross shapes"""
    g = torch.Generator().manual_seed(4)
    S, Lq, Lk, H, dh = 3, 5, 7, 2, 8
    q, dctx = (torch.randn(S, Lq, H * dh, generator=g, dtype=torch.float64) for _ in range(2))
    k, v = (torch.randn(S, Lk, H * dh, generator=g, dtype=torch.float64) for _ in range(2))
    kpm = torch.rand(S, Lk, generator=g) < 0.3
    kpm[:, 0] = False
    kpm[S - 1] = True
    P = FR.attn_probs_cross(q, k, kpm, False, H, per_head=True).requires_grad_(True)
    ctx = (P @ XR._heads(v, H)).transpose(1, 2).reshape(S, Lq, H * dh)
    (G,) = torch.autograd.grad((ctx * dctx).sum(), P)
    want = R.abar_of(P.detach(), G)
    got = XR.attn_grad_probs_cross(q, k, v, dctx, kpm, False, H)
    assert (got - want).abs().max().item() <= 1e-12 and (got[S - 1] == 0).all() and (got[FR.masked_entries(kpm, False, S, Lq, Lk)] == 0).all()


@pytest.mark.parametrize("T,A,n", [(1, 1, 1), (7, 33, 2), (16, 33, 3), (5, 3, 0)])
def test_quadrant_chain_equals_the_dense_chain(T, A, n):
    g = torch.Generator().manual_seed(T + A + n)
    S, J = 2, T + A
    rnd = lambda *s: torch.rand(*s, generator=g, dtype=torch.float64) / J  # noqa: E731
    args = (torch.eye(T, dtype=torch.float64) + rnd(S, T, T), torch.eye(A, dtype=torch.float64) + rnd(S, A, A), rnd(n, S, T, A), rnd(n, S, A, T), rnd(n, S, T, T),
            rnd(n, 2, S, A, A))
    dense, quad = XR.joint_rollout_dense(*args), XR.joint_rollout_quadrants(*args)
    assert dense.shape == (S, J, J) and (dense - quad).abs().max().item() <= 1e-12 * dense.abs().max().item()
    if n == 0:
        assert torch.equal(dense, XR.blockdiag(args[0], args[1]))


def test_zero_fusion_maps_reduce_to_the_unimodal_rollouts():
    g = torch.Generator().manual_seed(8)
    S, T, A, N = 3, 6, 4, 5
    r_tp = torch.eye(T, dtype=torch.float64) + torch.rand(S, T, T, generator=g, dtype=torch.float64).tril()
    r_app = torch.eye(A, dtype=torch.float64) + torch.rand(S, A, A, generator=g, dtype=torch.float64)
    r_sp = torch.rand(S, T, N, N, generator=g, dtype=torch.float64)
    z = lambda *s: torch.zeros(*s, dtype=torch.float64)  # noqa: E731
    Rj = XR.joint_rollout_dense(r_tp, r_app, z(2, S, T, A), z(2, S, A, T), z(2, S, T, T), z(2, 2, S, A, A))
    assert torch.equal(Rj, XR.blockdiag(r_tp, r_app))
    lengths = torch.tensor([6, 4, 1])
    rel, frame_rel, app_rel = XR.read_out(Rj, r_sp, lengths, T, 1.0, 1.0)
    assert torch.equal(frame_rel, r_tp[torch.arange(S), lengths - 1]) and torch.equal(app_rel, r_app[:, 0])
    assert torch.equal(rel, torch.einsum("bt,btn->btn", frame_rel, r_sp[:, :, 0, :]))
    rel, frame_rel, app_rel = XR.read_out(Rj, r_sp, lengths, T, 0.0, 1.0)
    assert (frame_rel == 0).all() and (rel == 0).all() and torch.equal(app_rel, r_app[:, 0])
    rel, frame_rel, app_rel = XR.read_out(Rj, r_sp, lengths, T, 1.0, 0.0)
    assert (app_rel == 0).all() and torch.equal(frame_rel, r_tp[torch.arange(S), lengths - 1])


@pytest.mark.parametrize("model_name,head,form", WHOLE_PATH_CASES)
def test_exact_zeros_and_non_degeneracy(model_name, head, form):
    """Padded entries are exactly 0 with nothing forced; every map the head reaches has max > 0; every map it does not reach is exactly 0."""
    sd, batch, _, _, ref = reference(model_name, head, form)
    B, T, N = batch["categories"].shape
    A = ref["appearance_rollout"].shape[-1]
    kpm = batch["src_key_padding_mask_frames"].bool()
    assert kpm.any()
    # masked entries of the maps
    assert (ref["temporal_layers"][:, FR.masked_entries(kpm, True, B, T, T)] == 0).all()
    assert (ref["appearance_to_layout_layers"][:, FR.masked_entries(kpm, False, B, A, T)] == 0).all()
    assert (ref["fusion_layout_layers"][:, FR.masked_entries(kpm, True, B, T, T)] == 0).all()
    # a padded frame's column of R is the unit vector, and the outputs there are exactly 0
    Rj = ref["fusion_rollout"]
    cols = XR.padded_joint_columns(batch, A)
    eye = torch.eye(T + A, dtype=Rj.dtype).expand(B, -1, -1)
    assert torch.equal(Rj.transpose(1, 2)[cols], eye.transpose(1, 2)[cols])
    pad = R.padded_entries(batch)
    assert pad.any() and (ref["relevance"][pad] == 0).all() and (ref["frame_relevance"][kpm] == 0).all()
    assert all((ref[k] >= 0).all() for k in XR.OUTPUT_KEYS + XR.LAYER_KEYS)
    for k in XR.LAYER_KEYS:
        if k in reached(model_name, head):
            assert ref[k].numel() > 0 and ref[k].max().item() > 0, k
            print(f"\n[fusion relevance] {model_name}/{head}/{form} max {k}: {ref[k].max().item():.3g}", file=sys.stderr)
        else:
            assert (ref[k] == 0).all(), k
    if head != "resnet3d":
        assert ref["relevance"][~pad].max().item() > 0 and ref["frame_relevance"].max().item() > 0
    if head != "stlt":
        assert ref["appearance_relevance"].max().item() > 0


def test_the_names_are_declared_bound_and_exported(pkg):
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
    assert "models.py:403-431" in header and "ICCV 2021" in header  # the reference lines the joint rollout follows; the rule's source
    assert re.search(r"#define STLT_K_COUNT\s+17\b", header) and len(pkg._lib.K_NAMES) == 17  # no new profiling id
    for op in ("attn_grad_probs_cross", "attn_rollout_joint", "relevance_combine_joint", "RelevanceRecorder"):
        assert callable(getattr(pkg.ops, op))
    for model in ("caf", "cacnf", "lcf", "resnet3d-transformer"):
        assert callable(getattr(pkg.models_factory[model], "forward_relevance"))
    # refusals of the launchers are host arithmetic: nothing is launched, no GPU is needed
    EINVAL = -1
    err = lambda: lib.stlt_last_error().decode()  # noqa: E731
    f = lib.stlt_attn_grad_probs_cross
    assert f(None, 64, None, None, 64, None, None, 0, 1, 4, 4, 1, 64, None, None) == EINVAL and "null" in err()
    assert f(16, 64, 16, 16, 64, 16, 16, 1, 1, 4, 5, 1, 64, 16, None) == EINVAL and "causal" in err()
    assert f(16, 64, 16, 16, 64, 16, 16, 0, 1, 4, 257, 1, 64, 16, None) == EINVAL and "length" in err()
    assert f(16, 64, 16, 16, 64, 16, 16, 0, 1, 4, 4, 1, 257, 16, None) == EINVAL and "head dim" in err()
    assert f(16, 63, 16, 16, 64, 16, 16, 0, 1, 4, 4, 1, 64, 16, None) == EINVAL and "ldq" in err()
    g = lib.stlt_attn_rollout_joint
    assert g(None, None, 16, 16, 16, 16, 1, 1, 257, 4, 16, None) == EINVAL and "token counts" in err()
    assert g(None, None, None, 16, 16, 16, 1, 1, 4, 4, 16, None) == EINVAL and "null" in err()
    assert g(None, None, 16, 16, 16, 16, 65, 1, 4, 4, 16, None) == EINVAL and "layer count" in err()
    h = lib.stlt_relevance_combine_joint
    assert h(16, 16, None, 1, 4, 4, 4, 1.0, 1.0, 16, 16, 16, None) == EINVAL and "null" in err()
    assert h(16, 16, 16, 1, 0, 4, 4, 1.0, 1.0, 16, 16, 16, None) == EINVAL and "shape" in err()


@pytest.mark.parametrize("model_name", ["caf", "cacnf", "lcf"])
def test_forward_relevance_refuses_cpu_tensors(pkg, model_name):
    m = pkg.models_factory[model_name](pkg.MultimodalModelConfig(**dict(pkg.synth.model_kwargs("cfg1"), **EXTRA)))
    m.train(False)
    c = pkg.synth.CONFIGS["cfg1"]
    batch = pkg.synth.make_batch(2, c["T"], c["N"], seed=1)
    batch["appearance_features"] = pkg.synth.make_appearance_features(2, seed=2)
    with pytest.raises(pkg.StltHipError, match="CPU"):
        m.forward_relevance(batch)


@pytest.mark.parametrize("model_name,head,form", WHOLE_PATH_CASES)
def test_fp32_floor_of_the_whole_path(model_name, head, form):
    """The restatement in fp32 against itself in fp64, same objective: max|fp32 - fp64| / max|fp64| per output, the four rollouts minus their
    identity.  The largest value over all cases is the `f` of tests/test_fusion_relevance_gpu.py's bound max(2e-4, 4 f), kept there as
    FP32_FLOOR.  torch's fp32 CPU sums change order from run to run, so what is asserted is that no case leaves the band the bound grants
    a different summation order, 4 f — the GPU's allowance, nothing wider."""
    gpu_test = importlib.import_module("test_fusion_relevance_gpu")
    sd, batch, _, target, ref = reference(model_name, head, form)
    low = XR.relevance(model_name, sd, batch, _H(_synth()), head, target if target is not None else ref["target"], dtype=torch.float32)
    worst = 0.0
    for k in XR.OUTPUT_KEYS:
        assert low[k].dtype == torch.float32
        want = differenced(k, ref[k])
        if want.abs().max().item() == 0:  # an output the head does not reach: exactly 0 in either precision
            assert (differenced(k, low[k]) == 0).all(), k
            continue
        e = _rel(differenced(k, low[k]), want)
        worst = max(worst, e)
        print(f"\n[fusion relevance] fp32 floor {model_name}/{head}/{form} {k}: {e:.3g}", file=sys.stderr)
    print(f"\n[fusion relevance] fp32 floor {model_name}/{head}/{form} f = {worst:.3g}", file=sys.stderr)
    assert worst <= 4 * gpu_test.FP32_FLOOR <= gpu_test.CAP, (model_name, head, form, worst)
