"""Integrated gradients, host side: the NumPy restatement (tests/ig_restated.py) on a function whose integral the trapezoid rule gets
exactly, its bitwise endpoints, the names in the header, the ctypes table, the ops wrappers and the export map, the refusals that need no
GPU, and the condition the GPU tolerance rests on: the oracle's own float32 run stays within a quarter of the bound of its fp64 run.  No GPU."""
import fnmatch
import inspect
import os
import re
import sys

import numpy as np
import pytest
import torch

import ig_cases as IC
import ig_restated as R
from conftest import ROOT

NAMES = ("stlt_ig_path", "stlt_ig_path_dense", "stlt_ig_reduce", "stlt_ig_delta_scratch_bytes", "stlt_ig_delta", "stlt_cell_pool_sum")
WRAPPERS = ("ig_path", "ig_path_dense", "ig_reduce", "ig_delta", "cell_pool_sum")


def _report(what, value):
    print(f"\n[integrated gradients] {what}: {value}", file=sys.stderr)


@pytest.mark.parametrize("steps", [1, 2, 7])
def test_trapezoid_is_exact_on_a_quadratic(steps):
    """F(x) = x'Ax + b'x: the gradient is linear in alpha, so the trapezoid rule integrates it exactly and delta is 0 to fp64 rounding"""
    g = np.random.default_rng(3)
    n = 9
    A, b = g.standard_normal((n, n)), g.standard_normal(n)
    x, x0 = g.standard_normal((2, n)), g.standard_normal((2, n))
    F = lambda v: np.einsum("bi,ij,bj->b", v, A, v) + v @ b  # noqa: E731
    acc = np.zeros_like(x)
    for s in range(steps + 1):
        p = x0 + (s / steps) * (x - x0)
        w = 1 / (2 * steps) if s in (0, steps) else 1 / steps
        acc += w * (p @ (A + A.T) + b)
    attr = (x - x0) * acc
    delta = attr.sum(axis=1) - (F(x) - F(x0))
    scale = np.abs(attr).sum(axis=1)
    _report(f"quadratic, steps={steps}: |delta| / sum|attr|", (np.abs(delta) / scale).tolist())
    assert (np.abs(delta) <= 1e-13 * scale).all()
    # the restated weights are that rule, and sum to 1 to a few float32 roundings
    w32 = np.array([R.weight(s, steps) for s in range(steps + 1)], dtype=np.float64)
    assert w32.dtype == np.float64 and abs(w32.sum() - 1) <= (steps + 1) * 2.0 ** -24
    assert all(type(R.weight(s, steps)) is np.float32 and type(R.alpha(s, steps)) is np.float32 for s in range(steps + 1))


def test_restated_path_endpoints_are_bitwise_and_the_reduction_splits():
    g = np.random.default_rng(5)
    x = g.standard_normal((2, 3, 5)).astype(np.float32)
    x[0, 0, 0], x[0, 0, 1] = -0.0, np.float32(1e-41)  # a signed zero and a subnormal survive as bits
    x0 = g.standard_normal((2, 3, 5)).astype(np.float32)
    steps = 5
    full = R.path_dense(x, x0, steps, 0, steps).reshape(steps + 1, 2, 3, 5)
    assert full[0].tobytes() == x0.tobytes() and full[steps].tobytes() == x.tobytes()
    mid = x0 + np.float32(np.float32(3) / np.float32(5)) * (x - x0)  # numpy rounds every float32 operation on its own
    assert full[3].tobytes() == mid.astype(np.float32).tobytes()
    assert R.path_dense(x, 0.25, steps, 0, 0).tobytes() == np.full_like(x, 0.25).tobytes()
    assert R.path_dense(x, x0, steps, 2, 3).tobytes() == full[2:4].reshape(4, 3, 5).tobytes()
    grads = g.standard_normal((steps + 1) * 2 * 15).astype(np.float32).reshape((steps + 1) * 2, 3, 5)
    whole = R.reduce(grads, steps, 0, steps)
    split = R.reduce(grads[6:], steps, 3, 5, acc=R.reduce(grads[:6], steps, 0, 2))
    assert whole.tobytes() == split.tobytes()
    attr = R.finish(whole, x, x0)
    want = ((x.astype(np.float64) - x0) * sum(float(R.weight(s, steps)) * grads.reshape(6, 2, 3, 5)[s].astype(np.float64) for s in range(6)))
    assert np.abs(attr - want).max() <= 1e-5 * np.abs(want).max()
    obj = R.grouped(attr, 5, extra=np.ones((2, 3), dtype=np.float32))
    assert obj.shape == (2, 3) and np.abs(obj - (attr.astype(np.float64).sum(-1) + 1)).max() <= 1e-5
    d, mag, n = R.delta([attr], np.ones((2, 4)), np.full((2, 4), 2.0), np.full((2, 4), 0.5))
    assert n == 15 and np.allclose(d, attr.astype(np.float64).reshape(2, -1).sum(1) - 6.0) and (mag >= np.abs(d + 6.0)).all()


def test_restated_layout_path_replicates_the_integer_keys():
    batch = {"categories": np.arange(12).reshape(1, 3, 4), "boxes": np.ones((1, 3, 4, 4), np.float32), "scores": np.full((1, 3, 4), 0.5, np.float32),
             "src_key_padding_mask_boxes": np.zeros((1, 3, 4), np.uint8), "frame_types": np.array([[1, 2, 3]]), "src_key_padding_mask_frames": np.zeros((1, 3), np.uint8),
             "lengths": np.array([3])}
    out = R.path_layout(batch, 2, 0, 2)
    assert out["categories"].shape == (3, 3, 4) and (out["categories"] == batch["categories"]).all() and out["lengths"].tolist() == [3, 3, 3]
    assert (out["boxes"][0] == 0).all() and (out["boxes"][1] == 0.5).all() and (out["boxes"][2] == 1).all() and (out["scores"][1] == 0.25).all()


def test_pool_restatements_agree():
    g = np.random.default_rng(7).standard_normal((2, 3, 3, 5, 6)).astype(np.float32)
    cell = (2, 2, 4)
    bits = R.cell_pool_abs_bits(g, cell)
    assert bits.dtype == np.float32 and bits.shape == (2, 2 * 3 * 2)
    assert np.abs(bits - R.cell_pool(g, cell, absolute=True)).max() <= 1e-5
    assert np.allclose(R.cell_pool(g, cell).sum(axis=1), g.astype(np.float64).reshape(2, -1).sum(axis=1))


def test_the_names_are_declared_bound_wrapped_and_exported(pkg):
    header = open(os.path.join(ROOT, "include", "stlt_hip.h")).read()
    export_map = open(os.path.join(ROOT, "revisiting-spatial-temporal-layouts_amd", "csrc", "exports.map")).read()
    patterns = re.search(r"global:([^;]*);", export_map).group(1).split()
    lib = pkg._lib.load()
    flat = re.sub(r"\s+", " ", header)
    for name in NAMES:
        m = re.search(rf"\b(?:int|size_t) {name}\(([^)]*)\);", flat)
        assert m, f"{name} is not declared in include/stlt_hip.h"
        assert name in pkg._lib.SIGNATURES, f"{name} has no ctypes signature"
        n_args = len([a for a in m.group(1).split(",") if a.strip() and a.strip() != "void"])
        assert len(pkg._lib.SIGNATURES[name][1]) == n_args, f"{name}: the header declares {n_args} arguments, _lib.py binds {len(pkg._lib.SIGNATURES[name][1])}"
        assert any(fnmatch.fnmatchcase(name, pat) for pat in patterns), f"{name} is not a global of csrc/exports.map"
        assert hasattr(lib, name)
    for w in WRAPPERS:
        assert callable(getattr(pkg.ops, w)) and "include/stlt_hip.h" in inspect.getdoc(getattr(pkg.ops, w)), w
    for macro, value in (("STLT_IG_MAX_STEPS", pkg._lib.IG_MAX_STEPS), ("STLT_IG_DELTA_CHUNK", pkg._lib.IG_DELTA_CHUNK), ("STLT_IG_BEGIN", pkg._lib.IG_BEGIN),
                         ("STLT_IG_FINISH", pkg._lib.IG_FINISH)):
        assert re.search(rf"#define {macro}\s+{value}\b", header), macro
    assert pkg._lib.SIGNATURES["stlt_cell_pool_sum"] == pkg._lib.SIGNATURES["stlt_cell_pool_abs"]
    # host arithmetic: one partial per chunk, per tensor, per clip
    ch = pkg._lib.IG_DELTA_CHUNK
    assert lib.stlt_ig_delta_scratch_bytes(3, ch, ch + 1, 0) == 3 * 3 * 4 and lib.stlt_ig_delta_scratch_bytes(1, 3 * 16 * 112 * 112, 0, 0) == 147 * 4
    assert lib.stlt_ig_delta_scratch_bytes(2, 0, 0, 0) == 0 and lib.stlt_ig_delta_scratch_bytes(2, 1 << 31, 0, 0) == 0
    for cls in (pkg.Stlt, pkg.Resnet3D, pkg.models_factory["resnet3d-transformer"], pkg.models_factory["caf"], pkg.models_factory["cacnf"], pkg.models_factory["lcf"]):
        assert callable(getattr(cls, "forward_integrated_gradients")), cls.__name__
    assert "integrated_gradients" in pkg.infer._PERTURB_METHODS


def test_refusals_without_a_gpu(pkg):
    m = pkg.Stlt(pkg.StltModelConfig(**pkg.synth.model_kwargs("micro")))
    m.train(False)
    c = pkg.synth.CONFIGS["micro"]
    batch = pkg.synth.make_batch(2, c["T"], c["N"], seed=1)
    with pytest.raises(pkg.StltHipError, match="CPU"):
        m.forward_integrated_gradients(batch)
    for bad in (0, -1, 2.5, True):
        with pytest.raises(pkg.StltHipError, match="steps"):
            m.forward_integrated_gradients(batch, steps=bad)
    with pytest.raises(pkg.StltHipError, match="steps_per_pass"):
        m.forward_integrated_gradients(batch, steps_per_pass=0)
    lib = pkg._lib.load()
    for call in (lambda: lib.stlt_ig_path_dense(None, None, 0.0, 2, 8, 4, 0, 4, None, None),                      # NULL x
                 lambda: lib.stlt_ig_path_dense(8, None, 0.0, 2, 8, 0, 0, 0, 8, None),                              # steps < 1
                 lambda: lib.stlt_ig_path_dense(8, None, 0.0, 2, 8, 4, 3, 2, 8, None),                              # s0 > s1
                 lambda: lib.stlt_ig_path_dense(8, None, 0.0, 2, 8, 4, 0, 5, 8, None),                              # s1 > steps
                 lambda: lib.stlt_ig_path_dense(8, None, 0.0, 2, 8, 1000, 0, 256, 8, None),                         # 257 steps in one call
                 lambda: lib.stlt_ig_path_dense(8, None, 0.0, 2, 1 << 30, 4, 0, 4, 8, None),                        # 2^31 elements
                 lambda: lib.stlt_ig_reduce(8, 2, 8, 4, 0, 4, 4, 8, None, None, 0.0, None, 1, None, None, None),    # an unknown flag
                 lambda: lib.stlt_ig_reduce(8, 2, 8, 4, 0, 4, 2, 8, None, None, 0.0, None, 1, None, None, None),    # FINISH without x
                 lambda: lib.stlt_ig_reduce(8, 2, 8, 4, 0, 4, 1, 8, None, None, 0.0, None, 4, None, 8, None),       # grouped without FINISH
                 lambda: lib.stlt_ig_delta(8, 4, None, 0, None, 0, 8, 8, 8, 2, 3, 0, 8, 4, 8, None)):               # scratch too small
        assert call() == -1
        assert lib.stlt_last_error().decode().startswith("stlt_ig_")


@pytest.mark.parametrize("name,B", IC.CASES)
def test_the_oracle_in_float32_stays_within_a_quarter_of_the_gpu_bound(name, B):
    """The condition behind the GPU tolerance: on the end-to-end cases, the oracle's float32 integrated gradients differ from its own
    fp64 run by at most a quarter of CAP * max|x - x0| * max_s max|g_s| per attribution, and its delta by a quarter of the delta bound:
    a float32 computation can meet the bound, so the GPU test cannot be failed by the reference alone."""
    target = IC.oracle_top1(name, B)
    ref = IC.oracle_ig(name, B, target)
    f32 = IC.oracle_ig(name, B, target, torch.float32)
    _, _, batch = IC.layout_case(name, B)
    per, dbound = IC.bounds(ref)
    for k in ref["attr"]:
        err = (f32["attr"][k].double() - ref["attr"][k]).abs().max().item()
        _report(f"{name} B={B} {k}: float32 oracle vs fp64, err / bound", f"{err / per[k]:.3g}")
        assert err <= per[k] / 4, (k, err, per[k])
        assert ref["attr"][k].abs().max().item() > 0
    derr = (f32["delta"].double() - ref["delta"]).abs()
    _report(f"{name} B={B} delta: float32 oracle vs fp64, err / bound; |delta| fp64", ((derr / dbound).tolist(), ref["delta"].abs().tolist()))
    assert (derr <= dbound / 4).all()
    pad = batch["src_key_padding_mask_boxes"].bool()
    assert (ref["attr"]["boxes"][pad] == 0).all()
