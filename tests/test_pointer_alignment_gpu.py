"""Base pointers off a 16-byte boundary: every op-level entry point does what include/stlt_hip.h says about it.

torch's allocator hands out 256-byte-aligned blocks, so before this module no test ever gave the library a pointer that is only
4-byte aligned — although a contiguous view such as flat[1:1 + n].view(M, K) is legal torch and reaches the C-ABI through ops.*.
For each entry point, at one ragged and one whole-tile shape, each pointer operand in turn is placed 4, 8 and 12 bytes past its
256-byte boundary inside the guard arena (tests/guard_arena.py), all others aligned.  The header's rule for that operand is one of
    runs     the call succeeds, the arena's bands / gaps / inputs are untouched, every output element is written, and the result
             meets the fp64 reference at the tolerance of the entry point's test in test_kernels_gpu.py / test_any_head_dim_gpu.py
             (bit-equality with the aligned run is not asked for: the products take the four-byte loads of csrc/gemm_any.hip or the
             guarded scalar epilogue of csrc/gemm.hip instead of LDS-DMA and 16-byte stores);
    refused  the call returns STLT_EINVAL, stlt_last_error() names the operand, and nothing was launched (every output still holds
             the arena's fill pattern).
The contract dictionaries below are that rule, operand by operand: None = runs, a string = refused under that name.
"""
import math
from types import SimpleNamespace

import pytest
import torch

import guard_arena as GA
from guard_arena import Out
from oracle import stlt_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda"
_stream, _rand, _pitched = GA.stream, GA.rand, GA.pitched


@pytest.fixture(scope="module")
def arena():
    a = GA.Arena(448 << 20, DEV)  # the grouped weight gradient's 64 MiB scratch with its two bands, plus small operands
    yield a
    del a
    torch.cuda.empty_cache()


@pytest.fixture(scope="module")
def lib(pkg):
    return pkg._lib.load()


def _case(specs, call, outs, verify, contract):
    return SimpleNamespace(specs=specs, call=call, outs=outs, verify=verify, contract=contract)


def _close(got, ref, tol, rel=False):
    err = (got.double() - ref).abs().max().item()
    if rel:
        err /= max(ref.abs().max().item(), 1e-6)
    assert err <= tol, err


# ---- products: routed, never refused (n_split = 1) ---------------------------------------------------------------------------------
def linear_fwd(lib, pkg, kind):
    M, N, K = (257, 129, 96) if kind == "ragged" else (256, 128, 96)
    x, w, b = _rand(M, K, seed=1), _rand(N, K, seed=2, scale=1 / math.sqrt(K)), _rand(N, seed=3, scale=0.1)
    ref = O.gelu(x.double() @ w.double().t() + b.double())
    specs = {"x": (x, "in"), "w": (w, "in"), "b": (b, "in"), "y": (Out((M, N)), "out")}
    call = lambda o: lib.stlt_linear_fwd(o.x.ptr, K, o.w.ptr, o.b.ptr, o.y.ptr, N, M, N, K, 1, _stream())
    return _case(specs, call, ["y"], lambda g: _close(g["y"], ref, 2e-5), {"x": None, "w": None, "b": None, "y": None})


def linear_fwd_large_tiles(lib, pkg, kind):
    """Rows enough that the product stays on the 256 x 128 kernel when everything is aligned: a misaligned y then takes that kernel's
    guarded scalar epilogue, a misaligned x or w the fallback."""
    M, N, K = (1025, 132, 64) if kind == "ragged" else (1024, 128, 64)
    x, w, b = _rand(M, K, seed=1), _rand(N, K, seed=2, scale=1 / math.sqrt(K)), _rand(N, seed=3, scale=0.1)
    ref = x.double() @ w.double().t() + b.double()
    specs = {"x": (x, "in"), "w": (w, "in"), "b": (b, "in"), "y": (Out((M, N)), "out")}

    def call(o):
        lib.stlt_set_gemm_small_tiles(0)  # keep the aligned product off the small-tile kernel for this case
        try:
            return lib.stlt_linear_fwd(o.x.ptr, K, o.w.ptr, o.b.ptr, o.y.ptr, N, M, N, K, 0, _stream())
        finally:
            lib.stlt_set_gemm_small_tiles(-2)

    return _case(specs, call, ["y"], lambda g: _close(g["y"], ref, 2e-5), {"x": None, "w": None, "b": None, "y": None})


def gemm_nn(lib, pkg, kind):
    M, N, K = (300, 200, 96) if kind == "ragged" else (256, 128, 96)
    a, b, r = _rand(M, K, seed=1), _rand(K, N, seed=2, scale=1 / math.sqrt(K)), _rand(M, N, seed=3)
    ref = a.double() @ b.double() + r.double()
    specs = {"a": (a, "in"), "b": (b, "in"), "r": (r, "in"), "c": (Out((M, N)), "out")}
    call = lambda o: lib.stlt_gemm(0, 1, o.a.ptr, K, o.b.ptr, N, o.r.ptr, N, o.c.ptr, N, 0, M, N, K, 1, _stream())
    return _case(specs, call, ["c"], lambda g: _close(g["c"], ref, 3e-5), {"a": None, "b": None, "r": None, "c": None})


def gemm_tn(lib, pkg, kind):
    M, N, K = (200, 132, 96) if kind == "ragged" else (256, 128, 160)  # K = 160: more than the 128 rows the few-row path takes
    a, b = _rand(K, M, seed=4), _rand(K, N, seed=5)
    ref = a.double().t() @ b.double()
    specs = {"a": (a, "in"), "b": (b, "in"), "c": (Out((M, N)), "out")}
    call = lambda o: lib.stlt_gemm(1, 1, o.a.ptr, M, o.b.ptr, N, None, 0, o.c.ptr, N, 0, M, N, K, 1, _stream())
    return _case(specs, call, ["c"], lambda g: _close(g["c"], ref, 2e-5 * math.sqrt(K)), {"a": None, "b": None, "c": None})


def gemm_tn_split(lib, pkg, kind):
    """A split product exists on the LDS-DMA kernel only: a / b off 16 bytes are refused; the slabs may lie anywhere."""
    M, N, K, n_split = (200, 132, 96, 3) if kind == "ragged" else (256, 128, 128, 2)
    a, b = _rand(K, M, seed=4), _rand(K, N, seed=5)
    ref = a.double().t() @ b.double()
    specs = {"a": (a, "in"), "b": (b, "in"), "c": (Out((n_split * M, N)), "out")}
    call = lambda o: lib.stlt_gemm(1, 1, o.a.ptr, M, o.b.ptr, N, None, 0, o.c.ptr, N, M * N, M, N, K, n_split, _stream())
    return _case(specs, call, ["c"], lambda g: _close(g["c"].view(n_split, M, N).double().sum(0), ref, 2e-5 * math.sqrt(K)), {"a": "a", "b": "b", "c": None})


def reduce_slabs(lib, pkg, kind):
    n, n_slabs = (15 if kind == "ragged" else 4096), 3
    stride = (n + 3) // 4 * 4
    slabs, dst0 = _rand(n_slabs, stride, seed=n), _rand(n, seed=7)
    ref = slabs[:, :n].double().sum(0) + dst0.double()
    mag = slabs[:, :n].double().abs().sum(0) + dst0.double().abs()
    specs = {"slabs": (slabs, "in"), "dst": (dst0, "out")}
    call = lambda o: lib.stlt_reduce_slabs(o.slabs.ptr, stride, n_slabs, o.dst.ptr, n, 1, _stream())

    def verify(g):  # k + 1 fp32 terms summed in any order: within k * 2^-24 * sum|terms| of the exact sum
        assert bool(((g["dst"].double() - ref).abs() <= (n_slabs + 1) * 2.0 ** -24 * 1.01 * mag).all())

    return _case(specs, call, ["dst"], verify, {"slabs": None, "dst": None})


def weight_grad_group(lib, pkg, kind):
    rows, n_out, k_in = (32, 300, 36) if kind == "ragged" else (64, 256, 128)
    gen = torch.Generator().manual_seed(1)
    dy, x, g0 = torch.rand(rows, n_out, generator=gen) * 2 - 1, torch.rand(rows, k_in, generator=gen) * 2 - 1, torch.rand(n_out, k_in, generator=gen)
    ref = g0.double() + dy.double().t() @ x.double()
    specs = {"dy": (dy, "in"), "x": (x, "in"), "g": (g0, "out"),
             "scratch": (Out((int(lib.stlt_gemm_scratch_bytes()),), torch.uint8, must_write=False), "out")}

    def call(o):
        arr = (pkg._lib.WgradItem * 1)(pkg._lib.WgradItem(o.dy.ptr, n_out, o.x.ptr, k_in, rows, o.g.ptr))
        assert lib.stlt_gemm_set_scratch(o.scratch.ptr, o.scratch.nbytes) == 0, GA.last_error(lib)
        try:
            return lib.stlt_weight_grad_group(arr, 1, _stream())
        finally:
            lib.stlt_gemm_set_scratch(None, 0)

    return _case(specs, call, ["g"], lambda g: _close(g["g"], ref, 3e-6 * max(1.0, rows ** 0.5) * 8), {"dy": "dy", "x": "x", "g": None})


# ---- the small-tile kernel with the tile given: refused ------------------------------------------------------------------------------
def linear_small(lib, pkg, kind):
    rows, cols = 64, 64
    M, N, K = (rows + 1, cols + 4, 96) if kind == "ragged" else (rows, cols, 64)
    x, w, b, r = _rand(M, K, seed=1, scale=1.5), _rand(N, K, seed=2, scale=2.0 / math.sqrt(K)), _rand(N, seed=3, scale=0.5), _rand(M, N, seed=7)
    ref = x.double() @ w.double().t()
    tol = 3e-6 * math.sqrt(K) * max(1.0, ref.abs().max().item())
    specs = {"x": (x, "in"), "w": (w, "in"), "b": (b, "in"), "r": (r, "in"), "y": (Out((M, N)), "out")}
    call = lambda o: lib.stlt_linear_small_fwd(o.x.ptr, K, o.w.ptr, o.b.ptr, o.r.ptr, N, o.y.ptr, N, M, N, K, 0, pkg.ops.small_tile(cols, rows), _stream())
    return _case(specs, call, ["y"], lambda g: _close(g["y"], ref + b.double() + r.double(), tol), {"x": "x", "w": "w", "b": "bias", "r": "r", "y": "y"})


def input_grad_small(lib, pkg, kind):
    rows, cols = 64, 64
    M, n_out, k_in = (rows + 1, 96, cols + 4) if kind == "ragged" else (rows, 64, cols)
    dy, w, r = _rand(M, n_out, seed=1, scale=1.5), _rand(n_out, k_in, seed=2, scale=2.0 / math.sqrt(n_out)), _rand(M, k_in, seed=9)
    ref = dy.double() @ w.double()
    tol = 3e-6 * math.sqrt(n_out) * max(1.0, ref.abs().max().item())
    specs = {"dy": (dy, "in"), "w": (w, "in"), "r": (r, "in"), "dx": (Out((M, k_in)), "out")}
    call = lambda o: lib.stlt_input_grad_small(o.dy.ptr, n_out, o.w.ptr, n_out, k_in, o.r.ptr, k_in, o.dx.ptr, k_in, M, pkg.ops.small_tile(cols, rows), None, _stream())
    return _case(specs, call, ["dx"], lambda g: _close(g["dx"], ref + r.double(), tol), {"dy": "dy", "w": "w", "r": "r", "dx": "dx"})


# ---- attention ------------------------------------------------------------------------------------------------------------------------
def _attn_ref(qkv, kpm, causal, H):
    S, L, _ = qkv.shape
    masked = kpm[:, None, :].expand(S, L, L).clone()
    if causal:
        masked |= torch.triu(torch.ones(L, L, dtype=torch.bool), diagonal=1)[None]
    return O.attention_core(qkv.double(), torch.zeros(S, L, L, dtype=torch.float64).masked_fill(masked, float("-inf")), H)


def _attn_core(lib, kind, dh, contract):
    S, L, H = (5, 17, 2) if kind == "ragged" else (8, 16, 2)
    d = H * dh
    qkv = _rand(S, L, 3 * d, seed=L, scale=1.5)
    kpm = torch.rand(S, L, generator=torch.Generator().manual_seed(100 + L)) < 0.3
    kpm[:, 0] = False
    ref = _attn_ref(qkv, kpm, True, H).reshape(S * L, d)
    specs = {"qkv": (qkv, "in"), "kpm": (kpm.to(torch.uint8), "extent", 0), "ctx": (Out((S * L, d)), "out")}
    call = lambda o: lib.stlt_attn_core_fwd(o.qkv.ptr, o.kpm.ptr, 1, S, L, H, dh, o.ctx.ptr, _stream())
    return _case(specs, call, ["ctx"], lambda g: _close(g["ctx"], ref, 2e-5), contract)


def attn_core(lib, pkg, kind):
    return _attn_core(lib, kind, 64, {"qkv": "qkv", "ctx": "ctx", "kpm": None})


def attn_core_head_dim_25(lib, pkg, kind):
    """csrc/attn_any.hip tests its pointers itself and falls back to four-byte accesses."""
    return _attn_core(lib, kind, 25, {"qkv": None, "ctx": None, "kpm": None})


def attn_cross(lib, pkg, kind):
    S, H, Lq, Lk = (5, 2, 17, 70) if kind == "ragged" else (4, 2, 32, 32)
    d = 64 * H
    q, kv = _rand(S * Lq, d, seed=Lq, scale=1.5), _rand(S * Lk, 2 * d, seed=100 + Lk, scale=1.5)
    kpm = torch.rand(S, Lk, generator=torch.Generator().manual_seed(3)) < 0.3
    kpm[:, 0] = False
    sp = lambda t, Lx: t.double().reshape(S, Lx, H, 64).transpose(1, 2)
    sc = (sp(q, Lq) @ sp(kv[:, :d], Lk).transpose(-1, -2) / 8.0).masked_fill(kpm[:, None, None, :], float("-inf"))
    ref = (torch.softmax(sc, -1) @ sp(kv[:, d:], Lk)).transpose(1, 2).reshape(S * Lq, d)
    specs = {"q": (q, "in"), "kv": (kv, "in"), "kpm": (kpm.to(torch.uint8), "extent", 0), "ctx": (Out((S * Lq, d)), "out")}
    call = lambda o: lib.stlt_attn_cross_fwd(o.q.ptr, d, o.kv.ptr, o.kv.ptr + 4 * d, 2 * d, o.kpm.ptr, 0, S, Lq, Lk, H, 64, o.ctx.ptr, _stream())
    return _case(specs, call, ["ctx"], lambda g: _close(g["ctx"], ref, 2e-5), {"q": "q", "kv": "k", "ctx": "ctx", "kpm": None})


def attn_ragged(lib, pkg, kind):
    lens, H = ([7, 1, 3] if kind == "ragged" else [32, 32]), 2
    d, M = 64 * H, sum(lens)
    qkv = _rand(M, 3 * d, seed=M, scale=1.5)
    ln = torch.tensor(lens)
    ends = torch.cumsum(ln, 0)
    seg_start, seg_end = torch.repeat_interleave(ends - ln, ln).to(torch.int32), torch.repeat_interleave(ends, ln).to(torch.int32)
    ref, r0 = torch.zeros(M, d, dtype=torch.float64), 0
    for n in lens:
        q, k, v = [qkv[r0:r0 + n, i * d:(i + 1) * d].double().view(n, H, 64).transpose(0, 1) for i in range(3)]
        ref[r0:r0 + n] = (torch.softmax(q @ k.transpose(1, 2) / 8.0, -1) @ v).transpose(0, 1).reshape(n, d)
        r0 += n
    specs = {"qkv": (qkv, "in"), "seg_start": (seg_start, "extent", 0), "seg_end": (seg_end, "extent", M), "ctx": (Out((M, d)), "out")}
    call = lambda o: lib.stlt_attn_ragged_fwd(o.qkv.ptr, o.seg_start.ptr, o.seg_end.ptr, 0, M, H, 64, o.ctx.ptr, _stream())
    return _case(specs, call, ["ctx"], lambda g: _close(g["ctx"], ref, 2e-5), {"qkv": "qkv", "ctx": "ctx", "seg_start": None, "seg_end": None})


def mhsa_fused(lib, pkg, kind):
    S, L, H = (8, 17, 2) if kind == "ragged" else (4, 32, 2)
    d = 64 * H
    x, w, b = _rand(S * L, d, seed=1, scale=1.5), _rand(3 * d, d, seed=2, scale=2.0 / math.sqrt(d)), _rand(3 * d, seed=3, scale=0.5)
    kpm = torch.rand(S, L, generator=torch.Generator().manual_seed(4)) < 0.3
    kpm[:, 0] = False
    qkv_ref = (x.double() @ w.double().t() + b.double()).view(S, L, 3 * d)
    ref = _attn_ref(qkv_ref, kpm, True, H).reshape(S * L, d)
    specs = {"x": (x, "in"), "w": (w, "in"), "b": (b, "in"), "kpm": (kpm.to(torch.uint8), "extent", 0), "ctx": (Out((S * L, d)), "out"),
             "qkv": (Out((S * L, 3 * d)), "out")}
    call = lambda o: lib.stlt_mhsa_fused_fwd_ex(o.x.ptr, o.w.ptr, o.b.ptr, o.kpm.ptr, 1, S, L, H, d, 0.0, 0, 0, o.ctx.ptr, o.qkv.ptr, _stream())

    def verify(g):
        _close(g["ctx"], ref, 5e-5)
        _close(g["qkv"], qkv_ref.view(S * L, 3 * d), 3e-5)

    return _case(specs, call, ["ctx", "qkv"], verify, {"x": "x", "w": "in_proj_w", "b": None, "ctx": "ctx", "qkv": "qkv_out", "kpm": None})


# ---- row-wise and element-wise kernels: 16 bytes per lane on every float pointer ---------------------------------------------------------
def add_layernorm(lib, pkg, kind):
    M, d = (5, 68) if kind == "ragged" else (4, 768)
    x, r, w, b = _rand(M, d, seed=1, scale=3), _rand(M, d, seed=2, scale=3), 1 + _rand(d, seed=3, scale=0.2), _rand(d, seed=4, scale=0.2)
    ref = O.layer_norm((x + r).double(), w.double(), b.double(), 1e-5)
    specs = {"x": (x, "in"), "res": (r, "in"), "w": (w, "in"), "b": (b, "in"), "out": (Out((M, d)), "out")}
    call = lambda o: lib.stlt_add_layernorm_fwd(o.x.ptr, d, o.res.ptr, d, o.w.ptr, o.b.ptr, 1e-5, M, d, o.out.ptr, d, _stream())
    return _case(specs, call, ["out"], lambda g: _close(g["out"], ref, 2e-5), {"x": "x", "res": "res", "w": "ln_w", "b": "ln_b", "out": "out"})


def embed(lib, pkg, kind):
    n, d, C = (5 if kind == "ragged" else 32), 64, 9
    g = torch.Generator().manual_seed(21)
    cats, boxes, scores = torch.randint(0, C, (n,), generator=g), torch.rand(n, 4, generator=g), torch.rand(n, generator=g)
    sd = {"category_embeddings.weight": _rand(C, d, seed=8), "box_embedding.weight": _rand(d, 4, seed=9, scale=0.5),
          "box_embedding.bias": _rand(d, seed=10, scale=0.5), "score_embeddings.weight": _rand(d, 1, seed=11),
          "score_embeddings.bias": _rand(d, seed=12, scale=0.5), "layer_norm.weight": 1 + _rand(d, seed=13, scale=0.1),
          "layer_norm.bias": _rand(d, seed=14, scale=0.1)}
    ref = O.category_box_embeddings({k: v.double() for k, v in sd.items()}, "", {"categories": cats, "boxes": boxes, "scores": scores}, 1e-12)
    table = torch.cat([sd["category_embeddings.weight"], torch.full((1, d), float("nan"))])
    specs = {"cats": (cats, "index", C), "boxes": (boxes, "in"), "scores": (scores, "in"), "table": (table, "in"), "box_w": (sd["box_embedding.weight"], "in"),
             "box_b": (sd["box_embedding.bias"], "in"), "score_w": (sd["score_embeddings.weight"], "in"), "score_b": (sd["score_embeddings.bias"], "in"),
             "ln_w": (sd["layer_norm.weight"], "in"), "ln_b": (sd["layer_norm.bias"], "in"), "out": (Out((n, d)), "out")}
    call = lambda o: lib.stlt_embed_fwd(o.cats.ptr, o.boxes.ptr, o.scores.ptr, o.table.ptr, C + 1, o.box_w.ptr, o.box_b.ptr, o.score_w.ptr, o.score_b.ptr, o.ln_w.ptr,
                                        o.ln_b.ptr, 1e-12, n, d, o.out.ptr, _stream())
    contract = {"cats": None, "boxes": "boxes", "scores": None, "table": "cat_table", "box_w": "box_w", "box_b": "box_b", "score_w": "score_w", "score_b": "score_b",
                "ln_w": "ln_w", "ln_b": "ln_b", "out": "out"}
    return _case(specs, call, ["out"], lambda g: _close(g["out"], ref, 2e-5), contract)


def frames_embed(lib, pkg, kind):
    B, T, d = (3, 5, 68) if kind == "ragged" else (2, 4, 256)
    sp, ft = _rand(B * T, d, seed=1), torch.randint(0, 5, (B, T), generator=torch.Generator().manual_seed(2))
    P, F = _rand(16, d, seed=3), torch.cat([_rand(5, d, seed=4), torch.full((1, d), float("nan"))])
    w, b = 1 + _rand(d, seed=5, scale=0.1), _rand(d, seed=6, scale=0.1)
    ref = O.layer_norm((sp.view(B, T, d) + P[:T][None] + F[ft]).double(), w.double(), b.double(), 1e-12).reshape(B * T, d)
    specs = {"sp": (sp, "in"), "ft": (ft, "index", 5), "P": (P, "in"), "F": (F, "in"), "w": (w, "in"), "b": (b, "in"), "out": (Out((B * T, d)), "out")}
    call = lambda o: lib.stlt_frames_embed_fwd(o.sp.ptr, d, o.ft.ptr, o.P.ptr, o.F.ptr, o.w.ptr, o.b.ptr, 1e-12, B, T, d, o.out.ptr, _stream())
    return _case(specs, call, ["out"], lambda g: _close(g["out"], ref, 2e-5),
                 {"sp": "spatial", "ft": None, "P": "pos_table", "F": "type_table", "w": "ln_w", "b": "ln_b", "out": "out"})


def gather_last(lib, pkg, kind):
    B, T, d = (3, 6, 68) if kind == "ragged" else (4, 4, 256)
    x = _rand(B, T, d, seed=1)
    lengths = torch.tensor([T, 2, 4, 1][:B])
    specs = {"x": (x, "in"), "lengths": (lengths, "extent", 1), "out": (Out((B, d)), "out")}
    call = lambda o: lib.stlt_gather_last_fwd(o.x.ptr, o.lengths.ptr, B, T, d, o.out.ptr, _stream())

    def verify(g):
        assert torch.equal(g["out"], x[torch.arange(B), lengths - 1])

    return _case(specs, call, ["out"], verify, {"x": "x", "out": "out", "lengths": None})


def collate(lib, pkg, kind):
    specs, call, want = GA.collate_case(kind == "ragged")

    def verify(g):
        for n, ref in want.items():
            assert torch.equal(g[n], ref), n

    contract = {"box_r": "boxes_ragged", "box": "boxes", "cat_r": None, "ft_r": None, "offsets": None, "cat": None, "ft": None, "kpm_boxes": None, "kpm_frames": None}
    if kind == "ragged":
        contract.update({"sc_r": None, "sc": None})  # scores move one float at a time
    return _case(specs, call(lib), list(want), verify, contract)


def gelu_fwd(lib, pkg, kind):
    n = 1028 if kind == "ragged" else 1024
    x = _rand(n, seed=1, scale=3)
    specs = {"x": (x, "in"), "y": (Out((n,)), "out")}
    return _case(specs, lambda o: lib.stlt_gelu_fwd(o.x.ptr, o.y.ptr, n, _stream()), ["y"], lambda g: _close(g["y"], O.gelu(x.double()), 2e-5), {"x": "u", "y": "h"})


def gelu_bwd(lib, pkg, kind):
    n = 1028 if kind == "ragged" else 1024
    x, dy = _rand(n, seed=1, scale=3), _rand(n, seed=2)
    x64 = x.double().requires_grad_(True)
    O.gelu(x64).backward(dy.double())
    specs = {"dy": (dy, "in"), "x": (x, "in"), "dx": (Out((n,)), "out")}
    return _case(specs, lambda o: lib.stlt_gelu_bwd(o.dy.ptr, o.x.ptr, o.dx.ptr, n, _stream()), ["dx"], lambda g: _close(g["dx"], x64.grad, 2e-5, rel=True),
                 {"dy": "dh", "x": "u", "dx": "du"})


def dropout(lib, pkg, kind):
    import numpy as np
    n, p, seed, site = (1027 if kind == "ragged" else 1024), 0.3, 12345, 0x200000
    x = _rand(n, seed=4) + 3.0
    keep = torch.from_numpy(O.dropout_keep(p, seed, site, np.arange(n, dtype=np.uint64)))
    specs = {"x": (x, "in"), "y": (Out((n,)), "out")}

    def verify(g):
        assert torch.equal(g["y"] != 0, keep) and (g["y"][keep] - x[keep] / (1 - p)).abs().max().item() <= 1e-6 * 8

    return _case(specs, lambda o: lib.stlt_dropout(o.x.ptr, o.y.ptr, n, p, seed, site, _stream()), ["y"], verify, {"x": "x", "y": "y"})


def relu_bwd(lib, pkg, kind):
    n = 1027 if kind == "ragged" else 1024
    dy, y = _rand(n, seed=2), torch.relu(_rand(n, seed=3))
    specs = {"dy": (dy, "in"), "y": (y, "in"), "dx": (Out((n,)), "out")}

    def verify(g):
        assert torch.equal(g["dx"], torch.where(y > 0, dy, torch.zeros_like(dy)))

    return _case(specs, lambda o: lib.stlt_relu_bwd(o.dy.ptr, o.y.ptr, o.dx.ptr, n, _stream()), ["dx"], verify, {"dy": "dy", "y": "y", "dx": "dx"})


# ---- op-level backward, criterion, optimiser, evaluators ---------------------------------------------------------------------------------
def _scratch_spec(nbytes):
    return (Out((int(nbytes),), torch.uint8, must_write=False), "out")


def _rel_all(got, refs, tol=2e-5):
    for k, r in refs.items():
        _close(got[k], r, tol, rel=True)


def linear_bwd(lib, pkg, kind):
    M, N, K = (40, 64, 32) if kind == "ragged" else (256, 128, 64)
    x, w, b, g = _rand(M, K, seed=1), _rand(N, K, seed=2, scale=1 / math.sqrt(K)), _rand(N, seed=3, scale=0.1), _rand(M, N, seed=4)
    x64, w64, b64 = [t.double().requires_grad_(True) for t in (x, w, b)]
    (x64 @ w64.t() + b64).backward(g.double())
    nbytes = int(lib.stlt_linear_bwd_scratch_bytes(N))
    specs = {"x": (x, "in"), "w": (w, "in"), "dy": (g, "in"), "dx": (Out((M, K)), "out"), "dw": (torch.zeros(N, K), "out"), "db": (torch.zeros(N), "out"),
             "scratch": _scratch_spec(nbytes)}
    call = lambda o: lib.stlt_linear_bwd(o.x.ptr, o.w.ptr, o.dy.ptr, M, N, K, o.dx.ptr, o.dw.ptr, o.db.ptr, None, o.scratch.ptr, nbytes, _stream())
    return _case(specs, call, ["dx", "dw", "db"], lambda got: _rel_all(got, {"dx": x64.grad, "dw": w64.grad, "db": b64.grad}),
                 {"x": None, "w": None, "dx": None, "dw": None, "dy": "dy", "db": "db", "scratch": "scratch"})  # the products route, the column sums do not


def add_layernorm_bwd(lib, pkg, kind):
    M, d = (5, 1028) if kind == "ragged" else (8, 256)
    x, r, w, g = _rand(M, d, seed=1), _rand(M, d, seed=2), 1 + _rand(d, seed=3, scale=0.1), _rand(M, d, seed=5)
    s64, w64, b64 = (x + r).double().requires_grad_(True), w.double().requires_grad_(True), torch.zeros(d, dtype=torch.float64, requires_grad=True)
    torch.nn.functional.layer_norm(s64, (d,), w64, b64, 1e-5).backward(g.double())
    nbytes = int(lib.stlt_add_layernorm_bwd_scratch_bytes(d))
    specs = {"dy": (g, "in"), "x": (x, "in"), "res": (r, "in"), "w": (w, "in"), "ds": (Out((M, d)), "out"), "gw": (torch.zeros(d), "out"), "gb": (torch.zeros(d), "out"),
             "scratch": _scratch_spec(nbytes)}
    call = lambda o: lib.stlt_add_layernorm_bwd(o.dy.ptr, o.x.ptr, o.res.ptr, o.w.ptr, 1e-5, M, d, o.ds.ptr, o.gw.ptr, o.gb.ptr, o.scratch.ptr, nbytes, _stream())
    return _case(specs, call, ["ds", "gw", "gb"], lambda got: _rel_all(got, {"ds": s64.grad, "gw": w64.grad, "gb": b64.grad}),
                 {"dy": "dy", "x": "x", "res": "res", "w": "ln_w", "ds": "ds", "gw": "g_w", "gb": "g_b", "scratch": "scratch"})


def _attn_core_bwd(lib, kind, dh, contract):
    S, L, H = (5, 17, 2) if kind == "ragged" else (4, 32, 2)
    d = dh * H
    qkv, g = _rand(S, L, 3 * d, seed=L, scale=1.5), _rand(S, L, d, seed=L + 1)
    kpm = torch.rand(S, L, generator=torch.Generator().manual_seed(L)) < 0.3
    kpm[:, 0] = False
    x = qkv.double().requires_grad_(True)
    _attn_ref(x, kpm, True, H).backward(g.double())
    ref = x.grad.reshape(S * L, 3 * d)
    nbytes = int(lib.stlt_attn_core_bwd_scratch_bytes(H))
    specs = {"qkv": (qkv, "in"), "dctx": (g, "in"), "kpm": (kpm.to(torch.uint8), "extent", 0), "dqkv": (Out((S * L, 3 * d)), "out"), "gb": (torch.zeros(3 * d), "out"),
             "scratch": _scratch_spec(nbytes)}
    call = lambda o: lib.stlt_attn_core_bwd(o.qkv.ptr, o.dctx.ptr, o.kpm.ptr, 1, S, L, H, dh, 0.0, 0, 0, o.dqkv.ptr, o.gb.ptr, o.scratch.ptr, nbytes, _stream())

    def verify(got):
        _close(got["dqkv"], ref, 2e-5, rel=True)
        _close(got["gb"], ref.sum(0), 5e-5, rel=True)

    return _case(specs, call, ["dqkv", "gb"], verify, contract)


def attn_core_bwd(lib, pkg, kind):
    return _attn_core_bwd(lib, kind, 64, {"qkv": "qkv", "dctx": "dctx", "dqkv": "dqkv", "gb": "in_proj_b_grad", "scratch": "scratch", "kpm": None})


def attn_core_bwd_head_dim_25(lib, pkg, kind):
    """Bars of test_attn_core_bwd_any_head_dim_vs_fp64 (2e-5 / 5e-5 of scale): csrc/attn_any.hip falls back to four-byte accesses."""
    return _attn_core_bwd(lib, kind, 25, {"qkv": None, "dctx": None, "dqkv": None, "kpm": None})


def _attn_bwd(lib, kind, dh, contract):
    S, H, Lq, Lk = (5, 2, 33, 16) if kind == "ragged" else (4, 2, 32, 32)
    d = dh * H
    q, kv, g = _rand(S * Lq, d, seed=Lq, scale=1.5), _rand(S * Lk, 2 * d, seed=Lk + 100, scale=1.5), _rand(S * Lq, d, seed=Lq + Lk)
    kpm = torch.rand(S, Lk, generator=torch.Generator().manual_seed(Lk)) < 0.3
    kpm[:, 0] = False
    qr, kvr = q.double().requires_grad_(True), kv.double().requires_grad_(True)
    sp = lambda t, L_: t.reshape(S, L_, H, dh).transpose(1, 2)
    sc = (sp(qr, Lq) @ sp(kvr[..., :d], Lk).transpose(-1, -2) / math.sqrt(dh)).masked_fill(kpm[:, None, None, :].expand(S, H, Lq, Lk), float("-inf"))
    (torch.softmax(sc, -1) @ sp(kvr[..., d:], Lk)).transpose(1, 2).reshape(S * Lq, d).backward(g.double())
    specs = {"q": (q, "in"), "kv": (kv, "in"), "dctx": (g, "in"), "kpm": (kpm.to(torch.uint8), "extent", 0), "dq": (Out((S * Lq, d)), "out"),
             "dkv": (Out((S * Lk, 2 * d)), "out")}
    call = lambda o: lib.stlt_attn_bwd(o.q.ptr, d, o.kv.ptr, o.kv.ptr + 4 * d, 2 * d, o.dctx.ptr, o.kpm.ptr, 0, S, Lq, Lk, H, dh, 0.0, 0, 0, o.dq.ptr, d, o.dkv.ptr,
                                       o.dkv.ptr + 4 * d, 2 * d, _stream())
    return _case(specs, call, ["dq", "dkv"], lambda got: _rel_all(got, {"dq": qr.grad, "dkv": kvr.grad}), contract)


def attn_bwd(lib, pkg, kind):
    return _attn_bwd(lib, kind, 64, {"q": "q", "kv": "k", "dctx": "dctx", "dq": "dq", "dkv": "dk", "kpm": None})


def attn_bwd_head_dim_25(lib, pkg, kind):
    """Bar of test_attention_autograd_any_head_dim (2e-5 of scale)."""
    return _attn_bwd(lib, kind, 25, {"q": None, "kv": None, "dctx": None, "dq": None, "dkv": None, "kpm": None})


def adamw_step(lib, pkg, kind):
    """One parameter tensor cut into chunks of 16384 (the last one odd-sized), no clipping: the parameter, the flat gradient and either
    moment off a 16-byte boundary send every chunk through the one-float-at-a-time branch.  Against torch.optim.AdamW in fp32 on the host,
    2e-6 (test_fused_adamw_matches_torch_adamw_and_clip)."""
    import numpy as np
    n, CH, wd = (50003 if kind == "ragged" else 32768), 16384, 1e-2
    g0 = torch.Generator().manual_seed(0)
    p0, grad = torch.randn(n, generator=g0), torch.randn(n, generator=g0)
    ref = torch.nn.Parameter(p0.clone())
    ref.grad = grad.clone()
    opt = torch.optim.AdamW([ref], lr=3e-3, weight_decay=wd)
    opt.step()
    n4, n_chunks = (n + 3) // 4 * 4, (n + CH - 1) // CH
    flat = torch.zeros(n4)
    flat[:n] = grad
    specs = {"p": (p0.clone(), "out"), "flat": (flat, "in"), "m": (torch.zeros(n4), "out"), "v": (torch.zeros(n4), "out"),
             "table": (torch.zeros(n_chunks * 24, dtype=torch.uint8), "extent", 0)}

    def call(o):
        arr = np.zeros(n_chunks, dtype=np.dtype([("param", "<u8"), ("off", "<i8"), ("n", "<i4"), ("wd", "<f4")]))
        for i in range(n_chunks):
            arr[i] = (o.p.ptr + 4 * CH * i, CH * i, min(CH, n - CH * i), wd)
        o.table.flat.copy_(torch.from_numpy(arr.view(np.uint8).copy()))
        o.table.saved = o.table.flat.clone()  # the table holds this placement's pointers: written by the host here, not by a kernel
        return lib.stlt_adamw_step(o.table.ptr, n_chunks, o.flat.ptr, o.m.ptr, o.v.ptr, None, 3e-3, 0.9, 0.999, 1e-8, 1, _stream())

    st = opt.state[ref]

    def verify(got):
        _close(got["p"], ref.detach().double(), 2e-6)
        _close(got["m"][:n], st["exp_avg"].double(), 2e-6)
        _close(got["v"][:n], st["exp_avg_sq"].double(), 2e-6)

    return _case(specs, call, ["p", "m", "v"], verify, {"p": None, "flat": None, "m": None, "v": None})


def embed_bwd(lib, pkg, kind):
    n, d, C = (90 if kind == "ragged" else 64), 64, 9
    g0 = torch.Generator().manual_seed(7)
    cats, boxes, scores, d_pre = torch.randint(0, C, (n,), generator=g0), torch.rand(n, 4, generator=g0), torch.rand(n, generator=g0), _rand(n, d, seed=5)
    g64 = d_pre.double()
    refs = {"g_cat": torch.zeros(C + 1, d, dtype=torch.float64).index_add_(0, cats, g64), "g_box_w": g64.t() @ boxes.double(), "g_box_b": g64.sum(0),
            "g_sw": (g64 * scores.double()[:, None]).sum(0)[:, None], "g_sb": g64.sum(0)}
    refs["g_cat"][0] = 0.0
    nbytes = int(lib.stlt_embed_bwd_scratch_bytes(n, C + 1, d))
    specs = {"d_pre": (d_pre, "in"), "cats": (cats, "index", C), "boxes": (boxes, "in"), "scores": (scores, "in"), "g_cat": (torch.zeros(C + 1, d), "out"),
             "g_box_w": (torch.zeros(d, 4), "out"), "g_box_b": (torch.zeros(d), "out"), "g_sw": (torch.zeros(d, 1), "out"), "g_sb": (torch.zeros(d), "out"),
             "scratch": _scratch_spec(nbytes)}
    call = lambda o: lib.stlt_embed_bwd(o.d_pre.ptr, o.cats.ptr, o.boxes.ptr, o.scores.ptr, C + 1, n, d, o.g_cat.ptr, o.g_box_w.ptr, o.g_box_b.ptr, o.g_sw.ptr, o.g_sb.ptr,
                                        o.scratch.ptr, nbytes, _stream())
    return _case(specs, call, list(refs), lambda got: _rel_all(got, refs),
                 {"cats": None, "scores": None, "d_pre": "d_pre", "boxes": "boxes", "g_cat": "g_cat", "g_box_w": "g_box_w", "g_box_b": "g_box_b", "g_sw": "g_score_w", "g_sb": "g_score_b",
                  "scratch": "scratch"})


def frames_embed_bwd(lib, pkg, kind):
    B, T, d, n_types = (3, 5, 68, 5) if kind == "ragged" else (2, 4, 256, 5)
    ft, d_pre = torch.randint(0, n_types, (B, T), generator=torch.Generator().manual_seed(2)), _rand(B, T, d, seed=3)
    g64 = d_pre.double()
    ref_type = torch.zeros(n_types + 1, d, dtype=torch.float64).index_add_(0, ft.reshape(-1), g64.reshape(-1, d))
    ref_type[0] = 0.0
    nbytes = int(lib.stlt_frames_embed_bwd_scratch_bytes(T, d))
    specs = {"d_pre": (d_pre, "in"), "ft": (ft, "index", n_types), "g_pos": (torch.zeros(T, d), "out"), "g_type": (torch.zeros(n_types + 1, d), "out"),
             "scratch": _scratch_spec(nbytes)}
    call = lambda o: lib.stlt_frames_embed_bwd(o.d_pre.ptr, o.ft.ptr, B, T, d, o.g_pos.ptr, o.g_type.ptr, o.scratch.ptr, nbytes, _stream())
    return _case(specs, call, ["g_pos", "g_type"], lambda got: _rel_all(got, {"g_pos": g64.sum(0), "g_type": ref_type}),
                 {"ft": None, "d_pre": "d_pre", "g_pos": "g_pos", "g_type": "g_type", "scratch": "scratch"})


def loss_fwd_bwd(lib, pkg, kind):
    """Cross entropy ("ragged": B = 37, K = 157) and BCE with logits ("whole": B = 32, K = 128): scalar accesses, nothing to align."""
    B, K, which = (37, 157, 0) if kind == "ragged" else (32, 128, 1)
    g0 = torch.Generator().manual_seed(3)
    logits = torch.randn(B, K, generator=g0) * 3
    l64 = logits.double().requires_grad_(True)
    if which == 0:
        labels = torch.randint(0, K, (B,), generator=g0)
        ref, lab_spec = torch.nn.functional.cross_entropy(l64, labels), (labels, "index", 0)
    else:
        labels = (torch.rand(B, K, generator=g0) < 0.1).float()
        ref, lab_spec = torch.nn.functional.binary_cross_entropy_with_logits(l64, labels.double()), (labels, "in")
    ref.backward()
    specs = {"logits": (logits, "in"), "labels": lab_spec, "scratch": (Out((B,), must_write=False), "out"), "loss": (Out((1,)), "out"), "dl": (Out((B, K)), "out")}
    call = lambda o: lib.stlt_loss_fwd_bwd(o.logits.ptr, o.labels.ptr, which, B, K, 1.0, o.scratch.ptr, o.loss.ptr, o.dl.ptr, _stream())

    def verify(got):
        assert abs(got["loss"].item() - ref.item()) <= 2e-6 * max(1.0, abs(ref.item()))
        _close(got["dl"], l64.grad, 1e-7)

    contract = {"logits": None, "scratch": None, "loss": None, "dl": None}
    contract["labels"] = None  # int64 classes: 8 bytes; float multi-hot: 4
    return _case(specs, call, ["loss", "dl"], verify, contract)


def grad_norm(lib, pkg, kind):
    n = 50003 if kind == "ragged" else 4096
    flat = torch.zeros((n + 3) // 4 * 4)
    flat[:n] = _rand(n, seed=1, scale=2.0)
    ref = flat.double().norm().item()
    specs = {"flat": (flat, "in"), "scratch": (Out((1024,), must_write=False), "out"), "norm": (Out((2,)), "out")}
    call = lambda o: lib.stlt_grad_norm(o.flat.ptr, flat.numel(), 5.0, o.scratch.ptr, o.norm.ptr, _stream())

    def verify(got):  # test_fused_adamw_matches_torch_adamw_and_clip: the norm to 1e-5 relative; the factor is min(1, max_norm / (norm + 1e-6))
        assert abs(got["norm"][0].item() - ref) <= 1e-5 * ref and abs(got["norm"][1].item() - min(1.0, 5.0 / (ref + 1e-6))) <= 1e-5

    return _case(specs, call, ["norm"], verify, {"flat": "flat_grad", "scratch": None, "norm": None})


def eval_topk(lib, pkg, kind):
    B, K = (37, 157) if kind == "ragged" else (32, 128)
    g0 = torch.Generator().manual_seed(3)
    logits, labels = torch.randn(B, K, generator=g0), torch.randint(0, K, (B,), generator=g0)
    own = logits[torch.arange(B), labels][:, None]
    rank = ((logits > own) | ((logits == own) & (torch.arange(K)[None] < labels[:, None]))).sum(1)
    want = torch.tensor([int((rank == 0).sum()), int((rank < 5).sum())])
    specs = {"logits": (logits, "in"), "labels": (labels, "index", 0), "counts": (torch.zeros(2, dtype=torch.int64), "out")}
    call = lambda o: lib.stlt_eval_topk(o.logits.ptr, K, o.labels.ptr, B, K, o.counts.ptr, _stream())

    def verify(got):
        assert torch.equal(got["counts"], want)

    return _case(specs, call, ["counts"], verify, {"logits": None, "labels": None, "counts": None})


def eval_store_sigmoid(lib, pkg, kind):
    B, C = (5, 157) if kind == "ragged" else (8, 128)
    g0 = torch.Generator().manual_seed(4)
    logits, labels = torch.randn(B, C, generator=g0) * 3, (torch.rand(B, C, generator=g0) < 0.1).float()
    specs = {"logits": (logits, "in"), "labels": (labels, "in"), "pred": (Out((B, C), torch.float64), "out"), "truth": (Out((B, C), torch.float64), "out")}
    call = lambda o: lib.stlt_eval_store_sigmoid(o.logits.ptr, C, o.labels.ptr, B, C, o.pred.ptr, o.truth.ptr, 0, _stream())

    def verify(got):
        assert (got["pred"] - logits.sigmoid().double()).abs().max().item() <= 1.2e-7 and torch.equal(got["truth"], labels.double())

    return _case(specs, call, ["pred", "truth"], verify, {"logits": None, "labels": None, "pred": None, "truth": None})


def eval_average_precision(lib, pkg, kind):
    n, C = (1025 if kind == "ragged" else 64), 3
    g0 = torch.Generator().manual_seed(n)
    scores, truths = torch.rand(n, C, generator=g0), (torch.rand(n, C, generator=g0) < 0.3).float()
    ref = pkg.utils.evaluation.charades_map(scores.double(), truths.double())[2]
    specs = {"scores": (scores, "in"), "truths": (truths, "in"), "ap": (Out((C,), torch.float64), "out"), "pos": (Out((C,), torch.float64), "out"),
             "scratch": (Out((n,), torch.uint8, must_write=False), "out")}
    call = lambda o: lib.stlt_eval_average_precision(o.scores.ptr, o.truths.ptr, n, C, o.ap.ptr, o.pos.ptr, o.scratch.ptr, _stream())

    def verify(got):
        _close(got["ap"], ref, 1e-12)
        assert torch.equal(got["pos"], truths.double().sum(0))

    return _case(specs, call, ["ap", "pos"], verify, {"scores": None, "truths": None, "ap": None, "pos": None, "scratch": None})


ENTRIES = [linear_bwd, add_layernorm_bwd, attn_core_bwd, attn_core_bwd_head_dim_25, attn_bwd, attn_bwd_head_dim_25, adamw_step, embed_bwd, frames_embed_bwd, loss_fwd_bwd, grad_norm, eval_topk, eval_store_sigmoid,
           eval_average_precision,
           linear_fwd, linear_fwd_large_tiles, gemm_nn, gemm_tn, gemm_tn_split, reduce_slabs, weight_grad_group, linear_small, input_grad_small, attn_core,
           attn_core_head_dim_25, attn_cross, attn_ragged, mhsa_fused, add_layernorm, embed, frames_embed, gather_last, collate, gelu_fwd, gelu_bwd, dropout, relu_bwd]


@pytest.mark.parametrize("kind", ["ragged", "whole"])
@pytest.mark.parametrize("entry", ENTRIES, ids=lambda f: f.__name__)
def test_each_pointer_off_a_16_byte_boundary(pkg, lib, arena, entry, kind):
    case = entry(lib, pkg, kind)
    case.verify(GA.misaligned(lib, arena, case.specs, case.call, case.outs))  # all aligned: the case itself is sound
    for operand, refused_as in case.contract.items():
        for mis in (4, 8, 12):
            if mis % case.specs[operand][0].dtype.itemsize:
                continue  # an int64 operand 4 bytes off would break its natural alignment: not a legal pointer of its type
            got = GA.misaligned(lib, arena, case.specs, case.call, case.outs, operand, mis, refused_as)
            if got is not None:
                case.verify(got)


def test_the_products_run_on_a_view_that_starts_one_float_into_a_buffer(pkg):
    """What reaches the C-ABI through ops.* today: contiguous views of a flat buffer that start 4 bytes past its 256-byte-aligned
    base (x, w, bias and the output at once, and the add-source of the backward layout)."""
    M, N, K = 257, 129, 96
    x, w, b, r = _rand(M, K, seed=1), _rand(N, K, seed=2, scale=1 / math.sqrt(K)), _rand(N, seed=3, scale=0.1), _rand(M, K, seed=4)

    def off_by_one_float(t):
        flat = torch.empty(t.numel() + 1, device=DEV)
        v = flat[1:].view(t.shape)
        v.copy_(t)
        assert v.data_ptr() % 16 == 4 and v.is_contiguous()
        return v

    xd, wd, bd, rd = (off_by_one_float(t) for t in (x, w, b, r))
    ref = x.double() @ w.double().t() + b.double()
    y = pkg.ops.linear(xd, wd, bd, out=off_by_one_float(torch.zeros(M, N)))
    assert (y.cpu().double() - ref).abs().max().item() <= 2e-5
    dy = off_by_one_float(_rand(M, N, seed=5))
    dx = pkg.ops.gemm(dy, wd, trans_b=True, add=rd)  # dX = dY·W + r
    assert (dx.cpu().double() - (dy.cpu().double() @ w.double() + r.double())).abs().max().item() <= 3e-5
    dw = pkg.ops.gemm(dy, xd, trans_a=True, trans_b=True)  # dW = dYᵀ·X
    assert (dw.cpu().double() - dy.cpu().double().t() @ x.double()).abs().max().item() <= 2e-5 * math.sqrt(M)


def test_a_lent_scratch_off_a_16_byte_boundary_is_refused(lib, arena):
    """stlt_gemm_set_scratch: partial tiles are 16-byte stores, so the buffer is refused (and stays untouched) at +4 / +8 / +12 bytes."""
    nbytes = int(lib.stlt_gemm_scratch_bytes())
    for mis in (4, 8, 12):
        arena.reset()
        sc = arena.place(Out((nbytes,), torch.uint8, must_write=False), "out", misalign=mis, name="scratch")
        try:
            assert lib.stlt_gemm_set_scratch(sc.ptr, nbytes) == GA.STLT_EINVAL and "scratch" in GA.last_error(lib) and "aligned" in GA.last_error(lib)
        finally:
            assert lib.stlt_gemm_set_scratch(None, 0) == 0
        arena.check(launched=False)
