"""Guard bands around every operand of the C-ABI kernels (tests/guard_arena.py).

Each case runs its call three ways: plainly on separate torch tensors (what every other GPU test does), inside the arena, and inside
the arena again without touching the inputs.  Asserted: the arena's bands, gap columns and inputs are untouched and every output
element was written (Arena.check); the arena result is bit-identical to the plain one (same kernel, same address path: base
pointers are 256-byte aligned in both); the second arena run repeats the first; the result meets the fp64 reference of the entry
point's existing test (tests/test_kernels_gpu.py, test_any_head_dim_gpu.py) at that test's tolerance.

The whole-path cases lend the library exactly the bytes its own size functions return, carved from the arena, instead of the
grow-only / reused buffers of modelling.models, and compare with an unpatched run of the same model bit for bit.
"""
import math
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import guard_arena as GA
from guard_arena import Out
from oracle import stlt_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda"
NAN = float("nan")


@pytest.fixture(scope="module")
def arena():
    # the largest case: the training step's tape and scratch (the scratch holds the 64 MiB stream-K scratch), each with two bands of its own size
    a = GA.Arena(4096 << 20, DEV)
    yield a
    del a
    torch.cuda.empty_cache()


@pytest.fixture(scope="module")
def lib(pkg):
    return pkg._lib.load()


_stream, _rand, _pitched, _err, three_ways = GA.stream, GA.rand, GA.pitched, GA.last_error, GA.three_ways


def _act(ref, act):
    return {0: lambda t: t, 1: O.gelu, 2: torch.relu}[act](ref)


# ---- stlt_linear_fwd -----------------------------------------------------------------------------------------------------------
def _linear_case(lib, arena, x, w, b, ldx, ldy, act, scratch=False, misalign=None):
    M, K = x.shape
    N = w.shape[0]
    specs = {"x": (_pitched(x, ldx), "in"), "w": (w, "in"), "y": (Out((M, N), ld=ldy), "out")}
    if b is not None:
        specs["b"] = (b, "in")
    if scratch:
        specs["scratch"] = (Out((int(lib.stlt_gemm_scratch_bytes()),), torch.uint8, must_write=False), "out")

    def call(o):
        if scratch:
            assert lib.stlt_gemm_set_scratch(o.scratch.ptr, o.scratch.nbytes) == 0, _err(lib)
        try:
            return lib.stlt_linear_fwd(o.x.ptr, ldx, o.w.ptr, o.b.ptr if b is not None else None, o.y.ptr, ldy, M, N, K, act, _stream())
        finally:
            if scratch:
                lib.stlt_gemm_set_scratch(None, 0)

    return three_ways(lib, arena, specs, call, ["y"], misalign)["y"]


@pytest.mark.parametrize("K", [32, 96])
@pytest.mark.parametrize("N", [4, 127, 129, 174])
@pytest.mark.parametrize("M", [1, 255, 257])
def test_linear_fwd_ragged_tiles_pitches_and_epilogues(lib, arena, M, N, K):
    """256 x 128 tiles, BK = 32: one row, one row short of / past a tile; N below, at and past a tile and the head's 174; pitches that
    take the 16-byte and the guarded scalar epilogue; every activation, with and without bias.  Reference and tolerance: test_linear."""
    x, w, b = _rand(M, K, seed=1), _rand(N, K, seed=2, scale=1 / math.sqrt(K)), _rand(N, seed=3, scale=0.1)
    ref = x.double() @ w.double().t()
    for ldx in (K, K + 4):
        for ldy in (N, N + 3, N + 4):
            for act in (0, 1, 2):
                for bias in (b, None):
                    y = _linear_case(lib, arena, x, w, bias, ldx, ldy, act)
                    want = _act(ref + (b.double() if bias is not None else 0.0), act)
                    err = (y.double() - want).abs().max().item()
                    assert err <= 2e-5, (ldx, ldy, act, bias is not None, err)


@pytest.mark.parametrize("M,N,K", [(300, 130, 96), (1, 64, 32), (14000, 776, 768), (65, 174, 768)])
def test_linear_fwd_with_scratch_lent_stays_inside_the_scratch(lib, arena, M, N, K):
    """Stream-K partial tiles ("a whole BMxBN image, no guards"), the hybrid launch (whole rounds + a stream-K tail) and the skinny
    split-k partials, with the scratch an arena operand of exactly stlt_gemm_scratch_bytes().  Reference / tolerance: test_linear_stream_k."""
    x, w, b = _rand(M, K, seed=1), _rand(N, K, seed=2, scale=1 / math.sqrt(K)), _rand(N, seed=3, scale=0.1)
    ref = x.double() @ w.double().t() + b.double()
    for act in ((0, 1, 2) if M < 10000 else (1,)):
        y = _linear_case(lib, arena, x, w, b, K, N, act, scratch=True)
        assert (y.double() - _act(ref, act)).abs().max().item() <= 2e-5, act
    if M < 10000:
        y = _linear_case(lib, arena, x, w, b, K, N + 3, 0, scratch=True)
        assert (y.double() - ref).abs().max().item() <= 2e-5


@pytest.mark.parametrize("N", [8, 65])
@pytest.mark.parametrize("M", [4, 63, 65])
def test_linear_fwd_contraction_length_20_on_the_64x64_fallback(lib, arena, M, N):
    """K = 20 is no multiple of 32: csrc/gemm_any.hip, zero-filled 64 x 64 tiles.  Reference / tolerance:
    test_linear_with_a_contraction_length_that_is_not_a_multiple_of_32."""
    K = 20
    x, w, b = _rand(M, K, seed=1), _rand(N, K, seed=2), _rand(N, seed=3, scale=0.1)
    ref = x.double() @ w.double().t()
    for ldx in (K, K + 4, K + 1):
        for ldy in (N, N + 3):
            for act, bias in ((0, None), (0, b), (1, b), (2, b)):
                y = _linear_case(lib, arena, x, w, bias, ldx, ldy, act)
                want = _act(ref + (b.double() if bias is not None else 0.0), act)
                assert (y.double() - want).abs().max().item() <= 2e-5, (ldx, ldy, act)


# ---- stlt_gemm, stlt_reduce_slabs, stlt_weight_grad_group ---------------------------------------------------------------------------
def test_gemm_nn_with_add_source_at_odd_pitches(lib, arena):
    """dX = dY·W + r: (300, 200, 96), ldr = N + 4, ldc = N + 1 (scalar stores).  Reference / tolerance: test_gemm_nn_dx_layout."""
    M, N, K = 300, 200, 96
    a, b, r = _rand(M, K, seed=1), _rand(K, N, seed=2, scale=1 / math.sqrt(K)), _rand(M, N, seed=3)
    specs = {"a": (a, "in"), "b": (b, "in"), "r": (_pitched(r, N + 4), "in"), "c": (Out((M, N), ld=N + 1), "out")}
    got = three_ways(lib, arena, specs, lambda o: lib.stlt_gemm(0, 1, o.a.ptr, K, o.b.ptr, N, o.r.ptr, N + 4, o.c.ptr, N + 1, 0, M, N, K, 1, _stream()), ["c"])["c"]
    assert (got.double() - (a.double() @ b.double() + r.double())).abs().max().item() <= 3e-5


@pytest.mark.parametrize("n_split", [1, 3])
def test_gemm_tn_split_slabs_and_their_reduction(lib, arena, n_split):
    """dW = dYᵀ·X: (200, 132, 96); split s writes its slab at c + s * slab_stride, the guard band follows the last slab; the slabs are
    then summed by stlt_reduce_slabs.  Reference / tolerance: test_gemm_tn_dw_layout_with_split_k."""
    M, N, K = 200, 132, 96
    a, b = _rand(K, M, seed=4), _rand(K, N, seed=5)
    ref = a.double().t() @ b.double()
    specs = {"a": (a, "in"), "b": (b, "in"), "c": (Out((n_split * M, N)), "out")}
    slabs = three_ways(lib, arena, specs, lambda o: lib.stlt_gemm(1, 1, o.a.ptr, M, o.b.ptr, N, None, 0, o.c.ptr, N, M * N, M, N, K, n_split, _stream()), ["c"])["c"]
    tol = 2e-5 * math.sqrt(K)
    assert (slabs.view(n_split, M, N).double().sum(0) - ref).abs().max().item() <= tol
    specs = {"slabs": (slabs.contiguous(), "in"), "dst": (Out((M, N)), "out")}
    got = three_ways(lib, arena, specs, lambda o: lib.stlt_reduce_slabs(o.slabs.ptr, M * N, n_split, o.dst.ptr, M * N, 0, _stream()), ["dst"])["dst"]
    assert (got.double() - ref).abs().max().item() <= tol


@pytest.mark.parametrize("n_slabs", [3, 40])
@pytest.mark.parametrize("n", [15, 16, 16400])
@pytest.mark.parametrize("accumulate", [0, 1])
def test_reduce_slabs(lib, arena, accumulate, n, n_slabs):
    """The 16-byte kernel's scalar tail (n = 15), its whole-vector case (16) and the grid-stride form (16400); more than 32 slabs of at
    most 16384 columns take the tall kernel.  The slab stride is n rounded up to 4 floats.  Bound: a sum of k + 1 fp32 terms in any
    order is within k * 2^-24 * sum|terms| * (1 + small) of the exact sum."""
    stride = (n + 3) // 4 * 4
    slabs = _rand(n_slabs, stride, seed=n + n_slabs)
    slabs[:, n:] = NAN  # the pitch gap: never read
    dst0 = _rand(n, seed=7)
    ref = slabs[:, :n].double().sum(0) + (dst0.double() if accumulate else 0.0)
    mag = slabs[:, :n].double().abs().sum(0) + dst0.double().abs()
    specs = {"slabs": (slabs, "in"), "dst": ((dst0 if accumulate else Out((n,))), "out")}
    got = three_ways(lib, arena, specs, lambda o: lib.stlt_reduce_slabs(o.slabs.ptr, stride, n_slabs, o.dst.ptr, n, accumulate, _stream()), ["dst"])["dst"]
    assert bool(((got.double() - ref).abs() <= (n_slabs + 1) * 2.0 ** -24 * 1.01 * mag).all())


def test_weight_grad_group_ragged_tiles(pkg, lib, arena):
    """The "ragged tiles" item list of test_weight_grad_group_matches_per_product_sums, every dy / x / g_w an arena operand (rows are
    multiples of 32 as the header demands, so no padding belongs to the operands), the scratch exactly stlt_gemm_scratch_bytes()."""
    shapes = [(416, 132, 260), (32, 300, 36), (1024, 4, 4), (96, 256, 128), (4096, 260, 516)]
    gen = torch.Generator().manual_seed(len(shapes))
    specs, refs = {}, []
    for i, (rows, n_out, k_in) in enumerate(shapes):
        dy = torch.rand(rows, n_out, generator=gen) * 2 - 1
        x = torch.rand(rows, k_in, generator=gen) * 2 - 1
        g0 = torch.rand(n_out, k_in, generator=gen)
        refs.append(g0.double() + dy.double().t() @ x.double())
        specs[f"dy{i}"], specs[f"x{i}"], specs[f"g{i}"] = (dy, "in"), (x, "in"), (g0, "out")
    specs["scratch"] = (Out((int(lib.stlt_gemm_scratch_bytes()),), torch.uint8, must_write=False), "out")

    def call(o):
        arr = (pkg._lib.WgradItem * len(shapes))()
        for i, (rows, n_out, k_in) in enumerate(shapes):
            arr[i] = pkg._lib.WgradItem(getattr(o, f"dy{i}").ptr, n_out, getattr(o, f"x{i}").ptr, k_in, rows, getattr(o, f"g{i}").ptr)
        assert lib.stlt_gemm_set_scratch(o.scratch.ptr, o.scratch.nbytes) == 0, _err(lib)
        try:
            return lib.stlt_weight_grad_group(arr, len(shapes), _stream())
        finally:
            lib.stlt_gemm_set_scratch(None, 0)

    got = three_ways(lib, arena, specs, call, [f"g{i}" for i in range(len(shapes))])
    for i, (rows, n_out, k_in) in enumerate(shapes):
        assert (got[f"g{i}"].double() - refs[i]).abs().max().item() <= 3e-6 * max(1.0, rows ** 0.5) * 8, shapes[i]


# ---- the small-tile kernel -------------------------------------------------------------------------------------------------------
def _small_tiles(pkg):
    return list(pkg.ops.SMALL_TILES)


@pytest.mark.parametrize("tile_index", range(15))
def test_linear_small_and_input_grad_small_around_a_tile(pkg, lib, arena, tile_index):
    """Every tile of ops.SMALL_TILES: one row short of / past a tile row boundary, one multiple of 4 past a tile column boundary,
    two and three k-slabs; bias / GELU / ReLU / residual at ldr = N + 4.  References / tolerances: test_linear_small_tiles_vs_fp64,
    test_input_grad_small_tiles_vs_fp64."""
    tiles = _small_tiles(pkg)
    assert len(tiles) == 15
    rows, cols = tiles[tile_index]
    tile = pkg.ops.small_tile(cols, rows)
    N = cols + 4
    for M in (rows - 1, rows + 1):
        for K in (64, 96):
            x, w = _rand(M, K, seed=M + K, scale=1.5), _rand(N, K, seed=N + 1, scale=2.0 / math.sqrt(K))
            b, r = _rand(N, seed=N + 2, scale=0.5), _rand(M, N, seed=7)
            ref = x.double() @ w.double().t()
            tol = 3e-6 * math.sqrt(K) * max(1.0, ref.abs().max().item())
            for act, bias, res in ((0, b, None), (1, b, None), (2, b, None), (0, None, None), (0, b, r)):
                specs = {"x": (x, "in"), "w": (w, "in"), "y": (Out((M, N)), "out")}
                if bias is not None:
                    specs["b"] = (b, "in")
                if res is not None:
                    specs["r"] = (_pitched(r, N + 4), "in")
                got = three_ways(lib, arena, specs, lambda o: lib.stlt_linear_small_fwd(
                    o.x.ptr, K, o.w.ptr, o.b.ptr if bias is not None else None, o.r.ptr if res is not None else None, N + 4, o.y.ptr, N, M, N, K, act, tile,
                    _stream()), ["y"])["y"]
                want = ref + (b.double() if bias is not None else 0.0)
                want = torch.nn.functional.gelu(want) if act == 1 else (torch.relu(want) if act == 2 else want)
                if res is not None:
                    want = want + r.double()
                assert (got.double() - want).abs().max().item() <= tol, (M, K, act, bias is not None, res is not None)
            # the input gradient on the same tile: dx (M, k_in) = dy (M, n_out = K) · w (n_out, k_in = N) (+ r)
            n_out, k_in = K, N
            dy, wg, rg = _rand(M, n_out, seed=M + n_out, scale=1.5), _rand(n_out, k_in, seed=k_in + 1, scale=2.0 / math.sqrt(n_out)), _rand(M, k_in, seed=9)
            ref = dy.double() @ wg.double()
            tol = 3e-6 * math.sqrt(n_out) * max(1.0, ref.abs().max().item())
            for res in (None, rg):
                specs = {"dy": (dy, "in"), "w": (wg, "in"), "dx": (Out((M, k_in)), "out")}
                if res is not None:
                    specs["r"] = (_pitched(rg, k_in + 4), "in")
                got = three_ways(lib, arena, specs, lambda o: lib.stlt_input_grad_small(
                    o.dy.ptr, n_out, o.w.ptr, n_out, k_in, o.r.ptr if res is not None else None, k_in + 4, o.dx.ptr, k_in, M, tile, None, _stream()), ["dx"])["dx"]
                assert (got.double() - (ref + (rg.double() if res is not None else 0.0))).abs().max().item() <= tol, (M, K, res is not None)


# ---- attention --------------------------------------------------------------------------------------------------------------------
def _attn_ref(qkv, kpm, causal, H):
    S, L, _ = qkv.shape
    masked = kpm[:, None, :].expand(S, L, L).clone()
    if causal:
        masked |= torch.triu(torch.ones(L, L, dtype=torch.bool), diagonal=1)[None]
    m = torch.zeros(S, L, L, dtype=torch.float64).masked_fill(masked, float("-inf"))
    return O.attention_core(qkv.double(), m, H)


def _kpm(S, L, seed):
    """Random padding with key 0 kept; from two sequences on, sequence 1 is padded as a whole (its rows come out as zeros, which the
    kernel has to WRITE: the output starts as FILL here)."""
    kpm = torch.rand(S, L, generator=torch.Generator().manual_seed(seed)) < 0.3
    kpm[:, 0] = False
    if S > 1:
        kpm[1, :] = True
    return kpm


def _attn_core_case(lib, arena, S, L, H, dh, causal):
    d = H * dh
    qkv = _rand(S, L, 3 * d, seed=L, scale=1.5)
    kpm = _kpm(S, L, 100 + L)
    specs = {"qkv": (qkv, "in"), "kpm": (kpm.to(torch.uint8), "extent", 0), "ctx": (Out((S * L, d)), "out")}
    got = three_ways(lib, arena, specs, lambda o: lib.stlt_attn_core_fwd(o.qkv.ptr, o.kpm.ptr, int(causal), S, L, H, dh, o.ctx.ptr, _stream()), ["ctx"])["ctx"]
    got = got.view(S, L, d)
    ref = _attn_ref(qkv, kpm, causal, H)
    if S > 1:
        assert got[1].abs().max().item() == 0.0
        ref[1] = 0.0
    assert (got.double() - ref).abs().max().item() <= 2e-5


@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("S", [1, 5])
@pytest.mark.parametrize("L", [1, 15, 17, 33, 65])
def test_attn_core_fwd(lib, arena, L, S, causal):
    """16-row tiles (L <= 64) and 32-row tiles (65), one sequence and a ragged last item, padded keys and a fully padded sequence.
    Reference / tolerance: test_attn_core, test_attn_core_short_sequences_many_items_and_masked_rows."""
    _attn_core_case(lib, arena, S, L, 2, 64, causal)


@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("L", [1, 17])
def test_attn_core_fwd_head_dim_25(lib, arena, L, causal):
    """csrc/attn_any.hip (rows of 50 floats: no 16-byte row alignment).  Reference / tolerance: test_attn_core_any_head_dim."""
    _attn_core_case(lib, arena, 5, L, 2, 25, causal)


@pytest.mark.parametrize("Lq,Lk", [(1, 5), (33, 16), (17, 70)])
def test_attn_cross_fwd_with_pitches_larger_than_the_rows(lib, arena, Lq, Lk):
    """q at ldq = d + 4, k / v inside one buffer at ldkv = 2d + 4 (gap columns NaN).  Reference / tolerance: test_attn_cross."""
    S, H = 5, 2
    d = 64 * H
    q, kv = _rand(S * Lq, d, seed=Lq, scale=1.5), _rand(S * Lk, 2 * d, seed=100 + Lk, scale=1.5)
    kpm = torch.rand(S, Lk, generator=torch.Generator().manual_seed(3)) < 0.3
    kpm[:, 0] = False
    ldq, ldkv = d + 4, 2 * d + 4
    specs = {"q": (_pitched(q, ldq), "in"), "kv": (_pitched(kv, ldkv), "in"), "kpm": (kpm.to(torch.uint8), "extent", 0), "ctx": (Out((S * Lq, d)), "out")}
    got = three_ways(lib, arena, specs, lambda o: lib.stlt_attn_cross_fwd(o.q.ptr, ldq, o.kv.ptr, o.kv.ptr + 4 * d, ldkv, o.kpm.ptr, 0, S, Lq, Lk, H, 64, o.ctx.ptr,
                                                                       _stream()), ["ctx"])["ctx"]
    sp = lambda t, Lx: t.double().reshape(S, Lx, H, 64).transpose(1, 2)
    sc = sp(q, Lq) @ sp(kv[:, :d], Lk).transpose(-1, -2) / 8.0
    sc = sc.masked_fill(kpm[:, None, None, :], float("-inf"))
    ref = (torch.softmax(sc, -1) @ sp(kv[:, d:], Lk)).transpose(1, 2).reshape(S * Lq, d)
    assert (got.double() - ref).abs().max().item() <= 2e-5


@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("lens", [[7, 1, 3], [31, 1, 33, 64, 2]])
def test_attn_ragged_fwd(lib, arena, lens, causal):
    """Segments shorter than, across and longer than the 32-row tile; seg_start / seg_end bands hold the in-range segment [0, M).
    Reference / tolerance: test_attn_ragged_matches_per_segment_softmax."""
    H = 2
    d = 64 * H
    M = sum(lens)
    qkv = _rand(M, 3 * d, seed=M + int(causal), scale=1.5)
    ln = torch.tensor(lens)
    ends = torch.cumsum(ln, 0)
    seg_start = torch.repeat_interleave(ends - ln, ln).to(torch.int32)
    seg_end = torch.repeat_interleave(ends, ln).to(torch.int32)
    specs = {"qkv": (qkv, "in"), "seg_start": (seg_start, "extent", 0), "seg_end": (seg_end, "extent", M), "ctx": (Out((M, d)), "out")}
    got = three_ways(lib, arena, specs, lambda o: lib.stlt_attn_ragged_fwd(o.qkv.ptr, o.seg_start.ptr, o.seg_end.ptr, int(causal), M, H, 64, o.ctx.ptr, _stream()),
                     ["ctx"])["ctx"]
    ref = torch.zeros(M, d, dtype=torch.float64)
    r0 = 0
    for n in lens:
        q, k, v = [qkv[r0:r0 + n, i * d:(i + 1) * d].double().view(n, H, 64).transpose(0, 1) for i in range(3)]
        sc = q @ k.transpose(1, 2) / 8.0
        if causal:
            sc = sc.masked_fill(torch.ones(n, n, dtype=torch.bool).triu(1), float("-inf"))
        ref[r0:r0 + n] = (torch.softmax(sc, -1) @ v).transpose(0, 1).reshape(n, d)
        r0 += n
    assert (got.double() - ref).abs().max().item() <= 2e-5


@pytest.mark.parametrize("causal", [True, False])
@pytest.mark.parametrize("L", [7, 17, 33, 64])
def test_mhsa_fused_fwd_ex_around_one_work_item(lib, arena, L, causal):
    """A work item is 128 rows: S·L just under and just over it; the inference form (qkv_out NULL), the training form (qkv_out
    given) and dropout of the probabilities.  References / tolerances: test_mhsa_fused_every_sequence_length (3e-5),
    test_mhsa_fused_training_form_vs_masked_oracle (qkv 3e-5, ctx 5e-5, the oracle's attention under the same counter mask)."""
    H = 2
    d = 64 * H
    seed, site = 777 + L, 8 * 5
    for S in ((128 - 1) // L, 128 // L + 1):
        x = _rand(S * L, d, seed=1000 + L, scale=1.5)
        w, b = _rand(3 * d, d, seed=1001 + L, scale=2.0 / math.sqrt(d)), _rand(3 * d, seed=1002 + L, scale=0.5)
        kpm = _kpm(S, L, 1000 + L)
        qkv_ref = (x.double() @ w.double().t() + b.double()).view(S, L, 3 * d)
        sp = lambda t: t.reshape(S, L, H, 64).transpose(1, 2)
        sc = sp(qkv_ref[..., :d]) @ sp(qkv_ref[..., d:2 * d]).transpose(-1, -2) / 8.0
        masked = kpm[:, None, None, :].expand(S, H, L, L).clone()
        if causal:
            masked |= torch.ones(L, L, dtype=torch.bool).triu(1)
        pr = torch.nan_to_num(torch.softmax(sc.masked_fill(masked, float("-inf")), -1), nan=0.0)
        for want_qkv, p in ((False, 0.0), (True, 0.0), (True, 0.25)):
            specs = {"x": (x, "in"), "w": (w, "in"), "b": (b, "in"), "kpm": (kpm.to(torch.uint8), "extent", 0), "ctx": (Out((S * L, d)), "out")}
            if want_qkv:
                specs["qkv"] = (Out((S * L, 3 * d)), "out")
            got = three_ways(lib, arena, specs, lambda o: lib.stlt_mhsa_fused_fwd_ex(
                o.x.ptr, o.w.ptr, o.b.ptr, o.kpm.ptr, int(causal), S, L, H, d, p, seed, site, o.ctx.ptr, o.qkv.ptr if want_qkv else None, _stream()),
                ["ctx"] + (["qkv"] if want_qkv else []))
            prd = O.Dropout(p, seed).attention(site, pr) if p > 0 else pr
            ref = (prd @ sp(qkv_ref[..., 2 * d:])).transpose(1, 2).reshape(S * L, d)
            assert (got["ctx"].double() - ref).abs().max().item() <= (5e-5 if want_qkv else 3e-5), (S, want_qkv, p)
            if S > 1:
                assert got["ctx"].view(S, L, d)[1].abs().max().item() == 0.0
            if want_qkv:
                assert (got["qkv"].double() - qkv_ref.view(S * L, 3 * d)).abs().max().item() <= 3e-5


# ---- row-wise kernels -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", [4, 68, 768, 2048])
def test_add_layernorm_fwd_pitches(lib, arena, d):
    """One and five rows (a block holds four), every pitch at d and d + 4, with and without the residual.  Reference / tolerance:
    test_add_layernorm."""
    w, b = 1 + _rand(d, seed=3, scale=0.2), _rand(d, seed=4, scale=0.2)
    for M in (1, 5):
        x, r = _rand(M, d, seed=1, scale=3), _rand(M, d, seed=2, scale=3)
        for ldx in (d, d + 4):
            for ldres in (d, d + 4):
                for ldout in (d, d + 4):
                    for with_res in (True, False):
                        if not with_res and ldres != d:
                            continue
                        specs = {"x": (_pitched(x, ldx), "in"), "w": (w, "in"), "b": (b, "in"), "out": (Out((M, d), ld=ldout), "out")}
                        if with_res:
                            specs["res"] = (_pitched(r, ldres), "in")
                        got = three_ways(lib, arena, specs, lambda o: lib.stlt_add_layernorm_fwd(
                            o.x.ptr, ldx, o.res.ptr if with_res else None, ldres, o.w.ptr, o.b.ptr, 1e-5, M, d, o.out.ptr, ldout, _stream()), ["out"])["out"]
                        ref = O.layer_norm((x + r if with_res else x).double(), w.double(), b.double(), 1e-5)
                        assert (got.double() - ref).abs().max().item() <= 2e-5, (M, ldx, ldres, ldout, with_res)


@pytest.mark.parametrize("n_tokens", [5, 32768 + 8 * 3 + 5])
@pytest.mark.parametrize("with_scores", [True, False])
def test_embed_fwd(lib, arena, n_tokens, with_scores):
    """The per-token kernel and the eight-tokens-per-wave kernel (last wave: 5 tokens), d = 64.  The category table has one extra row
    of NaN that no token names; the bands of `categories` hold that row's index.  Reference / tolerance: test_embed."""
    d, C = 64, 9
    g = torch.Generator().manual_seed(21)
    cats = torch.randint(0, C, (n_tokens,), generator=g)
    boxes, scores = torch.rand(n_tokens, 4, generator=g), torch.rand(n_tokens, generator=g)
    sd = {"category_embeddings.weight": _rand(C, d, seed=8), "box_embedding.weight": _rand(d, 4, seed=9, scale=0.5),
          "box_embedding.bias": _rand(d, seed=10, scale=0.5), "score_embeddings.weight": _rand(d, 1, seed=11),
          "score_embeddings.bias": _rand(d, seed=12, scale=0.5), "layer_norm.weight": 1 + _rand(d, seed=13, scale=0.1),
          "layer_norm.bias": _rand(d, seed=14, scale=0.1)}
    table = torch.cat([sd["category_embeddings.weight"], torch.full((1, d), NAN)])
    specs = {"cats": (cats, "index", C), "boxes": (boxes, "in"), "table": (table, "in"), "box_w": (sd["box_embedding.weight"], "in"),
             "box_b": (sd["box_embedding.bias"], "in"), "score_w": (sd["score_embeddings.weight"], "in"), "score_b": (sd["score_embeddings.bias"], "in"),
             "ln_w": (sd["layer_norm.weight"], "in"), "ln_b": (sd["layer_norm.bias"], "in"), "out": (Out((n_tokens, d)), "out")}
    if with_scores:
        specs["scores"] = (scores, "in")
    got = three_ways(lib, arena, specs, lambda o: lib.stlt_embed_fwd(
        o.cats.ptr, o.boxes.ptr, o.scores.ptr if with_scores else None, o.table.ptr, C + 1, o.box_w.ptr, o.box_b.ptr, o.score_w.ptr, o.score_b.ptr, o.ln_w.ptr,
        o.ln_b.ptr, 1e-12, n_tokens, d, o.out.ptr, _stream()), ["out"])["out"]
    batch = {"categories": cats, "boxes": boxes}
    if with_scores:
        batch["scores"] = scores
    ref = O.category_box_embeddings({k: v.double() for k, v in sd.items()}, "", batch, 1e-12)
    assert (got.double() - ref).abs().max().item() <= 2e-5


def test_frames_embed_fwd_and_gather_last(lib, arena):
    """stlt_frames_embed_fwd reading token 0 of (B, T, N, d) rows (row_stride = N * d; the other tokens are NaN here), frame_types
    bands naming an extra NaN row of the type table; then stlt_gather_last_fwd (lengths bands: 1).  Reference / tolerance:
    test_frames_embed_and_gather."""
    B, T, N, d = 3, 6, 4, 256
    sp = torch.full((B * T, N * d), NAN)
    sp0 = _rand(B * T, d, seed=1)
    sp[:, :d] = sp0
    ft = torch.randint(0, 5, (B, T), generator=torch.Generator().manual_seed(2))
    P, F = _rand(256, d, seed=3), torch.cat([_rand(5, d, seed=4), torch.full((1, d), NAN)])
    w, b = 1 + _rand(d, seed=5, scale=0.1), _rand(d, seed=6, scale=0.1)
    specs = {"sp": (sp, "in"), "ft": (ft, "index", 5), "P": (P, "in"), "F": (F, "in"), "w": (w, "in"), "b": (b, "in"), "out": (Out((B * T, d)), "out")}
    got = three_ways(lib, arena, specs, lambda o: lib.stlt_frames_embed_fwd(o.sp.ptr, N * d, o.ft.ptr, o.P.ptr, o.F.ptr, o.w.ptr, o.b.ptr, 1e-12, B, T, d, o.out.ptr,
                                                                         _stream()), ["out"])["out"]
    ref = O.layer_norm((sp0.view(B, T, d) + P[:T][None] + F[ft]).double(), w.double(), b.double(), 1e-12)
    assert (got.view(B, T, d).double() - ref).abs().max().item() <= 2e-5
    lengths = torch.tensor([6, 2, 4])
    specs = {"x": (got.contiguous(), "in"), "lengths": (lengths, "extent", 1), "out": (Out((B, d)), "out")}
    h = three_ways(lib, arena, specs, lambda o: lib.stlt_gather_last_fwd(o.x.ptr, o.lengths.ptr, B, T, d, o.out.ptr, _stream()), ["out"])["out"]
    assert torch.equal(h, got.view(B, T, d)[torch.arange(B), lengths - 1])  # pure data movement: bit exact


@pytest.mark.parametrize("with_scores", [True, False])
def test_collate_fwd(lib, arena, with_scores):
    """Ragged lengths, scores given and NULL.  Pure data movement: bit exact against the padding rule of include/stlt_hip.h."""
    specs, call, want = GA.collate_case(with_scores)
    got = three_ways(lib, arena, specs, call(lib), list(want))
    for n, ref in want.items():
        assert torch.equal(got[n], ref), n


# ---- element-wise ops -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 1027])
def test_gelu_dropout_relu_elementwise(lib, arena, n):
    """One element and a count off every vector width, on aligned buffers.  GELU against the exact erf form in fp64 (2e-5 relative to
    the gradient scale, as test_add_layernorm_and_gelu_autograd); dropout keeps exactly the oracle's counter mask, survivors
    x / (1 - p) to 8e-6 (test_dropout_op_mask_scale_and_backward); the ReLU backward is a select (bit exact)."""
    x, dy = _rand(n, seed=1, scale=3), _rand(n, seed=2)
    # the two GELU entry points take whole 16-byte vectors only (include/stlt_hip.h: n % 4 == 0): 1 and 1027 are refused before anything is
    # launched, and the nearest counts they do take (4, 1028) run inside the bands
    arena.reset()
    xa, ya = arena.place(x, "in"), arena.place(Out((n,)), "out")
    assert lib.stlt_gelu_fwd(xa.ptr, ya.ptr, n, _stream()) == -1 and "multiple of 4" in _err(lib)
    assert lib.stlt_gelu_bwd(xa.ptr, xa.ptr, ya.ptr, n, _stream()) == -1 and "multiple of 4" in _err(lib)
    arena.check(launched=False)
    n4 = (n + 3) // 4 * 4
    x4, dy4 = _rand(n4, seed=1, scale=3), _rand(n4, seed=2)
    got = three_ways(lib, arena, {"x": (x4, "in"), "y": (Out((n4,)), "out")}, lambda o: lib.stlt_gelu_fwd(o.x.ptr, o.y.ptr, n4, _stream()), ["y"])["y"]
    assert (got.double() - O.gelu(x4.double())).abs().max().item() <= 2e-5
    x64 = x4.double().requires_grad_(True)
    O.gelu(x64).backward(dy4.double())
    got = three_ways(lib, arena, {"x": (x4, "in"), "dy": (dy4, "in"), "dx": (Out((n4,)), "out")},
                     lambda o: lib.stlt_gelu_bwd(o.dy.ptr, o.x.ptr, o.dx.ptr, n4, _stream()), ["dx"])["dx"]
    assert (got.double() - x64.grad).abs().max().item() / max(x64.grad.abs().max().item(), 1e-6) <= 2e-5
    p, seed, site = 0.3, 12345, 0x200000
    xd = _rand(n, seed=4) + 3.0  # no zeros in the input: a zero in the output is a dropped element
    got = three_ways(lib, arena, {"x": (xd, "in"), "y": (Out((n,)), "out")}, lambda o: lib.stlt_dropout(o.x.ptr, o.y.ptr, n, p, seed, site, _stream()), ["y"])["y"]
    keep = torch.from_numpy(O.dropout_keep(p, seed, site, np.arange(n, dtype=np.uint64)))
    assert torch.equal(got != 0, keep)
    assert (got[keep] - xd[keep] / (1 - p)).abs().max().item() <= 1e-6 * 8 if bool(keep.any()) else True
    y = torch.relu(_rand(n, seed=3))
    got = three_ways(lib, arena, {"dy": (dy, "in"), "y": (y, "in"), "dx": (Out((n,)), "out")},
                     lambda o: lib.stlt_relu_bwd(o.dy.ptr, o.y.ptr, o.dx.ptr, n, _stream()), ["dx"])["dx"]
    assert torch.equal(got, torch.where(y > 0, dy, torch.zeros_like(dy)))


# ---- op-level backward and optimiser: scratch of exactly the bytes the library asks for ---------------------------------------------------
def _scratch_spec(nbytes):
    return (Out((int(nbytes),), torch.uint8, must_write=False), "out")


def _rel(got, ref):
    return (got.double() - ref).abs().max().item() / max(ref.abs().max().item(), 1e-6)


def test_linear_bwd(lib, arena):
    """(40, 64, 32), the smallest shape of test_linear_autograd (2e-5 of each gradient's scale).  dw / db accumulate: they start as zeros."""
    M, N, K = 40, 64, 32
    x, w, b, g = _rand(M, K, seed=1), _rand(N, K, seed=2, scale=1 / math.sqrt(K)), _rand(N, seed=3, scale=0.1), _rand(M, N, seed=4)
    x64, w64, b64 = [t.double().requires_grad_(True) for t in (x, w, b)]
    (x64 @ w64.t() + b64).backward(g.double())
    nbytes = int(lib.stlt_linear_bwd_scratch_bytes(N))
    specs = {"x": (x, "in"), "w": (w, "in"), "dy": (g, "in"), "dx": (Out((M, K)), "out"), "dw": (torch.zeros(N, K), "out"), "db": (torch.zeros(N), "out"),
             "scratch": _scratch_spec(nbytes)}
    got = three_ways(lib, arena, specs, lambda o: lib.stlt_linear_bwd(o.x.ptr, o.w.ptr, o.dy.ptr, M, N, K, o.dx.ptr, o.dw.ptr, o.db.ptr, None, o.scratch.ptr, nbytes,
                                                                   _stream()), ["dx", "dw", "db"])
    for name, ref in (("dx", x64.grad), ("dw", w64.grad), ("db", b64.grad)):
        assert _rel(got[name], ref) <= 2e-5, name


def test_add_layernorm_bwd_wide_rows(lib, arena):
    """d = 1028 (above 1024: the wide-row kernel), M = 1300 as test_add_layernorm_and_gelu_autograd (2e-5 of each gradient's scale)."""
    M, d = 1300, 1028
    x, r, w, b, g = _rand(M, d, seed=1), _rand(M, d, seed=2), 1 + _rand(d, seed=3, scale=0.1), _rand(d, seed=4, scale=0.1), _rand(M, d, seed=5)
    s64, w64, b64 = (x + r).double().requires_grad_(True), w.double().requires_grad_(True), b.double().requires_grad_(True)
    torch.nn.functional.layer_norm(s64, (d,), w64, b64, 1e-5).backward(g.double())
    nbytes = int(lib.stlt_add_layernorm_bwd_scratch_bytes(d))
    specs = {"dy": (g, "in"), "x": (x, "in"), "res": (r, "in"), "w": (w, "in"), "ds": (Out((M, d)), "out"), "gw": (torch.zeros(d), "out"), "gb": (torch.zeros(d), "out"),
             "scratch": _scratch_spec(nbytes)}
    got = three_ways(lib, arena, specs, lambda o: lib.stlt_add_layernorm_bwd(o.dy.ptr, o.x.ptr, o.res.ptr, o.w.ptr, 1e-5, M, d, o.ds.ptr, o.gw.ptr, o.gb.ptr,
                                                                          o.scratch.ptr, nbytes, _stream()), ["ds", "gw", "gb"])
    for name, ref in (("ds", s64.grad), ("gw", w64.grad), ("gb", b64.grad)):
        assert _rel(got[name], ref) <= 2e-5, name


def test_attn_core_bwd(lib, arena):
    """L = 17 (two sixteen-row blocks), causal, padded keys and a fully padded sequence, no dropout: dqkv and its column sums as
    test_attn_core_bwd_mfma_blocks_vs_fp64 (2e-5 / 5e-5 of scale)."""
    S, L, H = 5, 17, 2
    d = 64 * H
    qkv, g, kpm = _rand(S, L, 3 * d, seed=L, scale=1.5), _rand(S, L, d, seed=L + 1), _kpm(S, L, L)
    x = qkv.double().requires_grad_(True)
    sp = lambda t: t.reshape(S, L, H, 64).transpose(1, 2)
    sc = sp(x[..., :d]) @ sp(x[..., d:2 * d]).transpose(-1, -2) / 8.0
    masked = kpm[:, None, None, :].expand(S, H, L, L).clone() | torch.ones(L, L, dtype=torch.bool).triu(1)
    pr = torch.nan_to_num(torch.softmax(sc.masked_fill(masked, float("-inf")), -1), nan=0.0)
    (pr @ sp(x[..., 2 * d:])).transpose(1, 2).reshape(S, L, d).backward(g.double())
    nbytes = int(lib.stlt_attn_core_bwd_scratch_bytes(H))
    specs = {"qkv": (qkv, "in"), "dctx": (g, "in"), "kpm": (kpm.to(torch.uint8), "extent", 0), "dqkv": (Out((S * L, 3 * d)), "out"), "gb": (torch.zeros(3 * d), "out"),
             "scratch": _scratch_spec(nbytes)}
    got = three_ways(lib, arena, specs, lambda o: lib.stlt_attn_core_bwd(o.qkv.ptr, o.dctx.ptr, o.kpm.ptr, 1, S, L, H, 64, 0.0, 0, 0, o.dqkv.ptr, o.gb.ptr, o.scratch.ptr,
                                                                      nbytes, _stream()), ["dqkv", "gb"])
    ref = x.grad.reshape(S * L, 3 * d)
    assert _rel(got["dqkv"], ref) <= 2e-5 and _rel(got["gb"], ref.sum(0)) <= 5e-5
    assert got["dqkv"].view(S, L, 3 * d)[1].abs().max().item() == 0.0


@pytest.mark.parametrize("Lq,Lk", [(1, 5), (33, 16)])
def test_attn_bwd(lib, arena, Lq, Lk):
    """Queries and keys from different buffers, k | v the halves of one packed projection, dq / dk / dv with their own pitches; padded
    keys and a fully padded sequence, no dropout.  Reference / tolerance: test_attn_cross_bwd_mfma_vs_fp64 (2e-5 of scale)."""
    S, H = 5, 2
    d = 64 * H
    q, kv, g = _rand(S * Lq, d, seed=Lq, scale=1.5), _rand(S * Lk, 2 * d, seed=Lk + 100, scale=1.5), _rand(S * Lq, d, seed=Lq + Lk)
    kpm = _kpm(S, Lk, Lk)
    qr, kvr = q.double().requires_grad_(True), kv.double().requires_grad_(True)
    sp = lambda t, L_: t.reshape(S, L_, H, 64).transpose(1, 2)
    sc = sp(qr, Lq) @ sp(kvr[..., :d], Lk).transpose(-1, -2) / 8.0
    pr = torch.nan_to_num(torch.softmax(sc.masked_fill(kpm[:, None, None, :].expand(S, H, Lq, Lk), float("-inf")), -1), nan=0.0)
    (pr @ sp(kvr[..., d:], Lk)).transpose(1, 2).reshape(S * Lq, d).backward(g.double())
    specs = {"q": (q, "in"), "kv": (kv, "in"), "dctx": (g, "in"), "kpm": (kpm.to(torch.uint8), "extent", 0), "dq": (Out((S * Lq, d)), "out"),
             "dkv": (Out((S * Lk, 2 * d)), "out")}
    got = three_ways(lib, arena, specs, lambda o: lib.stlt_attn_bwd(o.q.ptr, d, o.kv.ptr, o.kv.ptr + 4 * d, 2 * d, o.dctx.ptr, o.kpm.ptr, 0, S, Lq, Lk, H, 64, 0.0, 0, 0,
                                                                 o.dq.ptr, d, o.dkv.ptr, o.dkv.ptr + 4 * d, 2 * d, _stream()), ["dq", "dkv"])
    assert _rel(got["dq"], qr.grad) <= 2e-5 and _rel(got["dkv"], kvr.grad) <= 2e-5
    assert got["dq"].view(S, Lq, d)[1].abs().max().item() == 0.0 and got["dkv"].view(S, Lk, 2 * d)[1].abs().max().item() == 0.0


@pytest.mark.parametrize("with_scores", [True, False])
def test_embed_bwd(lib, arena, with_scores):
    """Parameter gradients of K1 from the gradient wrt the pre-LayerNorm sum (they accumulate: zeros to start with), 90 tokens (the
    3 x 5 x 6 batch of test_embed), scratch of exactly stlt_embed_bwd_scratch_bytes.  The category table has one extra row that no token
    names and the bands of `categories` hold its index: that row's gradient must stay zero, like row 0's (the padding index).  The ops
    have no op-level test of their own; the bar is the 2e-5 of each gradient's scale of the other op-level backward tests."""
    n, d, C = 90, 64, 9
    g0 = torch.Generator().manual_seed(7)
    cats, boxes, scores, d_pre = torch.randint(0, C, (n,), generator=g0), torch.rand(n, 4, generator=g0), torch.rand(n, generator=g0), _rand(n, d, seed=5)
    g64 = d_pre.double()
    ref = {"g_cat": torch.zeros(C + 1, d, dtype=torch.float64).index_add_(0, cats, g64), "g_box_w": g64.t() @ boxes.double(), "g_box_b": g64.sum(0)}
    ref["g_cat"][0] = 0.0
    nbytes = int(lib.stlt_embed_bwd_scratch_bytes(n, C + 1, d))
    specs = {"d_pre": (d_pre, "in"), "cats": (cats, "index", C), "boxes": (boxes, "in"), "g_cat": (torch.zeros(C + 1, d), "out"), "g_box_w": (torch.zeros(d, 4), "out"),
             "g_box_b": (torch.zeros(d), "out"), "scratch": _scratch_spec(nbytes)}
    if with_scores:
        specs.update({"scores": (scores, "in"), "g_sw": (torch.zeros(d, 1), "out"), "g_sb": (torch.zeros(d), "out")})
        ref["g_sw"], ref["g_sb"] = (g64 * scores.double()[:, None]).sum(0)[:, None], g64.sum(0)
    sc = lambda o, k: getattr(o, k).ptr if with_scores else None
    got = three_ways(lib, arena, specs, lambda o: lib.stlt_embed_bwd(o.d_pre.ptr, o.cats.ptr, o.boxes.ptr, sc(o, "scores"), C + 1, n, d, o.g_cat.ptr, o.g_box_w.ptr,
                                                                  o.g_box_b.ptr, sc(o, "g_sw"), sc(o, "g_sb"), o.scratch.ptr, nbytes, _stream()), list(ref))
    for k, r in ref.items():
        assert _rel(got[k], r) <= 2e-5, k
    assert got["g_cat"][C].abs().max().item() == 0.0 and got["g_cat"][0].abs().max().item() == 0.0


def test_frames_embed_bwd(lib, arena):
    """Position and frame-type gradients of K7 (accumulating), B = 3, T = 6, d = 256 (test_frames_embed_and_gather), scratch of exactly
    stlt_frames_embed_bwd_scratch_bytes; the type table's extra row, named only by the bands of frame_types, stays zero like row 0."""
    B, T, d, n_types = 3, 6, 256, 5
    ft, d_pre = torch.randint(0, n_types, (B, T), generator=torch.Generator().manual_seed(2)), _rand(B, T, d, seed=3)
    g64 = d_pre.double()
    ref_pos = g64.sum(0)
    ref_type = torch.zeros(n_types + 1, d, dtype=torch.float64).index_add_(0, ft.reshape(-1), g64.reshape(-1, d))
    ref_type[0] = 0.0
    nbytes = int(lib.stlt_frames_embed_bwd_scratch_bytes(T, d))
    specs = {"d_pre": (d_pre, "in"), "ft": (ft, "index", n_types), "g_pos": (torch.zeros(T, d), "out"), "g_type": (torch.zeros(n_types + 1, d), "out"),
             "scratch": _scratch_spec(nbytes)}
    got = three_ways(lib, arena, specs, lambda o: lib.stlt_frames_embed_bwd(o.d_pre.ptr, o.ft.ptr, B, T, d, o.g_pos.ptr, o.g_type.ptr, o.scratch.ptr, nbytes, _stream()),
                     ["g_pos", "g_type"])
    assert _rel(got["g_pos"], ref_pos) <= 2e-5 and _rel(got["g_type"], ref_type) <= 2e-5
    assert got["g_type"][n_types].abs().max().item() == 0.0 and got["g_type"][0].abs().max().item() == 0.0


@pytest.mark.parametrize("kind", [0, 1])
def test_loss_fwd_bwd(lib, arena, kind):
    """Cross entropy (labels int64) and BCE with logits (labels float multi-hot), B = 37, K = 157, scratch of exactly B floats.  The label
    bands hold the in-range class 0 (an out-of-range label is flagged by design) and the logits bands NaN.  Reference / tolerance:
    test_fused_criterion_matches_torch (loss 2e-6 relative, gradient 1e-7)."""
    B, K = 37, 157
    g0 = torch.Generator().manual_seed(3)
    logits = torch.randn(B, K, generator=g0) * 3
    l64 = logits.double().requires_grad_(True)
    if kind == 0:
        labels = torch.randint(0, K, (B,), generator=g0)
        ref = torch.nn.functional.cross_entropy(l64, labels)
        lab_spec = (labels, "index", 0)
    else:
        labels = (torch.rand(B, K, generator=g0) < 0.1).float()
        ref = torch.nn.functional.binary_cross_entropy_with_logits(l64, labels.double())
        lab_spec = (labels, "in")
    ref.backward()
    specs = {"logits": (logits, "in"), "labels": lab_spec, "scratch": (Out((B,), must_write=False), "out"), "loss": (Out((1,)), "out"), "dl": (Out((B, K)), "out")}
    got = three_ways(lib, arena, specs, lambda o: lib.stlt_loss_fwd_bwd(o.logits.ptr, o.labels.ptr, kind, B, K, 1.0, o.scratch.ptr, o.loss.ptr, o.dl.ptr, _stream()),
                     ["loss", "dl"])
    assert abs(got["loss"].item() - ref.item()) <= 2e-6 * max(1.0, abs(ref.item()))
    assert (got["dl"].double() - l64.grad).abs().max().item() <= 1e-7


@pytest.mark.parametrize("scale", [10.0, 0.01])
def test_grad_norm_and_adamw_step(pkg, lib, arena, scale):
    """One step of stlt_grad_norm + stlt_adamw_step on the odd-sized tensors of test_fused_adamw_matches_torch_adamw_and_clip (norm above
    and below max_norm = 5): parameters, moments, the flat gradient, the 1024-float scratch and the two-float result are arena
    operands.  Against clip_grad_norm_ + torch.optim.AdamW in fp32 on the host, that test's tolerances (norm 1e-5 relative, parameters 2e-6)."""
    g0 = torch.Generator().manual_seed(0)
    shapes = [(174, 96), (174,), (33, 7), (50000,), (3,)]
    wds = [1e-2, 0.0, 1e-2, 1e-2, 0.0]
    params = [torch.randn(*s, generator=g0) for s in shapes]
    grads = [torch.randn(*s, generator=g0) * scale for s in shapes]
    ref_p = [torch.nn.Parameter(p.clone()) for p in params]
    for p, g in zip(ref_p, grads):
        p.grad = g.clone()
    n_ref = torch.nn.utils.clip_grad_norm_(ref_p, 5.0)
    torch.optim.AdamW([{"params": [p], "weight_decay": wd} for p, wd in zip(ref_p, wds)], lr=3e-3).step()
    offs, off = [], 0
    for p in params:
        offs.append(off)
        off += (p.numel() + 3) // 4 * 4
    flat = torch.zeros(off)
    for o, g in zip(offs, grads):
        flat[o:o + g.numel()] = g.reshape(-1)
    CH = 16384
    specs = {"flat": (flat, "in"), "m": (torch.zeros(off), "out"), "v": (torch.zeros(off), "out"), "scratch": (Out((1024,), must_write=False), "out"),
             "norm": (Out((2,)), "out")}
    for i, p in enumerate(params):
        specs[f"p{i}"] = (p.reshape(-1).clone(), "out")
    n_chunks = sum((p.numel() + CH - 1) // CH for p in params)
    specs["table"] = (torch.zeros(n_chunks * 24, dtype=torch.uint8), "extent", 0)  # filled per run: it holds the run's own pointers

    def call(o):
        rows = []
        for i, p in enumerate(params):
            for c0 in range(0, p.numel(), CH):
                rows.append((getattr(o, f"p{i}").ptr + 4 * c0, offs[i] + c0, min(CH, p.numel() - c0), wds[i]))
        arr = np.zeros(len(rows), dtype=np.dtype([("param", "<u8"), ("off", "<i8"), ("n", "<i4"), ("wd", "<f4")]))
        for i, r in enumerate(rows):
            arr[i] = r
        assert arr.dtype.itemsize == 24 and len(rows) == n_chunks
        o.table.flat.copy_(torch.from_numpy(arr.view(np.uint8).copy()))
        rc = lib.stlt_grad_norm(o.flat.ptr, off, 5.0, o.scratch.ptr, o.norm.ptr, _stream())
        return rc or lib.stlt_adamw_step(o.table.ptr, n_chunks, o.flat.ptr, o.m.ptr, o.v.ptr, o.norm.ptr, 3e-3, 0.9, 0.999, 1e-8, 1, _stream())

    outs = ["norm", "m", "v"] + [f"p{i}" for i in range(len(params))]
    P = {n: GA.plain(s[0], DEV) for n, s in specs.items()}
    assert call(SimpleNamespace(**P)) == 0, _err(lib)
    torch.cuda.synchronize()
    base = {n: P[n].view.clone() for n in outs}
    for rep in range(2):  # the table holds this placement's pointers, so it is re-placed with everything else (an input that cannot be kept)
        arena.reset()
        A = SimpleNamespace(**{n: arena.place(s[0], s[1], band=(s[2] if len(s) > 2 else None), name=n) for n, s in specs.items()})
        assert call(A) == 0, _err(lib)
        A.table.saved = arena.buf[A.table.start:A.table.start + A.table.nbytes].clone()  # written by the host above, not by a kernel
        arena.check()
        for n in outs:
            assert torch.equal(getattr(A, n).view, base[n]), n
    assert abs(base["norm"][0].item() - n_ref.item()) <= 1e-5 * n_ref.item()
    for i, p in enumerate(ref_p):
        assert (base[f"p{i}"].cpu() - p.detach().reshape(-1)).abs().max().item() <= 2e-6, i


# ---- evaluators -------------------------------------------------------------------------------------------------------------------------
def test_eval_topk_with_a_pitch(lib, arena):
    """logits at ld = K + 3 (gap columns NaN: a NaN that entered a comparison would change a rank), the two int64 counters accumulate
    from 5 / 7.  Exact: the label's rank is the number of classes with a larger logit, or an equal one at a lower index."""
    B, K = 37, 157
    g0 = torch.Generator().manual_seed(3)
    logits, labels = torch.randn(B, K, generator=g0), torch.randint(0, K, (B,), generator=g0)
    logits[5, 9] = logits[5, labels[5]]  # a tie
    own = logits[torch.arange(B), labels][:, None]
    idx = torch.arange(K)[None]
    rank = ((logits > own) | ((logits == own) & (idx < labels[:, None]))).sum(1)
    want = torch.tensor([5 + int((rank == 0).sum()), 7 + int((rank < 5).sum())])
    specs = {"logits": (_pitched(logits, K + 3), "in"), "labels": (labels, "index", 0), "counts": (torch.tensor([5, 7]), "out")}
    got = three_ways(lib, arena, specs, lambda o: lib.stlt_eval_topk(o.logits.ptr, K + 3, o.labels.ptr, B, K, o.counts.ptr, _stream()), ["counts"])["counts"]
    assert torch.equal(got, want)


def test_eval_store_sigmoid_into_rows_past_the_first(lib, arena):
    """Rows [row0, row0 + B) of the two float64 tables are written; the rows before and after keep what they held (they are part of the
    guard).  pred = (double)sigmoid_f32(logits) to 1.2e-7 (test_evaluation.py), truth exact."""
    B, C, total, row0 = 5, 157, 12, 4
    g0 = torch.Generator().manual_seed(4)
    logits, labels = torch.randn(B, C, generator=g0) * 3, (torch.rand(B, C, generator=g0) < 0.1).float()
    keep = torch.full((total, C), -7.0, dtype=torch.float64)
    specs = {"logits": (_pitched(logits, C + 3), "in"), "labels": (labels, "in"), "pred": (keep.clone(), "out"), "truth": (keep.clone(), "out")}
    got = three_ways(lib, arena, specs, lambda o: lib.stlt_eval_store_sigmoid(o.logits.ptr, C + 3, o.labels.ptr, B, C, o.pred.ptr, o.truth.ptr, row0, _stream()),
                     ["pred", "truth"])
    for name in ("pred", "truth"):
        rest = torch.cat([got[name][:row0], got[name][row0 + B:]])
        assert bool((rest == -7.0).all()), name
    assert (got["pred"][row0:row0 + B] - logits.sigmoid().double()).abs().max().item() <= 1.2e-7
    assert torch.equal(got["truth"][row0:row0 + B], labels.double())


@pytest.mark.parametrize("n", [1, 1025])
def test_eval_average_precision(pkg, lib, arena, n):
    """One clip and 1025 clips (past 1024), C = 3, scratch of exactly n bytes; a class without positives (NaN) and clips without
    any positive (the empty-clip rule).  Against the package's batched float64 form of the same arithmetic on the host, 1e-12
    (test_evaluation.py)."""
    C = 3
    g0 = torch.Generator().manual_seed(n)
    scores = torch.rand(n, C, generator=g0)
    truths = (torch.rand(n, C, generator=g0) < 0.3).float()
    truths[:, 2] = 0.0 if n == 1 else truths[:, 2]
    ref = pkg.utils.evaluation.charades_map(scores.double(), truths.double())[2]
    specs = {"scores": (scores, "in"), "truths": (truths, "in"), "ap": (Out((C,), torch.float64), "out"), "pos": (Out((C,), torch.float64), "out"),
             "scratch": (Out((n,), torch.uint8, must_write=False), "out")}
    P = SimpleNamespace(**{k: GA.plain(v[0], DEV) for k, v in specs.items()})
    call = lambda o: lib.stlt_eval_average_precision(o.scores.ptr, o.truths.ptr, n, C, o.ap.ptr, o.pos.ptr, o.scratch.ptr, _stream())
    assert call(P) == 0, _err(lib)
    torch.cuda.synchronize()
    for rep in range(2):  # NaN results: compared as bits, which torch.equal (and so three_ways) cannot do
        if rep == 0:
            arena.reset()
            A = SimpleNamespace(**{k: arena.place(v[0], v[1], name=k) for k, v in specs.items()})
        else:
            arena.refill_outputs()
        assert call(A) == 0, _err(lib)
        arena.check()
        for k in ("ap", "pos"):
            assert torch.equal(getattr(A, k).view.view(torch.int64), getattr(P, k).view.view(torch.int64)), k
    np.testing.assert_allclose(A.ap.view.cpu().numpy(), ref.numpy(), rtol=0, atol=1e-12, equal_nan=True)
    assert torch.equal(A.pos.view.cpu(), truths.double().sum(0))


# ---- whole-path calls inside exactly the bytes the library asks for -----------------------------------------------------------------
def _stlt_model(pkg, name="cfg1"):
    model = pkg.Stlt(pkg.StltModelConfig(**pkg.synth.model_kwargs(name)))
    sd = pkg.synth.make_state_dict({k: tuple(v.shape) for k, v in model.state_dict().items()}, seed=1234)
    model.load_state_dict(sd)
    model.train(False)
    return model.to(DEV)


def _batch(pkg, B, name="cfg1", seed=0):
    c = pkg.synth.CONFIGS[name]
    return {k: v.to(DEV) for k, v in pkg.synth.make_batch(B, c["T"], c["N"], seed=seed).items()}


def _exact_buffers(pkg, monkeypatch, arena):
    """modelling.models hands the library grow-only / reused buffers; here every request is an arena operand of exactly the bytes
    asked for (the training buffers zero-filled and kept for the step, as _train_buf's contract says)."""
    models = pkg.modelling.models
    kept = {}

    def get(self, nbytes, device):
        return arena.place(Out((nbytes,), torch.uint8, must_write=False), "out", name=f"workspace[{nbytes}]").flat

    def train_buf(self, name, nbytes, device):
        if (name, nbytes) not in kept:
            kept[(name, nbytes)] = arena.place(torch.zeros(nbytes, dtype=torch.uint8), "out", name=f"{name}[{nbytes}]").flat
        return kept[(name, nbytes)]

    monkeypatch.setattr(models._Workspace, "get", get)
    monkeypatch.setattr(models.StltBackbone, "_train_buf", train_buf)
    return kept


@pytest.mark.parametrize("variant", ["padded", "skip_padding", "no_elision"])
def test_stlt_forward_inside_exactly_stlt_workspace_bytes(pkg, arena, monkeypatch, variant):
    """cfg1, B = 3 then the strictly smaller B = 1 on ONE model instance (with exact-size buffers this is the case the grow-only cache
    hides), each inside a workspace of exactly stlt_workspace_bytes: bands intact, logits bit-identical to the unpatched run."""
    model = _stlt_model(pkg)
    if variant == "skip_padding":
        model.backbone.skip_padding = True
    elif variant == "no_elision":
        model.backbone.cls_only_last_spatial = model.backbone.last_row_only_temporal = False
    batches = [_batch(pkg, B) for B in (3, 1)]
    with torch.no_grad():
        want = [model(b)["stlt"].clone() for b in batches]
        _exact_buffers(pkg, monkeypatch, arena)
        for b, ref in zip(batches, want):
            arena.reset()
            got = model(b)["stlt"]
            arena.check()
            assert len(arena.operands) == 1 and torch.equal(got, ref), tuple(b["categories"].shape)


def test_stlt_train_step_inside_exactly_the_tape_and_scratch_bytes(pkg, arena, monkeypatch):
    """One grad-enabled forward + backward at cfg1, B = 3: the tape is exactly stlt_train_tape_bytes, the scratch exactly
    stlt_train_scratch_bytes; logits and every gradient bit-identical to the unpatched run."""
    model = _stlt_model(pkg)
    batch = _batch(pkg, 3)

    def step():
        model.zero_grad(set_to_none=True)
        logits = model(batch)["stlt"]
        logits.square().sum().backward()
        torch.cuda.synchronize()
        return logits.detach().clone(), {n: q.grad.clone() for n, q in model.named_parameters() if q.grad is not None}

    ref_logits, ref_grads = step()
    kept = _exact_buffers(pkg, monkeypatch, arena)
    arena.reset()
    logits, grads = step()
    arena.check()
    assert {k[0] for k in kept} == {"tape", "scratch"}
    assert torch.equal(logits, ref_logits) and grads.keys() == ref_grads.keys() and len(grads) > 0
    for n in grads:
        assert torch.equal(grads[n], ref_grads[n]), n


def _fusion_model(pkg, name, S):
    small = dict(num_spatial_layers=2, num_temporal_layers=1, num_appearance_layers=1, num_fusion_layers=1)  # test_fusion_train_gpu.SMALL
    kw = dict(pkg.synth.model_kwargs("cfg1"), **small, appearance_num_frames=S, hidden_dropout_prob=0.0)
    m = pkg.models_factory[name](pkg.MultimodalModelConfig(**kw))
    m.load_state_dict(pkg.synth.make_state_dict({k: tuple(v.shape) for k, v in m.state_dict().items()}, seed=17))
    return m.to(DEV).train(False)


def _fusion_batch(pkg, B, T, N, grid, seed):
    batch = pkg.synth.make_batch(B, T, N, seed=seed, min_len=2)
    batch["appearance_features"] = pkg.synth.make_appearance_features(B, seed=seed + 1, grid=grid)
    return {k: v.to(DEV) for k, v in batch.items()}


def _exact_op_scratch(pkg, monkeypatch, arena):
    """ops._scratch / ops._sk_scratch are grow-only caches too: here each distinct request is an arena operand of exactly its size
    (one per (bytes, slot) for the step, as calls of one stream may share a buffer)."""
    kept = {}

    def scratch(nbytes, device, slot=0):
        if (nbytes, slot) not in kept:
            kept[(nbytes, slot)] = arena.place(Out((nbytes,), torch.uint8, must_write=False), "out", name=f"scratch{slot}[{nbytes}]").flat
        return kept[(nbytes, slot)]

    monkeypatch.setattr(pkg.ops, "_scratch", scratch)
    monkeypatch.setattr(pkg.ops, "_sk_scratch", lambda device: scratch(int(pkg._lib.load().stlt_gemm_scratch_bytes()), device, "sk"))
    return kept


@pytest.mark.parametrize("name", ["caf", "cacnf", "lcf"])
def test_fusion_forward_inside_exactly_stlt_caf_workspace_bytes(pkg, arena, monkeypatch, name):
    """The smallest SHAPES entry of test_fusion_train_gpu.py, (B, T, N, grid) = (1, 2, 1, (1, 2, 4)): every logit head bit-identical to
    the unpatched forward, the workspace's bands intact."""
    B, T, N, grid = 1, 2, 1, (1, 2, 4)
    m = _fusion_model(pkg, name, 8)
    batch = _fusion_batch(pkg, B, T, N, grid, seed=100 * T + N + B)
    with torch.no_grad():
        want = {k: v.clone() for k, v in m(batch).items()}
        _exact_buffers(pkg, monkeypatch, arena)
        arena.reset()
        got = m(batch)
        arena.check()
    assert len(arena.operands) >= 1 and got.keys() == want.keys()
    for k in want:
        assert torch.equal(got[k], want[k]), k


def test_cacnf_training_step_inside_exactly_the_bytes_asked_for(pkg, arena, monkeypatch):
    """One CACNF forward + backward (eval mode: no dropout; grad on: the training composition of block calls over the layout branch's
    native tape) with the tape, the sweep's scratch, every block keep / work buffer and every op-level scratch an exact-size arena
    operand: logits and gradients bit-identical to the unpatched step."""
    B, T, N, grid = 1, 2, 1, (1, 2, 4)
    m = _fusion_model(pkg, "cacnf", 8)
    batch = _fusion_batch(pkg, B, T, N, grid, seed=100 * T + N + B)
    labels = torch.tensor([3], device=DEV)

    def step():
        m.zero_grad(set_to_none=True)
        out = m(batch)
        (sum(torch.nn.functional.cross_entropy(v, labels) for v in out.values()) / len(out)).backward()
        torch.cuda.synchronize()
        return {k: v.detach().clone() for k, v in out.items()}, {n: q.grad.clone() for n, q in m.named_parameters() if q.grad is not None}

    ref_out, ref_g = step()
    _exact_buffers(pkg, monkeypatch, arena)
    kept = _exact_op_scratch(pkg, monkeypatch, arena)
    arena.reset()
    out, g = step()
    arena.check()
    assert len(kept) > 0 and g.keys() == ref_g.keys() and len(g) >= 20
    for k in ref_out:
        assert torch.equal(out[k], ref_out[k]), k
    for n in ref_g:
        assert torch.equal(g[n], ref_g[n]), n


# ---- the R3D-50 trunk inside exactly its workspace, tape and backward workspace ------------------------------------------------------------
class _TorchWithExactTape:
    """Stands in for the `torch` module inside modelling.resnet3d: its tape is a plain torch.empty there, so the one-dimensional uint8
    allocations of that module come from the arena instead; every other attribute is torch's."""

    def __init__(self, arena):
        self._arena = arena

    def __getattr__(self, name):
        return getattr(torch, name)

    def empty(self, *size, **kw):
        if kw.get("dtype") == torch.uint8 and len(size) == 1 and isinstance(size[0], int):
            return self._arena.place(Out((size[0],), torch.uint8, must_write=False), "out", name=f"tape[{size[0]}]").flat
        return torch.empty(*size, **kw)


def test_r3d_trunk_forward_and_backward_inside_exactly_the_bytes_asked_for(pkg, arena, monkeypatch):
    """Resnet3D at (1, 8, 64, 64), the smallest shape of tests/test_r3d_shapes_gpu.py: the inference forward inside exactly
    stlt_r3d_workspace_bytes, then a grad-enabled forward + backward with the tape (stlt_r3d_tape_bytes) and the backward workspace
    (stlt_r3d_backward_workspace_bytes) exact as well; features and every weight gradient bit-identical to the unpatched run."""
    kw = pkg.synth.model_kwargs("cfg1")
    cfg = pkg.AppearanceModelConfig(num_classes=kw["num_classes"], hidden_size=kw["hidden_size"], num_attention_heads=kw["num_attention_heads"],
                                    hidden_dropout_prob=0.0, appearance_num_frames=32, train_trunk=True)
    m = pkg.Resnet3D(cfg)
    m.load_state_dict(pkg.synth.make_r3d_state_dict({k: tuple(v.shape) for k, v in m.state_dict().items()}, seed=4242), strict=True)
    m = m.to(DEV).train(True)
    v = pkg.synth.make_video(1, 8, 64, 64, seed=502).to(DEV)

    def run():
        with torch.no_grad():
            f0 = m._runner.run(m.resnet, v, features=True)[0].clone()
        m.zero_grad(set_to_none=True)
        f = m._runner.run(m.resnet, v, features=True)[0]
        assert f.requires_grad
        f.backward(_rand(*f.shape, seed=9).to(DEV))
        torch.cuda.synchronize()
        return f0, f.detach().clone(), {n: q.grad.clone() for n, q in m.named_parameters() if q.grad is not None}

    ref = run()
    _exact_buffers(pkg, monkeypatch, arena)
    monkeypatch.setattr(pkg.modelling.resnet3d, "torch", _TorchWithExactTape(arena))
    arena.reset()
    got = run()
    arena.check()
    assert len(arena.operands) >= 4  # workspace (twice), tape, backward workspace
    assert torch.equal(got[0], ref[0]) and torch.equal(got[1], ref[1]) and got[2].keys() == ref[2].keys() and len(got[2]) >= 53
    for n in ref[2]:
        assert torch.equal(got[2][n], ref[2][n]), n
