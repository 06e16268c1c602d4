"""The GEMM and Conv3d products off the unit scale, block by block against torch's own fp32 error and an in-order fp32 chain.

The GEMM tests beside this one draw unit-scale inputs and hold one max-abs bar over the whole output, where an output row, column group
or channel that is small beside its neighbours (a bias-dominated projection, a zero-initialised BatchNorm gamma, a gradient accumulated
into a much larger buffer) is compared at the neighbours' scale and a wrong epilogue on it passes.  Here every case comes from
tests/product_cases.py (whose docstring states blocks, groups and the two yardsticks; tests/test_product_scale_cpu.py holds the cases
to their conditions and shows on an emulation that the bar can fail), and every route a product can take runs on them: the whole-tile
kernel, its stream-K form and fix-up, the small-tile kernel at each tile height, the skinny split-k pair, the compatibility kernel, the
backward layouts with their add-sources, the split contraction with its slab reduction, the grouped weight gradient, the input gradient
on small tiles, the opt-in split-bf16 build, and the Conv3d forward with BatchNorm, residual and ReLU.  Each GEMM route proves through
the launch recorder that it ran (the notes of the launchers); stlt_conv3d_fwd records no launch, its split route is proven by the split
count its workspace size implies, as tests/test_r3d_gpu.py does.  Every case prints the [scale] lines of scale_cases.judge
(profiles/product_scale.md keeps the table of one run).

No route needed an analytic term: every case holds the plain bar 4 * max(E_t, E_c, u).  The whole-tile kernels add the bias from an LDS
strip behind a tile's last k-step; test_bias_strip_of_every_tile_under_load holds that schedule where tiles are shortest.
"""
import ctypes

import pytest
import torch

import product_cases as P
import scale_cases as SC
import test_r3d_gpu as R3

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _recorded(pkg, fn):
    """fn() with the launch recorder on -> (fn's result, the notes of the launches it made)."""
    pkg.ops.prof_enable(True)
    try:
        pkg.ops.prof_launches()
        out = fn()
        torch.cuda.synchronize()
        notes = [r["note"] for r in pkg.ops.prof_launches()]
    finally:
        pkg.ops.prof_enable(False)
    return out, notes


def _cut(notes, head, *needles):
    """The first note that holds `head`; it must hold every needle too."""
    hits = [n for n in notes if head in n]
    assert hits, (head, notes)
    for k in needles:
        assert k in hits[0], (k, hits[0])
    return hits[0]


def _hold(tag, got, case, name="y", term=None):
    fails = SC.judge(tag, got, case["outs"][name], term=term)[1]
    assert not fails, "\n".join(fails[:40]) + f"\n({len(fails)} blocks over the bar)"


def _ceil(a, b):
    return -(-a // b)


def _dev(case, *keys):
    return [None if case[k] is None else case[k].to(DEV) for k in keys]


@pytest.fixture()
def no_small_tiles(pkg):
    pkg.ops.set_gemm_small_tiles(0)
    try:
        yield
    finally:
        pkg.ops.set_gemm_small_tiles(-2)


FWD = [(K, act, kind) for K in P.K_STEPS for act, kind in ((P.ACT_NONE, "full"), (P.ACT_RELU, "full"), (P.ACT_GELU, "gelu"))]


# ---- ops.linear: the 256 x 128 kernel on whole tiles, and its stream-K form -----------------------------------------------------------
@pytest.mark.parametrize("K,act,kind", FWD)
def test_linear_whole_tiles(pkg, no_small_tiles, K, act, kind):
    """M = 260: a second row tile of 4 rows; N = 320 / 384: a ragged third column tile.  No scratch lent: whole tiles, split=1."""
    case = P.linear_case(P.M_MAIN, K, act, False, True, kind)
    x, w, b = _dev(case, "x", "w", "bias")
    y, notes = _recorded(pkg, lambda: pkg.ops.linear(x, w, b, act))
    note = _cut(notes, "gemm M=", "tile=256x128", "split=1", f"K={K} ", f"act={act}")
    assert "stream-K" not in note and len(notes) == 1, notes
    _hold(f"linear whole tiles K={K} act={act}", y, case)


@pytest.mark.parametrize("K,act,kind", FWD)
def test_linear_stream_k(pkg, no_small_tiles, K, act, kind):
    """The same call with scratch lent: 4 - 6 tiles on the whole chip, partial segments summed, bias / activation applied by the fix-up."""
    case = P.linear_case(P.M_MAIN, K, act, False, True, kind)
    x, w, b = _dev(case, "x", "w", "bias")
    with pkg.ops.gemm_scratch():
        y, notes = _recorded(pkg, lambda: pkg.ops.linear(x, w, b, act))
    _cut(notes, "gemm M=", "tile=256x128", "stream-K", "(+fix-up)", f"K={K} ")
    _hold(f"linear stream-K K={K} act={act}", y, case)


@pytest.mark.parametrize("K,split_bf16", [(32, False), (64, False), (64, True)])
def test_bias_strip_of_every_tile_under_load(pkg, no_small_tiles, K, split_bf16):
    """The bias joins a tile's sums behind its last k-step, from an LDS strip that the loaders rewrite for later tiles while the workgroup
    walks on: three or more short tiles per workgroup (K = 32: one k-step a tile, the tightest schedule; the split-bf16 build needs two),
    three column tiles with their own large bias each.  A strip read too late is another column tile's bias, far outside the bar (2e-5 of
    the output's scale, the whole-output bar of the neighbouring GEMM tests: this case is about the schedule, not the rounding)."""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    M, N = 256 * (cus + 1), 384
    g = SC._gen("bias strip", K)
    x, w = torch.randn(M, K, generator=g), torch.randn(N, K, generator=g) / K ** 0.5
    b = 10.0 * torch.arange(1, N + 1, dtype=torch.float32) * (1 - 2 * (torch.arange(N) % 2))
    if split_bf16:
        pkg.ops.set_gemm_split_bf16(6)
    try:
        y, notes = _recorded(pkg, lambda: pkg.ops.linear(x.to(DEV), w.to(DEV), b.to(DEV)))
    finally:
        pkg.ops.set_gemm_split_bf16(0)
    note = _cut(notes, "gemm(split-bf16)" if split_bf16 else "gemm M=", "tile=256x128", f"tiles={3 * (cus + 1)}")
    assert split_bf16 or "rounds=4 " in note, note
    ref = x.double() @ w.double().T + b.double()
    err = (y.cpu().double() - ref).abs().max().item() / ref.abs().max().item()
    print(f"[scale] bias strips under load K={K} split_bf16={int(split_bf16)}: {err:.3e} of the output's scale (bar 2e-5)")
    assert err <= 2e-5, err


# ---- ops.linear_small: one tile of each height ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_res", [False, True])
@pytest.mark.parametrize("tile_rows,tile_cols", [(128, 64), (64, 64), (32, 128)])
@pytest.mark.parametrize("K", P.K_STEPS)
def test_linear_small_tiles(pkg, K, tile_rows, tile_cols, with_res):
    """260 rows: whole tiles and a ragged last one at every height; with the bias alone and with bias + residual."""
    case = P.linear_case(P.M_MAIN, K, P.ACT_NONE, with_res, True, "full")
    x, w, b, r = _dev(case, "x", "w", "bias", "res")
    y, notes = _recorded(pkg, lambda: pkg.ops.linear_small(x, w, b, tile_cols, residual=r, tile_rows=tile_rows))
    _cut(notes, "gemm16 M=", f"tile={tile_rows}x{tile_cols} ", f"K={K} ", "act=0+R" if with_res else "act=0 ")
    _hold(f"linear_small {tile_rows}x{tile_cols} K={K} res={int(with_res)}", y, case)


@pytest.mark.parametrize("K", P.K_STEPS)
def test_linear_small_relu(pkg, K):
    """The small-tile kernel's ReLU epilogue: the -30 regime must come out as exact zeros."""
    case = P.linear_case(P.M_MAIN, K, P.ACT_RELU)
    x, w, b = _dev(case, "x", "w", "bias")
    y, notes = _recorded(pkg, lambda: pkg.ops.linear_small(x, w, b, 128, act=P.ACT_RELU, tile_rows=64))
    _cut(notes, "gemm16 M=", "tile=64x128 ", "act=2")
    _hold(f"linear_small 64x128 relu K={K}", y, case)


# ---- a few rows: split-k partial tiles + finish ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", P.K_STEPS)
def test_linear_skinny_split_k(pkg, K):
    """M = 8 through ops.linear, which lends the scratch itself."""
    case = P.linear_case(P.M_SKINNY, K)
    x, w, b = _dev(case, "x", "w", "bias")
    y, notes = _recorded(pkg, lambda: pkg.ops.linear(x, w, b))
    _cut(notes, "gemm(skinny)", "(+finish)", f"K={K} ", "splits=")
    _hold(f"linear skinny K={K}", y, case)


# ---- K = 100: the compatibility kernel ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("act", [P.ACT_NONE, P.ACT_RELU])
def test_linear_compatibility_kernel(pkg, act):
    case = P.linear_case(P.M_MAIN, P.K_ANY, act)
    x, w, b = _dev(case, "x", "w", "bias")
    y, notes = _recorded(pkg, lambda: pkg.ops.linear(x, w, b, act))
    _cut(notes, "gemm(any)", f"K={P.K_ANY} ", "tile=64x64")
    _hold(f"linear compatibility kernel K={P.K_ANY} act={act}", y, case)


# ---- backward layouts -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("stream_k", [False, True])
@pytest.mark.parametrize("K", P.K_STEPS)
def test_input_gradient_layout_with_add_source(pkg, K, stream_k):
    """dX = dY · W + R through ops.gemm(trans_b=True, add=R), R at 1e3 x and 1e-3 x the product's scale; whole tiles and stream-K."""
    case = P.linear_case(P.M_MAIN, K, P.ACT_NONE, True, False, "full")
    dy, wt, r = _dev(case, "x", "w", "res")
    w_kn = wt.T.contiguous()
    if stream_k:
        with pkg.ops.gemm_scratch():
            y, notes = _recorded(pkg, lambda: pkg.ops.gemm(dy, w_kn, trans_b=True, add=r))
        _cut(notes, "gemm(dX)", "+R", "stream-K", "(+fix-up)")
    else:
        y, notes = _recorded(pkg, lambda: pkg.ops.gemm(dy, w_kn, trans_b=True, add=r))
        assert "stream-K" not in _cut(notes, "gemm(dX)", "+R", "tile=256x128", "split=1")
    _hold(f"gemm dX + R K={K} stream_k={int(stream_k)}", y, case)


@pytest.mark.parametrize("tile_cols", [64, 0])
@pytest.mark.parametrize("K", P.K_STEPS)
def test_input_grad_small(pkg, K, tile_cols):
    """The same product on the small-tile kernel, W read as it lies: on the 128 x 64 tile, and routed by the estimate (tile_cols = 0, the
    routing set to `always` so that the estimate only picks the tile)."""
    case = P.linear_case(P.M_MAIN, K, P.ACT_NONE, True, False, "full")
    dy, wt, r = _dev(case, "x", "w", "res")
    w_kn = wt.T.contiguous()
    if tile_cols == 0:
        pkg.ops.set_gemm_small_tiles(1)
    try:
        y, notes = _recorded(pkg, lambda: pkg.ops.input_grad_small(dy, w_kn, tile_cols, residual=r))
    finally:
        pkg.ops.set_gemm_small_tiles(-2)
    note = _cut(notes, "gemm16(dX,W as it lies)", "+R", f"K={K} ")
    assert tile_cols == 0 or "tile=128x64 " in note, note
    _hold(f"input_grad_small tile_cols={tile_cols} K={K}", y, case)


@pytest.mark.parametrize("rows", P.DW_ROWS)
def test_weight_gradient_layout_with_add_source(pkg, rows):
    """dW = dYᵀ · X + G0 through ops.gemm(trans_a=True, trans_b=True, add=G0): 96 rows take the compatibility kernel's whole 64 x 64
    tiles, 2048 the large kernel; G0 at 1e3 x and 1e-3 x the update."""
    case = P.weight_grad_case(rows)
    dy, x, g0 = _dev(case, "dy", "x", "g0")
    y, notes = _recorded(pkg, lambda: pkg.ops.gemm(dy, x, trans_a=True, trans_b=True, add=g0))
    if rows <= 128:
        _cut(notes, "gemm(any, dW)", f"K={rows} ", "+R")
    else:
        assert "stream-K" not in _cut(notes, "gemm(dW)", f"K={rows} ", "+R", "tile=256x128", "split=1")
    _hold(f"gemm dW + G0 rows={rows}", y, case, "dW")


def test_weight_gradient_stream_k_split_and_group(pkg):
    """The 2048-row weight gradient on the other routes: stream-K + fix-up, n_split = 4 + stlt_reduce_slabs (accumulating into G0), and
    ops.weight_grad_group (g_w += ..., one grouped stream-K launch) together with the 96-row product."""
    case = P.weight_grad_case(2048)
    dy, x, g0 = _dev(case, "dy", "x", "g0")
    with pkg.ops.gemm_scratch():
        y, notes = _recorded(pkg, lambda: pkg.ops.gemm(dy, x, trans_a=True, trans_b=True, add=g0))
    _cut(notes, "gemm(dW)", "+R", "stream-K", "(+fix-up)")
    _hold("gemm dW + G0 stream-K rows=2048", y, case, "dW")
    y, notes = _recorded(pkg, lambda: pkg.ops.gemm(dy, x, trans_a=True, trans_b=True, add=g0, n_split=4))
    _cut(notes, "gemm(dW)", "split=4")
    _cut(notes, "reduce n=", "slabs=4")
    _hold("gemm dW n_split=4 + reduce_slabs rows=2048", y, case, "dW")
    small = P.weight_grad_case(96)
    dy2, x2, g2 = _dev(small, "dy", "x", "g0")
    gw, gw2 = g0.clone(), g2.clone()
    with pkg.ops.gemm_scratch():
        _, notes = _recorded(pkg, lambda: pkg.ops.weight_grad_group([(dy, x, gw), (dy2, x2, gw2)]))
    _cut(notes, "gemm(dW group)", "products=2", "stream-K", "(+fix-up)")
    _hold("weight_grad_group rows=2048", gw, case, "dW")
    _hold("weight_grad_group rows=96", gw2, small, "dW")


# ---- the opt-in split-bf16 build ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K,act", [(64, P.ACT_NONE), (768, P.ACT_NONE), (768, P.ACT_RELU), (3072, P.ACT_NONE)])
def test_linear_split_bf16(pkg, K, act):
    """stlt_set_gemm_split_bf16(6): the header calls its results f32-equivalent, so it is held to the plain bar.  The kernel takes launches
    whose whole tiles fill half the chip: the 260 rows of the case are repeated (row i of the launch is row i % 260 of the case, the four
    x scales stay interleaved) until they do, and every block of every repetition is compared."""
    case = P.linear_case(P.M_MAIN, K, act)
    x, w, b = _dev(case, "x", "w", "bias")
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    tiles_n = _ceil(w.shape[0], 128)
    reps = _ceil((_ceil(_ceil(cus, 2), tiles_n) + 1) * 256, P.M_MAIN)   # row tiles x column tiles >= half the compute units
    xr = x.repeat(reps, 1)
    pkg.ops.set_gemm_split_bf16(6)
    try:
        y, notes = _recorded(pkg, lambda: pkg.ops.linear(xr, w, b, act))
    finally:
        pkg.ops.set_gemm_split_bf16(0)
    _cut(notes, "gemm(split-bf16)", f"K={K} ", f"M={xr.shape[0]} ")
    assert len(notes) == 1, notes
    y = y.reshape(reps, P.M_MAIN, -1)
    worst = (y - y[0]).abs().amax(0)   # the repetition that strays furthest from the first one is judged as well
    far = torch.gather(y, 0, (y - y[0]).abs().argmax(0, keepdim=True))[0]
    print(f"[scale] split-bf16 K={K} act={act}: {reps} repetitions, largest difference between repetitions {float(worst.max()):.3e}")
    _hold(f"linear split-bf16 K={K} act={act} (first repetition)", y[0], case)
    _hold(f"linear split-bf16 K={K} act={act} (per element the repetition furthest from the first)", far, case)


# ---- Conv3d + BatchNorm + residual + ReLU ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(P.CONV_SHAPES))
def test_conv3d_channel_regimes(pkg, name):
    """One output channel of one sample is a block, the channel's BatchNorm regime the group (BN scale 1e-3 / 1 / 1e3 through running_var,
    negative gamma, gamma exactly 0, |beta| = 30, and beta = -30 whose ReLU output is identically zero); channel c has regime c % 7, so
    every tile mixes them."""
    assert P.CONV_SHAPES[name] == R3.CASES[name]
    case = P.conv_case(name)
    B, Ci, T, H, W, Co, k, s, p, with_res, relu, n_split = case["shape"]
    if n_split > 1:  # the split route: the workspace holds one M x c_out slab per split
        d = pkg._lib.Conv3dDesc(B, T, H, W, Ci, Co, *k, *s, *p)
        M = B * case["outs"]["y"].ref.shape[1]
        assert int(pkg._lib.load().stlt_conv3d_workspace_bytes(ctypes.byref(d), n_split)) == R3.PLANNED_SPLITS[name] * M * Co * 4
    res = None if case["res"] is None else case["res"].permute(0, 2, 3, 4, 1).contiguous().to(R3.DEV)
    y = R3._conv(pkg, R3._to_ndhwc(pkg, case["x"], Ci), R3._repack(pkg, case["w"], Ci), Co, k, s, p, bn=[t.to(R3.DEV) for t in case["bn"]], res=res,
                 relu=relu, n_split=n_split)
    _hold(f"conv3d {name}", y.permute(0, 4, 1, 2, 3).contiguous(), case)
