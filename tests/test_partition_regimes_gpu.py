"""The partitioned reduction kernels on both sides of every split of their launchers.

Every backward / reduction kernel outside the GEMMs cuts its rows into a capped number of parts, lets a block or a persistent wave
walk its part, and adds the partial rows in a fixed order.  The cut changes shape at fixed counts (one row per wave -> several with the
next row prefetched -> a capped grid with ragged or empty trailing parts).  The cases below are the smallest counts on both sides of
each such count, at unit scale (tests/test_off_unit_scale_gpu.py takes the same kernels off it, row by row against torch's own
fp32 error; the GEMMs and the Conv3d forward, on every route they can take: tests/test_product_scale_gpu.py, profiles/product_scale.md), against plain fp64 references on the CPU, with the bars of the neighbouring op-level tests:
2e-5 of each result's max-abs scale (5e-5 for the column sums of the attention gradient, loss 2e-6 * max(1, |ref|), loss gradient
1e-7, norm 1e-5 relative, reduce_slabs the element-wise bound of test_reduce_slabs).

Each case also proves that it ran the regime it names: the launchers report their cut through the launch recorder (stlt_prof_note,
read back with ops.prof_enable / ops.prof_launches) and the case asserts the cut and the fact that makes it a boundary case
("blocks == 512 and M > 16 * blocks", "an entire trailing part is empty", "items > chunks").  A launcher whose constants move makes
these assertions fail instead of silently turning the case into a small-side one.  Every case prints its largest error.
"""
import math
import os
import re

import pytest
import torch

import partition_refs as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
EPS24 = 2.0 ** -24


def _rand(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(*shape, generator=g) * 2 - 1) * scale


@pytest.fixture(scope="module")
def lib(pkg):
    return pkg._lib.load()


def _stream():
    return torch.cuda.current_stream().cuda_stream


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


def _cut(notes, head, *keys):
    """The integers behind `key=` in the first note that holds `head`."""
    hits = [n for n in notes if head in n]
    assert hits, (head, notes)
    out = []
    for k in keys:
        m = re.search(rf"(?<![\w/]){re.escape(k)}=(-?\d+)", hits[0])
        assert m, (k, hits[0])
        out.append(int(m.group(1)))
    return out[0] if len(out) == 1 else out


def _ceil(a, b):
    return -(-a // b)


def _rel(got, ref):
    return (got.detach().cpu().double() - ref).abs().max().item() / max(ref.abs().max().item(), 1e-6)


def _check(what, got, ref, bar=2e-5):
    err = _rel(got, ref)
    print(f"[partition] {what}: {err:.3e} of scale (bar {bar:.0e})")
    assert math.isfinite(err) and err <= bar, (what, err)


def _check_sum(what, got, ref, mag, k, bar=2e-5):
    """A result that only sums k fp32 terms: the bar, with the share of the a-priori bound k * 2^-24 * sum|terms| * 1.01 printed beside it."""
    err = (got.detach().cpu().double() - ref).abs()
    share = (err / (k * EPS24 * 1.01 * mag).clamp_min(1e-300)).max().item()
    rel = err.max().item() / max(ref.abs().max().item(), 1e-6)
    print(f"[partition] {what}: {rel:.3e} of scale (bar {bar:.0e}); {share:.3e} of the a-priori bound of a {k}-term sum")
    assert math.isfinite(rel) and rel <= bar, (what, rel, share)


# ---- stlt_add_layernorm_bwd -----------------------------------------------------------------------------------------------------
LN_M = [2048, 2049, 2064, 8192, 8193, 8200]
LN_D = [64, 260, 768, 1024, 1028, 2048]
LN_CASES = sorted({(M, d) for M in LN_M for d in (64, 768)} | {(M, d) for M in (2049, 8200) for d in LN_D})
LN_CUT = {2048: (512, 1), 2049: (129, 4), 2064: (129, 4), 8192: (512, 4), 8193: (512, 5), 8200: (512, 5)}  # blocks, most rows of one wave


@pytest.mark.parametrize("M,d", LN_CASES)
def test_add_layernorm_bwd_rows_per_wave_regimes(pkg, lib, M, d):
    """launch_ln_bwd: up to 2048 rows a wave per row (2048: the last such count); from 2049 four rows per wave (129 blocks: the last
    waves hold three rows at 2049, 2064 is exact); 8192 fills 512 blocks x 4 waves x 4 rows; from 8193 the cap binds and some waves
    walk a fifth row.  d = 64 .. 1024: one to four vector groups in registers (260: a second group of one lane; 260 and 1028 are no
    multiples of 16, so the three partial-row sums are reduced per destination); 1028 and 2048: the wide kernel (accumulators in LDS).
    With and without the residual; ds, and g_w / g_b accumulated into non-zero starting values."""
    x, r, g = _rand(M, d, seed=1), _rand(M, d, seed=2), _rand(M, d, seed=3)
    w, gw0, gb0 = 1 + _rand(d, seed=4, scale=0.1), _rand(d, seed=5), _rand(d, seed=6)
    xd, rd, gd, wd = x.to(DEV), r.to(DEV), g.to(DEV), w.to(DEV)
    nbytes = int(lib.stlt_add_layernorm_bwd_scratch_bytes(d))
    sc = pkg.ops._scratch(nbytes, torch.device(DEV, torch.cuda.current_device()))
    rpw_env = int(os.environ.get("STLT_LN_BWD_ROWS_PER_WAVE", "0") or 0)
    for with_res in (True, False):
        ds, gw, gb = torch.empty(M, d, device=DEV), gw0.to(DEV), gb0.to(DEV)
        _, notes = _recorded(pkg, lambda: pkg._lib.check(lib.stlt_add_layernorm_bwd(
            gd.data_ptr(), xd.data_ptr(), rd.data_ptr() if with_res else None, wd.data_ptr(), 1e-5, M, d, ds.data_ptr(), gw.data_ptr(), gb.data_ptr(),
            sc.data_ptr(), nbytes, _stream()), "stlt_add_layernorm_bwd"))
        rows, dd, blocks = _cut(notes, "ln_bwd", "rows", "d", "blocks")
        assert (rows, dd) == (M, d)
        note = [n for n in notes if "ln_bwd" in n][0]
        assert ("wide" in note) == (d > 1024) and ("reduce n=%d " % d in note) == (d % 16 != 0), note
        if rpw_env <= 0:
            waves = 4 * blocks
            assert (blocks, _ceil(M, waves)) == LN_CUT[M], note
            if M == 2048:
                assert M == waves                     # every wave has exactly one row: no second trip, no prefetch
            elif M in (2049, 2064):
                assert blocks < 512 and M > waves and (M % waves != 0) == (M == 2049)  # the loop runs; at 2049 the last waves hold a row less
            elif M == 8192:
                assert blocks == 512 and M == 4 * waves
            else:
                assert blocks == 512 and M > 16 * blocks  # the cap binds: M - 8192 waves walk a fifth row
        s64, w64 = ((x + r) if with_res else x).double().requires_grad_(True), w.double().requires_grad_(True)
        b64 = torch.zeros(d, dtype=torch.float64, requires_grad=True)
        torch.nn.functional.layer_norm(s64, (d,), w64, b64, 1e-5).backward(g.double())
        tag = f"ln_bwd M={M} d={d} res={int(with_res)}"
        _check(tag + " ds", ds, s64.grad)
        _check(tag + " g_w", gw, gw0.double() + w64.grad)
        _check(tag + " g_b", gb, gb0.double() + b64.grad)


# ---- column sums through stlt_linear_bwd (db) -----------------------------------------------------------------------------------
COLSUM_CUT = {1: (1, 1, 0), 15: (1, 15, 0), 16: (1, 16, 0), 17: (2, 9, 0), 1024: (64, 16, 0), 1025: (64, 17, 3), 1040: (64, 17, 2),
              1100: (64, 18, 2)}  # parts, rows per part, wholly empty trailing parts


@pytest.mark.parametrize("N", [4, 132, 260])
@pytest.mark.parametrize("M", sorted(COLSUM_CUT))
def test_linear_bwd_bias_gradient_parts(pkg, lib, M, N):
    """launch_colsum_acc: ceil(M / 16) parts, at most 64.  16 / 17: one part -> two; 1024: 64 exact parts; 1025: 17-row parts whose last
    three are empty (they must write zeros); N = 4 / 132 / 260: one column block, and a second one of 4 columns.  db accumulates."""
    K = 64
    x, w, dy, db0 = _rand(M, K, seed=M), _rand(N, K, seed=N), _rand(M, N, seed=M + N), _rand(N, seed=7)
    xd, wd, dyd, db = x.to(DEV), w.to(DEV), dy.to(DEV), db0.to(DEV)
    nbytes = int(lib.stlt_linear_bwd_scratch_bytes(N))
    sc = pkg.ops._scratch(nbytes, torch.device(DEV, torch.cuda.current_device()))
    _, notes = _recorded(pkg, lambda: pkg._lib.check(lib.stlt_linear_bwd(xd.data_ptr(), wd.data_ptr(), dyd.data_ptr(), M, N, K, None, None, db.data_ptr(), None,
                                                                         sc.data_ptr(), nbytes, _stream()), "stlt_linear_bwd"))
    rows, cols, parts, per = _cut(notes, "colsum", "rows", "cols", "parts", "rows/part")
    assert (rows, cols) == (M, N)
    assert (parts, per, parts - _ceil(M, per)) == COLSUM_CUT[M], notes
    assert parts * per >= M and (parts - 1 - COLSUM_CUT[M][2]) * per < M
    if M == 1025:
        assert parts * per > M and (parts - 1) * per >= M  # an entire trailing part is empty
    _check_sum(f"colsum M={M} N={N} db", db, db0.double() + dy.double().sum(0), db0.double().abs() + dy.double().abs().sum(0), M + 1)


# ---- stlt_embed_bwd --------------------------------------------------------------------------------------------------------------
EMBED_CUT = {1: (1, 1), 32: (1, 32), 33: (2, 17), 511: (16, 32), 16384: (512, 32), 16385: (512, 33), 16400: (512, 33)}  # blocks, tokens per block
EMBED_CASES = ([(n, 64, 38, True) for n in sorted(EMBED_CUT)] + [(33, 64, 38, False), (16385, 64, 38, False)]
               + [(33, 260, 2, False), (16400, 260, 2, True), (32, 768, 2, True), (16400, 768, 2, False)]
               + [(511, 260, 49, False), (16400, 260, 49, True), (1, 260, 128, False), (511, 64, 128, True), (16400, 260, 128, False)])


def _embed_case(pkg, lib, n, d, C, with_scores, cats, tag):
    g0 = torch.Generator().manual_seed(n + d + C)
    boxes, scores, d_pre = torch.rand(n, 4, generator=g0), (torch.rand(n, generator=g0) if with_scores else None), _rand(n, d, seed=n + 1)
    ref, mag = R.embed_param_grads(d_pre, cats, boxes, scores, C)
    shapes = {"g_cat": (C, d), "g_box_w": (d, 4), "g_box_b": (d,), "g_score_w": (d, 1), "g_score_b": (d,)}
    names = list(ref)
    dev = {"d_pre": d_pre.to(DEV), "cats": cats.to(DEV), "boxes": boxes.to(DEV), "scores": scores.to(DEV) if with_scores else None}
    nbytes = int(lib.stlt_embed_bwd_scratch_bytes(n, C, d))
    sc = pkg.ops._scratch(nbytes, torch.device(DEV, torch.cuda.current_device()))
    p = pkg.ops._p

    def call(out):
        return pkg._lib.check(lib.stlt_embed_bwd(p(dev["d_pre"]), p(dev["cats"]), p(dev["boxes"]), p(dev["scores"]), C, n, d, p(out["g_cat"]), p(out["g_box_w"]),
                                                 p(out["g_box_b"]), p(out.get("g_score_w")), p(out.get("g_score_b")), sc.data_ptr(), nbytes, _stream()), "stlt_embed_bwd")

    zero = {k: torch.zeros(shapes[k], device=DEV) for k in names}
    _, notes = _recorded(pkg, lambda: call(zero))
    tokens, dd, CC, blocks, tpb, slices, lds = _cut(notes, "embed_bwd", "tokens", "d", "C", "blocks", "tok/block", "slices", "lds")
    assert (tokens, dd, CC) == (n, d, C) and (blocks, tpb) == EMBED_CUT[n] and slices == _ceil(d, 256) and lds == C * 1024, notes
    assert blocks * tpb >= n and (n == 1 or blocks * (tpb - 1) < n)
    if n == 16400:
        assert blocks == 512 and _ceil(n, tpb) < blocks  # the last blocks hold no token: their partial rows must be zeros
    if n == 16384:
        assert blocks * tpb == n
    if C in (49, 128):
        assert lds > 48 * 1024  # the dynamic-LDS opt-in
    if d in (260, 768):
        assert slices > 1 and (d % 256 != 0) == (d == 260)  # a second channel slice, partly filled at 260
    start = {k: _rand(*shapes[k], seed=11 + i) for i, k in enumerate(names)}
    acc = {k: v.to(DEV) for k, v in start.items()}
    call(acc)
    named = torch.zeros(C, dtype=torch.bool)
    named[cats.unique()] = True
    named[0] = False  # the padding index
    for k in names:
        _check_sum(f"{tag} {k}", zero[k], ref[k], mag[k], n)
        _check_sum(f"{tag} {k} accumulated", acc[k], start[k].double() + ref[k], start[k].double().abs() + mag[k], n + 1)
    assert zero["g_cat"][~named.to(DEV)].abs().max().item() == 0.0                      # row 0 and the rows no token names: exactly zero
    assert torch.equal(acc["g_cat"][~named.to(DEV)].cpu(), start["g_cat"][~named])      # ... and left as they were when accumulating
    return named


@pytest.mark.parametrize("n,d,C,with_scores", EMBED_CASES)
def test_embed_bwd_token_blocks_slices_and_category_counts(pkg, lib, n, d, C, with_scores):
    """launch_embed_bwd: ceil(n / 32) blocks, at most 512, of ceil(n / blocks) tokens: 32 / 33 one block -> two, 16384 fills 512 blocks of 32,
    16385 / 16400 make them 33 and leave the last blocks empty; d = 260 / 768: further 256-channel slices (260: four channels in the
    second); C x 1 KB of dynamic LDS, opted in above 48 KB (C = 49, 128 = the limit).  The finalize pass sums every 16th block partial
    per lane.  No token names category C - 1 (C > 2), tokens name the padding index 0."""
    g0 = torch.Generator().manual_seed(n * 7 + C)
    cats = torch.randint(0, max(C - 1, 2), (n,), generator=g0)
    named = _embed_case(pkg, lib, n, d, C, with_scores, cats, f"embed_bwd n={n} d={d} C={C} scores={int(with_scores)}")
    if C > 2:
        assert not named[C - 1]


def test_embed_bwd_every_token_in_one_category(pkg, lib):
    n, d, C = 16400, 64, 38
    named = _embed_case(pkg, lib, n, d, C, True, torch.full((n,), 5), "embed_bwd one category")
    assert named.sum().item() == 1 and named[5]


def test_embed_bwd_refuses_more_categories_than_the_lds_holds(pkg, lib):
    n, d, C = 33, 64, 129
    nbytes = int(lib.stlt_embed_bwd_scratch_bytes(n, C, d))
    sc = torch.zeros(nbytes // 4, device=DEV)
    g_cat = torch.zeros(C, d, device=DEV)
    rc = lib.stlt_embed_bwd(torch.zeros(n, d, device=DEV).data_ptr(), torch.zeros(n, dtype=torch.int64, device=DEV).data_ptr(), torch.zeros(n, 4, device=DEV).data_ptr(), None,
                            C, n, d, g_cat.data_ptr(), None, None, None, None, sc.data_ptr(), nbytes, _stream())
    assert rc != 0 and "at most 128 categories" in lib.stlt_last_error().decode()
    torch.cuda.synchronize()
    assert g_cat.abs().max().item() == 0.0


# ---- stlt_frames_embed_bwd -------------------------------------------------------------------------------------------------------
FRAMES_CUT = {1: (1, 1, 0), 15: (15, 1, 0), 16: (16, 1, 0), 17: (16, 2, 7), 33: (16, 3, 5)}  # chunks, clips per chunk, empty chunks


@pytest.mark.parametrize("B", sorted(FRAMES_CUT))
def test_frames_embed_bwd_clip_chunks(pkg, lib, B):
    """launch_frames_bwd: min(B, 16) clip chunks of ceil(B / chunks) clips: 16 -> 17 doubles the clips of a chunk and leaves seven chunks
    empty.  T = 1 / 6 / 65 position rows, d = 64 / 260 (a second column block of four channels).  Frame type 0 (the padding index: no
    gradient) and all of 1 .. 4 occur, one clip is entirely type 0.  Gradients accumulate."""
    dev = torch.device(DEV, torch.cuda.current_device())
    for T in (1, 6, 65):
        for d in (64, 260):
            g0 = torch.Generator().manual_seed(B * 100 + T)
            ft = torch.randint(0, 5, (B, T), generator=g0)
            if B > 1:
                ft[B // 2, :] = 0
            if B * T >= 10:
                ft.view(-1)[:5] = torch.arange(5)
            d_pre = _rand(B, T, d, seed=B + T + d)
            ref, mag = R.frames_param_grads(d_pre, ft)
            start = {"g_pos": _rand(T, d, seed=1), "g_type": _rand(5, d, seed=2)}
            out = {k: v.to(DEV) for k, v in start.items()}
            dd, fd = d_pre.to(DEV), ft.to(DEV)
            nbytes = int(lib.stlt_frames_embed_bwd_scratch_bytes(T, d))
            sc = pkg.ops._scratch(nbytes, dev)
            _, notes = _recorded(pkg, lambda: pkg._lib.check(lib.stlt_frames_embed_bwd(dd.data_ptr(), fd.data_ptr(), B, T, d, out["g_pos"].data_ptr(),
                                                                                       out["g_type"].data_ptr(), sc.data_ptr(), nbytes, _stream()), "stlt_frames_embed_bwd"))
            nB, nT, nd, chunks, per = _cut(notes, "frames_bwd", "B", "T", "d", "chunks", "clips/chunk")
            assert (nB, nT, nd) == (B, T, d) and (chunks, per, chunks - _ceil(B, per)) == FRAMES_CUT[B], notes
            if B == 17:
                assert per == 2 and chunks * per > B and (chunks - 1) * per >= B  # whole chunks without a clip
            for k in ("g_pos", "g_type"):
                _check_sum(f"frames_bwd B={B} T={T} d={d} {k}", out[k], start[k].double() + ref[k], start[k].double().abs() + mag[k], B * T + 1)
            assert torch.equal(out["g_type"][0].cpu(), start["g_type"][0])  # the padding type's row is left as it was


# ---- stlt_loss_fwd_bwd -----------------------------------------------------------------------------------------------------------
LOSS_SHAPES = [(1, 1), (3, 256), (3, 257), (5, 1000), (256, 7), (257, 7), (300, 513)]


def _loss_call(pkg, lib, logits, labels, kind, weight):
    B, K = logits.shape
    ld, yd = logits.to(DEV), labels.to(DEV)
    sc, loss, dl = torch.empty(B, device=DEV), torch.empty(1, device=DEV), torch.empty(B, K, device=DEV)
    _, notes = _recorded(pkg, lambda: pkg._lib.check(lib.stlt_loss_fwd_bwd(ld.data_ptr(), yd.data_ptr(), kind, B, K, weight, sc.data_ptr(), loss.data_ptr(), dl.data_ptr(),
                                                                           _stream()), "stlt_loss_fwd_bwd"))
    nk, nB, nK, blocks, class_trips, clip_trips = _cut(notes, "loss kind", "kind", "B", "K", "blocks", "class_trips", "clip_trips")
    assert (nk, nB, nK, blocks) == (kind, B, K, B) and class_trips == _ceil(K, 256) and clip_trips == _ceil(B, 256), notes
    assert (class_trips > 1) == (K > 256) and (clip_trips > 1) == (B > 256)  # 256 -> 257: the class loop / the clip loop takes a second trip
    return loss.cpu(), dl.cpu()


def _loss_check(tag, loss, dl, ref, ref_grad):
    err_l, err_g = abs(loss.item() - ref.item()), (dl.double() - ref_grad).abs().max().item()
    print(f"[partition] {tag}: loss {err_l:.3e} (bar {2e-6 * max(1.0, abs(ref.item())):.1e}), gradient {err_g:.3e} (bar 1e-07)")
    assert err_l <= 2e-6 * max(1.0, abs(ref.item())) and err_g <= 1e-7, (tag, err_l, err_g)


@pytest.mark.parametrize("weight", [1.0, 0.5])
@pytest.mark.parametrize("B,K", LOSS_SHAPES)
@pytest.mark.parametrize("kind", [0, 1])
def test_loss_class_and_clip_loops(pkg, lib, kind, B, K, weight):
    """loss_rows_kernel walks a clip's classes 256 at a time (K = 256 -> 257, 1000: four trips, 513: a third trip of one class),
    loss_finish_kernel the clips 256 at a time (B = 256 -> 257).  Cross entropy (kind 0) and BCE with logits (kind 1), mean reduction
    times `weight`."""
    g0 = torch.Generator().manual_seed(B * 1000 + K)
    logits = torch.randn(B, K, generator=g0)
    l64 = logits.double().requires_grad_(True)
    if kind == 0:
        labels = torch.randint(0, K, (B,), generator=g0)
        ref = weight * torch.nn.functional.cross_entropy(l64, labels)
    else:
        labels = (torch.rand(B, K, generator=g0) < 0.1).float()
        ref = weight * torch.nn.functional.binary_cross_entropy_with_logits(l64, labels.double())
    ref.backward()
    loss, dl = _loss_call(pkg, lib, logits, labels, kind, weight)
    _loss_check(f"loss kind={kind} B={B} K={K} weight={weight}", loss, dl, ref.detach(), l64.grad)


@pytest.mark.parametrize("weight", [1.0, 0.5])
def test_cross_entropy_with_ignored_clips_rescales_every_gradient_row(pkg, lib, weight):
    """Labels of -100: the mean runs over the other clips, and one block rescales the B * K = 153 900 gradient elements already written
    with 1 / B (256 per trip).  Every label -100: the loss is NaN and the gradient zero, as torch gives."""
    B, K = 300, 513
    g0 = torch.Generator().manual_seed(5)
    logits = torch.randn(B, K, generator=g0)
    labels = torch.randint(0, K, (B,), generator=g0)
    labels[torch.rand(B, generator=g0) < 0.3] = -100
    labels[B - 1] = -100  # the last row is rescaled (a zero row) and the one before it holds values
    labels[B - 2] = 7
    assert B * K > 256 and 0 < int((labels == -100).sum()) < B
    l64 = logits.double().requires_grad_(True)
    ref = weight * torch.nn.functional.cross_entropy(l64, labels)
    ref.backward()
    loss, dl = _loss_call(pkg, lib, logits, labels, 0, weight)
    _loss_check(f"loss ignored clips weight={weight}", loss, dl, ref.detach(), l64.grad)
    assert dl[labels == -100].abs().max().item() == 0.0
    none = torch.full((B,), -100)
    l64 = logits.double().requires_grad_(True)
    ref = weight * torch.nn.functional.cross_entropy(l64, none)
    ref.backward()
    loss, dl = _loss_call(pkg, lib, logits, none, 0, weight)
    assert math.isnan(ref.item()) and math.isnan(loss.item())
    assert l64.grad.abs().max().item() == 0.0 and dl.abs().max().item() == 0.0


# ---- stlt_grad_norm --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("clipping", [True, False])
@pytest.mark.parametrize("n", [1, 3, 4, 5, 1048576, 1048577, 1050001])
def test_grad_norm_block_cap_and_scalar_tail(pkg, lib, n, clipping):
    """sumsq_kernel: 16-byte loads over n / 4 vectors on at most 1024 blocks (1 048 576 elements: every thread of 1024 blocks one
    vector; 1 050 001: a second grid-stride trip for some), the n % 4 last elements by one thread (n = 1, 3: nothing but the tail)."""
    g = _rand(n, seed=n)
    ref = math.sqrt(float((g.double() ** 2).sum()))
    max_norm = ref * (0.5 if clipping else 2.0)
    coef = min(1.0, max_norm / (ref + 1e-6))
    assert (coef < 1.0) == clipping
    gd, sc, out = g.to(DEV), torch.empty(1024, device=DEV), torch.empty(2, device=DEV)
    _, notes = _recorded(pkg, lambda: pkg._lib.check(lib.stlt_grad_norm(gd.data_ptr(), n, max_norm, sc.data_ptr(), out.data_ptr(), _stream()), "stlt_grad_norm"))
    nn, blocks, tail = _cut(notes, "grad_norm", "n", "blocks", "tail")
    assert nn == n and tail == n % 4 and blocks == max(1, min(1024, _ceil(n // 4, 256)))
    if n >= 1048576:
        assert blocks == 1024 and (n // 4 > 256 * blocks) == (n == 1050001) and (tail > 0) == (n != 1048576)
    else:
        assert blocks == 1 and (n // 4 == 0) == (n < 4)
    norm, c = out.cpu().double().tolist()
    print(f"[partition] grad_norm n={n} clipping={clipping}: norm {abs(norm - ref) / ref:.3e}, coefficient {abs(c - coef) / coef:.3e} (bar 1e-05 relative)")
    assert abs(norm - ref) <= 1e-5 * ref and abs(c - coef) <= 1e-5 * coef
    assert c == 1.0 if not clipping else c < 1.0


# ---- stlt_gelu_fwd / stlt_gelu_bwd -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [4, 4194304, 4194308, 4200000])
def test_gelu_block_cap_and_grid_stride(pkg, lib, n):
    """At most 4096 blocks x 256 threads x 4 elements = 4 194 304 elements in one trip; one vector more starts the grid stride."""
    u, dh = _rand(n, seed=n), _rand(n, seed=n + 1)
    ud, dhd, h, du = u.to(DEV), dh.to(DEV), torch.empty(n, device=DEV), torch.empty(n, device=DEV)
    _, notes = _recorded(pkg, lambda: (pkg._lib.check(lib.stlt_gelu_fwd(ud.data_ptr(), h.data_ptr(), n, _stream()), "stlt_gelu_fwd"),
                                       pkg._lib.check(lib.stlt_gelu_bwd(dhd.data_ptr(), ud.data_ptr(), du.data_ptr(), n, _stream()), "stlt_gelu_bwd")))
    for head in ("gelu_fwd", "gelu_bwd n"):
        nn, blocks = _cut(notes, head, "n", "blocks")
        assert nn == n and blocks == min(4096, _ceil(n // 4, 256)), notes
        assert (n // 4 > 256 * blocks) == (n > 4194304)  # a second trip of the grid-stride loop
    u64 = u.double().requires_grad_(True)
    ref = torch.nn.functional.gelu(u64)
    ref.backward(dh.double())
    _check(f"gelu_fwd n={n}", h, ref.detach())
    _check(f"gelu_bwd n={n}", du, u64.grad)


# ---- the FFN hidden gradient with its column sums (gelu_bwd_colsum_kernel or the product epilogue that replaces it) --------------
@pytest.mark.parametrize("M", [16384, 16385, 16400])
def test_ffn_block_bwd_hidden_gradient_column_sums_past_512_parts(pkg, M):
    """launch_gelu_bwd_colsum cuts the rows into 32-row parts and, past 16384 rows, into 512 parts of ceil(M / 512) rows.
    stlt_ffn_block_bwd_train (blocks.hip: stlt_ffn_hidden_bwd) sends du = (df·W2) ∘ gelu'(u) and its column sums there when the partial
    rows of the dX product's epilogue (ceil(M / 256) * 16 of them) do not fit the lent reduction scratch, as at these counts, or with
    STLT_FUSE_GELU_BWD=0; otherwise to that epilogue.  Whichever took it (the case prints which) must give the first Linear's bias
    gradient and the input gradient (and the other gradients of the block) to the op-level bar; the kernel's cut is asserted from its note."""
    d = 64
    x, g = _rand(M, d, seed=1), _rand(M, d, seed=2)
    w1, b1 = _rand(4 * d, d, seed=3, scale=1 / math.sqrt(d)), _rand(4 * d, seed=4, scale=0.1)
    w2, b2 = _rand(d, 4 * d, seed=5, scale=1 / math.sqrt(4 * d)), _rand(d, seed=6, scale=0.1)
    ln_w, ln_b = 1 + 0.1 * _rand(d, seed=7), 0.1 * _rand(d, seed=8)
    host = (x, w1, b1, w2, b2, ln_w, ln_b)
    leaves = [t.clone().to(DEV).requires_grad_(True) for t in host]
    out = pkg.ops.FfnBlockFn.apply(leaves[0], 1e-5, pkg._lib.ACT_GELU, True, 0.0, *leaves[1:])
    _, notes = _recorded(pkg, lambda: out.backward(g.to(DEV)))
    kernel = [n for n in notes if "gelu_bwd+colsum" in n]
    if kernel:
        rows, cols, parts, per = _cut(kernel, "gelu_bwd+colsum", "rows", "cols", "parts", "rows/part")
        assert (rows, cols) == (M, 4 * d) and per == (32 if M <= 16384 else _ceil(M, 512)) and parts == _ceil(M, per) and parts <= 512, kernel
        assert (per > 32) == (M > 16384)
        print(f"[partition] ffn M={M}: gelu_bwd_colsum_kernel, {parts} parts of {per} rows")
    else:
        epi = [n for n in notes if n.startswith("gemm") and f"M={M} " in n and f"N={4 * d} " in n and f"K={d} " in n]
        assert epi, notes  # the dX product of the hidden gradient: M x 4d over a contraction of d
        print(f"[partition] ffn M={M}: the product epilogue took the hidden gradient ({epi[0]})")
    r = [t.double().requires_grad_(True) for t in host]
    hid = torch.nn.functional.gelu(r[0] @ r[1].t() + r[2])
    torch.nn.functional.layer_norm(r[0] + hid @ r[3].t() + r[4], (d,), r[5], r[6], 1e-5).backward(g.double())
    for got, want, name in zip(leaves, r, ("dx", "dw1", "db1", "dw2", "db2", "dln_w", "dln_b")):
        _check(f"ffn M={M} {name}", got.grad, want.grad)


# ---- stlt_attn_core_bwd ----------------------------------------------------------------------------------------------------------
def _attn_bwd_ref(qkv, g, kpm, causal, H):
    S, L, d3 = qkv.shape
    d = d3 // 3
    x = qkv.double().requires_grad_(True)
    sp = lambda t: t.reshape(S, L, H, 64).transpose(1, 2)
    sc = sp(x[..., :d]) @ sp(x[..., d:2 * d]).transpose(-1, -2) / 8.0
    masked = kpm[:, None, None, :].expand(S, H, L, L).clone()
    if causal:
        masked |= torch.ones(L, L, dtype=torch.bool).triu(1)
    pr = torch.nan_to_num(torch.softmax(sc.masked_fill(masked, float("-inf")), -1), nan=0.0)  # fully masked rows
    (pr @ sp(x[..., 2 * d:])).transpose(1, 2).reshape(S, L, d).backward(g.double())
    return x.grad


@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("S,L,H", [(300, 17, 2), (21, 17, 2), (1500, 7, 2), (21, 7, 2), (257, 33, 4), (21, 33, 4)])
def test_attn_core_bwd_waves_with_more_than_one_item(pkg, S, L, H, causal):
    """attn_bwd16 (and its fallback for short causal sequences): chunks = min(CUs * waves / H, items, 256) persistent waves per head; a
    wave walks item, item + chunks, ... and adds the column sums of dqkv (the in-projection bias gradient) across its items.  S = 300 x 17
    tokens: 300 items on 256 chunks; 1500 x 7: 375 items of four sequences; 257 x 33 at four heads: 257 items on 192 chunks.  S = 21 is the
    one-item-per-wave control of each.  Padded keys and one fully padded sequence, no dropout."""
    d = 64 * H
    qkv, g = _rand(S, L, 3 * d, seed=L + S, scale=1.5), _rand(S, L, d, seed=L + S + 1)
    kpm = torch.rand(S, L, generator=torch.Generator().manual_seed(L)) < 0.3
    kpm[:, 0] = False
    kpm[4, :] = True  # a fully padded sequence: zero gradient
    (dqkv, gb), notes = _recorded(pkg, lambda: pkg.ops.attn_core_bwd(qkv.to(DEV), g.to(DEV), kpm.to(DEV), causal, H, 0.0, 0, 0, want_bias_grad=True))
    note = [n for n in notes if n.startswith("attn_bwd")][0]
    if "bwd16" in note:
        items, chunks = _cut(notes, "bwd16", "items", "chunks")
        assert items == (S if L > 16 else _ceil(S * L, 2 * (16 // L) * L)), note
    else:  # sequences of at most 16 tokens under a causal mask: the FMA kernel on groups of floor(32 / L) sequences
        items, chunks = _cut(notes, "fma groups", "groups", "chunks")
        assert items == (_ceil(S, 32 // L) if L <= 32 else S), note
    assert (items > chunks) == (S > 21) and chunks <= 256, note  # some wave takes a second item / every wave has one
    ref = _attn_bwd_ref(qkv, g, kpm, causal, H)
    tag = f"attn_bwd S={S} L={L} H={H} causal={int(causal)} items={items} chunks={chunks}"
    _check(tag + " dqkv", dqkv, ref)
    _check(tag + " column sums", gb, ref.reshape(-1, 3 * d).sum(0), bar=5e-5)
    assert dqkv[4].abs().max().item() == 0.0 and torch.isfinite(dqkv).all()


# ---- stlt_reduce_slabs -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("accumulate", [0, 1])
@pytest.mark.parametrize("n,n_slabs", [(2097152, 2), (2097156, 2), (2100000, 2), (16384, 33), (16385, 33)])
def test_reduce_slabs_block_cap_and_tall_boundary(pkg, lib, n, n_slabs, accumulate):
    """reduce_slabs_kernel: at most 2048 blocks x 1024 elements in one trip (2 097 152), then a grid stride; more than 32 slabs of at
    most 16384 columns take the tall kernel, 16385 columns the wide one.  The element-wise bound of test_reduce_slabs."""
    stride = (n + 3) // 4 * 4  # a slab stride of whole 16-byte vectors, as test_reduce_slabs
    slabs, dst0 = _rand(n_slabs, stride, seed=n % 1000 + n_slabs), _rand(n, seed=7)
    slabs[:, n:] = float("nan")  # the pitch gap: never read
    sd, dst = slabs.to(DEV), dst0.to(DEV) if accumulate else torch.empty(n, device=DEV)
    _, notes = _recorded(pkg, lambda: pkg._lib.check(lib.stlt_reduce_slabs(sd.data_ptr(), stride, n_slabs, dst.data_ptr(), n, accumulate, _stream()), "stlt_reduce_slabs"))
    slabs = slabs[:, :n]
    nn, ns, blocks = _cut(notes, "reduce n", "n", "slabs", "blocks")
    note = [x for x in notes if "reduce n" in x][0]
    assert (nn, ns) == (n, n_slabs) and ("tall" in note) == (n_slabs > 32 and n <= 16384), note
    if "tall" in note:
        assert blocks == _ceil(n, 16)
    else:
        assert blocks == min(2048, _ceil(n, 1024)) and (n > 1024 * blocks) == (n > 2097152 and n_slabs == 2), note
    ref = slabs.double().sum(0) + (dst0.double() if accumulate else 0.0)
    mag = slabs.double().abs().sum(0) + dst0.double().abs()
    err = (dst.cpu().double() - ref).abs()
    print(f"[partition] reduce_slabs n={n} slabs={n_slabs} accumulate={accumulate}: {(err / ((n_slabs + 1) * EPS24 * 1.01 * mag)).max().item():.3e} of the element-wise bound")
    assert bool((err <= (n_slabs + 1) * EPS24 * 1.01 * mag).all())
