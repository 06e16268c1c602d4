"""What the R3D-50 GPU tests reach, asserted on the host from the library's own workspace queries (pure host arithmetic, no GPU): a
split launch needs one slab of partial sums per split, so workspace bytes ÷ slab bytes is the split count the library plans.

- each splitting op-level case of tests/test_r3d_gpu.py and tests/test_r3d_train_gpu.py reaches the count its comment names
  (PLANNED_SPLITS), so a change of the plans cannot make a case stop splitting unnoticed;
- the whole-trunk sweep of tests/test_r3d_shapes_gpu.py reaches an unsplit and a >= 32-split forward, a >= 200-split weight gradient, a
  split stride-2 data gradient, a stride-2 parity class without rows and odd input extents under stride 2 in t, h and w;
- the general cases of tests/test_conv3d_general_gpu.py reach what their table says (negative sub-padding, unread planes, per-class split
  clamping), and the forward, data-gradient and weight-gradient workspace queries equal what an enumeration of the convolution gives."""
import ctypes

import pytest
import torch

import test_conv3d_general_gpu as GEN
import test_r3d_gpu as FWD
import test_r3d_shapes_gpu as SWEEP
import test_r3d_train_gpu as BWD

BLOCKS = (3, 4, 6, 3)
PLANES = (64, 128, 256, 512)


def _out(n, k, s, p):
    return (n + 2 * p - k) // s + 1


def trunk_descs(B, T, H, W):
    """The trunk's 53 convs for video (B, 3, T, H, W) in state-dict order: (B, T, H, W, c_in, c_out, k, stride (t, h, w), pad), the
    stem's c_in padded to 4 as the trunk stores it."""
    out = [(B, T, H, W, 4, 64, 7, (1, 2, 2), 3)]
    t, h, w = _out(T, 7, 1, 3), _out(H, 7, 2, 3), _out(W, 7, 2, 3)
    t, h, w = _out(t, 3, 2, 1), _out(h, 3, 2, 1), _out(w, 3, 2, 1)  # max-pool
    cin = 64
    for L, (n, planes) in enumerate(zip(BLOCKS, PLANES)):
        for b in range(n):
            s = 2 if (L > 0 and b == 0) else 1
            t2, h2, w2 = _out(t, 3, s, 1), _out(h, 3, s, 1), _out(w, 3, s, 1)
            out += [(B, t, h, w, cin, planes, 1, (1, 1, 1), 0), (B, t, h, w, planes, planes, 3, (s, s, s), 1),
                    (B, t2, h2, w2, planes, planes * 4, 1, (1, 1, 1), 0)]
            if b == 0:
                out.append((B, t, h, w, cin, planes * 4, 1, (s, s, s), 0))
            t, h, w, cin = t2, h2, w2, planes * 4
    return out


def _desc(pkg, B, T, H, W, ci, co, k, s, p):
    return pkg._lib.Conv3dDesc(B, T, H, W, ci, co, *k, *s, *p)


def _dims(B, T, H, W, co, k, s, p):
    To, Ho, Wo = [_out(n, kk, ss, pp) for n, kk, ss, pp in zip((T, H, W), k, s, p)]
    return B * To * Ho * Wo, (To, Ho, Wo)


def fwd_splits(lib, d, M, co, n_split=0):
    return int(lib.stlt_conv3d_workspace_bytes(ctypes.byref(d), n_split)) // (M * co * 4) or 1


def wgrad_splits(lib, d, co, K, n_split=0):
    return int(lib.stlt_conv3d_bwd_weight_workspace_bytes(ctypes.byref(d), n_split)) // (co * K * 4)


def dgrad_bytes(lib, d, n_split=0):
    return int(lib.stlt_conv3d_bwd_data_workspace_bytes(ctypes.byref(d), n_split))


@pytest.mark.parametrize("case", sorted(FWD.PLANNED_SPLITS))
def test_forward_cases_split_as_planned(pkg, case):
    lib = pkg._lib.load()
    B, Ci, T, H, W, Co, k, s, p, _, _, n_split = FWD.CASES[case]
    M, _ = _dims(B, T, H, W, Co, k, s, p)
    assert fwd_splits(lib, _desc(pkg, B, T, H, W, (Ci + 3) // 4 * 4, Co, k, s, p), M, Co, n_split) == FWD.PLANNED_SPLITS[case]


@pytest.mark.parametrize("case", sorted(BWD.PLANNED_SPLITS))
def test_backward_cases_split_as_planned(pkg, case):
    lib = pkg._lib.load()
    B, Ci, T, H, W, Co, k, s, p, n_split = BWD.CASES[case]
    want_wg, want_dg = BWD.PLANNED_SPLITS[case]
    c_pad = (Ci + 3) // 4 * 4
    d = _desc(pkg, B, T, H, W, c_pad, Co, k, s, p)
    assert wgrad_splits(lib, d, Co, k[0] * k[1] * k[2] * c_pad, n_split) == want_wg
    nbytes = dgrad_bytes(lib, d, n_split)
    if s == (1, 1, 1):
        assert nbytes // (B * T * H * W * Ci * 4) == want_dg or (want_dg == 1 and nbytes == 0)
    else:  # parity classes of different sizes: only "some class splits" (nonzero workspace) or not
        assert (nbytes > 0) == (want_dg > 1)
    if any(n == 1 for n, ss in zip((T, H, W), s) if ss == 2):  # an input extent of 1 under stride 2: classes without rows
        assert "rowless" in case


def test_trunk_descs_match_the_trunk(pkg):
    for shape in list(SWEEP.SHAPES) + [SWEEP.BIG]:
        descs = trunk_descs(*shape)
        assert len(descs) == 53
        B, t, h, w, ci, co, k, s, p = descs[-1]
        _, (To, Ho, Wo) = _dims(B, t, h, w, co, (k,) * 3, s, (p,) * 3)
        R = pkg.modelling.resnet3d
        assert (co, To, Ho, Wo) == (2048, R._trunk_out(shape[1]), R._trunk_out(shape[2], 2), R._trunk_out(shape[3], 2))


def test_sweep_reaches_the_plans(pkg):
    lib = pkg._lib.load()
    fwd, wg_max, dg_s2_split, rowless, odd = set(), 0, False, False, [False] * 3
    for shape in list(SWEEP.SHAPES) + [SWEEP.BIG]:
        grad = SWEEP.SHAPES.get(shape) == "grad"
        # the training trunk plans every shape (T <= 8 once divided by zero planning layer 4's row-less parity classes)
        assert lib.stlt_r3d_tape_bytes(*shape) > 0 and lib.stlt_r3d_backward_workspace_bytes(*shape) > 0, shape
        for B, T, H, W, ci, co, k, s, p in trunk_descs(*shape):
            kk, pp = (k,) * 3, (p,) * 3
            d = _desc(pkg, B, T, H, W, ci, co, kk, s, pp)
            M, _ = _dims(B, T, H, W, co, kk, s, pp)
            fwd.add(fwd_splits(lib, d, M, co))
            if not grad:
                continue
            wg_max = max(wg_max, wgrad_splits(lib, d, co, k ** 3 * ci))
            if s == (2, 2, 2):
                dg_s2_split |= dgrad_bytes(lib, d) > 0
                rowless |= min(T, H, W) == 1
            for i, (n, st) in enumerate(zip((T, H, W), s)):
                odd[i] |= st == 2 and n % 2 == 1
    assert 1 in fwd and max(fwd) >= 32, sorted(fwd)
    assert wg_max >= 200, wg_max
    assert dg_s2_split and rowless
    assert all(odd), odd


# ---- the whole-trunk size queries against an enumeration of the 53 descriptors and the op-level queries ----
QUERY_SHAPES = list(SWEEP.SHAPES) + [SWEEP.BIG, (2, 32, 112, 112), (1, 1, 1, 1), (2, 3, 17, 9), (5, 7, 33, 40)]
OVERSIZED = [(2 ** 20, 32, 112, 112), (1, 4096, 4096, 4096)]  # within the trunk's own limits, refused by a conv's (rows and elements below 2^31)


def _a(n):
    return -(-n // 256) * 256


def enumerated_sizes(pkg, lib, B, T, H, W):
    """(inference workspace, tape, backward workspace) bytes from the descriptors: block-level activations, and per conv the op-level
    workspace queries with n_split = 0 (the library's plan, which is what the trunk runs)."""
    descs = trunk_descs(B, T, H, W)
    out_elems, fwd_ws, wg_ws, dg_ws = [], [], [], []
    for b, t, h, w, ci, co, k, s, p in descs:
        d = _desc(pkg, b, t, h, w, ci, co, (k,) * 3, s, (p,) * 3)
        M, _ = _dims(b, t, h, w, co, (k,) * 3, s, (p,) * 3)
        out_elems.append(M * co)
        fwd_ws.append(int(lib.stlt_conv3d_workspace_bytes(ctypes.byref(d), 0)))
        wg_ws.append(int(lib.stlt_conv3d_bwd_weight_workspace_bytes(ctypes.byref(d), 0)))
        dg_ws.append(int(lib.stlt_conv3d_bwd_data_workspace_bytes(ctypes.byref(d), 0)))
    stem = out_elems[0]
    _, t, h, w = descs[1][:4]  # the first block's conv1 reads the max-pool's output
    pool = B * t * h * w * 64
    blocks, i = [], 1
    for n in BLOCKS:
        for b in range(n):
            blocks.append(out_elems[i:i + 3])  # conv1, conv2, conv3; the downsample's output is no larger than conv3's
            i += 4 if b == 0 else 3
    assert i == 53 and len(blocks) == 16
    act = max([pool] + [e for blk in blocks for e in blk])
    video = _a(16 * B * T * H * W)
    infer = video + 3 * _a(4 * act) + _a(4 * max(stem, 2 * act)) + _a(max(fwd_ws))
    tape = video + _a(4 * stem) + _a(4 * pool) + _a(pool) + sum(_a(4 * e) for blk in blocks for e in blk)
    bwd = 4 * _a(4 * act) + _a(4 * stem) + _a(max(wg_ws + dg_ws[1:]))
    return infer, tape, bwd


def trunk_queries(lib, shape):
    return int(lib.stlt_r3d_workspace_bytes(*shape)), int(lib.stlt_r3d_tape_bytes(*shape)), int(lib.stlt_r3d_backward_workspace_bytes(*shape))


@pytest.mark.parametrize("shape", QUERY_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_trunk_size_queries_match_the_enumeration(pkg, shape):
    lib = pkg._lib.load()
    assert trunk_queries(lib, shape) == enumerated_sizes(pkg, lib, *shape)


def test_trunk_size_queries_pinned_and_oversized(pkg):
    lib = pkg._lib.load()
    assert trunk_queries(lib, (1, 8, 64, 64)) == (16252928, 10575872, 34603008)
    for shape in OVERSIZED:  # all three refuse what one of the trunk's convs refuses
        assert trunk_queries(lib, shape) == (0, 0, 0), shape


# ---- the general op-level cases of tests/test_conv3d_general_gpu.py: what each reaches, and the three workspace queries, against an
# enumeration of the convolution itself (which output positions read which input positions through which taps) ----
def parity_classes(n, k, s, p):
    """One dimension of a data gradient by brute force: every (input i, tap d, output o) with o·s - p + d = i, o unbounded (a dy index
    outside [0, To) reads as zero), grouped by i mod s.  Per class: rows (inputs 0 <= i < n of that residue), taps (distinct d), and
    first = the lowest dy index a row reads, relative to the row's own index a = i // s (the same for every row of a class)."""
    out = []
    for r in range(s):
        rows = [i for i in range(n) if i % s == r]
        rel = {}
        for i in range(r, r + 4 * s, s):  # four rows suffice to see that the pattern does not depend on the row
            reach = [(d, (i + p - d) // s) for d in range(k) if (i + p - d) % s == 0]
            rel.setdefault("taps", sorted(d for d, _ in reach))
            assert rel["taps"] == sorted(d for d, _ in reach)
            first = min(o for _, o in reach) - i // s if reach else None
            assert rel.setdefault("first", first) == first
        out.append({"rows": len(rows), "taps": len(rel["taps"]), "first": rel["first"]})
    return out


def _clamp(n, slabs):
    """an explicit request of n ranges over `slabs` slabs of 32, as the launchers divide them"""
    if slabs == 0 or n <= 1:
        return 1
    per = -(-slabs // min(n, slabs))
    return -(-slabs // per)


def _general_desc(pkg, case):
    B, Ci, T, H, W, Co, k, s, p, _ = GEN.CASES[case]
    return pkg._lib.Conv3dDesc(B, T, H, W, Ci, Co, *k, *s, *p), (B, Ci, T, H, W, Co, k, s, p)


@pytest.mark.parametrize("case", GEN.DGRAD)
def test_general_dgrad_workspace_matches_the_enumerated_classes(pkg, case):
    lib = pkg._lib.load()
    d, (B, Ci, T, H, W, Co, k, s, p) = _general_desc(pkg, case)
    per_dim = [parity_classes(n, kk, ss, pp) for n, kk, ss, pp in zip((T, H, W), k, s, p)]
    classes = [(B * a["rows"] * b["rows"] * c["rows"], a["taps"] * b["taps"] * c["taps"] * Co) for a in per_dim[0] for b in per_dim[1] for c in per_dim[2]]
    assert sum(M for M, _ in classes) == B * T * H * W and sum(K for _, K in classes) == k[0] * k[1] * k[2] * Co
    for n in (1, 2, 3, 1024):
        want = 0
        for M, K in classes:
            splits = _clamp(n, -(-K // 32))
            want = max(want, splits * M * Ci * 4 if splits > 1 else 0)
        assert dgrad_bytes(lib, d, n) == want, (case, n)
    assert dgrad_bytes(lib, d, 1) == 0


@pytest.mark.parametrize("case", GEN.ALL)
def test_general_forward_and_wgrad_workspace(pkg, case):
    lib = pkg._lib.load()
    d, (B, Ci, T, H, W, Co, k, s, p) = _general_desc(pkg, case)
    M, _ = _dims(B, T, H, W, Co, k, s, p)
    K = k[0] * k[1] * k[2] * Ci
    for n in (1, 2, 3, 1024):
        splits = _clamp(n, -(-K // 32))
        assert int(lib.stlt_conv3d_workspace_bytes(ctypes.byref(d), n)) == (splits * M * Co * 4 if splits > 1 else 0), (case, n)
        if case in GEN.WGRAD:  # the weight gradient always goes through its partial slabs: one (c_out, K) slab per range of m-slabs
            assert int(lib.stlt_conv3d_bwd_weight_workspace_bytes(ctypes.byref(d), n)) == _clamp(n, -(-M // 32)) * Co * K * 4, (case, n)
    assert int(lib.stlt_conv3d_workspace_bytes(ctypes.byref(d), 1)) == 0


def test_general_cases_reach_what_they_claim():
    def dims(case):
        B, Ci, T, H, W, Co, k, s, p, n_split = GEN.CASES[case]
        return [parity_classes(n, kk, ss, pp) for n, kk, ss, pp in zip((T, H, W), k, s, p)], Co, n_split

    # negative sub-padding: a class whose rows start reading dy one past their own index, in t, h and w
    for case in ("k345_s2_p234_negpad", "k322_s2_p211_negpad"):
        per_dim, _, _ = dims(case)
        assert all(any(c["first"] == 1 for c in dim) for dim in per_dim), (case, per_dim)
    per_dim, _, _ = dims("k322_s2_p211_negpad")
    assert all(any(c["first"] == 1 and c["taps"] == 1 for c in dim) for dim in per_dim)
    # planes no window reads, in t, h and w; the other data-gradient cases have none where the table does not say so
    B, Ci, T, H, W, Co, k, s, p, _ = GEN.CASES["k222_s2_p000_unread"]
    assert [GEN.unread_planes(n, kk, ss, pp) for n, kk, ss, pp in zip((T, H, W), k, s, p)] == [[T - 1], [H - 1], [W - 1]]
    B, Ci, T, H, W, Co, k, s, p, _ = GEN.CASES["k222_s3_p011"]
    assert all(GEN.unread_planes(n, kk, ss, pp) for n, kk, ss, pp in zip((T, H, W), k, s, p))  # stride above the kernel: gaps
    # even kernels under stride 2: every class has taps, and one explicit request of 3 becomes different counts in different classes
    per_dim, Co, n_split = dims("k234_s2_p011_split3")
    taps = sorted({a["taps"] * b["taps"] * c["taps"] for a in per_dim[0] for b in per_dim[1] for c in per_dim[2]})
    assert taps == [2, 4] and n_split == 3
    assert sorted({_clamp(n_split, -(-t * Co // 32)) for t in taps}) == [2, 3]
    assert GEN.CASES["k234_s2_p011"][:9] == GEN.CASES["k234_s2_p011_split3"][:9]
    # stride 1: the data gradient's padding is k - 1 - p, so first = -(k - 1 - p): "full" (p = 0) and none (p = k - 1)
    assert [c[0]["first"] for c in dims("k333_p000_valid")[0]] == [-2, -2, -2]
    assert [c[0]["first"] for c in dims("k333_p222_grow")[0]] == [0, 0, 0]
    # no exchange of two dimensions maps a case onto itself
    for case, (B, Ci, T, H, W, Co, k, s, p, _) in GEN.CASES.items():
        sig = list(zip((T, H, W), k, s, p))
        assert len(set(sig)) == 3, (case, sig)
    # which families run which cases
    assert set(GEN.ALL) - set(GEN.WGRAD) == {"k212_cout5"}
    assert set(GEN.WGRAD) - set(GEN.DGRAD) == {"k133_s122_p011", "k151_s213_p040", "k222_s3_p011"}


@pytest.mark.parametrize("case", GEN.ALL)
def test_general_integer_references_stay_exact(case):
    """the integer variant's float64 references of |x|, |w|, |dy| bound every partial sum of the fp32 kernels: below 2^24, so exact"""
    R = GEN.references(case, integer=True)
    assert max(R[key].max().item() for key in ("y_mag", "dx_mag", "dw_mag")) < 2 ** 24
    x, w, dy = GEN.inputs(case, integer=True)
    assert all(t.abs().max().item() == 2 and torch.equal(t, t.round()) for t in (x, w, dy))
