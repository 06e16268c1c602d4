"""Attention relevance of the fusion models on the GPU: the cross grad-probs kernel, the joint rollout and the joint read-out alone against
fp64 inside guard bands, the block call and the backbone-flag sweep, and forward_relevance of CAF / CACNF / LCF / TransformerResnet against
the fp64 restatement (tests/fusion_relevance_restated.py, which tests/test_fusion_relevance_cpu.py holds to the attention restatement and
to the closed form).  Every test prints its worst figure (profiles/fusion_relevance_bench.md records them)."""
import ctypes as C
import functools
import sys

import pytest
import torch

import fusion_attention_restated as FR
import fusion_relevance_restated as XR
import guard_arena as GA
import relevance_restated as R
from guard_arena import Out
from test_fusion_attention_cpu import EXTRA
from test_fusion_relevance_cpu import WHOLE_PATH_CASES, differenced, reached, reference
from test_relevance_cpu import _rel

pytestmark = pytest.mark.gpu
DEV = "cuda"
EINVAL = -1
OP_CAP = 1e-5       # the project's op-level bound (tests/test_relevance_gpu.py)
ROLLOUT_CAP = 1e-5  # every term of the chain is non-negative: no cancellation
# Whole path: max(2e-4, 4 f), the rule of tests/test_relevance_gpu.py; f is the fp32 floor of the restatement, measured by
# tests/test_fusion_relevance_cpu.py::test_fp32_floor_of_the_whole_path (largest figure over its cases and over repeated runs, the rollouts
# taken minus their identity): 2.93e-5, caf/top1 appearance_rollout - I — the appearance encoder's maps are small differences of 64-term dot
# products (the three relevance outputs, which no identity dominates, are at 2.8e-7 at most — the figure the issue's prototype gave)
FP32_FLOOR = 2.93e-5
CAP = max(2e-4, 4 * FP32_FLOOR)
LOGIT_TOL = 1e-4


def _report(what, value):
    print(f"\n[fusion relevance] {what}: {value}", file=sys.stderr)


def _to(batch):
    return {k: (v.to(DEV) if isinstance(v, torch.Tensor) else v) for k, v in batch.items()}


@pytest.fixture(scope="module")
def arena():
    a = GA.Arena(96 << 20, DEV)
    yield a
    del a
    torch.cuda.empty_cache()


# ---- the cross grad-probs kernel alone -------------------------------------------------------------------------------------------------
def _op_case(S, Lq, Lk, H, dh, seed):
    """q, kv and dctx uniform in [-1, 1]; about 30 % of the keys padded with key 0 kept — and, when there is more than one sequence, the
    last sequence fully masked"""
    d = H * dh
    q, kv, dctx = GA.rand(S, Lq, d, seed=seed), GA.rand(S, Lk, 2 * d, seed=seed + 1), GA.rand(S, Lq, d, seed=seed + 2)
    kpm = torch.rand(S, Lk, generator=torch.Generator().manual_seed(100 + seed)) < 0.3
    kpm[:, 0] = False
    if S > 1:
        kpm[S - 1, :] = True
    return q, kv, dctx, kpm


def _op_specs(q, kv, dctx, kpm):
    S, Lq, _ = q.shape
    Lk = kv.shape[1]
    return {"q": (q.reshape(S * Lq, -1), "in"), "kv": (kv.reshape(S * Lk, -1), "in"), "dctx": (dctx.reshape(S * Lq, -1), "in"),
            "kpm": (kpm.to(torch.uint8), "extent", 0), "abar": (Out((S * Lq, Lk)), "out")}


def _op_call(lib, S, Lq, Lk, H, dh, causal):
    d = H * dh  # the cross block's buffers: q (S*Lq, d) and the packed kv (S*Lk, 2d)
    return lambda o: lib.stlt_attn_grad_probs_cross(o.q.ptr, d, o.kv.ptr, o.kv.ptr + 4 * d, 2 * d, o.dctx.ptr, o.kpm.ptr, causal, S, Lq, Lk, H, dh, o.abar.ptr,
                                                    GA.stream())


def _op_ref(q, kv, dctx, kpm, causal, H):
    d = q.shape[-1]
    return XR.attn_grad_probs_cross(q.double(), kv[..., :d].double(), kv[..., d:].double(), dctx.double(), kpm, bool(causal), H)


SHAPES = [(1, 1, 0), (16, 33, 0), (33, 16, 0), (7, 64, 0), (64, 17, 0), (17, 65, 0), (65, 17, 0), (256, 33, 0), (33, 256, 0), (16, 16, 1), (33, 33, 1),
          (65, 65, 1)]


def _sizes(Lq, Lk, dh):
    """S = 1 and 5 — and, where the launcher routes by the number of work units (head dim 64 with 33 ... 64 keys: the vector kernel below
    128 units of 16 query rows, the MFMA kernel from there on), the two sequence counts on either side of that threshold"""
    if dh != 64 or not 32 < Lk <= 64:
        return (1, 5)
    s_mfma = -(-128 // ((Lq + 15) // 16))
    return tuple(sorted({1, 5, s_mfma - 1, s_mfma}))


@pytest.mark.parametrize("H,dh", [(2, 64), (3, 16), (2, 20)])
@pytest.mark.parametrize("Lq,Lk,causal", SHAPES)
def test_attn_grad_probs_cross_vs_fp64_inside_guard_bands(pkg, arena, Lq, Lk, causal, H, dh):
    """S = 1 and 5 (and both sides of the routing threshold: _sizes).  Plain call == arena call == second call bit for bit, no byte outside
    abar changes and every element of it is written (GA.three_ways); <= OP_CAP of max|ref| against the restated formula in fp64; masked
    entries exactly 0."""
    lib = pkg._lib.load()
    worst = 0.0
    for S in _sizes(Lq, Lk, dh):
        q, kv, dctx, kpm = _op_case(S, Lq, Lk, H, dh, seed=1000 * Lq + 7 * Lk + 10 * dh + S)
        got = GA.three_ways(lib, arena, _op_specs(q, kv, dctx, kpm), _op_call(lib, S, Lq, Lk, H, dh, causal), ["abar"])["abar"].view(S, Lq, Lk)
        ref = _op_ref(q, kv, dctx, kpm, causal, H)
        assert torch.isfinite(got).all() and (got >= 0).all()
        assert (got[FR.masked_entries(kpm, bool(causal), S, Lq, Lk)] == 0).all()
        if S > 1:
            assert (got[S - 1] == 0).all()  # the fully masked sequence: zeros, written
        assert Lk == 1 or ref.abs().max().item() > 0
        worst = max(worst, _rel(got, ref))
        assert worst <= OP_CAP, (S, Lq, Lk, H, dh, causal, worst)
    _report(f"attn_grad_probs_cross Lq={Lq} Lk={Lk} H={H} dh={dh} causal={causal} worst err / max|ref|", f"{worst:.2e}")


# (S, L, H, dh, causal, same kernel).  S = 4: the two launchers run different kernels (diag against one sided block; the packed vector kernel
# against the cross one — at L = 33 and head dim 64 too, where 12 units over three key blocks send the cross launcher to its vector kernel).
# Head dim 64, 17 ... 64 tokens and enough units: both run the sided MFMA kernel on the same views — 3 x 17 (two key blocks, the 17th row alone
# in its block), 43 x 33 (129 units, one above GX_MIN_UNITS at three key blocks), 32 x 64 (128 units at four key blocks).
PACKED_VIEWS = ([(4, L, H, dh, c, False) for c in (False, True) for H, dh in ((2, 64), (3, 16), (2, 20)) for L in (7, 16, 33, 65)]
                + [(S, L, 2, 64, c, True) for c in (False, True) for S, L in ((3, 17), (43, 33), (32, 64))])


@pytest.mark.parametrize("S,L,H,dh,causal,same_kernel", PACKED_VIEWS,
                         ids=[f"{f'{S}x' if same else ''}{L}-{H}-{dh}-{c}" for S, L, H, dh, c, same in PACKED_VIEWS])
def test_cross_kernel_on_a_packed_buffer_agrees_with_attn_grad_probs(pkg, S, L, H, dh, causal, same_kernel):
    """q = qkv, k = qkv + d, v = qkv + 2d, ld = 3d: stlt_attn_grad_probs' result within OP_CAP (and the fp64 formula's) — bit for bit where
    both launchers run the same kernel"""
    d = H * dh
    qkv, dctx = GA.rand(S, L, 3 * d, seed=L + dh).to(DEV), GA.rand(S, L, d, seed=L + dh + 1).to(DEV)
    kpm = torch.rand(S, L, generator=torch.Generator().manual_seed(L)) < 0.3
    kpm[:, 0] = False
    want = pkg.ops.attn_grad_probs(qkv, dctx, kpm.to(DEV), causal, H)
    got = pkg.ops.attn_grad_probs_cross(qkv[..., :d], qkv[..., d:2 * d], qkv[..., 2 * d:], dctx, kpm.to(DEV), causal, H)
    ref = R.attn_grad_probs(qkv.cpu().double(), dctx.cpu().double(), kpm, causal, H)
    e = (_rel(got, want.cpu().double()), _rel(got, ref))
    _report(f"cross vs packed kernel L={L} H={H} dh={dh} causal={causal}: vs packed, vs fp64", f"{e[0]:.2e}, {e[1]:.2e}")
    assert max(e) <= OP_CAP
    if same_kernel:
        assert torch.equal(got, want)


def test_attn_grad_probs_cross_refusals_leave_the_output_untouched(pkg, arena):
    """One refusal per rule: STLT_EINVAL, the message names the cause, nothing is launched.  A four-byte displacement is refused on the
    MFMA shapes (dh == 64, Lk <= 64) and accepted, with the aligned call's bits, at dh = 25."""
    lib = pkg._lib.load()
    S, Lq, Lk, H, dh = 3, 7, 9, 2, 64
    d = H * dh
    q, kv, dctx, kpm = _op_case(S, Lq, Lk, H, dh, seed=5)
    specs = _op_specs(q, kv, dctx, kpm)
    for operand in ("q", "kv", "dctx"):
        arena.reset()
        A = {k: arena.place(s[0], s[1], band=(s[2] if len(s) > 2 else None), name=k, misalign=(4 if k == operand else 0)) for k, s in specs.items()}
        o = type("O", (), A)
        assert _op_call(lib, S, Lq, Lk, H, dh, 0)(o) == EINVAL and "16-byte aligned" in GA.last_error(lib), operand
        arena.check(launched=False)
    arena.reset()
    A = {k: arena.place(s[0], s[1], band=(s[2] if len(s) > 2 else None), name=k) for k, s in specs.items()}
    qp, kp, gp, mp, ap = (A[n].ptr for n in ("q", "kv", "dctx", "kpm", "abar"))
    vp, s = kp + 4 * d, GA.stream()
    f = lib.stlt_attn_grad_probs_cross
    for args, word in (((qp, d, kp, vp, 2 * d, gp, mp, 0, S, 0, Lk, H, dh, ap, s), "lengths"), ((qp, d, kp, vp, 2 * d, gp, mp, 0, 1, 257, Lk, H, dh, ap, s), "lengths"),
                       ((qp, d, kp, vp, 2 * d, gp, mp, 0, 1, Lq, 257, H, dh, ap, s), "lengths"), ((qp, d, kp, vp, 2 * d, gp, mp, 0, S, Lq, Lk, H, 0, ap, s), "head dim"),
                       ((qp, d, kp, vp, 2 * d, gp, mp, 0, S, Lq, Lk, H, 257, ap, s), "head dim"), ((qp, d, kp, vp, 2 * d, gp, mp, 0, S, Lq, Lk, 0, dh, ap, s), "head count"),
                       ((qp, d, kp, vp, 2 * d, gp, mp, 0, -1, Lq, Lk, H, dh, ap, s), "sequence"), ((qp, d, kp, vp, 2 * d, gp, mp, 1, S, Lq, Lk, H, dh, ap, s), "causal"),
                       ((qp, d - 1, kp, vp, 2 * d, gp, mp, 0, S, Lq, Lk, H, dh, ap, s), "ldq"), ((qp, d, kp, vp, d - 1, gp, mp, 0, S, Lq, Lk, H, dh, ap, s), "ldkv"),
                       ((qp, d + 2, kp, vp, 2 * d, gp, mp, 0, S, Lq, Lk, H, dh, ap, s), "multiples of 4"),
                       ((None, d, kp, vp, 2 * d, gp, mp, 0, S, Lq, Lk, H, dh, ap, s), "null"), ((qp, d, None, vp, 2 * d, gp, mp, 0, S, Lq, Lk, H, dh, ap, s), "null"),
                       ((qp, d, kp, None, 2 * d, gp, mp, 0, S, Lq, Lk, H, dh, ap, s), "null"), ((qp, d, kp, vp, 2 * d, None, mp, 0, S, Lq, Lk, H, dh, ap, s), "null"),
                       ((qp, d, kp, vp, 2 * d, gp, None, 0, S, Lq, Lk, H, dh, ap, s), "null"), ((qp, d, kp, vp, 2 * d, gp, mp, 0, S, Lq, Lk, H, dh, None, s), "null"),
                       ((qp, d, kp, vp, 2 * d, gp, mp, 0, S, Lq, Lk, H, dh, ap + 2, s), "abar")):
        assert f(*args) == EINVAL and word in GA.last_error(lib), (word, GA.last_error(lib))
    arena.check(launched=False)
    # dh = 25: four-byte alignment is enough, and the displaced call gives the aligned call's bits
    S, Lq, Lk, H, dh = 3, 9, 11, 4, 25
    d = H * dh
    q, kv, dctx, kpm = _op_case(S, Lq, Lk, H, dh, seed=6)
    specs = _op_specs(q, kv, dctx, kpm)
    want = pkg.ops.attn_grad_probs_cross(q.to(DEV), kv.to(DEV)[..., :d], kv.to(DEV)[..., d:], dctx.to(DEV), kpm.to(DEV), False, H).cpu()
    for operand in ("q", "kv", "dctx", "abar"):
        got = GA.misaligned(lib, arena, specs, _op_call(lib, S, Lq, Lk, H, dh, 0), ["abar"], operand=operand, mis=4)
        assert torch.equal(got["abar"].view(S, Lq, Lk), want), operand
    assert _rel(want, _op_ref(q, kv, dctx, kpm, 0, H)) <= OP_CAP


# ---- the joint rollout and the read-out alone ------------------------------------------------------------------------------------------
def _joint_case(S, T, A, n, seed):
    """non-negative maps uniform in [0, 1/J] (row sums of X below 1), initial rollouts the identity plus such a map (the layout one lower
    triangular, as a causal tower's is)"""
    g = torch.Generator().manual_seed(seed)
    J = T + A
    rnd = lambda *s: torch.rand(*s, generator=g) / J  # noqa: E731
    return {"r_layout": torch.eye(T) + rnd(S, T, T).tril(), "r_appearance": torch.eye(A) + rnd(S, A, A), "l2a": rnd(max(n, 1), S, T, A),
            "a2l": rnd(max(n, 1), S, A, T), "f_layout": rnd(max(n, 1), S, T, T), "f_appearance": rnd(max(n, 1), 2, S, A, A)}


def _joint_ref(c, n):
    return XR.joint_rollout_dense(c["r_layout"].double(), c["r_appearance"].double(), c["l2a"][:n].double(), c["a2l"][:n].double(), c["f_layout"][:n].double(),
                                  c["f_appearance"][:n].double())


@pytest.mark.parametrize("n_fusion", [0, 1, 3])
@pytest.mark.parametrize("T,A", [(1, 1), (7, 33), (16, 33), (33, 33), (64, 33), (65, 33), (130, 130)])
def test_attn_rollout_joint_vs_fp64_chain_inside_guard_bands(pkg, arena, T, A, n_fusion):
    """S = 1 and 5: <= ROLLOUT_CAP of max|ref| against the dense fp64 chain; plain == arena == second call, bands intact, every element of
    R written; the wrapper gives the same bits."""
    lib = pkg._lib.load()
    J, n, worst, off = T + A, n_fusion, 0.0, 0.0
    for S in (1, 5):
        c = _joint_case(S, T, A, n, seed=13 * T + A + S + n)
        specs = {k: (v.reshape(-1, v.shape[-1]), "in") for k, v in c.items()}
        specs["R"] = (Out((S * J, J)), "out")
        m = lambda o, k: getattr(o, k).ptr if n else None  # noqa: E731
        call = lambda o: lib.stlt_attn_rollout_joint(o.r_layout.ptr, o.r_appearance.ptr, m(o, "l2a"), m(o, "a2l"), m(o, "f_layout"), m(o, "f_appearance"), n,  # noqa: E731
                                                     S, T, A, o.R.ptr, GA.stream())
        got = GA.three_ways(lib, arena, specs, call, ["R"])["R"].view(S, J, J)
        ref = _joint_ref(c, n)
        worst = max(worst, _rel(got, ref))
        assert worst <= ROLLOUT_CAP, (S, T, A, n, worst)
        # (reported only: the same absolute error against max|R - I|, which is far smaller than max|R| here)
        off = max(off, _rel(differenced("fusion_rollout", got.double()), differenced("fusion_rollout", ref)))
        if n == 0:
            assert torch.equal(got, XR.blockdiag(c["r_layout"], c["r_appearance"]))
        dev = {k: v.to(DEV) for k, v in c.items()}
        assert torch.equal(pkg.ops.attn_rollout_joint(dev["r_layout"], dev["r_appearance"], dev["l2a"][:n], dev["a2l"][:n], dev["f_layout"][:n],
                                                      dev["f_appearance"][:n]).cpu(), got)
    _report(f"attn_rollout_joint T={T} A={A} layers={n} worst err / max|ref|, and of R - I", f"{worst:.2e}, {off:.2e}")


@pytest.mark.parametrize("T,A,n", [(7, 33, 2), (65, 33, 1), (5, 3, 0)])
def test_null_initial_rollouts_are_the_identity(pkg, T, A, n):
    S = 3
    c = {k: v.to(DEV) for k, v in _joint_case(S, T, A, n, seed=T).items()}
    maps = [c[k][:n] for k in ("l2a", "a2l", "f_layout", "f_appearance")]
    eye_t, eye_a = torch.eye(T, device=DEV).expand(S, T, T).contiguous(), torch.eye(A, device=DEV).expand(S, A, A).contiguous()
    want = pkg.ops.attn_rollout_joint(eye_t, eye_a, *maps)
    assert torch.equal(pkg.ops.attn_rollout_joint(None, None, *maps), want)
    assert torch.equal(pkg.ops.attn_rollout_joint(eye_t, None, *maps), want) and torch.equal(pkg.ops.attn_rollout_joint(None, eye_a, *maps), want)
    if n == 0:
        assert torch.equal(want, torch.eye(T + A, device=DEV).expand(S, -1, -1))


@pytest.mark.parametrize("w", [(1.0, 0.0), (0.0, 1.0), (1.0, 1.0)])
@pytest.mark.parametrize("B,T,A,N", [(1, 1, 1, 1), (3, 7, 33, 5), (5, 65, 33, 9)])
def test_relevance_combine_joint_vs_fp64_inside_guard_bands(pkg, arena, B, T, A, N, w):
    """the three weightings against the fp64 read-out; a length outside 1 ... T makes that clip's three outputs NaN and nothing else"""
    lib = pkg._lib.load()
    g = torch.Generator().manual_seed(B + T + A + N)
    J = T + A
    Rj, r_sp = torch.rand(B, J, J, generator=g), torch.rand(B, T, N, N, generator=g)
    lengths = torch.randint(1, T + 1, (B,), generator=g)
    if B > 1:
        lengths[1] = T + 1
    if B > 2:
        lengths[2] = 0
    specs = {"R": (Rj.reshape(B * J, J), "in"), "r_sp": (r_sp.reshape(-1, N), "in"), "lengths": (lengths, "extent", 1), "rel": (Out((B * T, N)), "out"),
             "frame_rel": (Out((B, T)), "out"), "app_rel": (Out((B, A)), "out")}
    call = lambda o: lib.stlt_relevance_combine_joint(o.R.ptr, o.r_sp.ptr, o.lengths.ptr, B, T, A, N, w[0], w[1], o.rel.ptr, o.frame_rel.ptr, o.app_rel.ptr,  # noqa: E731
                                                      GA.stream())
    # (GA.three_ways compares with torch.equal, and NaN != NaN: the plain run and the arena run by hand, NaN mapped to -1)
    P = {n: GA.plain(s[0], DEV) for n, s in specs.items()}
    assert call(type("O", (), P)) == 0, GA.last_error(lib)
    torch.cuda.synchronize()
    got = {n: P[n].view.cpu() for n in ("rel", "frame_rel", "app_rel")}
    arena.reset()
    Ar = {n: arena.place(s[0], s[1], band=(s[2] if len(s) > 2 else None), name=n) for n, s in specs.items()}
    assert call(type("O", (), Ar)) == 0, GA.last_error(lib)
    arena.check()
    for n in got:
        assert torch.equal(torch.nan_to_num(Ar[n].view.cpu(), nan=-1.0), torch.nan_to_num(got[n], nan=-1.0)), n
    good = (lengths >= 1) & (lengths <= T)
    rel, frame_rel, app_rel = got["rel"].view(B, T, N), got["frame_rel"], got["app_rel"]
    assert torch.isnan(rel[~good]).all() and torch.isnan(frame_rel[~good]).all() and torch.isnan(app_rel[~good]).all()
    want = XR.read_out(Rj[good].double(), r_sp[good].double(), lengths[good], T, *w)
    for name, a, b in zip(("rel", "frame_rel", "app_rel"), (rel, frame_rel, app_rel), want):
        assert torch.isfinite(a[good]).all() and (b.abs().max().item() == 0 and (a[good] == 0).all() or _rel(a[good], b) <= ROLLOUT_CAP), name
    dev_out = pkg.ops.relevance_combine_joint(Rj.to(DEV), r_sp.to(DEV), lengths.to(DEV), *w)
    for a, b in zip(dev_out, (rel, frame_rel, app_rel)):
        assert torch.equal(torch.nan_to_num(a.cpu(), nan=-1.0), torch.nan_to_num(b, nan=-1.0))


def test_joint_rollout_and_combine_refusals(pkg):
    lib = pkg._lib.load()
    s = GA.stream()
    buf = torch.zeros(4096, device=DEV)
    out = torch.full((4096,), 7.0, device=DEV)
    lengths = torch.tensor([1, 2, 3], device=DEV)
    b, o = buf.data_ptr(), out.data_ptr()
    f = lib.stlt_attn_rollout_joint
    for args, word in (((b, b, b, b, b, b, 1, 2, 0, 3, o, s), "token counts"), ((b, b, b, b, b, b, 1, 2, 3, 257, o, s), "token counts"),
                       ((b, b, b, b, b, b, 65, 2, 3, 3, o, s), "layer count"), ((b, b, b, b, b, b, -1, 2, 3, 3, o, s), "layer count"),
                       ((b, b, b, b, b, b, 1, -1, 3, 3, o, s), "sequence"), ((b, b, None, b, b, b, 1, 2, 3, 3, o, s), "null"),
                       ((b, b, b, b, b, None, 1, 2, 3, 3, o, s), "null"), ((b, b, b, b, b, b, 1, 2, 3, 3, None, s), "null"),
                       ((b + 2, b, b, b, b, b, 1, 2, 3, 3, o, s), "r_layout"), ((b, b, b, b + 2, b, b, 1, 2, 3, 3, o, s), "appearance_to_layout"),
                       ((b, b, b, b, b, b, 1, 2, 3, 3, o + 2, s), "R must")):
        assert f(*args) == EINVAL and word in GA.last_error(lib), (word, GA.last_error(lib))
    g = lib.stlt_relevance_combine_joint
    ln = lengths.data_ptr()
    for args, word in (((None, b, ln, 3, 2, 2, 2, 1.0, 1.0, o, o, o, s), "null"), ((b, b, None, 3, 2, 2, 2, 1.0, 1.0, o, o, o, s), "null"),
                       ((b, b, ln, 3, 2, 2, 2, 1.0, 1.0, o, None, o, s), "null"), ((b, b, ln, 3, 0, 2, 2, 1.0, 1.0, o, o, o, s), "shape"),
                       ((b, b, ln, 3, 2, 0, 2, 1.0, 1.0, o, o, o, s), "shape"), ((b, b, ln, 3, 2, 2, 2, 1.0, 1.0, o, o, o + 2, s), "app_rel"),
                       ((b, b, ln + 4, 3, 2, 2, 2, 1.0, 1.0, o, o, o, s), "lengths")):
        assert g(*args) == EINVAL and word in GA.last_error(lib), (word, GA.last_error(lib))
    torch.cuda.synchronize()
    assert (out == 7.0).all()


# ---- the block call --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["self_causal_16", "cross_16x33", "cross_33x16_masked"])
def test_block_backward_with_a_recorder(pkg, kind):
    """stlt_attn_block_bwd_relevance (AttnBlockFn inside a RelevanceRecorder): dx and dc bit-equal to stlt_attn_block_bwd_train with an
    all-NULL gradient table (AttnBlockFn with every parameter frozen), the map within OP_CAP of the fp64 restatement of the block."""
    S, d, H, eps = 3, 256, 4, 1e-12
    Lq, Lk, causal, cross = {"self_causal_16": (16, 16, True, False), "cross_16x33": (16, 33, False, True), "cross_33x16_masked": (33, 16, False, True)}[kind]
    g = torch.Generator().manual_seed(len(kind))
    x, c = torch.randn(S, Lq, d, generator=g), (torch.randn(S, Lk, d, generator=g) if cross else None)
    dy = torch.randn(S, Lq, d, generator=g)
    kpm = torch.zeros(S, Lk, dtype=torch.bool)
    if kind != "cross_16x33":
        kpm[1, Lk - 5:] = True
        kpm[2, Lk // 2:] = True
    sd = {"attn.in_proj_weight": torch.randn(3 * d, d, generator=g) * 0.05, "attn.in_proj_bias": torch.randn(3 * d, generator=g) * 0.1,
          "attn.out_proj.weight": torch.randn(d, d, generator=g) * 0.05, "attn.out_proj.bias": torch.randn(d, generator=g) * 0.1,
          "ln.weight": 1 + 0.1 * torch.randn(d, generator=g), "ln.bias": 0.1 * torch.randn(d, generator=g)}
    ws = [sd[k].to(DEV) for k in sd]  # (frozen: no requires_grad)

    def run(slot):
        xl = x.to(DEV).requires_grad_(True)
        cl = c.to(DEV).requires_grad_(True) if cross else None
        with (pkg.ops.RelevanceRecorder([slot]) if slot is not None else torch.enable_grad()):
            out = pkg.ops.AttnBlockFn.apply(xl, cl, kpm.to(DEV), causal, H, eps, 0.0, *ws)
        return out, torch.autograd.grad(out, [xl, cl] if cross else [xl], dy.to(DEV))

    out0, grads0 = run(None)
    abar = torch.zeros(S, Lq, Lk, device=DEV)
    out1, grads1 = run(abar)
    assert torch.equal(out0, out1) and all(torch.equal(a, b) for a, b in zip(grads0, grads1))
    # fp64: the block with P a graph node
    sd64 = {k: v.double() for k, v in sd.items()}
    x64 = x.double().requires_grad_(True)
    c64 = c.double() if cross else x64
    nodes = []
    o64 = XR._block(sd64, "", x64, c64, H, eps, kpm, causal, nodes)
    (G,) = torch.autograd.grad((o64 * dy.double()).sum(), nodes[0][0], retain_graph=True)
    ref = R.abar_of(nodes[0][0].detach(), G)
    (dx64,) = torch.autograd.grad((o64 * dy.double()).sum(), x64)
    e_map, e_dx = _rel(abar, ref), _rel(grads1[0], dx64)
    _report(f"block {kind}: abar err / max|ref|, dx err / max|ref|", f"{e_map:.2e}, {e_dx:.2e}")
    assert ref.abs().max().item() > 0 and e_map <= OP_CAP and e_dx <= 2e-4
    assert (abar.cpu()[FR.masked_entries(kpm, causal, S, Lq, Lk)] == 0).all()


# ---- the sweep with STLT_FLAG_TRAIN_BACKBONE ---------------------------------------------------------------------------------------------
def _model(pkg, model_name, sd):
    m = pkg.models_factory[model_name](pkg.MultimodalModelConfig(**dict(pkg.synth.model_kwargs("cfg1"), **EXTRA)))
    m.load_state_dict(sd, strict=True)
    m.train(False)
    return m.to(DEV)


def test_backbone_flag_sweep_vs_fp64_restatement(pkg):
    """stlt_train_backward_relevance with STLT_FLAG_TRAIN_BACKBONE from a random (B,T,d) seed at cfg1: every layout map and both rollouts
    against the restatement's layout branch; a relevance sink is refused in that mode, the maps untouched."""
    lib, L = pkg._lib.load(), pkg._lib
    sd, batch, _, _, _ = reference("caf", "caf", "top1")
    m = _model(pkg, "caf", sd)
    lb = m.caf_backbone.layout_branch
    dev = _to(batch)
    B, T, N = batch["categories"].shape
    H = pkg.synth.CONFIGS["cfg1"]["num_attention_heads"]
    out, step = lb._train_forward(dev, None, L.FLAG_TRAIN_BACKBONE)
    seed = GA.rand(B, T, out.shape[-1], seed=77)
    maps = lb._train_relevance(step, seed.to(DEV))
    assert set(maps) == {"spatial_layers", "temporal_layers", "spatial_rollout", "temporal_rollout"}
    sd64 = {k: (v.double() if v.is_floating_point() else v) for k, v in sd.items()}
    b64 = {k: (v.double() if v.is_floating_point() else v) for k, v in batch.items()}
    b64["boxes"] = b64["boxes"].clone().requires_grad_(True)
    spatial, temporal = [], []
    g = XR._layout(sd64, "caf_backbone.layout_branch.", b64, H, 1e-12, spatial, temporal)
    assert (out.cpu().double() - g.detach()).abs().max().item() <= LOGIT_TOL
    G = torch.autograd.grad((g * seed.double()).sum(), [P for P, _, _ in spatial + temporal])
    sp = [R.abar_of(P.detach(), q) for (P, _, _), q in zip(spatial, G)]
    tp = [R.abar_of(P.detach(), q) for (P, _, _), q in zip(temporal, G[len(spatial):])]
    want = {"spatial_layers": torch.stack(sp).reshape(-1, B, T, N, N), "temporal_layers": torch.stack(tp),
            "spatial_rollout": R.rollout(sp).reshape(B, T, N, N), "temporal_rollout": R.rollout(tp)}
    errs = {k: _rel(differenced(k, maps[k].cpu().double()), differenced(k, want[k])) for k in want}
    _report(f"backbone-flag sweep err / max|ref| (bound {CAP:.1e})", ", ".join(f"{k} {v:.2e}" for k, v in errs.items()))
    assert all(v <= CAP for v in errs.values()), errs
    # the refusal
    outs = {k: torch.full_like(v, 7.0) for k, v in maps.items()}
    rel = torch.full((B, T, N), 7.0, device=DEV)
    p, _, _ = lb.c_params(None)
    d = lb.config.hidden_size
    tape = lb._train_buf("tape", int(lib.stlt_train_tape_bytes(B, T, N, d, p.n_spatial, p.n_temporal)), out.device)
    scratch = lb._train_buf("scratch", int(lib.stlt_train_scratch_bytes(B, T, N, d, p.n_categories)), out.device)
    sink = L.RelevanceMaps(outs["spatial_layers"].data_ptr(), outs["temporal_layers"].data_ptr(), outs["spatial_rollout"].data_ptr(),
                           outs["temporal_rollout"].data_ptr(), rel.data_ptr())
    sdev = seed.to(DEV)
    rc = lib.stlt_train_backward_relevance(C.byref(p), C.byref(step["inp"]), tape.data_ptr(), tape.numel(), scratch.data_ptr(), scratch.numel(), sdev.data_ptr(),
                                           0.0, 0, L.FLAG_TRAIN_BACKBONE, None, C.byref(sink), GA.stream())
    assert rc == EINVAL and "relevance must be NULL" in GA.last_error(lib)
    torch.cuda.synchronize()
    assert (rel == 7.0).all() and all((v == 7.0).all() for v in outs.values())


# ---- the whole path --------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _run(pkg, model_name, head, form):
    """(model, device batch, CPU batch, target, fp64 reference, forward_relevance's output with the per-layer maps) of a case, once"""
    sd, batch, z, target, ref = reference(model_name, head, form)
    m = _model(pkg, model_name, sd)
    dev = _to(batch)
    out = m.forward_relevance(dev, None if target is None else target.to(DEV), head=head, return_layers=True)
    return m, dev, batch, target, ref, out


@pytest.mark.parametrize("model_name,head,form", WHOLE_PATH_CASES)
def test_forward_relevance_vs_fp64_restatement(pkg, model_name, head, form):
    m, dev, batch, target, ref, out = _run(pkg, model_name, head, form)
    B, T, N = batch["categories"].shape
    A = EXTRA["appearance_num_frames"] + 1
    names = XR.HEADS[model_name]
    assert set(out) == set(names) | {"target"} | set(XR.OUTPUT_KEYS) | set(XR.LAYER_KEYS)
    assert out["relevance"].shape == (B, T, N) and out["frame_relevance"].shape == (B, T) and out["appearance_relevance"].shape == (B, A)
    assert out["fusion_rollout"].shape == (B, T + A, T + A)
    keys = XR.OUTPUT_KEYS + XR.LAYER_KEYS
    assert all(out[k].dtype == torch.float32 and torch.isfinite(out[k]).all() and tuple(out[k].shape) == tuple(ref[k].shape) for k in keys)
    with torch.no_grad():
        fwd = m(dev)
    e_fwd = max((fwd[k] - out[k]).abs().max().item() for k in names)
    e_ref = max((out[k].cpu().double() - ref[k]).abs().max().item() for k in names)
    assert e_fwd <= LOGIT_TOL and e_ref <= LOGIT_TOL
    if form == "seed":
        assert torch.equal(out["target"].cpu(), target)
    else:
        assert torch.equal(out["target"].cpu(), ref["target"])
    errs = {}
    for k in keys:
        want = differenced(k, ref[k])
        got = differenced(k, out[k].cpu().double())
        if want.numel() == 0 or want.abs().max().item() == 0:  # a map the head does not reach (or LCF's empty fusion maps): exactly 0
            assert (got == 0).all(), k
        else:
            errs[k] = _rel(got, want)
    _report(f"forward_relevance {model_name}/{head}/{form} err / max|ref| (bound {CAP:.1e}); logits vs forward {e_fwd:.2e}, vs fp64 {e_ref:.2e}",
            ", ".join(f"{k} {v:.2e}" for k, v in errs.items()))
    assert all(v <= CAP for v in errs.values()), errs
    # exact zeros: masked entries, padded frames and object slots, the maps of blocks the head does not read
    kpm = batch["src_key_padding_mask_frames"].bool()
    assert (out["temporal_layers"].cpu()[:, FR.masked_entries(kpm, True, B, T, T)] == 0).all()
    assert (out["appearance_to_layout_layers"].cpu()[:, FR.masked_entries(kpm, False, B, A, T)] == 0).all()
    assert (out["fusion_layout_layers"].cpu()[:, FR.masked_entries(kpm, True, B, T, T)] == 0).all()
    pad = R.padded_entries(batch)
    assert pad.any() and (out["relevance"].cpu()[pad] == 0).all() and (out["frame_relevance"].cpu()[kpm] == 0).all()
    for k in XR.LAYER_KEYS:
        if k not in reached(model_name, head):
            assert (out[k] == 0).all(), k
    # without return_layers: the same bits, no per-layer keys
    short = m.forward_relevance(dev, None if target is None else target.to(DEV), head=head)
    assert set(short) == set(names) | {"target"} | set(XR.OUTPUT_KEYS) and all(torch.equal(short[k], out[k]) for k in XR.OUTPUT_KEYS + names)


@pytest.mark.parametrize("model_name,head,form", [("caf", "caf", "top1"), ("cacnf", "ensemble", "top1"), ("cacnf", "stlt", "top1"), ("lcf", "lcf", "seed")])
def test_layers_through_the_ops_reproduce_the_one_call_result(pkg, model_name, head, form):
    """The per-layer maps pushed through the ops: the one-call rollouts and relevances, bit for bit."""
    m, dev, _, _, _, out = _run(pkg, model_name, head, form)
    r_sp, r_tp, r_app = (pkg.ops.attn_rollout(out[k]) for k in ("spatial_layers", "temporal_layers", "appearance_layers"))
    assert torch.equal(r_sp, out["spatial_rollout"]) and torch.equal(r_tp, out["temporal_rollout"]) and torch.equal(r_app, out["appearance_rollout"])
    Rj = pkg.ops.attn_rollout_joint(r_tp, r_app, out["layout_to_appearance_layers"], out["appearance_to_layout_layers"], out["fusion_layout_layers"],
                                    out["fusion_appearance_layers"])
    assert torch.equal(Rj, out["fusion_rollout"])
    got = pkg.ops.relevance_combine_joint(Rj, r_sp, dev["lengths"], *XR.WEIGHTS.get(head, (1.0, 1.0)))
    assert all(torch.equal(a, out[k]) for a, k in zip(got, ("relevance", "frame_relevance", "appearance_relevance")))


def test_forward_relevance_leaves_no_state_behind(pkg):
    """forward, forward_attention and forward_saliency give the same bits before and after; no parameter gets a .grad or changes its
    requires_grad; two calls give the same bits; a training step after the call is the step of a model that never made it."""
    sd, batch, _, _, _ = reference("cacnf", "ensemble", "top1")
    dev = _to(batch)
    m = _model(pkg, "cacnf", sd)

    def others():
        with torch.no_grad():
            return {"forward": m(dev), "attention": m.forward_attention(dev), "saliency": m.forward_saliency(dev)}

    before = others()
    flags = [q.requires_grad for q in m.parameters()]
    first = m.forward_relevance(dev, return_layers=True)
    after = others()
    for call, outs in before.items():
        for k, v in outs.items():
            assert torch.equal(v, after[call][k]), (call, k)
    assert all(q.grad is None for q in m.parameters()) and flags == [q.requires_grad for q in m.parameters()]
    second = m.forward_relevance(dev, return_layers=True)
    assert all(torch.equal(first[k], second[k]) for k in first)
    assert pkg.ops.RelevanceRecorder._active is None

    def step(model, with_call):
        if with_call:
            model.forward_relevance(dev)
        labels = torch.randint(0, sd["fusion_classifier.fc2.bias"].shape[0], (batch["categories"].shape[0],), generator=torch.Generator().manual_seed(0))
        trainer = pkg.train.Trainer(model.train(True), "something", learning_rate=5e-5, warmup_steps=0, total_steps=10)
        torch.manual_seed(3)
        res = trainer.step(dict(dev, labels=labels.to(DEV)))
        return float(res["loss"]), float(res["grad_norm"]), [q.detach().clone() for q in model.parameters()]

    a, b = step(m, True), step(_model(pkg, "cacnf", sd), False)
    assert a[0] == b[0] and a[1] == b[1] and all(torch.equal(p, q) for p, q in zip(a[2], b[2]))


def test_forward_relevance_refusals(pkg):
    sd, batch, _, _, _ = reference("cacnf", "ensemble", "top1")
    m = _model(pkg, "cacnf", sd)
    dev = _to(batch)
    with pytest.raises(pkg.StltHipError, match="CPU tensors"):
        m.forward_relevance(batch)
    m.backbone.layout_branch.skip_padding = True
    with pytest.raises(pkg.StltHipError, match="skip_padding"):
        m.forward_relevance(dev)
    m.backbone.layout_branch.skip_padding = False
    with pytest.raises(pkg.StltHipError, match="head must be one of"):
        m.forward_relevance(dev, head="lcf")
    with pytest.raises(pkg.StltHipError, match="appearance_features"):
        m.forward_relevance({k: v for k, v in dev.items() if k != "appearance_features"})
    with pytest.raises(pkg.StltHipError, match="target"):
        m.forward_relevance(dev, target=torch.zeros(5, dtype=torch.int64, device=DEV))
    m.train(True)
    with pytest.raises(pkg.StltHipError, match="training mode"):
        m.forward_relevance(dev)
    m.train(False)
    assert set(m.forward_relevance(dev)) >= {"relevance", "fusion_rollout"}  # and the model still answers


def test_transformer_resnet_forward_relevance(pkg):
    """The appearance-only model on the r3d_transformer fixture's shapes: the appearance encoder's maps and rollout against the restatement
    on the trunk's own features; appearance_relevance is the CLS row of the rollout."""
    import json
    import os

    from conftest import GOLDEN
    meta = json.load(open(os.path.join(GOLDEN, "r3d_schema.json")))
    kw = pkg.synth.model_kwargs("cfg1")
    cfg = pkg.AppearanceModelConfig(num_classes=kw["num_classes"], hidden_size=kw["hidden_size"], num_attention_heads=kw["num_attention_heads"],
                                    hidden_dropout_prob=0.0, appearance_num_frames=32)
    m = pkg.TransformerResnet(cfg)
    sd = pkg.synth.make_r3d_state_dict({k: tuple(v.shape) for k, v in m.state_dict().items()}, seed=meta["weight_seed"])
    m.load_state_dict(sd, strict=True)
    m = m.to(DEV).train(False)
    video = pkg.synth.make_video(meta["clips"], seed=meta["video_seed"]).to(DEV)
    out = m.forward_relevance({"video_frames": video}, return_layers=True)
    again = m.forward_relevance({"video_frames": video}, return_layers=True)
    assert set(out) == {"resnet3d", "target", "appearance_rollout", "appearance_relevance", "appearance_layers"}
    assert all(torch.equal(out[k], again[k]) for k in out) and all(q.grad is None for q in m.parameters())
    with torch.no_grad():
        feats = m.resnet.forward_features({"video_frames": video})
        assert (m({"video_frames": video})["resnet3d"] - out["resnet3d"]).abs().max().item() <= LOGIT_TOL
    H = kw["num_attention_heads"]
    sd64 = {k: v.double() for k, v in sd.items() if not k.startswith("resnet.") and v.is_floating_point()}
    nodes = []
    x = XR._appearance(sd64, "", feats.cpu().double().requires_grad_(True), H, nodes)
    logits = x[:, 0] @ sd64["classifier.weight"].t() + sd64["classifier.bias"]
    seed = torch.nn.functional.one_hot(out["target"].cpu(), logits.shape[1]).double()
    G = torch.autograd.grad((logits * seed).sum(), [P for P, _, _ in nodes])
    layers = [R.abar_of(P.detach(), g) for (P, _, _), g in zip(nodes, G)]
    want = {"appearance_layers": torch.stack(layers), "appearance_rollout": R.rollout(layers)}
    errs = {k: _rel(differenced(k, out[k].cpu().double()), differenced(k, want[k])) for k in want}
    _report(f"TransformerResnet.forward_relevance err / max|ref| (bound {CAP:.1e})", ", ".join(f"{k} {v:.2e}" for k, v in errs.items()))
    assert all(v <= CAP for v in errs.values()) and want["appearance_layers"].max().item() > 0
    assert torch.equal(out["appearance_relevance"], out["appearance_rollout"][:, 0, :])
