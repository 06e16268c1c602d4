"""Cases, fp64 references and torch-fp32 yardsticks that hold the explanation kernels to fp32 error off the unit scale: attention maps
(attn_probs, packed and cross), gradient-weighted maps (attn_grad_probs, packed and cross), probe attention (attn_prefix_probe), the rollouts and read-outs (attn_rollout,
attn_rollout_joint, relevance_combine, relevance_combine_joint), Grad-CAM (cam_weights, cam_map, cam_upsample), the input-gradient
product of the embeddings (embed_bwd_inputs), the cell pools, the perturbation curves and the
attribution sum of ig_delta.  tests/test_explain_scale_gpu.py runs the kernels on them, tests/test_explain_scale_cpu.py
holds THEM to their own conditions and shows on fp32 emulations that the rule rejects the lazy forms.  Plain torch on the CPU, no
package import, no GPU.

The metric is the one of tests/scale_cases.py (u = 2^-24, a row passes at e_k <= 4 * max(E_t, u), a zero row must be exactly zero; out /
judge / conditions / row_errors are reused, and so are its attention reference `attention`, the q / k scales ATTN_QK and the rise
ATTN_RISE).  One launch holds rows of very different magnitudes: one scale per sequence, clip or item, another per head.  Rows:
  * attention maps: one query row of one head (per head) or of the head average.  Heads of one sequence have different q / k scales.
  * probe attention: one probe's context in one head.
  * rollouts: one row of one item's R; read-outs: one clip's relevance.
  * cam_weights: the alphas of one clip within one channel group (a short group repeats its first element: `index`); cam_map and
    cam_upsample: one clip's map; cell_pool_abs / cell_pool_sum: one clip's cells; perturb_curve: one clip's curve over the steps.
  * embed_bwd_inputs: one output element — one token against one weight column, each column having a scale of its own (the product rule
    of tests/product_cases.py with a block of one column), held to max(E_t, E_c) with E_c the in-order chain of product_cases.

Where the cases leave the plain recipe "rows of every magnitude", they say so:
  * q / k at scale 17 (score std near 300) are rounded to multiples of 1/2, as scale_cases.attention_case does and for its reason; at
    head dims other than 64 the factor 1 / sqrt(dh) then still rounds the scores once (E_t stays below 256 u on the row metric, which a
    probability far below the row's maximum does not move).
  * the kernels' domain: softmax16 takes -1e30 for a masked score and "> -1e29" for a visible one, so every visible score here lies
    above -1e29 by 26 orders of magnitude (the largest |score| is near 2000), and exp(score - max) below 2^-126 counts as 0 in every
    implementation compared: the selected-tail rows keep their positive gradients 20 to 40 below the peak, where exp is 4e-18 .. 2e-9.
  * the selected-tail sequence has exact scores (q = 4 e_0, k_j = 2 t_j e_0 + free columns that q does not see, t_j multiples of 1/8,
    1 / sqrt(64) exact) and gradients of one product (dctx and v are zero outside column 0 of each head), so the row measures exp at
    s - m = -20 .. -40 alone; at head dim 20 the scale rounds and E_t says how much.
  * the sequences with a peaked head (q / k 5.5 or 17: sequences 1 to 3) have non-negative v and dctx, so G > 0 and a row's largest
    element sits at its peak key.  With signed gradients some peak has a negative one and the row's largest element lies 30 and more
    below it, where the rounding of free fp32 scores alone is a relative error of 30 u and more: torch's own E_t was 527 u there.  That
    row is the selected-tail sequence, with exact scores.
  * v and dctx: the large v goes with the flat softmax, the small with the peaked one (scale_cases.ATTN_V), dctx the other way round.
  * rollout maps are non-negative, like the maps the kernels are fed; every product of a read-out stays a normal fp32 number
    (map scales 1e-6 .. 30 over 4 layers: R between 1e-12 and 1e6).
  * cam_map of the clip at gradient scale 1e-8 with HiResCAM: products of 1e-8 stay normal numbers; no clip has all-zero activations.
"""
import functools
import math

import torch
import torch.nn.functional as F

import product_cases as PC
import scale_cases as SC
from scale_cases import MARGIN, U, YARD_CAP, judge, out, row_errors, yardstick  # noqa: F401  (the metric, not a copy of it)

H = 2
TAIL_BAND = (20.0, 40.0)   # how far below the peak the keys with a positive gradient lie


def indexed(values, index):
    """values (any shape) -> rows (len(index), width) by a flat index table: a ragged partition as padded rows (a short row repeats its first element)."""
    return values.detach().cpu().double().reshape(-1)[index]


def _index_of(members, n):
    width = max(len(m) for m in members)
    idx = torch.stack([torch.cat([m, m[:1].expand(width - len(m))]) for m in members])
    assert sorted(set(idx.reshape(-1).tolist())) == list(range(n))  # every element is in a row
    return idx


# ---- attention maps ------------------------------------------------------------------------------------------------------------------
PACKED_SHAPES = ((7, 64), (17, 64), (64, 64), (7, 20), (65, 64))            # (L, dh): mfma-diag, mfma-full (2 and 4 key blocks), generic, generic
CROSS_SHAPES = ((7, 33, 64, 1), (33, 17, 64, 1), (16, 65, 64, 1), (7, 33, 64, 16), (17, 17, 64, 1), (7, 33, 20, 1))  # (Lq, Lk, dh, repeats of the sequences)
N_SEQ = 8
V_SCALES = SC.ATTN_V                   # by q / k scale of head 0: (1e3, 1, 1e-3, 1)
DCTX_SCALES = (1e-3, 1.0, 1e3, 1.0)


@functools.lru_cache(maxsize=None)
def attention_map_case(Lq, Lk, dh, causal, reps=1):
    """Eight sequences (times `reps`: the same sequences again, for launches that need many units):
      0-3  head h has the q / k scale ATTN_QK[(s + h) % 4] (score std 1e-3, 2, 30, 300; 17 rounded to halves), v and dctx of the scales that
           go with head 0's; in sequence 1 the values of head 1 are 1e-3 of head 0's (heads of different magnitude inside one average);
      4    scores rising along the keys by ATTN_RISE;
      5    every key masked (exact zeros);
      6    a single visible key (probability exactly 1 on it; causal: key 0, so that every query sees it);
      7    the selected tail: the peak key 0 has score 0 and a negative gradient, every other key lies 20 to 40 below and four in five of
           them have a positive gradient: the row's largest element is p_j g_j with p_j = exp(-20 .. -40).
    30 % of the keys of sequences 0-4 and 7 are masked, key 0 never.  Packed (Lq == Lk): q, k, v are the thirds of one buffer.
    Outputs: "probabilities per head" (S, H, Lq, Lk), "probabilities" (S, Lq, Lk), "abar" (S, Lq, Lk) = mean_h max(P_h G_h, 0)."""
    S, d = N_SEQ, H * dh
    g = SC._gen("explain attention", Lq, Lk, dh, causal)
    q, k, v = torch.randn(S, Lq, d, generator=g), torch.randn(S, Lk, d, generator=g), torch.randn(S, Lk, d, generator=g)
    dctx = torch.randn(S, Lq, d, generator=g)
    head = lambda t, s, h: t[s, :, h * dh:(h + 1) * dh]  # noqa: E731
    names = []
    for s in range(4):
        per_head = []
        for h in range(H):
            a = SC.ATTN_QK[(s + h) % 4]
            head(q, s, h).mul_(a)
            head(k, s, h).mul_(a)
            if a == 17.0:
                head(q, s, h).copy_(torch.round(head(q, s, h) * 2) / 2)
                head(k, s, h).copy_(torch.round(head(k, s, h) * 2) / 2)
            per_head.append(f"q/k {a:g}")
        v[s] *= V_SCALES[s]
        dctx[s] *= DCTX_SCALES[s]
        if s >= 1:  # a peaked head: see the module docstring
            v[s], dctx[s] = v[s].abs(), dctx[s].abs()
        names.append(per_head)
    head(v, 1, 1).mul_(1e-3)
    u = torch.randn(d, generator=g)
    u = u / u.reshape(H, -1).norm(dim=1).repeat_interleave(dh)  # unit length inside each head
    rise = math.sqrt(SC.ATTN_RISE * math.sqrt(dh))
    q[4] = 0.1 * q[4] + rise * u
    k[4] = 0.1 * k[4] + rise * u * (torch.arange(Lk) / max(Lk - 1, 1))[:, None]
    names += [["scores rising along the keys"] * H, ["every key masked"] * H, ["a single visible key"] * H, ["selected tail"] * H]
    # the selected tail
    t = -(TAIL_BAND[0] + torch.round(torch.rand(H, Lk, generator=g) * (TAIL_BAND[1] - TAIL_BAND[0]) * 8) / 8)
    t[:, 0] = 0.0
    sign = torch.where(torch.rand(H, Lk, generator=g) < 0.8, 1.0, -1.0)
    sign[:, 0] = -1.0
    sign[:, 1:2] = 1.0  # at least one positive key (when Lk > 1)
    amp = 0.5 + 1.5 * torch.rand(H, Lk, generator=g)
    q[7], k[7] = 0.0, torch.round(k[7] * 2) / 2
    v[7], dctx[7] = 0.0, 0.0  # G = dctx_0 v_0, one product: 63 more terms would each round at G's magnitude (E_t = 5 - 11 u, all of it G's)
    for h in range(H):
        head(q, 7, h)[:, 0] = 4.0
        head(k, 7, h)[:, 0] = (t[h] * (math.sqrt(dh) / 4.0)).float()
        head(v, 7, h)[:, 0] = sign[h] * amp[h]
        head(dctx, 7, h)[:, 0] = 0.5 + 1.5 * torch.rand(Lq, generator=g)
    kpm = torch.rand(S, Lk, generator=g) < 0.3
    kpm[:, 0] = False
    kpm[5, :] = True
    kpm[6, :] = True
    kpm[6, 0 if causal else Lk // 2] = False
    v[6], dctx[6] = v[6].abs(), dctx[6].abs()  # a row of one element: its gradient must not cancel (signed: E_t = 309 u)
    if Lk > 1:
        kpm[7, 1] = False
    if reps > 1:
        q, k, v, dctx, kpm = (x.repeat(reps, *[1] * (x.dim() - 1)) for x in (q, k, v, dctx, kpm))
        names = names * reps
        S = S * reps
    res = {}
    for dt in (torch.float64, torch.float32):
        _, pr = SC.attention(q.to(dt), k.to(dt), v.to(dt), kpm, causal, H)
        sp = lambda x: x.to(dt).reshape(S, -1, H, dh).transpose(1, 2)  # noqa: E731
        grad = sp(dctx) @ sp(v).transpose(-1, -2)
        res[dt] = (pr, (pr * grad).clamp_min(0.0).mean(1))
    per_head = [n for seq in names for n in seq for _ in range(Lq)]
    mean = [" | ".join(seq) if seq[0] != seq[1] else seq[0] for seq in names for _ in range(Lq)]
    outs = {"probabilities per head": out(SC.rows(res[torch.float64][0], S * H * Lq), res[torch.float32][0], per_head),
            "probabilities": out(SC.rows(res[torch.float64][0].mean(1), S * Lq), res[torch.float32][0].mean(1), mean),
            "abar": out(SC.rows(res[torch.float64][1], S * Lq), res[torch.float32][1], mean)}
    return {"q": q, "k": k, "v": v, "dctx": dctx, "kpm": kpm, "causal": causal, "H": H, "dh": dh, "outs": outs}


def lazy_softmax_probs(case, shifted):
    """Head-averaged probabilities in fp32 with (shifted) or without the row maximum subtracted before exp."""
    q, k, kpm = case["q"], case["k"], case["kpm"]
    S, Lq, d = q.shape
    dh = case["dh"]
    sp = lambda x: x.reshape(S, -1, H, dh).transpose(1, 2)  # noqa: E731
    sc = sp(q) @ sp(k).transpose(-1, -2) / math.sqrt(dh)
    masked = kpm[:, None, None, :].expand(S, H, Lq, k.shape[1])
    if case["causal"]:
        masked = masked | torch.ones(Lq, k.shape[1], dtype=torch.bool).triu(1)
    sc = sc.masked_fill(masked, -math.inf)
    if shifted:
        sc = sc - sc.amax(-1, keepdim=True).clamp_min(-1e30)
    e = torch.exp(sc)
    return torch.nan_to_num(e / e.sum(-1, keepdim=True), nan=0.0).mean(1)


def fast_exp(x, exact):
    """exp(x) for x <= 0 in fp32 as exp2 of x * log2(e): the product rounded to fp32 (`exact` False: the native exp of the matrix-core
    kernels as they were), or carried with its rounding error and log2(e)'s own, exp2(t) * (1 + r ln 2) (the form they have now).  exp2
    itself is taken in fp64 and rounded once: the hardware instruction's 1 ulp is not what is shown here."""
    log2e = torch.tensor(1.4426950408889634, dtype=torch.float32)
    t = x * log2e
    main = torch.exp2(t.double()).float()
    if not exact:
        return main
    r = (x.double() * 1.4426950408889634 - t.double()).float()
    return main * (1.0 + r * torch.tensor(0.6931471805599453, dtype=torch.float32))


def lazy_exp_abar(case, exact):
    """abar in fp32 with the stabilised softmax whose exp is fast_exp."""
    q, k, v, dctx, kpm = case["q"], case["k"], case["v"], case["dctx"], case["kpm"]
    S, Lq, d = q.shape
    dh = case["dh"]
    sp = lambda x: x.reshape(S, -1, H, dh).transpose(1, 2)  # noqa: E731
    sc = sp(q) @ sp(k).transpose(-1, -2) * torch.tensor(1.0 / math.sqrt(dh), dtype=torch.float32)
    masked = kpm[:, None, None, :].expand(S, H, Lq, k.shape[1])
    if case["causal"]:
        masked = masked | torch.ones(Lq, k.shape[1], dtype=torch.bool).triu(1)
    m = sc.masked_fill(masked, -1e30).amax(-1, keepdim=True)
    e = torch.where(masked, torch.zeros(()), fast_exp((sc - m).clamp_max(0.0), exact))
    s = e.sum(-1, keepdim=True)
    p = e * torch.where(s > 0, 1.0 / s, torch.zeros(()))
    return (p * (sp(dctx) @ sp(v).transpose(-1, -2))).clamp_min(0.0).mean(1)


# ---- probe attention -------------------------------------------------------------------------------------------------------------------
PROBE_SHAPES = ((64, 17), (64, 65), (25, 7))   # (dh, T): 65 frames: a second key tile; 25: the one-float loads


def probe_attention(qkv_f, qkv_p, kpm):
    """Probe (s, t) attends to the frame keys j < t that are not masked and to its own key, one softmax: qkv_f, qkv_p (S, T, 3d) -> ctx (S, T, d)"""
    S, T, d3 = qkv_p.shape
    d = d3 // 3
    dh = d // H
    sp = lambda z: z.reshape(S, T, H, dh).transpose(1, 2)  # noqa: E731
    _, kf, vf = [sp(z) for z in qkv_f.split(d, -1)]
    qp, kp, vp = [sp(z) for z in qkv_p.split(d, -1)]
    seen = torch.tril(torch.ones(T, T, dtype=torch.bool), diagonal=-1)[None] & ~kpm[:, None, :]
    s = ((qp @ kf.transpose(-1, -2)) / math.sqrt(dh)).masked_fill(~seen[:, None], -math.inf)
    s_self = (qp * kp).sum(-1, keepdim=True) / math.sqrt(dh)
    pr = torch.softmax(torch.cat([s, s_self], -1), -1)
    return (pr[..., :T] @ vf + pr[..., T:] * vp).transpose(1, 2).reshape(S, T, d)


@functools.lru_cache(maxsize=None)
def probe_case(dh, T):
    """stlt_attn_prefix_probe_fwd on six clips: four whose head h has the q / k scale ATTN_QK[(s + h) % 4] (17 rounded to halves) and values
    of the scale that goes with head 0's, one with rising scores, one with every frame masked (a probe then sees its own key alone and
    returns its own value).  30 % of the frames of the others are masked.  A row is one probe's context in one head."""
    S, d = 6, H * dh
    g = SC._gen("explain probe", dh, T)
    f, p = torch.randn(S, T, 3, d, generator=g), torch.randn(S, T, 3, d, generator=g)
    names = []
    for s in range(4):
        per_head = []
        for h in range(H):
            a = SC.ATTN_QK[(s + h) % 4]
            for t in (f[s, :, 1], p[s, :, 0], p[s, :, 1]):   # frame keys, probe queries and keys
                t[:, h * dh:(h + 1) * dh] *= a
                if a == 17.0:
                    t[:, h * dh:(h + 1) * dh] = torch.round(t[:, h * dh:(h + 1) * dh] * 2) / 2
            per_head.append(f"q/k {a:g} v {V_SCALES[s]:g}")
        f[s, :, 2] *= V_SCALES[s]
        p[s, :, 2] *= V_SCALES[s]
        names.append(per_head)
    u = torch.randn(d, generator=g)
    u = u / u.reshape(H, -1).norm(dim=1).repeat_interleave(dh)
    rise = math.sqrt(SC.ATTN_RISE * math.sqrt(dh))
    ramp = (torch.arange(T) / max(T - 1, 1))[:, None]
    p[4, :, 0] = 0.1 * p[4, :, 0] + rise * u
    f[4, :, 1] = 0.1 * f[4, :, 1] + rise * u * ramp
    p[4, :, 1] = 0.1 * p[4, :, 1] + rise * u * ramp
    names += [["scores rising along the keys"] * H, ["every frame masked"] * H]
    kpm = torch.rand(S, T, generator=g) < 0.3
    kpm[5, :] = True
    qkv_f, qkv_p = f.reshape(S, T, 3 * d), p.reshape(S, T, 3 * d)
    head_rows = lambda c: c.reshape(S, T, H, dh).transpose(1, 2).reshape(S * H * T, dh)  # noqa: E731
    ref, yard = probe_attention(qkv_f.double(), qkv_p.double(), kpm), probe_attention(qkv_f, qkv_p, kpm)
    return {"qkv_f": qkv_f, "qkv_p": qkv_p, "kpm": kpm, "head_rows": head_rows,
            "outs": {"ctx": out(head_rows(ref), head_rows(yard), [n for seq in names for n in seq for _ in range(T)])}}


# ---- rollouts and read-outs ------------------------------------------------------------------------------------------------------------
MAP_SCALES = (1e-6, 1e-2, 1.0, 30.0)
MIXED = (1e-2, 30.0, 1e-6, 1.0)   # the layers' scales of the last item
N_LAYERS, N_FUSION = 4, 2
ROLLOUT_L = (7, 64, 65)           # 64 / 65: every column in one workgroup / blocks of 16 columns
JOINT_SHAPES = ((7, 33), (65, 33))
N_OBJ = 5
W_LAYOUT, W_APPEARANCE = 0.7, 0.3


def _item_names():
    return [f"maps {s:g}" for s in MAP_SCALES] + ["layers of mixed scales"]


def _maps(g, n, rows, cols):
    """(n, 5 items, rows, cols) non-negative maps with row sums near scale / 2; item 4 has another scale in every layer"""
    m = torch.rand(n, len(MAP_SCALES) + 1, rows, cols, generator=g) / cols
    for i, s in enumerate(MAP_SCALES):
        m[:, i] *= s
    for l in range(n):
        m[l, -1] *= MIXED[l % len(MIXED)]
    return m


def chain_from_old(A, R):
    """One rollout step in fp32 the way the kernels had it: every element's FMA chain starts from the old R[i,j] and the L products join it
    one rounding at a time, k ascending."""
    acc = R.clone()
    for k in range(A.shape[-1]):
        acc = (acc.double() + A[..., :, k:k + 1].double() * R[..., k:k + 1, :].double()).float()
    return acc


def chain_added_last(A, R):
    """... and the way they have it now: the chain starts from zero and the old R[i,j] is added once, last."""
    acc = torch.zeros_like(R)
    for k in range(A.shape[-1]):
        acc = (acc.double() + A[..., :, k:k + 1].double() * R[..., k:k + 1, :].double()).float()
    return R + acc


def rollout_by(step, abar):
    S, L = abar.shape[1], abar.shape[-1]
    R = torch.eye(L, dtype=abar.dtype).expand(S, L, L).clone()
    for a in abar:
        R = step(a, R)
    return R


@functools.lru_cache(maxsize=None)
def rollout_case(L):
    """attn_rollout on 4 layers of five items' maps, and relevance_combine on top: the temporal rollout is this one (T = L), the spatial
    one that of N_OBJ objects per frame with the same item scales; clip b reads frame lengths[b] - 1."""
    g = SC._gen("explain rollout", L)
    abar = _maps(g, N_LAYERS, L, L)
    S = abar.shape[1]
    plain = lambda a, r: r + a @ r  # noqa: E731
    ref, yard = rollout_by(plain, abar.double()), rollout_by(plain, abar)
    names = _item_names()
    outs = {"R": out(SC.rows(ref, S * L), yard, [n for n in names for _ in range(L)])}
    sp = _maps(g, N_LAYERS, N_OBJ, N_OBJ)[:, :, None].expand(-1, -1, L, -1, -1).reshape(N_LAYERS, S * L, N_OBJ, N_OBJ)
    sp = (sp * (0.5 + torch.rand(1, S * L, 1, 1, generator=g))).contiguous()
    rt, rs = ref.float(), rollout_by(plain, sp.double()).float().reshape(S, L, N_OBJ, N_OBJ)
    lengths = torch.tensor([L, 1, (L + 1) // 2, L, max(L - 1, 1)])
    pick = lambda t: t[torch.arange(S), lengths - 1]  # noqa: E731
    rel64, rel32 = pick(rt.double())[:, :, None] * rs.double()[:, :, 0, :], pick(rt)[:, :, None] * rs[:, :, 0, :]
    assert float(rel64[rel64 > 0].min()) > 1e-30 and float(rel64.max()) < 1e30
    outs["relevance"] = out(SC.rows(rel64, S), rel32, names)
    return {"abar": abar, "rt": rt, "rs": rs, "lengths": lengths, "outs": outs}


@functools.lru_cache(maxsize=None)
def joint_case(T, A, given):
    """attn_rollout_joint over J = T + A stacked tokens, 2 fusion layers of three steps each, the branches' rollouts given (R of the
    items' own scales) or NULL (the identity); relevance_combine_joint on top with the head weights 0.7 / 0.3."""
    g = SC._gen("explain joint", T, A, given)
    J, n = T + A, N_FUSION
    l2a, a2l, fl = _maps(g, n, T, A), _maps(g, n, A, T), _maps(g, n, T, T)
    fa = torch.stack([_maps(g, n, A, A), _maps(g, n, A, A)], 1)  # (n, 2, S, A, A)
    S = l2a.shape[1]
    plain = lambda a, r: r + a @ r  # noqa: E731
    r_l = r_a = None
    if given:
        r_l, r_a = rollout_by(plain, _maps(g, 2, T, T).double()).float(), rollout_by(plain, _maps(g, 2, A, A).double()).float()

    def run(dt):
        R = torch.zeros(S, J, J, dtype=dt)
        R[:, :T, :T] = torch.eye(T, dtype=dt) if r_l is None else r_l.to(dt)
        R[:, T:, T:] = torch.eye(A, dtype=dt) if r_a is None else r_a.to(dt)
        for l in range(n):
            for tl, tr, bl, br in ((None, l2a[l], a2l[l], None), (fl[l], None, None, fa[l, 0]), (None, None, None, fa[l, 1])):
                X = torch.zeros(S, J, J, dtype=dt)
                for blk, (r0, c0) in ((tl, (0, 0)), (tr, (0, T)), (bl, (T, 0)), (br, (T, T))):
                    if blk is not None:
                        X[:, r0:r0 + blk.shape[1], c0:c0 + blk.shape[2]] = blk.to(dt)
                R = R + X @ R
        return R

    ref, yard = run(torch.float64), run(torch.float32)
    names = _item_names()
    outs = {"R": out(SC.rows(ref, S * J), yard, [x for x in names for _ in range(J)])}
    R32 = ref.float()
    rs = rollout_by(plain, (_maps(g, 2, N_OBJ, N_OBJ)[:, :, None].expand(-1, -1, T, -1, -1).reshape(2, S * T, N_OBJ, N_OBJ)).double()).float().reshape(S, T, N_OBJ, N_OBJ)
    lengths = torch.tensor([T, 1, (T + 1) // 2, T, max(T - 1, 1)])

    def read(dt):
        R = R32.to(dt)
        row = torch.tensor(W_LAYOUT, dtype=torch.float32).to(dt) * R[torch.arange(S), lengths - 1] + torch.tensor(W_APPEARANCE, dtype=torch.float32).to(dt) * R[:, T]
        return row[:, :T, None] * rs.to(dt)[:, :, 0, :], row[:, :T], row[:, T:]

    r64, r32 = read(torch.float64), read(torch.float32)
    assert all(float(x[x > 0].min()) > 1e-30 and float(x.max()) < 1e30 for x in r64)
    for key, a, b in zip(("relevance", "frame relevance", "appearance relevance"), r64, r32):
        outs[key] = out(SC.rows(a, S), b, names)
    return {"r_layout": r_l, "r_appearance": r_a, "l2a": l2a, "a2l": a2l, "f_layout": fl, "f_appearance": fa, "R32": R32, "rs": rs, "lengths": lengths,
            "outs": outs}


# ---- Grad-CAM ------------------------------------------------------------------------------------------------------------------------------
CAM_P = (1, 31, 32, 33, 100)     # the NDHWC weights cut the positions into chunks of 32
CAM_C = (4, 6, 260)
CAM_LONG = (1000, 6)             # (P, C) of one longer case: 32 chunks; there a single accumulator misses the bar in most groups
CAM_CLIPS = (1e-8, 1.0, 1e6)     # the gradient scale of each clip
CAM_SPREADS = (0.0, 10.0, 100.0)  # channel c has the mean / spread CAM_SPREADS[c % 3]
UPSAMPLE = (((1, 2, 3), (5, 4, 7)), ((2, 4, 4), (8, 16, 16)))
UPSAMPLE_CLIPS = (1e-30, 1.0, 1e30)


def chunked_mean(g):
    """mean over dim 1 of g (B, P, C) in fp32 in the order of cam_weights' NDHWC kernels: chunks of 32 positions, inside a chunk four
    accumulators taking the positions in turn, (a0 + a1) + (a2 + a3), the chunks' partials added in ascending order, one division by P"""
    B, P, C = g.shape
    parts = []
    for p0 in range(0, P, 32):
        acc = [torch.zeros(B, C) for _ in range(4)]
        for i, p in enumerate(range(p0, min(p0 + 32, P))):
            acc[i % 4] = acc[i % 4] + g[:, p]
        parts.append((acc[0] + acc[1]) + (acc[2] + acc[3]))
    total = parts[0]
    if len(parts) > 1:
        total = torch.zeros(B, C)
        for x in parts:
            total = total + x
    return total / P


def single_accumulator_mean(g):
    """mean over dim 1 of g (B, P, C) in fp32 with one accumulator, positions ascending"""
    acc = torch.zeros(g.shape[0], g.shape[2])
    for p in range(g.shape[1]):
        acc = acc + g[:, p]
    return acc / g.shape[1]


@functools.lru_cache(maxsize=None)
def cam_case(P, C, layout):
    """Gradients g and activations a of three clips as (B, P, C) ("ndhwc") or (B, C, P) ("ncdhw"): g = clip scale * (randn + mean / spread
    of the channel's group), a = relu(randn).  Outputs: "alpha" = mean_p g as rows (clip, channel group) through `index`; the maps
    sum_c w a with w = alpha (Grad-CAM; the fp32 rounding of the reference alpha, an input like any other) or w = g (HiResCAM), with and
    without the ReLU, one row per clip."""
    gen = SC._gen("explain cam", P, C)
    B = len(CAM_CLIPS)
    ms = torch.tensor([CAM_SPREADS[c % 3] for c in range(C)])
    g = (torch.randn(B, P, C, generator=gen) + ms) * torch.tensor(CAM_CLIPS)[:, None, None]
    a = torch.randn(B, P, C, generator=gen).clamp_min(0.0)
    a[:, :, 0] += 0.1   # no clip without an activation
    alpha64 = g.double().mean(1)
    w = alpha64.float()
    members = [torch.tensor([b * C + c for c in range(C) if c % 3 == k]) for b in range(B) for k in range(3)]
    index = _index_of(members, B * C)
    group = [f"gradients {s:g} mean/spread {m:g}" for s in CAM_CLIPS for m in CAM_SPREADS]
    outs = {"alpha": out(indexed(alpha64, index), indexed(g.mean(1), index), group)}
    clip = [f"gradients {s:g}" for s in CAM_CLIPS]
    for name, wt in (("grad-cam", w[:, None, :].expand(B, P, C)), ("hirescam", g)):
        r64, r32 = (wt.double() * a.double()).sum(-1), (wt * a).sum(-1)
        outs[name] = out(r64, r32, clip)
        outs[name + " relu"] = out(r64.clamp_min(0.0), r32.clamp_min(0.0), clip)
    lay = (lambda t: t) if layout == "ndhwc" else (lambda t: t.transpose(1, 2).contiguous())
    return {"g": lay(g), "a": lay(a), "w": w, "layout": layout, "index": {"alpha": index}, "outs": outs}


@functools.lru_cache(maxsize=None)
def upsample_case(which):
    grid, size = UPSAMPLE[which]
    cam = torch.randn(len(UPSAMPLE_CLIPS), *grid, generator=SC._gen("explain upsample", which)).clamp_min(0.0) + 0.01
    cam = cam * torch.tensor(UPSAMPLE_CLIPS)[:, None, None, None]
    up = lambda t: F.interpolate(t[:, None], size=size, mode="trilinear", align_corners=False)[:, 0]  # noqa: E731
    return {"cam": cam, "size": size, "outs": {"map": out(SC.rows(up(cam.double()), cam.shape[0]), up(cam), [f"clip {s:g}" for s in UPSAMPLE_CLIPS])}}


# ---- embed_bwd_inputs ----------------------------------------------------------------------------------------------------------------
EMBED_D = (64, 768)
EMBED_TOKENS = 37
TOKEN_SCALES = (1e-6, 1e-3, 1.0, 1e3)
BOX_COLUMNS = (1e-2, 1.0, 30.0, 1e-3)
SCORE_COLUMN = 0.1


@functools.lru_cache(maxsize=None)
def embed_bwd_case(d, with_scores):
    """d_boxes (37, 4) = d_pre (37, d) · box_w (d, 4) and d_scores (37,) = d_pre · score_w: token i has the scale TOKEN_SCALES[i % 4],
    weight column j the scale BOX_COLUMNS[j].  Every output element is a block of its own, so a token's row is drawn again until none of
    its five sums cancels more than six bits (sum |terms| <= 64 |sum|): with free rows torch's own E_t reached 392 u at d = 768."""
    g = SC._gen("explain embed_bwd", d)
    n = EMBED_TOKENS
    box_w = torch.randn(d, 4, generator=g) * torch.tensor(BOX_COLUMNS)
    score_w = torch.randn(d, 1, generator=g) * SCORE_COLUMN
    w_all = torch.cat([box_w, score_w], 1).double()
    d_pre = torch.empty(n, d)
    for i in range(n):
        while True:  # an element is a row of its own and has nothing beside it to set its scale: no sum may cancel more than six bits
            row = torch.randn(d, generator=g)
            if float(((row.double().abs() @ w_all.abs()) / (row.double() @ w_all).abs()).max()) <= 64.0:
                break
        d_pre[i] = row * TOKEN_SCALES[i % 4]
    outs = {"d_boxes": out(SC.rows(d_pre.double() @ box_w.double(), n * 4), d_pre @ box_w,
                           [f"token {TOKEN_SCALES[i % 4]:g} | column {c:g}" for i in range(n) for c in BOX_COLUMNS], PC.chain(d_pre, box_w.T.contiguous()))}
    if with_scores:
        outs["d_scores"] = out(SC.rows(d_pre.double() @ score_w.double(), n), d_pre @ score_w, [f"token {TOKEN_SCALES[i % 4]:g} | score column" for i in range(n)],
                               PC.chain(d_pre, score_w.T.contiguous()))
    return {"d_pre": d_pre, "box_w": box_w, "score_w": score_w if with_scores else None, "outs": outs}


# ---- cell pooling and the perturbation curves ------------------------------------------------------------------------------------------
POOL_SHAPE, POOL_CELL = (3, 4, 9, 10), (2, 4, 4)   # (channels, T, H, W): cells of 2 x 4 x 4 with ragged last rows and columns
POOL_CLIPS = (1e-8, 1.0, 1e6)
CURVE_SHAPE = (6, 174)                             # steps, classes
CURVE_SCALES = (1e-3, 1.0, 30.0, 100.0, 1000.0)
CURVE_GAPS = (5.0, 0.0, -3.0, -20.0, -50.0, -70.0)   # the target's logit against the best other one, step by step, in units of min(scale, 1)


@functools.lru_cache(maxsize=None)
def cell_pool_case():
    """cell_pool_abs and cell_pool_sum: three clips of scale 1e-8, 1, 1e6, values randn + 0.5 (a cell's signed sum cancels little); one row
    per clip."""
    g = (torch.randn(len(POOL_CLIPS), *POOL_SHAPE, generator=SC._gen("explain pool")) + 0.5) * torch.tensor(POOL_CLIPS)[:, None, None, None, None]
    ct, ch, cw = POOL_CELL
    _, T, Hh, W = POOL_SHAPE

    def pool(x):
        return torch.stack([x[:, :, t:t + ct, h:h + ch, w:w + cw].reshape(x.shape[0], -1).sum(1)
                            for t in range(0, T, ct) for h in range(0, Hh, ch) for w in range(0, W, cw)], 1)

    names = [f"clip {s:g}" for s in POOL_CLIPS]
    return {"g": g, "cell": POOL_CELL, "outs": {"sum": out(pool(g.double()), pool(g), names), "abs": out(pool(g.double().abs()), pool(g.abs()), names)}}


@functools.lru_cache(maxsize=None)
def perturb_curve_case():
    """perturb_curve with softmax: five clips of logit scale 1e-3 .. 1000 over six steps.  Step 0 has the target on top; in the later steps
    every logit moves by 2 % of the scale and the target's is set CURVE_GAPS below the best other one, at most 70: its probability stays
    a normal fp32 number (exp(-70) = 4e-31).  A row is one clip's curve over the steps."""
    S, K = CURVE_SHAPE
    B = len(CURVE_SCALES)
    g = SC._gen("explain curve")
    base = torch.randn(B, K, generator=g) * torch.tensor(CURVE_SCALES)[:, None]
    target = torch.randint(0, K, (B,), generator=g)
    logits = torch.empty(S, B, K)
    for s in range(S):
        x = base + (0.02 * torch.randn(B, K, generator=g) * torch.tensor(CURVE_SCALES)[:, None] if s else 0.0)
        for b in range(B):
            others = torch.cat([x[b, :target[b]], x[b, target[b] + 1:]]).max()
            x[b, target[b]] = others + CURVE_GAPS[s] * min(CURVE_SCALES[b], 1.0)
        logits[s] = x
    pick = lambda p: p.gather(2, target[None, :, None].expand(S, B, 1))[..., 0].T  # noqa: E731
    ref, yard = pick(torch.softmax(logits.double(), -1)), pick(torch.softmax(logits, -1))
    assert float(ref.min()) > 1e-37
    return {"logits": logits, "target": target, "outs": {"probability": out(ref, yard, [f"logits {s:g}" for s in CURVE_SCALES])}}


IG_CLIPS = (1e-8, 1e-3, 1.0, 1e6)
IG_SIZES = (70001, 37)   # per clip: several blocks with a tail, and less than one vector row


@functools.lru_cache(maxsize=None)
def ig_delta_case():
    """Stage 1 of ig_delta, the sum of a clip's attributions (the seed is zero, so the logit term vanishes): four clips of scale 1e-8 .. 1e6,
    two attribution tensors, values randn + 0.05 so that a clip's sum cancels at most six bits (asserted).  One row of one element per clip."""
    g = SC._gen("explain ig delta")
    attrs = [(torch.randn(len(IG_CLIPS), n, generator=g) + 0.05) * torch.tensor(IG_CLIPS)[:, None] for n in IG_SIZES]
    ref = sum(a.double().sum(1) for a in attrs)
    assert bool((sum(a.double().abs().sum(1) for a in attrs) <= 64.0 * ref.abs()).all())
    yard = sum(a.sum(1) for a in attrs)
    return {"attrs": attrs, "K": 5, "outs": {"delta": out(ref.reshape(-1, 1), yard, [f"clip {s:g}" for s in IG_CLIPS])}}


ATTENTION_CASES = ([(L, L, dh, causal, 1) for L, dh in PACKED_SHAPES for causal in (False, True)]
                   + [(Lq, Lk, dh, Lq == Lk, reps) for Lq, Lk, dh, reps in CROSS_SHAPES])
ALL_CASES = ([("attention maps", attention_map_case, a) for a in dict.fromkeys(ATTENTION_CASES)]
             + [("probe attention", probe_case, a) for a in PROBE_SHAPES]
             + [("rollout", rollout_case, (L,)) for L in ROLLOUT_L]
             + [("joint rollout", joint_case, (T, A, given)) for T, A in JOINT_SHAPES for given in (True, False)]
             + [("cam", cam_case, (P, C, layout)) for P in CAM_P for C in CAM_C for layout in ("ndhwc", "ncdhw")]
             + [("cam", cam_case, CAM_LONG + (layout,)) for layout in ("ndhwc", "ncdhw")]
             + [("upsample", upsample_case, (i,)) for i in range(len(UPSAMPLE))]
             + [("embed_bwd_inputs", embed_bwd_case, (d, s)) for d in EMBED_D for s in (True, False)]
             + [("cell pool", cell_pool_case, ()), ("perturb curve", perturb_curve_case, ()), ("ig delta", ig_delta_case, ())])
