"""Cases, fp64 references, torch-fp32 yardsticks and the metric of the off-unit-scale tests: tests/test_off_unit_scale_gpu.py holds the
softmax, LayerNorm, GELU, criterion and optimizer kernels to them, tests/test_off_unit_scale_cpu.py holds THEM to their own conditions.
Plain torch on the CPU, no package import, no GPU.

The metric (one rule for every case).  u = 2^-24.  Every output is cut into rows, the unit the kernel reduces or normalises over (a logits
row, a LayerNorm row, one (sequence, head) block of an attention output, one parameter of the AdamW table, one (sign, binade) group of
GELU points; a scalar is a row of one element), and one batch holds rows of very different magnitudes.  For a row, S = max |fp64
reference| and e = max |result - reference| / S: e_k for the kernel, e_t for torch's own fp32 implementation of the same op on the CPU on
the same fp32 inputs.  E_t is the largest e_t among the rows of the case that share their scale parameters (their `group`).  A kernel row
passes when e_k <= 4 * max(E_t, u) (an analytic term per element is taken off first where a documented approximation of that kernel calls for one);
a row whose reference is identically zero must be exactly zero.  (An output may carry a second yardstick that is independent of the
code under test; a group's bar is then 4 * max(E_t, E_c, u): tests/product_cases.py.)  4: an equally sound fp32 evaluation in another order lands within about
2x of torch's error (two-pass LayerNorm emulated over d, mean/spread, spread and eps: worst 2.1x; the sound softmax gradient: 1.2x).

The cases keep three conditions, which the CPU test asserts: every reference is finite, no element is left out of a comparison (the rows
of an output are a reshape of all of it), and E_t <= 256 u in every group — past that torch itself is lost on the input and the bar means
nothing.  Where the plain recipe "rows of every magnitude" would break the last condition, the cases say what they do instead:
  * cross entropy, the label on the arg-max at logit scales >= 8: the true gradient p_y - 1 is then below fp32's resolution of p_y (at
    scale 1000 it is 1e-130) and any fp32 evaluation returns 0 or noise.  The runner-up logit of such a row is set 4 below the maximum, so
    that 1 - p_y is about 1/64: p_y - 1 still cancels six bits, and torch keeps the rest.
  * GELU for x <= -4: 1 + erf(x / sqrt 2) cancels to nothing in fp32 (torch's result at -8 is 0, the value -5e-15).  The negative binades
    from [4, 8) on, with -5.586, -8, -20, -1e4, -1e30 and -FLT_MAX, form one row that is judged at the scale of the binade [-4, -2) (it
    also holds that binade's largest point): every point is still compared, and [-4, -2) keeps a row and a bar of its own.  Subnormals
    and the zeros join the row of the smallest binade of their sign.
  * attention at q/k scale 17 (score std near 300), the pairing of v scales with score scales and the rising scores: see attention_case
    and mhsa_case; the constant LayerNorm row in the backward: see layernorm_case; torch's own overflow at gelu(FLT_MAX): see gelu_case.
"""
import collections
import functools
import math
import zlib

import torch
import torch.nn.functional as F

U = 2.0 ** -24
MARGIN = 4.0
YARD_CAP = 256.0
FLT_MAX = 3.4028234663852886e38

Out = collections.namedtuple("Out", "ref yard group yard2", defaults=(None,))  # ref, yard: (rows, n) float64; group: one name per row; yard2: an optional second yardstick (tests/product_cases.py)


def rows(t, n_rows):
    return t.detach().cpu().double().reshape(n_rows, -1)


def out(ref, yard, group, yard2=None):
    """One compared output: reference and yardstick as (rows, n) with one group name per row (a single name: the same for every row).
    yard2: a second fp32 evaluation that is independent of the code under test (tests/product_cases.py: an in-order chain); a group's
    yardstick is then the larger of the two errors."""
    group = [group] * ref.shape[0] if isinstance(group, str) else list(group)
    assert ref.dim() == 2 and len(group) == ref.shape[0]
    return Out(ref.double(), rows(yard, ref.shape[0]), group, None if yard2 is None else rows(yard2, ref.shape[0]))


def scalar(ref, yard, group):
    return out(torch.as_tensor(ref, dtype=torch.float64).reshape(1, 1), torch.as_tensor(yard).reshape(1, 1), group)


def row_errors(got, ref):
    """Per row: max |got - ref| / max |ref|; a row whose reference is identically zero: 0 if got is exactly zero, else inf.  NaN counts as inf."""
    got = rows(got, ref.shape[0])
    assert got.shape == ref.shape, (got.shape, ref.shape)
    scale = ref.abs().amax(1)
    err = torch.nan_to_num((got - ref).abs(), nan=math.inf).amax(1)
    zero = scale == 0
    return torch.where(zero, torch.where(err == 0, 0.0, math.inf).double(), err / scale.clamp_min(1e-300)), zero


def _group_worst(yard, o):
    e_t, zero = row_errors(yard, o.ref)
    worst = {}
    for e, z, g in zip(e_t.tolist(), zero.tolist(), o.group):
        worst[g] = max(worst.get(g, 0.0), 0.0 if z else e)
    return worst


def yardsticks(o):
    """({group: E_t}, {group: E_c} or None): the largest row error of each group for torch's fp32 op and for the second yardstick, where
    the output has one (zero rows have no scale and set no bar)."""
    return _group_worst(o.yard, o), (None if o.yard2 is None else _group_worst(o.yard2, o))


def yardstick(o):
    """{group: E_t} — the largest torch-fp32 row error of each group; with a second yardstick max(E_t, E_c)."""
    e_t, e_c = yardsticks(o)
    return e_t if e_c is None else {g: max(e, e_c[g]) for g, e in e_t.items()}


def judge(tag, got, o, term=None):
    """Hold `got` to the rule, row by row.  term: the analytic term of a documented approximation of the kernel, an absolute allowance per
    element (the reference's shape); an element's error counts by what exceeds it.  Prints one line per group (the raw e_k, and the e_k
    left after the term where one is given) and returns (lines, failures)."""
    e_raw, _ = row_errors(got, o.ref)
    e_k = e_raw
    if term is not None:
        term = term.double().reshape(o.ref.shape)
        err = torch.nan_to_num((rows(got, o.ref.shape[0]) - o.ref).abs(), nan=math.inf)
        e_k = torch.where(o.ref.abs().amax(1) == 0, e_raw, (err - term).clamp_min(0.0).amax(1) / o.ref.abs().amax(1).clamp_min(1e-300))
    e_t = yardstick(o)
    e_1, e_2 = yardsticks(o)
    worst, fails = {}, []
    for i, (e, raw, g) in enumerate(zip(e_k.tolist(), e_raw.tolist(), o.group)):
        bar = MARGIN * max(e_t[g], U)
        if not e <= bar:
            fails.append(f"{tag} [{g}] row {i}: e_k = {e / U:.2f} u over the bar {bar / U:.2f} u (E_t = {e_t[g] / U:.2f} u" + (f", {raw / U:.2f} u before the analytic term)" if term is not None else ")"))
        worst[g] = (max(e, worst[g][0]), max(raw, worst[g][1])) if g in worst else (e, raw)
    lines = []
    for g, (e, raw) in worst.items():
        note = f" | after the analytic term {e / U:.2f}, ratio {e / max(e_t[g], U):.2f}" if term is not None else ""
        yards = f"E_t/u {e_t[g] / U:.2f}" if e_2 is None else f"E_t/u {e_1[g] / U:.2f} | E_c/u {e_2[g] / U:.2f}"
        lines.append(f"[scale] {tag} | {g} | e_k/u {raw / U:.2f} | {yards} | ratio {raw / max(e_t[g], U):.2f}{note}")
    print("\n".join(lines))
    return lines, fails


def conditions(o):
    """The three conditions on one output of a case -> list of what is broken."""
    bad = []
    if not bool(torch.isfinite(o.ref).all()):
        bad.append("a reference value is not finite")
    if o.yard.shape != o.ref.shape or (o.yard2 is not None and o.yard2.shape != o.ref.shape):
        bad.append("the yardstick does not cover the reference")
    for g, e in yardstick(o).items():
        if not e <= YARD_CAP * U:
            bad.append(f"[{g}] E_t = {e / U:.1f} u: torch itself is lost here")
    return bad


def _gen(*seed):
    return torch.Generator().manual_seed(zlib.crc32(repr(seed).encode()))


# ---- criterion --------------------------------------------------------------------------------------------------------------------
CE_SHAPES = ((6, 5), (6, 174), (5, 300))
CE_SCALES = (1e-3, 1.0, 8.0, 30.0, 100.0, 1000.0)
BCE_SHAPES = ((6, 157), (5, 300))
BCE_SCALES = (1e-3, 1.0, 30.0, 100.0)
WEIGHTS = (1.0, 0.5)


@functools.lru_cache(maxsize=None)
def cross_entropy_case(B, K, variant, weight, ignored_row=-1):
    """Row i has the logit scale CE_SCALES[(i + variant) % 6]; its label is the arg-max (loss near 0: p_y - 1 cancels) or the arg-min, and
    variant 0 / 1 swap which of the two a scale gets.  ignored_row >= 0: that row's label is -100 (the mean runs over the others and the
    kernel rescales the rows it has written)."""
    g = _gen("ce", B, K, variant)
    logits = torch.randn(B, K, generator=g)
    labels = torch.zeros(B, dtype=torch.int64)
    group = []
    for i in range(B):
        si = (i + variant) % len(CE_SCALES)
        s = CE_SCALES[si]
        logits[i] *= s
        on_max = (si + variant) % 2 == 0
        if on_max:
            order = logits[i].argsort(descending=True)
            if s >= 8.0:
                logits[i, order[1]] = logits[i, order[0]] - 4.0  # see the module docstring
            labels[i] = order[0]
        else:
            labels[i] = logits[i].argmin()
        group.append(f"scale {s:g} label on the arg-{'max' if on_max else 'min'}")
    if ignored_row >= 0:
        labels[ignored_row] = -100
        group[ignored_row] = "ignored"
    res = {}
    for dt in (torch.float64, torch.float32):
        x = logits.to(dt).requires_grad_(True)
        loss = weight * F.cross_entropy(x, labels)
        loss.backward()
        res[dt] = (loss.detach(), x.grad)
    return {"logits": logits, "labels": labels, "kind": 0, "weight": weight,
            "outs": {"gradient": out(rows(res[torch.float64][1], B), res[torch.float32][1], group),
                     "loss": scalar(res[torch.float64][0], res[torch.float32][0], "loss")}}


@functools.lru_cache(maxsize=None)
def bce_case(B, K, weight):
    """Row i has the logit scale BCE_SCALES[i % 4] (100: exp(-v) overflows fp32 and must give a gradient of 0 - t, not NaN); multi-hot labels at density 0.1."""
    g = _gen("bce", B, K)
    logits = torch.randn(B, K, generator=g)
    group = []
    for i in range(B):
        s = BCE_SCALES[i % len(BCE_SCALES)]
        logits[i] *= s
        group.append(f"scale {s:g}")
    labels = (torch.rand(B, K, generator=g) < 0.1).float()
    res = {}
    for dt in (torch.float64, torch.float32):
        x = logits.to(dt).requires_grad_(True)
        loss = weight * F.binary_cross_entropy_with_logits(x, labels.to(dt))
        loss.backward()
        res[dt] = (loss.detach(), x.grad)
    return {"logits": logits, "labels": labels, "kind": 1, "weight": weight,
            "outs": {"gradient": out(rows(res[torch.float64][1], B), res[torch.float32][1], group),
                     "loss": scalar(res[torch.float64][0], res[torch.float32][0], "loss")}}


# ---- gradient norm and AdamW ------------------------------------------------------------------------------------------------------
OPT_SIZES = (1, 3, 4, 5, 1023, 16391)
OPT_GRAD_SCALES = (1e-6, 1e3, 1e-12, 1.0, 1e-3, 1e-6)   # one per parameter: every value of {1e-12, 1e-6, 1e-3, 1, 1e3}
OPT_PARAM_SCALES = (1.0, 1e-3, 1e2, 1e-3, 1.0, 1e2)
OPT_DECAYS = (0.0, 1e-2, 1e-2, 0.0, 1e-2, 0.0)
OPT_LRS = (1e-5, 1e-3)
OPT_CHUNK = 16384
BETAS, ADAM_EPS = (0.9, 0.999), 1e-8
NORM_SIZES = (5, 4099, 70001)
NORM_SCALES = (1e-15, 1e-6, 1.0, 1e15)


def opt_layout():
    """Where the parameters lie.  In the flat gradient / moment buffers every parameter starts on a 16-byte boundary, as the training
    step lays them out; in the parameter buffer they are packed back to back, so those of 3 and 1023 elements (float offsets 1 and 13)
    are not 16-byte aligned and take the update kernel's one-element path, while the last one spans two chunks (16384 + 7: whole
    vectors, and one vector with a three-element tail).  -> (parameter offsets, flat offsets, flat length, [(parameter, first element, n)])."""
    p_off, f_off, chunks, po, fo = [], [], [], 0, 0
    for i, n in enumerate(OPT_SIZES):
        p_off.append(po)
        f_off.append(fo)
        for c0 in range(0, n, OPT_CHUNK):
            chunks.append((i, c0, min(OPT_CHUNK, n - c0)))
        po += n
        fo += (n + 3) // 4 * 4
    return p_off, f_off, fo, chunks


def _adamw_ref(p, m, v, g, step, lr, decay, max_norm):
    """One clip_grad_norm_ + AdamW step written out in fp64 on lists of tensors -> (norm, coefficient)."""
    norm = math.sqrt(sum(float((x * x).sum()) for x in g))
    coef = min(1.0, max_norm / (norm + 1e-6))
    bc1, bc2 = 1.0 - BETAS[0] ** step, 1.0 - BETAS[1] ** step
    for i in range(len(p)):
        gi = g[i] * coef
        p[i] *= 1.0 - lr * decay[i]
        m[i] += (1.0 - BETAS[0]) * (gi - m[i])
        v[i] = BETAS[1] * v[i] + (1.0 - BETAS[1]) * gi * gi
        p[i] -= (lr / bc1) * m[i] / (v[i].sqrt() / math.sqrt(bc2) + ADAM_EPS)
    return norm, coef


@functools.lru_cache(maxsize=None)
def adamw_case(lr, clipping, late):
    """late = False: three consecutive steps from zero moments (steps 1, 2, 3); True: one step at step = 100000 from given moments of the
    gradients' scale.  Every parameter has its own gradient scale, parameter scale and weight decay; max_norm is half (clipping) or twice
    the step's norm, rounded to fp32.  Compared after every step: the parameters, both moments, the norm and the coefficient."""
    g0 = _gen("adamw", lr, clipping, late)
    n_par = len(OPT_SIZES)
    p0 = [torch.randn(n, generator=g0) * s for n, s in zip(OPT_SIZES, OPT_PARAM_SCALES)]
    steps = [100000] if late else [1, 2, 3]
    grads = [[torch.randn(n, generator=g0) * s for n, s in zip(OPT_SIZES, OPT_GRAD_SCALES)] for _ in steps]
    if late:
        m0 = [torch.randn(n, generator=g0) * s for n, s in zip(OPT_SIZES, OPT_GRAD_SCALES)]
        v0 = [(torch.randn(n, generator=g0) * s) ** 2 for n, s in zip(OPT_SIZES, OPT_GRAD_SCALES)]
    else:
        m0, v0 = [torch.zeros(n) for n in OPT_SIZES], [torch.zeros(n) for n in OPT_SIZES]
    max_norms = []
    for g in grads:
        norm = math.sqrt(sum(float((x.double() ** 2).sum()) for x in g))
        max_norms.append(float(torch.tensor(norm * (0.5 if clipping else 2.0), dtype=torch.float32)))
    group = [f"parameter of {n} (gradients {gs:g}, values {ps:g}, decay {wd:g})" for n, gs, ps, wd in zip(OPT_SIZES, OPT_GRAD_SCALES, OPT_PARAM_SCALES, OPT_DECAYS)]
    # fp64 reference
    p, m, v = [x.double().clone() for x in p0], [x.double().clone() for x in m0], [x.double().clone() for x in v0]
    ref = []
    for step, g, mx in zip(steps, grads, max_norms):
        norm, coef = _adamw_ref(p, m, v, [x.double() for x in g], step, lr, OPT_DECAYS, mx)
        ref.append(([x.clone() for x in p], [x.clone() for x in m], [x.clone() for x in v], norm, coef))
    # torch's fp32 on the CPU
    tp = [torch.nn.Parameter(x.clone()) for x in p0]
    opt = torch.optim.AdamW([{"params": [tp[i]], "weight_decay": OPT_DECAYS[i]} for i in range(n_par)], lr=lr, betas=BETAS, eps=ADAM_EPS)
    if late:
        for i, q in enumerate(tp):
            opt.state[q] = {"step": torch.tensor(float(steps[0] - 1)), "exp_avg": m0[i].clone(), "exp_avg_sq": v0[i].clone()}
    outs = {}
    for (step, g, mx), (rp, rm, rv, rnorm, rcoef) in zip(zip(steps, grads, max_norms), ref):
        for q, x in zip(tp, g):
            q.grad = x.clone()
        tnorm = torch.nn.utils.clip_grad_norm_(tp, mx)
        tcoef = torch.clamp(mx / (tnorm + 1e-6), max=1.0)
        opt.step()
        assert (rcoef < 1.0) == clipping
        for name, r, t in (("parameters", rp, [q.detach() for q in tp]), ("exp_avg", rm, [opt.state[q]["exp_avg"] for q in tp]),
                           ("exp_avg_sq", rv, [opt.state[q]["exp_avg_sq"] for q in tp])):
            for i in range(n_par):
                outs[f"step {step} {name} [{i}]"] = out(r[i].reshape(1, -1), t[i], group[i])
        outs[f"step {step} norm"] = scalar(rnorm, tnorm, "norm")
        outs[f"step {step} coefficient"] = scalar(rcoef, tcoef, "coefficient")
    return {"p0": p0, "m0": m0, "v0": v0, "grads": grads, "steps": steps, "max_norms": max_norms, "lr": lr, "outs": outs}


@functools.lru_cache(maxsize=None)
def norm_case(n, scale, clipping):
    """stlt_grad_norm alone on n gradients of one magnitude; [1e-15, 1e15]: the squares stay normal fp32 numbers."""
    g = torch.randn(n, generator=_gen("norm", n, scale)) * scale
    ref = math.sqrt(float((g.double() ** 2).sum()))
    max_norm = float(torch.tensor(ref * (0.5 if clipping else 2.0), dtype=torch.float32))
    tnorm = torch.linalg.vector_norm(g)
    return {"g": g, "max_norm": max_norm,
            "outs": {"norm": scalar(ref, tnorm, "norm"),
                     "coefficient": scalar(min(1.0, max_norm / (ref + 1e-6)), torch.clamp(max_norm / (tnorm + 1e-6), max=1.0), "coefficient")}}


# ---- LayerNorm --------------------------------------------------------------------------------------------------------------------
LN_D = (64, 260, 768, 1028)   # 1028: the wide backward kernel
LN_EPS = (1e-5, 1e-12)
LN_COMBOS = tuple((ms, sp) for ms in (0, 10, 100) for sp in (1e-4, 1.0, 1e4))  # (mean / spread, spread)
LN_DY = (1e-4, 1.0, 1e4)
LN_CONSTANT = 3.0            # 3 * d is exact in fp32 for every d here, 1 / d is not: a mean taken as sum * (1 / d) has to come out as 3 all the same


def _ln_rows(d, seed, combos=LN_COMBOS, per=6, specials=True):
    """Pre-LayerNorm rows and their split into x + residual.  `per` rows for each (mean / spread, spread); with specials two constant rows
    (variance 0: the output is the shift, the gradient rstd * (g - mean g) with rstd = 1 / sqrt(eps)), one of LN_CONSTANT and one of
    zeros, and two rows whose residual cancels x to 1e-4 of its size.  -> x, residual (the rows themselves are x + residual, or x alone
    when the op runs without a residual), names."""
    g = _gen("ln", d, seed)
    xs, rs, names = [], [], []
    for ms, sp in combos:
        for _ in range(per):
            xs.append(sp * (torch.randn(d, generator=g) + ms))
            rs.append(0.5 * sp * torch.randn(d, generator=g))
            names.append(f"mean/spread {ms} spread {sp:g}")
    if specials:
        for c in (LN_CONSTANT, 0.0):
            xs.append(torch.full((d,), c))
            rs.append(torch.zeros(d))
            names.append(f"constant row of {c:g}")
        for _ in range(2):
            x = torch.randn(d, generator=g) + 1.0
            xs.append(x)
            rs.append(-x + 1e-4 * torch.randn(d, generator=g))
            names.append("residual cancels x to 1e-4")
    return torch.stack(xs), torch.stack(rs), names


def _ln_params(d):
    g = _gen("ln params", d)
    return 1.0 + 0.1 * torch.randn(d, generator=g), 0.1 * torch.randn(d, generator=g)


@functools.lru_cache(maxsize=None)
def layernorm_case(d, eps, with_res):
    """Forward and input gradient of LayerNorm_eps(x [+ residual]) on rows of every (mean / spread, spread), gradient rows of scales
    1e-4 / 1 / 1e4 (two rows of each per combination).  The constant row of LN_CONSTANT gets a zero gradient row: torch's own backward
    (dx = a dy w + b x + c with b = (mean * sum(dy w) - sum(dy w x)) * rstd^3 / d) loses that row at eps = 1e-12, where rstd^3 = 1e18
    multiplies the rounding of a difference (E_t = 1e5 u), so the row only has to come out exactly zero (rstd = 1e6 must not turn it into
    NaN or noise); the constant row of zeros carries the gradient check at variance 0, there torch's b is exactly 0."""
    x, r, names = _ln_rows(d, 0)
    if not with_res:  # the same designed rows, given whole (the cancelling rows are then ordinary rows of spread 1e-4)
        x = x + r
    w, b = _ln_params(d)
    M = x.shape[0]
    g = _gen("ln dy", d)
    dy_scale = torch.tensor([LN_DY[(i // 2) % 3] for i in range(M)])
    dy = torch.randn(M, d, generator=g) * dy_scale[:, None]
    dy[names.index(f"constant row of {LN_CONSTANT:g}")] = 0.0
    res = {}
    for dt in (torch.float64, torch.float32):
        xx, rr = x.to(dt).requires_grad_(True), r.to(dt)
        y = F.layer_norm(xx + rr if with_res else xx, (d,), w.to(dt), b.to(dt), eps)
        y.backward(dy.to(dt))
        res[dt] = (y.detach(), xx.grad)
    bwd_names = [f"{n} dy {s:g}" for n, s in zip(names, dy_scale.tolist())]
    return {"x": x, "res": r if with_res else None, "w": w, "b": b, "dy": dy, "eps": eps,
            "outs": {"forward": out(rows(res[torch.float64][0], M), res[torch.float32][0], names),
                     "ds": out(rows(res[torch.float64][1], M), res[torch.float32][1], bwd_names)}}


@functools.lru_cache(maxsize=None)
def layernorm_param_grad_case(d, eps, combo):
    """Scale and shift gradients (column sums over the rows, so every row of the batch has the one (mean / spread, spread) `combo`)."""
    x, r, _ = _ln_rows(d, 1 + combo, combos=(LN_COMBOS[combo],), per=8, specials=False)
    w, b = _ln_params(d)
    dy = torch.randn(x.shape[0], d, generator=_gen("ln dy", d, combo))
    res = {}
    for dt in (torch.float64, torch.float32):
        ww, bb = w.to(dt).requires_grad_(True), b.to(dt).requires_grad_(True)
        F.layer_norm(x.to(dt) + r.to(dt), (d,), ww, bb, eps).backward(dy.to(dt))
        res[dt] = (ww.grad, bb.grad)
    name = "mean/spread %g spread %g" % LN_COMBOS[combo]
    return {"x": x, "res": r, "w": w, "dy": dy, "eps": eps,
            "outs": {"g_w": out(rows(res[torch.float64][0], 1), res[torch.float32][0], name),
                     "g_b": out(rows(res[torch.float64][1], 1), res[torch.float32][1], name)}}


@functools.lru_cache(maxsize=None)
def frames_embed_case(d, eps=1e-12):
    """FramesEmbeddings: LayerNorm_eps((cls row + position row) + frame-type row), one clip whose frames are the designed rows."""
    x, _, names = _ln_rows(d, 2, specials=False)  # the sum of three tables is neither constant nor cancelling by design
    T = x.shape[0]
    g = _gen("frames", d)
    pos, typ = 1e-5 * torch.randn(T, d, generator=g), 1e-5 * torch.randn(5, d, generator=g)
    ft = torch.randint(0, 5, (1, T), generator=g)
    w, b = _ln_params(d)
    res = {}
    for dt in (torch.float64, torch.float32):
        s = (x.to(dt) + pos.to(dt)) + typ.to(dt)[ft[0]]
        res[dt] = F.layer_norm(s, (d,), w.to(dt), b.to(dt), eps)
    return {"spatial": x.reshape(1, T, d), "frame_types": ft, "pos": pos, "type": typ, "w": w, "b": b, "eps": eps,
            "outs": {"forward": out(rows(res[torch.float64], T), res[torch.float32], names)}}


@functools.lru_cache(maxsize=None)
def embed_case(d, with_scores, eps=1e-12):
    """CategoryBoxEmbeddings: LayerNorm_eps(table row + box projection [+ score projection]); token i names table row i, a designed row."""
    x, _, names = _ln_rows(d, 3, specials=False)
    n = x.shape[0]
    g = _gen("embed", d)
    boxes, scores = torch.rand(n, 4, generator=g), torch.rand(n, generator=g)
    box_w, box_b = 1e-5 * torch.randn(d, 4, generator=g), 1e-5 * torch.randn(d, generator=g)
    score_w, score_b = 1e-5 * torch.randn(d, 1, generator=g), 1e-5 * torch.randn(d, generator=g)
    w, b = _ln_params(d)
    res = {}
    for dt in (torch.float64, torch.float32):
        s = x.to(dt) + F.linear(boxes.to(dt), box_w.to(dt), box_b.to(dt))
        if with_scores:
            s = s + F.linear(scores.to(dt)[:, None], score_w.to(dt), score_b.to(dt))
        res[dt] = F.layer_norm(s, (d,), w.to(dt), b.to(dt), eps)
    return {"categories": torch.arange(n), "boxes": boxes, "scores": scores if with_scores else None, "table": x, "box_w": box_w, "box_b": box_b,
            "score_w": score_w, "score_b": score_b, "w": w, "b": b, "eps": eps,
            "outs": {"forward": out(rows(res[torch.float64], n), res[torch.float32], names)}}


# ---- GELU -------------------------------------------------------------------------------------------------------------------------
GELU_BINADES = (-30, 6)          # 64 log-uniform points in every binade [2^e, 2^(e+1)), e = -30 .. 5, both signs
GELU_SPECIALS = (0.0, 1e-45, 1e-40, 1.1754942e-38, 5.586, 8.0, 20.0, 1e4, 1e30, FLT_MAX)  # 5.586: the fit's clamp at z = 3.95
GELU_NEGATIVE_TAIL = 2           # negative points from -4 on are one row, judged at the scale of the binade [-4, -2)


@functools.lru_cache(maxsize=None)
def gelu_case():
    """64 log-uniform points in every binade of GELU_BINADES and the special points, both signs -> the points x (n,), the row of each
    (`row_of`, `names`: sign and binade, clamped as the module docstring says), gelu and gelu' at them in fp64 and from torch in fp32."""
    g = _gen("gelu")
    lo, hi = GELU_BINADES
    mags = torch.cat([2.0 ** (e + torch.rand(64, generator=g, dtype=torch.float64)) for e in range(lo, hi)] + [torch.tensor(GELU_SPECIALS, dtype=torch.float64)])
    x = torch.cat([mags, -mags]).float()
    # row of a point: its sign and the binade of |x|, clamped as the module docstring says
    binade = torch.floor(torch.log2(x.double().abs().clamp_min(2.0 ** -160)))
    binade = binade.clamp_min(lo)
    negative = torch.signbit(x)
    binade = torch.where(negative, binade.clamp_max(GELU_NEGATIVE_TAIL), binade)
    key = binade * 2 + negative.double()
    keys = sorted(set(key.tolist()))
    row_of = torch.tensor([keys.index(k) for k in key.tolist()])
    names = []
    for k in keys:
        e, neg = int(k // 2), bool(k % 2)
        names.append((f"{'-' if neg else '+'}2^{e}" if not (neg and e == GELU_NEGATIVE_TAIL) else "the negative tail from -4 on, at the scale of -2^1")
                     + (" with zero and the subnormals" if e == lo else ""))
    x64 = x.double().requires_grad_(True)
    F.gelu(x64).sum().backward()
    x32 = x.clone().requires_grad_(True)
    F.gelu(x32).sum().backward()
    fwd64, fwd32 = F.gelu(x.double()), F.gelu(x)
    # torch multiplies x by 1 + erf before it halves: gelu(FLT_MAX) = FLT_MAX comes out as inf.  That one point has no yardstick; it takes
    # the reference's value there, so its row (+2^127, the point alone) is held to the floor of the bar, 4 u.
    lost = ~torch.isfinite(fwd32)
    assert bool((x[lost] == FLT_MAX).all()) and int(lost.sum()) <= 1
    fwd32 = torch.where(lost, fwd64.float(), fwd32)
    # the tail's row also holds the point of [-4, -2) nearest -2 (a second comparison of that point): it is the largest value of that binade,
    # of gelu and of gelu' alike, and so sets the tail's scale, while [-4, -2) itself keeps a row and a bar of its own
    near = (x >= -4.0) & (x < -2.0)
    anchor = int(torch.where(near, x, torch.full_like(x, -math.inf)).argmax())
    assert bool(near[anchor]) and abs(float(fwd64[anchor])) == float(fwd64[near].abs().max())
    anchors = {keys.index(GELU_NEGATIVE_TAIL * 2 + 1.0): anchor}
    return {"x": x, "row_of": row_of, "names": names, "anchors": anchors, "fwd64": fwd64, "fwd32": fwd32, "bwd64": x64.grad, "bwd32": x32.grad}


def gelu_out(case, which):
    """The points' values as padded rows: (rows, widest row), a short row repeating its first point (so that no element is added or lost)."""
    return out(gelu_rows(case, case[which + "64"]), gelu_rows(case, case[which + "32"]), case["names"])


def gelu_scaled_derivative_out(case, v):
    """v (n,) fp32, one multiplier per point -> the rows of v * gelu'(x): what a backward pass hands on when v arrives at the points
    (the reference from v as it is, in fp64; torch's yardstick as the fp32 product with its own fp32 gelu')."""
    return out(gelu_rows(case, v.double().cpu() * case["bwd64"]), gelu_rows(case, v.float().cpu() * case["bwd32"]), case["names"])


def gelu_block_chunks(case, d):
    """The points as the pre-activations of a feed-forward block of width d with ONE row: the first weight is zero and the first bias holds
    4 d points, so u = b1 to the bit whatever x is; column j of the second weight holds the single entry alpha_j in row j % d, a power of two
    that brings gelu(u_j) back to order 1 (the block's own forward must stay finite at 1e30 and FLT_MAX).  Then the hidden gradient is
    du_j = ds[j % d] * alpha_j * gelu'(u_j) with ds the gradient at the block's LayerNorm input, which the block returns as dx (W1 = 0),
    and the first bias's gradient, a column sum over one row, is du itself.  -> [(positions of the chunk's points, b1, W2, alpha)]"""
    x = case["x"]
    n, width = x.numel(), 4 * d
    chunks = []
    for c0 in range(0, n, width):
        pos = torch.arange(c0, c0 + width).clamp_max(n - 1)   # the last chunk repeats the last point
        b1 = x[pos]
        alpha = 2.0 ** -torch.floor(torch.log2(b1.double().abs().clamp_min(1.0))).float()
        w2 = torch.zeros(d, width)
        w2[torch.arange(width) % d, torch.arange(width)] = alpha
        chunks.append((pos, b1, w2, alpha))
    return chunks


def gelu_rows(case, values):
    values = values.detach().cpu().double().reshape(-1)
    row_of = case["row_of"]
    n_rows = len(case["names"])
    members = [torch.nonzero(row_of == r).reshape(-1) for r in range(n_rows)]
    for r, i in case["anchors"].items():
        members[r] = torch.cat([torch.tensor([i]), members[r]])
    width = max(len(m) for m in members)
    idx = torch.stack([torch.cat([m, m[:1].expand(width - len(m))]) for m in members])
    assert sorted(set(idx.reshape(-1).tolist())) == list(range(values.numel()))  # every point is in a row
    return values[idx]


# ---- attention --------------------------------------------------------------------------------------------------------------------
ATTN_H, ATTN_DH = 2, 64
ATTN_L = (5, 33, 70, 200)
ATTN_QK = (0.03, 1.5, 5.5, 17.0)   # score std about 1e-3, 2, 30, 300
ATTN_V = (1e3, 1.0, 1e-3, 1.0)       # the v scale of each q / k scale: see attention_case
ATTN_DCTX = (1e-6, 1.0, 1e3, 1.0)
ATTN_RISE = 16.0                     # how far the scores of the rising sequence climb from the first key to the last


def attention(q, k, v, kpm, causal, H=ATTN_H):
    """softmax(q kᵀ / sqrt(dh) + masks) v in the dtype given: q (S, Lq, d), k and v (S, Lk, d), kpm (S, Lk) True = key masked.
    -> ctx (S, Lq, d), probabilities (S, H, Lq, Lk); a query with every key masked gets zeros."""
    S, Lq, d = q.shape
    Lk = k.shape[1]
    sp = lambda t: t.reshape(S, -1, H, d // H).transpose(1, 2)
    sc = sp(q) @ sp(k).transpose(-1, -2) / math.sqrt(d // H)
    masked = kpm[:, None, None, :].expand(S, H, Lq, Lk)
    if causal:
        masked = masked | torch.ones(Lq, Lk, dtype=torch.bool).triu(1)
    pr = torch.nan_to_num(torch.softmax(sc.masked_fill(masked, -math.inf), -1), nan=0.0)
    return (pr @ sp(v)).transpose(1, 2).reshape(S, Lq, d), pr


def head_rows(t, H=ATTN_H):
    """(S, L, n * d) packed per head inside each of the n parts -> one row per (sequence, head)."""
    S, L, nd = t.shape
    dh = ATTN_DH
    return t.detach().cpu().double().reshape(S, L, nd // (H * dh), H, dh).permute(0, 3, 1, 2, 4).reshape(S * H, -1)


@functools.lru_cache(maxsize=None)
def attention_case(Lq, Lk, causal):
    """Six sequences: four with the q / k scales of ATTN_QK and the v scales of ATTN_V, one whose scores rise along the keys by ATTN_RISE
    over the sequence (the running maximum of the kernel changes in every key tile), one with every key masked (zeros).  30 % of the keys
    are masked, key 0 never.  Self-attention (Lq == Lk): q, k, v are the thirds of one packed buffer.

    The large v goes with the flat softmax and the small v with the peaked one: the gradient of a peaked softmax, p (dP - sum p dP), is a
    cancellation whose absolute error is u |dP| = u |dctx| |v| in any fp32 evaluation, while the block's scale is set by dv = pᵀ dctx; with
    v = 1e3 on scores of std 30 torch's E_t of the dqkv block is 1e4 u.  A rise of 60 loses the rising sequence the same way (the
    scores' own rounding, E_t = 375 u at 200 keys).

    q / k of the scale-17 sequence are rounded to multiples of 1/2: their products and the 64-term sums are then exact in fp32 in any
    order, so that sequence measures the softmax at scores of +-300 alone.  With free fp32 inputs the scores themselves carry an absolute
    error near 64 * ulp(300) / 2, which exp turns into a relative error of the probabilities of 1e-4 and more: torch's own E_t passes 256 u."""
    S, H, d = 6, ATTN_H, ATTN_H * ATTN_DH
    g = _gen("attn", Lq, Lk, causal)
    q, k, v = torch.randn(S, Lq, d, generator=g), torch.randn(S, Lk, d, generator=g), torch.randn(S, Lk, d, generator=g)
    dctx = torch.randn(S, Lq, d, generator=g)
    group = []
    for s in range(4):
        q[s] *= ATTN_QK[s]
        k[s] *= ATTN_QK[s]
        v[s] *= ATTN_V[s]
        dctx[s] *= ATTN_DCTX[s]
        group.append(f"q/k {ATTN_QK[s]:g} v {ATTN_V[s]:g}")
    q[3], k[3] = torch.round(q[3] * 2) / 2, torch.round(k[3] * 2) / 2
    u = torch.randn(d, generator=g)
    u = u / u.reshape(H, -1).norm(dim=1).repeat_interleave(ATTN_DH)        # unit length inside each head
    q[4] = 0.1 * q[4] + math.sqrt(ATTN_RISE * 8.0) * u
    k[4] = 0.1 * k[4] + math.sqrt(ATTN_RISE * 8.0) * u * (torch.arange(Lk) / max(Lk - 1, 1))[:, None]
    group += ["scores rising along the keys", "every key masked"]
    kpm = torch.rand(S, Lk, generator=g) < 0.3
    kpm[:, 0] = False
    kpm[5, :] = True
    res = {}
    for dt in (torch.float64, torch.float32):
        qq, kk, vv = (t.to(dt).requires_grad_(True) for t in (q, k, v))
        ctx, pr = attention(qq, kk, vv, kpm, causal)
        ctx.backward(dctx.to(dt))
        res[dt] = (ctx.detach(), pr.detach(), torch.cat([qq.grad, kk.grad, vv.grad], -1) if Lq == Lk else None)
    rows2 = [n for n in group for _ in range(H)]
    outs = {"ctx": out(head_rows(res[torch.float64][0]), head_rows(res[torch.float32][0]), rows2),
            "probabilities per head": out(rows(res[torch.float64][1], S * H), res[torch.float32][1], rows2),
            "probabilities": out(rows(res[torch.float64][1].mean(1), S), res[torch.float32][1].mean(1), group)}
    if Lq == Lk:
        outs["dqkv"] = out(head_rows(res[torch.float64][2]), head_rows(res[torch.float32][2]), rows2)
    return {"q": q, "k": k, "v": v, "kpm": kpm, "dctx": dctx, "causal": causal, "outs": outs}


@functools.lru_cache(maxsize=None)
def mhsa_case(L, causal):
    """The fused in-projection + attention: x rows of the scales that give q / k of ATTN_QK[:3] through one projection (so v follows
    q / k).  No sequence at 17: scores of std 300 out of a rounded projection carry an error that exp turns into E_t = 400 - 900 u."""
    S, H, d = 6, ATTN_H, ATTN_H * ATTN_DH
    g = _gen("mhsa", L, causal)
    x = torch.randn(S, L, d, generator=g)
    w, b = torch.randn(3 * d, d, generator=g) / math.sqrt(d), 0.1 * torch.randn(3 * d, generator=g)
    group = []
    for s in range(S - 1):
        sc = ATTN_QK[s % 3]
        x[s] *= sc
        group.append(f"x {sc:g}")
    group.append("every key masked")
    kpm = torch.rand(S, L, generator=g) < 0.3
    kpm[:, 0] = False
    kpm[S - 1, :] = True
    res = {}
    for dt in (torch.float64, torch.float32):
        qkv = F.linear(x.to(dt), w.to(dt), b.to(dt))
        res[dt] = attention(qkv[..., :d], qkv[..., d:2 * d], qkv[..., 2 * d:], kpm, causal)[0]
    rows2 = [n for n in group for _ in range(H)]
    return {"x": x, "w": w, "b": b, "kpm": kpm, "causal": causal, "outs": {"ctx": out(head_rows(res[torch.float64]), head_rows(res[torch.float32]), rows2)}}
