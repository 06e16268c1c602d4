"""The perturbation test on the GPU: the three kernels alone against the NumPy restatement (tests/perturbation_restated.py) inside guard
bands, the curve kernel against fp64 under the off-unit-scale rule (tests/scale_cases.py), Stlt.forward_perturbed and the runner against
the fixtures the reference made (tests/golden/perturbation_<cfg>.npz), and the refusals."""
import ctypes as C
import importlib
import math

import numpy as np
import pytest
import torch

import perturbation_cases as PC
import perturbation_restated as R
import scale_cases as SC
from conftest import PKG_NAME
from guard_arena import STLT_EINVAL, Arena, Out, last_error, stream, three_ways

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TOL = 1e-4  # the project's bound on logits (tests/test_attention_gpu.py)
SHAPES = [(2, 2), (3, 11), (4, 8), (5, 7), (17, 5), (33, 8), (64, 36), (128, 128)]
EMPTY, REGULAR, EXTRACT = 3, 2, 4


@pytest.fixture(scope="module")
def lib():
    return importlib.import_module(PKG_NAME + "._lib").load()


@pytest.fixture(scope="module")
def arena():
    return Arena(160 << 20, DEV)


def kernel_case(T, N, with_scores, seed):
    """Six clips: length 1, length 2, a full clip of random objects, a clip without any object (every frame empty: no candidate), a clip
    whose scores are all equal, a clip of special values (both zeros, both infinities, NaN) in blocks of ties.  -> batch, object scores"""
    g = torch.Generator().manual_seed(seed)
    B = 6
    lengths = torch.tensor([1, min(2, T), T, T, T, max(T - 1, 1)])
    real = torch.rand(B, T, N, generator=g) < 0.6
    real[3] = False
    real[:, :, 0] = True
    for b in range(B):
        real[b, int(lengths[b]) - 1:, 1:] = False  # the extract frame and the padding hold no object
    cats = torch.where(real, torch.randint(1, 5, (B, T, N), generator=g), torch.zeros((), dtype=torch.int64))
    kpm = cats == 0
    boxes = torch.where(kpm[..., None], torch.zeros(()), torch.rand(B, T, N, 4, generator=g))
    ft = torch.full((B, T), REGULAR)
    ft[~real[:, :, 1:].any(-1)] = EMPTY
    for b in range(B):
        ft[b, int(lengths[b]) - 1] = EXTRACT
        ft[b, int(lengths[b]):] = 0
    batch = {"categories": cats, "boxes": boxes, "src_key_padding_mask_boxes": kpm, "frame_types": ft, "src_key_padding_mask_frames": ft == 0, "lengths": lengths}
    if with_scores:
        batch["scores"] = torch.where(kpm, torch.zeros(()), 0.5 + 0.5 * torch.rand(B, T, N, generator=g))
    scores = torch.randn(B, T, N, generator=g)
    scores[4] = 0.75
    blocks = torch.round(torch.randn(T, N, generator=g) * 2) / 2
    pick = torch.rand(T, N, generator=g)
    for lo, v in ((0.0, -0.0), (0.1, 0.0), (0.2, math.inf), (0.3, -math.inf), (0.4, math.nan)):
        blocks[(pick >= lo) & (pick < lo + 0.1)] = v
    scores[5] = blocks
    scores[2, 0] = scores[2, -1]  # the CLS slots and the extract frame carry scores too: they must not matter
    return batch, scores


def run_rank(lib, arena, batch, scores, unit, descending, misalign=None):
    B, T, N = batch["categories"].shape
    shape = (B, T, N) if unit == "object" else (B, T)
    specs = {"scores": (scores, "in"), "kpm": (batch["src_key_padding_mask_boxes"].to(torch.uint8), "extent", 1), "lengths": (batch["lengths"], "extent", 1),
             "rank": (Out(shape, torch.int32), "out"), "n_cand": (Out((B,), torch.int32), "out")}
    call = lambda o: lib.stlt_perturb_rank(o.scores.ptr, o.kpm.ptr, o.lengths.ptr, B, T, N, R.UNITS.index(unit), int(descending), o.rank.ptr, o.n_cand.ptr, stream())  # noqa: E731
    return three_ways(lib, arena, specs, call, ("rank", "n_cand"), misalign=misalign)


_APPLY_OUT = (("categories", torch.int64, 3), ("boxes", torch.float32, 4), ("scores", torch.float32, 3), ("src_key_padding_mask_boxes", torch.uint8, 3),
              ("frame_types", torch.int64, 2), ("src_key_padding_mask_frames", torch.uint8, 2), ("lengths", torch.int64, 1))
_FIELD = {"src_key_padding_mask_boxes": "kpm_boxes", "src_key_padding_mask_frames": "kpm_frames"}


def run_apply(lib, arena, L, batch, rank, n_cand, steps, s0, s1, misalign=None):
    B, T, N = batch["categories"].shape
    n = s1 - s0 + 1
    dims = {3: (T, N), 4: (T, N, 4), 2: (T,), 1: ()}
    specs = {"rank": (rank, "extent", -1), "n_cand": (n_cand, "extent", 0), "removed": (torch.full((steps + 1, B), -1, dtype=torch.int32), "out")}  # rows outside [s0, s1] must keep what they held
    for key, dtype, nd in _APPLY_OUT:
        if key not in batch:
            continue
        host = batch[key].to(dtype).contiguous()
        specs["in_" + key] = (host, "in") if dtype == torch.float32 else (host, "extent", 0)
        specs["out_" + key] = (Out((n * B,) + dims[nd], dtype), "out")

    def call(o):
        inp = L.Inputs()
        inp.B, inp.T, inp.N = B, T, N
        for key, _, _ in _APPLY_OUT:
            if key in batch:
                setattr(inp, _FIELD.get(key, key), getattr(o, "in_" + key).ptr)
        outs = [getattr(o, "out_" + key).ptr if key in batch else None for key, _, _ in _APPLY_OUT]
        return lib.stlt_perturb_apply(C.byref(inp), o.rank.ptr, o.n_cand.ptr, 0 if rank.dim() == 3 else 1, steps, s0, s1, EMPTY, *outs, o.removed.ptr, stream())

    return three_ways(lib, arena, specs, call, ["removed"] + ["out_" + k for k, _, _ in _APPLY_OUT if k in batch], misalign=misalign)


@pytest.mark.parametrize("T,N", SHAPES)
def test_rank_and_apply_kernels_equal_the_restatement(T, N, lib, arena, pkg):
    L = pkg._lib
    batch, obj_scores = kernel_case(T, N, with_scores=(T + N) % 2 == 0, seed=T * 1000 + N)
    nb = {k: v.numpy() for k, v in batch.items()}
    B = batch["categories"].shape[0]
    max_cand = int(R.candidates(nb["src_key_padding_mask_boxes"], nb["lengths"], "object").sum(axis=(1, 2)).max())
    for unit in R.UNITS:
        scores = obj_scores if unit == "object" else obj_scores[:, :, min(1, N - 1)].contiguous()
        for descending in (True, False):
            got = run_rank(lib, arena, batch, scores, unit, descending)
            want_rank, want_n = R.rank(scores.numpy(), nb["src_key_padding_mask_boxes"], nb["lengths"], unit, descending)
            assert np.array_equal(got["rank"].numpy(), want_rank), (unit, descending)
            assert np.array_equal(got["n_cand"].numpy(), want_n), (unit, descending)
            assert want_n[0] == 0 and want_n[3] == 0 and (T < 3 or want_n[2] > 0)
            # steps 1, 3, 10 and a count above the candidates'; ranges that split S
            for steps, ranges in ((1, [(0, 1)]), (3, [(0, 3)]), (10, [(0, 4), (5, 10)]), (max_cand + 3, [(max_cand, max_cand + 3), (2, 2)])):
                for s0, s1 in ranges:
                    out = run_apply(lib, arena, L, batch, got["rank"], got["n_cand"], steps, s0, s1)
                    want = R.apply(nb, want_rank, want_n, steps, s0, s1, EMPTY)
                    for key, dtype, _ in _APPLY_OUT:
                        if key in batch:
                            assert PC.same_bits(out["out_" + key], torch.from_numpy(want[key]).to(dtype)), (unit, descending, steps, s0, s1, key)
                    assert np.array_equal(out["removed"][s0:s1 + 1].numpy(), want["removed"]), (unit, descending, steps, s0, s1)
                    assert (out["removed"][:s0] == -1).all() and (out["removed"][s1 + 1:] == -1).all()
                    if s0 == 0:
                        for key, dtype, _ in _APPLY_OUT:
                            if key in batch:
                                assert PC.same_bits(out["out_" + key][:B], batch[key].to(dtype)), key


def test_pointers_need_only_the_alignment_of_their_element_type(lib, arena, pkg):
    """include/stlt_hip.h: every access of the three launchers is one element wide.  Every operand sits one element past a 256-byte boundary."""
    T, N = 5, 7
    batch, scores = kernel_case(T, N, with_scores=True, seed=77)
    nb = {k: v.numpy() for k, v in batch.items()}
    for unit in R.UNITS:
        sc = scores if unit == "object" else scores[:, :, 1].contiguous()
        got = run_rank(lib, arena, batch, sc, unit, True, misalign={"scores": 4, "kpm": 1, "lengths": 8, "rank": 4, "n_cand": 4})
        want_rank, want_n = R.rank(sc.numpy(), nb["src_key_padding_mask_boxes"], nb["lengths"], unit, True)
        assert np.array_equal(got["rank"].numpy(), want_rank) and np.array_equal(got["n_cand"].numpy(), want_n)
        mis = {"rank": 4, "n_cand": 4, "removed": 4}
        for key, dtype, _ in _APPLY_OUT:
            size = torch.empty((), dtype=dtype).element_size()
            mis["in_" + key], mis["out_" + key] = size, 3 * size if size == 1 else size
        out = run_apply(lib, arena, pkg._lib, batch, got["rank"], got["n_cand"], 3, 1, 3, misalign=mis)
        want = R.apply(nb, want_rank, want_n, 3, 1, 3, EMPTY)
        for key, dtype, _ in _APPLY_OUT:
            assert PC.same_bits(out["out_" + key], torch.from_numpy(want[key]).to(dtype)), (unit, key)
    x, target, _ = curve_case(65, seed=1)
    S, B, K = x.shape
    specs = {"logits": (x.reshape(S * B, K).contiguous(), "in"), "target": (target, "extent", 0), "prob": (Out((S, B)), "out"), "hit": (Out((S, B), torch.uint8), "out"),
             "target_out": (Out((B,), torch.int64), "out")}
    call = lambda o: lib.stlt_perturb_curve(o.logits.ptr, K, o.target.ptr, 0, S, B, K, o.prob.ptr, o.hit.ptr, o.target_out.ptr, stream())  # noqa: E731
    got = three_ways(lib, arena, specs, call, ("prob", "hit", "target_out"), misalign={"logits": 4, "target": 8, "prob": 4, "hit": 1, "target_out": 8})
    ref_prob, ref_hit, _ = R.curve(x.numpy(), target.numpy())
    assert np.array_equal(got["hit"].numpy().astype(bool), ref_hit) and np.abs(got["prob"].numpy() - ref_prob).max() <= 1e-6 and torch.equal(got["target_out"], target)


def test_the_domain_ends_at_16384_slots(lib, arena):
    assert lib.stlt_perturb_max_items() == 128 * 128
    B, T, N = 1, 129, 128
    arena.reset()
    sc = arena.place(torch.zeros(B, T, N), "in")
    kpm = arena.place(torch.ones(B, T, N, dtype=torch.uint8), "extent", band=1)
    ln = arena.place(torch.tensor([T]), "extent", band=1)
    rank, n_cand = arena.place(Out((B, T, N), torch.int32), "out"), arena.place(Out((B,), torch.int32), "out")
    for unit in (0, 1):
        assert lib.stlt_perturb_rank(sc.ptr, kpm.ptr, ln.ptr, B, T, N, unit, 1, rank.ptr, n_cand.ptr, stream()) == STLT_EINVAL
        assert "16384" in last_error(lib)
    arena.check(launched=False)


def test_launchers_refuse_bad_arguments_without_launching(lib, arena, pkg):
    L = pkg._lib
    B, T, N = 2, 3, 4
    arena.reset()
    sc = arena.place(torch.zeros(B, T, N), "in")
    kpm = arena.place(torch.zeros(B, T, N, dtype=torch.uint8), "extent", band=1)
    ln = arena.place(torch.tensor([T, T]), "extent", band=1)
    rank, n_cand = arena.place(Out((B, T, N), torch.int32), "out"), arena.place(Out((B,), torch.int32), "out")
    prob, hit, tgt = arena.place(Out((2, B)), "out"), arena.place(Out((2, B), torch.uint8), "out"), arena.place(Out((B,), torch.int64), "out")
    s = stream()
    bad_rank = [(None, kpm.ptr, ln.ptr, B, T, N, 0, 1, rank.ptr, n_cand.ptr), (sc.ptr, kpm.ptr, ln.ptr, B, T, N, 0, 1, None, n_cand.ptr),
                (sc.ptr, kpm.ptr, ln.ptr, B, 0, N, 0, 1, rank.ptr, n_cand.ptr), (sc.ptr, kpm.ptr, ln.ptr, -1, T, N, 0, 1, rank.ptr, n_cand.ptr),
                (sc.ptr, kpm.ptr, ln.ptr, B, T, N, 2, 1, rank.ptr, n_cand.ptr), (sc.ptr, kpm.ptr, ln.ptr, B, T, N, 0, 2, rank.ptr, n_cand.ptr)]
    for a in bad_rank:
        assert lib.stlt_perturb_rank(*a, s) == STLT_EINVAL and "stlt_perturb_rank" in last_error(lib), a
    inp = L.Inputs()
    inp.B, inp.T, inp.N = B, T, N
    for f in ("categories", "boxes", "kpm_boxes", "frame_types", "kpm_frames", "lengths"):
        setattr(inp, f, sc.ptr)  # never read: every call below is refused
    outs = [sc.ptr] * 7
    for steps, s0, s1 in ((0, 0, 0), (3, -1, 2), (3, 2, 1), (3, 0, 4)):
        assert lib.stlt_perturb_apply(C.byref(inp), rank.ptr, n_cand.ptr, 0, steps, s0, s1, EMPTY, *outs, rank.ptr, s) == STLT_EINVAL and "steps" in last_error(lib)
    assert lib.stlt_perturb_apply(C.byref(inp), rank.ptr, n_cand.ptr, 0, 3, 0, 3, EMPTY, *outs, None, s) == STLT_EINVAL
    assert lib.stlt_perturb_apply(C.byref(inp), None, n_cand.ptr, 0, 3, 0, 3, EMPTY, *outs, rank.ptr, s) == STLT_EINVAL
    assert lib.stlt_perturb_apply(None, rank.ptr, n_cand.ptr, 0, 3, 0, 3, EMPTY, *outs, rank.ptr, s) == STLT_EINVAL
    for a in ((None, 4, None, 0, 2, B, 4, prob.ptr, hit.ptr, tgt.ptr), (sc.ptr, 3, None, 0, 2, B, 4, prob.ptr, hit.ptr, tgt.ptr), (sc.ptr, 4, None, 2, 2, B, 4, prob.ptr, hit.ptr, tgt.ptr),
              (sc.ptr, 4, None, 0, 0, B, 4, prob.ptr, hit.ptr, tgt.ptr), (sc.ptr, 4, None, 0, 2, B, 0, prob.ptr, hit.ptr, tgt.ptr), (sc.ptr, 4, None, 0, 2, B, 4, prob.ptr, hit.ptr, None),
              (sc.ptr, 4, None, 0, 2, B, 4, None, hit.ptr, tgt.ptr)):
        assert lib.stlt_perturb_curve(*a, s) == STLT_EINVAL and "stlt_perturb_curve" in last_error(lib), a
    arena.check(launched=False)


# ---- the curve kernel ------------------------------------------------------------------------------------------------------------------
CURVE_SCALES = (1e-3, 1.0, 30.0, 1e3)
CURVE_KINDS = ("maximum", "minimum", "tied with a lower index", "tied with a higher index", "out of range")


def curve_case(K, seed):
    """(S,B,K) logits, S = 3, one clip per (scale, kind of target): rows of every scale in one batch.  -> logits, target, scale name per clip"""
    g = torch.Generator().manual_seed(seed)
    S, B = 3, len(CURVE_SCALES) * len(CURVE_KINDS)
    x = torch.randn(S, B, K, generator=g)
    target = torch.zeros(B, dtype=torch.int64)
    group = []
    for b in range(B):
        scale, kind = CURVE_SCALES[b // len(CURVE_KINDS)], CURVE_KINDS[b % len(CURVE_KINDS)]
        x[:, b] *= scale
        group.append(f"scale {scale:g}")
        if kind == "maximum":
            target[b] = x[1, b].argmax()
        elif kind == "minimum":
            target[b] = x[1, b].argmin()
        elif kind == "out of range":
            target[b] = K if b % 2 else -1
        else:
            t = K // 2
            j = t - 1 if kind == "tied with a lower index" else t + 1
            target[b] = t
            top = x[:, b].max(dim=1).values + scale
            x[:, b, t] = top
            if 0 <= j < K:
                x[:, b, j] = top
    x[0, 0, K - 1] = x[0, 0, 0] = x[0, 0].max() + 1  # a tie at the top of a step-0 row: the NULL-target arg-max takes the first
    return x, target, group


@pytest.mark.parametrize("activation", ["softmax", "sigmoid"])
@pytest.mark.parametrize("K", [1, 2, 64, 65, 174, 300])
def test_curve_kernel_against_fp64(K, activation, lib, arena):
    x, target, group = curve_case(K, seed=K)
    S, B, _ = x.shape
    ld = K + 3
    pitched = torch.full((S * B, ld), float("nan"))
    pitched[:, :K] = x.reshape(S * B, K)
    act = ("softmax", "sigmoid").index(activation)
    yard = torch.softmax(x, dim=2) if activation == "softmax" else torch.sigmoid(x)  # torch's fp32 on the CPU, the same rows
    for tgt in (target, None):
        specs = {"logits": (pitched, "in"), "prob": (Out((S, B)), "out"), "hit": (Out((S, B), torch.uint8), "out"), "target_out": (Out((B,), torch.int64), "out")}
        if tgt is not None:
            specs["target"] = (tgt, "extent", 0)
        call = lambda o: lib.stlt_perturb_curve(o.logits.ptr, ld, o.target.ptr if tgt is not None else None, act, S, B, K, o.prob.ptr, o.hit.ptr, o.target_out.ptr, stream())  # noqa: E731
        got = three_ways(lib, arena, specs, call, ("prob", "hit", "target_out"))
        ref_prob, ref_hit, ref_target = R.curve(x.numpy(), None if tgt is None else tgt.numpy(), activation)
        assert np.array_equal(got["target_out"].numpy(), ref_target)
        if tgt is None:
            assert int(got["target_out"][0]) == 0
        assert np.array_equal(got["hit"].numpy().astype(bool), ref_hit)
        valid = torch.from_numpy((ref_target >= 0) & (ref_target < K))
        idx = torch.from_numpy(ref_target).clamp(0, K - 1)[None, :, None].expand(S, B, 1)
        yard_t = torch.where(valid[None], yard.gather(2, idx)[..., 0], torch.zeros(()))
        o = SC.out(torch.from_numpy(ref_prob).reshape(S * B, 1), yard_t.reshape(S * B, 1), group * S)  # one element per row, grouped by scale
        _, fails = SC.judge(f"perturb_curve {activation} K={K} target {'given' if tgt is not None else 'NULL'}", got["prob"], o)
        assert not fails, "\n".join(fails)
        assert (got["prob"][:, ~valid] == 0).all()
        # Where the probability underflows fp32 torch returns 0 too, E_t of that group is 1 and the rule above says nothing.  The number
        # format does: a probability that is a normal fp32 number is held to 4 u on its own, one below half the smallest subnormal is 0.
        p, ref = got["prob"].double().numpy(), ref_prob
        normal, gone = ref >= 2.0 ** -126, ref < 2.0 ** -150
        assert (np.abs(p - ref)[normal] <= SC.MARGIN * SC.U * ref[normal]).all() and (p[gone] == 0).all()


# ---- the whole path --------------------------------------------------------------------------------------------------------------------
_MODELS = {}


def model_of(pkg, name):
    """the fixture's model on the device — built once per config, shared, left in inference mode with skip_padding off"""
    if name not in _MODELS:
        m = pkg.Stlt(pkg.StltModelConfig(**pkg.synth.model_kwargs(name)))
        m.load_state_dict(PC.fixture(name)["sd"], strict=True)
        _MODELS[name] = m.train(False).to(DEV)
    return _MODELS[name]


def on_device(batch):
    return {k: (v.to(DEV) if isinstance(v, torch.Tensor) else v) for k, v in batch.items()}


@pytest.mark.parametrize("skip_padding", [False, True])
@pytest.mark.parametrize("name", PC.CONFIGS)
def test_forward_perturbed_against_the_fixtures(name, skip_padding, pkg):
    fx = PC.fixture(name)
    m = model_of(pkg, name)
    z, S, B = fx["z"], fx["steps"] + 1, fx["batch"]["categories"].shape[0]
    dev = on_device(fx["batch"])
    if skip_padding:
        dev.update(pkg.collate.real_counts(fx["batch"]))  # carried as upper bounds: nothing is read back
    m.backbone.skip_padding = skip_padding
    try:
        for order, unit in PC.COMBOS:
            tag = f"{order}_{unit}"
            out = m.forward_perturbed(dev, fx["scores"][unit].to(DEV), steps=fx["steps"], order=order, unit=unit, dataset_name=fx["dataset"])
            ref = z[f"logits_{tag}"]
            err = np.abs(out["stlt"].cpu().numpy() - ref).max()
            print(f"[perturbation] {name} {tag} skip_padding={skip_padding}: max|logits - reference| = {err:.2e}")
            assert tuple(out["stlt"].shape) == (S, B, ref.shape[2]) and err <= TOL, (tag, err)
            ref_prob, ref_hit, ref_target = R.curve(ref)
            assert np.array_equal(out["target"].cpu().numpy(), ref_target), tag
            assert np.abs(out["prob"].cpu().numpy() - ref_prob).max() <= TOL, tag
            sure = z[f"margin_{tag}"] >= 1e-3
            assert sure.mean() >= 0.95 and np.array_equal(out["hit"].cpu().numpy()[sure], ref_hit[sure]), tag
            assert out["hit"].dtype == torch.bool
            assert np.array_equal(out["removed"].cpu().numpy(), z[f"removed_{tag}"]) and np.array_equal(out["n_candidates"].cpu().numpy(), z[f"n_candidates_{tag}"]), tag
            auc = (ref_prob[1:] + ref_prob[:-1]).sum(0) / 2 / fx["steps"]
            assert np.abs(out["auc"].cpu().numpy() - auc).max() <= TOL, tag
    finally:
        m.backbone.skip_padding = False


@pytest.mark.parametrize("name", ["cfg1", "cfg4"])
def test_device_perturb_batch_equals_the_fixtures_and_one_pass_equals_the_plain_forward(name, pkg):
    fx = PC.fixture(name)
    m = model_of(pkg, name)
    S, B = fx["steps"] + 1, fx["batch"]["categories"].shape[0]
    dev = on_device(fx["batch"])
    for order, unit in PC.COMBOS:
        scores = fx["scores"][unit].to(DEV)
        pb = pkg.collate.perturb_batch(dev, scores, steps=fx["steps"], order=order, unit=unit, dataset_name=fx["dataset"])
        for k, v in PC.expected_batch(fx, order, unit).items():
            assert PC.same_bits(pb[k], v), (order, unit, k)
        assert np.array_equal(pb["removed"].cpu().numpy(), fx["z"][f"removed_{order}_{unit}"])
        with torch.no_grad():
            plain = m(pb)["stlt"]
        whole = m.forward_perturbed(dev, scores, steps=fx["steps"], order=order, unit=unit, dataset_name=fx["dataset"], steps_per_pass=S)
        assert torch.equal(whole["stlt"].view(S * B, -1), plain), (order, unit)
        for per in (1, 2):
            part = m.forward_perturbed(dev, scores, steps=fx["steps"], order=order, unit=unit, dataset_name=fx["dataset"], steps_per_pass=per)
            assert (part["stlt"] - whole["stlt"]).abs().max().item() <= TOL, (order, unit, per)
            assert torch.equal(part["removed"], whole["removed"]) and torch.equal(part["target"], whole["target"])
    # a given target: the curves follow that class
    target = torch.arange(B, device=DEV) % whole["stlt"].shape[2]
    given = m.forward_perturbed(dev, scores, steps=fx["steps"], order=order, unit=unit, dataset_name=fx["dataset"], target=target)
    assert torch.equal(given["target"], target) and torch.equal(given["stlt"], whole["stlt"])
    ref_prob, ref_hit, _ = R.curve(given["stlt"].cpu().numpy(), target.cpu().numpy())
    assert np.abs(given["prob"].cpu().numpy() - ref_prob).max() <= 1e-6 and np.array_equal(given["hit"].cpu().numpy(), ref_hit)


@pytest.mark.parametrize("skip_padding", [False, True])
def test_one_captured_graph_of_forward_perturbed_replays_to_the_same_bits(skip_padding, pkg):
    """Capture fails on any stream synchronisation: with the batch's row counts carried, skip-padding included, the call makes none."""
    name = "cfg1"
    fx = PC.fixture(name)
    m = model_of(pkg, name)
    static = on_device(fx["batch"])
    static.update(pkg.collate.real_counts(fx["batch"]))
    scores = fx["scores"]["object"].to(DEV)
    m.backbone.skip_padding = skip_padding
    try:
        run = lambda: m.forward_perturbed(static, scores, steps=fx["steps"], steps_per_pass=2)  # noqa: E731
        eager = {k: v.clone() for k, v in run().items()}
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            run()
        torch.cuda.current_stream().wait_stream(side)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            out = run()
        for _ in range(2):
            g.replay()
            torch.cuda.synchronize()
            for k, v in eager.items():
                assert torch.equal(out[k], v), k
        # other scores through the same graph
        scores.copy_(torch.flip(fx["scores"]["object"], dims=(1,)).to(DEV))
        g.replay()
        torch.cuda.synchronize()
        again = run()
        assert all(torch.equal(out[k], again[k]) for k in eager) and not torch.equal(out["stlt"], eager["stlt"])
    finally:
        m.backbone.skip_padding = False


@pytest.mark.parametrize("method", ["relevance", "saliency", "attention"])
def test_runner_end_to_end_reproduces_forward_perturbed_called_by_hand(method, pkg):
    name = "cfg1"
    fx = PC.fixture(name)
    m = model_of(pkg, name)
    B = fx["batch"]["categories"].shape[0]
    K = pkg.synth.CONFIGS[name]["num_classes"]
    batches = [dict(fx["batch"], labels=torch.arange(B) % K), dict({k: v[:3] for k, v in fx["batch"].items()}, labels=torch.tensor([5, 0, 7]))]
    for unit, target in (("object", "top1"), ("frame", "label")):
        res = pkg.infer.run_perturbation_test(m, batches, method=method, steps=4, unit=unit, target=target)
        for order in R.ORDERS:
            prob, hits, n = torch.zeros(5, dtype=torch.float64), torch.zeros(5, dtype=torch.int64), 0
            for b in batches:
                dev = on_device(b)
                scores = pkg.infer.attribution_scores(m, dev, method)
                assert tuple(scores.shape) == tuple(dev["categories"].shape) and bool(torch.isfinite(scores).all())
                scores = scores if unit == "object" else scores[:, :, 1:].sum(2)
                out = m.forward_perturbed(dev, scores.contiguous(), steps=4, order=order, unit=unit, target=dev["labels"] if target == "label" else None)
                prob += out["prob"].sum(1, dtype=torch.float64).cpu()
                hits += out["hit"].sum(1).cpu()
                n += dev["categories"].shape[0]
            r = res[order]
            assert r["num_clips"] == n == B + 3
            assert r["prob"] == (prob / n).tolist() and r["accuracy"] == (hits.double() / n).tolist(), (unit, order)
            assert abs(r["auc_prob"] - float((prob[1:] + prob[:-1]).sum() / 2 / 4 / n)) <= 1e-12
    # the runner through `forward=` (collate.perturb_batch + the model's plain forward) gives the same curves
    with torch.no_grad():
        via = pkg.infer.run_perturbation_test(m, batches, method=method, steps=4, unit="frame", target="label", forward=lambda pb: m(pb)["stlt"])
    for order in R.ORDERS:
        assert via[order]["accuracy"] == res[order]["accuracy"] and np.abs(np.array(via[order]["prob"]) - np.array(res[order]["prob"])).max() <= 1e-12


def test_refusals(pkg):
    name = "micro"
    fx = PC.fixture(name)
    m = model_of(pkg, name)
    dev = on_device(fx["batch"])
    obj, frm = fx["scores"]["object"].to(DEV), fx["scores"]["frame"].to(DEV)
    E = pkg.StltHipError
    with pytest.raises(E, match="GPU tensor"):
        pkg.ops.perturb_rank(fx["scores"]["object"], dev["src_key_padding_mask_boxes"], dev["lengths"])
    with pytest.raises(E, match="GPU tensor"):
        pkg.ops.perturb_curve(torch.zeros(2, 2, 3))
    with pytest.raises(E, match="GPU tensor"):
        pkg.ops.perturb_apply(fx["batch"], torch.zeros(4, 5, 3, dtype=torch.int32, device=DEV), torch.zeros(4, dtype=torch.int32, device=DEV), 3, 0, 3, EMPTY)
    with pytest.raises(E, match="CPU tensors"):
        m.forward_perturbed(fx["batch"], fx["scores"]["object"])
    with pytest.raises(E, match="CPU tensors"):
        m.forward_perturbed(dev, fx["scores"]["object"])
    with pytest.raises(E, match="unit 'object' takes"):
        m.forward_perturbed(dev, frm)
    with pytest.raises(E, match="unit 'frame' takes"):
        m.forward_perturbed(dev, obj, unit="frame")
    with pytest.raises(E, match="steps must be >= 1"):
        m.forward_perturbed(dev, obj, steps=0)
    with pytest.raises(E, match="steps_per_pass"):
        m.forward_perturbed(dev, obj, steps_per_pass=0)
    with pytest.raises(E, match="order"):
        m.forward_perturbed(dev, obj, order="up")
    with pytest.raises(E, match="unit"):
        m.forward_perturbed(dev, obj, unit="pixel")
    with pytest.raises(E, match="target"):
        m.forward_perturbed(dev, obj, target=torch.zeros(4, device=DEV))
    with pytest.raises(E, match="activation"):
        pkg.ops.perturb_curve(torch.zeros(2, 2, 3, device=DEV), activation="tanh")
    with pytest.raises(E, match="steps"):
        rank, n = pkg.ops.perturb_rank(obj, dev["src_key_padding_mask_boxes"], dev["lengths"])
        pkg.ops.perturb_apply(dev, rank, n, 3, 2, 4, EMPTY)
    big = on_device(pkg.synth.make_batch(1, 129, 128, seed=0))
    with pytest.raises(E, match="16384"):
        pkg.ops.perturb_rank(torch.zeros(1, 129, 128, device=DEV), big["src_key_padding_mask_boxes"], big["lengths"])
    with pytest.raises(E, match="16384"):
        pkg.collate.perturb_batch(big, torch.zeros(1, 129, 128, device=DEV))
    kw = pkg.synth.model_kwargs(name)
    kw["hidden_dropout_prob"] = 0.1
    live = pkg.Stlt(pkg.StltModelConfig(**kw))
    live.load_state_dict(fx["sd"], strict=True)
    live.train(True).to(DEV)
    with pytest.raises(E, match="dropout"):
        live.forward_perturbed(dev, obj)
