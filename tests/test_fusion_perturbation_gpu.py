"""The appearance side of the perturbation test on the GPU: the three cell kernels alone against the torch restatement
(tests/fusion_perturbation_restated.py) inside guard bands, forward_perturbed of Resnet3D, TransformerResnet and CACNF against the fixtures
the reference made (tests/golden/fusion_perturbation_<model>.npz), one pass against the plain forward, a captured graph, the runner end to
end, and the refusals."""
import importlib
import json
import os

import numpy as np
import pytest
import torch

import fusion_perturbation_restated as FR
import perturbation_restated as R
from conftest import GOLDEN, PKG_NAME
from guard_arena import STLT_EINVAL, Arena, Out, last_error, stream, three_ways
from perturbation_cases import same_bits

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TOL = 1e-4  # the bound tests/test_r3d_gpu.py holds these models to against the reference's goldens
# (x shape, cell, what the case is there for)
KERNEL_CASES = [((2, 3, 20, 40, 70), (16, 32, 32), "grid 2x2x3, ragged last cells on every axis, W % 4 != 0: the scalar path"),
                ((3, 3, 16, 64, 64), (16, 32, 32), "aligned: the 16-byte path"),
                ((2, 8, 2, 3, 3), (1, 1, 1), "the feature-space form")]


@pytest.fixture(scope="module")
def lib():
    return importlib.import_module(PKG_NAME + "._lib").load()


@pytest.fixture(scope="module")
def arena():
    return Arena(192 << 20, DEV)


def _x(shape, seed=0, nan=False):
    x = torch.randn(shape, generator=torch.Generator().manual_seed(seed))
    x.view(-1)[::7] = 0.0  # values equal to the default fill: the mask, not the value, says what was deleted
    x.view(-1)[4] = -0.0
    if nan:  # moved as bits (not through the guard-band harness, which compares its runs as floats)
        x.view(-1)[3] = float("nan")
    return x


def _n_cells(shape, cell):
    g = FR.grid(shape[2:], cell)
    return g[0] * g[1] * g[2]


def run_rank_cells(lib, arena, scores, descending, misalign=None):
    B, C = scores.shape
    specs = {"scores": (scores, "in"), "rank": (Out((B, C), torch.int32), "out"), "n_cand": (Out((B,), torch.int32), "out")}
    call = lambda o: lib.stlt_perturb_rank_cells(o.scores.ptr, B, C, int(descending), o.rank.ptr, o.n_cand.ptr, stream())  # noqa: E731
    return three_ways(lib, arena, specs, call, ("rank", "n_cand"), misalign=misalign)


def run_apply_cells(lib, arena, x, cell, rank, n_cand, steps, s0, s1, fill, misalign=None, with_removed=True):
    B, Cch, T, H, W = x.shape
    n = s1 - s0 + 1
    specs = {"x": (x, "in"), "rank": (rank, "extent", -1), "n_cand": (n_cand, "extent", 0), "out": (Out((n * B, Cch, T, H, W)), "out")}
    if with_removed:
        specs["removed"] = (Out((n, B), torch.int32), "out")
    call = lambda o: lib.stlt_perturb_apply_cells(o.x.ptr, B, Cch, T, H, W, *cell, o.rank.ptr, o.n_cand.ptr, steps, s0, s1, fill, o.out.ptr,  # noqa: E731
                                                  o.removed.ptr if with_removed else None, stream())
    return three_ways(lib, arena, specs, call, ["out"] + (["removed"] if with_removed else []), misalign=misalign)


@pytest.mark.parametrize("shape,cell,why", KERNEL_CASES)
def test_rank_and_apply_kernels_equal_the_restatement(shape, cell, why, lib, arena):
    x = _x(shape, seed=shape[3])
    B, C = shape[0], _n_cells(shape, cell)
    scores = FR.special_scores(B, C, seed=C)  # ties, both zeros, both infinities, NaN; clip 0 all equal
    for descending in (True, False):
        got = run_rank_cells(lib, arena, scores, descending)
        want_rank, want_n = FR.rank_cells(scores, descending)
        assert torch.equal(got["rank"], want_rank) and torch.equal(got["n_cand"], want_n), (why, descending)
        assert want_rank[0].tolist() == list(range(C))
        # steps 1, 3, a count above the cells'; sub-ranges that split S, against the full range
        for steps, ranges, fill in ((1, [(0, 1)], 0.0), (3, [(0, 3), (0, 1), (2, 3)], 0.0), (C + 3, [(C, C + 3), (2, 2)], -1.5)):
            full, full_removed = FR.apply_cells(x, cell, want_rank, want_n, steps, 0, steps, fill)
            full = full.view(steps + 1, *shape)
            for s0, s1 in ranges:
                out = run_apply_cells(lib, arena, x, cell, got["rank"], got["n_cand"], steps, s0, s1, fill)
                assert same_bits(out["out"], full[s0:s1 + 1].reshape(-1, *shape[1:])), (why, descending, steps, s0, s1)
                assert torch.equal(out["removed"], full_removed[s0:s1 + 1]), (why, descending, steps, s0, s1)
                if s0 == 0:
                    assert same_bits(out["out"][:B], x)
                if s1 == steps:
                    assert (out["out"][-B:].view(torch.int32) == torch.tensor(fill).view(torch.int32)).all()
    # removed is optional
    out = run_apply_cells(lib, arena, x, cell, want_rank, want_n, 3, 1, 2, 0.0, with_removed=False)
    assert same_bits(out["out"], FR.apply_cells(x, cell, want_rank, want_n, 3, 1, 2, 0.0)[0])


def test_the_aligned_case_four_bytes_off_takes_the_scalar_path_to_the_same_bits(lib, arena):
    shape, cell, _ = KERNEL_CASES[1]
    x = _x(shape, seed=9)
    B, C = shape[0], _n_cells(shape, cell)
    scores = FR.special_scores(B, C, seed=2)
    rank, n = FR.rank_cells(scores, True)
    want, want_removed = FR.apply_cells(x, cell, rank, n, 3, 0, 3, 0.0)
    for mis in ({"x": 4, "out": 4}, {"x": 4}, {"out": 4}, {"x": 16, "out": 32}, {"rank": 4, "n_cand": 4, "removed": 4, "x": 8, "out": 12}):
        out = run_apply_cells(lib, arena, x, cell, rank, n, 3, 0, 3, 0.0, misalign=mis)
        assert same_bits(out["out"], want) and torch.equal(out["removed"], want_removed), mis
    got = run_rank_cells(lib, arena, scores, True, misalign={"scores": 4, "rank": 4, "n_cand": 4})
    assert torch.equal(got["rank"], rank)


@pytest.mark.parametrize("C", [1, 2, 3, 255, 256, 257, 2049, 16384])
def test_rank_cells_at_every_sort_size(C, lib, arena):
    scores = FR.special_scores(2, C, seed=C)
    for descending in (True, False):
        got = run_rank_cells(lib, arena, scores, descending)
        want, n = FR.rank_cells(scores, descending)
        assert torch.equal(got["rank"], want) and got["n_cand"].tolist() == [C, C]


def test_many_cells_in_lds(lib, arena):
    """16384 feature columns: every workgroup of the apply kernel holds the whole rank table in 64 KB of LDS"""
    shape, cell = (2, 2, 4, 64, 64), (1, 1, 1)
    x = _x(shape, seed=5)
    C = _n_cells(shape, cell)
    assert C == 16384
    rank, n = FR.rank_cells(torch.randn(2, C, generator=torch.Generator().manual_seed(1)), True)
    counts = FR.removal_counts(n, 4, 1, 2)
    out = run_apply_cells(lib, arena, x, cell, rank, n, 4, 1, 2, 0.0)
    gone = (rank.long()[None] < counts.long()[:, :, None]).view(2, 2, 1, 4, 64, 64)  # cells of 1x1x1: the mask is the rank table itself
    want = torch.where(gone, torch.zeros(()), x[None]).reshape(4, *shape[1:])
    assert same_bits(out["out"], want) and torch.equal(out["removed"], counts)


@pytest.mark.parametrize("shape,cell,why", KERNEL_CASES)
def test_cell_pool_abs_against_fp64(shape, cell, why, lib, arena):
    g = _x(shape, seed=3)
    g = g * torch.logspace(-3, 3, shape[0] * shape[1]).view(shape[0], shape[1], 1, 1, 1)  # channels of very different size in one sum
    B, Cch, T, H, W = shape
    C = _n_cells(shape, cell)
    specs = {"g": (g, "in"), "out": (Out((B, C)), "out")}
    call = lambda o: lib.stlt_cell_pool_abs(o.g.ptr, B, Cch, T, H, W, *cell, o.out.ptr, stream())  # noqa: E731
    got = three_ways(lib, arena, specs, call, ("out",), misalign={"g": 4, "out": 4})["out"]  # three_ways: two launches, the same bits
    ref = FR.cell_pool_abs(g, cell)
    err = ((got.double() - ref).abs() / ref).max().item()
    print(f"[cell_pool_abs] {why}: max relative error {err:.2e}")
    assert ((got.double() - ref).abs() <= 1e-5 * ref).all(), err


def test_launchers_refuse_bad_arguments_without_launching(lib, arena):
    B, Cch, T, H, W, cell = 2, 3, 16, 32, 64, (16, 32, 32)
    arena.reset()
    x = arena.place(torch.zeros(B, Cch, T, H, W), "in")
    sc = arena.place(torch.zeros(B, 2), "in")
    rank = arena.place(torch.zeros(B, 2, dtype=torch.int32), "extent", band=-1)
    n_cand = arena.place(torch.full((B,), 2, dtype=torch.int32), "extent", band=0)
    out = arena.place(Out((4 * B, Cch, T, H, W)), "out")
    removed, pooled = arena.place(Out((4, B), torch.int32), "out"), arena.place(Out((B, 2)), "out")
    rank_out, n_out = arena.place(Out((B, 2), torch.int32), "out"), arena.place(Out((B,), torch.int32), "out")
    s = stream()
    for a in ((None, B, 2, 1, rank_out.ptr, n_out.ptr), (sc.ptr, B, 2, 1, None, n_out.ptr), (sc.ptr, B, 2, 1, rank_out.ptr, None), (sc.ptr, -1, 2, 1, rank_out.ptr, n_out.ptr),
              (sc.ptr, B, 0, 1, rank_out.ptr, n_out.ptr), (sc.ptr, B, 2, 2, rank_out.ptr, n_out.ptr), (sc.ptr, B, 16385, 1, rank_out.ptr, n_out.ptr)):
        assert lib.stlt_perturb_rank_cells(*a, s) == STLT_EINVAL and "stlt_perturb_rank_cells" in last_error(lib), a
    assert "16384" in last_error(lib)
    good = dict(x=x.ptr, B=B, Cch=Cch, T=T, H=H, W=W, ct=cell[0], ch=cell[1], cw=cell[2], rank=rank.ptr, n=n_cand.ptr, steps=3, s0=0, s1=3, fill=0.0, out=out.ptr, removed=removed.ptr)
    bad = [dict(x=None), dict(rank=None), dict(n=None), dict(out=None), dict(B=-1), dict(Cch=0), dict(T=0), dict(H=-3), dict(W=0), dict(ct=0), dict(ch=-1), dict(cw=0),
           dict(steps=0), dict(s0=-1), dict(s0=2, s1=1), dict(s1=4), dict(steps=1 << 31, s1=0), dict(steps=1000, s0=0, s1=256), dict(T=1 << 20, H=1 << 10, W=1 << 10),
           dict(ct=1, ch=1, cw=1)]  # 16 * 32 * 64 cells of 1x1x1: more than a clip is ranked with
    for b in bad:
        a = dict(good, **b)
        assert lib.stlt_perturb_apply_cells(*a.values(), s) == STLT_EINVAL and "stlt_perturb_apply_cells" in last_error(lib), (b, last_error(lib))
        if set(b) <= {"B", "Cch", "T", "H", "W", "ct", "ch", "cw"}:
            pool = [a[k] for k in ("x", "B", "Cch", "T", "H", "W", "ct", "ch", "cw")] + [pooled.ptr]
            assert lib.stlt_cell_pool_abs(*pool, s) == STLT_EINVAL and "stlt_cell_pool_abs" in last_error(lib), b
    assert lib.stlt_cell_pool_abs(None, B, Cch, T, H, W, *cell, pooled.ptr, s) == STLT_EINVAL and lib.stlt_cell_pool_abs(x.ptr, B, Cch, T, H, W, *cell, None, s) == STLT_EINVAL
    arena.check(launched=False)
    # an empty batch is no error and no launch
    assert lib.stlt_perturb_apply_cells(None, 0, Cch, T, H, W, *cell, None, None, 3, 0, 3, 0.0, None, None, s) == 0
    assert lib.stlt_perturb_rank_cells(None, 0, 2, 1, None, None, s) == 0 and lib.stlt_cell_pool_abs(None, 0, Cch, T, H, W, *cell, None, s) == 0
    arena.check(launched=False)


def test_device_perturb_cells_equals_the_restatement(pkg):
    for shape, cell, why in KERNEL_CASES:
        key = "video_frames" if cell != (1, 1, 1) else "appearance_features"
        x = _x(shape, seed=1, nan=True)
        B, C = shape[0], _n_cells(shape, cell)
        scores = FR.special_scores(B, C, 4)
        batch = {key: x, "labels": torch.arange(B)}
        for order in FR.ORDERS:
            want = FR.perturb_cells(batch, scores, steps=3, order=order, step_range=(1, 3), fill=0.5)
            got = pkg.collate.perturb_cells({k: v.to(DEV) for k, v in batch.items()}, scores.to(DEV), steps=3, order=order, step_range=(1, 3), fill=0.5)
            assert got[key].is_cuda and same_bits(got[key], want[key]) and torch.equal(got["removed"].cpu(), want["removed"]), (why, order)
            assert torch.equal(got["labels"].cpu(), want["labels"]) and torch.equal(got["n_candidates"].cpu(), want["n_candidates"])
        assert torch.equal(pkg.ops.cell_pool_abs(x.nan_to_num().to(DEV), cell), pkg.ops.cell_pool_abs(x.nan_to_num().to(DEV), cell))


# ---- the whole path --------------------------------------------------------------------------------------------------------------------
_CACHE = {}


def meta():
    if "meta" not in _CACHE:
        _CACHE["meta"] = json.load(open(os.path.join(GOLDEN, "fusion_perturbation_schema.json")))
    return _CACHE["meta"]


def fixture(name):
    if name not in _CACHE:
        _CACHE[name] = np.load(os.path.join(GOLDEN, f"fusion_perturbation_{name}.npz"))
    return _CACHE[name]


def model_of(pkg, name):
    """the fixture's model on the device: built once, shared, left in inference mode"""
    key = "model_" + name
    if key not in _CACHE:
        m = meta()
        kw = pkg.synth.model_kwargs(m["config"])
        app = dict(num_classes=kw["num_classes"], hidden_size=kw["hidden_size"], num_attention_heads=kw["num_attention_heads"], hidden_dropout_prob=0.0,
                   appearance_num_frames=m["appearance_num_frames"])
        if name == "resnet3d":
            model = pkg.Resnet3D(pkg.AppearanceModelConfig(**app))
        elif name == "transformer":
            model = pkg.TransformerResnet(pkg.AppearanceModelConfig(**app))
        else:
            model = pkg.CrossAttentionCentralNetFusion(pkg.MultimodalModelConfig(**dict(kw, appearance_num_frames=m["appearance_num_frames"], appearance_trunk=True,
                                                                                       num_appearance_layers=m["cacnf_num_appearance_layers"],
                                                                                       num_fusion_layers=m["cacnf_num_fusion_layers"])))
        shapes = {k: tuple(v.shape) for k, v in model.state_dict().items()}
        assert shapes == {k: tuple(v["shape"]) for k, v in m["models"][name]["keys"].items()}, "the fixture was made for other state-dict keys"
        model.load_state_dict(pkg.synth.make_r3d_state_dict(shapes, seed=m["weight_seed"]), strict=True)
        _CACHE[key] = model.to(DEV).train(False)
    return _CACHE[key]


def batch_of(pkg, name):
    m = meta()
    batch = {"video_frames": pkg.synth.make_video(m["clips"], seed=m["video_seed"], **m["video"]).to(DEV)}
    if name == "cacnf":
        c = pkg.synth.CONFIGS[m["config"]]
        batch.update({k: v.to(DEV) for k, v in pkg.synth.make_batch(m["clips"], c["T"], c["N"], seed=m["batch_seed"]).items()})
    return batch


def scores_of(name, modality):
    z = fixture(name)
    cells = torch.from_numpy(z["scores_cells"]).to(DEV)
    return {"layout": torch.from_numpy(z["scores_layout"]).to(DEV), "appearance": cells} if modality == "both" else cells


@pytest.mark.parametrize("name", ["resnet3d", "transformer", "cacnf"])
def test_forward_perturbed_against_the_reference(name, pkg):
    m, z, model, batch = meta(), fixture(name), model_of(pkg, name), batch_of(pkg, name)
    S, B, steps = m["steps"] + 1, m["clips"], m["steps"]
    names = m["models"][name]["logit_names"]
    assert tuple(model.logit_names) == tuple(names)
    for tag in m["models"][name]["cases"]:
        modality, order = tag.split("_")
        out = model.forward_perturbed(batch, scores_of(name, modality), steps=steps, order=order, modality=modality)
        for k in names:
            ref = z[f"logits_{k}_{tag}"]
            err = np.abs(out[k].cpu().numpy() - ref).max()
            print(f"[fusion perturbation] {name} {tag} {k}: max|logits - reference| = {err:.2e}")
            assert tuple(out[k].shape) == ref.shape and err <= TOL, (tag, k, err)
        ref = z[f"logits_{names[-1]}_{tag}"]
        ref_prob, ref_hit, ref_target = R.curve(ref)
        assert np.array_equal(out["target"].cpu().numpy(), ref_target), tag
        assert np.abs(out["prob"].cpu().numpy() - ref_prob).max() <= TOL, tag
        sure = z[f"margin_{tag}"] >= m["margin"]
        assert sure.mean() >= 1 - m["cap"] and np.array_equal(out["hit"].cpu().numpy()[sure], ref_hit[sure]) and out["hit"].dtype == torch.bool, tag
        auc = (ref_prob[1:] + ref_prob[:-1]).sum(0) / 2 / steps
        assert np.abs(out["auc"].cpu().numpy() - auc).max() <= TOL, tag
        if modality == "both":
            assert np.array_equal(out["removed_appearance"].cpu().numpy(), z[f"removed_{tag}"]) and np.array_equal(out["removed_layout"].cpu().numpy(), z[f"removed_layout_{tag}"])
            assert np.array_equal(out["n_candidates_layout"].cpu().numpy(), z[f"n_candidates_layout_{tag}"]) and out["n_candidates_appearance"].tolist() == [4] * B
        else:
            assert np.array_equal(out["removed"].cpu().numpy(), z[f"removed_{tag}"]) and out["n_candidates"].tolist() == [4] * B and tuple(out["removed"].shape) == (S, B)
    # token scores (B, A): the CLS column is dropped
    cells = scores_of(name, "appearance")
    tok = torch.cat([torch.full((B, 1), 9.0, device=DEV), cells], dim=1)
    assert torch.equal(model.forward_perturbed(batch, tok, steps=steps)[names[-1]], model.forward_perturbed(batch, cells, steps=steps)[names[-1]])


@pytest.mark.parametrize("name", ["resnet3d", "transformer", "cacnf"])
def test_one_pass_equals_the_plain_forward_bit_for_bit(name, pkg):
    m, model, batch = meta(), model_of(pkg, name), batch_of(pkg, name)
    S, B, steps = m["steps"] + 1, m["clips"], m["steps"]
    cells = scores_of(name, "appearance")
    for order in FR.ORDERS:
        pb = pkg.collate.perturb_cells(batch, cells, steps=steps, order=order)
        with torch.no_grad():
            plain = model(pb)
        whole = model.forward_perturbed(batch, cells, steps=steps, order=order, steps_per_pass=S)
        for k in model.logit_names:
            assert torch.equal(whole[k].view(S * B, -1), plain[k]), (order, k)
        assert torch.equal(whole["removed"], pb["removed"])
        for per in (1, 3):
            part = model.forward_perturbed(batch, cells, steps=steps, order=order, steps_per_pass=per)
            for k in model.logit_names:
                assert (part[k] - whole[k]).abs().max().item() <= TOL, (order, per, k)
            assert torch.equal(part["removed"], whole["removed"]) and torch.equal(part["target"], whole["target"])
    # a given target, a non-zero fill
    target = torch.arange(B, device=DEV) % 5
    given = model.forward_perturbed(batch, cells, steps=steps, order=order, target=target)
    assert torch.equal(given["target"], target) and torch.equal(given[model.logit_names[-1]], whole[model.logit_names[-1]])
    grey = model.forward_perturbed(batch, cells, steps=steps, fill=1.0)
    with torch.no_grad():
        assert torch.equal(grey[model.logit_names[-1]].view(S * B, -1), model(pkg.collate.perturb_cells(batch, cells, steps=steps, fill=1.0))[model.logit_names[-1]])
    if name == "cacnf":
        # the heads: the curves are read from the one asked for; the layout side and both through the same call
        for head in model.logit_names:
            out = model.forward_perturbed(batch, cells, steps=steps, head=head)
            p, h, t = R.curve(out[head].cpu().numpy())
            assert np.array_equal(out["target"].cpu().numpy(), t) and np.abs(out["prob"].cpu().numpy() - p).max() <= 1e-6
        both = scores_of(name, "both")
        lay = model.forward_perturbed(batch, both["layout"], steps=steps, modality="layout")
        with torch.no_grad():
            plain = model(pkg.collate.perturb_batch(batch, both["layout"], steps=steps))
        assert all(torch.equal(lay[k].view(S * B, -1), plain[k]) for k in model.logit_names)
        two = model.forward_perturbed(batch, both, steps=steps, modality="both")
        pb = pkg.collate.perturb_batch(batch, both["layout"], steps=steps)
        pb["video_frames"] = pkg.collate.perturb_cells(batch, cells, steps=steps)["video_frames"]
        with torch.no_grad():
            plain = model(pb)
        assert all(torch.equal(two[k].view(S * B, -1), plain[k]) for k in model.logit_names)
        # precomputed features: the feature column is the cell
        with torch.no_grad():
            feats = model.backbone.appearance_branch.resnet.forward_features(batch)
        fb = {k: v for k, v in batch.items() if k != "video_frames"} | {"appearance_features": feats}
        out = model.forward_perturbed(fb, cells, steps=steps)
        with torch.no_grad():
            plain = model(pkg.collate.perturb_cells(fb, cells, steps=steps))
        assert all(torch.equal(out[k].view(S * B, -1), plain[k]) for k in model.logit_names)
        assert (out["ensemble"][0] - whole["ensemble"][0]).abs().max().item() <= TOL and not torch.equal(out["ensemble"][1], out["ensemble"][0])


def test_one_captured_graph_of_forward_perturbed_replays_to_the_same_bits(pkg):
    """Capture fails on any stream synchronisation or read-back: the call makes none.  Default queue settings."""
    m, model = meta(), model_of(pkg, "transformer")
    static = batch_of(pkg, "transformer")
    scores = scores_of("transformer", "appearance").clone()
    run = lambda: model.forward_perturbed(static, scores, steps=m["steps"], steps_per_pass=2)  # noqa: E731
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
    scores.copy_(torch.flip(scores, dims=(1,)) + torch.arange(4, device=DEV))  # other scores through the same graph
    g.replay()
    torch.cuda.synchronize()
    again = run()
    assert all(torch.equal(out[k], again[k]) for k in eager) and not torch.equal(out["resnet3d"], eager["resnet3d"])


@pytest.mark.parametrize("modality", ["appearance", "layout", "both"])
@pytest.mark.parametrize("method", ["relevance", "saliency", "attention", "random"])
def test_runner_end_to_end_reproduces_forward_perturbed_called_by_hand(method, modality, pkg):
    model, batch = model_of(pkg, "cacnf"), batch_of(pkg, "cacnf")
    B = batch["categories"].shape[0]
    batches = [dict(batch, labels=torch.arange(B, device=DEV) % 5), dict({k: v[:1] for k, v in batch.items()}, labels=torch.tensor([3], device=DEV))]
    steps, seed = 2, 7
    for target, head in (("top1", None), ("label", "caf")):
        res = pkg.infer.run_perturbation_test(model, batches, method=method, steps=steps, target=target, modality=modality, head=head, seed=seed)
        gen = torch.Generator(device=DEV).manual_seed(seed) if method == "random" else None
        sums = {o: [torch.zeros(steps + 1, dtype=torch.float64), torch.zeros(steps + 1, dtype=torch.int64)] for o in FR.ORDERS}
        n = 0
        for b in batches:
            lay = pkg.infer.attribution_scores(model, b, method, gen, head) if modality != "appearance" else None
            app = pkg.infer.appearance_attribution_scores(model, b, method, gen, head) if modality != "layout" else None
            if app is not None:
                assert tuple(app.shape) == (b["categories"].shape[0], 4) and bool(torch.isfinite(app).all())
            scores = {"layout": lay, "appearance": app} if modality == "both" else (lay if app is None else app)
            for order in FR.ORDERS:
                out = model.forward_perturbed(b, scores, steps=steps, order=order, modality=modality, head=head, target=b["labels"] if target == "label" else None)
                sums[order][0] += out["prob"].sum(1, dtype=torch.float64).cpu()
                sums[order][1] += out["hit"].sum(1).cpu()
            n += b["categories"].shape[0]
        for order in FR.ORDERS:
            r, (prob, hits) = res[order], sums[order]
            assert r["num_clips"] == n == B + 1
            assert r["prob"] == (prob / n).tolist() and r["accuracy"] == (hits.double() / n).tolist(), (target, order)


def test_runner_on_the_video_models(pkg):
    tr, r3 = model_of(pkg, "transformer"), model_of(pkg, "resnet3d")
    batch = batch_of(pkg, "transformer")
    B = batch["video_frames"].shape[0]
    for model, methods in ((tr, ("relevance", "saliency", "attention", "random")), (r3, ("saliency", "random"))):
        for method in methods:
            res = pkg.infer.run_perturbation_test(model, [batch], method=method, steps=2, modality="appearance", seed=3)
            gen = torch.Generator(device=DEV).manual_seed(3) if method == "random" else None
            scores = pkg.infer.appearance_attribution_scores(model, batch, method, gen)
            assert tuple(scores.shape) == (B, 4) and bool(torch.isfinite(scores).all()) and bool((scores >= 0).all())
            for order in FR.ORDERS:
                out = model.forward_perturbed(batch, scores, steps=2, order=order)
                assert res[order]["prob"] == (out["prob"].sum(1, dtype=torch.float64).cpu() / B).tolist() and res[order]["num_clips"] == B
    # the attention method of TransformerResnet is a row of probabilities: the CLS row without its own column
    att = pkg.infer.appearance_attribution_scores(tr, batch, "attention")
    assert bool((att.sum(1) < 1).all()) and bool((att.sum(1) > 0).all())
    # saliency is the pooled gradient
    grad = tr.forward_saliency(batch)["video_frames_grad"]
    assert torch.equal(pkg.infer.appearance_attribution_scores(tr, batch, "saliency"), pkg.ops.cell_pool_abs(grad, (16, 32, 32)))
    assert ((pkg.ops.cell_pool_abs(grad, (16, 32, 32)).double().cpu() - FR.cell_pool_abs(grad.cpu(), (16, 32, 32))).abs() <= 1e-5 * FR.cell_pool_abs(grad.cpu(), (16, 32, 32))).all()
    E = pkg.StltHipError
    for method in ("relevance", "attention"):
        with pytest.raises(E, match="no attention and no relevance"):
            pkg.infer.run_perturbation_test(r3, [batch], method=method, steps=2, modality="appearance")
    with pytest.raises(E, match="appearance side only"):
        pkg.infer.run_perturbation_test(tr, [batch], method="random", steps=2, modality="both")


def test_refusals(pkg):
    E = pkg.StltHipError
    m = meta()
    cacnf, tr, r3 = model_of(pkg, "cacnf"), model_of(pkg, "transformer"), model_of(pkg, "resnet3d")
    batch = batch_of(pkg, "cacnf")
    cells, lay = scores_of("cacnf", "appearance"), scores_of("cacnf", "both")["layout"]
    cpu = {k: v.cpu() for k, v in batch.items()}
    for model in (cacnf, tr, r3):
        b = batch if model is cacnf else {"video_frames": batch["video_frames"]}
        with pytest.raises(E, match="CPU tensors"):
            model.forward_perturbed(cpu if model is cacnf else {"video_frames": cpu["video_frames"]}, cells.cpu())
        with pytest.raises(E, match="CPU tensors"):
            model.forward_perturbed(b, cells.cpu())
        with pytest.raises(E, match="cell scores"):
            model.forward_perturbed(b, cells[:, :3].contiguous())
        with pytest.raises(E, match="cell scores"):
            model.forward_perturbed(b, lay)
        with pytest.raises(E, match="steps must be >= 1"):
            model.forward_perturbed(b, cells, steps=0)
        with pytest.raises(E, match="steps_per_pass"):
            model.forward_perturbed(b, cells, steps_per_pass=0)
        with pytest.raises(E, match="order"):
            model.forward_perturbed(b, cells, order="up")
        with pytest.raises(E, match="modality"):
            model.forward_perturbed(b, cells, modality="sound")
        with pytest.raises(E, match="target"):
            model.forward_perturbed(b, cells, target=torch.zeros(2, device=DEV))
    for model in (tr, r3):
        with pytest.raises(E, match="appearance side only"):
            model.forward_perturbed({"video_frames": batch["video_frames"]}, cells, modality="layout")
        with pytest.raises(E, match="video_frames"):
            model.forward_perturbed({"appearance_features": torch.zeros(2, 2048, 2, 1, 2, device=DEV)}, cells)
        with pytest.raises(TypeError):
            model.forward_perturbed({"video_frames": batch["video_frames"]}, cells, unit="object")
    with pytest.raises(E, match="unit"):
        cacnf.forward_perturbed(batch, lay, modality="layout", unit="pixel")
    with pytest.raises(E, match="unit 'object' takes"):
        cacnf.forward_perturbed(batch, cells, modality="layout")
    with pytest.raises(E, match="unit 'frame' takes"):
        cacnf.forward_perturbed(batch, lay, modality="layout", unit="frame")
    with pytest.raises(E, match='"both" takes'):
        cacnf.forward_perturbed(batch, cells, modality="both")
    with pytest.raises(E, match="head"):
        cacnf.forward_perturbed(batch, cells, head="lcf")
    with pytest.raises(E, match="activation"):
        cacnf.forward_perturbed(batch, cells, activation="tanh")
    # more cells than a clip is ranked with
    big = {k: v[:1] for k, v in batch.items() if k != "video_frames"} | {"appearance_features": torch.zeros(1, 1, 1, 129, 128, device=DEV)}
    with pytest.raises(E, match="16384"):
        cacnf.forward_perturbed(big, torch.zeros(1, 129 * 128, device=DEV))
    with pytest.raises(E, match="16384"):
        pkg.ops.perturb_rank_cells(torch.zeros(1, 16385, device=DEV))
    with pytest.raises(E, match="steps"):
        pkg.ops.perturb_apply_cells(batch["video_frames"], (16, 32, 32), torch.zeros(2, 4, dtype=torch.int32, device=DEV), torch.zeros(2, dtype=torch.int32, device=DEV), 3, 2, 4)
    with pytest.raises(E, match="rank is"):
        pkg.ops.perturb_apply_cells(batch["video_frames"], (16, 32, 32), torch.zeros(2, 5, dtype=torch.int32, device=DEV), torch.zeros(2, dtype=torch.int32, device=DEV), 3, 0, 3)
    with pytest.raises(E, match="cell"):
        pkg.ops.cell_pool_abs(batch["video_frames"], (16, 0, 32))
    # live dropout
    for model in (cacnf, tr):
        model.train(True)
        try:
            with pytest.raises(E, match="dropout"):
                model.forward_perturbed(batch if model is cacnf else {"video_frames": batch["video_frames"]}, cells)
        finally:
            model.train(False)
    # a fusion model without the trunk handed video_frames; LCF and CAF share the call
    kw = pkg.synth.model_kwargs(m["config"])
    for cls in (pkg.CrossAttentionFusion, pkg.LateConcatenationFusion):
        bare = cls(pkg.MultimodalModelConfig(**dict(kw, appearance_num_frames=m["appearance_num_frames"], num_appearance_layers=1, num_fusion_layers=1))).to(DEV).train(False)
        with pytest.raises(E, match="appearance_trunk=True"):
            bare.forward_perturbed(batch, cells)
        fb = {k: v for k, v in batch.items() if k != "video_frames"} | {"appearance_features": torch.randn(2, 2048, 2, 1, 2, device=DEV)}
        out = bare.forward_perturbed(fb, cells, steps=2)
        with torch.no_grad():
            plain = bare(pkg.collate.perturb_cells(fb, cells, steps=2))
        name = bare.logit_names[-1]
        assert torch.equal(out[name].view(6, -1), plain[name]) and tuple(out["prob"].shape) == (3, 2)
