"""Layout gradients on the GPU: the op-level kernel against an fp64 product inside the guard arena, boxes.grad / scores.grad of Stlt and of a
fusion model against the fp64 oracle's autograd on both schedules, the frozen model, Stlt.forward_saliency, and the input-only sweep's work.

Gradient accuracy is the project's measure (tests/test_train_gpu.py): max|got - ref| / max|ref| <= 2e-4 per tensor, the reference being the
fp64 oracle with batch["boxes"] / batch["scores"] as fp64 leaves (its own fp32 run stays within 3.1e-6 of it on these cases).  The op-level
kernel is held to 1e-5 of max|ref|, the cap of the product tests.  The oracle's gradient is exactly 0.0 under both padding masks
(tests/test_layout_gradients_cpu.py checks that), hence the exact-zero assertions.  Every test prints its worst figure."""
import functools
import sys

import pytest
import torch
import torch.nn.functional as F

import guard_arena as GA
from oracle import caf_oracle as CO
from oracle import stlt_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda"
CAP = 2e-4
OP_CAP = 1e-5
EINVAL = -1


def _report(what, value):
    print(f"\n[layout gradients] {what}: {value}", file=sys.stderr)


def _rel(got, ref):
    return (got.detach().cpu().double() - ref).abs().max().item() / max(ref.abs().max().item(), 1e-30)


# ---------------------------------------------------------------------------------------------------------------- 1. op-level kernel
@pytest.fixture(scope="module")
def arena():
    return GA.Arena(12 << 20)


def _op_specs(n, d, with_scores, seed):
    specs = {"d_pre": (GA.rand(n, d, seed=seed), "in"), "box_w": (GA.rand(d, 4, seed=seed + 1), "in"), "d_boxes": (GA.Out((n, 4)), "out")}
    if with_scores:
        specs["score_w"] = (GA.rand(d, 1, seed=seed + 2), "in")
        specs["d_scores"] = (GA.Out((n,)), "out")
    return specs


def _op_call(lib, n, d, with_scores):
    return lambda o: lib.stlt_embed_bwd_inputs(o.d_pre.ptr, o.box_w.ptr, o.score_w.ptr if with_scores else None, n, d, o.d_boxes.ptr,
                                               o.d_scores.ptr if with_scores else None, GA.stream())


@pytest.mark.parametrize("with_scores", [False, True])
@pytest.mark.parametrize("d", [4, 100, 256, 768])
def test_embed_bwd_inputs_matches_fp64_product_inside_guard_bands(pkg, arena, d, with_scores):
    lib = pkg._lib.load()
    worst = 0.0
    for n in (1, 7, 64, 65, 1000):
        specs = _op_specs(n, d, with_scores, seed=1000 * d + n)
        outs = ("d_boxes", "d_scores") if with_scores else ("d_boxes",)
        got = GA.three_ways(lib, arena, specs, _op_call(lib, n, d, with_scores), outs)  # plain == arena == second call, bit for bit; bands, inputs intact
        ref_b = specs["d_pre"][0].double() @ specs["box_w"][0].double()
        worst = max(worst, _rel(got["d_boxes"], ref_b))
        if with_scores:
            worst = max(worst, _rel(got["d_scores"], specs["d_pre"][0].double() @ specs["score_w"][0].double()[:, 0]))
        assert worst <= OP_CAP, (n, d, worst)
    _report(f"embed_bwd_inputs d={d} scores={with_scores} worst err / max|ref|", f"{worst:.2e}")


def test_embed_bwd_inputs_refusals_leave_the_outputs_untouched(pkg, arena):
    lib = pkg._lib.load()
    n, d = 65, 100
    specs = _op_specs(n, d, True, seed=3)
    outs = ("d_boxes", "d_scores")
    for operand in ("d_pre", "box_w", "score_w", "d_boxes", "d_scores"):
        for mis in (4, 8):
            assert GA.misaligned(lib, arena, specs, _op_call(lib, n, d, True), outs, operand=operand, mis=mis, refused_as=operand) is None
    arena.reset()
    A = {k: arena.place(s[0], s[1], name=k) for k, s in specs.items()}
    p = {k: v.ptr for k, v in A.items()}
    s = GA.stream()
    refused = {
        "d = 6": lib.stlt_embed_bwd_inputs(p["d_pre"], p["box_w"], p["score_w"], n, 6, p["d_boxes"], p["d_scores"], s),
        "d_scores without score_w": lib.stlt_embed_bwd_inputs(p["d_pre"], p["box_w"], None, n, d, p["d_boxes"], p["d_scores"], s),
        "score_w without d_scores": lib.stlt_embed_bwd_inputs(p["d_pre"], p["box_w"], p["score_w"], n, d, p["d_boxes"], None, s),
        "n_tokens < 0": lib.stlt_embed_bwd_inputs(p["d_pre"], p["box_w"], p["score_w"], -1, d, p["d_boxes"], p["d_scores"], s),
        "null d_pre": lib.stlt_embed_bwd_inputs(None, p["box_w"], p["score_w"], n, d, p["d_boxes"], p["d_scores"], s),
        "null d_boxes": lib.stlt_embed_bwd_inputs(p["d_pre"], p["box_w"], None, n, d, None, None, s),
    }
    assert all(rc == EINVAL for rc in refused.values()), refused
    arena.check(launched=False)


# ---------------------------------------------------------------------------------------------------------------- shared set-up
def _model(pkg, name, skip_padding=False, train=True):
    m = pkg.Stlt(pkg.StltModelConfig(**pkg.synth.model_kwargs(name)))
    sd = pkg.synth.make_state_dict({k: tuple(v.shape) for k, v in m.state_dict().items()}, seed=31, gain=1.5)
    m.load_state_dict(sd)
    m.train(train)  # hidden_dropout_prob = 0 in model_kwargs
    m.to(DEV)
    m.backbone.skip_padding = skip_padding
    return m, sd


def _dev(batch, grad=True):
    dev = {k: v.to(DEV) for k, v in batch.items()}
    if grad:
        for k in ("boxes", "scores"):
            if k in dev:
                dev[k].requires_grad_(True)
    return dev


@functools.lru_cache(maxsize=None)
def _case(pkg, name, B, with_scores, T=None, N=None, multi_hot=False):
    """The seeded case of the existing gradient tests and its fp64 oracle, computed once: cross-entropy gradients wrt every parameter, the
    boxes and the scores; `multi_hot`: also the gradients of sum(seed * logits) for a seeded multi-hot seed (a saliency objective)."""
    c = dict(pkg.synth.CONFIGS[name])
    if T is not None:
        c["T"], c["N"] = T, N
    shapes = {k: tuple(v.shape) for k, v in pkg.Stlt(pkg.StltModelConfig(**pkg.synth.model_kwargs(name))).state_dict().items()}
    sd = pkg.synth.make_state_dict(shapes, seed=31, gain=1.5)
    batch = pkg.synth.make_batch(B, c["T"], c["N"], dataset=c["dataset"], seed=77, with_scores=with_scores)
    labels = torch.randint(0, c["num_classes"], (B,), generator=torch.Generator().manual_seed(5))
    leaves = {k: (v.detach().double().requires_grad_(True) if v.is_floating_point() else v) for k, v in sd.items()}
    b = {k: (v.double() if v.is_floating_point() else v) for k, v in batch.items()}
    inputs = [b[k].requires_grad_(True) for k in ("boxes", "scores") if k in b]
    logits = O.stlt_forward(leaves, b, c["num_attention_heads"], dtype=torch.float64)["stlt"]
    keys = [k for k, v in leaves.items() if v.is_floating_point()]
    seed = None
    sal = None
    if multi_hot:
        seed = (torch.rand(B, c["num_classes"], generator=torch.Generator().manual_seed(9)) < 0.03).float()
        seed[:, 1] = 1.0  # never an empty row
        sal = torch.autograd.grad(logits, inputs, grad_outputs=seed.double(), retain_graph=True)
    grads = torch.autograd.grad(F.cross_entropy(logits, labels), inputs + [leaves[k] for k in keys], allow_unused=True)
    ref = {"boxes": grads[0], "scores": grads[1] if with_scores else None, "params": dict(zip(keys, grads[len(inputs):])), "logits": logits.detach(),
           "seed": seed, "sal_boxes": None if sal is None else sal[0], "sal_scores": None if sal is None or not with_scores else sal[1]}
    return c, sd, batch, labels, ref


def _assert_zero_under_masks(batch, g_boxes, g_scores):
    pad_obj = batch["src_key_padding_mask_boxes"].bool()
    pad_frm = batch["src_key_padding_mask_frames"].bool()
    for g in (g_boxes.detach().cpu().abs().sum(-1),) + (() if g_scores is None else (g_scores.detach().cpu().abs(),)):
        assert g[pad_obj].numel() == 0 or g[pad_obj].max().item() == 0.0, "a padded object slot has a gradient"
        assert g[pad_frm].numel() == 0 or g[pad_frm].max().item() == 0.0, "a padded frame has a gradient"
        assert g[~pad_obj].max().item() > 0.0


# ---------------------------------------------------------------------------------------------------------------- 2. autograd, Stlt
CASES = [("cfg1", 3, False, None, None), ("cfg1", 5, True, None, None), ("cfg1", 3, False, 17, 2), ("cfg1", 2, False, 29, 16), ("cfg2", 2, False, None, None)]


def _check_autograd(pkg, name, B, with_scores, T, N, skip_padding):
    c, sd, batch, labels, ref = _case(pkg, name, B, with_scores, T, N, multi_hot=name == "cfg4")
    m, _ = _model(pkg, name, skip_padding)
    dev = _dev(batch)
    out = m(dev)["stlt"]
    assert out.requires_grad
    assert (out.detach().cpu().double() - ref["logits"]).abs().max().item() <= 1e-4
    F.cross_entropy(out, labels.to(DEV)).backward()
    assert dev["boxes"].grad is not None and tuple(dev["boxes"].grad.shape) == tuple(batch["boxes"].shape)
    worst = {"boxes": _rel(dev["boxes"].grad, ref["boxes"])}
    if with_scores:
        assert dev["scores"].grad is not None and tuple(dev["scores"].grad.shape) == tuple(batch["scores"].shape)
        worst["scores"] = _rel(dev["scores"].grad, ref["scores"])
    worst["params"] = 0.0
    for k, p in m.named_parameters():
        g_ref = ref["params"][k]
        if "encoder_layer." in k or ("score_embeddings" in k and not with_scores):
            assert p.grad is None or p.grad.abs().max().item() == 0.0, k
            continue
        assert p.grad is not None, k
        err = _rel(p.grad, g_ref)
        assert err <= CAP, f"{k}: relative grad error {err:.2e}"
        worst["params"] = max(worst["params"], err)
    _report(f"{name} B={B} T={c['T']} N={c['N']} skip_padding={skip_padding} worst err / max|ref|", {k: f"{v:.2e}" for k, v in worst.items()})
    assert worst["boxes"] <= CAP and worst.get("scores", 0.0) <= CAP, worst
    _assert_zero_under_masks(batch, dev["boxes"].grad, dev["scores"].grad if with_scores else None)


@pytest.mark.parametrize("skip_padding", [False, True])
@pytest.mark.parametrize("name,B,with_scores,T,N", CASES)
def test_layout_gradients_match_oracle_autograd(pkg, name, B, with_scores, T, N, skip_padding):
    _check_autograd(pkg, name, B, with_scores, T, N, skip_padding)


def test_layout_gradients_match_oracle_autograd_cfg4_with_scores(pkg):
    _check_autograd(pkg, "cfg4", 2, True, None, None, False)


# ---------------------------------------------------------------------------------------------------------------- 3. frozen model
def test_frozen_model_still_differentiates_in_the_layout(pkg):
    c, sd, batch, labels, ref = _case(pkg, "cfg1", 5, True)
    for skip in (False, True):
        m, _ = _model(pkg, "cfg1", skip)
        for q in m.parameters():
            q.requires_grad_(False)
        dev = _dev(batch)
        out = m(dev)["stlt"]
        assert out.requires_grad
        F.cross_entropy(out, labels.to(DEV)).backward()
        errs = (_rel(dev["boxes"].grad, ref["boxes"]), _rel(dev["scores"].grad, ref["scores"]))
        _report(f"frozen cfg1 B=5 skip_padding={skip} boxes / scores err / max|ref|", errs)
        assert max(errs) <= CAP
        assert all(q.grad is None for q in m.parameters())
        _assert_zero_under_masks(batch, dev["boxes"].grad, dev["scores"].grad)


def test_no_input_grad_leaves_the_training_step_bit_identical(pkg):
    c, sd, batch, labels, ref = _case(pkg, "cfg1", 5, True)

    def step(m, dev):
        m.zero_grad(set_to_none=True)
        out = m(dev)["stlt"]
        F.cross_entropy(out, labels.to(DEV)).backward()
        return out.detach().clone(), {k: p.grad.clone() for k, p in m.named_parameters() if p.grad is not None}

    m, _ = _model(pkg, "cfg1")
    before = step(m, _dev(batch, grad=False))            # the inputs were never marked
    marked = _dev(batch)
    with_inputs = step(m, marked)                        # boxes and scores require grad
    assert marked["boxes"].grad is not None
    after = step(m, _dev(batch, grad=False))
    for logits, grads in (with_inputs, after):
        assert torch.equal(logits, before[0])
        assert set(grads) == set(before[1])
        for k in grads:
            assert torch.equal(grads[k], before[1][k]), k


# ---------------------------------------------------------------------------------------------------------------- 4. forward_saliency
def _autograd_saliency(m, batch, seed):
    """gradient of sum(seed * logits) wrt the layout through the autograd path of the same model"""
    dev = _dev(batch)
    out = m(dev)["stlt"]
    (out * seed).sum().backward()
    return out.detach(), dev["boxes"].grad, dev["scores"].grad if "scores" in dev else None


@pytest.mark.parametrize("name,B", [("cfg1", 4), ("refdef", 2)])
def test_forward_saliency_equals_the_autograd_gradient_of_the_selected_logit(pkg, name, B):
    c = pkg.synth.CONFIGS[name]
    batch = pkg.synth.make_batch(B, c["T"], c["N"], dataset=c["dataset"], seed=77, with_scores=name == "cfg1")
    if name == "cfg1":
        batch = pkg.synth.make_batch(B + 1, c["T"], c["N"], dataset=c["dataset"], seed=77, with_scores=True)  # the seeded batch whose clip 4 is short ...
        batch = {k: v[1:].contiguous() for k, v in batch.items()}                                          # ... as clips 1..4: B = 4 with padded frames
    m, _ = _model(pkg, name, train=False)
    dev = _dev(batch, grad=False)
    with torch.no_grad():
        fwd = m(dev)["stlt"]
    res = {}
    for skip in (False, True):
        m.backbone.skip_padding = skip
        r = m.forward_saliency(dev)
        again = m.forward_saliency(dev)
        assert all(torch.equal(r[k], again[k]) for k in r), "two calls differ"
        assert set(r) == {"stlt", "target", "boxes_grad"} | ({"scores_grad"} if "scores" in batch else set())
        assert (r["stlt"] - fwd).abs().max().item() <= 1e-4
        assert r["target"].dtype == torch.int64 and r["target"].is_cuda and torch.equal(r["target"], r["stlt"].argmax(dim=1))
        assert tuple(r["boxes_grad"].shape) == tuple(batch["boxes"].shape)
        onehot = F.one_hot(r["target"], r["stlt"].shape[1]).float()
        by_index, by_seed = m.forward_saliency(dev, target=r["target"]), m.forward_saliency(dev, target=onehot)
        for k in ("boxes_grad", "scores_grad"):
            if k in r:
                assert torch.equal(by_index[k], r[k]) and torch.equal(by_seed[k], r[k]), k
        assert by_seed["target"] is onehot
        assert all(q.grad is None for q in m.parameters()), "forward_saliency created a parameter gradient"
        _, g_boxes, g_scores = _autograd_saliency(m, batch, onehot)  # the autograd path of the same model: this one does fill the parameters' .grad
        m.zero_grad(set_to_none=True)
        errs = [_rel(r["boxes_grad"], g_boxes.cpu().double())] + ([_rel(r["scores_grad"], g_scores.cpu().double())] if g_scores is not None else [])
        _report(f"forward_saliency {name} B={B} skip_padding={skip} err / max|autograd|", errs)
        assert max(errs) <= CAP
        _assert_zero_under_masks(batch, r["boxes_grad"], r.get("scores_grad"))
        res[skip] = r
    assert _rel(res[True]["boxes_grad"], res[False]["boxes_grad"].cpu().double()) <= CAP
    # with the batch's row counts the ragged schedule reads nothing back: same result
    m.backbone.skip_padding = True
    counted = m.forward_saliency(dict(dev, **pkg.collate.real_counts(batch)))
    assert torch.equal(counted["boxes_grad"], res[True]["boxes_grad"])
    # an out-of-range class: that clip's seed row is NaN (test_saliency_seed_rows), so its gradients are
    bad = res[True]["target"].clone()
    bad[0] = r["stlt"].shape[1]
    assert torch.isnan(m.forward_saliency(dev, target=bad)["boxes_grad"][0]).any()


def test_saliency_seed_rows(pkg):
    """stlt_saliency_seed: e_k with k = target[b], or the row's argmax with the lowest index on ties; an out-of-range target gives a NaN row."""
    lib = pkg._lib.load()
    B, K = 5, 300  # more classes than the block has threads
    logits = GA.rand(B, K, seed=4)
    logits[0, 17] = logits[0, 290] = 5.0    # a tie across two trips of a thread's loop and two threads
    logits[1, 299] = 7.0
    logits[2, 0] = 9.0
    logits[3, 40] = logits[3, 41] = 6.0     # a tie between neighbouring threads
    logits[4, 3] = float("nan")             # a NaN never wins
    logits[4, 200] = 2.0
    x = logits.to(DEV)
    seed = torch.full((B, K), 3.0, device=DEV)
    assert lib.stlt_saliency_seed(x.data_ptr(), None, B, K, seed.data_ptr(), GA.stream()) == 0, GA.last_error(lib)
    want = torch.zeros(B, K)
    for b, k in enumerate((17, 299, 0, 40, 200)):
        want[b, k] = 1.0
    assert torch.equal(seed.cpu(), want)
    target = torch.tensor([299, 0, -1, K, 41], device=DEV)
    assert lib.stlt_saliency_seed(None, target.data_ptr(), B, K, seed.data_ptr(), GA.stream()) == 0, GA.last_error(lib)
    got = seed.cpu()
    assert torch.isnan(got[2]).all() and torch.isnan(got[3]).all()
    for b, k in ((0, 299), (1, 0), (4, 41)):
        assert got[b, k] == 1.0 and got[b].sum() == 1.0 and (got[b] != 0).sum() == 1


def test_forward_saliency_multi_hot_seed_matches_oracle_cfg4(pkg):
    c, sd, batch, labels, ref = _case(pkg, "cfg4", 2, True, None, None, multi_hot=True)
    m, _ = _model(pkg, "cfg4", train=False)
    r = m.forward_saliency(_dev(batch, grad=False), target=ref["seed"].to(DEV))
    errs = (_rel(r["boxes_grad"], ref["sal_boxes"]), _rel(r["scores_grad"], ref["sal_scores"]))
    _report("forward_saliency cfg4 B=2 multi-hot boxes / scores err / max|ref|", errs)
    assert max(errs) <= CAP
    _assert_zero_under_masks(batch, r["boxes_grad"], r["scores_grad"])


def test_forward_saliency_refuses_live_dropout_and_retires_a_pending_tape(pkg):
    name = "cfg1"
    c = pkg.synth.CONFIGS[name]
    batch = pkg.synth.make_batch(2, c["T"], c["N"], seed=1)
    dev = _dev(batch, grad=False)
    m = pkg.Stlt(pkg.StltModelConfig(**dict(pkg.synth.model_kwargs(name), hidden_dropout_prob=0.1))).to(DEV)
    m.train(True)
    with pytest.raises(pkg._lib.StltHipError, match="training mode with dropout"):
        m.forward_saliency(dev)
    m.train(False)
    pending = m(dev)["stlt"]  # grad-enabled forward: its graph owns the backbone's tape
    m.forward_saliency(dev)   # ... until this pass re-records it
    with pytest.raises(pkg._lib.StltHipError, match="tape was overwritten"):
        pending.sum().backward()
    m(dev)["stlt"].sum().backward()  # the next forward trains as ever


# ---------------------------------------------------------------------------------------------------------------- 5. less work
def test_input_only_sweep_enqueues_fewer_matrix_flops_than_a_training_step(pkg):
    c, sd, batch, labels, ref = _case(pkg, "cfg1", 5, True)
    m, _ = _model(pkg, "cfg1")
    dev = _dev(batch, grad=False)
    F.cross_entropy(m(dev)["stlt"], labels.to(DEV)).backward()  # buffers, contexts
    m.forward_saliency(dev)
    torch.cuda.synchronize()
    pkg.ops.prof_enable(True)
    try:
        pkg.ops.prof_take_gemm_flops()
        m.zero_grad(set_to_none=True)
        F.cross_entropy(m(dev)["stlt"], labels.to(DEV)).backward()
        torch.cuda.synchronize()
        full = pkg.ops.prof_take_gemm_flops()
        m.forward_saliency(dev)
        torch.cuda.synchronize()
        sal = pkg.ops.prof_take_gemm_flops()
        launches = pkg.ops.prof_launches()
    finally:
        pkg.ops.prof_enable(False)
        pkg.ops.prof_collect()
    _report("GEMM flops forward_saliency / (training forward + full backward), cfg1 B=5", f"{sal:.4g} / {full:.4g} = {sal / full:.3f}")
    assert 0 < sal < full
    assert any("embed_bwd_inputs" in l["note"] for l in launches), "the saliency pass did not run the input-gradient kernel"


# ---------------------------------------------------------------------------------------------------------------- 6. fusion model
def test_fusion_model_routes_boxes_grad_through_its_layout_branch(pkg):
    small = dict(num_spatial_layers=2, num_temporal_layers=1, num_appearance_layers=1, num_fusion_layers=1)
    B, T, N, grid = 3, 16, 4, (1, 4, 4)
    kw = dict(pkg.synth.model_kwargs("cfg1"), **small, appearance_num_frames=16, hidden_dropout_prob=0.0)
    m = pkg.CrossAttentionFusion(pkg.MultimodalModelConfig(**kw))
    sd = pkg.synth.make_state_dict({k: tuple(v.shape) for k, v in m.state_dict().items()}, seed=17)
    m.load_state_dict(sd)
    m.to(DEV).train(False)  # eval mode: no dropout anywhere; grad on -> the training composition
    batch = pkg.synth.make_batch(B, T, N, seed=1619, min_len=2)
    batch["appearance_features"] = pkg.synth.make_appearance_features(B, seed=1620, grid=grid)
    labels = torch.randint(0, 174, (B,), generator=torch.Generator().manual_seed(1621))
    loss_of = lambda out, y: sum(F.cross_entropy(v, y) for v in out.values()) / len(out)  # noqa: E731
    leaves = {k: (v.detach().double() if v.is_floating_point() else v) for k, v in sd.items()}
    b64 = dict(batch, boxes=batch["boxes"].double().requires_grad_(True))
    loss_of(CO.caf_forward(leaves, b64, kw["num_attention_heads"], dtype=torch.float64), labels).backward()
    ref = b64["boxes"].grad
    assert batch["src_key_padding_mask_frames"].any()
    for frozen_branch in (False, True):
        (bb,) = [mod for mod in m.modules() if isinstance(mod, pkg.StltBackbone)]
        for q in bb.parameters():
            q.requires_grad_(not frozen_branch)
        m.zero_grad(set_to_none=True)
        dev = _dev(batch)
        loss_of(m(dev), labels.to(DEV)).backward()
        assert dev["boxes"].grad is not None
        err = _rel(dev["boxes"].grad, ref)
        _report(f"CrossAttentionFusion boxes.grad err / max|ref| (layout branch frozen={frozen_branch})", f"{err:.2e}")
        assert err <= CAP
        _assert_zero_under_masks(batch, dev["boxes"].grad, None)
