"""The explanation kernels off the unit scale, held to torch's own fp32 error row by row: attention maps and gradient-weighted maps (packed
and cross, every route), probe attention, the rollouts and read-outs, Grad-CAM's three kernels and the embeddings' input-gradient product.

Every case comes from tests/explain_scale_cases.py (its docstring states the rows and where the cases leave the plain recipe; the metric
is the one of tests/scale_cases.py: rows of very different magnitudes in one launch, each judged on its own scale, the bar
4 * max(E_t, u)); tests/test_explain_scale_cpu.py holds the cases to the conditions that make that bar mean something and shows that the
lazy forms miss it.  Kernels are reached through pkg.ops.*; the route a launch took is read from the launch recorder's notes, not
inferred from the shape.  Every case prints e_k / u, E_t / u and their ratio per group (profiles/explain_scale.md keeps the table of
one run).  No kernel needed an analytic term.
"""
import pytest
import torch

import explain_scale_cases as E
import scale_cases as SC

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _hold(tag, results, case, terms=None):
    """results: {output name: what the kernel gave}; every output of the case must be among them."""
    assert set(results) == set(case["outs"]), (sorted(results), sorted(case["outs"]))
    fails = []
    for name, got in results.items():
        if name in case.get("index", {}):
            got = E.indexed(got, case["index"][name])
        fails += SC.judge(f"{tag} {name}", got, case["outs"][name], term=(terms or {}).get(name))[1]
    assert not fails, "\n".join(fails)


def _noted(pkg, fn):
    """fn() with the launch recorder on -> (its result, the notes of its launches)"""
    pkg.ops.prof_enable(True)
    try:
        pkg.ops.prof_launches()
        got = fn()
        torch.cuda.synchronize()
        notes = [r["note"] for r in pkg.ops.prof_launches()]
    finally:
        pkg.ops.prof_enable(False)
    return got, notes


def _dev(case, *keys):
    return [None if case[k] is None else case[k].to(DEV) for k in keys]


# ---- attention maps ----------------------------------------------------------------------------------------------------------------
PACKED_ROUTES = {(7, 64): "mfma-diag", (17, 64): "mfma-full", (64, 64): "mfma-full", (7, 20): "generic", (65, 64): "generic"}  # as the launchers' notes name them


@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("L,dh", E.PACKED_SHAPES)
def test_packed_attention_maps_of_every_score_scale(pkg, L, dh, causal):
    """ops.attn_probs (per head and averaged) and ops.attn_grad_probs on one packed buffer: heads of score std 1e-3 .. 300 in one sequence,
    rising scores, a masked sequence (exact zeros), a single visible key, and the selected tail, whose largest element is p g at 20 to 40
    score units below a peak with a negative gradient (an exp taken as exp2 of the rounded x * log2(e) is 8 - 28 u off there against bars of
    4.5 - 10 u: profiles/explain_scale.md).  L = 7: several
    sequences per 16-row block; 17 and 64: two and four key blocks; dh = 20 and L = 65: the vector kernels."""
    case = E.attention_map_case(L, L, dh, causal)
    q, k, v, dctx, kpm = _dev(case, "q", "k", "v", "dctx", "kpm")
    qkv = torch.cat([q, k, v], -1)
    got, notes = _noted(pkg, lambda: {"probabilities per head": pkg.ops.attn_probs(qkv, kpm, causal, E.H, per_head=True),
                                      "probabilities": pkg.ops.attn_probs(qkv, kpm, causal, E.H),
                                      "abar": pkg.ops.attn_grad_probs(qkv, dctx, kpm, causal, E.H)})
    route = PACKED_ROUTES[(L, dh)]
    assert len(notes) == 3 and all(n.startswith(f"attn_probs {route} ") for n in notes[:2]) and notes[2].startswith(f"attn_grad_probs {route} "), notes
    _hold(f"packed maps L={L} dh={dh} causal={int(causal)}", got, case)


# (Lq, Lk, dh, repeats) -> the routes of attn_probs_cross and of attn_grad_probs_cross, as the launchers' notes name them.  The gradient
# launcher sends fewer than 128 units over three or four key blocks to its vector kernel: (7, 33) runs on both sides of that rule.
CROSS_ROUTES = {(7, 33, 64, 1): ("mfma-full", "generic"), (7, 33, 64, 16): ("mfma-full", "mfma-full"), (33, 17, 64, 1): ("mfma-full", "mfma-full"),
                (17, 17, 64, 1): ("mfma-full", "mfma-full"), (16, 65, 64, 1): ("generic", "generic"), (7, 33, 20, 1): ("generic", "generic")}


@pytest.mark.parametrize("Lq,Lk,dh,reps", E.CROSS_SHAPES)
def test_cross_attention_maps_of_every_score_scale(pkg, Lq, Lk, dh, reps):
    """ops.attn_probs_cross and ops.attn_grad_probs_cross on the same sequences, keys and values as the two halves of one packed buffer.
    (7, 33) with 8 sequences is below the gradient launcher's 128 units and takes its vector kernel, with 128 sequences it takes the MFMA
    kernel; (17, 17) runs causal."""
    causal = Lq == Lk
    case = E.attention_map_case(Lq, Lk, dh, causal, reps)
    q, k, v, dctx, kpm = _dev(case, "q", "k", "v", "dctx", "kpm")
    kv = torch.cat([k, v], -1)
    d = E.H * dh
    got, notes = _noted(pkg, lambda: {"probabilities per head": pkg.ops.attn_probs_cross(q, kv[..., :d], kpm, causal, E.H, per_head=True),
                                      "probabilities": pkg.ops.attn_probs_cross(q, kv[..., :d], kpm, causal, E.H),
                                      "abar": pkg.ops.attn_grad_probs_cross(q, kv[..., :d], kv[..., d:], dctx, kpm, causal, E.H)})
    probs_route, grad_route = CROSS_ROUTES[(Lq, Lk, dh, reps)]
    assert len(notes) == 3 and all(n.startswith(f"attn_probs_cross {probs_route} ") for n in notes[:2]) and notes[2].startswith(f"attn_grad_probs_cross {grad_route} "), notes
    _hold(f"cross maps Lq={Lq} Lk={Lk} dh={dh} S={q.shape[0]}", got, case)


@pytest.mark.parametrize("dh,T", E.PROBE_SHAPES)
def test_probe_attention_of_every_score_scale(pkg, dh, T):
    """ops.attn_prefix_probe: heads of score std 1e-3 .. 300 in one clip, rising scores, a clip with every frame masked."""
    case = E.probe_case(dh, T)
    qkv_f, qkv_p, kpm = _dev(case, "qkv_f", "qkv_p", "kpm")
    got, notes = _noted(pkg, lambda: pkg.ops.attn_prefix_probe(qkv_f, qkv_p, kpm, E.H))
    assert len(notes) == 1 and notes[0].startswith(f"attn_prefix_probe S=6 T={T} H={E.H} dh={dh} "), notes
    _hold(f"probe attention dh={dh} T={T}", {"ctx": case["head_rows"](got.cpu())}, case)


# ---- rollouts and read-outs ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L", E.ROLLOUT_L)
def test_rollout_items_of_every_map_scale(pkg, L):
    """ops.attn_rollout over 4 layers and ops.relevance_combine: items whose maps have the scales 1e-6 .. 30 and one whose layers differ.
    At scale 1e-2 the diagonal of R is 1 + 1e-2; a chain that starts from the old R[i,j] rounds each of the L products at that magnitude
    (45 u against a bar of 10 u: profiles/explain_scale.md).  64 / 65: all columns in one workgroup / blocks of 16."""
    case = E.rollout_case(L)
    abar, rt, rs, lengths = _dev(case, "abar", "rt", "rs", "lengths")
    got, notes = _noted(pkg, lambda: {"R": pkg.ops.attn_rollout(abar), "relevance": pkg.ops.relevance_combine(rt, rs, lengths)})
    assert len(notes) == 2 and notes[0].startswith(f"attn_rollout layers={E.N_LAYERS} S=5 L={L} ") and notes[0].endswith(f"cols/wg={L if L <= 64 else 16}"), notes
    assert notes[1].startswith("relevance_combine "), notes
    _hold(f"rollout L={L}", got, case)


@pytest.mark.parametrize("given", [True, False])
@pytest.mark.parametrize("T,A", E.JOINT_SHAPES)
def test_joint_rollout_items_of_every_map_scale(pkg, T, A, given):
    """ops.attn_rollout_joint over 2 fusion layers (six steps) from given branch rollouts or from the identity, and
    ops.relevance_combine_joint with the head weights 0.7 / 0.3."""
    case = E.joint_case(T, A, given)
    r_l, r_a, l2a, a2l, fl, fa, R32, rs, lengths = _dev(case, "r_layout", "r_appearance", "l2a", "a2l", "f_layout", "f_appearance", "R32", "rs", "lengths")

    def run():
        R = pkg.ops.attn_rollout_joint(r_l, r_a, l2a, a2l, fl, fa)
        rel, frame, app = pkg.ops.relevance_combine_joint(R32, rs, lengths, E.W_LAYOUT, E.W_APPEARANCE)
        return {"R": R, "relevance": rel, "frame relevance": frame, "appearance relevance": app}

    got, notes = _noted(pkg, run)
    assert len(notes) == 2 and notes[0].startswith(f"attn_rollout_joint layers={E.N_FUSION} S=5 T={T} A={A} ") and notes[1].startswith("relevance_combine_joint "), notes
    _hold(f"joint rollout T={T} A={A} given={int(given)}", got, case)


# ---- Grad-CAM --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", ["ndhwc", "ncdhw"])
@pytest.mark.parametrize("C", E.CAM_C)
def test_cam_clips_of_every_gradient_scale(pkg, C, layout):
    """ops.cam_weights and ops.cam_map (Grad-CAM and HiResCAM, with and without the ReLU) at P = 1, 31, 32, 33 and 100 positions (one
    chunk with a tail, exactly one, two, four with a tail): clips of gradient scale 1e-8, 1, 1e6, channel groups of mean / spread 0, 10,
    100.  C = 4: the 16-byte channel loads; 6: one float per load; 260: a second trip of the map's channel loop."""
    for P in E.CAM_P:
        case = E.cam_case(P, C, layout)
        g, a, w = _dev(case, "g", "a", "w")
        got, notes = _noted(pkg, lambda: {"alpha": pkg.ops.cam_weights(g, layout),
                                          "grad-cam": pkg.ops.cam_map(a, w, layout, relu=False), "grad-cam relu": pkg.ops.cam_map(a, w, layout, relu=True),
                                          "hirescam": pkg.ops.cam_map(a, g, layout, relu=False), "hirescam relu": pkg.ops.cam_map(a, g, layout, relu=True)})
        assert len(notes) == 5 and notes[0].startswith(f"cam_weights B=3 P={P} C={C} layout="), notes
        assert [n.split("per_element=")[1] for n in notes[1:]] == ["0 relu=0", "0 relu=1", "1 relu=0", "1 relu=1"], notes
        _hold(f"cam P={P} C={C} {layout}", got, case)


@pytest.mark.parametrize("layout", ["ndhwc", "ncdhw"])
def test_cam_weights_over_a_thousand_positions(pkg, layout):
    """ops.cam_weights (and the maps) at P = 1000, C = 6: 32 chunks whose partials the finishing launch adds in turn, 16 elements per lane
    in the NCDHW kernel; a single accumulator would miss these bars (tests/test_explain_scale_cpu.py)."""
    P, C = E.CAM_LONG
    case = E.cam_case(P, C, layout)
    g, a, w = _dev(case, "g", "a", "w")
    got = {"alpha": pkg.ops.cam_weights(g, layout), "grad-cam": pkg.ops.cam_map(a, w, layout, relu=False), "grad-cam relu": pkg.ops.cam_map(a, w, layout, relu=True),
           "hirescam": pkg.ops.cam_map(a, g, layout, relu=False), "hirescam relu": pkg.ops.cam_map(a, g, layout, relu=True)}
    _hold(f"cam P={P} C={C} {layout}", got, case)


@pytest.mark.parametrize("which", range(len(E.UPSAMPLE)))
def test_cam_upsample_clips_of_every_scale(pkg, which):
    """ops.cam_upsample against F.interpolate(mode="trilinear", align_corners=False): clips of scale 1e-30, 1, 1e30 in one launch."""
    case = E.upsample_case(which)
    _hold(f"cam_upsample {E.UPSAMPLE[which]}", {"map": pkg.ops.cam_upsample(case["cam"].to(DEV), case["size"])}, case)


# ---- embed_bwd_inputs ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_scores", [True, False])
@pytest.mark.parametrize("d", E.EMBED_D)
def test_embed_input_gradients_block_by_block(pkg, d, with_scores):
    """ops.embed_bwd_inputs: 37 tokens of scale 1e-6 .. 1e3 against four box columns and a score column of their own scales, every output
    element judged alone under the product rule (torch's product and the in-order chain).  d = 64: four tokens per wave; 768: a wave per token."""
    case = E.embed_bwd_case(d, with_scores)
    d_pre, box_w, score_w = _dev(case, "d_pre", "box_w", "score_w")
    (d_boxes, d_scores), notes = _noted(pkg, lambda: pkg.ops.embed_bwd_inputs(d_pre, box_w, score_w))
    assert len(notes) == 1 and notes[0].startswith(f"embed_bwd_inputs rows={E.EMBED_TOKENS} d={d} ") and notes[0].endswith(f"tokens/wave={4 if d <= 64 else 1}"), notes
    got = {"d_boxes": d_boxes}
    if with_scores:
        got["d_scores"] = d_scores
    _hold(f"embed_bwd_inputs d={d} scores={int(with_scores)}", got, case)


# ---- the smaller entry points ------------------------------------------------------------------------------------------------------------
def test_cell_pools_of_every_clip_scale(pkg):
    """ops.cell_pool_abs and ops.cell_pool_sum: clips of scale 1e-8, 1, 1e6 in one launch, cells with ragged last rows and columns."""
    case = E.cell_pool_case()
    g = case["g"].to(DEV)
    _hold("cell pools", {"sum": pkg.ops.cell_pool_sum(g, case["cell"]), "abs": pkg.ops.cell_pool_abs(g, case["cell"])}, case)


def test_perturb_curve_clips_of_every_logit_scale(pkg):
    """ops.perturb_curve (softmax): logit scales 1e-3 .. 1000, the target from on top to 70 below the prediction; given and found targets."""
    case = E.perturb_curve_case()
    logits, target = case["logits"].to(DEV), case["target"].to(DEV)
    prob, hit, tgt = pkg.ops.perturb_curve(logits, target)
    found, _, tgt0 = pkg.ops.perturb_curve(logits)
    assert torch.equal(tgt.cpu(), case["target"]) and torch.equal(tgt0.cpu(), case["target"]) and torch.equal(found, prob)
    assert bool(hit[0].all()) and not bool(hit[2:].any())
    _hold("perturb_curve", {"probability": prob.T}, case)


def test_ig_delta_attribution_sums_of_every_clip_scale(pkg):
    """ops.ig_delta with a zero seed: delta is the sum of each clip's attributions, clips of scale 1e-8 .. 1e6, sums that cancel at most six bits."""
    case = E.ig_delta_case()
    B, K = len(E.IG_CLIPS), case["K"]
    zeros = torch.zeros(B, K, device=DEV)
    logits = torch.randn(B, K, generator=torch.Generator().manual_seed(0)).to(DEV)
    got = pkg.ops.ig_delta([a.to(DEV) for a in case["attrs"]], zeros, logits, zeros)
    _hold("ig_delta stage 1", {"delta": got}, case)
