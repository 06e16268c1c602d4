"""Cases, batches, fp64 references, bounds and step helpers shared by tests/test_ragged_dropout_cpu.py, tests/test_ragged_dropout_gpu.py and
its child process tests/ragged_dropout_child.py: skip-padding training with dropout against tests/ragged_restated.py.  TEST INFRASTRUCTURE ONLY."""
import functools
import importlib

import numpy as np
import torch
import torch.nn.functional as F

import ragged_restated as RR
from conftest import PKG_NAME
from oracle import stlt_oracle as O

WEIGHT_SEED, DROP_SEED, NUM_CLASSES = 41, 123456789, 174

# The project's bounds for the padded schedule under the same masks (tests/test_train_gpu.py, test_dropout_forward_and_gradients_match_
# masked_oracle): logits 2e-5 at p <= 0.1, 4e-4 at p = 0.5; gradients 5e-4 of the parameter's largest reference gradient.  p = 0.3 (case D)
# has no bound of the project's: its logit bound is 4 x the fp32 rounding floor of the restatement itself on that case — stlt_forward_ragged in
# float32 against float64, same masks — measured by test_fp32_floor_of_the_measured_cases below: 1.7e-6, recorded here as
# FLOOR_LOGITS and held there to within a factor of two.  4 x: the kernels sum in another order than torch on the CPU, and the padded test
# records a 4 x seed-to-seed spread of the same noise.
GRAD_BOUND = 5e-4
FLOOR_LOGITS = {"D": 1.7e-6}

# d, H, T, N, B, batch recipe, p; then what the schedule makes of the batch (asserted by test_cases_reach_the_schedules_they_claim):
# sp_tail / tp_tail — the tower ends in a tail layer (2 * picked rows <= rows); fpg — whole frames per spatial backward group.
# routes — the kernels of one step as the library's launch recorder lists them (asserted on the GPU by assert_routes): the attention
# backward of the spatial / temporal tower ("mfma", 16-row blocks per group: attn_bwd16_kernel<NB, RAGGED>; "vector": attn_any_bwd_kernel,
# head dim != 64; "long": attn_bwd_long_kernel, L > 64; "fma": the ragged form of attn_bwd_kernel, behind STLT_ATTN_BWD16=0) and the FFN
# hidden site forward / backward ("gemm16+keep" / "gemm16+gelu_bwd": small-tile products with the STLT_ACT_GELU_KEEP / STLT_ACT_GELU_BWD
# epilogue; "gemm+gelu_bwd": gemm.hip's large tiles with the GELU_BWD epilogue; "gelu_fwd" / "gelu_bwd_colsum" / "gelu_bwd": the
# stand-alone kernels of backward.hip after / before a plain product)
_MFMA2 = dict(sp=("mfma", 2), tp=("mfma", 2), ffn_fwd="gemm16+keep", ffn_bwd="gemm16+gelu_bwd")
CASES = {
    "A-p0.1": dict(d=256, H=4, T=16, N=4, B=3, batch="A", p=0.1, sp_tail=True, tp_tail=True, fpg=8, routes=_MFMA2),
    "A-p0.5": dict(d=256, H=4, T=16, N=4, B=3, batch="A", p=0.5, sp_tail=True, tp_tail=True, fpg=8, routes=_MFMA2),
    "B": dict(d=256, H=4, T=16, N=4, B=3, batch="B", p=0.1, sp_tail=False, tp_tail=True, fpg=8, routes=_MFMA2),
    "C": dict(d=256, H=4, T=1, N=3, B=4, batch="C", p=0.1, sp_tail=True, tp_tail=False, fpg=10, routes=_MFMA2),
    "D": dict(d=32, H=4, T=5, N=3, B=4, batch="D", p=0.3, sp_tail=True, tp_tail=True, fpg=10,
              routes=dict(sp=("vector", 0), tp=("vector", 0), ffn_fwd="gelu_fwd", ffn_bwd="gemm+gelu_bwd")),
    "E": dict(d=128, H=2, T=4, N=36, B=2, batch="E", p=0.1, sp_tail=True, tp_tail=True, fpg=1, routes=dict(_MFMA2, sp=("mfma", 3))),
    "F": dict(d=64, H=1, T=70, N=2, B=2, batch="F", p=0.1, sp_tail=False, tp_tail=True, fpg=16, routes=dict(_MFMA2, tp=("long", 0))),
    "G": dict(d=256, H=4, T=16, N=4, B=3, batch="G", p=0.1, sp_tail=True, tp_tail=True, fpg=8, routes=_MFMA2),
    # hidden size 48 (head dim 12): not a multiple of 32, so neither product carries the FFN hidden site — gelu_fwd_kernel forward and
    # gelu_bwd_colsum_kernel backward, in the full layers and (with drop_rows) in both tail layers
    "H": dict(d=48, H=4, T=6, N=4, B=3, batch="H", p=0.1, sp_tail=True, tp_tail=True, fpg=8,
              routes=dict(sp=("vector", 0), tp=("vector", 0), ffn_fwd="gelu_fwd", ffn_bwd="gelu_bwd_colsum")),
}


def logit_bound(name):
    c = CASES[name]
    if name in FLOOR_LOGITS:
        return 4.0 * FLOOR_LOGITS[name]
    return 2e-5 if c["p"] <= 0.1 else 4e-4


def _synth():
    return importlib.import_module(PKG_NAME + ".synth")


def _remask(batch):
    batch["src_key_padding_mask_boxes"] = batch["categories"] == 0
    return batch


def make_case_batch(recipe):
    synth = _synth()
    if recipe == "A":
        return synth.make_batch(3, 16, 4, seed=9)
    if recipe == "B":  # CLS-only frames, as in test_skip_padding_training_edge_layouts_and_alternation: as many tokens as frames
        b = synth.make_batch(3, 16, 4, seed=45)
        b["categories"][:, :, 1:] = 0
        b["boxes"][:, :, 1:] = 0
        return _remask(b)
    if recipe == "C":  # one frame per clip (lengths 1), 1 / 2 / 2 / 2 objects beside the CLS slot: 11 tokens, 4 frames
        b = synth.make_batch(4, 1, 3, seed=5)
        assert b["lengths"].tolist() == [1, 1, 1, 1]
        ids = synth.DATASETS["something"]["obj_ids"]
        rng = np.random.Generator(np.random.PCG64(17))
        for clip, k in enumerate((1, 2, 2, 2)):
            for n in range(1, k + 1):
                b["categories"][clip, 0, n] = int(ids[int(rng.integers(0, len(ids)))])
                lo, hi = np.sort(rng.random((2, 2)), axis=0)
                b["boxes"][clip, 0, n] = torch.tensor([lo[0], lo[1], hi[0], hi[1]], dtype=torch.float32)
        return _remask(b)
    if recipe == "D":
        return synth.make_batch(4, 5, 3, seed=13, min_len=2)  # 28 tokens in 14 frames: the spatial tower just keeps its tail layer
    if recipe == "E":  # dense, then about a third of the object slots masked (holes inside the frames); clip 0's first frame stays full: 36 rows
        b = synth.make_batch(2, 4, 36, seed=3, dense=True)
        hole = torch.rand(2, 4, 36, generator=torch.Generator().manual_seed(4)) < 0.35
        hole[:, :, 0] = False
        hole[0, 0] = False
        b["categories"][hole] = 0
        b["boxes"][hole] = 0
        return _remask(b)
    if recipe == "F":  # clip 0 has all 70 frames: a temporal segment of more than 64 rows
        b = synth.make_batch(2, 70, 2, seed=6)
        assert int(b["lengths"][0]) == 70
        return b
    if recipe == "H":
        return synth.make_batch(3, 6, 4, seed=2, min_len=3)  # 27 tokens in 12 frames: both towers keep their tail layer
    if recipe == "G":  # case A's batch with a hole in a frame (slot 2 masked, slot 3 real) and a hole in a clip (a masked frame with real frames behind it)
        b = synth.make_batch(3, 16, 4, seed=9)
        full = (b["categories"] != 0).all(dim=2).nonzero()
        assert len(full) >= 2, "case A's batch has no frame with every slot real"
        for clip, t in full[:2].tolist():
            b["categories"][clip, t, 2] = 0
            b["boxes"][clip, t, 2] = 0
        assert int(b["lengths"][0]) == 16
        b["frame_types"][0, 5] = 0
        b["src_key_padding_mask_frames"] = b["frame_types"] == 0
        return _remask(b)
    raise KeyError(recipe)


def model_kwargs(name):
    c = CASES[name]
    return dict(_synth().model_kwargs("cfg1"), hidden_size=c["d"], num_attention_heads=c["H"], num_spatial_layers=2, num_temporal_layers=2,
                hidden_dropout_prob=c["p"])


@functools.lru_cache(maxsize=None)
def case_inputs(name):
    """(state dict, batch, labels) of a case — built once, shared, never modified."""
    pkg = importlib.import_module(PKG_NAME)
    c = CASES[name]
    m = pkg.Stlt(pkg.StltModelConfig(**model_kwargs(name)))
    sd = _synth().make_state_dict({k: tuple(v.shape) for k, v in m.state_dict().items()}, seed=WEIGHT_SEED, gain=1.5)
    batch = make_case_batch(c["batch"])
    assert tuple(batch["categories"].shape) == (c["B"], c["T"], c["N"]) and "scores" not in batch
    labels = torch.randint(0, NUM_CLASSES, (c["B"],), generator=torch.Generator().manual_seed(1))
    return sd, batch, labels


def is_dead(key):
    """the parameters no forward uses: the reference's unused `encoder_layer` copy, and score_embeddings (no case's batch carries scores)"""
    return "encoder_layer." in key or "score_embeddings" in key


def _run(name, forward, dtype):
    sd, batch, labels = case_inputs(name)
    leaves = {k: (v.detach().to(dtype).requires_grad_(True) if v.is_floating_point() else v) for k, v in sd.items()}
    logits = forward(leaves, batch)
    F.cross_entropy(logits, labels).backward()
    return logits.detach(), {k: v.grad for k, v in leaves.items() if v.is_floating_point()}


@functools.lru_cache(maxsize=None)
def ragged_reference(name, p=None, dtype=torch.float64):
    """(logits, gradients) of the ragged restatement under RaggedDropout(p, DROP_SEED) — p: the case's own unless given.  Shared, never modified."""
    c = CASES[name]
    p = c["p"] if p is None else p
    ix = RR.ragged_index(case_inputs(name)[1])
    drop = RR.RaggedDropout(p, DROP_SEED, ix, 2) if p > 0 else None
    return _run(name, lambda sd, b: RR.stlt_forward_ragged(sd, b, c["H"], drop, dtype=dtype)["stlt"], dtype)


@functools.lru_cache(maxsize=None)
def padded_reference(name, p=None):
    """(logits, gradients) of the padded oracle under Dropout(p, DROP_SEED): padded-position masks."""
    c = CASES[name]
    p = c["p"] if p is None else p
    drop = O.Dropout(p, DROP_SEED) if p > 0 else None

    def fwd(sd, b):
        b = {k: (v.double() if v.is_floating_point() else v) for k, v in b.items()}
        return O.stlt_forward(sd, b, c["H"], dtype=torch.float64, drop=drop)["stlt"]
    return _run(name, fwd, torch.float64)


def grad_errors(got, ref):
    """{parameter: largest error relative to the parameter's largest reference gradient} over the live parameters; the dead ones must be
    absent or zero on both sides."""
    out = {}
    for k, g_ref in ref.items():
        g = got.get(k)
        if is_dead(k):
            assert g is None or g.abs().max().item() == 0.0, k
            assert g_ref is None or g_ref.abs().max().item() == 0.0, k
            continue
        assert g is not None and g_ref is not None, k
        out[k] = (g.detach().cpu().double() - g_ref.double()).abs().max().item() / max(g_ref.abs().max().item(), 1e-6)
    return out




# ---- one step on the native tape (GPU) ------------------------------------------------------------------------------------------------
DEV = "cuda"


def build_model(pkg, name):
    sd, _, _ = case_inputs(name)
    m = pkg.Stlt(pkg.StltModelConfig(**model_kwargs(name)))
    m.load_state_dict(sd)
    m.train(True).to(DEV)
    m._dropout_seed_override = DROP_SEED
    return m


def train_step(m, name, skip_padding):
    """one cross-entropy step of case `name` on the native tape -> (logits, {parameter: gradient or None})"""
    _, batch, labels = case_inputs(name)
    m.backbone.skip_padding = skip_padding
    m.zero_grad(set_to_none=True)
    out = m({k: v.to(DEV) for k, v in batch.items()})["stlt"]
    F.cross_entropy(out, labels.to(DEV)).backward()
    return out.detach().cpu().double(), {k: (None if p.grad is None else p.grad.detach().cpu()) for k, p in m.named_parameters()}


def check_step(tag, name, got, ref, bound, frozen=()):
    """logits within `bound`, every live parameter's gradient within GRAD_BOUND of its largest reference gradient; figures printed first.
    `frozen`: parameters whose requires_grad the test switched off — they must have no gradient, every other one is still held."""
    (logits, grads), (ref_logits, ref_grads) = got, ref
    err = (logits - ref_logits).abs().max().item()
    assert all(grads[k] is None for k in frozen), frozen
    live = [k for k in grads if not is_dead(k) and k not in frozen]
    assert all(grads[k] is not None for k in live), [k for k in live if grads[k] is None]
    errs = grad_errors({k: g for k, g in grads.items() if k not in frozen}, {k: ref_grads[k] for k in grads if k not in frozen})
    assert sorted(errs) == sorted(live)  # no parameter skipped: the dead ones are named by is_dead, and grad_errors holds them to zero
    worst = max(errs, key=errs.get)
    print(f"{tag}: logits err {err:.2e} (bound {bound:.1e}); {len(errs)} gradients, worst {errs[worst]:.2e} (bound {GRAD_BOUND:.0e}) at {worst}")
    # logits: the project's bound for the padded schedule under the same masks (2e-5 at p <= 0.1, 4e-4 at p = 0.5); case D (p = 0.3):
    # 4 x the fp32 floor of the restatement on that case, 1.7e-6 -> 6.8e-6 (FLOOR_LOGITS above)
    assert err <= bound
    assert errs[worst] <= GRAD_BOUND, (worst, errs[worst])


def observed_routes(pkg, m, name):
    """One more ragged step of `name` under the library's launch recorder (ops.prof_launches: every launch's kernel class and the
    launcher's own note) -> the routes in the vocabulary of CASES[...]["routes"]."""
    c = CASES[name]
    torch.cuda.synchronize()
    pkg.ops.prof_enable(True)
    try:
        pkg.ops.prof_launches()
        train_step(m, name, True)
        torch.cuda.synchronize()
        recs = pkg.ops.prof_launches()
    finally:
        pkg.ops.prof_enable(False)
    notes = [r["note"] for r in recs]

    def attn(causal):  # the tower's attention backward launches (two layers), all on one route
        mine = [n for n in notes if n.startswith("attn_bwd ") and f"causal={causal} ragged" in n]
        assert len(mine) == 2, notes
        kinds = set()
        for n in mine:
            L = int(n.split(" L=")[1].split()[0])
            if "bwd16 items=" in n:  # NB from the workgroup count: 4 / 3 / 2 waves per workgroup at NB = 2 / 3 / 4 (attn_bwd16.hip: waves_for)
                chunks, wg = int(n.split("chunks=")[1].split()[0]), int(n.split("wg=")[1].split()[0])
                nb = [b for b, waves in ((2, 4), (3, 3), (4, 2)) if wg == -(-chunks * c["H"] // waves)]
                assert len(nb) == 1, n
                kinds.add(("mfma", nb[0]))
            elif "fma groups=" in n:
                kinds.add(("fma", 0))
            else:  # launch_attn_bwd: head dim != 64 -> attn_any.hip whatever L; head dim 64 and L > 64 -> the long kernel
                kinds.add(("vector", 0) if c["d"] // c["H"] != 64 else ("long", 0) if L > 64 else ("?", 0))
        assert len(kinds) == 1, mine
        return kinds.pop()

    count = lambda frag: sum(frag in n for n in notes)  # noqa: E731
    fwd = {"gemm16+keep": count("act=4"), "gelu_fwd": count("gelu_fwd n=") - 1}  # (one gelu_fwd / gelu_bwd launch is the head's)
    bwd = {"gemm16+gelu_bwd": sum("act=3" in n and n.startswith("gemm16") for n in notes),
           "gemm+gelu_bwd": sum("act=3" in n and n.startswith("gemm") and not n.startswith("gemm16") for n in notes),
           "gelu_bwd_colsum": count("gelu_bwd+colsum"), "gelu_bwd": count("gelu_bwd n=") - 1}
    one = lambda d: next(iter(k for k, v in d.items() if v == 4)) if sorted(d.values()) == [0] * (len(d) - 1) + [4] else d  # noqa: E731
    return dict(sp=attn(0), tp=attn(1), ffn_fwd=one(fwd), ffn_bwd=one(bwd))


def assert_routes(pkg, m, name, **override):
    want = dict(CASES[name]["routes"], **override)
    got = observed_routes(pkg, m, name)
    print(f"{name}: routes {got}")
    assert got == want, (got, want)
