"""The appearance side of the perturbation test without a GPU: the restatement's own invariants, collate.perturb_cells' torch form against
the restatement (bit for bit), the runner on one rank and on two over gloo with a stand-in forward, the fixtures and their recorded caps,
and the C-ABI's declarations."""
import importlib
import json
import os
import socket
import sys

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

import fusion_perturbation_restated as FR
import perturbation_restated as R
from conftest import GOLDEN, PKG_NAME, ROOT
from perturbation_cases import same_bits

# (x shape, cell): ragged last cells on every axis; aligned; the feature-space form
CASES = [((2, 3, 20, 40, 70), (16, 32, 32)), ((3, 3, 16, 64, 64), (16, 32, 32)), ((2, 8, 2, 3, 3), (1, 1, 1))]


def _x(shape, seed=0):
    x = torch.randn(shape, generator=torch.Generator().manual_seed(seed))
    x.view(-1)[::7] = 0.0  # values equal to the default fill: the mask, not the value, says what was deleted
    return x


def _n_cells(shape, cell):
    g = FR.grid(shape[2:], cell)
    return g[0] * g[1] * g[2]


@pytest.mark.parametrize("shape,cell", CASES)
@pytest.mark.parametrize("steps", [1, 3, 10])
def test_restatement_invariants(shape, cell, steps):
    x = _x(shape)
    B, C = shape[0], _n_cells(shape, cell)
    rank, n = FR.rank_cells(FR.special_scores(B, C, 3), True)
    assert n.tolist() == [C] * B and all(sorted(rank[b].tolist()) == list(range(C)) for b in range(B))
    fill = 7.5
    out, removed = FR.apply_cells(x, cell, rank, n, steps, 0, steps, fill)
    out = out.view(steps + 1, *shape)
    mask, counts = FR.cell_masks(rank, n, steps, 0, steps, shape[2:], cell)
    assert same_bits(out[0], x), "step 0 is the input bit for bit"
    assert (out[steps] == fill).all(), "the last step has every cell at fill"
    assert removed.tolist() == [[(s * C) // steps] * B for s in range(steps + 1)] and torch.equal(removed, counts)
    for s in range(steps + 1):
        if s:
            assert bool((mask[s] | ~mask[s - 1]).all()), "the cells deleted at step s contain those of step s-1"
        # removed equals the cell count of the mask: a cell is deleted whole or not at all
        for b in range(B):
            cells = [bool(mask[(s, b) + FR.cell_box(c, shape[2:], cell)].all()) for c in range(C)]
            part = [bool(mask[(s, b) + FR.cell_box(c, shape[2:], cell)].any()) for c in range(C)]
            assert cells == part and sum(cells) == int(removed[s, b])
        assert same_bits(torch.where(mask[s][:, None].expand(shape), x, out[s]), x) and (out[s][mask[s][:, None].expand(shape)] == fill).all()
    # the cells partition the volume
    cover = torch.zeros(shape[2:], dtype=torch.int64)
    for c in range(C):
        cover[FR.cell_box(c, shape[2:], cell)] += 1
    assert (cover == 1).all()
    pooled = FR.cell_pool_abs(x, cell)
    assert tuple(pooled.shape) == (B, C) and torch.allclose(pooled.sum(1), x.double().abs().sum(dim=(1, 2, 3, 4)), rtol=1e-12)


@pytest.mark.parametrize("order", FR.ORDERS)
def test_rank_torch_form_against_the_restatement_on_special_values(order, pkg):
    s = FR.special_scores(5, 37, 11)
    rank, n = pkg.collate.perturb_rank_cells(s, order)
    want, want_n = FR.rank_cells(s, order == "descending")
    assert rank.dtype == torch.int32 and torch.equal(rank, want) and torch.equal(n, want_n)
    assert rank[0].tolist() == list(range(37)), "ties go to the lower index in both orders"
    for b in range(1, 5):
        nan = torch.isnan(s[b])
        if nan.any() and (~nan).any():
            assert rank[b][nan].min() > rank[b][~nan].max(), "NaN is removed last in both orders"
        z = s[b] == 0
        assert (rank[b][z].sort().values.diff() == 1).all(), "-0 and +0 tie"
    # the layout side's rule, as restated there: the same integers
    kpm = torch.zeros(5, 2, 38, dtype=torch.bool)
    lay = torch.cat([torch.zeros(5, 1), s], dim=1)[:, None].repeat(1, 2, 1)
    want_lay, _ = R.rank(lay.numpy(), kpm.numpy(), np.full(5, 2), "object", order == "descending")
    assert np.array_equal(want_lay[:, 0, 1:], rank.numpy())


@pytest.mark.parametrize("shape,cell", [((2, 3, 20, 40, 70), (16, 32, 32)), ((2, 8, 2, 3, 3), (1, 1, 1))])
def test_perturb_cells_on_cpu_tensors_equals_the_restatement_bit_for_bit(shape, cell, pkg):
    key = "video_frames" if cell != (1, 1, 1) else "appearance_features"
    B, C = shape[0], _n_cells(shape, cell)
    x = _x(shape, 1)
    x.view(-1)[5] = float("nan")
    batch = {key: x, "labels": torch.arange(B), "video_id": [f"v{b}" for b in range(B)], "categories": torch.arange(B * 6).view(B, 2, 3), "num_real_tokens": 7}
    for order in FR.ORDERS:
        for steps, rng, fill in ((3, None, 0.0), (10, (2, 6), -0.0), (C + 3, (C, C + 3), 1.25), (1, None, 0.0)):
            scores = FR.special_scores(B, C, steps)
            got = pkg.collate.perturb_cells(batch, scores, steps=steps, order=order, step_range=rng, fill=fill)
            want = FR.perturb_cells(batch, scores, steps=steps, order=order, step_range=rng, fill=fill)
            n = steps + 1 if rng is None else rng[1] - rng[0] + 1
            assert same_bits(got[key], want[key]) and tuple(got[key].shape) == (n * B,) + shape[1:], (order, steps)
            assert torch.equal(got["removed"], want["removed"]) and got["removed"].dtype == torch.int32 and torch.equal(got["n_candidates"], want["n_candidates"])
            assert torch.equal(got["labels"], torch.arange(B).repeat(n)) and got["video_id"] == [f"v{b}" for b in range(B)] * n
            assert torch.equal(got["categories"], batch["categories"].repeat(n, 1, 1)) and got["num_real_tokens"] == 7 * n
        # token scores (B, C+1): the CLS column is dropped
        tok = torch.cat([torch.full((B, 1), 99.0), scores], dim=1)
        assert same_bits(pkg.collate.perturb_cells(batch, tok, steps=1, order=order)[key], pkg.collate.perturb_cells(batch, scores, steps=1, order=order)[key])
    # a batch with both tensors: the video is what is perturbed
    if key == "video_frames":
        both = pkg.collate.perturb_cells(dict(batch, appearance_features=torch.zeros(B, 4, 1, 1, 1)), scores, steps=2)
        assert same_bits(both["video_frames"], pkg.collate.perturb_cells(batch, scores, steps=2)["video_frames"]) and tuple(both["appearance_features"].shape) == (3 * B, 4, 1, 1, 1)


def test_the_grid_is_the_trunks_plan(pkg):
    """collate.appearance_cells takes the token grid from modelling.resnet3d's plan: for every extent the stride blocks and the plan agree,
    and a cell index built from them is the flatten(2) order."""
    from_plan = importlib.import_module(PKG_NAME + ".modelling.resnet3d")._trunk_out
    for n in list(range(1, 70)) + [112, 224]:
        assert from_plan(n) == -(-n // 16) and from_plan(n, 2) == -(-n // 32), n
    key, cell, grid = pkg.collate.appearance_cells({"video_frames": torch.zeros(1, 3, 32, 112, 112)})
    assert (key, cell, grid) == ("video_frames", (16, 32, 32), (2, 4, 4))
    idx = pkg.collate.cell_index((32, 112, 112), cell)
    assert int(idx[16, 32, 64]) == (1 * 4 + 1) * 4 + 2 and int(idx.max()) == 31
    for c in range(32):
        assert (idx[FR.cell_box(c, (32, 112, 112), cell)] == c).all()


def test_bad_arguments_are_refused_with_a_message(pkg):
    E = pkg.StltHipError
    x = torch.zeros(2, 3, 16, 32, 64)
    batch = {"video_frames": x}
    sc = torch.zeros(2, 2)
    with pytest.raises(E, match="steps must be >= 1"):
        pkg.collate.perturb_cells(batch, sc, steps=0)
    with pytest.raises(E, match="order"):
        pkg.collate.perturb_cells(batch, sc, order="up")
    with pytest.raises(E, match="step_range"):
        pkg.collate.perturb_cells(batch, sc, steps=3, step_range=(2, 4))
    with pytest.raises(E, match="cell scores"):
        pkg.collate.perturb_cells(batch, torch.zeros(2, 4))
    with pytest.raises(E, match="video_frames"):
        pkg.collate.perturb_cells({"labels": torch.zeros(2)}, sc)
    with pytest.raises(E, match="16384"):
        pkg.collate.perturb_cells({"appearance_features": torch.zeros(1, 1, 1, 129, 128)}, torch.zeros(1, 129 * 128))
    with pytest.raises(E, match="GPU tensor"):
        pkg.ops.perturb_rank_cells(sc)
    with pytest.raises(E, match="GPU tensor"):
        pkg.ops.perturb_apply_cells(x, (16, 32, 32), torch.zeros(2, 2, dtype=torch.int32), torch.zeros(2, dtype=torch.int32), 3, 0, 3)
    with pytest.raises(E, match="GPU tensor"):
        pkg.ops.cell_pool_abs(x, (16, 32, 32))
    with pytest.raises(E, match="modality"):
        pkg.infer.run_perturbation_test(None, [batch], method=lambda m, b: sc, forward=lambda b: torch.zeros(2, 3), modality="sound")


# ---- the runner with a stand-in model ----------------------------------------------------------------------------------------------------
K = 5


def _standin(batch):
    """a model in four lines: logits from the video's cell means and the layout's object count, so that deleting either moves them"""
    v = batch["video_frames"]
    feats = torch.stack([v[:, i % 3, :, :, (i * 13) % v.shape[4]:].mean(dim=(1, 2, 3)) * (1 + i) for i in range(K)], dim=1)
    if "src_key_padding_mask_boxes" in batch:
        real = (~batch["src_key_padding_mask_boxes"][:, :, 1:]).float()
        feats = feats + torch.stack([(real * batch["boxes"][:, :, 1:, i % 4]).sum((1, 2)) * 0.1 * (1 + i) for i in range(K)], dim=1)
    return feats - feats.mean(dim=1, keepdim=True)


def _runner_batches(synth, n_clips, layout=False):
    out = []
    for i, n in enumerate(n_clips):
        b = synth.make_batch(n, 7, 4, seed=50 + i) if layout else {}
        b["video_frames"] = synth.make_video(n, T=20, H=40, W=70, seed=60 + i)
        b["labels"] = torch.randint(0, K, (n,), generator=torch.Generator().manual_seed(i))
        out.append(b)
    return out


def _cell_energy(model, batch):
    return FR.cell_pool_abs(batch["video_frames"], FR.VIDEO_CELL).float()


def _box_area(batch):
    bx = batch["boxes"]
    return (bx[..., 2] - bx[..., 0]) * (bx[..., 3] - bx[..., 1])


def _both(model, batch):
    return {"layout": _box_area(batch), "appearance": _cell_energy(model, batch)}


def _area(curve):
    return float((curve[1:] + curve[:-1]).sum() / 2 / (len(curve) - 1))


def test_runner_with_a_standin_forward_on_one_rank(pkg, synth):
    steps = 4
    for modality in ("appearance", "both"):
        batches = _runner_batches(synth, (5, 3), layout=modality == "both")
        method = _cell_energy if modality == "appearance" else _both
        for target in ("top1", "label"):
            res = pkg.infer.run_perturbation_test(None, batches, method=method, steps=steps, target=target, forward=_standin, modality=modality, fill=0.5)
            assert res["fractions"] == [0.0, 0.25, 0.5, 0.75, 1.0]
            for order in FR.ORDERS:
                prob, hits = np.zeros(steps + 1), np.zeros(steps + 1)
                for b in batches:
                    pert = FR.perturb_cells({"video_frames": b["video_frames"]}, _cell_energy(None, b), steps=steps, order=order, fill=0.5)
                    if modality == "both":
                        nb = {k: b[k].numpy() for k in ("categories", "boxes", "src_key_padding_mask_boxes", "frame_types", "src_key_padding_mask_frames", "lengths")}
                        rank, n = R.rank(_box_area(b).numpy(), nb["src_key_padding_mask_boxes"], nb["lengths"], "object", order == "descending")
                        pert.update({k: torch.from_numpy(v) for k, v in R.apply(nb, rank, n, steps, 0, steps, 3).items() if k != "removed"})
                    logits = _standin(pert).numpy().reshape(steps + 1, -1, K)
                    p, h, _ = R.curve(logits, b["labels"].numpy() if target == "label" else None)
                    prob += p.sum(1)
                    hits += h.sum(1)
                r = res[order]
                assert r["num_clips"] == 8
                assert np.abs(np.array(r["prob"]) - prob / 8).max() <= 1e-6 and np.array_equal(np.array(r["accuracy"]) * 8, hits), (modality, target, order)
                assert abs(r["auc_prob"] - _area(prob / 8)) <= 1e-6 and abs(r["auc_accuracy"] - _area(hits / 8)) <= 1e-12
    batches = _runner_batches(synth, (5, 3))
    rnd = pkg.infer.run_perturbation_test(None, batches, method="random", steps=3, forward=_standin, seed=5, modality="appearance")
    again = pkg.infer.run_perturbation_test(None, batches, method="random", steps=3, forward=_standin, seed=5, modality="appearance")
    assert rnd == again and rnd["descending"]["prob"][0] == rnd["ascending"]["prob"][0]
    # the default is the layout side, as before this modality existed
    lay = _runner_batches(synth, (4,), layout=True)
    assert pkg.infer.run_perturbation_test(None, lay, method=lambda m, b: _box_area(b), steps=2, forward=_standin) == \
        pkg.infer.run_perturbation_test(None, lay, method=lambda m, b: _box_area(b), steps=2, forward=_standin, modality="layout")


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _worker(rank, world, port, n_clips, q):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    os.environ.update(RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    torch.set_num_threads(2)
    pkg = importlib.import_module(PKG_NAME)
    r, w = pkg.dist.init_distributed("gloo")
    assert (r, w) == (rank, world)
    res = pkg.infer.run_perturbation_test(None, _runner_batches(pkg.synth, n_clips), method=_cell_energy, steps=4, rank=rank, world=world, forward=_standin,
                                          modality="appearance")
    if rank == 0:
        q.put(res)
    torch.distributed.barrier()
    torch.distributed.destroy_process_group()


def test_runner_on_two_ranks_over_gloo_matches_one_rank(pkg, synth):
    n_clips = (5, 1, 4)  # uneven shards and a batch smaller than the world
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, 2, port, n_clips, q)) for r in range(2)]
    for p in procs:
        p.start()
    got = q.get(timeout=240)
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    one = pkg.infer.run_perturbation_test(None, _runner_batches(synth, n_clips), method=_cell_energy, steps=4, forward=_standin, modality="appearance")
    assert got["fractions"] == one["fractions"]
    for order in FR.ORDERS:
        assert got[order]["num_clips"] == one[order]["num_clips"] == 10
        assert got[order]["accuracy"] == one[order]["accuracy"]
        assert np.abs(np.array(got[order]["prob"]) - np.array(one[order]["prob"])).max() <= 1e-12


# ---- the fixtures ------------------------------------------------------------------------------------------------------------------------
def test_fixtures_load_and_the_recorded_caps_hold(pkg):
    meta = json.load(open(os.path.join(GOLDEN, "fusion_perturbation_schema.json")))
    S, B, C = meta["steps"] + 1, meta["clips"], meta["appearance_num_frames"]
    v = meta["video"]
    assert tuple(meta["grid"]) == FR.grid((v["T"], v["H"], v["W"]), FR.VIDEO_CELL) and int(np.prod(meta["grid"])) == C
    assert pkg.collate.appearance_cells({"video_frames": torch.zeros(1, 3, v["T"], v["H"], v["W"])})[2] == tuple(meta["grid"])
    assert meta["cap"] == 0.05 and meta["margin"] == 1e-3 and meta["clip_index"] == list(range(B))
    assert set(meta["models"]) == {"resnet3d", "transformer", "cacnf"}
    for name, m in meta["models"].items():
        z = np.load(os.path.join(GOLDEN, f"fusion_perturbation_{name}.npz"))
        assert os.path.getsize(os.path.join(GOLDEN, f"fusion_perturbation_{name}.npz")) < 1 << 20
        assert z["scores_cells"].shape == (B, C)
        low = total = 0
        for tag in m["cases"]:
            for k in m["logit_names"]:
                lg = z[f"logits_{k}_{tag}"]
                assert lg.shape[:2] == (S, B) and lg.dtype == np.float32 and np.isfinite(lg).all()
            assert np.array_equal(z[f"removed_{tag}"], FR.removal_counts([C] * B, meta["steps"], 0, meta["steps"]).numpy())
            mg = z[f"margin_{tag}"]
            assert mg.shape == (S, B)
            low += int((mg < meta["margin"]).sum())
            total += mg.size
            # step 0 is the untouched batch: the same logits in every case of a model
            first = m["cases"][0]
            assert np.array_equal(z[f"logits_{m['logit_names'][-1]}_{tag}"][0], z[f"logits_{m['logit_names'][-1]}_{first}"][0])
        assert (low, total) == (m["low_margin"], m["entries"]) and low <= meta["cap"] * total and abs(m["low_margin_share"] - low / total) < 1e-12
    assert any(t.startswith("both_") for t in meta["models"]["cacnf"]["cases"]) and meta["models"]["cacnf"]["logit_names"][-1] == "ensemble"


def test_abi_declares_the_three_cell_launchers(pkg):
    header = open(os.path.join(ROOT, "include", "stlt_hip.h")).read()
    for name in ("stlt_perturb_rank_cells", "stlt_perturb_apply_cells", "stlt_cell_pool_abs"):
        assert name in pkg._lib.SIGNATURES and f" {name}(" in header
    src = open(os.path.join(ROOT, PKG_NAME, "csrc", "perturb.hip")).read()
    assert src.count("for (int size = 2; size <= n_pow2; size <<= 1)") == 1, "one LDS sort serves both rank launchers"
    for cls in ("Resnet3D", "TransformerResnet", "CrossAttentionFusion", "CrossAttentionCentralNetFusion", "LateConcatenationFusion"):
        assert callable(getattr(getattr(pkg, cls), "forward_perturbed"))
