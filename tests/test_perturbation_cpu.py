"""The perturbation test without a GPU: collate.perturb_batch's torch form against the fixtures the reference made (bit for bit), the
repository's oracle on the perturbed batches against the reference's logits, the integer removal counts, the curves' torch form against the
fp64 restatement, the runner on one rank and on two over gloo with a stand-in forward, and the C-ABI's declarations."""
import importlib
import math
import os
import socket
import sys

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

import perturbation_cases as PC
import perturbation_restated as R
from conftest import PKG_NAME, ROOT
from oracle import stlt_oracle as O

ORACLE_BAR = 2e-5  # tests/test_oracle_golden.py: fp32 oracle against the fp32 reference


def _np(batch):
    return {k: v.numpy() for k, v in batch.items()}


@pytest.mark.parametrize("name", PC.CONFIGS)
def test_perturb_batch_on_cpu_tensors_equals_the_fixtures_bit_for_bit(name, pkg):
    fx = PC.fixture(name)
    z, S, B = fx["z"], fx["steps"] + 1, fx["batch"]["categories"].shape[0]
    for order, unit in PC.COMBOS:
        tag = f"{order}_{unit}"
        rank, n_cand = pkg.collate.perturb_rank(fx["scores"][unit], fx["batch"]["src_key_padding_mask_boxes"], fx["batch"]["lengths"], unit, order)
        assert rank.dtype == torch.int32 and np.array_equal(rank.numpy(), z[f"rank_{tag}"]), tag
        assert np.array_equal(n_cand.numpy(), z[f"n_candidates_{tag}"]), tag
        got = pkg.collate.perturb_batch(dict(fx["batch"], labels=torch.arange(B), video_id=[f"v{b}" for b in range(B)], num_real_tokens=7, num_real_frames=3),
                                        fx["scores"][unit], steps=fx["steps"], order=order, unit=unit, dataset_name=fx["dataset"])
        want = PC.expected_batch(fx, order, unit)
        for k, v in want.items():
            assert PC.same_bits(got[k], v), (tag, k)
        assert np.array_equal(got["removed"].numpy(), z[f"removed_{tag}"]) and got["removed"].dtype == torch.int32, tag
        assert np.array_equal(got["n_candidates"].numpy(), z[f"n_candidates_{tag}"]), tag
        # the other per-clip entries are tiled, the row counts multiplied by the steps written
        assert torch.equal(got["labels"], torch.arange(B).repeat(S)) and got["video_id"] == [f"v{b}" for b in range(B)] * S
        assert got["num_real_tokens"] == 7 * S and got["num_real_frames"] == 3 * S
        # step 0 is the batch itself, the last step has no candidate left, and a step range is a slice of the whole
        for k, v in fx["batch"].items():
            assert PC.same_bits(got[k][:B], v), (tag, k)
        cand = R.candidates(got["src_key_padding_mask_boxes"][-B:].numpy(), fx["batch"]["lengths"].numpy(), "object")
        assert not cand.any(), tag
        part = pkg.collate.perturb_batch(fx["batch"], fx["scores"][unit], steps=fx["steps"], order=order, unit=unit, step_range=(1, 2), dataset_name=fx["dataset"])
        for k in want:
            assert PC.same_bits(part[k], got[k][B:3 * B]), (tag, k)
        assert torch.equal(part["removed"], got["removed"][1:3]) and "num_real_tokens" not in part


@pytest.mark.parametrize("name", PC.CONFIGS)
def test_the_fixtures_hold_the_four_mistakes_apart(name):
    """What a wrong removal rule would change is present in every fixture: the CLS slot and the extract frame are never deleted although
    their scores would put them first, ties exist and go to the lower index, frames turn empty, and some count is floored, not rounded."""
    fx = PC.fixture(name)
    z, batch, steps = fx["z"], fx["batch"], fx["steps"]
    B, T, N = batch["categories"].shape
    S = steps + 1
    ds = importlib.import_module(PKG_NAME + ".synth").DATASETS[fx["dataset"]]
    rounded_differs = False
    for order, unit in PC.COMBOS:
        tag = f"{order}_{unit}"
        cats = z[f"categories_{tag}"].reshape(S, B, T, N)
        assert (cats[:, :, :, 0] == ds["cls"]).all(), tag
        ft = z[f"frame_types_{tag}"].reshape(S, B, T)
        for b in range(B):
            e = int(batch["lengths"][b]) - 1
            assert (ft[:, b, e] == ds["extract"]).all() and (cats[:, b, e] == batch["categories"][b, e].numpy()).all(), tag
        assert ((ft == ds["empty"]) & (batch["frame_types"].numpy()[None] != ds["empty"])).any(), tag
        n = z[f"n_candidates_{tag}"].astype(np.int64)
        rounded = np.array([[int(math.floor(s * int(c) / steps + 0.5)) for c in n] for s in range(S)])
        rounded_differs |= bool((rounded != z[f"removed_{tag}"]).any())
        rank, sc = z[f"rank_{tag}"].reshape(B, -1), fx["scores"][unit].numpy().reshape(B, -1)
        ties = 0
        for b in range(B):
            idx = np.flatnonzero(rank[b] >= 0)
            by_rank = idx[np.argsort(rank[b][idx])]
            same = sc[b][by_rank][1:] == sc[b][by_rank][:-1]
            ties += int(same.sum())
            assert (by_rank[1:][same] > by_rank[:-1][same]).all(), tag
        assert ties > 0, tag
    assert rounded_differs


@pytest.mark.parametrize("name", PC.CONFIGS)
def test_oracle_on_the_perturbed_batches_matches_the_reference(name):
    fx = PC.fixture(name)
    S, B = fx["steps"] + 1, fx["batch"]["categories"].shape[0]
    for order, unit in PC.COMBOS:
        batch = PC.expected_batch(fx, order, unit)
        with torch.no_grad():
            got = O.stlt_forward(fx["sd"], batch, fx["heads"])["stlt"].numpy().reshape(S, B, -1)
        err = np.abs(got - fx["z"][f"logits_{order}_{unit}"]).max()
        assert err <= ORACLE_BAR, (order, unit, err)


@pytest.mark.parametrize("steps", [1, 3, 10, 1000])
def test_removal_counts_are_floored_integers(steps, pkg):
    n_cand = [0, 1, 2, 7, 2304]
    T, N = 65, 37  # 64 * 36 = 2304 candidates at most
    B = len(n_cand)
    kpm = torch.ones(B, T, N, dtype=torch.bool)
    kpm[:, :, 0] = False
    for b, n in enumerate(n_cand):
        kpm[b, :T - 1, 1:] = (torch.arange((T - 1) * (N - 1)) >= n).reshape(T - 1, N - 1)
    batch = {"categories": (~kpm).long(), "boxes": torch.rand(B, T, N, 4, generator=torch.Generator().manual_seed(1)), "src_key_padding_mask_boxes": kpm,
             "frame_types": torch.full((B, T), 2), "src_key_padding_mask_frames": torch.zeros(B, T, dtype=torch.bool), "lengths": torch.full((B,), T)}
    scores = torch.rand(B, T, N, generator=torch.Generator().manual_seed(2))
    rng = (0, steps) if steps < 1000 else (331, 340)
    out = pkg.collate.perturb_batch(batch, scores, steps=steps, step_range=rng)
    assert out["n_candidates"].tolist() == n_cand
    want = [[(s * n) // steps for n in n_cand] for s in range(rng[0], rng[1] + 1)]
    assert out["removed"].tolist() == want
    assert np.array_equal(R.removal_counts(n_cand, steps)[rng[0]:rng[1] + 1], np.array(want))
    # ... and they are what was deleted
    gone = (out["src_key_padding_mask_boxes"] & ~kpm.repeat(len(want), 1, 1)).reshape(len(want), B, -1).sum(-1)
    assert gone.tolist() == want
    if steps < 1000:
        assert out["removed"][0].tolist() == [0] * B and out["removed"][-1].tolist() == n_cand


def special_scores(B, T, N, seed):
    """scores with blocks of ties, both zeros, both infinities and NaN"""
    g = torch.Generator().manual_seed(seed)
    s = torch.round(torch.randn(B, T, N, generator=g) * 2) / 2
    pick = torch.rand(B, T, N, generator=g)
    for lo, v in ((0.0, -0.0), (0.07, 0.0), (0.14, math.inf), (0.2, -math.inf), (0.26, math.nan)):
        s[(pick >= lo) & (pick < lo + 0.06)] = v
    return s


@pytest.mark.parametrize("unit", R.UNITS)
@pytest.mark.parametrize("order", R.ORDERS)
def test_rank_torch_form_against_the_restatement_on_special_values(order, unit, pkg, synth):
    batch = synth.make_batch(6, 9, 6, seed=3, min_len=1)
    batch["lengths"][1], batch["lengths"][2] = 1, 2
    s = special_scores(6, 9, 6, 5)
    s = s if unit == "object" else s[:, :, 0].contiguous()
    rank, n = pkg.collate.perturb_rank(s, batch["src_key_padding_mask_boxes"], batch["lengths"], unit, order)
    want, want_n = R.rank(s.numpy(), batch["src_key_padding_mask_boxes"].numpy(), batch["lengths"].numpy(), unit, order == "descending")
    assert np.array_equal(rank.numpy(), want) and np.array_equal(n.numpy(), want_n)
    assert int(n[1]) == 0 and (rank[1] == -1).all()
    # NaN last in both orders, the zeros tied
    flat, sc = rank.reshape(6, -1), s.reshape(6, -1)
    for b in range(6):
        c = flat[b] >= 0
        nan = torch.isnan(sc[b]) & c
        if nan.any() and (c & ~nan).any():
            assert flat[b][nan].min() > flat[b][c & ~nan].max()


@pytest.mark.parametrize("activation", ["softmax", "sigmoid"])
def test_curve_torch_form_against_the_restatement(activation, pkg):
    g = torch.Generator().manual_seed(4)
    S, B, K = 4, 7, 9
    x = torch.randn(S, B, K, generator=g) * 3
    x[0, 1, 2] = x[0, 1, 5] = x[0, 1].max() + 1  # a tie at the top of a step-0 row: the first maximum is the target
    x[2, 3] = 0.25                               # every class tied
    for target in (None, torch.tensor([0, 2, 8, 9, -1, 3, 5])):
        prob, hit, tgt = pkg.infer.perturb_curve(x, target, activation)
        rp, rh, rt = R.curve(x.numpy(), None if target is None else target.numpy(), activation)
        assert np.array_equal(tgt.numpy(), rt) and np.array_equal(hit.numpy(), rh)
        assert np.abs(prob.numpy() - rp).max() <= 1e-6
        if target is None:
            assert int(tgt[1]) == 2
        else:
            assert (prob[:, 3:5] == 0).all() and not hit[:, 3:5].any()


def _standin(K=5):
    """a model in three lines: logits from the object count per class-like bucket, so deleting objects moves them"""
    def forward(batch):
        real = (~batch["src_key_padding_mask_boxes"][:, :, 1:]).float()
        feats = torch.stack([(real * batch["boxes"][:, :, 1:, i % 4]).sum((1, 2)) * (1 + i) for i in range(K)], dim=1)
        return feats - feats.mean(dim=1, keepdim=True)
    return forward


def _runner_batches(synth, n_clips):
    out = []
    for i, n in enumerate(n_clips):
        b = synth.make_batch(n, 7, 4, seed=50 + i)
        b["labels"] = torch.randint(0, 5, (n,), generator=torch.Generator().manual_seed(i))
        out.append(b)
    return out


def _box_area(model, batch):
    bx = batch["boxes"]
    return (bx[..., 2] - bx[..., 0]) * (bx[..., 3] - bx[..., 1])


def _area(curve):
    """trapezoid over the fractions 0, 1/steps, ..., 1"""
    return float((curve[1:] + curve[:-1]).sum() / 2 / (len(curve) - 1))


def test_runner_with_a_standin_forward_on_one_rank(pkg, synth):
    batches = _runner_batches(synth, (5, 3))
    fwd = _standin()
    for unit in R.UNITS:
        for target in ("top1", "label"):
            res = pkg.infer.run_perturbation_test(None, batches, method=_box_area, steps=4, unit=unit, target=target, forward=fwd)
            assert res["fractions"] == [0.0, 0.25, 0.5, 0.75, 1.0]
            for order in R.ORDERS:
                prob, hits = np.zeros(5), np.zeros(5)
                for b in batches:
                    sc = _box_area(None, b).numpy()
                    sc = sc if unit == "object" else sc[:, :, 1:].sum(2)
                    rank, n = R.rank(sc, b["src_key_padding_mask_boxes"].numpy(), b["lengths"].numpy(), unit, order == "descending")
                    pert = R.apply(_np({k: b[k] for k in PC.BATCH_KEYS if k in b}), rank, n, 4, 0, 4, 3)
                    logits = fwd({k: torch.from_numpy(v) for k, v in pert.items()}).numpy().reshape(5, -1, 5)
                    p, h, _ = R.curve(logits, b["labels"].numpy() if target == "label" else None)
                    prob += p.sum(1)
                    hits += h.sum(1)
                r = res[order]
                assert r["num_clips"] == 8
                assert np.abs(np.array(r["prob"]) - prob / 8).max() <= 1e-6 and np.array_equal(np.array(r["accuracy"]) * 8, hits)
                assert abs(r["auc_prob"] - _area(prob / 8)) <= 1e-6 and abs(r["auc_accuracy"] - _area(hits / 8)) <= 1e-12
    rnd = pkg.infer.run_perturbation_test(None, batches, method="random", steps=3, forward=fwd, seed=5)
    again = pkg.infer.run_perturbation_test(None, batches, method="random", steps=3, forward=fwd, seed=5)
    assert rnd == again and rnd["descending"]["prob"][0] == rnd["ascending"]["prob"][0]
    for bad in (dict(method="nonsense"), dict(orders=("up",)), dict(unit="pixel"), dict(target="best"), dict(steps=0)):
        with pytest.raises(pkg.StltHipError):
            pkg.infer.run_perturbation_test(None, batches, **dict(dict(method=_box_area, forward=fwd), **bad))


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
    batches = _runner_batches(pkg.synth, n_clips)
    res = pkg.infer.run_perturbation_test(None, batches, method=_box_area, steps=4, rank=rank, world=world, forward=_standin())
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
    one = pkg.infer.run_perturbation_test(None, _runner_batches(synth, n_clips), method=_box_area, steps=4, forward=_standin())
    assert got["fractions"] == one["fractions"]
    for order in R.ORDERS:
        assert got[order]["num_clips"] == one[order]["num_clips"] == 10
        assert got[order]["accuracy"] == one[order]["accuracy"]
        assert np.abs(np.array(got[order]["prob"]) - np.array(one[order]["prob"])).max() <= 1e-12


def test_abi_declares_the_three_launchers(pkg):
    header = open(os.path.join(ROOT, "include", "stlt_hip.h")).read()
    for name in ("stlt_perturb_rank", "stlt_perturb_apply", "stlt_perturb_curve", "stlt_perturb_max_items"):
        assert name in pkg._lib.SIGNATURES and f" {name}(" in header
    assert pkg._lib.load().stlt_perturb_max_items() == 16384
    assert "perturb.hip" in importlib.import_module(PKG_NAME + ".build").SOURCES


def test_cpu_tensors_and_bad_arguments_are_refused_with_a_message(pkg, synth):
    batch = synth.make_batch(2, 5, 3, seed=0)
    scores = torch.rand(2, 5, 3)
    with pytest.raises(pkg.StltHipError, match="GPU tensor"):
        pkg.ops.perturb_rank(scores, batch["src_key_padding_mask_boxes"], batch["lengths"])
    with pytest.raises(pkg.StltHipError, match="GPU tensor"):
        pkg.ops.perturb_apply(batch, torch.zeros(2, 5, 3, dtype=torch.int32), torch.zeros(2, dtype=torch.int32), 3, 0, 3, 3)
    with pytest.raises(pkg.StltHipError, match="GPU tensor"):
        pkg.ops.perturb_curve(torch.zeros(2, 2, 4))
    with pytest.raises(pkg.StltHipError, match="unit 'frame' takes"):
        pkg.collate.perturb_batch(batch, scores, unit="frame")
    with pytest.raises(pkg.StltHipError, match="steps must be >= 1"):
        pkg.collate.perturb_batch(batch, scores, steps=0)
    with pytest.raises(pkg.StltHipError, match="order"):
        pkg.collate.perturb_batch(batch, scores, order="up")
    with pytest.raises(pkg.StltHipError, match="unit"):
        pkg.collate.perturb_batch(batch, scores, unit="pixel")
    with pytest.raises(pkg.StltHipError, match="step_range"):
        pkg.collate.perturb_batch(batch, scores, steps=3, step_range=(2, 4))
    big = synth.make_batch(1, 129, 128, seed=0)
    with pytest.raises(pkg.StltHipError, match="16384"):
        pkg.collate.perturb_batch(big, torch.zeros(1, 129, 128))
