"""Device layout dataset on the GPU: every golden batch of the reference (tools/gen_golden_layout_dataset.py) bit for bit through
DeviceStltDataset.collate in both modes and both datasets, the two golden shuffled epochs through loader(shuffle=True), randomised
annotation sets against the numpy restatement (tests/layout_restated.py), the host-counted real_counts, Stlt logits on loader batches
against the same batch from the restatement through DeviceCollater, one Trainer.fit_epochs epoch and one run_inference pass on the
loader, and a captured torch.cuda.graph of collate."""

import numpy as np
import pytest
import torch

import layout_restated as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def ld(pkg):
    return pkg.layout_data


@pytest.mark.parametrize("dataset", ["something", "action_genome"])
def test_golden_batches_bit_identical(ld, dataset):
    z = R.golden_arrays()
    dss = {m: ld.DeviceStltDataset(R.config(dataset, m), device=DEV) for m in (False, True)}
    for case in R.golden_cases(dataset):
        if case["mode"] != "epoch":
            R.seed_for(case)
            R.check_case(case, z, dss[case["mode"] == "train"].collate(case["indices"]))


@pytest.mark.parametrize("dataset", ["something", "action_genome"])
def test_golden_shuffled_epochs(ld, dataset):
    meta = R.golden_meta()
    z = R.golden_arrays()
    cases = R.golden_cases(dataset, "epoch")
    ds = ld.DeviceStltDataset(R.config(dataset, True), device=DEV)
    # the batch order of a live DataLoader over range(n) on this torch: a difference here is a torch version difference, not a content one
    torch.manual_seed(meta["epoch_seed"])
    live = torch.utils.data.DataLoader(range(len(ds)), batch_size=meta["batch_size"], shuffle=True, collate_fn=lambda b: b)
    order = [list(map(int, b)) for _ in range(2) for b in live]
    assert order == [c["indices"] for c in cases], f"DataLoader order differs from the golden's (torch {torch.__version__} vs {meta['torch']})"
    torch.manual_seed(meta["epoch_seed"])
    np.random.seed(meta["epoch_seed"])
    loader = ds.loader(meta["batch_size"], shuffle=True)
    got = [b for _ in range(2) for b in loader]
    assert len(got) == len(cases)
    for case, batch in zip(cases, got):
        R.check_case(case, z, batch)


@pytest.mark.parametrize("dataset,seed,T", [("something", 101, 16), ("action_genome", 102, 16), ("something", 103, 5), ("action_genome", 104, 33)])
def test_random_sets_match_the_restatement(ld, pkg, tmp_path, dataset, seed, T):
    p, _ = pkg.synth.write_layout_annotations(str(tmp_path), dataset, 60, seed, max_frames=70, max_objects=7)
    videos, labels, sizes = R.load_annotations(dataset, p)
    rng = np.random.Generator(np.random.PCG64(seed))
    for train in (False, True):
        ds = ld.DeviceStltDataset(R.config(dataset, train, p, T), device=DEV)
        r = R.Restated(videos, labels, sizes, dataset, T, train, 0.5, ld.CATEGORY2ID[dataset], ld.FRAME2TYPE[dataset])
        assert ds.max_num_objects == r.max_num_objects
        for it in range(6):
            idx = rng.integers(0, len(videos), size=int(rng.integers(1, 40))).tolist()
            np.random.seed(seed * 10 + it)
            want = r.collate(idx)
            np.random.seed(seed * 10 + it)
            got = ds.collate(idx, real_counts=True)
            for k in want:
                if k != "video_id":
                    R.same(got[k], want[k], (dataset, train, it, k))
            assert got["video_id"] == want["video_id"]
            assert {k: got[k] for k in ("num_real_tokens", "num_real_frames")} == pkg.collate.real_counts(got)
    torch.cuda.synchronize()


def _model(pkg, dataset, N, T):
    synth = pkg.synth
    classes = 174 if dataset == "something" else 157
    cfg = pkg.StltModelConfig(num_classes=classes, unique_categories=synth.DATASETS[dataset]["unique_categories"], hidden_size=64,
                              num_attention_heads=4, num_spatial_layers=1, num_temporal_layers=2, hidden_dropout_prob=0.0,
                              layout_num_frames=T + 1)
    m = pkg.Stlt(cfg)
    m.load_state_dict(synth.make_state_dict({k: tuple(v.shape) for k, v in m.state_dict().items()}, seed=7))
    return m.to(DEV)


@pytest.mark.parametrize("dataset", ["something", "action_genome"])
def test_stlt_logits_from_loader_equal_restated_batches(ld, pkg, dataset):
    ds = ld.DeviceStltDataset(R.config(dataset, False), device=DEV)
    r = R.Restated(*R.load_annotations(dataset), dataset, 16, False, 0.5,
                   ld.CATEGORY2ID[dataset], ld.FRAME2TYPE[dataset])
    model = _model(pkg, dataset, ds.N, ds.T)
    model.train(False)
    col = pkg.collate.DeviceCollater(dataset, DEV)
    for idx, batch in zip(ds.loader(8).index_loader, ds.loader(8)):
        items = [r.item(i) for i in idx]
        samples = [{k: torch.as_tensor(v) for k, v in it.items() if k != "video_id"} for it in items]
        ref_batch = col(samples)
        with torch.no_grad():
            a = model(batch)["stlt"]
            b = model(ref_batch)["stlt"]
        assert torch.equal(a, b)


def test_fit_epochs_and_inference_run_on_the_loader(ld, pkg):
    dataset = "something"
    train_ds = ld.DeviceStltDataset(R.config(dataset, True), device=DEV)
    val_ds = ld.DeviceStltDataset(R.config(dataset, False), device=DEV)
    model = _model(pkg, dataset, train_ds.N, train_ds.T)
    train_loader = train_ds.loader(8, shuffle=True, drop_last=True)
    trainer = pkg.train.Trainer(model, dataset, learning_rate=1e-4, warmup_steps=0, total_steps=len(train_loader))
    evaluator = pkg.evaluators_factory[dataset](len(val_ds), 174, ("stlt",))
    torch.manual_seed(0)
    np.random.seed(0)
    hist = trainer.fit_epochs(lambda e: train_loader, val_ds.loader(8), evaluator, 1, DEV)
    assert len(hist) == 1 and len(hist[0]["steps"]) == len(train_loader)
    assert all(np.isfinite(s["loss"]) for s in hist[0]["steps"])
    out = pkg.infer.run_inference(model, val_ds.loader(8, real_counts=True), DEV)
    assert out["num_clips"] == len(val_ds)


def test_captured_graph_replays_the_batch(ld):
    ds = ld.DeviceStltDataset(R.config("action_genome", False), device=DEV)
    idx = [5, 3, 2, 9, 0, 1, 17, 30]
    want = ds.collate(idx)  # warm-up: pinned blocks and the device tables exist before the capture
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        ds.collate(idx)
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        got = ds.collate(idx)
    for k in got:
        if isinstance(got[k], torch.Tensor):
            got[k].zero_()
    g.replay()
    torch.cuda.synchronize()
    for k in want:
        if k != "video_id":
            assert torch.equal(got[k], want[k]), k
    ds.collate([1, 2])  # the ring keeps serving eager batches after the capture took a block
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(got["boxes"], want["boxes"])
