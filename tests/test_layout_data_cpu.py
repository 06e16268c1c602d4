"""Device layout dataset, host side (no GPU): the numpy restatement (tests/layout_restated.py) against the reference's own batches
(tests/golden/layout_dataset.npz, tools/gen_golden_layout_dataset.py); the host half of DeviceStltDataset — parse, max_num_objects,
frame indices, labels, real counts, the batched training uniforms, the epoch order of loader() — against the goldens and the
restatement; a numpy emulation of the batch kernel over the parsed tables against every golden batch; and the host checks of the two
C-ABI launchers, through ctypes, with no launch."""
import ctypes as C
import json

import numpy as np
import pytest
import torch

import layout_restated as R


@pytest.fixture(scope="module")
def ld(pkg):
    return pkg.layout_data


def _restated(ld, dataset, train, T=16):
    return R.Restated(*R.load_annotations(dataset), dataset, T, train, 0.5, ld.CATEGORY2ID[dataset], ld.FRAME2TYPE[dataset])


def test_golden_covers_the_edge_cases(ld):
    meta = R.golden_meta()
    for dataset in ("something", "action_genome"):
        videos = R.load_annotations(dataset)[0]
        nframes = [len(v["frames"]) for v in videos]
        assert {0, 1, 15, 16, 17}.issubset(nframes) and max(nframes) >= 300
        objs = [o for v in videos for fr in v["frames"] for o in fr["frame_objects"]]
        assert any(o["x1"] > o["x2"] for o in objs) and any(o["y1"] > o["y2"] for o in objs)
        assert any(min(o["x1"], o["y1"]) < 0 for o in objs) and any(o["x1"] == o["x2"] for o in objs)
        assert any(o["score"] == 0.5 for o in objs) and any(isinstance(o["x1"], float) for o in objs)
        assert any(not fr["frame_objects"] for v in videos for fr in v["frames"])
        assert any(fr["frame_objects"] and all(o["score"] < 0.5 for o in fr["frame_objects"]) for v in videos for fr in v["frames"])
        if dataset == "something":
            assert any("[" in v["template"] for v in videos)
        else:
            assert any(len(v["actions"]) > 1 for v in videos)
        modes = {c["mode"] for c in meta["cases"] if c["dataset"] == dataset}
        assert modes == {"test", "train", "epoch"}
        assert {c["epoch"] for c in meta["cases"] if c["dataset"] == dataset and c["mode"] == "epoch"} == {0, 1}


@pytest.mark.parametrize("dataset", ["something", "action_genome"])
def test_restatement_equals_the_reference(ld, dataset):
    z = R.golden_arrays()
    rs = {False: _restated(ld, dataset, False), True: _restated(ld, dataset, True)}
    for case in R.golden_cases(dataset):
        r = rs[case["mode"] != "test"]
        assert r.max_num_objects == case["max_num_objects"]
        R.seed_for(case)
        R.check_case(case, z, r.collate(case["indices"]))


def _emulate(ds, indices, frames, counts):
    """The batch kernel (csrc/layout_data.hip) in numpy over the dataset's parsed tables, boxes through the restated fix_box."""
    v = np.asarray(indices, np.int64)
    B, Lf, N = len(v), int(counts.max()) + 1, ds.N
    cls = ds.category2id["cls"]
    cats = np.zeros((B, Lf, N), np.int64)
    cats[:, :, 0] = cls
    boxes = np.zeros((B, Lf, N, 4), np.float32)
    boxes[:, :, 0] = (0, 0, 1, 1)
    scores = np.zeros((B, Lf, N), np.float32)
    scores[:, :, 0] = 1
    ft = np.zeros((B, Lf), np.int64)
    for b in range(B):
        w, h = ds.video_size[v[b]]
        for t in range(counts[b]):
            gf = ds.video_frames[v[b]] + frames[b, t]
            o0, o1 = ds.frame_objects[gf], ds.frame_objects[gf + 1]
            for k, o in enumerate(range(o0, o1)):
                cats[b, t, k + 1] = ds.object_category[o]
                scores[b, t, k + 1] = ds.object_score[o]
                boxes[b, t, k + 1] = np.asarray(R.fix_box(list(ds.object_box_raw[o]), h, w), np.float32) / np.float32([w, h, w, h])
            ft[b, t] = ds.frame2type["empty"] if ds.frame_empty[gf] else ds.frame2type["regular"]
        ft[b, counts[b]] = ds.frame2type["extract"]
    out = dict(categories=cats, boxes=boxes, frame_types=ft, lengths=counts.astype(np.int64) + 1, labels=ds.host_labels(v),
               src_key_padding_mask_boxes=cats == 0, src_key_padding_mask_frames=ft == 0, video_id=[ds.video_ids[i] for i in v])
    if ds.dataset_name == "action_genome":
        out["scores"] = scores
    return out


def _real_counts(batch):
    real = ~batch["src_key_padding_mask_frames"]
    return {"num_real_tokens": int(((~batch["src_key_padding_mask_boxes"]) & real[:, :, None]).sum()), "num_real_frames": int(real.sum())}


@pytest.mark.parametrize("dataset", ["something", "action_genome"])
def test_host_tables_reproduce_every_golden_batch(ld, dataset):
    z = R.golden_arrays()
    dss = {m: ld.DeviceStltDataset(R.config(dataset, m), device="cpu") for m in (False, True)}
    for case in R.golden_cases(dataset):
        ds = dss[case["mode"] != "test"]
        assert ds.max_num_objects == case["max_num_objects"] and ds.config.max_num_objects == case["max_num_objects"]
        R.seed_for(case)
        frames, counts = ds.sample_indices(case["indices"])
        got = _emulate(ds, case["indices"], frames, counts)
        R.check_case(case, z, got)
        assert ds.host_real_counts(case["indices"], frames, counts) == _real_counts(got)


def test_parse_and_vocabularies(ld):
    ds = ld.DeviceStltDataset(R.config("action_genome", False), device="cpu")
    videos, labels, _ = R.load_annotations("action_genome")
    assert len(ds) == len(videos) and ds.video_ids == [v["id"] for v in videos]
    assert ds.category2id["cls"] == 1 and ds.category2id["person"] == 37 and len(ds.category2id) == 38
    assert ds.frame2type == {"pad": 0, "regular": 1, "extract": 2, "empty": 3}
    assert ds.labels == labels and ds.n_classes == 157
    assert len(ds.frame_empty) == sum(len(v["frames"]) for v in videos)
    kept = [o for v in videos for fr in v["frames"] for o in fr["frame_objects"] if o["score"] >= 0.5]
    assert len(ds.object_category) == len(kept)
    assert np.array_equal(ds.object_score, np.asarray([o["score"] for o in kept], np.float64).astype(np.float32))
    assert ds.object_box_raw.min() >= 0 and ds.object_box_raw.max() == ld.BOX_SATURATION  # the > 2^31 coordinates saturate
    s = ld.DeviceStltDataset(R.config("something", True), device="cpu")
    assert s.category2id == {"pad": 0, "hand": 1, "object": 2, "cls": 3} and s.frame2type["extract"] == 4 and s.n_classes == 0


def test_bad_annotations_raise_the_reference_errors(ld, tmp_path):
    videos, labels, sizes = R.load_annotations("something")

    def build(v=videos, lab=labels, sz=sizes):
        p = {}
        for k, obj in (("annotations", v), ("labels", lab), ("sizes", sz)):
            p[k] = str(tmp_path / f"{k}.json")
            json.dump(obj, open(p[k], "w"))
        return ld.DeviceStltDataset(R.config("something", False, paths=p), device="cpu")

    build()
    vid = next(v for v in videos if any(o["score"] >= 0.5 for fr in v["frames"] for o in fr["frame_objects"]))
    bad = json.loads(json.dumps(videos))
    o = next(o for v in bad if v["id"] == vid["id"] for fr in v["frames"] for o in fr["frame_objects"] if o["score"] >= 0.5)
    o["category"] = "spoon"
    with pytest.raises(KeyError):
        build(v=bad)
    o["score"] = 0.25  # below the threshold an unknown category is never looked up (datasets.py:72-84)
    build(v=bad)
    with pytest.raises(ValueError):
        build(sz=dict(sizes, **{vid["id"]: [320.0, 240]}))
    with pytest.raises(ValueError):
        build(sz=dict(sizes, **{vid["id"]: [0, 240]}))
    with pytest.raises(KeyError):
        build(sz={k: s for k, s in sizes.items() if k != vid["id"]})
    with pytest.raises(KeyError):
        build(lab={k: s for i, (k, s) in enumerate(labels.items()) if i})


def test_eval_indices_equal_the_reference_expression(ld):
    for T in range(1, 65):
        n = np.arange(0, 301)
        idx, cnt = ld.layout_test_indices(T, n)
        for ni in n:
            ref = R.eval_indices(T, int(ni))
            assert cnt[ni] == len(ref) == min(ni, T) and idx[ni, :len(ref)].tolist() == ref, (T, ni)


def test_train_indices_equal_the_per_sample_draws(ld):
    rng = np.random.Generator(np.random.PCG64(5))
    for T in range(1, 65):
        n = rng.integers(0, 301, size=12)
        n[:3] = (0, T, max(T - 1, 0))
        np.random.seed(T)
        ref = [R.train_indices(T, int(ni)) for ni in n]
        after_ref = np.random.random_sample()
        np.random.seed(T)
        idx, cnt = ld.layout_train_indices(T, n)
        assert np.random.random_sample() == after_ref  # the same number of draws
        for b, r in enumerate(ref):
            assert cnt[b] == len(r) == (T if n[b] > 0 else 0) and idx[b, :len(r)].tolist() == r, (T, n[b])
    # the batched stream: avg * random_sample == np.random.uniform(0, avg), value by value
    avgs = np.asarray([0.3, 1.0, 18.75, 299 / 7])
    np.random.seed(3)
    want = np.stack([np.random.uniform(0, a, size=16) for a in avgs])
    np.random.seed(3)
    u = np.random.random_sample(4 * 16).reshape(4, 16)
    assert np.array_equal(avgs[:, None] * u, want)
    # a floor that reaches n raises IndexError, as the reference's frames[n] would
    with pytest.raises(IndexError):
        ld.layout_train_indices(4, np.asarray([9]), uniforms=np.ones((1, 4)))


@pytest.mark.parametrize("dataset", ["something", "action_genome"])
def test_loader_batch_order_is_the_reference_dataloaders(ld, dataset):
    ds = ld.DeviceStltDataset(R.config(dataset, True), device="cpu")
    loader = ds.loader(8, shuffle=True)
    cases = R.golden_cases(dataset, "epoch")
    torch.manual_seed(cases[0]["seed"])
    got = [list(map(int, idx)) for _ in range(2) for idx in loader.index_loader]
    assert got == [c["indices"] for c in cases] and len(loader) == len(cases) // 2
    assert len(ds.loader(8, drop_last=True)) == len(ds) // 8


def _table(ld, ds, fake=0x1000):
    tab = ld.L.LayoutTable()
    tab.n_videos, tab.n_frames, tab.n_objects, tab.n_actions = len(ds), len(ds.frame_empty), len(ds.object_category), len(ds.actions)
    tab.n_classes, tab.cls_id, tab.type_regular, tab.type_empty, tab.type_extract = ds.n_classes, 1, 1, 3, 2
    ds._keep = np.append(ds.actions, 0).astype(np.int32)
    tab.video_frames_host, tab.frame_objects_host = ds.video_frames.ctypes.data, ds.frame_objects.ctypes.data
    tab.video_actions_host, tab.actions_host = ds.video_actions.ctypes.data, ds._keep.ctypes.data
    for k in ("video_frames", "frame_objects", "frame_empty", "object_category", "object_score", "object_box", "video_label", "video_actions",
              "actions"):
        setattr(tab, k, fake)
    return tab


def test_cabi_rejects_bad_batches_before_touching_hip(ld):
    """Every case fails in the launcher's host checks (fake device pointers, never dereferenced, nothing launched)."""
    lib = ld.L.load()
    ds = ld.DeviceStltDataset(R.config("action_genome", False), device="cpu")
    T, N = ds.T, ds.N
    fake = 0x1000
    v = np.asarray([5, 3], np.int64)  # videos of 300 and 16 frames
    frames, counts = ds.sample_indices(v)
    Lf = int(counts.max()) + 1

    def call(vids=v, cnt=counts, fr=frames, tab=None, B=2, T_=T, L_=Lf, N_=N, boxes=fake, labels=fake):
        packed = np.concatenate([np.asarray(vids), np.asarray(cnt), np.asarray(fr).reshape(-1)]).astype(np.int32)
        t = tab if tab is not None else _table(ld, ds)
        return lib.stlt_layout_batch_fwd(C.byref(t), packed.ctypes.data, fake, B, T_, L_, N_, fake, boxes, fake, fake, fake, fake, fake, labels, None)

    fr_bad = frames.copy()
    fr_bad[0, 3] = 300
    fr_neg = frames.copy()
    fr_neg[1, 0] = -1
    t_small = _table(ld, ds)
    t_small.n_objects = 3
    t_noact = _table(ld, ds)
    t_noact.actions_host = None
    t_badact = _table(ld, ds)
    t_badact.n_classes = 1
    bad = {
        "video index": lambda: call(vids=[5, len(ds)]),
        "negative video": lambda: call(vids=[-1, 3]),
        "count above T": lambda: call(cnt=[T + 1, 1]),
        "negative count": lambda: call(cnt=[-1, 1]),
        "frame past the video": lambda: call(fr=fr_bad),
        "negative frame": lambda: call(fr=fr_neg),
        "L too small": lambda: call(L_=Lf - 1),
        "N too small": lambda: call(N_=1),
        "objects past the table": lambda: call(tab=t_small),
        "no action lists": lambda: call(tab=t_noact),
        "action out of range": lambda: call(tab=t_badact),
        "zero B": lambda: call(B=0),
        "misaligned boxes": lambda: call(boxes=fake + 4),
        "null labels": lambda: call(labels=None),
    }
    for name, f in bad.items():
        assert f() == -1, name
        assert lib.stlt_last_error().decode().startswith("stlt_layout_batch_fwd"), name
    assert lib.stlt_layout_batch_fwd(None, fake, fake, 1, T, 1, N, fake, fake, fake, fake, fake, fake, fake, fake, None) == -1
    # the box pass: counts and alignment; zero objects is a no-op
    assert lib.stlt_layout_boxes_fwd(fake, fake, -1, fake, None) == -1
    assert lib.stlt_layout_boxes_fwd(fake + 4, fake, 10, fake, None) == -1
    assert lib.stlt_layout_boxes_fwd(fake, fake, 10, fake + 8, None) == -1
    assert lib.stlt_layout_boxes_fwd(None, fake, 10, fake, None) == -1
    assert lib.stlt_layout_boxes_fwd(None, None, 0, None, None) == 0


def test_collate_contract_errors_on_the_host(ld, pkg):
    ds = ld.DeviceStltDataset(R.config("something", False), device="cpu")
    with pytest.raises(pkg.StltHipError, match="empty batch"):
        ds.collate([])
    with pytest.raises(IndexError):
        ds.collate([len(ds)])
