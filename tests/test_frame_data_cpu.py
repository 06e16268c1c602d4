"""Device appearance / multimodal datasets, host side (no GPU): appearance_indices against the reference's sample_appearance_indices
(tests/golden/frame_data.npz, tools/gen_golden_frame_data.py), values and RNG position; the numpy draw order of a shuffled
DeviceMultimodalDataset epoch against the fixture's composed MultimodalDataset epoch; the host checks of the two C-ABI launchers of
csrc/frame_store.hip, through ctypes, with no launch; and the store's bookkeeping (offsets, nbytes, the resident / spill split)."""
import ctypes as C
import io
import json
import os
import types

import numpy as np
import pytest
import torch

from conftest import GOLDEN


@pytest.fixture(scope="module")
def fd(pkg):
    return pkg.frame_data


@pytest.fixture(scope="module")
def golden():
    with open(os.path.join(GOLDEN, "frame_data_schema.json")) as f:
        return np.load(os.path.join(GOLDEN, "frame_data.npz")), json.load(f)


def frame_source(video_ids, frame_counts, sizes):
    """Nested dicts shaped like the reference's HDF5 file: source[video_id][str(frame)] -> a decoded (H, W, 3) uint8 frame."""
    out = {}
    for vid, n, (h, w) in zip(video_ids, frame_counts, sizes):
        frame = np.zeros((h, w, 3), np.uint8)
        out[vid] = {str(j): frame for j in range(int(n))}
    return out


def epoch_config(pkg, meta, directory, train=True):
    e = meta["epoch"]
    p, digest = pkg.synth.write_layout_annotations(str(directory), e["dataset"], e["n_videos"], e["annotation_seed"])
    assert digest == e["digest"], "synth.write_layout_annotations no longer rebuilds the fixture's annotation set"
    return types.SimpleNamespace(dataset_name=e["dataset"], dataset_path=p["annotations"], labels_path=p["labels"], videoid2size_path=p["sizes"],
                                 videos_path="", train=train, layout_num_frames=e["layout_num_frames"],
                                 appearance_num_frames=e["appearance_num_frames"], spatial_size=32, score_threshold=0.5, max_num_objects=7)


def test_fixture_holds_every_branch(golden):
    z, meta = golden
    n, k, train = z["table/frame_count"], z["table/wanted"], z["table/train"]
    assert sorted(set(n.tolist())) == [1, 2, 3, 5, 17, 18, 19, 32, 33, 34, 40, 64, 65, 80] == meta["table"]["frame_counts"]
    assert len(n) == 14 * 2 * 2 and set(k.tolist()) == {16, 32} and set(train.tolist()) == {0, 1}
    row = {(int(a), int(b), int(c)): i for i, (a, b, c) in enumerate(zip(n, k, train))}
    idx = z["table/indices"]
    assert idx[row[1, 16, 1], :16].tolist() == [0] * 16 and idx[row[2, 16, 1], :16].tolist() == [0] * 16  # max(x, 0)
    assert idx[row[17, 16, 1], :16].tolist() == idx[row[17, 16, 0], :16].tolist()  # linspace in training too
    assert sorted(idx[row[18, 16, 1], :16].tolist()) == list(range(16))  # np.random.choice without replacement
    assert idx[row[33, 16, 1], :16].tolist() == list(range(0, 32, 2))  # randint(0, 1)
    assert idx[row[80, 16, 1], :16].tolist() != idx[row[80, 16, 0], :16].tolist()
    assert (idx[k == 16][:, 16:] == -1).all()


def test_appearance_indices_equal_the_reference(fd, golden):
    z, _ = golden
    for r in range(len(z["table/seed"])):
        n, k, train = int(z["table/frame_count"][r]), int(z["table/wanted"][r]), bool(z["table/train"][r])
        np.random.seed(int(z["table/seed"][r]))
        got = fd.appearance_indices(k, n, train)
        assert all(type(i) is int for i in got)
        assert got == z["table/indices"][r, :k].tolist(), (n, k, train)
        assert np.random.random_sample() == z["table/probe"][r], (n, k, train)  # the same draws consumed


def test_multimodal_epoch_draws_in_the_reference_order(fd, pkg, golden, tmp_path):
    z, meta = golden
    e = meta["epoch"]
    cfg = epoch_config(pkg, meta, tmp_path)
    ids = [v["id"] for v in json.load(open(cfg.dataset_path))]
    source = frame_source(ids, z["epoch/frame_counts"], [(40, 52)] * len(ids))
    ds = fd.DeviceMultimodalDataset(cfg, source, device="cpu")
    assert len(ds) == e["n_videos"] and ds.labels is ds.layout_dataset.labels
    assert np.array_equal(ds.appearance_dataset.store.frame_count, z["epoch/frame_counts"])
    loader = ds.loader(e["batch_size"], shuffle=True)
    torch.manual_seed(e["epoch_seed"])
    np.random.seed(e["epoch_seed"])
    order, layout, counts, appearance = [], [], [], []
    for _ in range(e["epochs"]):
        for idx in loader.index_loader:
            (frames, cnt), app = ds.sample_indices([int(i) for i in idx])
            order += [int(i) for i in idx]
            layout.append(np.where(np.arange(frames.shape[1])[None, :] < cnt[:, None], frames, -1))
            counts.append(cnt)
            appearance.append(app)
    assert order == z["epoch/order"].tolist()
    assert np.array_equal(np.concatenate(counts), z["epoch/layout_count"])
    assert np.array_equal(np.concatenate(layout), z["epoch/layout"])
    assert np.array_equal(np.concatenate(appearance), z["epoch/appearance"])
    assert np.random.random_sample() == z["epoch/probe"][0]  # numpy's RNG stands where the reference's epochs left it


def test_layout_collate_checks_indices_drawn_by_the_caller(pkg, golden, tmp_path):
    cfg = epoch_config(pkg, golden[1], tmp_path)
    ds = pkg.layout_data.DeviceStltDataset(cfg, device="cpu")
    with pytest.raises(pkg.StltHipError, match="sampled indices"):
        ds.collate([0, 1], sampled=(np.zeros((2, 3), np.int64), np.zeros(2, np.int64)))
    with pytest.raises(pkg.StltHipError, match="sampled indices"):
        ds.collate([0, 1], sampled=(np.zeros((2, ds.T), np.int64), np.zeros(3, np.int64)))


def _block(fd, offsets, clips):
    """The host block of stlt_frames_batch_fwd: B x T int64 offsets, then B descriptors."""
    raw = np.concatenate([np.asarray(offsets, np.int64).reshape(-1).view(np.uint8), np.asarray(clips, fd.CLIP_DTYPE).view(np.uint8)])
    block = np.zeros(len(raw) // 8 + 1, np.int64)  # 8-byte aligned
    block.view(np.uint8)[:len(raw)] = raw
    return block


def test_cabi_rejects_bad_batches_before_touching_hip(fd):
    """Every case fails in the launcher's host checks (fake device pointers, never dereferenced, nothing copied or launched)."""
    lib = fd.L.load()
    fake = 0x10000
    B, T, S, rh, rw = 2, 3, 32, 40, 50
    fb = rh * rw * 3
    store_bytes, spill_bytes = 4 * fb, 2 * fb  # multiples of 4
    assert lib.stlt_frames_batch_block_bytes(B, T) == B * T * 8 + B * C.sizeof(fd.L.FramesClip)
    assert lib.stlt_frames_batch_block_bytes(0, T) == 0 and lib.stlt_frames_batch_block_bytes(B, 0) == 0 and lib.stlt_frames_batch_block_bytes(1 << 16, 1) == 0

    def clips(**kw):
        c = np.zeros(B, fd.CLIP_DTYPE)
        c["rh"], c["rw"], c["top"], c["left"] = rh, rw, 4, 9
        c["jitter"], c["order"] = 1, (2, 0, 3, 1)
        c["brightness"] = c["contrast"] = c["saturation"] = 1.1
        c["hue_shift"] = 250
        for k, v in kw.items():
            c[k][1] = v
        return c

    good = np.asarray([[0, 2 * fb, fb], [3 * fb, store_bytes, store_bytes + fb]], np.int64)  # the last two lie in the spill area

    def call(offsets=good, c=None, B_=B, T_=T, S_=S, store=fake, sb=store_bytes, spill=fake, pb=spill_bytes, lut=fake, sums=fake, out=fake, dev=fake):
        block = _block(fd, offsets, clips() if c is None else c)
        return lib.stlt_frames_batch_fwd(store, sb, spill, pb, block.ctypes.data, dev, lut, B_, T_, S_, sums, out, None)

    resident = np.asarray([[0, 2 * fb, fb], [3 * fb, 0, fb]], np.int64)  # no frame in the spill area

    def off(b, t, value, base=good):
        o = base.copy()
        o[b, t] = value
        return o

    bad = {
        "offset past the store": lambda: call(off(1, 1, store_bytes - fb + 4, resident), pb=0, spill=None),
        "offset in the last frame's tail": lambda: call(off(1, 2, 3 * fb + 1, resident), pb=0, spill=None),
        "negative offset": lambda: call(off(1, 0, -fb)),
        "offset past the spill area": lambda: call(off(1, 2, store_bytes + fb + 4)),
        "spill offset without a spill area": lambda: call(pb=0, spill=None),
        "crop below the frame": lambda: call(c=clips(top=rh - S + 1)),
        "crop right of the frame": lambda: call(c=clips(left=rw - S + 1)),
        "negative crop origin": lambda: call(c=clips(top=-1)),
        "frame size zero": lambda: call(c=clips(rh=0)),
        "zero T": lambda: call(T_=0),
        "zero B": lambda: call(B_=0),
        "zero S": lambda: call(S_=0),
        "S above the staged row": lambda: call(S_=1025),
        "order repeats an op": lambda: call(c=clips(order=(0, 1, 1, 3))),
        "order out of range": lambda: call(c=clips(order=(0, 1, 2, 4))),
        "jitter flag": lambda: call(c=clips(jitter=2)),
        "hue shift": lambda: call(c=clips(hue_shift=256)),
        "infinite factor": lambda: call(c=clips(contrast=np.inf)),
        "jitter without sums": lambda: call(sums=None),
        "misaligned store": lambda: call(store=fake + 1),
        "unpadded store": lambda: call(sb=store_bytes + 2),
        "misaligned out": lambda: call(out=fake + 4),
        "null lut": lambda: call(lut=None),
        "null device block": lambda: call(dev=None),
        "store size without a store": lambda: call(store=None),
    }
    for name, f in bad.items():
        assert f() == -1, name
        assert lib.stlt_last_error().decode().startswith("stlt_frames_batch_fwd"), name


def test_cabi_rejects_bad_resizes_before_touching_hip(fd, pkg):
    lib = fd.L.load()
    fake = 0x10000
    n, h, w, rh, rw = 3, 40, 50, 36, 45
    kx, tx = pkg.video.resample_table(w, rw)
    ky, ty = pkg.video.resample_table(h, rh)
    out_bytes = n * rh * rw * 3
    ws = lib.stlt_frames_resize_workspace_bytes(n, h, w, rh, rw, kx, ky)
    assert ws >= n * h * rw * 3 + 4 * (tx.size + ty.size)
    assert lib.stlt_frames_resize_workspace_bytes(0, h, w, rh, rw, kx, ky) == 0
    assert lib.stlt_frames_resize_workspace_bytes(n, h, w, rh, rw, 0, ky) == 0
    assert lib.stlt_frames_resize_workspace_bytes(n, h, 1 << 16, rh, rw, kx, ky) == 0
    assert lib.stlt_frames_resize_workspace_bytes(n, h, w, h, w, 0, 0) > 0  # nothing to resample: a copy

    def call(n_=n, tx_=tx, ty_=ty, kx_=kx, ky_=ky, store_bytes=4 * out_bytes, offset=out_bytes, ws_=ws, src=fake, store=fake, work=fake):
        return lib.stlt_frames_resize_fwd(src, n_, h, w, rh, rw, tx_.ctypes.data if tx_ is not None else None, kx_,
                                          ty_.ctypes.data if ty_ is not None else None, ky_, store, store_bytes, offset, work, ws_, None)

    tx_bad = tx.copy()
    tx_bad[2 * 7] = w - 1  # first + count leaves the source row
    ty_bad = ty.copy()
    ty_bad[1] = ky + 1  # more taps than the row of weights holds
    bad = {
        "frames past the store": lambda: call(offset=3 * out_bytes + 1),
        "negative offset": lambda: call(offset=-1),
        "empty store": lambda: call(store_bytes=0, offset=0),
        "workspace too small": lambda: call(ws_=ws - 256),
        "no horizontal table": lambda: call(tx_=None),
        "no vertical table": lambda: call(ty_=None),
        "horizontal entry out of range": lambda: call(tx_=tx_bad),
        "vertical entry out of range": lambda: call(ty_=ty_bad),
        "zero frames": lambda: call(n_=0),
        "zero taps": lambda: call(kx_=0),
        "null source": lambda: call(src=None),
        "null store": lambda: call(store=None),
        "null workspace": lambda: call(work=None),
    }
    for name, f in bad.items():
        assert f() == -1, name
        assert lib.stlt_last_error().decode().startswith("stlt_frames_resize_fwd"), name


def test_store_bookkeeping_and_the_resident_spill_split(fd, pkg):
    video = pkg.video
    S, target = 32, 36
    sizes = [(40, 50), (36, 61), (53, 37), (30, 41), (36, 36), (40, 50)]
    counts = [5, 3, 7, 1, 4, 2]
    ids = [f"v{i}" for i in range(len(sizes))]
    source = frame_source(ids, counts, sizes)
    store = fd.DeviceFrameStore(source, ids, spatial_size=S, device="cpu")
    assert store.target == target and len(store) == 6
    resized = [video.resized_size(h, w, target) for h, w in sizes]
    assert resized[1] == (36, 61) and resized[4] == (36, 36)  # a short side equal to the target is kept
    assert store.size.tolist() == [list(r) for r in resized] and store.source_size.tolist() == [list(s) for s in sizes]
    video_bytes = [n * rh * rw * 3 for n, (rh, rw) in zip(counts, resized)]
    assert store.frame_count.tolist() == counts and store.video_bytes.tolist() == video_bytes
    assert store.video_offset.tolist() == np.concatenate([[0], np.cumsum(video_bytes)[:-1]]).tolist()
    assert store.nbytes == store.total_bytes == sum(video_bytes) and all(store.resident(i) for i in range(6))
    assert store.center.tolist() == [list(video.center_crop_offsets(rh, rw, S)) for rh, rw in resized]
    # a capacity that cuts the set in the middle: videos 0..2 fit, video 3 would too but comes after the first one that does not
    cap = sum(video_bytes[:3]) + video_bytes[3] - 1
    cut = fd.DeviceFrameStore(source, ids, spatial_size=S, device="cpu", capacity_bytes=cap)
    assert [cut.resident(i) for i in range(6)] == [True, True, True, False, False, False]
    assert cut.nbytes == sum(video_bytes[:3]) and cut.total_bytes == sum(video_bytes)
    assert cut.video_offset.tolist()[:3] == store.video_offset.tolist()[:3] and cut.video_offset.tolist()[3:] == [-1, -1, -1]
    exact = fd.DeviceFrameStore(source, ids, spatial_size=S, device="cpu", capacity_bytes=sum(video_bytes[:2]))
    assert [exact.resident(i) for i in range(6)] == [True, True, False, False, False, False] and exact.nbytes == sum(video_bytes[:2])
    none = fd.DeviceFrameStore(source, ids, spatial_size=S, device="cpu", capacity_bytes=0)
    assert none.nbytes == 0 and not any(none.resident(i) for i in range(6))
    with pytest.raises(ValueError):
        fd.DeviceFrameStore(source, ids, spatial_size=S, device="cpu", capacity_bytes=-1)
    with pytest.raises(KeyError):
        fd.DeviceFrameStore(source, ids + ["absent"], spatial_size=S, device="cpu")
    with pytest.raises(ValueError, match="no frames"):
        fd.DeviceFrameStore(dict(source, empty={}), ["empty"], spatial_size=S, device="cpu")
    with pytest.raises(pkg.StltHipError, match="GPU"):
        store.ingest()


def test_frames_must_be_rgb_and_share_one_size(fd):
    good = np.zeros((40, 50, 3), np.uint8)
    assert fd.decode_frame(good) is good
    for bad in (np.zeros((40, 50), np.uint8), np.zeros((40, 50, 4), np.uint8), np.zeros((40, 50, 3), np.uint16), np.zeros((40, 50, 3), np.float32)):
        with pytest.raises(ValueError):
            fd.decode_frame(bad)
    source = {"a": {"0": good, "1": good, "2": np.zeros((41, 50, 3), np.uint8)}, "b": {"0": good, "1": np.zeros((40, 50), np.uint8)}}
    store = fd.DeviceFrameStore(source, ["a", "b"], spatial_size=32, device="cpu")
    assert store._decode(0, [0, 1]).shape == (2, 40, 50, 3)
    with pytest.raises(ValueError, match="share one size"):
        store._decode(0, [0, 1, 2])
    with pytest.raises(ValueError, match="uint8"):
        store._decode(1, [0, 1])


def test_encoded_frames_decode_through_pillow(fd):
    Image = pytest.importorskip("PIL.Image")
    rng = np.random.default_rng(0)
    frame = rng.integers(0, 256, (40, 50, 3), dtype=np.uint8)

    def encoded(img, fmt):
        b = io.BytesIO()
        img.save(b, fmt)
        return b.getvalue()

    png = encoded(Image.fromarray(frame, "RGB"), "PNG")
    assert np.array_equal(fd.decode_frame(png), frame)
    assert np.array_equal(fd.decode_frame(np.frombuffer(png, np.uint8)), frame)  # what an HDF5 dataset of bytes reads as
    store = fd.DeviceFrameStore({"a": {"0": png, "1": np.frombuffer(png, np.uint8)}}, ["a"], spatial_size=32, device="cpu")
    assert store.source_size.tolist() == [[40, 50]] and store.frame_count.tolist() == [2]
    with pytest.raises(ValueError, match="mode"):
        fd.decode_frame(encoded(Image.fromarray(frame[..., 0], "L"), "PNG"))


def test_dataset_contract_on_the_host(fd, pkg, golden, tmp_path):
    z, meta = golden
    cfg = epoch_config(pkg, meta, tmp_path, train=False)
    videos = json.load(open(cfg.dataset_path))
    ids = [v["id"] for v in videos]
    source = frame_source(ids, z["epoch/frame_counts"], [(40, 52)] * len(ids))
    app = fd.DeviceAppearanceDataset(cfg, source, device="cpu")
    lay = pkg.layout_data.DeviceStltDataset(cfg, device="cpu")
    assert len(app) == len(videos) and app.video_ids == ids and np.array_equal(app.video_label, lay.video_label)
    # evaluation draws nothing and takes the centre window or the spread
    np.random.seed(1)
    before = np.random.get_state()[1].copy()
    idx = app.sample_indices(list(range(len(app))))
    assert np.array_equal(np.random.get_state()[1], before)
    rows = {int(n): z["table/indices"][r, :16] for r, n in enumerate(z["table/frame_count"]) if z["table/wanted"][r] == 16 and not z["table/train"][r]}
    for i, n in enumerate(z["epoch/frame_counts"]):
        assert np.array_equal(idx[i], rows[int(n)])
    with pytest.raises(pkg.StltHipError, match="empty batch"):
        app.collate([])
    with pytest.raises(IndexError):
        app.collate([len(app)])
    with pytest.raises(ValueError, match="something"):
        fd.DeviceAppearanceDataset(types.SimpleNamespace(**dict(vars(cfg), dataset_name="action_genome")), source, device="cpu")
    assert len(app.loader(8)) == len(app) // 8 and len(fd.DeviceMultimodalDataset(cfg, source, device="cpu").loader(8, drop_last=True)) == 5


def test_appearance_only_batches_shard_and_count(pkg):
    """Batches without `categories` (DeviceAppearanceDataset) go through the sharding and the inference loop by their video_frames."""
    labels = torch.tensor([0, 1, 2, 1, 0])
    batch = {"video_frames": torch.zeros(5, 3, 2, 4, 4), "labels": labels, "video_id": list("abcde")}
    assert pkg.dist.batch_size(batch) == 5 and pkg.dist.batch_size(dict(batch, categories=torch.zeros(4, 1, 1))) == 4
    parts = [pkg.dist.shard_batch(batch, r, 2) for r in range(2)]
    assert sum(p["video_frames"].shape[0] for p in parts) == 5
    assert all(p["video_frames"].shape[0] == p["labels"].shape[0] == len(p["video_id"]) for p in parts)
    assert parts[0]["video_id"] + parts[1]["video_id"] == list("abcde")
    hit = torch.nn.functional.one_hot(labels, 8).float()
    out = pkg.infer.run_inference(object(), [batch, batch], "cpu", forward=lambda b: hit[:b["video_frames"].shape[0]])
    assert out == {"top1_accuracy": 100.0, "top5_accuracy": 100.0, "num_clips": 10}
