"""Device video collater, host side (no GPU): the numpy restatement of the Pillow arithmetic (tests/pil_restated.py) against the installed
Pillow — exhaustively for L and both HSV conversions, over random frames and factors for the blends and every hue shift, over >= 200 size
pairs for the resampling — and the package's own host half against the restatement: resample tables, normalisation table, resize and
centre-crop geometry, the torch draw sequence of draw_clip_params, the C-ABI's descriptor checks, and the fixture's crops."""
import ctypes as C
import json
import math
import os

import numpy as np
import pytest
import torch

import pil_restated as R
from conftest import GOLDEN

BIG = 1 << 24


@pytest.fixture(scope="module")
def video(pkg):
    return pkg.video


def _all_rgb():
    v = np.arange(BIG, dtype=np.uint32)
    return np.stack([(v >> 16) & 255, (v >> 8) & 255, v & 255], -1).astype(np.uint8).reshape(4096, 4096, 3)


def test_luma_and_hsv_exhaustive():
    Image = pytest.importorskip("PIL.Image")
    rgb = _all_rgb()
    im = Image.fromarray(rgb, "RGB")
    assert np.array_equal(np.asarray(im.convert("L")), R.luma(rgb))
    for rows in (slice(0, 2048), slice(2048, 4096)):  # halves keep the float64 temporaries small
        part = np.ascontiguousarray(rgb[rows])
        assert np.array_equal(np.asarray(Image.fromarray(part, "RGB").convert("HSV")), R.rgb_to_hsv(part)), "RGB -> HSV"
        assert np.array_equal(np.asarray(Image.fromarray(part, "HSV").convert("RGB")), R.hsv_to_rgb(part)), "HSV -> RGB"


def test_blends_and_hue_against_pil():
    Image = pytest.importorskip("PIL.Image")
    ImageEnhance = pytest.importorskip("PIL.ImageEnhance")
    rng = np.random.default_rng(3)
    for i in range(60):
        img = rng.integers(0, 256, (int(rng.integers(1, 40)), int(rng.integers(1, 40)), 3), dtype=np.uint8)
        if i % 4 == 0:  # low-contrast frames put the contrast mean and the clipping at their edges
            img = (img // 16 + rng.integers(0, 240)).astype(np.uint8)
        f = float(np.float32(rng.uniform(0.0, 2.0) if i % 3 else rng.uniform(0.75, 1.25)))
        im = Image.fromarray(img, "RGB")
        assert np.array_equal(np.asarray(ImageEnhance.Brightness(im).enhance(f)), R.brightness(img, f)), ("brightness", i, f)
        assert np.array_equal(np.asarray(ImageEnhance.Contrast(im).enhance(f)), R.contrast(img, f)), ("contrast", i, f)
        assert np.array_equal(np.asarray(ImageEnhance.Color(im).enhance(f)), R.saturation(img, f)), ("color", i, f)
    img = rng.integers(0, 256, (64, 64, 3), dtype=np.uint8)
    h, s, v = Image.fromarray(img, "RGB").convert("HSV").split()
    for shift in range(256):  # adjust_hue's uint8 add, every shift
        np_h = (np.array(h, dtype=np.uint8) + np.uint8(shift)).astype(np.uint8)
        ref = np.asarray(Image.merge("HSV", (Image.fromarray(np_h, "L"), s, v)).convert("RGB"))
        assert np.array_equal(ref, R.hue(img, shift)), shift


def test_hue_shift_truncates_then_wraps(video):
    for f, want in ((0.0, 0), (0.1, 25), (0.0999, 25), (-0.0999, 231), (-0.1, 231), (-0.003, 0), (-0.004, 255), (0.05, 12), (-0.05, 244)):
        assert R.hue_shift(f) == want == video.hue_shift(f), f
    fs = torch.empty(2000).uniform_(-0.1, 0.1, generator=torch.Generator().manual_seed(0)).tolist()
    assert all(video.hue_shift(f) == (int(f * 255) & 255) for f in fs)


def _size_pairs():
    rng = np.random.default_rng(11)
    pairs = [(240, 128), (427, 227), (128, 112), (30, 36), (1, 5), (5, 1), (1000, 37), (37, 1000), (113, 112), (112, 113)]
    while len(pairs) < 220:
        a = int(rng.integers(1, 400))
        pairs.append((a, int(rng.integers(1, 400))))
    return pairs


def test_resample_against_pil(video):
    Image = pytest.importorskip("PIL.Image")
    rng = np.random.default_rng(5)
    for i, (a, b) in enumerate(_size_pairs()):
        k, bounds, coeffs = R.resample_table(a, b)
        k2, table = video.resample_table(a, b)
        assert k == k2 and np.array_equal(table, np.concatenate([bounds.ravel(), coeffs.ravel()])), (a, b)
        h = int(rng.integers(1, 24))
        img = rng.integers(0, 256, (h, a, 3), dtype=np.uint8)
        if i % 3 == 0:
            oh, ow = h, b  # horizontal only
        elif i % 3 == 1:
            img = np.ascontiguousarray(img.transpose(1, 0, 2))[:, :h]
            oh, ow = b, img.shape[1]  # vertical only
        else:
            oh, ow = int(rng.integers(1, 48)), b  # both axes
        ref = np.asarray(Image.fromarray(np.ascontiguousarray(img)).resize((ow, oh), Image.BILINEAR))
        assert np.array_equal(ref, R.resize(img, oh, ow)), (img.shape, oh, ow)


def test_normalize_table(video):
    lut = video.normalize_table()
    ref = torch.arange(256, dtype=torch.uint8)[None, None].to(torch.float32).div(255)  # ToTensor
    ref = ref.sub_(torch.tensor([0.5])[:, None, None]).div_(torch.tensor([0.5])[:, None, None])  # Normalize
    assert torch.equal(lut, ref.flatten()) and np.array_equal(lut.numpy(), R.normalize_table())


def test_resize_and_center_crop_geometry(video):
    t = math.floor(112 * 1.15)
    assert t == 128 and math.floor(32 * 1.15) == 36
    assert video.resized_size(240, 427, t) == (128, 227)
    assert video.resized_size(427, 240, t) == (227, 128)
    assert video.resized_size(128, 300, t) == (128, 300)  # short side == target: returned as is
    assert video.resized_size(300, 128, t) == (300, 128)
    assert video.resized_size(100, 100, t) == (128, 128)
    assert video.resized_size(60, 61, t) == (128, 130)  # int(128 * 61 / 60) = 130.13 -> 130
    for h, w in [(240, 427), (37, 36), (1080, 1920), (36, 45), (29, 33), (480, 640)]:
        assert video.resized_size(h, w, t) == R.resized_size(h, w, t)
    # Python's round: half to even
    assert video.center_crop_offsets(128, 227, 112) == (8, 58)  # (115 / 2 = 57.5 -> 58)
    assert video.center_crop_offsets(37, 36, 32) == (2, 2)  # 2.5 -> 2
    assert video.center_crop_offsets(39, 41, 32) == (4, 4)  # 3.5 -> 4, 4.5 -> 4
    assert video.center_crop_offsets(32, 33, 32) == (0, 0)  # 0.5 -> 0


def _torchvision_draws(rh, rw, S, gen):
    """ColorJitter.get_params((0.75, 1.25) x 3, (-0.1, 0.1)) then RandomCrop.get_params, as torchvision 0.11.2 writes them."""
    fn_idx = torch.randperm(4, generator=gen)
    b = float(torch.empty(1).uniform_(0.75, 1.25, generator=gen))
    c = float(torch.empty(1).uniform_(0.75, 1.25, generator=gen))
    s = float(torch.empty(1).uniform_(0.75, 1.25, generator=gen))
    h = float(torch.empty(1).uniform_(-0.1, 0.1, generator=gen))
    if rh == S and rw == S:
        return fn_idx.tolist(), b, c, s, h, 0, 0
    i = torch.randint(0, rh - S + 1, size=(1,), generator=gen).item()
    j = torch.randint(0, rw - S + 1, size=(1,), generator=gen).item()
    return fn_idx.tolist(), b, c, s, h, i, j


def test_draw_clip_params_reproduces_the_torch_sequence(video):
    sizes = [(240, 427), (37, 36), (128, 171), (480, 270), (36, 36), (100, 90)]
    for S in (112, 32):
        g1, g2 = torch.Generator().manual_seed(99), torch.Generator().manual_seed(99)
        for h, w in sizes * 3:
            rh, rw = video.resized_size(h, w, math.floor(1.15 * S))
            if min(rh, rw) < S:
                continue
            p = video.draw_clip_params(h, w, S, True, g1)
            order, b, c, s, hf, top, left = _torchvision_draws(rh, rw, S, g2)
            assert (p.rh, p.rw, list(p.order), p.brightness, p.contrast, p.saturation, p.hue_factor, p.top, p.left) == \
                (rh, rw, order, b, c, s, hf, top, left)
        assert torch.equal(g1.get_state(), g2.get_state())
    # the default is torch's global RNG, consumed clip after clip
    torch.manual_seed(7)
    ps = [video.draw_clip_params(240, 427, 112, True) for _ in range(3)]
    torch.manual_seed(7)
    g = torch.default_generator
    assert [(list(p.order), p.brightness, p.top, p.left) for p in ps] == [
        (o, b, i, j) for o, b, _, _, _, i, j in (_torchvision_draws(128, 227, 112, g) for _ in range(3))]
    # evaluation draws nothing
    st = torch.get_rng_state()
    p = video.draw_clip_params(240, 427, 112, False)
    assert torch.equal(st, torch.get_rng_state()) and (p.top, p.left, p.train) == (8, 58, False)


def _fixture():
    z = np.load(os.path.join(GOLDEN, "video_prep.npz"))
    meta = json.load(open(os.path.join(GOLDEN, "video_prep_schema.json")))
    return z, meta


def _case_frames(z, case):
    return [z[f"{case['name']}/src{i}"] if stored else R.pattern_clip(case["T"], h, w)
            for i, ((h, w), stored) in enumerate(zip(case["sizes"], case["stored_frames"]))]


def _restated_params(p):
    return dict(rh=p["rh"], rw=p["rw"], top=p["top"], left=p["left"], train=p["train"], order=p.get("order"), b=p.get("b"), c=p.get("c"),
                s=p.get("s"), shift=R.hue_shift(p["hue"]) if p["train"] else 0)


def test_fixture_covers_the_cases_and_equals_the_restatement(video):
    z, meta = _fixture()
    assert meta["pillow"] and "assumed, not checked" in meta["note"]
    seen = {"landscape": False, "portrait": False, "odd": False, "same_short": False, "upscale": False, "one_axis": False, "neg_hue": False}
    contrast_pos = set()
    for case in meta["cases"]:
        S = case["S"]
        frames = _case_frames(z, case)
        crops = z[f"{case['name']}/crops"]
        assert crops.shape == (len(frames), case["T"], S, S, 3)
        for i, (fr, p) in enumerate(zip(frames, case["params"])):
            h, w = fr.shape[1:3]
            seen["landscape"] |= w > h
            seen["portrait"] |= h > w
            seen["odd"] |= bool(h % 2 and w % 2)
            seen["same_short"] |= (p["rh"], p["rw"]) == (h, w)
            seen["upscale"] |= min(p["rh"], p["rw"]) > min(h, w)
            seen["one_axis"] |= (p["rh"] == h) != (p["rw"] == w)
            if p["train"]:
                seen["neg_hue"] |= p["hue"] < 0
                contrast_pos.add(p["order"].index(1))
            if not case["explicit_resize"]:
                assert (p["rh"], p["rw"]) == video.resized_size(h, w, math.floor(1.15 * S))
            assert np.array_equal(R.clip_crops(fr, _restated_params(p), S), crops[i]), (case["name"], i)
        if case["train"] and not case["explicit_resize"]:  # the stored draws are draw_clip_params' under the case's seed
            torch.manual_seed(case["seed"])
            for fr, p in zip(frames, case["params"]):
                q = video.draw_clip_params(fr.shape[1], fr.shape[2], S, True)
                assert (list(q.order), q.brightness, q.contrast, q.saturation, q.hue_factor, q.top, q.left) == \
                    (p["order"], p["b"], p["c"], p["s"], p["hue"], p["top"], p["left"])
    assert all(seen.values()), seen
    assert contrast_pos == {0, 1, 2, 3}
    assert {c["S"] for c in meta["cases"]} == {32, 112}


def _clip(video, **kw):
    d = video.L.VideoClip()
    base = dict(src_offset=0, h=40, w=50, rh=36, rw=45, top=0, left=0, tab_x=0, ksize_x=3, tab_y=0, ksize_y=3, jitter=0)
    base.update(kw)
    for k, v in base.items():
        if k == "order":
            d.order[:] = v
        else:
            setattr(d, k, v)
    return d


def test_cabi_rejects_bad_descriptors_before_touching_hip(video):
    lib = video.L.load()
    S, T = 32, 2
    kx, tx = video.resample_table(50, 45)
    ky, ty = video.resample_table(40, 36)
    tables = np.concatenate([tx, ty]).astype(np.int32)
    good = dict(tab_x=0, ksize_x=kx, tab_y=tx.size, ksize_y=ky)
    frames_bytes = T * 40 * 50 * 3
    lut = np.zeros(256, np.float32)
    ws = lib.stlt_video_prep_workspace_bytes(1, T, tables.size)
    assert ws > 0 and lib.stlt_video_prep_workspace_bytes(0, T, 0) == 0 and lib.stlt_video_prep_workspace_bytes(1, 0, 0) == 0
    fake = 0x1000  # never dereferenced: every case below fails in the host checks

    def call(clip, n_table=tables.size, fb=frames_bytes, ws_bytes=ws, S_=S):
        arr = (video.L.VideoClip * 1)(clip)
        return lib.stlt_video_prep_fwd(fake, fb, arr, tables.ctypes.data, n_table, lut.ctypes.data, 1, T, S_, fake, fake, ws_bytes, None)

    bad = {
        "zero size": _clip(video, **good, h=0),
        "zero resized": _clip(video, **good, rw=0),
        "crop below": _clip(video, **good, top=5),
        "crop right": _clip(video, **good, left=14),
        "negative crop": _clip(video, **good, left=-1),
        "frames past the buffer": _clip(video, **good, src_offset=1),
        "negative offset": _clip(video, **good, src_offset=-8),
        "table past the buffer": _clip(video, **dict(good, tab_y=tx.size + 1)),
        "taps too few": _clip(video, **dict(good, ksize_x=1)),
        "table on a kept axis": _clip(video, **dict(good, tab_x=0), rw=50),
        "no table on a changed axis": _clip(video, **dict(good, tab_x=-1)),
        "table misread": _clip(video, **dict(good, tab_x=tx.size, ksize_x=ky)),
        "order repeats": _clip(video, **good, jitter=1, order=[0, 1, 1, 3], brightness=1.0, contrast=1.0, saturation=1.0),
        "order out of range": _clip(video, **good, jitter=1, order=[0, 1, 2, 4], brightness=1.0, contrast=1.0, saturation=1.0),
        "jitter flag": _clip(video, **good, jitter=2),
        "hue shift": _clip(video, **good, jitter=1, order=[3, 2, 1, 0], brightness=1.0, contrast=1.0, saturation=1.0, hue_shift=256),
        "nan factor": _clip(video, **good, jitter=1, order=[3, 2, 1, 0], brightness=float("nan"), contrast=1.0, saturation=1.0),
    }
    for name, clip in bad.items():
        assert call(clip) == -1, name
        assert lib.stlt_last_error().decode().startswith("stlt_video_prep_fwd"), name
    ok = _clip(video, **good)
    assert call(ok, ws_bytes=ws - 1) == -1  # workspace too small
    assert call(ok, fb=frames_bytes - 1) == -1
    assert call(ok, S_=37) == -1  # crop larger than the resized frame
    assert lib.stlt_video_prep_fwd(fake, frames_bytes, None, tables.ctypes.data, tables.size, lut.ctypes.data, 1, T, S, fake, fake, ws, None) == -1
    arr = (video.L.VideoClip * 1)(ok)
    assert lib.stlt_video_prep_fwd(fake, frames_bytes, arr, tables.ctypes.data, tables.size, lut.ctypes.data, 70000, T, S, fake, fake, ws, None) == -1


def test_collater_contract_errors_on_the_host(video, pkg):
    col = video.DeviceVideoCollater(32, device="cpu")
    a = {"frames": np.zeros((2, 40, 40, 3), np.uint8), "labels": 0, "video_id": "a"}
    b = {"frames": np.zeros((3, 40, 40, 3), np.uint8), "labels": 0, "video_id": "b"}
    with pytest.raises(pkg.StltHipError, match="same number of frames"):
        col([a, b])
    with pytest.raises(pkg.StltHipError, match="uint8"):
        col([{"frames": np.zeros((2, 40, 40, 3), np.float32), "labels": 0, "video_id": "c"}])
