"""Device-side counterpart of the reference's ``StltCollater`` (src/modelling/datasets.py:239-288).

``DeviceCollater(dataset_name, device)(samples)`` takes the list of per-video dicts that ``StltDataset.__getitem__``
produces (datasets.py:52-125: ``categories (T_i,N)``, ``boxes (T_i,N,4)``, ``scores (T_i,N)``, ``frame_types (T_i)``,
``lengths``, ``labels``, ``video_id``) and returns the collated batch ON THE GPU with the reference's keys.  The ragged
per-video tensors are concatenated once, copied once per field, and one HIP kernel writes the padded tensors and both
key-padding masks (instead of five ``pad_sequence`` loops plus seven host-to-device copies of padded data).
"""
from __future__ import annotations

from typing import Dict, List

import torch

from . import _lib as L
from . import ops
from .synth import DATASETS


class DeviceCollater:
    def __init__(self, dataset_name: str = "something", device="cuda"):
        self.dataset_name = dataset_name
        self.cls_id = DATASETS[dataset_name]["cls"]  # category2id["cls"] (src/modelling/configs.py:40-78)
        self.device = torch.device(device)

    def __call__(self, samples: List[Dict[str, torch.Tensor]]) -> Dict[str, object]:
        lib = L.load()
        dev = self.device
        B = len(samples)
        lens = [int(s["categories"].shape[0]) for s in samples]
        T, N = max(lens), int(samples[0]["categories"].shape[1])
        off = torch.zeros(B + 1, dtype=torch.int64)
        off[1:] = torch.cumsum(torch.tensor(lens, dtype=torch.int64), 0)
        cat_r = torch.cat([s["categories"].to(torch.int64) for s in samples]).contiguous().to(dev, non_blocking=True)
        box_r = torch.cat([s["boxes"].to(torch.float32) for s in samples]).contiguous().to(dev, non_blocking=True)
        ft_r = torch.cat([s["frame_types"].to(torch.int64) for s in samples]).contiguous().to(dev, non_blocking=True)
        keep_scores = self.dataset_name == "action_genome"  # datasets.py:253-260
        sc_r = (torch.cat([s["scores"].to(torch.float32) for s in samples]).contiguous().to(dev, non_blocking=True)
                if keep_scores else None)
        off_d = off.to(dev, non_blocking=True)
        out = {
            "categories": torch.empty(B, T, N, dtype=torch.int64, device=dev),
            "boxes": torch.empty(B, T, N, 4, dtype=torch.float32, device=dev),
            "frame_types": torch.empty(B, T, dtype=torch.int64, device=dev),
            "src_key_padding_mask_boxes": torch.empty(B, T, N, dtype=torch.bool, device=dev),
            "src_key_padding_mask_frames": torch.empty(B, T, dtype=torch.bool, device=dev),
        }
        if keep_scores:
            out["scores"] = torch.empty(B, T, N, dtype=torch.float32, device=dev)
        with torch.cuda.device(dev):
            L.check(lib.stlt_collate_fwd(cat_r.data_ptr(), box_r.data_ptr(), ops._p(sc_r), ft_r.data_ptr(), off_d.data_ptr(), B, T, N,
                                         self.cls_id, out["categories"].data_ptr(), out["boxes"].data_ptr(),
                                         ops._p(out.get("scores")), out["frame_types"].data_ptr(),
                                         out["src_key_padding_mask_boxes"].data_ptr(),
                                         out["src_key_padding_mask_frames"].data_ptr(),
                                         torch.cuda.current_stream().cuda_stream), "stlt_collate_fwd")
        out["lengths"] = torch.stack([torch.as_tensor(s["lengths"]) for s in samples]).to(torch.int64).to(dev)
        out["labels"] = torch.stack([torch.as_tensor(s["labels"]) for s in samples]).to(dev)
        out["video_id"] = [s.get("video_id") for s in samples]
        return out


def real_counts(batch, round_up_to: int = 1) -> dict:
    """{"num_real_tokens", "num_real_frames"} of a collated batch, counted from its masks (on whatever device they live: call it on the host
    side of the loader, where the masks are made — reference datasets.py:274-286): frames = zeros of src_key_padding_mask_frames, tokens =
    zeros of src_key_padding_mask_boxes inside those frames.  Added to the batch as host integers they let a skip-padding forward / training
    step run without reading its row counts back (include/stlt_hip.h: stlt_inputs.n_real_tokens / n_real_frames).  round_up_to > 1 rounds both
    up to a multiple (capped at the padded sizes): upper bounds, which the inference calls accept."""
    real = ~batch["src_key_padding_mask_frames"].bool()
    tokens = int(((~batch["src_key_padding_mask_boxes"].bool()) & real[:, :, None]).sum())
    frames = int(real.sum())
    if round_up_to > 1:  # inference only: upper bounds are enough, so one captured hipGraph (or one launch plan) serves a bucket of batches
        B, T, N = batch["src_key_padding_mask_boxes"].shape
        up = lambda v, cap: min(cap, (v + round_up_to - 1) // round_up_to * round_up_to)  # noqa: E731
        tokens, frames = up(tokens, B * T * N), up(frames, B * T)
    return {"num_real_tokens": tokens, "num_real_frames": frames}


_PREFIX_KEYS = ("categories", "boxes", "scores", "frame_types", "src_key_padding_mask_boxes", "src_key_padding_mask_frames")


def prefix_batch(batch: Dict[str, torch.Tensor], t: int) -> Dict[str, object]:
    """The collated batch after `t` observed frames: frames 0 .. t-1 of every clip followed by the clip's own extract frame (the frame at
    index lengths[b]-1, which the dataset appends behind the sampled frames, reference datasets.py:97-113), lengths = t+1.  `t = 0` is the
    extract frame alone; for a clip with lengths[b]-1 == t it is the clip itself, cut to t+1 columns.  Clips shorter than that carry
    their padding in front of the extract frame: they have no such prefix (`Stlt.forward_prefixes` marks them invalid).  Works on CPU
    and device tensors; `scores` is carried when present, other entries (labels, video_id) are passed through."""
    cats = batch["categories"]
    B, T = cats.shape[0], cats.shape[1]
    if not 0 <= t < T:
        raise ValueError(f"prefix length {t} outside [0, {T})")
    lengths = batch["lengths"]
    rows = torch.arange(B, device=lengths.device)
    ext = (lengths - 1).clamp(0, T - 1)
    out = dict(batch)
    for k in _PREFIX_KEYS:
        if k in batch:
            v = batch[k]
            out[k] = torch.cat([v[:, :t], v[rows.to(v.device), ext.to(v.device)].unsqueeze(1)], dim=1).contiguous()
    out["lengths"] = torch.full_like(lengths, t + 1)
    out.pop("num_real_tokens", None)  # counted for the whole clips
    out.pop("num_real_frames", None)
    return out



def _perturb_args(order: str, unit: str) -> bool:
    if order not in ("descending", "ascending"):
        raise L.StltHipError(f"order: expected 'descending' or 'ascending', got {order!r}")
    if unit not in ("object", "frame"):
        raise L.StltHipError(f"unit: expected 'object' or 'frame', got {unit!r}")
    return order == "descending"


def _step_range(steps, step_range=None, who: str = ""):
    """`steps` >= 1 and the steps `step_range` = (s0, s1) asks for (default: all of 0 .. steps) -> (steps, s0, s1); `who` names the call
    in front of the message.  Every perturbation call takes its `steps` check from here."""
    steps = int(steps)
    if steps < 1:
        raise L.StltHipError(f"{who + ': ' if who else ''}steps must be >= 1, got {steps}")
    s0, s1 = (0, steps) if step_range is None else (int(step_range[0]), int(step_range[1]))
    if not 0 <= s0 <= s1 <= steps:
        raise L.StltHipError(f"step_range: expected 0 <= s0 <= s1 <= steps = {steps}, got ({s0}, {s1})")
    return steps, s0, s1


def _tile_rest(batch, replaced, B: int, n: int) -> Dict[str, object]:
    """Every entry of `batch` whose key is not in `replaced`, for n * B clips: per-clip entries (a tensor or a list whose leading extent is
    B) tiled n times, num_real_tokens / num_real_frames multiplied by n, anything else as it is."""
    out = {}
    for key, v in batch.items():
        if key in replaced:
            continue
        if key in ("num_real_tokens", "num_real_frames"):
            out[key] = int(v) * n
        elif isinstance(v, torch.Tensor) and v.dim() >= 1 and v.shape[0] == B:
            out[key] = v.repeat((n,) + (1,) * (v.dim() - 1))
        elif isinstance(v, (list, tuple)) and len(v) == B:
            out[key] = type(v)(list(v) * n)
        else:
            out[key] = v
    return out


def perturb_rank(scores: torch.Tensor, kpm_boxes: torch.Tensor, lengths: torch.Tensor, unit: str = "object", order: str = "descending"):
    """The removal order of the perturbation test (include/stlt_hip.h: stlt_perturb_rank) -> (rank int32 of scores' shape, n_candidates (B,)
    int32).  Candidates of clip b: the object slots (t, n) with t < lengths[b]-1, n >= 1 and mask False (unit "object": scores (B,T,N)), or
    the frames t < lengths[b]-1 holding one (unit "frame": scores (B,T)).  rank = position in the removal order — by score, descending or
    ascending, -0 == +0, ties to the lower flat index, NaN last in both orders — and -1 for everything that is no candidate.  Device tensors
    go through the kernel; CPU tensors take the torch form below, same integers."""
    descending = _perturb_args(order, unit)
    B, T, N = kpm_boxes.shape
    want = (B, T, N) if unit == "object" else (B, T)
    if tuple(scores.shape) != want:
        raise L.StltHipError(f"scores: unit {unit!r} takes {want}, got {tuple(scores.shape)}")
    max_slots = L.load().stlt_perturb_max_items()  # a clip's T*N slots are sorted inside one workgroup's LDS; the torch form keeps the same domain
    if T * N > max_slots:
        raise L.StltHipError(f"T*N = {T * N} slots exceed the {max_slots} a clip is ranked with (STLT_EINVAL)")
    if scores.is_cuda:
        return ops.perturb_rank(scores.to(torch.float32).contiguous(), kpm_boxes, lengths, unit, descending)
    t_idx = torch.arange(T)[None, :, None]
    cand = (t_idx < (lengths.to(torch.int64) - 1)[:, None, None]) & (torch.arange(N)[None, None, :] >= 1) & ~kpm_boxes.bool()
    cand = (cand if unit == "object" else cand.any(dim=2)).reshape(B, -1)
    rank, n_cand = _rank_torch(scores.reshape(B, -1), cand, descending)
    return rank.reshape(want), n_cand


def _rank_torch(scores: torch.Tensor, cand: torch.Tensor, descending: bool):
    """The torch form of the rank kernels on CPU tensors: scores, cand (B,M) -> (rank (B,M) int32, n_candidates (B,) int32)"""
    B = scores.shape[0]
    v = scores.to(torch.float32).double()
    nan = torch.isnan(v)
    v = torch.where(nan | (v == 0), torch.zeros_like(v), -v if descending else v)  # canonical: -0 == +0; NaN sorted below
    order_ = torch.sort(v, dim=1, stable=True).indices
    for flag in (nan, ~cand):  # stable partitions: NaN behind the numbers, non-candidates behind the candidates
        order_ = order_.gather(1, torch.sort(flag.gather(1, order_).to(torch.int8), dim=1, stable=True).indices)
    n_cand = cand.sum(dim=1)
    pos = torch.arange(v.shape[1])[None, :].expand(B, -1)
    rank = torch.empty(B, v.shape[1], dtype=torch.int64).scatter_(1, order_, torch.where(pos < n_cand[:, None], pos, torch.full_like(pos, -1)))
    return rank.to(torch.int32), n_cand.to(torch.int32)


def perturb_batch(batch: Dict[str, torch.Tensor], scores: torch.Tensor, steps: int = 10, order: str = "descending", unit: str = "object", step_range=None,
                  dataset_name: str = "something") -> Dict[str, object]:
    """The batches of the perturbation test (Chefer, Gur, Wolf 2021): `batch` with the first k candidates of the removal order deleted, for
    every step s of `step_range` = (s0, s1) (default: all of 0 .. steps), k = floor(s * n_candidates[b] / steps).  The result holds
    (s1-s0+1)*B clips, step-major: clip (s-s0)*B + b is clip b at step s.  A deleted slot is what the reference's dataset and collater make
    of a slot without a detection (datasets.py:88-93, 274-278): category 0, box (0,0,0,0), score 0, mask True; a frame that had an object
    and has none left gets the dataset's frame type "empty" (datasets.py:64-69).  Everything else is copied; slots are not compacted.
    Step 0 is the batch itself, step `steps` has no candidate left.  Also returned: "removed" (s1-s0+1, B) int32 — k per step and clip — and
    "n_candidates" (B,) int32.  Other per-clip entries (labels, video_id, any tensor or list whose leading extent is B) are tiled to the new
    clip count; num_real_tokens / num_real_frames, when present, are multiplied by the number of steps written (upper bounds, which the
    inference calls accept).  Device tensors go through stlt_perturb_rank / stlt_perturb_apply; CPU tensors take the torch form, same bits."""
    _perturb_args(order, unit)
    steps, s0, s1 = _step_range(steps, step_range)
    empty_type = DATASETS[dataset_name]["empty"]  # frame2type["empty"] (src/modelling/configs.py:40-78)
    cats = batch["categories"]
    B, T, N = cats.shape
    n = s1 - s0 + 1
    rank, n_cand = perturb_rank(scores, batch["src_key_padding_mask_boxes"], batch["lengths"], unit, order)
    if cats.is_cuda:
        core = {k: batch[k] for k, _, _ in ops.PERTURB_KEYS if k in batch}
        for k in ("categories", "frame_types", "lengths"):
            core[k] = core[k].to(torch.int64).contiguous()
        core["boxes"] = core["boxes"].to(torch.float32).contiguous()
        if "scores" in core:
            core["scores"] = core["scores"].to(torch.float32).contiguous()
        new = ops.perturb_apply(core, rank, n_cand, steps, s0, s1, empty_type)
        removed = new.pop("removed")[s0:s1 + 1]
    else:
        k = (torch.arange(s0, s1 + 1, dtype=torch.int64)[:, None] * n_cand.to(torch.int64)[None, :]) // steps  # (n, B)
        kpm = batch["src_key_padding_mask_boxes"]
        slot_rank = rank if unit == "object" else torch.where((torch.arange(N)[None, None, :] >= 1) & ~kpm.bool(), rank[:, :, None], torch.full((), -1, dtype=torch.int32))
        slot_rank = slot_rank.to(torch.int64)
        gone = (slot_rank[None] >= 0) & (slot_rank[None] < k[:, :, None, None])      # (n, B, T, N)
        had = (slot_rank >= 0).any(dim=2)                                            # (B, T)
        left = ((slot_rank[None] >= 0) & ~gone).any(dim=3)                           # (n, B, T)
        tile = lambda t: t.unsqueeze(0).expand(n, *t.shape)  # noqa: E731
        new = {"categories": torch.where(gone, torch.zeros((), dtype=cats.dtype), tile(cats)),
               "boxes": torch.where(gone[..., None], torch.zeros((), dtype=batch["boxes"].dtype), tile(batch["boxes"])),
               "src_key_padding_mask_boxes": torch.where(gone, torch.ones((), dtype=kpm.dtype), tile(kpm)),
               "frame_types": torch.where(had[None] & ~left, torch.full((), empty_type, dtype=batch["frame_types"].dtype), tile(batch["frame_types"])),
               "src_key_padding_mask_frames": tile(batch["src_key_padding_mask_frames"]), "lengths": tile(batch["lengths"])}
        if "scores" in batch:
            new["scores"] = torch.where(gone, torch.zeros((), dtype=batch["scores"].dtype), tile(batch["scores"]))
        new = {key: v.reshape(n * B, *v.shape[2:]).contiguous() for key, v in new.items()}
        removed = k.to(torch.int32)
    out = _tile_rest(batch, new, B, n)
    out.update(new)
    out["removed"], out["n_candidates"] = removed, n_cand
    return out


VIDEO_CELL = (16, 32, 32)  # the R3D-50 trunk's total stride in (T, H, W): stem (1,2,2), max-pool 2, three stride-2 stages


def appearance_cells(batch: Dict[str, torch.Tensor]):
    """What the appearance side of the perturbation test deletes in `batch` -> (key, cell extents (ct,ch,cw), grid (Gt,Gh,Gw)).
    `video_frames` (B,3,T,H,W): the stride block of one appearance token, VIDEO_CELL, on the grid the trunk's own plan gives for this video
    (modelling.resnet3d: the extents of its feature map) — a video for which the blocks and the plan disagree is refused.  Without
    `video_frames`, `appearance_features` (B,Cf,Gt,Gh,Gw): the feature column, (1,1,1)."""
    from .modelling.resnet3d import _trunk_out
    if "video_frames" in batch:
        v = batch["video_frames"]
        if v.dim() != 5:
            raise L.StltHipError(f"video_frames must be (B, 3, T, H, W), got {tuple(v.shape)}")
        _, _, T, H, W = v.shape
        ct, ch, cw = VIDEO_CELL
        grid = (-(-T // ct), -(-H // ch), -(-W // cw))
        plan = (_trunk_out(T), _trunk_out(H, 2), _trunk_out(W, 2))
        if grid != plan:
            raise L.StltHipError(f"video_frames {tuple(v.shape)}: the cells {VIDEO_CELL} give the grid {grid}, the trunk's plan {plan} tokens")
        return "video_frames", VIDEO_CELL, grid
    if "appearance_features" in batch:
        f = batch["appearance_features"]
        if f.dim() != 5:
            raise L.StltHipError(f"appearance_features must be (B, Cf, Gt, Gh, Gw), got {tuple(f.shape)}")
        return "appearance_features", (1, 1, 1), tuple(f.shape[2:])
    raise L.StltHipError("the batch needs `video_frames` or `appearance_features`")


def cell_scores(scores: torch.Tensor, B: int, n_cells: int) -> torch.Tensor:
    """`scores` of an appearance call as (B,C) float32: (B,C) cell scores as they are, (B,C+1) token scores without the CLS column"""
    if not isinstance(scores, torch.Tensor) or scores.dim() != 2 or scores.shape[0] != B or scores.shape[1] not in (n_cells, n_cells + 1):
        raise L.StltHipError(f"scores: the appearance side takes ({B},{n_cells}) cell scores or ({B},{n_cells + 1}) token scores (CLS first), "
                             f"got {tuple(scores.shape) if isinstance(scores, torch.Tensor) else type(scores)}")
    if scores.shape[1] == n_cells + 1:
        scores = scores[:, 1:]
    return scores.to(torch.float32).contiguous()


def perturb_rank_cells(scores: torch.Tensor, order: str = "descending"):
    """The removal order of video cells or feature columns (include/stlt_hip.h: stlt_perturb_rank_cells): scores (B,C), every cell a
    candidate -> (rank (B,C) int32, n_candidates (B,) int32 = C), by perturb_rank's order rule.  Device tensors go through the kernel; CPU
    tensors take the torch form, same integers."""
    descending = _perturb_args(order, "object")
    if scores.dim() != 2 or scores.shape[1] < 1:
        raise L.StltHipError(f"scores: expected (B,C) with C >= 1, got {tuple(scores.shape)}")
    max_items = L.load().stlt_perturb_max_items()
    if scores.shape[1] > max_items:
        raise L.StltHipError(f"C = {scores.shape[1]} cells exceed the {max_items} a clip is ranked with (STLT_EINVAL)")
    if scores.is_cuda:
        return ops.perturb_rank_cells(scores.to(torch.float32).contiguous(), descending)
    return _rank_torch(scores, torch.ones(scores.shape, dtype=torch.bool), descending)


def cell_index(shape, cell) -> torch.Tensor:
    """(T,H,W) int64: the flat cell index of every position of a (T,H,W) volume cut into cells of (ct,ch,cw)"""
    (T, H, W), (ct, ch, cw) = shape, cell
    Gh, Gw = -(-H // ch), -(-W // cw)
    return ((torch.arange(T) // ct)[:, None, None] * Gh + (torch.arange(H) // ch)[None, :, None]) * Gw + (torch.arange(W) // cw)[None, None, :]


def perturb_cells(batch: Dict[str, torch.Tensor], scores: torch.Tensor, steps: int = 10, order: str = "descending", step_range=None,
                  fill: float = 0.0) -> Dict[str, object]:
    """The appearance counterpart of perturb_batch: `batch` with the first k cells of the removal order deleted from `video_frames` — or
    from `appearance_features` when the batch has no `video_frames` — for every step s of `step_range` = (s0, s1) (default: all of
    0 .. steps), k = floor(s * C / steps).  A cell (appearance_cells) is the stride block of one appearance token: frames
    [16 gt, 16 gt+16), rows [32 gh, 32 gh+32), columns [32 gw, 32 gw+32), clipped to the video, all channels; it is the block the trunk's
    strides map onto token 1 + (gt*Gh + gh)*Gw + gw, not the token's receptive field.  Deleting it sets its pixels to `fill` (0.0:
    mid-grey after the reference's Normalize(0.5, 0.5), datasets.py:151); the reference's appearance encoder takes no key-padding mask
    (models.py:269), so a token cannot be masked instead.  On `appearance_features` the cell is the feature column: a weaker test — the
    feature of a grey block is not `fill` — and the one there is when no trunk is loaded.  `scores`: (B,C) cell scores or (B,C+1) token
    scores, CLS first (dropped).  The result holds (s1-s0+1)*B clips, step-major; every other per-clip entry, the layout tensors among
    them, is tiled as perturb_batch tiles it.  Also returned: "removed" (s1-s0+1, B) int32 and "n_candidates" (B,) int32.  Device tensors
    go through stlt_perturb_rank_cells / stlt_perturb_apply_cells; CPU tensors take the torch form, same bits."""
    _perturb_args(order, "object")
    steps, s0, s1 = _step_range(steps, step_range)
    key, cell, grid = appearance_cells(batch)
    x = batch[key]
    B = x.shape[0]
    n = s1 - s0 + 1
    rank, n_cand = perturb_rank_cells(cell_scores(scores, B, grid[0] * grid[1] * grid[2]), order)
    if x.is_cuda:
        new, removed = ops.perturb_apply_cells(x.to(torch.float32).contiguous(), cell, rank, n_cand, steps, s0, s1, fill)
    else:
        k = (torch.arange(s0, s1 + 1, dtype=torch.int64)[:, None] * n_cand.to(torch.int64)[None, :]) // steps  # (n, B)
        gone = (rank.to(torch.int64)[None] >= 0) & (rank.to(torch.int64)[None] < k[:, :, None])  # (n, B, C)
        mask = gone[:, :, cell_index(tuple(x.shape[2:]), cell)]  # (n, B, T, H, W)
        new = torch.where(mask[:, :, None], torch.full((), float(fill), dtype=x.dtype), x[None]).reshape(n * B, *x.shape[1:]).contiguous()
        removed = k.to(torch.int32)
    rest = _tile_rest(batch, (key,), B, n)
    out = {name: new if name == key else rest[name] for name in batch}  # the batch's own key order
    out["removed"], out["n_candidates"] = removed, n_cand
    return out
