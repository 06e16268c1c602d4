"""The appearance side of the perturbation test restated in plain torch from the words of include/stlt_hip.h (stlt_perturb_rank_cells,
stlt_perturb_apply_cells, stlt_cell_pool_abs) and of collate.perturb_cells: loops over clips, steps and cells, a stable sort, float64 sums,
no package import, no GPU.  tools/gen_golden_fusion_perturbation.py builds the fixtures with it, tests/test_fusion_perturbation_cpu.py
holds collate.perturb_cells' torch form to it and tests/test_fusion_perturbation_gpu.py the kernels."""
import torch

ORDERS = ("descending", "ascending")
VIDEO_CELL = (16, 32, 32)  # the R3D-50 trunk's total stride along (T, H, W)


def grid(shape, cell):
    """(Gt, Gh, Gw) of a (T, H, W) volume cut into cells of (ct, ch, cw): every axis rounds up"""
    return tuple(-(-n // c) for n, c in zip(shape, cell))


def cell_box(c, shape, cell):
    """cell c = (gt*Gh + gh)*Gw + gw -> the slices of frames, rows and columns it covers (clipped to the volume)"""
    _, Gh, Gw = grid(shape, cell)
    gt, gh, gw = c // (Gh * Gw), (c // Gw) % Gh, c % Gw
    return tuple(slice(g * e, min(g * e + e, n)) for g, e, n in zip((gt, gh, gw), cell, shape))


def rank_cells(scores, descending=True):
    """scores (B,C) -> (rank (B,C) int32: the position of every cell in the removal order; n_candidates (B,) int32 = C).  By score as
    float32 values with -0 == +0, descending or ascending; ties to the lower index; NaN last in both orders."""
    scores = torch.as_tensor(scores, dtype=torch.float32)
    B, C = scores.shape
    rank = torch.empty(B, C, dtype=torch.int32)
    for b in range(B):
        v = scores[b].double()
        nan = torch.isnan(v)
        v = torch.where(nan | (v == 0), torch.zeros((), dtype=torch.float64), -v if descending else v)
        order = torch.sort(v, stable=True).indices
        order = order[torch.sort(nan[order].to(torch.int8), stable=True).indices]
        rank[b, order] = torch.arange(C, dtype=torch.int32)
    return rank, torch.full((B,), C, dtype=torch.int32)


def removal_counts(n_candidates, steps, s0, s1):
    """(s1-s0+1, B) int32: k = floor(s * n_candidates[b] / steps), in Python integers"""
    return torch.tensor([[(s * int(n)) // steps for n in n_candidates] for s in range(s0, s1 + 1)], dtype=torch.int32)


def cell_masks(rank, n_candidates, steps, s0, s1, shape, cell):
    """(s1-s0+1, B, T, H, W) bool: the positions deleted at every step, and the removal counts"""
    counts = removal_counts(n_candidates, steps, s0, s1)
    n, B = counts.shape
    mask = torch.zeros((n, B) + tuple(shape), dtype=torch.bool)
    for i in range(n):
        for b in range(B):
            for c in range(rank.shape[1]):
                if 0 <= int(rank[b, c]) < int(counts[i, b]):
                    mask[(i, b) + cell_box(c, shape, cell)] = True
    return mask, counts


def apply_cells(x, cell, rank, n_candidates, steps, s0, s1, fill=0.0):
    """x (B,Cch,T,H,W) float32 -> (out ((s1-s0+1)*B, Cch,T,H,W), step-major; removed (s1-s0+1, B) int32).  Deleted positions hold `fill`,
    every other element its input bits."""
    assert steps >= 1 and 0 <= s0 <= s1 <= steps
    shape = tuple(x.shape[2:])
    assert rank.shape[1] == grid(shape, cell)[0] * grid(shape, cell)[1] * grid(shape, cell)[2]
    mask, counts = cell_masks(rank, n_candidates, steps, s0, s1, shape, cell)
    n, B = counts.shape
    out = x.unsqueeze(0).repeat(n, 1, 1, 1, 1, 1).view(torch.int32)  # moved as the integers the floats are stored as
    fill_bits = torch.tensor(float(fill), dtype=torch.float32).view(torch.int32)
    out = torch.where(mask[:, :, None], fill_bits, out).view(torch.float32)
    return out.reshape((n * B,) + tuple(x.shape[1:])).contiguous(), counts


def cell_pool_abs(g, cell):
    """g (B,Cch,T,H,W) -> (B,C) float64: the sum of |g| over every cell and all channels"""
    shape = tuple(g.shape[2:])
    Gt, Gh, Gw = grid(shape, cell)
    out = torch.zeros(g.shape[0], Gt * Gh * Gw, dtype=torch.float64)
    for c in range(out.shape[1]):
        st, sh, sw = cell_box(c, shape, cell)
        out[:, c] = g[:, :, st, sh, sw].double().abs().sum(dim=(1, 2, 3, 4))
    return out


def perturb_cells(batch, scores, steps=10, order="descending", step_range=None, fill=0.0):
    """collate.perturb_cells restated: video_frames (cells of VIDEO_CELL), else appearance_features (cells of 1 x 1 x 1); a (B,C+1)
    score tensor loses its first column; every other per-clip entry is tiled."""
    key, cell = ("video_frames", VIDEO_CELL) if "video_frames" in batch else ("appearance_features", (1, 1, 1))
    x = batch[key]
    B = x.shape[0]
    Gt, Gh, Gw = grid(tuple(x.shape[2:]), cell)
    if scores.shape[1] == Gt * Gh * Gw + 1:
        scores = scores[:, 1:]
    s0, s1 = (0, steps) if step_range is None else step_range
    rank, n_cand = rank_cells(scores, order == "descending")
    new, removed = apply_cells(x, cell, rank, n_cand, steps, s0, s1, fill)
    n = s1 - s0 + 1
    out = {}
    for k, v in batch.items():
        if k == key:
            out[k] = new
        elif isinstance(v, torch.Tensor) and v.dim() >= 1 and v.shape[0] == B:
            out[k] = torch.cat([v] * n, dim=0)
        elif isinstance(v, (list, tuple)) and len(v) == B:
            out[k] = type(v)(list(v) * n)
        else:
            out[k] = v
    out["removed"], out["n_candidates"] = removed, n_cand
    return out


def special_scores(B, C, seed):
    """(B,C) scores on a grid of halves (blocks of ties) with both zeros, both infinities and NaN; clip 0 all equal"""
    g = torch.Generator().manual_seed(seed)
    s = torch.round(torch.randn(B, C, generator=g) * 2) / 2
    pick = torch.rand(B, C, generator=g)
    for lo, v in ((0.0, -0.0), (0.08, 0.0), (0.16, float("inf")), (0.22, float("-inf")), (0.28, float("nan"))):
        s[(pick >= lo) & (pick < lo + 0.07)] = v
    s[0] = 0.75
    return s
