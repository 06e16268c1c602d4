"""Integrated gradients on the GPU.  Op level: stlt_ig_path, stlt_ig_path_dense, stlt_ig_reduce, stlt_ig_delta and stlt_cell_pool_sum inside
guard bands, three ways, with offset pointers, bit for bit against tests/ig_restated.py (delta and the signed pool: against float64 within
the worst case of a float32 sum).  End to end: Stlt.forward_integrated_gradients against the fp64 oracle's IG on the same quadrature, the
bit-for-bit composition of every model's call from the public pieces, the runner, the refusals."""
import ctypes
import sys

import numpy as np
import pytest
import torch

import guard_arena as GA
import ig_cases as IC
import ig_restated as R
from guard_arena import Out

pytestmark = pytest.mark.gpu
DEV = "cuda"
EINVAL = -1
STEPS = 5
RANGES = [(0, 5), (0, 0), (2, 3), (5, 5)]


def _report(what, value):
    print(f"\n[integrated gradients] {what}: {value}", file=sys.stderr)


@pytest.fixture(scope="module")
def arena():
    return GA.Arena(24 << 20)


def _same_bits(got: torch.Tensor, want: np.ndarray, what):
    g = got.cpu().contiguous().numpy()
    assert g.shape == want.shape and g.dtype == want.dtype, (what, g.shape, want.shape, g.dtype, want.dtype)
    assert g.tobytes() == want.tobytes(), f"{what}: {int((g.view(np.uint8) != want.view(np.uint8)).sum())} bytes differ"


# ---------------------------------------------------------------------------------------------------------------- 1. stlt_ig_path
def _layout():
    """B = T = N = 3: 27 scores, an odd count; clip 1 has a padded last frame, clip 0 a padded slot"""
    B, T, N = 3, 3, 3
    g = torch.Generator().manual_seed(11)
    b = {"categories": torch.randint(1, 5, (B, T, N), generator=g), "boxes": torch.rand(B, T, N, 4, generator=g), "scores": torch.rand(B, T, N, generator=g),
         "src_key_padding_mask_boxes": torch.zeros(B, T, N, dtype=torch.uint8), "frame_types": torch.randint(1, 4, (B, T), generator=g),
         "src_key_padding_mask_frames": torch.zeros(B, T, dtype=torch.uint8), "lengths": torch.tensor([3, 2, 3])}
    b["src_key_padding_mask_frames"][1, 2] = 1
    b["src_key_padding_mask_boxes"][1, 2, :] = 1
    b["src_key_padding_mask_boxes"][0, 1, 2] = 1
    b["categories"][b["src_key_padding_mask_boxes"].bool()] = 0
    b["boxes"][0, 0, 0, 0] = -0.0
    base = {"boxes": torch.rand(B, T, N, 4, generator=g), "scores": torch.rand(B, T, N, generator=g)}
    return b, base


_ABI = {"src_key_padding_mask_boxes": "kpm_boxes", "src_key_padding_mask_frames": "kpm_frames"}
_ROLES = {"categories": ("index", 0), "boxes": ("in",), "scores": ("in",), "src_key_padding_mask_boxes": ("extent", 1), "frame_types": ("index", 0),
          "src_key_padding_mask_frames": ("extent", 1), "lengths": ("extent", 1)}
_PATH_MISALIGN = {"boxes": 4, "scores": 12, "boxes0": 8, "o_boxes": 12, "o_scores": 4, "categories": 8, "o_categories": 8, "src_key_padding_mask_boxes": 1,
                  "o_src_key_padding_mask_boxes": 3, "o_src_key_padding_mask_frames": 1, "o_lengths": 8}


@pytest.mark.parametrize("given", [False, True], ids=["zero-baseline", "baseline"])
@pytest.mark.parametrize("with_scores", [False, True], ids=["boxes", "boxes+scores"])
@pytest.mark.parametrize("s0,s1", RANGES)
def test_ig_path_is_the_restated_path_inside_guard_bands(pkg, arena, s0, s1, with_scores, given):
    lib = pkg._lib.load()
    b, base = _layout()
    if not with_scores:
        del b["scores"]
    B, T, N = b["categories"].shape
    n = s1 - s0 + 1
    specs = {k: (v, *_ROLES[k]) for k, v in b.items()}
    specs.update({"o_" + k: (Out((n * B,) + tuple(v.shape[1:]), v.dtype), "out") for k, v in b.items()})
    if given:
        specs["boxes0"] = (base["boxes"], "in")
        if with_scores:
            specs["scores0"] = (base["scores"], "in")

    def call(o):
        inp = pkg._lib.Inputs()
        inp.B, inp.T, inp.N = B, T, N
        for k in b:
            setattr(inp, _ABI.get(k, k), getattr(o, k).ptr)
        sc = o.o_scores.ptr if with_scores else None
        return lib.stlt_ig_path(ctypes.byref(inp), o.boxes0.ptr if given else None, o.scores0.ptr if given and with_scores else None, STEPS, s0, s1, o.o_categories.ptr,
                                o.o_boxes.ptr, sc, o.o_src_key_padding_mask_boxes.ptr, o.o_frame_types.ptr, o.o_src_key_padding_mask_frames.ptr, o.o_lengths.ptr, GA.stream())

    outs = ["o_" + k for k in b]
    want = R.path_layout({k: v.numpy() for k, v in b.items()}, STEPS, s0, s1, base["boxes"].numpy() if given else None, base["scores"].numpy() if given else None)
    for mis in (None, {k: v for k, v in _PATH_MISALIGN.items() if k in specs}):
        got = GA.three_ways(lib, arena, specs, call, outs, misalign=mis)
        for k in b:
            _same_bits(got["o_" + k], want[k], f"{k} steps [{s0},{s1}]")
    if s0 == 0:  # step 0 is the baseline's bits, step `steps` the input's
        first = got["o_boxes"][:B]
        assert torch.equal(first.view(torch.int32), (base["boxes"] if given else torch.zeros_like(b["boxes"])).view(torch.int32))
    if s1 == STEPS:
        assert torch.equal(got["o_boxes"][-B:].view(torch.int32), b["boxes"].view(torch.int32))


# ------------------------------------------------------------------------------------------------ 2. stlt_ig_path_dense, stlt_ig_reduce
DENSE_SHAPES = [(1, 1, 1, 1, 1), (2, 3, 2, 5, 5), (1, 3, 4, 32, 32)]  # one element; 150 per clip: clip starts are not 16-byte aligned; a vector body
DENSE_MISALIGN = [None, {"x": 4, "x0": 4, "out": 4}, {"x": 4, "x0": 8, "out": 12}, {"x": 8, "x0": 8, "out": 8}]  # aligned; a head of 3; scalar; a head of 2


def _dense(shape, seed=21):
    g = torch.Generator().manual_seed(seed)
    x, x0 = torch.randn(shape, generator=g), torch.randn(shape, generator=g)
    x.view(-1)[0] = -0.0
    return x, x0


@pytest.mark.parametrize("given", [False, True], ids=["fill", "baseline"])
@pytest.mark.parametrize("shape", DENSE_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_ig_path_dense_is_the_restated_path_inside_guard_bands(pkg, arena, shape, given):
    lib = pkg._lib.load()
    x, x0 = _dense(shape)
    B, n = shape[0], x[0].numel()
    fill = 0.25
    for s0, s1 in RANGES:
        cnt = s1 - s0 + 1
        specs = {"x": (x, "in"), "out": (Out((cnt * B,) + tuple(shape[1:])), "out")}
        if given:
            specs["x0"] = (x0, "in")
        call = lambda o: lib.stlt_ig_path_dense(o.x.ptr, o.x0.ptr if given else None, fill, B, n, STEPS, s0, s1, o.out.ptr, GA.stream())  # noqa: E731
        want = R.path_dense(x.numpy(), x0.numpy() if given else fill, STEPS, s0, s1)
        for mis in DENSE_MISALIGN:
            mis = None if mis is None else {k: v for k, v in mis.items() if k in specs}
            got = GA.three_ways(lib, arena, specs, call, ["out"], misalign=mis)
            _same_bits(got["out"], want, f"{shape} steps [{s0},{s1}] misalign {mis}")
    if given:
        assert torch.equal(got["out"].view(torch.int32), x.view(torch.int32))  # the last range is (5,5): the input's bits


@pytest.mark.parametrize("shape", DENSE_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_ig_reduce_is_the_restated_quadrature_and_splits_bitwise(pkg, arena, shape):
    lib = pkg._lib.load()
    x, x0 = _dense(shape)
    B, n = shape[0], x[0].numel()
    S = STEPS + 1
    g = torch.randn((S * B,) + tuple(shape[1:]), generator=torch.Generator().manual_seed(22))
    group = shape[-1] if shape[-1] in (1, 5) else 4
    extra = torch.randn(B, n // group, generator=torch.Generator().manual_seed(23))
    specs = {"g": (g, "in"), "x": (x, "in"), "x0": (x0, "in"), "extra": (extra, "in"), "acc": (Out(shape), "out"), "attr": (Out(shape), "out"),
             "grouped": (Out((B, n // group)), "out")}
    BEGIN, FINISH = pkg._lib.IG_BEGIN, pkg._lib.IG_FINISH

    def whole(o):
        return lib.stlt_ig_reduce(o.g.ptr, B, n, STEPS, 0, STEPS, BEGIN | FINISH, o.acc.ptr, o.x.ptr, o.x0.ptr, 0.0, o.attr.ptr, group, o.extra.ptr, o.grouped.ptr, GA.stream())

    def split(o):
        rc = lib.stlt_ig_reduce(o.g.ptr, B, n, STEPS, 0, 2, BEGIN, o.acc.ptr, None, None, 0.0, None, 1, None, None, GA.stream())
        return rc or lib.stlt_ig_reduce(o.g.ptr + 3 * B * n * 4, B, n, STEPS, 3, 5, FINISH, o.acc.ptr, o.x.ptr, o.x0.ptr, 0.0, o.attr.ptr, group, o.extra.ptr, o.grouped.ptr,
                                        GA.stream())

    acc = R.reduce(g.numpy(), STEPS, 0, STEPS)
    attr = R.finish(acc, x.numpy(), x0.numpy())
    want = {"acc": acc, "attr": attr, "grouped": R.grouped(attr, group, extra.numpy())}
    for call in (whole, split):
        for mis in (None, {"g": 4, "x": 12, "x0": 8, "acc": 4, "attr": 8, "grouped": 12, "extra": 4}):
            got = GA.three_ways(lib, arena, specs, call, ["acc", "attr", "grouped"], misalign=mis)
            for k in want:
                _same_bits(got[k], want[k], f"{k} {shape} {call.__name__}")
    # a NULL baseline is `fill`; without grouping nothing but acc and attr is written
    specs2 = {k: specs[k] for k in ("g", "x", "acc", "attr")}
    got = GA.three_ways(lib, arena, specs2, lambda o: lib.stlt_ig_reduce(o.g.ptr, B, n, STEPS, 0, STEPS, BEGIN | FINISH, o.acc.ptr, o.x.ptr, None, 0.5, o.attr.ptr, 1, None, None,
                                                                        GA.stream()), ["attr"])
    _same_bits(got["attr"], R.finish(acc, x.numpy(), 0.5), f"attr {shape} fill")


# ---------------------------------------------------------------------------------------------------------------- 3. stlt_ig_delta
def test_ig_delta_against_float64_and_across_grids(pkg, arena):
    """|delta - fp64| <= 2^-23 * (number of addends) * sum|attr|: the worst case of a float32 sum in any order.  Two stage-1 grids: same bits."""
    lib = pkg._lib.load()
    B, K = 3, 7
    ch = pkg._lib.IG_DELTA_CHUNK
    ns = (150, ch + 5, 27)  # an odd tensor, one that spills into a second chunk, a tiny one
    g = torch.Generator().manual_seed(31)
    a = [torch.randn(B, n, generator=g) for n in ns]
    seed, lx, lx0 = (torch.randn(B, K, generator=g) for _ in range(3))
    chunks = sum(-(-n // ch) for n in ns)
    assert lib.stlt_ig_delta_scratch_bytes(B, *ns) == B * chunks * 4
    specs = {"a0": (a[0], "in"), "a1": (a[1], "in"), "a2": (a[2], "in"), "seed": (seed, "in"), "lx": (lx, "in"), "lx0": (lx0, "in"),
             "scratch": (Out((B * chunks,)), "out"), "delta": (Out((B,)), "out")}
    res = {}
    for blocks in (0, 1, 5):
        call = lambda o: lib.stlt_ig_delta(o.a0.ptr, ns[0], o.a1.ptr, ns[1], o.a2.ptr, ns[2], o.seed.ptr, o.lx.ptr, o.lx0.ptr, B, K, blocks, o.scratch.ptr,  # noqa: E731
                                           B * chunks * 4, o.delta.ptr, GA.stream())
        for mis in (None, {"a0": 4, "a1": 12, "a2": 8, "seed": 4, "lx": 8, "lx0": 12, "scratch": 4, "delta": 4}):
            res[(blocks, mis is None)] = GA.three_ways(lib, arena, specs, call, ["delta", "scratch"], misalign=mis)
    first = res[(0, True)]
    for k, r in res.items():
        assert torch.equal(r["delta"].view(torch.int32), first["delta"].view(torch.int32)) and torch.equal(r["scratch"].view(torch.int32), first["scratch"].view(torch.int32)), k
    want, mag, n_add = R.delta([t.numpy() for t in a], seed.numpy(), lx.numpy(), lx0.numpy())
    err = np.abs(first["delta"].double().numpy() - want)
    bound = 2.0 ** -23 * n_add * mag
    _report("stlt_ig_delta |delta - fp64| / bound", (err / bound).tolist())
    assert (err <= bound).all()
    # one and two tensors: the absent ones are not read (NULL)
    dev = [t.to(DEV) for t in a] + [seed.to(DEV), lx.to(DEV), lx0.to(DEV)]
    got = pkg.ops.ig_delta(dev[:2], *dev[3:])
    want2, mag2, n2 = R.delta([t.numpy() for t in a[:2]], seed.numpy(), lx.numpy(), lx0.numpy())
    assert (np.abs(got.cpu().double().numpy() - want2) <= 2.0 ** -23 * n2 * mag2).all()


# ------------------------------------------------------------------------------------------------------- 4. stlt_cell_pool_sum / _abs
@pytest.mark.parametrize("shape,cell", [((2, 3, 3, 5, 6), (2, 2, 4)), ((1, 3, 16, 32, 32), (16, 32, 32))], ids=["ragged", "one-video-cell"])
def test_cell_pool_sum_against_float64_and_abs_keeps_its_bits(pkg, arena, shape, cell):
    lib = pkg._lib.load()
    g = torch.randn(shape, generator=torch.Generator().manual_seed(41))
    B = shape[0]
    C = int(np.prod([-(-e // c) for e, c in zip(shape[2:], cell)]))
    specs = {"g": (g, "in"), "out": (Out((B, C)), "out")}
    got = {}
    for name in ("stlt_cell_pool_sum", "stlt_cell_pool_abs"):
        call = lambda o: getattr(lib, name)(o.g.ptr, B, *shape[1:], *cell, o.out.ptr, GA.stream())  # noqa: E731
        for mis in (None, {"g": 4, "out": 12}):
            got[name] = GA.three_ways(lib, arena, specs, call, ["out"], misalign=mis)["out"]
    want = R.cell_pool(g.numpy(), cell)
    mag = R.cell_pool(g.numpy(), cell, absolute=True)
    per_cell = shape[1] * cell[0] * cell[1] * cell[2]
    err = np.abs(got["stlt_cell_pool_sum"].double().numpy() - want)
    _report(f"stlt_cell_pool_sum {shape} |sum - fp64| / (2^-23 n sum|g|)", float((err / (2.0 ** -23 * per_cell * mag)).max()))
    assert (err <= 2.0 ** -23 * per_cell * mag).all() and (np.abs(want) < mag).all()  # a signed sum: every cell holds both signs
    _same_bits(got["stlt_cell_pool_abs"], R.cell_pool_abs_bits(g.numpy(), cell), f"stlt_cell_pool_abs {shape}")
    assert torch.equal(pkg.ops.cell_pool_sum(g.to(DEV), cell).cpu(), got["stlt_cell_pool_sum"])


# ---------------------------------------------------------------------------------------------------------------- 5. refusals
def test_refusals_leave_every_output_untouched(pkg, arena):
    lib = pkg._lib.load()
    x, x0 = _dense((2, 3, 2, 5, 5))
    B, n = 2, 150
    g = torch.randn(2 * B, n)
    specs = {"x": (x, "in"), "x0": (x0, "in"), "g": (g, "in"), "seed": (torch.randn(B, 4), "in"), "out": (Out((2 * B, n)), "out"), "acc": (Out((B, n)), "out"),
             "attr": (Out((B, n)), "out"), "grouped": (Out((B, 30)), "out"), "scratch": (Out((B,)), "out"), "delta": (Out((B,)), "out"), "pool": (Out((B, 1)), "out")}
    b, _ = _layout()
    lay = {k: (v, *_ROLES[k]) for k, v in b.items()}
    lay.update({"o_" + k: (Out((2 * 3,) + tuple(v.shape[1:]), v.dtype), "out") for k, v in b.items()})
    specs.update(lay)
    arena.reset()
    o = type("O", (), {k: arena.place(s[0], s[1], band=(s[2] if len(s) > 2 else None), name=k) for k, s in specs.items()})
    st = GA.stream()
    F = pkg._lib.IG_FINISH

    def path(steps=4, s0=0, s1=1, null=None, B_=3):
        inp = pkg._lib.Inputs()
        inp.B, inp.T, inp.N = B_, 3, 3
        for k in b:
            setattr(inp, _ABI.get(k, k), None if k == null else getattr(o, k).ptr)
        return lib.stlt_ig_path(ctypes.byref(inp), None, None, steps, s0, s1, o.o_categories.ptr, None if null == "o_boxes" else o.o_boxes.ptr, o.o_scores.ptr,
                                o.o_src_key_padding_mask_boxes.ptr, o.o_frame_types.ptr, o.o_src_key_padding_mask_frames.ptr, o.o_lengths.ptr, st)

    calls = {
        "path: steps < 1": lambda: path(steps=0, s1=0), "path: s0 > s1": lambda: path(s0=2, s1=1), "path: s1 > steps": lambda: path(s1=5),
        "path: > 256 steps": lambda: path(steps=1000, s1=256), "path: null input": lambda: path(null="boxes"), "path: null output": lambda: path(null="o_boxes"),
        "path: null struct": lambda: lib.stlt_ig_path(None, None, None, 4, 0, 1, o.o_categories.ptr, o.o_boxes.ptr, o.o_scores.ptr, o.o_src_key_padding_mask_boxes.ptr,
                                                      o.o_frame_types.ptr, o.o_src_key_padding_mask_frames.ptr, o.o_lengths.ptr, st),
        "path: 2^31 elements": lambda: path(B_=1 << 28),
        "dense: null x": lambda: lib.stlt_ig_path_dense(None, o.x0.ptr, 0.0, B, n, 4, 0, 1, o.out.ptr, st),
        "dense: null out": lambda: lib.stlt_ig_path_dense(o.x.ptr, o.x0.ptr, 0.0, B, n, 4, 0, 1, None, st),
        "dense: steps < 1": lambda: lib.stlt_ig_path_dense(o.x.ptr, o.x0.ptr, 0.0, B, n, 0, 0, 0, o.out.ptr, st),
        "dense: s0 > s1": lambda: lib.stlt_ig_path_dense(o.x.ptr, o.x0.ptr, 0.0, B, n, 4, 2, 1, o.out.ptr, st),
        "dense: s1 > steps": lambda: lib.stlt_ig_path_dense(o.x.ptr, o.x0.ptr, 0.0, B, n, 4, 4, 5, o.out.ptr, st),
        "dense: > 256 steps": lambda: lib.stlt_ig_path_dense(o.x.ptr, o.x0.ptr, 0.0, B, n, 1000, 0, 256, o.out.ptr, st),
        "dense: 2^31 elements": lambda: lib.stlt_ig_path_dense(o.x.ptr, o.x0.ptr, 0.0, 1 << 16, 1 << 15, 4, 0, 1, o.out.ptr, st),
        "reduce: null g": lambda: lib.stlt_ig_reduce(None, B, n, 4, 0, 1, 1, o.acc.ptr, None, None, 0.0, None, 1, None, None, st),
        "reduce: null acc": lambda: lib.stlt_ig_reduce(o.g.ptr, B, n, 4, 0, 1, 1, None, None, None, 0.0, None, 1, None, None, st),
        "reduce: finish without x": lambda: lib.stlt_ig_reduce(o.g.ptr, B, n, 4, 0, 1, 1 | F, o.acc.ptr, None, None, 0.0, o.attr.ptr, 1, None, None, st),
        "reduce: finish without attr": lambda: lib.stlt_ig_reduce(o.g.ptr, B, n, 4, 0, 1, 1 | F, o.acc.ptr, o.x.ptr, None, 0.0, None, 1, None, None, st),
        "reduce: group does not divide n": lambda: lib.stlt_ig_reduce(o.g.ptr, B, n, 4, 0, 1, 1 | F, o.acc.ptr, o.x.ptr, None, 0.0, o.attr.ptr, 4, None, o.grouped.ptr, st),
        "reduce: grouped without finish": lambda: lib.stlt_ig_reduce(o.g.ptr, B, n, 4, 0, 1, 1, o.acc.ptr, None, None, 0.0, None, 5, None, o.grouped.ptr, st),
        "reduce: unknown flag": lambda: lib.stlt_ig_reduce(o.g.ptr, B, n, 4, 0, 1, 8, o.acc.ptr, None, None, 0.0, None, 1, None, None, st),
        "reduce: s1 > steps": lambda: lib.stlt_ig_reduce(o.g.ptr, B, n, 4, 4, 5, 1, o.acc.ptr, None, None, 0.0, None, 1, None, None, st),
        "reduce: steps < 1": lambda: lib.stlt_ig_reduce(o.g.ptr, B, n, 0, 0, 0, 1, o.acc.ptr, None, None, 0.0, None, 1, None, None, st),
        "delta: null seed": lambda: lib.stlt_ig_delta(o.x.ptr, n, None, 0, None, 0, None, o.seed.ptr, o.seed.ptr, B, 4, 0, o.scratch.ptr, B * 4, o.delta.ptr, st),
        "delta: null tensor with n > 0": lambda: lib.stlt_ig_delta(o.x.ptr, n, None, 5, None, 0, o.seed.ptr, o.seed.ptr, o.seed.ptr, B, 4, 0, o.scratch.ptr, 2 * B * 4, o.delta.ptr, st),
        "delta: scratch too small": lambda: lib.stlt_ig_delta(o.x.ptr, n, None, 0, None, 0, o.seed.ptr, o.seed.ptr, o.seed.ptr, B, 4, 0, o.scratch.ptr, B * 4 - 1, o.delta.ptr, st),
        "delta: no tensor": lambda: lib.stlt_ig_delta(None, 0, None, 0, None, 0, o.seed.ptr, o.seed.ptr, o.seed.ptr, B, 4, 0, o.scratch.ptr, B * 4, o.delta.ptr, st),
        "delta: 2^31 elements": lambda: lib.stlt_ig_delta(o.x.ptr, 1 << 31, None, 0, None, 0, o.seed.ptr, o.seed.ptr, o.seed.ptr, B, 4, 0, o.scratch.ptr, B * 4, o.delta.ptr, st),
        "delta: null delta": lambda: lib.stlt_ig_delta(o.x.ptr, n, None, 0, None, 0, o.seed.ptr, o.seed.ptr, o.seed.ptr, B, 4, 0, o.scratch.ptr, B * 4, None, st),
        "pool: null out": lambda: lib.stlt_cell_pool_sum(o.x.ptr, B, 3, 2, 5, 5, 2, 5, 5, None, st),
        "pool: zero cell": lambda: lib.stlt_cell_pool_sum(o.x.ptr, B, 3, 2, 5, 5, 0, 5, 5, o.pool.ptr, st),
    }
    for what, call in calls.items():
        rc = call()
        assert rc == EINVAL, f"{what}: expected STLT_EINVAL, got {rc} ({GA.last_error(lib)})"
        assert GA.last_error(lib).startswith(("stlt_ig_", "stlt_cell_pool_sum")), (what, GA.last_error(lib))
    arena.check(launched=False)


# ---------------------------------------------------------------------------------------------------------------- 6. Stlt, end to end
def _stlt(pkg, name):
    c, sd, batch = IC.layout_case(*[cs for cs in IC.CASES if cs[0] == name][0])
    m = pkg.Stlt(pkg.StltModelConfig(**pkg.synth.model_kwargs(name)))
    m.load_state_dict(sd)
    m.train(False).to(DEV)
    return m, batch, {k: v.to(DEV) for k, v in batch.items()}


def _zero_under_masks(batch, r):
    pad_obj, pad_frm = batch["src_key_padding_mask_boxes"].bool(), batch["src_key_padding_mask_frames"].bool()
    maps = [r["boxes_attribution"].cpu().abs().sum(-1), r["object_attribution"].cpu().abs()] + ([r["scores_attribution"].cpu().abs()] if "scores_attribution" in r else [])
    for a in maps:
        assert a[pad_obj].numel() == 0 or a[pad_obj].max().item() == 0.0, "a padded object slot has an attribution"
        assert a[pad_frm].numel() == 0 or a[pad_frm].max().item() == 0.0, "a padded frame has an attribution"
        assert a[~pad_obj].max().item() > 0.0


def _compose(pkg, m, dev, target, steps, per, moved, kw=None, baseline=None):
    """The call, by hand, from the public pieces: ops.ig_path / ig_path_dense, the model's forward_saliency on each pass with the tiled
    target, ops.ig_reduce — passes from the input end, `per` steps each.  -> {key: attribution}, object attribution or None"""
    ops, kw, baseline = pkg.ops, kw or {}, baseline or {}
    layout = {k: dev[k].contiguous() for k, _, _ in ops.PERTURB_KEYS if k in dev}
    lay_moves = "boxes" in moved
    acc, attr, obj = {k: torch.empty_like(dev[k]) for k in moved}, {}, None
    hi = steps
    while hi >= 0:
        lo = max(hi - per + 1, 0)
        n = hi - lo + 1
        tile = lambda v: v.repeat((n,) + (1,) * (v.dim() - 1))  # noqa: E731
        part = ops.ig_path(layout, steps, lo, hi, baseline.get("boxes"), baseline.get("scores")) if lay_moves else {k: tile(v) for k, v in layout.items()}
        for k in ("video_frames", "appearance_features"):
            if k in dev:
                part[k] = ops.ig_path_dense(dev[k], steps, lo, hi, baseline.get(k)) if k in moved else tile(dev[k])
        out = m.forward_saliency(part, target=tile(target), **kw)
        for k in sorted(moved, key=lambda k: k != "scores"):
            args = dict(begin=hi == steps)
            if lo == 0:
                args.update(finish=True, x=dev[k], baseline=baseline.get(k))
                if k == "boxes":
                    args.update(group=4, extra=attr.get("scores"))
                attr[k], grouped = ops.ig_reduce(out[k + "_grad"].contiguous(), acc[k], steps, lo, hi, **args)
                obj = grouped if k == "boxes" else obj
            else:
                ops.ig_reduce(out[k + "_grad"].contiguous(), acc[k], steps, lo, hi, **args)
        hi = lo - 1
    return attr, obj


@pytest.mark.parametrize("name,B", IC.CASES)
def test_stlt_integrated_gradients_match_the_fp64_oracle(pkg, name, B):
    """Every attribution within CAP * max|x - x0| * max_s max|g_s^ref| of the fp64 oracle's IG on the same quadrature (CAP = 2e-4: the bar
    every gradient of the path is held to; the weights sum to 1), zeros exactly under both masks, delta within the sum of those bounds plus
    1e-4 * sum|seed| (the logit bar) of the oracle's delta; skip_padding off and on."""
    m, batch, dev = _stlt(pkg, name)
    with torch.no_grad():
        fwd = m(dev)["stlt"]
    res = {}
    for skip in (False, True):
        m.backbone.skip_padding = skip
        r = m.forward_integrated_gradients(dev, steps=IC.STEPS)
        keys = {"boxes_attribution"} | ({"scores_attribution"} if "scores" in batch else set())
        assert set(r) == {"stlt", "baseline_logits", "target", "delta", "object_attribution"} | keys, sorted(r)
        assert r["target"].dtype == torch.int64 and r["target"].is_cuda and torch.equal(r["target"], r["stlt"].argmax(dim=1))
        assert tuple(r["object_attribution"].shape) == tuple(batch["categories"].shape) and tuple(r["delta"].shape) == (B,)
        assert (r["stlt"] - fwd).abs().max().item() <= IC.LOGIT_BAR
        ref = IC.oracle_ig(name, B, tuple(r["target"].tolist()))
        per, dbound = IC.bounds(ref)
        for k in ref["attr"]:
            err = (r[k + "_attribution"].cpu().double() - ref["attr"][k]).abs().max().item()
            _report(f"{name} B={B} skip_padding={skip} {k}_attribution err / bound", f"{err / per[k]:.3g}")
            assert err <= per[k], (k, err, per[k])
        obj = sum(ref["attr"][k].sum(-1) if k == "boxes" else ref["attr"][k] for k in ref["attr"])
        oerr = (r["object_attribution"].cpu().double() - obj).abs().max().item()
        _report(f"{name} B={B} skip_padding={skip} object_attribution err / sum of the five bounds", f"{oerr / (4 * per['boxes'] + per.get('scores', 0.0)):.3g}")
        assert oerr <= 4 * per["boxes"] + per.get("scores", 0.0)
        derr = (r["delta"].cpu().double() - ref["delta"]).abs()
        _report(f"{name} B={B} skip_padding={skip} delta err / bound; |delta| gpu; |delta| oracle", ((derr / dbound).tolist(), r["delta"].abs().tolist(), ref["delta"].abs().tolist()))
        assert (derr <= dbound).all()
        _zero_under_masks(batch, r)
        assert all(q.grad is None for q in m.parameters()), "forward_integrated_gradients created a parameter gradient"
        res[skip] = r
    # both schedules are within the bound of one oracle, so within twice the bound of each other
    per, _ = IC.bounds(IC.oracle_ig(name, B, tuple(res[False]["target"].tolist())))
    assert torch.equal(res[True]["target"], res[False]["target"])
    assert (res[True]["boxes_attribution"] - res[False]["boxes_attribution"]).abs().max().item() <= 2 * per["boxes"]


def test_stlt_call_is_the_composition_of_the_public_pieces(pkg):
    name, B = IC.CASES[0]
    m, batch, dev = _stlt(pkg, name)
    steps, S = IC.STEPS, IC.STEPS + 1
    with torch.no_grad():
        fwd = m(dev)["stlt"]
    g = torch.Generator().manual_seed(51)
    base = {"boxes": torch.rand(batch["boxes"].shape, generator=g).to(DEV), "scores": torch.rand(batch["scores"].shape, generator=g).to(DEV)}
    runs = {}
    for per in (1, 2, S):
        r = m.forward_integrated_gradients(dev, steps=steps, steps_per_pass=per, baseline=base)
        again = m.forward_integrated_gradients(dev, steps=steps, steps_per_pass=per, baseline=base)
        assert all(torch.equal(r[k], again[k]) for k in r), "two identical calls differ"
        attr, obj = _compose(pkg, m, dev, r["target"], steps, per, ("boxes", "scores"), baseline=base)
        for k in attr:
            assert torch.equal(attr[k], r[k + "_attribution"]), f"steps_per_pass={per}: {k}_attribution is not the composition's"
        assert torch.equal(obj, r["object_attribution"])
        assert (r["stlt"] - fwd).abs().max().item() <= IC.LOGIT_BAR
        with torch.no_grad():
            at_base = m(dict(dev, **base))["stlt"]
        assert (r["baseline_logits"] - at_base).abs().max().item() <= IC.LOGIT_BAR
        # the three target forms agree bit for bit
        onehot = torch.nn.functional.one_hot(r["target"], r["stlt"].shape[1]).float()
        for t in (r["target"], onehot):
            by = m.forward_integrated_gradients(dev, target=t, steps=steps, steps_per_pass=per, baseline=base)
            assert torch.equal(by["object_attribution"], r["object_attribution"]) and torch.equal(by["delta"], r["delta"]) and by["target"] is t
        runs[per] = r
    # another chunking is another order of the same sum: within the bound the oracle test holds each of them to
    c, sd, _ = IC.layout_case(name, B)
    seed = torch.nn.functional.one_hot(runs[S]["target"].cpu(), c["num_classes"]).double()
    ref = R.stlt_ig(sd, batch, c["num_attention_heads"], seed, steps, baseline={k: v.cpu() for k, v in base.items()})
    per = {k: IC.CAP * ref["diff_max"][k] * ref["grad_max"][k] for k in ref["attr"]}
    per = {"boxes_attribution": per["boxes"], "scores_attribution": per["scores"], "object_attribution": 4 * per["boxes"] + per["scores"]}
    for chunk in (1, 2):
        for k, bound in per.items():
            d = (runs[chunk][k] - runs[S][k]).abs().max().item()
            _report(f"steps_per_pass={chunk} vs {S}: {k} max diff / bound", f"{d / bound:.3g}")
            assert d <= bound
    for k in ("boxes", "scores"):
        err = (runs[S][k + "_attribution"].cpu().double() - ref["attr"][k]).abs().max().item()
        _report(f"random baseline: {k}_attribution err / bound", f"{err / per[k + '_attribution']:.3g}")
        assert err <= per[k + "_attribution"]
    _zero_under_masks(batch, runs[S])


def test_stlt_refusals_keep_a_pending_tape(pkg):
    name = "cfg1"
    c = pkg.synth.CONFIGS[name]
    batch = pkg.synth.make_batch(2, c["T"], c["N"], seed=1)
    dev = {k: v.to(DEV) for k, v in batch.items()}
    m = pkg.Stlt(pkg.StltModelConfig(**dict(pkg.synth.model_kwargs(name), hidden_dropout_prob=0.1))).to(DEV)
    m.train(False)
    pending = m(dev)["stlt"]  # a grad-enabled forward: its graph owns the backbone's tape
    Err = pkg._lib.StltHipError
    m.train(True)
    with pytest.raises(Err, match="training mode with dropout"):
        m.forward_integrated_gradients(dev)
    m.train(False)
    bad = [dict(steps=0), dict(steps=2.0), dict(steps_per_pass=0), dict(baseline={"boxes": dev["boxes"][:1]}), dict(baseline={"boxes": dev["boxes"].double()}),
           dict(baseline={"boxes": batch["boxes"]}), dict(baseline={"video_frames": dev["boxes"]}), dict(baseline=dev["boxes"]), dict(target=torch.zeros(3, dtype=torch.int64, device=DEV)),
           dict(target=torch.zeros(2, 5, device=DEV)), dict(target=[0, 1])]
    for kw in bad:
        with pytest.raises(Err):
            m.forward_integrated_gradients(dev, **kw)
    with pytest.raises(Err, match="CPU"):
        m.forward_integrated_gradients(batch)
    with pytest.raises(Err, match="modality"):
        pkg.modelling.explain.forward_integrated_gradients(m, dev, modality="appearance", modalities=m.perturb_modalities)
    pending.sum().backward()  # none of the refusals touched the tape
    assert any(q.grad is not None for q in m.parameters())
    m.zero_grad(set_to_none=True)
    pending = m(dev)["stlt"]
    m.forward_integrated_gradients(dev, steps=1)  # ... a call that runs re-records it, as forward_saliency does
    with pytest.raises(Err, match="tape was overwritten"):
        pending.sum().backward()


def test_runner_takes_integrated_gradients(pkg):
    name = "micro"
    c = pkg.synth.CONFIGS[name]
    m = pkg.Stlt(pkg.StltModelConfig(**pkg.synth.model_kwargs(name))).to(DEV)
    m.train(False)
    batch = pkg.synth.make_batch(3, c["T"], c["N"], seed=2)
    dev = {k: v.to(DEV) for k, v in batch.items()}
    scores = pkg.infer.attribution_scores(m, dev, "integrated_gradients")
    assert torch.equal(scores, m.forward_integrated_gradients(dev)["object_attribution"])
    a = pkg.infer.run_perturbation_test(m, [batch], method="integrated_gradients", steps=4)
    b = pkg.infer.run_perturbation_test(m, [batch], method="saliency", steps=4)
    assert set(a) == set(b) and a["fractions"] == b["fractions"]
    for order in ("descending", "ascending"):
        assert set(a[order]) == set(b[order]) and len(a[order]["prob"]) == 5 and a[order]["num_clips"] == 3
        assert a[order]["prob"][0] == b[order]["prob"][0]  # step 0 deletes nothing, whatever the map


# ---------------------------------------------------------------------------------------------------------------- 7. video and fusion
import test_pixel_gradients_gpu as PG  # noqa: E402  (the SMALL config, VIDEO and the seeded models of the pixel-gradient tests)


def _check_composition(pkg, m, dev, moved, names, modality=None, head=None):
    call = dict(steps=2, **({"modality": modality} if modality else {}), **({"head": head} if head else {}))
    r = m.forward_integrated_gradients(dev, **call)
    again = m.forward_integrated_gradients(dev, **call)
    assert all(torch.equal(r[k], again[k]) for k in r), "two identical calls differ"
    want = set(names) | {"baseline_logits", "target", "delta"} | {k + "_attribution" for k in moved}
    want |= {"object_attribution"} if "boxes" in moved else set()
    want |= {"cell_attribution"} if ("video_frames" in moved or "appearance_features" in moved) else set()
    assert set(r) == want, sorted(r)
    h = head or names[-1]
    assert torch.equal(r["target"], r[h].argmax(dim=1))
    with torch.no_grad():
        fwd = m(dev)
    assert all((r[n] - fwd[n]).abs().max().item() <= 1e-4 for n in names)
    for per in (3, 2):
        rr = r if per == 3 else m.forward_integrated_gradients(dev, steps_per_pass=per, **call)
        attr, obj = _compose(pkg, m, dev, r["target"], 2, per, moved, kw={"head": head} if head else {})
        for k in attr:
            assert tuple(attr[k].shape) == tuple(dev[k].shape) and torch.equal(attr[k], rr[k + "_attribution"]), f"steps_per_pass={per}: {k}"
        if obj is not None:
            assert torch.equal(obj, rr["object_attribution"])
    # delta covers every moved input together: the float64 sum of the returned attributions minus the returned logits' gap
    seed = torch.nn.functional.one_hot(r["target"], r[h].shape[1]).double().cpu()
    d64, mag, n_add = R.delta([r[k + "_attribution"].cpu().numpy() for k in moved], seed.numpy(), r[h].cpu().numpy(), r["baseline_logits"].cpu().numpy())
    assert (np.abs(r["delta"].cpu().double().numpy() - d64) <= 2.0 ** -23 * n_add * mag + 1e-30).all()
    for k in ("video_frames", "appearance_features"):
        if k in moved:
            _, cell, _ = pkg.collate.appearance_cells({k: dev[k]})
            assert torch.equal(r["cell_attribution"], pkg.ops.cell_pool_sum(r[k + "_attribution"], cell))
    assert all(q.grad is None for q in m.parameters())
    return r


@pytest.mark.parametrize("name", ["resnet3d", "resnet3d-transformer"])
def test_video_models_integrated_gradients_compose(pkg, name):
    m, _ = PG._load(pkg, pkg.models_factory[name](PG._app_cfg(pkg, PG.FRAMES, num_appearance_layers=2)))
    m.train(False)
    dev = {"video_frames": PG._video(pkg)}
    r = _check_composition(pkg, m, dev, ("video_frames",), ("resnet3d",))
    assert r["video_frames_attribution"].abs().max().item() > 0 and tuple(r["cell_attribution"].shape) == (PG.VIDEO[0], 4)
    Err = pkg._lib.StltHipError
    with pytest.raises(Err, match="GPU|CPU"):
        m.forward_integrated_gradients({"video_frames": dev["video_frames"].cpu()})
    with pytest.raises(Err):
        m.forward_integrated_gradients(dev, baseline={"video_frames": dev["video_frames"][:1]})
    with pytest.raises(Err):
        m.forward_integrated_gradients(dev, baseline={"boxes": dev["video_frames"]})
    if name == "resnet3d-transformer":
        m.train(True)
        with pytest.raises(Err, match="training mode with dropout"):
            m.forward_integrated_gradients(dev)


def test_caf_integrated_gradients_by_modality(pkg):
    m, sd, kw = PG._fusion(pkg, "caf")
    lay, _ = PG._fusion_batch(pkg)
    dev = dict(lay, video_frames=PG._video(pkg))
    both = _check_composition(pkg, m, dev, ("boxes", "scores", "video_frames"), m.logit_names, modality="both")
    layout = _check_composition(pkg, m, dev, ("boxes", "scores"), m.logit_names, modality="layout")
    app = _check_composition(pkg, m, dev, ("video_frames",), m.logit_names, modality="appearance")
    assert "video_frames_attribution" not in layout and "cell_attribution" not in layout and "boxes_attribution" not in app and "object_attribution" not in app
    assert both["video_frames_attribution"].abs().max().item() > 0 and both["boxes_attribution"].abs().max().item() > 0
    with pytest.raises(pkg._lib.StltHipError, match="modality"):
        m.forward_integrated_gradients(dev, modality="pixels")
    with pytest.raises(pkg._lib.StltHipError, match="does not move"):
        m.forward_integrated_gradients(dev, modality="layout", baseline={"video_frames": dev["video_frames"]})
    feats = pkg.synth.make_appearance_features(PG.VIDEO[0], seed=1620, grid=(1, 2, 2)).to(DEV)
    f = _check_composition(pkg, m, dict(lay, appearance_features=feats), ("appearance_features",), m.logit_names, modality="appearance")
    assert tuple(f["cell_attribution"].shape) == (PG.VIDEO[0], 4)
    # the runner's two score functions hand out the two maps
    assert torch.equal(pkg.infer.attribution_scores(m, dev, "integrated_gradients"), m.forward_integrated_gradients(dev, modality="layout")["object_attribution"])
    assert torch.equal(pkg.infer.appearance_attribution_scores(m, dev, "integrated_gradients"), m.forward_integrated_gradients(dev, modality="appearance")["cell_attribution"])


@pytest.mark.parametrize("name,head", [("cacnf", "caf"), ("lcf", "lcf")])
def test_cacnf_and_lcf_integrated_gradients_with_a_head(pkg, name, head):
    m, sd, kw = PG._fusion(pkg, name)
    lay, _ = PG._fusion_batch(pkg)
    feats = pkg.synth.make_appearance_features(PG.VIDEO[0], seed=1620, grid=(1, 2, 2)).to(DEV)
    _check_composition(pkg, m, dict(lay, appearance_features=feats), ("boxes", "scores", "appearance_features"), m.logit_names, head=head)
    with pytest.raises(pkg._lib.StltHipError, match="head must be one of"):
        m.forward_integrated_gradients(dict(lay, appearance_features=feats), head="nope")
