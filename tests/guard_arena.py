"""Guard-band arena for the C-ABI kernels: operands live inside ONE flat device allocation, each between two guard bands
the test owns, so a store past an extent lands in memory that is checked instead of in the allocator's slack.

    arena = Arena(nbytes)                                  # once per test module
    arena.reset()                                          # per case: forget the operands, keep the allocation
    x = arena.place(host_x, "in")                          # float input: NaN bands
    y = arena.place(Out((M, N), ld=N + 3), "out")          # output: extent, gap columns and bands hold FILL
    rc = lib.stlt_linear_fwd(x.ptr, ..., y.ptr, ...)
    arena.check()                                          # bands / inputs / gaps untouched, every output element written
    y.view                                                 # the logical (M, N) result

Every operand starts at a 256-byte-aligned offset plus `misalign` bytes and has a band of max(64 KiB, operand bytes) before and
after it.  Roles:
    "in"      float input.  Bands are NaN: a value read from a band that reaches the result poisons it.
    "out"     output / scratch / workspace.  Extent and bands hold FILL, a non-canonical NaN bit pattern no kernel computes (compared
              as int32 / bytes).  A host tensor may be given instead of an `Out`: then the extent starts from that content
              (accumulating outputs, in-place updates) and only the bands and gap columns are checked for FILL.
    "index"   integer input that names table rows (categories, frame_types, labels).  Bands hold `band`, an IN-RANGE index chosen
              by the test: the extra table row whose content the test filled with NaN.
    "extent"  integer input that carries extents or offsets (lengths, seg_start / seg_end, frame_offsets) and byte masks.  Bands
              hold `band`, an in-range value.
No band ever holds a value that would send a correct or an incorrect kernel to a wild address: an overrun must land in memory the
test owns and be seen, never fault.

Where include/stlt_hip.h documents an over-read (stlt_gemm's contraction-major rows beyond K, stlt_weight_grad_group's rows rounded
to 32) the documented padding is part of the operand the test places, zero-filled as the header demands; the band starts after it.

What this can and cannot see: a WRITE anywhere in a band, a gap column or an input is caught bit for bit.  An over-READ is caught
only when the value read reaches the result (NaN / FILL propagate); a kernel that reads past an operand and discards the value is
invisible here, and placing operands at allocation boundaries to catch that is deliberately not attempted (a fault on a shared
machine is not a test outcome).
"""
from __future__ import annotations

import re
from types import SimpleNamespace
from typing import Optional

import torch

FILL = 0x7FC5A5A5  # a quiet NaN with a payload: arithmetic yields the canonical NaN 0x7fc00000 or propagates another payload
BAND_MIN = 64 * 1024
ALIGN = 256
_FILL_BYTES = FILL.to_bytes(4, "little")


class Out:
    """Shape of an output operand: `shape` logical, `ld` the row pitch in elements of a 2-D (rows, cols) output (default: cols)."""

    def __init__(self, shape, dtype=torch.float32, ld: Optional[int] = None, must_write: bool = True):
        self.must_write = must_write  # False: scratch / workspace / tape — a call need not touch every byte of what it was lent
        self.shape = tuple(int(s) for s in (shape if isinstance(shape, (tuple, list)) else (shape,)))
        self.dtype = dtype
        self.ld = ld
        if ld is not None:
            assert len(self.shape) == 2 and ld >= self.shape[1]


def _round_up(v: int, a: int) -> int:
    return (v + a - 1) // a * a


class Operand:
    """One placed operand: `ptr` for the C-ABI, `view` the logical tensor (strided for an output with ld), `flat` the whole extent."""

    def __init__(self, name, role, start, nbytes, band, flat, view, ld_cols):
        self.name, self.role, self.start, self.nbytes, self.band = name, role, start, nbytes, band
        self.flat, self.view, self.ld_cols = flat, view, ld_cols
        self.saved = None  # inputs: the bytes copied in
        self.written = True  # "out": False while the extent must not hold FILL any more after the call

    @property
    def ptr(self) -> int:
        return self.flat.data_ptr()

    def numel_bytes(self) -> int:
        return self.nbytes


class Plain:
    """The same interface over an ordinary torch tensor (the "as today's tests do" run)."""

    def __init__(self, t: torch.Tensor, view: torch.Tensor):
        self.flat, self.view = t, view
        self.nbytes = t.numel() * t.element_size()

    @property
    def ptr(self) -> int:
        return self.flat.data_ptr()


def plain(spec, device="cuda"):
    """An operand outside the arena: a host tensor is uploaded, an `Out` becomes a fresh torch.empty (FILL is not written: this is
    the run every other GPU test makes)."""
    if isinstance(spec, Out):
        rows_ld = spec.ld if spec.ld is not None else None
        if rows_ld is None:
            t = torch.empty(spec.shape, dtype=spec.dtype, device=device)
            return Plain(t, t)
        t = torch.empty(spec.shape[0] * rows_ld, dtype=spec.dtype, device=device)
        return Plain(t, t.view(spec.shape[0], rows_ld)[:, :spec.shape[1]])
    t = spec.to(device)
    return Plain(t, t)


class Arena:
    def __init__(self, nbytes: int, device="cuda"):
        n = _round_up(nbytes, ALIGN)
        self._raw = torch.empty(n + ALIGN, dtype=torch.uint8, device=device)
        skip = -self._raw.data_ptr() % ALIGN
        self.buf = self._raw[skip:skip + n]
        assert self.buf.data_ptr() % ALIGN == 0
        self.device = device
        self._fill_cache = torch.tensor(list(_FILL_BYTES) * 2, dtype=torch.uint8, device=device)
        self.reset()

    # ---- layout ------------------------------------------------------------------------------------------------------------
    def reset(self):
        self.cursor = 0
        self.operands = []

    def _fill_like(self, start: int, stop: int) -> torch.Tensor:
        """The FILL byte pattern as it lies at arena bytes [start, stop) (the pattern is laid from 4-byte-aligned offsets)."""
        n = stop - start
        need = n + 8
        if self._fill_cache.numel() < need:
            self._fill_cache = torch.tensor(list(_FILL_BYTES), dtype=torch.uint8, device=self.device).repeat(_round_up(need, 4) // 4 + 1)
        ph = start % 4
        return self._fill_cache[ph:ph + n]

    def _set_fill(self, start: int, stop: int):
        a, b = start // 4 * 4, _round_up(stop, 4)
        self.buf[a:b].view(torch.int32).fill_(FILL - (1 << 32) if FILL >= (1 << 31) else FILL)

    def place(self, spec, role: str, misalign: int = 0, band=None, name: Optional[str] = None) -> Operand:
        assert role in ("in", "out", "index", "extent")
        host = None if isinstance(spec, Out) else spec
        if host is not None:
            assert not host.is_cuda and host.is_contiguous()
            dtype, n_el, shape, ld = host.dtype, host.numel(), tuple(host.shape), None
        else:
            dtype, shape, ld = spec.dtype, spec.shape, spec.ld
            n_el = shape[0] * ld if ld is not None else int(torch.Size(shape).numel())
        size = torch.empty((), dtype=dtype).element_size()
        assert misalign % size == 0 and 0 <= misalign < ALIGN, "misalign must keep the element type's natural alignment"
        nbytes = n_el * size
        band_bytes = _round_up(max(BAND_MIN, nbytes), ALIGN)
        region0 = self.cursor
        start = region0 + band_bytes + misalign
        region1 = _round_up(start + nbytes, ALIGN) + band_bytes
        assert region1 <= self.buf.numel(), f"arena too small: {region1} > {self.buf.numel()} bytes"
        self.cursor = region1
        flat = self.buf[start:start + nbytes].view(dtype)
        if ld is not None:
            view = flat.view(shape[0], ld)[:, :shape[1]]
        else:
            view = flat.view(shape)
        op = Operand(name or f"op{len(self.operands)}", role, start, nbytes, (region0, region1), flat, view, (ld, shape[1]) if ld is not None else None)
        # bands (and, for a shaped output, the extent)
        if role == "out":
            self._set_fill(region0, region1)
            op.written = host is not None or not spec.must_write
        elif role == "in":
            assert dtype.is_floating_point, "role 'in' is for float inputs; integer inputs are 'index' or 'extent'"
            self.buf[region0:region1].view(torch.float32).fill_(float("nan"))
        else:
            assert band is not None and not dtype.is_floating_point, "integer inputs need an in-range band value"
            a = region0 + (start - region0) % size  # element grid of the operand, extended over both bands
            b = region1 - (region1 - a) % size
            self.buf[region0:region1].zero_()
            self.buf[a:b].view(dtype).fill_(band)
        if host is not None:
            flat.copy_(host.reshape(-1).to(self.device))
            op.saved = self.buf[start:start + nbytes].clone()  # inputs: checked; initialised outputs: what restore_outputs puts back
        op.band_saved = None
        if role != "out":
            op.band_saved = (self.buf[region0:start].clone(), self.buf[start + nbytes:region1].clone())
        self.operands.append(op)
        return op

    def refill_outputs(self):
        """Before a second call on the same placement: FILL back into every shaped output (extent, gaps, bands), the initial
        content back into every output that was placed from a host tensor (an accumulator would otherwise add twice).  Inputs are
        left exactly as the previous call left them."""
        for op in self.operands:
            if op.role != "out":
                continue
            if op.saved is None:
                self._set_fill(*op.band)
            else:
                self.buf[op.start:op.start + op.nbytes].copy_(op.saved)

    # ---- checks ------------------------------------------------------------------------------------------------------------
    def check(self, launched: bool = True):
        """launched=False: the call was refused before anything ran, so every shaped output must still hold FILL everywhere."""
        if self.buf.is_cuda:
            torch.cuda.synchronize()
        for op in self.operands:
            r0, r1 = op.band
            s, e = op.start, op.start + op.nbytes
            if op.role == "out":
                for what, a, b in (("before", r0, s), ("after", e, r1)):
                    got, want = self.buf[a:b], self._fill_like(a, b)
                    if not torch.equal(got, want):
                        bad = (got != want).nonzero()
                        first, last = int(bad[0]), int(bad[-1])
                        off = (first - (s - a)) if what == "before" else first
                        raise AssertionError(f"{op.name}: guard band {what} the output was written: {bad.numel()} bytes, first at byte {off:+d} "
                                             f"from the extent's {'start' if what == 'before' else 'end'}, last {last - first} bytes later")
                size = op.flat.element_size()
                if op.ld_cols is not None:
                    ld, cols = op.ld_cols
                    rows = op.flat.numel() // ld
                    if ld > cols:
                        gaps = self.buf[s:e].view(rows, ld * size)[:, cols * size:]
                        want = self._fill_like(s, e).view(rows, ld * size)[:, cols * size:]
                        if not torch.equal(gaps, want):
                            r = (gaps != want).any(dim=1).nonzero()
                            raise AssertionError(f"{op.name}: gap columns {cols}..{ld - 1} were written in {r.numel()} rows (first row {int(r[0])})")
                if not launched:
                    if not torch.equal(self.buf[s:e], self._fill_like(s, e) if op.saved is None else op.saved):
                        raise AssertionError(f"{op.name}: the output was written although the call was refused")
                elif not op.written:
                    if op.ld_cols is not None:
                        ld, cols = op.ld_cols
                        rows = op.flat.numel() // ld
                        got = self.buf[s:e].view(rows, ld * size)[:, :cols * size].reshape(rows * cols, size)
                        want = self._fill_like(s, e).view(rows, ld * size)[:, :cols * size].reshape(rows * cols, size)
                    else:
                        got = self.buf[s:e].view(-1, size)
                        want = self._fill_like(s, e).view(-1, size)
                    still = (got == want).all(dim=1)
                    if bool(still.any()):
                        idx = still.nonzero()
                        raise AssertionError(f"{op.name}: {idx.numel()} of {still.numel()} output elements were never written (first: element {int(idx[0])})")
            else:
                if not (torch.equal(self.buf[r0:s], op.band_saved[0]) and torch.equal(self.buf[e:r1], op.band_saved[1])):
                    raise AssertionError(f"{op.name}: a guard band of this input was written")
                if not torch.equal(self.buf[s:e], op.saved):
                    bad = (self.buf[s:e] != op.saved).nonzero()
                    raise AssertionError(f"{op.name}: the input was modified ({bad.numel()} bytes, first at byte {int(bad[0])})")


def is_fill(t: torch.Tensor) -> torch.Tensor:
    """Elementwise: does a float32 / int32 device tensor still hold FILL?"""
    return t.contiguous().view(torch.int32) == (FILL - (1 << 32) if FILL >= (1 << 31) else FILL)


# ---- the harness both test modules share -------------------------------------------------------------------------------------------
def stream():
    return torch.cuda.current_stream().cuda_stream


def rand(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(*shape, generator=g) * 2 - 1) * scale


def pitched(t, ld):
    """(rows, cols) -> (rows, ld) with NaN in the gap columns: an input the kernel must read through its pitch."""
    if ld == t.shape[1]:
        return t.contiguous()
    out = torch.full((t.shape[0], ld), float("nan"), dtype=t.dtype)
    out[:, :t.shape[1]] = t
    return out


def last_error(lib):
    return lib.stlt_last_error().decode("utf-8", "replace")


def three_ways(lib, arena, specs, call, outs, misalign=None):
    """specs: {name: (host tensor | Out, role[, band])}.  call(o) -> return code, o.<name> has .ptr / .view / .nbytes.
    Runs the call plainly (separate torch tensors), inside the arena, and inside the arena again with the inputs as the first run left
    them; asserts Arena.check() after both arena runs, plain == arena bit for bit, second == first.  -> {name: host result}."""
    misalign = misalign or {}
    P = SimpleNamespace(**{n: plain(s[0], arena.device) for n, s in specs.items()})
    rc = call(P)
    assert rc == 0, last_error(lib)
    torch.cuda.synchronize()
    base = {n: getattr(P, n).view.clone() for n in outs}
    del P
    arena.reset()
    A = SimpleNamespace(**{n: arena.place(s[0], s[1], band=(s[2] if len(s) > 2 else None), name=n, misalign=misalign.get(n, 0)) for n, s in specs.items()})
    rc = call(A)
    assert rc == 0, last_error(lib)
    arena.check()
    first = {n: getattr(A, n).view.clone() for n in outs}
    for n in outs:
        assert torch.equal(first[n], base[n]), f"{n}: the arena run differs from the plain run"
    arena.refill_outputs()
    rc = call(A)
    assert rc == 0, last_error(lib)
    arena.check()
    for n in outs:
        assert torch.equal(getattr(A, n).view, first[n]), f"{n}: the second arena run differs from the first"
    return {n: t.cpu() for n, t in first.items()}


STLT_EINVAL = -1


def misaligned(lib, arena, specs, call, outs, operand=None, mis=0, refused_as=None):
    """One arena run with `operand` re-placed `mis` bytes past its 256-byte boundary, every other operand aligned.  refused_as = the
    name the error message must use for the operand: the call returns STLT_EINVAL, names it, and launches nothing (every output still
    holds FILL).  Otherwise the call succeeds inside the bands.  -> {name: host result} or None when refused."""
    arena.reset()
    A = SimpleNamespace(**{n: arena.place(s[0], s[1], band=(s[2] if len(s) > 2 else None), name=n, misalign=(mis if n == operand else 0)) for n, s in specs.items()})
    if operand is not None:
        assert getattr(A, operand).ptr % 16 == mis % 16
    rc = call(A)
    msg = last_error(lib)
    if refused_as is not None:
        assert rc == STLT_EINVAL, f"{operand} at +{mis} bytes: expected STLT_EINVAL, got {rc} ({msg})"
        assert re.search(rf"(?<![A-Za-z0-9_]){re.escape(refused_as)}(?![A-Za-z0-9_])", msg) and "aligned" in msg, f"{operand} at +{mis}: message does not name {refused_as}: {msg}"
        arena.check(launched=False)
        return None
    assert rc == 0, f"{operand} at +{mis} bytes: {msg}"
    arena.check()
    return {n: getattr(A, n).view.cpu() for n in outs}


def collate_case(with_scores):
    """B = 3 videos of 4, 1 and 5 frames padded to T = 5, N = 3 object slots; the expected batch restated from the header's words."""
    B, T, N, cls_id = 3, 5, 3, 77
    lens = [4, 1, 5]
    F = sum(lens)
    g = torch.Generator().manual_seed(5)
    cat_r = torch.randint(0, 6, (F, N), generator=g)
    cat_r[:, 0] = cls_id
    box_r, sc_r, ft_r = torch.rand(F, N, 4, generator=g), torch.rand(F, N, generator=g), torch.randint(1, 4, (F,), generator=g)
    offsets = torch.tensor([0, 4, 5, 10])
    cat, box, sc, ft = torch.zeros(B, T, N, dtype=torch.int64), torch.zeros(B, T, N, 4), torch.zeros(B, T, N), torch.zeros(B, T, dtype=torch.int64)
    cat[:, :, 0], sc[:, :, 0] = cls_id, 1.0
    box[:, :, 0] = torch.tensor([0.0, 0.0, 1.0, 1.0])
    for b, n in enumerate(lens):
        f0 = int(offsets[b])
        cat[b, :n], box[b, :n], sc[b, :n], ft[b, :n] = cat_r[f0:f0 + n], box_r[f0:f0 + n], sc_r[f0:f0 + n], ft_r[f0:f0 + n]
    want = {"cat": cat, "box": box, "ft": ft, "kpm_boxes": (cat == 0).to(torch.uint8), "kpm_frames": (ft == 0).to(torch.uint8)}
    specs = {"cat_r": (cat_r, "extent", 0), "box_r": (box_r, "in"), "ft_r": (ft_r, "extent", 0), "offsets": (offsets, "extent", F),
             "cat": (Out((B, T, N), torch.int64), "out"), "box": (Out((B, T, N, 4)), "out"), "ft": (Out((B, T), torch.int64), "out"),
             "kpm_boxes": (Out((B, T, N), torch.uint8), "out"), "kpm_frames": (Out((B, T), torch.uint8), "out")}
    if with_scores:
        specs["sc_r"], specs["sc"] = (sc_r, "in"), (Out((B, T, N)), "out")
        want["sc"] = sc

    def call(lib):
        return lambda o: lib.stlt_collate_fwd(o.cat_r.ptr, o.box_r.ptr, o.sc_r.ptr if with_scores else None, o.ft_r.ptr, o.offsets.ptr, B, T, N, cls_id, o.cat.ptr,
                                              o.box.ptr, o.sc.ptr if with_scores else None, o.ft.ptr, o.kpm_boxes.ptr, o.kpm_frames.ptr, stream())

    return specs, call, want
