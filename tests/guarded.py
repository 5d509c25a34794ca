"""Guarded allocations for the kernel tests (a helper module, not a conftest).

    with guarded_allocations() as g:
        C = functional.gemm(A, B)
        g.check()                 # every guard still holds its sentinel, bit for bit

Inside the context every buffer the library allocates through its allocation seam (functional._new / _new_zeros / _new_like /
_new_zeros_like) is a view into a larger buffer laid out as

    [head guard][body][tail guard]

- the guards hold a fixed, FINITE sentinel: a huge-magnitude value (+1.7e38) for float32 / bfloat16 buffers, 0xA5 bytes for every other
  dtype (integers, workspaces).  A kernel that reads past an operand and discards the value with a zero weight stays correct; one that
  lets it through shows a huge error.
- the head guard is a multiple of 4 KiB, so the body keeps (more than) the 256-byte alignment torch gives and the kernels choose the
  same vector paths as without guards.
- the tail guard is at least one 256-row tile at the buffer's row pitch (64 KiB at least, 4 MiB at most): a plausible tile overrun lands
  in memory the test owns.
- `empty` bodies are poisoned (NaN for floating point, 0xA5 bytes otherwise), so an element the kernel never writes reaches the test's
  comparison as NaN; `zeros` bodies are zero.

`Guards` works on any device (the CPU tests of the checker use it directly); `guarded_allocations()` guards the devices in
`device_types` (CUDA by default) and passes any other allocation through.  The registry belongs to the context: nothing survives it.
Not usable while a stream is capturing a graph (the fills would become graph nodes): it raises.  The library's gradient arena
(functional.GradArena) hands out slices of one buffer and is not covered.
"""
import contextlib
import traceback

import torch

HEAD_BYTES = 16 * 1024
TAIL_MIN, TAIL_MAX = 64 * 1024, 4 * 1024 * 1024
TILE_ROWS = 256
_BLOCK = 4096                                    # guard sizes are multiples of this; the sentinel is compared block by block
# sentinel element patterns: finite, huge, and not a value any kernel computes by accident
SENTINEL = {torch.float32: 0x7EFFA5A5, torch.bfloat16: 0x7EFF}
SEAM = ("_new", "_new_zeros", "_new_like", "_new_zeros_like")


def _pattern_block(dtype) -> torch.Tensor:
    """_BLOCK bytes of the guard pattern for `dtype` (uint8, CPU)."""
    bits = SENTINEL.get(dtype)
    if bits is None:
        return torch.full((_BLOCK,), 0xA5, dtype=torch.uint8)
    es = torch.tensor([], dtype=dtype).element_size()
    word = int(bits).to_bytes(es, "little")
    return torch.tensor(list(word * (_BLOCK // es)), dtype=torch.uint8)


def _round_up(n, m):
    return (int(n) + m - 1) // m * m


def _site() -> str:
    """A short traceback of the allocation: the innermost frames outside this module and torch."""
    frames = [f for f in traceback.extract_stack()[:-1] if not f.filename.endswith("guarded.py") and "/torch/" not in f.filename]
    return " <- ".join(f"{f.filename.rsplit('/', 1)[-1]}:{f.lineno} {f.name}" for f in reversed(frames[-4:]))


class GuardViolation(AssertionError):
    pass


class _Record:
    __slots__ = ("raw", "head", "body", "dtype", "shape", "site")

    def __init__(self, raw, head, body, dtype, shape, site):
        self.raw, self.head, self.body, self.dtype, self.shape, self.site = raw, head, body, dtype, shape, site


class Guards:
    """The registry of one guarded stretch.  `new` / `new_zeros` / `new_like` / `new_zeros_like` mirror the library's seam."""

    def __init__(self):
        self.records = []
        self._blocks = {}

    # ---- allocation -----------------------------------------------------------------------------------------------------------------
    def _alloc(self, shape, dtype, device, zero, strides=None) -> torch.Tensor:
        device = torch.device(device)
        if device.type == "cuda" and torch.cuda.is_current_stream_capturing():
            raise RuntimeError("guarded allocations during graph capture: the guard fills would become graph nodes")
        shape = tuple(int(s) for s in (shape if isinstance(shape, (tuple, list, torch.Size)) else (shape,)))
        es = torch.tensor([], dtype=dtype).element_size()
        if strides is None:
            span = 1
            for s in shape:
                span *= s
        else:
            span = 1 + sum((s - 1) * st for s, st in zip(shape, strides)) if all(s > 0 for s in shape) else 0
        body = _round_up(span * es, es)
        pitch = (shape[-1] if len(shape) >= 2 else 16) * es
        if strides is not None and len(shape) >= 2:
            pitch = max(strides[:-1] + (shape[-1],)) * es
        tail = _round_up(min(max(TILE_ROWS * pitch, TAIL_MIN), TAIL_MAX), _BLOCK)
        # the tail starts right after the body, at a multiple of the element size: the sentinel's period, so the pattern stays aligned
        raw = torch.empty(HEAD_BYTES + body + tail, dtype=torch.uint8, device=device)
        blk = self._block(dtype, device)
        raw[:HEAD_BYTES].view(-1, _BLOCK).copy_(blk.expand(HEAD_BYTES // _BLOCK, _BLOCK))
        t0 = HEAD_BYTES + body
        tail_all = raw[t0:]
        full = tail_all.numel() // _BLOCK * _BLOCK
        tail_all[:full].view(-1, _BLOCK).copy_(blk.expand(full // _BLOCK, _BLOCK))
        if tail_all.numel() > full:
            tail_all[full:].copy_(blk[: tail_all.numel() - full])
        flat = raw[HEAD_BYTES:HEAD_BYTES + body]
        if zero:
            flat.zero_()
        elif dtype.is_floating_point:
            flat.view(dtype).fill_(float("nan"))
        else:
            flat.fill_(0xA5)
        typed = flat.view(dtype)
        out = typed.view(shape) if strides is None else typed.as_strided(shape, strides)
        self.records.append(_Record(raw, HEAD_BYTES, body, dtype, shape, _site()))
        return out

    def _block(self, dtype, device):
        key = (dtype, device)
        if key not in self._blocks:
            self._blocks[key] = _pattern_block(dtype).to(device)
        return self._blocks[key]

    def new(self, shape, dtype, device):
        return self._alloc(shape, dtype, device, zero=False)

    def new_zeros(self, shape, dtype, device):
        return self._alloc(shape, dtype, device, zero=True)

    def new_like(self, t, dtype=None, zero=False):
        dtype = t.dtype if dtype is None else dtype
        strides = torch.empty_like(t, dtype=dtype, device="meta").stride()       # the layout torch.empty_like would give
        return self._alloc(t.shape, dtype, t.device, zero=zero, strides=tuple(strides))

    def new_zeros_like(self, t, dtype=None):
        return self.new_like(t, dtype, zero=True)

    # ---- inspection -----------------------------------------------------------------------------------------------------------------
    def raw(self, t: torch.Tensor):
        """(whole uint8 buffer, byte offset of the body) of a guarded tensor - for tests that write into the guards on purpose."""
        for r in self.records:
            if r.raw.untyped_storage().data_ptr() == t.untyped_storage().data_ptr():
                return r.raw, r.head
        raise KeyError("not a guarded allocation")

    def violations(self):
        """[(site, side, first bad byte offset relative to the body's first byte, shape, dtype)] of every guard that lost its sentinel."""
        if any(r.raw.is_cuda for r in self.records):
            torch.cuda.synchronize()
        bad = []
        for r in self.records:
            blk = self._block(r.dtype, r.raw.device)
            head = r.raw[:r.head].view(-1, _BLOCK)
            diff = head != blk
            if bool(diff.any()):
                first = int(diff.reshape(-1).nonzero()[0])
                bad.append((r.site, "head", first - r.head, r.shape, r.dtype))
            t0 = r.head + r.body
            tail = r.raw[t0:]
            full = tail.numel() // _BLOCK * _BLOCK
            ref = torch.cat([blk.expand(full // _BLOCK, _BLOCK).reshape(-1), blk[: tail.numel() - full]])
            diff = tail != ref
            if bool(diff.any()):
                first = int(diff.nonzero()[0])
                bad.append((r.site, "tail", r.body + first, r.shape, r.dtype))
        return bad

    def check(self) -> None:
        """Synchronise and compare every guard bitwise; raise GuardViolation naming the allocation site, the side and the first bad byte."""
        bad = self.violations()
        if bad:
            lines = [f"{side} guard of {tuple(shape)} {str(dtype).replace('torch.', '')} hit at body byte {off}: allocated at {site}"
                     for site, side, off, shape, dtype in bad]
            raise GuardViolation(f"{len(bad)} guard(s) overwritten:\n  " + "\n  ".join(lines[:8]))

    def clear(self) -> None:
        self.records = []


def _functional():
    from flamingo_mini_amd import functional
    return functional


@contextlib.contextmanager
def guarded_allocations(device_types=("cuda",), check_on_exit=True):
    """Swap the library's allocation seam for guarded versions (restored on exit, monkeypatch-style).  Yields the Guards registry; on a
    normal exit the guards are checked once more."""
    if torch.cuda.is_available() and torch.cuda.is_current_stream_capturing():
        raise RuntimeError("guarded_allocations() cannot be entered while a stream is capturing a graph")
    F = _functional()
    saved = {n: getattr(F, n) for n in SEAM}
    g = Guards()
    types = tuple(device_types)

    def pick(dev):
        return torch.device(dev).type in types

    F._new = lambda shape, dtype, device: g.new(shape, dtype, device) if pick(device) else saved["_new"](shape, dtype, device)
    F._new_zeros = lambda shape, dtype, device: g.new_zeros(shape, dtype, device) if pick(device) else saved["_new_zeros"](shape, dtype, device)
    F._new_like = lambda t, dtype=None: g.new_like(t, dtype) if pick(t.device) else saved["_new_like"](t, dtype)
    F._new_zeros_like = lambda t, dtype=None: g.new_zeros_like(t, dtype) if pick(t.device) else saved["_new_zeros_like"](t, dtype)
    ok = False
    try:
        yield g
        ok = True
    finally:
        for n, f in saved.items():
            setattr(F, n, f)
        try:
            if ok and check_on_exit:
                g.check()
        finally:
            g.clear()
