"""Row maps for the kernel tests (a helper module, not a conftest): the C ABI's ff_rowmap in plain Python, and buffers laid out by one.

A map is (ld, seg_stride, rows_per_seg), the fields of ffi.RowMap in their order: logical row r lives at
    (r // rows_per_seg) * seg_stride + (r % rows_per_seg) * ld          elements from the base,
rows_per_seg <= 0 is plain row-major with pitch ld, seg_stride == 0 with rows_per_seg > 0 broadcasts ONE segment to every logical row.

tests/test_hip_rowmaps.py builds every operand with `scatter` (the logical rows where the map puts them, a fill value everywhere else: in
the padding columns, between the segments and in front of `base`), reads results back with `gather` and compares everything the map does
not address with `holes_untouched`; tests/test_rowmap_cases.py holds these helpers to brute-force enumerations on the CPU.

Fills: OPERAND_FILL for what a kernel reads - huge and finite, so a kernel that reads a foreign row is wrong by orders of magnitude more
than any bound, but produces no NaN or inf that could mask a second fault; OUTPUT_FILL for what it writes."""
from collections import namedtuple

import torch

Map = namedtuple("Map", ["ld", "seg_stride", "rows_per_seg"], defaults=(0, 0))
OPERAND_FILL = 1.0e30
OUTPUT_FILL = -3.25
_INT_VIEW = {1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}


def plain(ld) -> Map:
    return Map(int(ld), 0, 0)


def is_broadcast(m) -> bool:
    m = Map(*m)
    return m.rows_per_seg > 0 and m.seg_stride == 0


def off(m, r: int) -> int:
    """element offset of logical row r from the base"""
    m = Map(*m)
    if m.rows_per_seg <= 0:
        return r * m.ld
    return (r // m.rows_per_seg) * m.seg_stride + (r % m.rows_per_seg) * m.ld


def span(m, rows: int, cols: int) -> int:
    """elements needed from the base to hold `rows` logical rows of `cols` elements"""
    return max(off(m, r) for r in range(rows)) + cols if rows > 0 else 0


def c_map(m):
    """the ffi.RowMap of a map"""
    from flamingo_mini_amd import ffi
    return ffi.rowmap(*Map(*m))


def _index(m, rows, cols, base, device):
    offs = torch.tensor([base + off(m, r) for r in range(rows)], dtype=torch.int64, device=device)
    return offs[:, None] + torch.arange(cols, dtype=torch.int64, device=device)[None, :]


def scatter(logical, m, dtype, fill, device=None, base=0, alloc=None):
    """A flat buffer of base + span elements of `dtype` holding `fill` everywhere and the rows of `logical` (rows, cols) where the map puts
    them.  For a broadcast map `logical` is ONE segment (at most rows_per_seg rows).  `alloc(n, dtype, device)` replaces torch.empty (the
    library's guarded allocation seam, for outputs)."""
    logical = torch.as_tensor(logical)
    rows, cols = logical.shape
    if is_broadcast(m):
        assert rows <= Map(*m).rows_per_seg, "a broadcast map stores one segment"
    device = logical.device if device is None else torch.device(device)
    n = base + span(m, rows, cols)
    buf = torch.empty(n, dtype=dtype, device=device) if alloc is None else alloc(n, dtype, device)
    buf.fill_(fill)
    idx = _index(m, rows, cols, base, device)
    assert torch.unique(idx).numel() == idx.numel(), "the map puts two logical rows on the same elements"
    buf[idx.reshape(-1)] = logical.to(device=device, dtype=dtype).reshape(-1)
    return buf


def filled(m, rows, cols, dtype, fill, device, base=0, alloc=None):
    """scatter's buffer without any logical rows: `fill` everywhere (an output before the call)"""
    n = base + span(m, min(rows, Map(*m).rows_per_seg) if is_broadcast(m) else rows, cols)
    buf = torch.empty(n, dtype=dtype, device=device) if alloc is None else alloc(n, dtype, device)
    return buf.fill_(fill)


def gather(buffer, m, rows: int, cols: int, base=0):
    """the (rows, cols) logical matrix a map addresses in a flat buffer (a broadcast map repeats its segment)"""
    flat = buffer.reshape(-1)
    return flat[_index(m, rows, cols, base, flat.device).reshape(-1)].reshape(rows, cols)


def holes_untouched(buffer, before, m, rows: int, cols: int, base=0) -> bool:
    """True iff every element of `buffer` that the map does NOT address equals `before`'s bit for bit (integer views: NaN payloads and
    signed zeros count)."""
    a, b = buffer.reshape(-1), before.reshape(-1)
    assert a.shape == b.shape and a.dtype == b.dtype, (a.shape, b.shape, a.dtype, b.dtype)
    hole = torch.ones(a.numel(), dtype=torch.bool, device=a.device)
    hole[_index(m, rows, cols, base, a.device).reshape(-1)] = False
    iv = _INT_VIEW[a.element_size()]
    return bool(torch.equal(a.view(iv)[hole], b.view(iv)[hole]))
