"""The row-map helpers of tests/rowmap_cases.py, on the CPU: what tests/test_hip_rowmaps.py trusts when it lays operands out and when it
declares an output's holes untouched."""
import numpy as np
import pytest
import torch

import rowmap_cases as rc

BF16, F32 = torch.bfloat16, torch.float32
# (map, logical rows, cols): plain with padding, segmented with foreign rows between the segments (the GEMM tests' 40 + 57), segmented
# with a ragged last segment, the resampler's media / latent interleaving, one row per segment, segments that run backwards in memory
MAPS = [(rc.Map(12), 7, 9), (rc.Map(336, 97 * 336, 40), 200, 328), (rc.Map(16, 5 * 16 + 8, 3), 11, 16),
        (rc.Map(36, 74 * 36, 50), 150, 36), (rc.Map(36, 74 * 36, 24), 72, 36), (rc.Map(8, 24, 1), 5, 8), (rc.Map(73, 40 * 73 + 5, 40), 100, 70)]
BCAST = [(rc.Map(36, 0, 24), 72, 36), (rc.Map(336, 0, 40), 200, 328), (rc.Map(10, 0, 4), 9, 7)]


def _brute_offsets(m, rows):
    """row offsets by walking the rows one at a time, without division"""
    out, seg, within = [], 0, 0
    for _ in range(rows):
        out.append(seg * m.seg_stride + within * m.ld if m.rows_per_seg > 0 else len(out) * m.ld)
        within += 1
        if m.rows_per_seg > 0 and within == m.rows_per_seg:
            seg, within = seg + 1, 0
    return out


@pytest.mark.parametrize("m,rows,cols", MAPS + BCAST, ids=str)
def test_off_and_span_agree_with_enumeration(m, rows, cols):
    brute = _brute_offsets(m, rows)
    assert [rc.off(m, r) for r in range(rows)] == brute
    assert rc.span(m, rows, cols) == max(brute) + cols
    if m.rows_per_seg <= 0:
        assert brute == [r * m.ld for r in range(rows)]
    if rc.is_broadcast(m):
        assert brute == [(r % m.rows_per_seg) * m.ld for r in range(rows)]


def test_off_matches_the_header_formula_on_a_grid():
    for ld in (1, 8, 13):
        for seg in (0, 5, 104, 1 << 33):
            for rps in (-1, 0, 1, 3, 40):
                for r in (0, 1, 2, 39, 40, 41, 199):
                    want = r * ld if rps <= 0 else (r // rps) * seg + (r % rps) * ld
                    assert rc.off((ld, seg, rps), r) == want


@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("base", [0, 40])
@pytest.mark.parametrize("m,rows,cols", MAPS, ids=str)
def test_gather_inverts_scatter(m, rows, cols, dtype, base):
    x = torch.as_tensor(np.random.default_rng(1).standard_normal((rows, cols)).astype(np.float32)).to(dtype)
    buf = rc.scatter(x, m, dtype, rc.OPERAND_FILL, base=base)
    assert buf.dtype == dtype and buf.numel() == base + rc.span(m, rows, cols)
    assert torch.equal(rc.gather(buf, m, rows, cols, base=base), x)
    # everything else holds the fill: as many elements as the map does not address
    fill = torch.tensor(rc.OPERAND_FILL).to(dtype)
    assert int((buf == fill).sum()) == buf.numel() - rows * cols
    # element by element against the enumeration
    flat = buf.tolist()
    for r in (0, rows // 2, rows - 1):
        o = base + _brute_offsets(m, rows)[r]
        assert flat[o:o + cols] == x[r].tolist()


@pytest.mark.parametrize("m,rows,cols", BCAST, ids=str)
def test_broadcast_scatter_takes_one_segment(m, rows, cols):
    seg = torch.as_tensor(np.random.default_rng(2).standard_normal((m.rows_per_seg, cols)).astype(np.float32))
    buf = rc.scatter(seg, m, F32, rc.OPERAND_FILL)
    assert buf.numel() == rc.span(m, m.rows_per_seg, cols) == rc.span(m, rows, cols)
    got = rc.gather(buf, m, rows, cols)
    assert torch.equal(got, seg.repeat(-(-rows // m.rows_per_seg), 1)[:rows])
    with pytest.raises(AssertionError):
        rc.scatter(torch.zeros(m.rows_per_seg + 1, cols), m, F32, 0.0)


def test_scatter_refuses_overlapping_rows():
    with pytest.raises(AssertionError):
        rc.scatter(torch.zeros(4, 8), rc.Map(4), F32, 0.0)          # pitch below the width
    with pytest.raises(AssertionError):
        rc.scatter(torch.zeros(6, 8), rc.Map(8, 16, 3), F32, 0.0)   # segments closer than their length


@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("base", [0, 40])
@pytest.mark.parametrize("m,rows,cols", MAPS, ids=str)
def test_holes_untouched_sees_every_hole_and_only_holes(m, rows, cols, dtype, base):
    before = rc.filled(m, rows, cols, dtype, rc.OUTPUT_FILL, "cpu", base=base)
    assert before.numel() == base + rc.span(m, rows, cols)
    assert rc.holes_untouched(before.clone(), before, m, rows, cols, base=base)
    addressed = set()
    for o in _brute_offsets(m, rows):
        addressed.update(range(base + o, base + o + cols))
    holes = [i for i in range(before.numel()) if i not in addressed]
    assert len(holes) == before.numel() - rows * cols
    # a change in addressed rows is not the holes' business
    after = before.clone()
    after[sorted(addressed)] = 7.0
    assert rc.holes_untouched(after, before, m, rows, cols, base=base)
    # one changed element in a hole is: the first, the last and a spread of holes, one at a time
    picks = [holes[0], holes[-1]] + holes[:: max(1, len(holes) // 25)] if holes else []
    for i in picks:
        bad = after.clone()
        bad[i] = 1.0
        assert not rc.holes_untouched(bad, before, m, rows, cols, base=base), i


def test_holes_untouched_is_bitwise():
    m, rows, cols = rc.Map(8, 40, 2), 4, 4
    before = rc.filled(m, rows, cols, F32, 0.0, "cpu")
    after = before.clone()
    after[5] = -0.0                                                  # equal as a float, another bit pattern
    assert bool(after[5] == before[5]) and not rc.holes_untouched(after, before, m, rows, cols)
    nan = before.clone().fill_(float("nan"))
    assert rc.holes_untouched(nan.clone(), nan, m, rows, cols)       # NaN == NaN bit for bit
