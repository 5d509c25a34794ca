"""Segmented and broadcast row maps (ff_rowmap) on every GEMM tile and LayerNorm path, on the MI355X.

The C ABI addresses every matrix through a row map: logical row r lives at (r / rows_per_seg) * seg_stride + (r % rows_per_seg) * ld, and
seg_stride = 0 broadcasts one segment.  The resampler interleaves media and latent rows in one buffer with such maps and repeats its latents
over the batch with a broadcast one; every other test of a GEMM / LayerNorm / rows_reduce entry point passes plain maps, and the resampler
parity tests run bf16 only where every segment edge is a tile edge (64 latents).  Here the maps go straight into ffi.GemmDesc / LnDesc /
ReduceDesc, with segments of 40 rows and 57 foreign rows between them, so that every 32- / 64- / 128- / 256-row tile edge and every
64-element k-step falls inside a segment somewhere, and the resampler runs where segments and tiles disagree (40, 24, 100, 72 latents).

Operands are laid out by tests/rowmap_cases.py: everything a map does not address holds 1e30 (operands) or -3.25 (outputs).  Every call
is checked in this order:
  1. no hole of an output buffer changed, bit for bit, and the guards of tests/guarded.py around outputs and workspace are intact;
  2. the gathered result equals, bit for bit, the same call on contiguous copies of the logical operands (same descriptor apart from the
     maps): a map changes addresses, not arithmetic or the order of additions - the library against itself;
  3. the gathered result is within the repository's float64 bounds, unchanged: util.gemm_bound_ok element by element (fp32 products through
     padded rows: u_out 2^-21 as in test_gemm_row_pitch_larger_than_width; activation epilogues: u_mid 2^-8 / 2^-19 and, for fp32, u_out
     2^-19 as in test_gemm_epilogues_guarded) plus GEMM_ROW_TOL per bf16 row; TOL and ROW_TOL of test_hip_bounds.py for the row-wise
     kernels and the resampler - the library against the reference.

No case lost assertion 2.  The one place where the two calls could take different code paths is the fp32 scalar-load section (an
unaligned ld switches the vector loads off, a contiguous twin could switch them back on): there the twin keeps the same unaligned pitch,
a plain map over padded rows, so both calls take the scalar path and the equality holds.

fp32 LayerNorm at 36 columns: 36 % 4 == 0, so unlike bf16 (36 % 8 != 0: the element-wise VEC = 1 kernels) it stays on the vector path.
"""
import functools

import numpy as np
import pytest
import torch

import rowmap_cases as rc
from detgen import det, resampler_params
from guarded import guarded_allocations
from oracle import flamingo_oracle as O
from test_hip_bounds import GEMM_ROW_TOL, ROW_TOL
from util import TOL, as64, dev, gemm_bound_ok, gemm_ref, rel, rel_rows, rnd

pytestmark = pytest.mark.gpu
BF16, F32 = torch.bfloat16, torch.float32
NAME = {BF16: "bf16", F32: "f32"}
SEG, GAP = 40, 57                       # rows per segment, foreign rows between two segments
FF_ERR_UNSUPPORTED = -2

# The bf16 resampler's worst-row bound (y per (sample, latent), d x per (sample, frame, token)) comes from the ALIGNED twins of RS_CASES -
# the same dims with 64 latents and 64 tokens per frame, the geometry the suite has long held to the oracle - never from the unaligned
# cases under test.  Measured on an MI355X (FF_TOL_REPORT + tools/tol_report.py, the [rows] entries of test_resampler_aligned_twin_rows,
# worst of y and d x, stack-level and layer by layer): q40-R140 1.121e-2, vit-tokens-q24 9.29e-3, q100 8.88e-3, dh128-q72 7.55e-3.
# All within ROW_TOL[BF16] = 1.2e-2, so ROW_TOL[BF16] is the bound (a twin above it would have set the bound to its worst row x 1.5,
# the margin ROW_TOL itself was given).  For the record, the unaligned cases under that bound: 1.012e-2, 1.095e-2, 8.71e-3, 8.36e-3.
RS_ROW_TWIN_MEASURED = {"q40-R140": 1.121e-2, "vit-tokens-q24": 9.29e-3, "q100": 8.88e-3, "dh128-q72": 7.55e-3}
assert max(RS_ROW_TWIN_MEASURED.values()) <= ROW_TOL[torch.bfloat16]["out"]
RS_ROW_TOL = {F32: ROW_TOL[F32], BF16: ROW_TOL[BF16]}


def F():
    from flamingo_mini_amd import functional
    return functional


def _ffi():
    from flamingo_mini_amd import ffi
    return ffi


def _seg(ld, rows_per_seg=SEG, gap=GAP):
    """segments of rows_per_seg rows at pitch ld with `gap` foreign rows between them"""
    return rc.Map(ld, (rows_per_seg + gap) * ld, rows_per_seg)


def _bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == BF16 else torch.int32)


def _same_bits(a, b):
    return a.shape == b.shape and torch.equal(_bits(a), _bits(b))


def _alloc(n, dtype, device):
    """outputs come from the library's allocation seam: inside guarded_allocations() they sit between guard bands"""
    return F()._new((n,), dtype, device)


@functools.lru_cache(maxsize=None)
def _data(dtype, rows, cols, seed, scale=1.0):
    return dev(rnd((rows, cols), seed, scale), dtype)


# ---------------------------------------------------------------------------------------------------------------------------------------
# GEMM
# ---------------------------------------------------------------------------------------------------------------------------------------
EPILOGUES = ("none", "scale", "act", "act_bwd", "res")
SCALE = 0.25
# aux_in of the act_bwd epilogue.  gemm_bound_ok's bound is proportional to |act'(h)|, which holds a float32 evaluation of
# gelu'(h) = Phi(h) + h phi(h) only where that sum is well conditioned.  It is not in two places: at h0 = -0.75179, where it changes sign
# (two terms of size 0.23 cancel: what util.quick_gelu_ref says of QuickGELU's derivative), and in the negative tail, where the fp32
# kernels form Phi(h) as 0.5 (1 + erff(h / sqrt 2)) like torch does and 1 + erf cancels (h = -4.18: gelu' = -2.5e-4 from terms of size 1).
# Among the 52800 normal values of a 200 x 264 aux_in a few fall within 1e-4 of h0 and the smallest is -4.18; test_gemm_epilogues_guarded
# has such values too, but its K = 1024 accumulation term covers them, and K = 70 and 328 here do not.  bf16 is safe either way (no grid
# point closer than 1.8e-3 to h0, the tail formed as erfc without cancellation).  So aux_in stays at or above -2 and 0.25 away from h0:
# |gelu'| >= 0.083 everywhere, and the 2^-18 |gelu'| that the fp32 bound allows (u_out + u_mid) is 5 x 2^-24 in absolute terms, several
# roundings of the size-1 terms.  Nothing else about the values is special: normal, fixed seed, the same for both dtypes and the plain twin.
GELU_GRAD_ROOT, GELU_GRAD_KEEPOUT, GELU_GRAD_TAIL = -0.7517915246935645, 0.25, -2.0


@functools.lru_cache(maxsize=None)
def _aux_in(dtype, M, N):
    h = np.maximum(rnd((M, N), 906), GELU_GRAD_TAIL)
    near = np.abs(h - GELU_GRAD_ROOT) < GELU_GRAD_KEEPOUT
    h[near] = GELU_GRAD_ROOT + np.where(h[near] >= GELU_GRAD_ROOT, GELU_GRAD_KEEPOUT, -GELU_GRAD_KEEPOUT)
    return dev(h, dtype)


def _gemm_call(dtype, M, N, K, al, bl, A, am, B, bm, cm, tile=0, stages=0, split=1, epi="none", H=None, R=None, gate=None):
    """One ff_gemm call: A / B flat device buffers addressed by am / bm, outputs into fresh -3.25 buffers laid out by cm, aux_in (H) and
    residual (R) given as logical (M, N) tensors and laid out by cm with 1e30 in the holes.  Assertion 1 happens here.  Returns the
    gathered (C, aux_out or None)."""
    ffi = _ffi()
    lib = ffi.lib()
    act = ffi.ACT_GELU if epi == "act" else ffi.ACT_NONE
    act_bwd = ffi.ACT_GELU if epi == "act_bwd" else ffi.ACT_NONE
    d = ffi.GemmDesc(ffi.dtype_code(dtype), M, N, K, al, bl, rc.c_map(am), rc.c_map(bm), rc.c_map(cm), SCALE if epi == "scale" else 1.0,
                     act, act_bwd, split, tile, stages)
    Hb = rc.scatter(H, cm, dtype, rc.OPERAND_FILL) if epi == "act_bwd" else None
    Rb = rc.scatter(R, cm, dtype, rc.OPERAND_FILL) if epi == "res" else None
    use_gate = epi in ("act_bwd", "res")
    with guarded_allocations() as g:
        Cb = rc.filled(cm, M, N, dtype, rc.OUTPUT_FILL, "cuda", alloc=_alloc)
        Xb = rc.filled(cm, M, N, dtype, rc.OUTPUT_FILL, "cuda", alloc=_alloc) if epi in ("act", "res") else None
        before = Cb.clone()
        ws = F()._empty_bytes(lib.ff_gemm_workspace_bytes(d), Cb.device)
        ffi.check(lib.ff_gemm(d, A.data_ptr(), B.data_ptr(), Cb.data_ptr(), ffi.ptr(Xb), ffi.ptr(Hb), ffi.ptr(Rb),
                              gate.data_ptr() if use_gate else None, ws.data_ptr(), ws.numel(), ffi.stream_handle(Cb.device)), "ff_gemm")
        g.check()
        what = (NAME[dtype], M, N, K, al, bl, tuple(am), tuple(bm), tuple(cm), tile, stages, split, epi)
        assert rc.holes_untouched(Cb, before, cm, M, N), f"{what}: C written outside its rows"
        assert Xb is None or rc.holes_untouched(Xb, before, cm, M, N), f"{what}: aux_out written outside its rows"
        return rc.gather(Cb, cm, M, N), (rc.gather(Xb, cm, M, N) if Xb is not None else None)


def _gemm_bounds(what, dtype, C_, aux, Al, Bl, al, bl, epi, H, R, gate):
    """assertion 3: the element bound of every output and, for bf16, the worst row"""
    def bound(got, name, **kw):
        ok, worst, idx = gemm_bound_ok(got, Al, Bl, a_layout=al, b_layout=bl, **kw)
        assert ok, f"{what} {name}: element {idx} is {worst:.3g} x its bound"

    def rows(got, ref, name):
        if dtype == BF16:
            worst, row = rel_rows(got, ref, (0,))
            assert worst < GEMM_ROW_TOL, f"{what} {name}: row {row} relative error {worst:.3g}"

    acc, _ = gemm_ref(Al, Bl, al, bl)
    g_ = float(np.tanh(as64(gate)[0])) if gate is not None else 1.0
    u_act = 2.0 ** -8 if dtype == BF16 else 2.0 ** -19
    u_out_act = None if dtype == BF16 else u_act
    u_pitch = None if dtype == BF16 else 2.0 ** -21
    if aux is not None:
        bound(aux, "aux_out")
        rows(aux, acc, "aux_out")
    if epi == "none":
        bound(C_, "C", u_out=u_pitch)
        rows(C_, acc, "C")
    elif epi == "scale":
        bound(C_, "C", scale=SCALE)
        rows(C_, SCALE * acc, "C")
    elif epi == "act":
        bound(C_, "C", epilogue=lambda a: (O.act_fwd(a, "gelu"), np.abs(O.act_bwd(np.ones_like(a), a, "gelu"))), u_mid=u_act, u_out=u_out_act)
        rows(C_, O.act_fwd(acc, "gelu"), "C")
    elif epi == "act_bwd":
        h = as64(H)
        dd = g_ * O.act_bwd(np.ones_like(h), h, "gelu")
        bound(C_, "C", epilogue=lambda a: (a * dd, np.abs(dd)), u_mid=u_act, u_out=u_out_act)
        rows(C_, acc * dd, "C")
    else:
        r = as64(R)
        bound(C_, "C", epilogue=lambda a: (r + g_ * a, np.full_like(a, g_)), u_out=u_pitch)
        rows(C_, r + g_ * acc, "C")


def _twin_map(m, cols, dtype):
    """the plain map of the twin call: contiguous rows - unless the pitch is off the vector grid, where contiguous rows could switch the
    vector loads back on: then the same pitch over padded rows"""
    vec = 8 if dtype == BF16 else 4
    return rc.plain(cols) if m.ld % vec == 0 and cols % vec == 0 else rc.plain(m.ld)


class _Operand:
    """a stored operand matrix (rows, cols) laid out by a map, and its twin"""

    def __init__(self, dtype, stored_rows, cols, m, seed, scale):
        seg_rows = min(stored_rows, m.rows_per_seg) if rc.is_broadcast(m) else stored_rows
        self.m, self.buf = m, rc.scatter(_data(dtype, seg_rows, cols, seed, scale), m, dtype, rc.OPERAND_FILL)
        self.logical = rc.gather(self.buf, m, stored_rows, cols)
        self.tm = _twin_map(m, cols, dtype)
        self.tbuf = rc.scatter(self.logical, self.tm, dtype, rc.OPERAND_FILL)


def _gemm_case(dtype, M, N, K, al, bl, a, b, cm, plans, epis=("none",)):
    """every plan x epilogue of one problem: the call through the maps (assertion 1), its plain twin (2), the float64 bounds (3)"""
    H, R = _aux_in(dtype, M, N), _data(dtype, M, N, 905, 1.0)
    gate = dev(np.array([0.7]), dtype)
    tcm = _twin_map(cm, N, dtype)
    for tile, stages, split in plans:
        for epi in epis:
            kw = dict(tile=tile, stages=stages, split=split, epi=epi, H=H, R=R, gate=gate)
            what = (NAME[dtype], (M, N, K), (al, bl), tuple(a.m), tuple(b.m), tuple(cm), tile, stages, split, epi)
            C_, aux = _gemm_call(dtype, M, N, K, al, bl, a.buf, a.m, b.buf, b.m, cm, **kw)
            Ct, auxt = _gemm_call(dtype, M, N, K, al, bl, a.tbuf, a.tm, b.tbuf, b.tm, tcm, **kw)
            assert _same_bits(C_, Ct), f"{what}: C differs from the plain twin's in {int((_bits(C_) != _bits(Ct)).sum())} elements"
            assert aux is None or _same_bits(aux, auxt), f"{what}: aux_out differs from the plain twin's"
            _gemm_bounds(what, dtype, C_, aux, a.logical, b.logical, al, bl, epi, H, R, gate if epi in ("act_bwd", "res") else None)


def _stored(layout, outer, k):
    """(stored rows, contiguous columns) of an operand: layout 0 keeps the contraction index contiguous"""
    return (outer, k) if layout == 0 else (k, outer)


A_TILES = (0, 64, 64002, 128, 128002, 6412, 128160, 128168, 256128, 3264, 256256)
A_CASES = [(bl, t) for bl in (0, 1) for t in A_TILES if bl == 0 or t not in (3264, 256256)]      # those two stage K-major operands only


@pytest.mark.parametrize("bl,tile", A_CASES)
def test_gemm_segmented_a_rows(bl, tile):
    """(a) the to_q form: A K-major with its M rows segmented (40-row segments, 57 foreign rows between them), plain B in both layouts, on
    every forced tile and the planner's own; split-K 1 and 3; the default ring depth, and 4 stages where the tile takes a ring depth."""
    M, N, K = 200, 264, 328
    a = _Operand(BF16, M, K, _seg(K + 8), 11, 0.5)
    b = _Operand(BF16, *_stored(bl, N, K), rc.plain((K if bl == 0 else N) + 16), 12, 0.05)
    plans = [(tile, 0, 1), (tile, 0, 3)] + ([(tile, 4, 1), (tile, 4, 3)] if tile in (64, 128, 6412, 128160, 128168) else [])
    _gemm_case(BF16, M, N, K, 0, bl, a, b, rc.plain(N), plans)


@pytest.mark.parametrize("tile", [0, 128, 128002, 128160, 256128, 256256, 3264, 64002])
def test_gemm_broadcast_a(tile):
    """(b) one 40-row segment serves all 200 logical rows of A (seg_stride = 0, the latents repeated over the batch)."""
    M, N, K = 200, 264, 328
    a = _Operand(BF16, M, K, rc.Map(K + 8, 0, SEG), 21, 0.5)
    assert a.buf.numel() == (SEG - 1) * (K + 8) + K
    b = _Operand(BF16, N, K, rc.plain(K), 22, 0.05)
    _gemm_case(BF16, M, N, K, 0, 0, a, b, rc.plain(N), [(tile, 0, 1), (tile, 0, 3)])


@pytest.mark.parametrize("tile", [0, 3216, 3264])
@pytest.mark.parametrize("K", [320, 1312])
def test_gemm_segmented_a_rows_decode(K, tile):
    """(c) M <= 32: 20 rows in segments of 8, the weight-streaming kernel (3216: a_map.off(c) / a_map.off(16 + c), K % 32 == 0 holds for
    both K) and the 32 x 64 tile; the planner picks 3216 at K = 320 and 3264 at K = 1312."""
    M, N = 20, 132
    a = _Operand(BF16, M, K, _seg(K + 8, 8), 31, 0.5)
    b = _Operand(BF16, N, K, rc.plain(K), 32, 0.05)
    _gemm_case(BF16, M, N, K, 0, 0, a, b, rc.plain(N), [(tile, 0, 1), (tile, 0, 2)])


@pytest.mark.parametrize("tile", [0, 64, 64002, 128, 128002, 6412, 256128])
@pytest.mark.parametrize("maps,bl", [("a-seg", 0), ("a-seg", 1), ("b-seg", 1), ("both-seg", 1)])
def test_gemm_segmented_k_rows(maps, bl, tile):
    """(d) the weight-gradient form: A stored [K][M] with its K rows segmented (d Wq = dQs^T . LN(latents) reads the latent rows of kv_in
    as the contraction index), B stored [K][N] segmented as well, with another gap.  K = 200 = 5 segments of 40: every 64-element k-step
    straddles a segment, and the second of two K splits starts at k = 128, inside one."""
    M, N, K = 264, 136, 200
    a = _Operand(BF16, K, M, _seg(M + 8) if maps != "b-seg" else rc.plain(M), 41, 0.5)
    bm = _seg(N + 8, SEG, 23) if maps != "a-seg" else rc.plain((K if bl == 0 else N))
    b = _Operand(BF16, *_stored(bl, N, K), bm, 42, 0.05)
    _gemm_case(BF16, M, N, K, 1, bl, a, b, rc.plain(N), [(tile, 0, 1), (tile, 0, 2)])


@pytest.mark.parametrize("tile", [0, 128160, 128168, 128002, 256128])
def test_gemm_segmented_k_rows_of_b_only(tile):
    """(d) A K-major and plain, B stored [K][N] with segmented K rows: the 128 x 160 tile's split 128 + 32 staging (BStage<160, 1>) on its
    per-k-step path, with four and eight MFMA waves."""
    M, N, K = 264, 136, 200
    a = _Operand(BF16, M, K, rc.plain(K), 43, 0.5)
    b = _Operand(BF16, K, N, _seg(N + 8, SEG, 23), 42, 0.05)
    _gemm_case(BF16, M, N, K, 0, 1, a, b, rc.plain(N), [(tile, 0, 1), (tile, 0, 2), (tile, 4, 1)])


@pytest.mark.parametrize("split", [1, 3])
@pytest.mark.parametrize("N,pad", [(264, 36), (132, 36), (264, 40)])
@pytest.mark.parametrize("dtype,tile", [(BF16, 0), (BF16, 128002), (BF16, 128160), (BF16, 256256), (F32, 0)],
                         ids=["bf16-planner", "bf16-128002", "bf16-128160", "bf16-256256", "f32"])
def test_gemm_segmented_c(dtype, tile, N, pad, split):
    """(e) C, aux_out, aux_in and the residual through a segmented c_map, every epilogue, in the tile epilogue (split 1) and in the
    split-K epilogue kernel (split 3).  N = 132 takes the element-wise pieces; so does pitch N + 36 in bf16 (300 and 168 are no multiples
    of 8), pitch 264 + 40 takes the 16-byte pieces in both types."""
    M, K = 200, 328
    a = _Operand(dtype, M, K, rc.plain(K), 51, 0.5)
    b = _Operand(dtype, N, K, rc.plain(K), 52, 0.05)
    _gemm_case(dtype, M, N, K, 0, 0, a, b, _seg(N + pad), [(tile, 0, split)], EPILOGUES)


@pytest.mark.parametrize("split", [1, 3])
@pytest.mark.parametrize("al,bl", [(0, 0), (0, 1), (1, 0), (1, 1)])
def test_gemm_fp32_scalar_paths(al, bl, split):
    """(f) fp32 with nothing vectorised: K = 70, pitches of K + 3 (M + 3, N + 3 for the operands stored the other way round) and odd
    segment strides - (a) with A's stored rows segmented, then (e) with a segmented C of odd pitch and every epilogue.  The twins keep
    the unaligned pitches (plain maps over padded rows), so both calls take the scalar path."""
    M, N, K = 200, 264, 70
    ar, ac = _stored(al, M, K)
    br, bc = _stored(bl, N, K)
    a = _Operand(F32, ar, ac, _seg(ac + 3), 61, 0.5)
    b = _Operand(F32, br, bc, rc.plain(bc + 3), 62, 0.05)
    assert a.m.seg_stride % 2 == 1 and a.tm.ld == a.m.ld and b.tm.ld == b.m.ld
    _gemm_case(F32, M, N, K, al, bl, a, b, rc.plain(N), [(0, 0, split)])
    ap = _Operand(F32, ar, ac, rc.plain(ac + 3), 61, 0.5)
    for n in (264, 132):
        bb = _Operand(F32, *_stored(bl, n, K), rc.plain(_stored(bl, n, K)[1] + 3), 63, 0.05)
        cm = _seg(n + 37)
        assert cm.ld % 2 == 1 and cm.seg_stride % 2 == 1 and _twin_map(cm, n, F32).ld == cm.ld
        _gemm_case(F32, M, n, K, al, bl, ap, bb, cm, [(0, 0, split)], EPILOGUES)


@pytest.mark.parametrize("which", ["a-stride", "b-stride", "a-span", "b-span"])
def test_gemm_refuses_unaligned_and_oversized_maps(which):
    """(g) host-side refusals: a bf16 operand map whose seg_stride is no multiple of 8 elements, and one whose last row lies 2^30 elements
    or more from the base (32-bit buffer offsets), return FF_ERR_UNSUPPORTED before anything is launched: C stays bit for bit.  The span
    check precedes every access, so the huge operand is never allocated."""
    ffi = _ffi()
    lib = ffi.lib()
    M, N, K = 200, 264, 328
    am, bm = (_seg(K + 8), rc.plain(K))
    if which == "a-stride":
        am = rc.Map(K + 8, 97 * (K + 8) + 4, SEG)
    elif which == "b-stride":
        bm = rc.Map(K + 8, 97 * (K + 8) + 4, SEG)
    elif which == "a-span":
        am = rc.Map(K + 8, 1 << 28, SEG)                      # row 160 starts at 2^30
    else:
        bm = rc.Map(K + 8, 1 << 28, SEG)
    small = torch.zeros(rc.span(_seg(K + 8), N, K), dtype=BF16, device="cuda")
    for tile, split in ((0, 1), (128002, 3)):
        d = ffi.GemmDesc(ffi.DTYPE_BF16, M, N, K, 0, 0, rc.c_map(am), rc.c_map(bm), ffi.rowmap(N), 1.0, ffi.ACT_NONE, ffi.ACT_NONE, split, tile, 0)
        with guarded_allocations() as g:
            C_ = F()._new((M, N), BF16, small.device).fill_(rc.OUTPUT_FILL)
            before = C_.clone()
            ws = F()._empty_bytes(lib.ff_gemm_workspace_bytes(d), small.device)
            rcode = lib.ff_gemm(d, small.data_ptr(), small.data_ptr(), C_.data_ptr(), None, None, None, None, ws.data_ptr(), ws.numel(),
                                ffi.stream_handle(small.device))
            g.check()
        assert rcode == FF_ERR_UNSUPPORTED, (which, tile, split, rcode, lib.ff_last_error())
        assert _same_bits(C_, before), (which, tile, split)


# ---------------------------------------------------------------------------------------------------------------------------------------
# LayerNorm and rows_reduce: the resampler's kv_in geometry
# ---------------------------------------------------------------------------------------------------------------------------------------
LB, LT, LV, LQ = 3, 2, 25, 24
LF, LR = LT * LV, LT * LV + LQ            # 50 media rows + 24 latent rows per sample: 150 media rows, 72 latent rows
LN_COLS = [(F32, 256), (F32, 36), (F32, 2560), (BF16, 256), (BF16, 36), (BF16, 2048)]
LN_IDS = [f"{NAME[d]}-c{c}" for d, c in LN_COLS]


def _kv_maps(D):
    """(media rows, latent rows and their base) inside one (batch, R, D) buffer"""
    return rc.Map(D, LR * D, LF), rc.Map(D, LR * D, LQ), LF * D


def _ptr(t, base=0):
    return t.data_ptr() + base * t.element_size()


def _ln_desc(dtype, rows, cols, xm, ym, dxm=None, add=False, stats_given=0):
    ffi = _ffi()
    return ffi.LnDesc(ffi.dtype_code(dtype), rows, cols, rc.c_map(xm), rc.c_map(ym), rc.c_map(dxm if dxm is not None else rc.plain(cols)),
                      LF if add else 0, LV if add else 0, 1e-5, stats_given)


def _ln_fwd(dtype, rows, D, x, xm, ybuf, ym, ybase, tpe, g, b, stats=None, want_y=True):
    """ff_layernorm_fwd into ybuf (None: a fresh plain buffer); returns (y buffer or None, mean, rstd)"""
    ffi = _ffi()
    d = _ln_desc(dtype, rows, D, xm, ym, add=tpe is not None, stats_given=1 if stats is not None else 0)
    if want_y and ybuf is None:
        ybuf = F()._new((rows * D,), dtype, x.device)
    mean, rstd = stats if stats is not None else (F()._new(rows, F32, x.device), F()._new(rows, F32, x.device))
    ffi.check(ffi.lib().ff_layernorm_fwd(d, x.data_ptr(), ffi.ptr(tpe), g.data_ptr(), b.data_ptr(), _ptr(ybuf, ybase) if want_y else None,
                                         mean.data_ptr(), rstd.data_ptr(), ffi.stream_handle(x.device)), "ff_layernorm_fwd")
    return (ybuf if want_y else None), mean, rstd


def _ln_inputs(dtype, D):
    x = dev(rnd((LB * LF, D), 1, 2.0), dtype)
    lat = dev(rnd((LQ, D), 6, 2.0), dtype)
    tpe = dev(rnd((4, D), 2), dtype)
    g, b = dev(1 + 0.2 * rnd((D,), 3), dtype), dev(0.1 * rnd((D,), 4), dtype)
    return x, lat, tpe, g, b


def _ln_rows(got, ref, dtype, kind, what):
    worst, row = rel_rows(got, ref, (0,))
    assert worst < ROW_TOL[dtype][kind], f"{what}: row {row} relative error {worst:.3g}"


def _x_media64(x, tpe):
    """x + time_pos_emb[(r % F) / v] in float64, the rows the addend descriptor (add_rows_per_seg = F, add_div = v) describes"""
    rows = x.shape[0]
    return as64(x) + as64(tpe)[(np.arange(rows) % LF) // LV]


@pytest.mark.parametrize("dtype,D", LN_COLS, ids=LN_IDS)
def test_layernorm_fwd_into_interleaved_rows(dtype, D):
    """Forward into kv_in: the media rows (x plain + the time-embedding addend, y_map = {D, R D, F}) in one call, as statistics only
    (y = NULL) and then with stats_given; the latent rows (x broadcast {D, 0, q}, y_map = {D, R D, q} at base F D) after the media rows
    and before them: each call leaves the other kind's rows bit for bit as they were."""
    x, lat, tpe, g, b = _ln_inputs(dtype, D)
    mm, lm, lbase = _kv_maps(D)
    nm, nl, total = LB * LF, LB * LQ, LB * LR * D
    bc = rc.Map(D, 0, LQ)
    with guarded_allocations() as gd:
        kv = _alloc(total, dtype, "cuda").fill_(rc.OUTPUT_FILL)
        empty = kv.clone()
        # media rows, three ways
        _, mean, rstd = _ln_fwd(dtype, nm, D, x, rc.plain(D), kv, mm, 0, tpe, g, b)
        gd.check()
        assert rc.holes_untouched(kv, empty, mm, nm, D), "media rows: the latent rows of kv_in were written"
        after_media = kv.clone()
        _, mean2, rstd2 = _ln_fwd(dtype, nm, D, x, rc.plain(D), None, mm, 0, tpe, g, b, want_y=False)
        assert torch.equal(mean.view(torch.int32), mean2.view(torch.int32)) and torch.equal(rstd.view(torch.int32), rstd2.view(torch.int32))
        kv2 = _alloc(total, dtype, "cuda").fill_(rc.OUTPUT_FILL)
        _ln_fwd(dtype, nm, D, x, rc.plain(D), kv2, mm, 0, tpe, g, b, stats=(mean2, rstd2))
        gd.check()
        assert _same_bits(kv2, after_media), "statistics-only + stats_given differs from the one-call form"
        assert torch.equal(mean.view(torch.int32), mean2.view(torch.int32)), "stats_given rewrote the statistics"
        # plain twin
        yt, meant, rstdt = _ln_fwd(dtype, nm, D, x, rc.plain(D), None, rc.plain(D), 0, tpe, g, b)
        y_media = rc.gather(kv, mm, nm, D)
        assert _same_bits(y_media, yt.view(nm, D)) and torch.equal(mean, meant) and torch.equal(rstd, rstdt), "media rows differ from the plain twin"
        # latent rows after the media rows
        _, lmean, lrstd = _ln_fwd(dtype, nl, D, lat, bc, kv, lm, lbase, None, g, b)
        gd.check()
        assert rc.holes_untouched(kv, after_media, lm, nl, D, base=lbase), "latent rows: the media rows of kv_in did not survive"
        y_lat = rc.gather(kv, lm, nl, D, base=lbase)
        latx = rc.gather(lat, bc, nl, D).contiguous()
        ylt, lmeant, lrstdt = _ln_fwd(dtype, nl, D, latx, rc.plain(D), None, rc.plain(D), 0, None, g, b)
        assert _same_bits(y_lat, ylt.view(nl, D)) and torch.equal(lmean, lmeant) and torch.equal(lrstd, lrstdt), "latent rows differ from the plain twin"
        # the other order: latent rows first, then the media rows around them
        kv3 = _alloc(total, dtype, "cuda").fill_(rc.OUTPUT_FILL)
        _ln_fwd(dtype, nl, D, lat, bc, kv3, lm, lbase, None, g, b)
        gd.check()
        assert rc.holes_untouched(kv3, empty, lm, nl, D, base=lbase), "latent rows: the media rows of kv_in were written"
        after_lat = kv3.clone()
        _ln_fwd(dtype, nm, D, x, rc.plain(D), kv3, mm, 0, tpe, g, b)
        gd.check()
        assert rc.holes_untouched(kv3, after_lat, mm, nm, D), "media rows: the latent rows of kv_in did not survive"
        assert _same_bits(kv3, kv), "the two orders give different kv_in buffers"
    t = TOL[dtype]
    xm64 = _x_media64(x, tpe)
    yr, cache = O.layernorm_fwd(xm64, as64(g), as64(b))
    assert rel(y_media, yr) < t["out"]
    _ln_rows(y_media, yr, dtype, "out", "media y")
    assert np.allclose(as64(mean), xm64.mean(-1), rtol=1e-5, atol=1e-5) and np.allclose(as64(rstd), cache[1][:, 0], rtol=1e-4)
    ylr, lcache = O.layernorm_fwd(as64(latx), as64(g), as64(b))
    assert rel(y_lat, ylr) < t["out"]
    _ln_rows(y_lat, ylr, dtype, "out", "latent y")
    assert np.allclose(as64(lmean), as64(latx).mean(-1), rtol=1e-5, atol=1e-5) and np.allclose(as64(lrstd), lcache[1][:, 0], rtol=1e-4)


def _ln_bwd(dtype, rows, D, dy, ym, ybase, x, xm, tpe, g, mean, rstd, res, alias):
    """ff_layernorm_bwd with a plain dx_map and dx_residual (alias: dx starts as the residual and is passed as both); the workspace has
    the size ff_layernorm_bwd_workspace_bytes gives.  Returns (dx, dgamma, dbeta)."""
    ffi = _ffi()
    lib = ffi.lib()
    d = _ln_desc(dtype, rows, D, xm, ym, rc.plain(D), add=tpe is not None, stats_given=1)
    dx = F()._new((rows, D), dtype, x.device)
    if alias:
        dx.copy_(res)
    dg, db = F()._new((D,), dtype, x.device), F()._new((D,), dtype, x.device)
    ws = F()._empty_bytes(lib.ff_layernorm_bwd_workspace_bytes(d), x.device)
    ffi.check(lib.ff_layernorm_bwd(d, _ptr(dy, ybase), x.data_ptr(), ffi.ptr(tpe), g.data_ptr(), mean.data_ptr(), rstd.data_ptr(), dx.data_ptr(),
                                   dx.data_ptr() if alias else res.data_ptr(), dg.data_ptr(), db.data_ptr(), ws.data_ptr(), ws.numel(),
                                   ffi.stream_handle(x.device)), "ff_layernorm_bwd")
    return dx, dg, db


@pytest.mark.parametrize("kind", ["media-rows", "latent-rows"])
@pytest.mark.parametrize("dtype,D", LN_COLS, ids=LN_IDS)
def test_layernorm_bwd_dy_through_interleaved_rows(dtype, D, kind):
    """Backward with dy read through the segmented y_map out of a kv_in-shaped buffer whose other rows hold 1e30: the fused one-pass kernel
    (256 columns; 36 in fp32; 2048 in bf16), the unfused ln_bwd_dx_kernel + col_reduce_kernel (2560 fp32 columns = 10 chunks; 36 bf16
    columns, element-wise), x plain or broadcast, with and without the addend, dx apart from dx_residual and aliasing it."""
    x, lat, tpe, g, b = _ln_inputs(dtype, D)
    mm, lm, lbase = _kv_maps(D)
    media = kind == "media-rows"
    rows, ym, ybase, rps = (LB * LF, mm, 0, LF) if media else (LB * LQ, lm, lbase, LQ)
    dy_l = dev(rnd((rows, D), 4), dtype)
    res = dev(rnd((rows, D), 5), dtype)
    dybuf = rc.scatter(dy_l, ym, dtype, rc.OPERAND_FILL, base=ybase)
    dy_before = dybuf.clone()
    for bcast in (False, True):
        xm = rc.Map(D, 0, rps) if bcast else rc.plain(D)
        xsrc = (x[:rps] if media else lat) if bcast else (x if media else dev(rnd((rows, D), 7, 2.0), dtype))
        xl = rc.gather(xsrc, xm, rows, D).contiguous()
        for add in (tpe, None):
            x64 = _x_media64(xl, tpe) if add is not None else as64(xl)
            _, cache = O.layernorm_fwd(x64, as64(g), as64(b))
            dxr, dgr, dbr = O.layernorm_bwd(as64(dy_l), cache, as64(g))
            for alias in (False, True):
                what = (NAME[dtype], D, kind, "x-broadcast" if bcast else "x-plain", "addend" if add is not None else "no-addend",
                        "dx-aliases-residual" if alias else "dx-apart")
                with guarded_allocations() as gd:
                    _, mean, rstd = _ln_fwd(dtype, rows, D, xl, rc.plain(D), None, rc.plain(D), 0, add, g, b, want_y=False)
                    dx, dg, db = _ln_bwd(dtype, rows, D, dybuf, ym, ybase, xsrc, xm, add, g, mean, rstd, res, alias)
                    gd.check()
                    assert _same_bits(dybuf, dy_before), f"{what}: dy was written"
                    dxt, dgt, dbt = _ln_bwd(dtype, rows, D, dy_l, rc.plain(D), 0, xl, rc.plain(D), add, g, mean, rstd, res, alias)
                    gd.check()
                assert _same_bits(dx, dxt) and _same_bits(dg, dgt) and _same_bits(db, dbt), f"{what}: differs from the plain twin"
                t = TOL[dtype]
                assert rel(dx, dxr + as64(res)) < t["grad"], what
                _ln_rows(dx, dxr + as64(res), dtype, "grad", f"{what} dx")
                assert rel(dg, dgr) < t["grad"] and rel(db, dbr) < t["grad"], what
                _ln_rows(dg.reshape(1, -1), dgr.reshape(1, -1), dtype, "grad", f"{what} dgamma")
                _ln_rows(db.reshape(1, -1), dbr.reshape(1, -1), dtype, "grad", f"{what} dbeta")


def _rows_reduce(dtype, rows, D, x, xm, xbase, rpb, rpg):
    ffi = _ffi()
    lib = ffi.lib()
    d = ffi.ReduceDesc(ffi.dtype_code(dtype), rows, D, rc.c_map(xm), rpb, rpg)
    out = F()._new((rpb // rpg, D), dtype, x.device)
    ws = F()._empty_bytes(lib.ff_rows_reduce_workspace_bytes(d), x.device)
    ffi.check(lib.ff_rows_reduce(d, _ptr(x, xbase), out.data_ptr(), ws.data_ptr(), ws.numel(), ffi.stream_handle(x.device)), "ff_rows_reduce")
    return out


@pytest.mark.parametrize("dtype,D", LN_COLS, ids=LN_IDS)
def test_rows_reduce_over_interleaved_rows(dtype, D):
    """ff_rows_reduce over the media rows of a kv_in-shaped buffer (the d time_pos_emb pattern: groups of v rows per frame) and over its
    latent rows (the d latents pattern: one group per latent); the other kind's rows hold 1e30."""
    mm, lm, lbase = _kv_maps(D)
    for name, rows, m, base, rpb, rpg, shape, axes in (("media", LB * LF, mm, 0, LF, LV, (LB, LT, LV, D), (0, 2)),
                                                       ("latent", LB * LQ, lm, lbase, LQ, 1, (LB, LQ, D), (0,))):
        xl = dev(rnd((rows, D), 8), dtype)
        buf = rc.scatter(xl, m, dtype, rc.OPERAND_FILL, base=base)
        before = buf.clone()
        with guarded_allocations() as gd:
            out = _rows_reduce(dtype, rows, D, buf, m, base, rpb, rpg)
            gd.check()
            twin = _rows_reduce(dtype, rows, D, xl, rc.plain(D), 0, rpb, rpg)
            gd.check()
        assert _same_bits(buf, before), f"{name}: the operand was written"
        assert _same_bits(out, twin), f"{name}: differs from the plain twin"
        ref = as64(xl).reshape(shape).sum(axes)
        assert rel(out, ref) < TOL[dtype]["grad"], name
        _ln_rows(out, ref, dtype, "grad", f"{name} rows")


# ---------------------------------------------------------------------------------------------------------------------------------------
# the resampler where segments and tiles disagree
# ---------------------------------------------------------------------------------------------------------------------------------------
#            dim, depth, heads, dim_head, q, T, v, batch
RS_CASES = {"q40-R140": (256, 2, 4, 64, 40, 2, 50, 3),            # every tile edge falls inside a segment
            "vit-tokens-q24": (128, 1, 2, 64, 24, 1, 257, 2),     # ViT token count with few latents
            "q100": (512, 2, 8, 64, 100, 3, 17, 2),               # more than 64 queries; segments longer than a tile
            "dh128-q72": (256, 1, 2, 128, 72, 1, 33, 2)}          # dim_head 128
RS_PARAMS = [(n, d) for n in RS_CASES for d in ((BF16, F32) if n in ("q40-R140", "vit-tokens-q24") else (BF16,))]


def _resampler_both_ways(name, dtype, dims):
    """forward + backward, stack-level and layer by layer, inside the guards, against the float64 oracle: whole-tensor TOL on y, d x and
    every parameter gradient, the worst row of y per (sample, latent) and of d x per (sample, frame, token), the two call forms against
    each other (outputs bit for bit, gradients within 1e-3 as between two plans of one product in test_hip_primitives.py)."""
    from test_hip_modules import build_resampler
    dim, depth, heads, dh, q, T, v, b = dims
    nte, ffm = 4, 4
    p = resampler_params(dim, depth, heads, dh, q, nte, ffm, tag="rowmaps" + name)
    m = build_resampler(p, dim, depth, heads, dh, q, nte, ffm, "gelu", dtype)
    xd = dev(det((b, T, v, dim), name + "-x"), dtype)
    dyd = dev(det((b, q, dim), name + "-dy"), dtype)
    p64 = {k: as64(t) for k, t in m.state_dict().items()}
    yr, cache = O.resampler_fwd(as64(xd), p64, heads=heads, dim_head=dh)
    dxr, gr = O.resampler_bwd(as64(dyd), cache, p64, heads=heads, dim_head=dh)
    t, rt = TOL[dtype], RS_ROW_TOL[dtype]
    got = {}
    for layerwise in (False, True):
        m.layerwise = layerwise
        m.zero_grad(set_to_none=True)
        xi = xd.clone().requires_grad_(True)
        with guarded_allocations() as g:
            y = m(xi)
            y.backward(dyd)
            g.check()
        what = (name, NAME[dtype], "layer-by-layer" if layerwise else "stack-level")
        assert rel(y, yr) < t["out"], what
        assert rel(xi.grad, dxr) < t["grad"], what
        grads = {k: prm.grad.detach().clone() for k, prm in m.named_parameters()}
        for k, gk in grads.items():
            assert rel(gk, gr[k]) < t["grad"], (what, k)
        worst, row = rel_rows(y, yr, (0, 1))
        assert worst < rt["out"], f"{what}: y row {row} relative error {worst:.3g}"
        worst, row = rel_rows(xi.grad, dxr, (0, 1, 2))
        assert worst < rt["grad"], f"{what}: dx row {row} relative error {worst:.3g}"
        got[layerwise] = (y.detach().clone(), xi.grad.detach().clone(), grads)
    assert _same_bits(got[False][0], got[True][0]), f"{name}: stack-level and layer-by-layer outputs differ"
    assert rel(got[True][1], got[False][1]) < 1e-3, name
    for k in got[False][2]:
        assert rel(got[True][2][k], got[False][2][k]) < 1e-3, (name, k)


@pytest.mark.parametrize("name,dtype", RS_PARAMS, ids=[f"{n}-{NAME[d]}" for n, d in RS_PARAMS])
def test_resampler_segments_off_the_tile_grid(name, dtype):
    """Layer 0 runs the broadcast latents as LayerNorm input and as the GEMM residual map, which the C ABI (residual through c_map) cannot
    reach; every layer runs kv_media / kv_lat with 40, 24, 100 or 72 latent rows per sample."""
    _resampler_both_ways(name, dtype, RS_CASES[name])


@pytest.mark.parametrize("name", list(RS_CASES))
def test_resampler_aligned_twin_rows(name):
    """The bf16 cases' aligned twins - the same dims with 64 latents and 64 tokens per frame, every segment edge a tile edge - under the
    same assertions: what RS_ROW_TOL is established from (FF_TOL_REPORT writes every worst row as a [rows] entry)."""
    dim, depth, heads, dh, _, T, _, b = RS_CASES[name]
    _resampler_both_ways(name + "-aligned", BF16, (dim, depth, heads, dh, 64, T, 64, b))
