"""Tile edges, unwritten elements and writes past the end, on the MI355X.

Everything here runs under tests/guarded.py's guarded_allocations(): each buffer the library allocates sits between guard bands holding a
finite sentinel, and its body starts as NaN (floating point) or 0xA5 bytes.  After every call the guards are compared bit for bit, and the
results are held to float64 references with the whole-tensor `rel` of the parity tests PLUS the per-row `rel_rows` and, for the GEMM, the
element-wise `gemm_bound_ok` (tests/util.py) - errors confined to one tile or a few rows do not drown in the rest of the tensor.

Row tolerances (worst row's relative L2 error), set like util.TOL from errors measured on an MI355X (FF_TOL_REPORT + tools/tol_report.py,
the [rows] entries) with a 1.3-2x margin - see ROW_TOL."""
import os
import sys

import numpy as np
import pytest
import torch

from attn_cases import attention_ref
from guarded import guarded_allocations
from oracle import flamingo_oracle as O
from util import TOL, as64, attn_bound_ok, dev, gemm_bound_ok, gemm_ref, rel, rel_rows, rnd

pytestmark = pytest.mark.gpu
BF16, F32 = torch.bfloat16, torch.float32
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

# Worst-row relative L2 error bounds, measured on an MI355X over this file (FF_TOL_REPORT, the [rows] entries) with a 1.5-2x margin:
#   fp32: <= 1.67e-6 (attention rows, n_kv 321, one query)                                                     -> 2.5e-6
#   bf16: <= 7.3e-3 (fused cross-attention block, (sample, token) rows of out - y and d y); attention rows <= 5.4e-3,
#         LayerNorm / rows_reduce rows <= 2.3e-3                                                              -> 1.2e-2
#   bf16 GEMM output rows (one rounding of an fp32 accumulator): <= 1.89e-3                                   -> GEMM_ROW_TOL 3e-3
# "out" / "grad" are kept apart for the callers' sake; the measurements did not call for different values.
ROW_TOL = {F32: dict(out=2.5e-6, grad=2.5e-6), BF16: dict(out=1.2e-2, grad=1.2e-2)}
GEMM_ROW_TOL = 3e-3


def F():
    from flamingo_mini_amd import functional
    return functional


def _bound(C_, A, B, what, **kw):
    ok, worst, idx = gemm_bound_ok(C_, A, B, **kw)
    assert ok, f"{what}: element {idx} is {worst:.3g} x its bound"


def _rows(got, ref, axes, dtype, kind, what):
    worst, row = rel_rows(got, ref, axes)
    assert worst < ROW_TOL[dtype][kind], f"{what}: row {row} relative error {worst:.3g}"


def _act_epi(act):
    return lambda acc: (O.act_fwd(acc, act), np.abs(O.act_bwd(np.ones_like(acc), acc, act)))


# ---------------------------------------------------------------------------------------------------------------------------------------
# GEMM
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("al,bl", [(0, 0), (0, 1), (1, 0), (1, 1)])
def test_gemm_every_tile_guarded(al, bl):
    """test_hip_primitives.py::test_gemm_every_instantiated_tile under the guards: every forced tile x stages x split-K, plus the planner's
    own choice (tile=0), on the ragged 408 x 424 x 328 problem (partial tiles in M and N, a K tail of 8).  Each call's C is fresh poison, so a
    tile plan that skipped the ragged last row / column tile leaves NaN; an overrun hits a guard; a dropped k-step fails the element bound."""
    M, N, K = 408, 424, 328
    A = dev(rnd((M, K) if al == 0 else (K, M), 11), BF16)
    B = dev(rnd((N, K) if bl == 0 else (K, N), 12), BF16)
    acc, _ = gemm_ref(A, B, al, bl)
    tiles = (128, 6412, 64, 64002, 128002, 256128) + ((128160, 128168) if al == 0 else ()) + ((256256, 3264) if (al, bl) == (0, 0) else ())
    with guarded_allocations() as g:
        plans = [(0, 0, 0), (0, 0, 2)] + [(t, s, k) for t in tiles for s in (2, 3, 4) for k in (1, 2)]
        for tile, stages, split in plans:
            C_ = F().gemm(A, B, a_layout=al, b_layout=bl, split_k=split, tile=tile, stages=stages)
            what = (tile, stages, split)
            g.check()
            assert rel(C_, acc) < 1e-2, what
            worst, row = rel_rows(C_, acc, (0,))
            assert worst < GEMM_ROW_TOL, f"{what}: row {row} relative error {worst:.3g}"
            _bound(C_, A, B, what, a_layout=al, b_layout=bl)
            g.clear()


@pytest.mark.parametrize("tile", [0, 3264], ids=["weight-streaming", "32x64-tiles"])
def test_gemm_decode_rows_guarded(tile):
    """M in {1, 5, 17, 32} with a partial last column group (N % 16 = 4) and K tails, every epilogue of the decode products, element bound."""
    kw = dict(tile=tile) if tile else {}
    gate = dev(np.array([0.7]), BF16)
    g_ = float(np.tanh(as64(gate)[0]))
    with guarded_allocations() as g:
        for M in (1, 5, 17, 32):
            for N, K in ((1284, 1312), (1284, 1304), (1280, 5120)):
                A, B = dev(rnd((M, K), 51, 0.5), BF16), dev(rnd((N, K), 52, 0.05), BF16)
                H, R = dev(rnd((M, N), 53), BF16), dev(rnd((M, N), 54), BF16)
                h, r = as64(H), as64(R)
                C_, aux = F().gemm(A, B, residual=R, gate=gate, want_aux_out=True, **kw)
                _bound(aux, A, B, ("aux", M, N, K))
                _bound(C_, A, B, ("residual", M, N, K), epilogue=lambda a: (r + g_ * a, np.full_like(a, g_)))
                for act in ("gelu", "sqrelu", "relu"):
                    C_, aux = F().gemm(A, B, act=act, want_aux_out=True, **kw)
                    _bound(aux, A, B, ("act aux", act, M, N, K))
                    _bound(C_, A, B, ("act", act, M, N, K), epilogue=_act_epi(act), u_mid=2.0 ** -8)
                    C_ = F().gemm(A, B, act_bwd=act, aux_in=H, gate=gate, **kw)
                    d = g_ * O.act_bwd(np.ones_like(h), h, act)
                    _bound(C_, A, B, ("act_bwd", act, M, N, K), epilogue=lambda a: (a * d, np.abs(d)), u_mid=2.0 ** -8)
                C_ = F().gemm(A, B, scale=0.125, **kw)
                _bound(C_, A, B, ("scale", M, N, K), scale=0.125)
                g.check()
                g.clear()


@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("split_k", [0, 3])
def test_gemm_epilogues_guarded(dtype, split_k):
    """Every epilogue (activation + saved pre-activation, activation gradient x aux_in x gate, gated residual, scale) on a ragged problem
    (N % 8 = 4: element-wise epilogue pieces; partial row tile), held element by element."""
    M, N, K = 136, 132, 1024
    A, B = dev(rnd((M, K), 3, 0.5), dtype), dev(rnd((N, K), 4, 0.05), dtype)
    H, R = dev(rnd((M, N), 6), dtype), dev(rnd((M, N), 5), dtype)
    gate = dev(np.array([0.7]), dtype)
    h, r, g_ = as64(H), as64(R), float(np.tanh(as64(gate)[0]))
    u_act = 2.0 ** -8 if dtype == BF16 else 2.0 ** -19        # the fp32 activations (erff / expf) carry a few ulp of their own
    u_out = None if dtype == BF16 else u_act                    # (None: gemm_bound_ok's bf16 default)
    with guarded_allocations() as g:
        for act in ("gelu", "sqrelu", "relu"):
            C_, aux = F().gemm(A, B, act=act, want_aux_out=True, split_k=split_k)
            _bound(aux, A, B, ("aux", act))
            _bound(C_, A, B, ("act", act), epilogue=_act_epi(act), u_mid=u_act, u_out=u_out)
            C_ = F().gemm(A, B, act_bwd=act, aux_in=H, gate=gate, split_k=split_k)
            d = g_ * O.act_bwd(np.ones_like(h), h, act)
            _bound(C_, A, B, ("act_bwd", act), epilogue=lambda a: (a * d, np.abs(d)), u_mid=u_act, u_out=u_out)
        C_, aux = F().gemm(A, B, residual=R, gate=gate, want_aux_out=True, split_k=split_k)
        _bound(aux, A, B, "residual aux")
        _bound(C_, A, B, "residual", epilogue=lambda a: (r + g_ * a, np.full_like(a, g_)), u_out=u_out)
        _bound(F().gemm(A, B, scale=0.25, split_k=split_k), A, B, "scale", scale=0.25)
        g.check()


def _padded(rows, cols, ld, dtype, seed, scale, fill):
    """a (rows, ld) buffer whose first `cols` columns hold data and whose padding holds `fill` (a huge finite sentinel for operands)"""
    buf = torch.full((rows, ld), fill, dtype=dtype, device="cuda")
    buf[:, :cols] = dev(rnd((rows, cols), seed, scale), dtype)
    return buf


@pytest.mark.parametrize("tile", [0, 128002, 128160, 3264, 256256])
@pytest.mark.parametrize("M", [5, 200])
def test_gemm_row_pitch_larger_than_width(M, tile):
    """The C ABI's row pitch (RowMap.ld) with padding between rows, through ffi.GemmDesc directly: operands whose padding columns hold a
    huge finite sentinel (the product must not see it) and an output whose padding must survive bit for bit, plus a guarded workspace."""
    from flamingo_mini_amd import ffi
    lib = ffi.lib()
    N, K = 264, 328
    lda, ldb, ldc = K + 24, K + 40, N + 36
    big = 1.0e30
    for dtype in (BF16, F32):
        if dtype == F32 and tile in (128160, 3264, 256256):
            continue                                            # bf16-only tiles
        A = _padded(M, K, lda, dtype, 61, 0.5, big)
        B = _padded(N, K, ldb, dtype, 62, 0.05, big)
        Cbuf = torch.full((M, ldc), -3.25, dtype=dtype, device="cuda")
        R = _padded(M, N, ldc, dtype, 63, 1.0, big)             # the residual is read through c_map too
        gate = dev(np.array([0.7]), dtype)
        g_ = float(np.tanh(as64(gate)[0]))
        Av, Bv = A[:, :K], B[:, :K]
        for split in (1, 3):
            for residual in (False, True):
                before = Cbuf.clone()
                d = ffi.GemmDesc(ffi.dtype_code(dtype), M, N, K, 0, 0, ffi.rowmap(lda), ffi.rowmap(ldb), ffi.rowmap(ldc), 1.0,
                                 ffi.ACT_NONE, ffi.ACT_NONE, split, tile, 0)
                with guarded_allocations() as g:
                    ws = F()._empty_bytes(lib.ff_gemm_workspace_bytes(d), A.device)
                    ffi.check(lib.ff_gemm(d, A.data_ptr(), B.data_ptr(), Cbuf.data_ptr(), None, None,
                                          R.data_ptr() if residual else None, gate.data_ptr() if residual else None,
                                          ws.data_ptr(), ws.numel(), ffi.stream_handle(A.device)), "ff_gemm")
                    g.check()
                what = (str(dtype), M, tile, split, residual)
                pad_b = Cbuf[:, N:].view(torch.int16 if dtype == BF16 else torch.int32)
                assert torch.equal(pad_b, before[:, N:].view(pad_b.dtype)), f"{what}: output padding overwritten"
                r = as64(R[:, :N])
                epi = (lambda a: (r + g_ * a, np.full_like(a, g_))) if residual else None
                _bound(Cbuf[:, :N], Av, Bv, what, epilogue=epi, u_out=None if dtype == BF16 else 2.0 ** -21)


def _profile_tiles(fn):
    from flamingo_mini_amd import ffi
    lib = ffi.lib()
    lib.ff_gemm_profile_enable(256)
    try:
        fn()
        torch.cuda.synchronize()
        recs = (ffi.GemmProfileRecord * 256)()
        n = lib.ff_gemm_profile_read(recs, 256)
    finally:
        lib.ff_gemm_profile_enable(0)
    return [(recs[i].tile, recs[i].split_k, recs[i].M, recs[i].N, recs[i].K) for i in range(n)]


def test_guards_do_not_change_the_dispatch():
    """The guards keep every buffer's alignment, so the kernels choose the same paths (vector widths, ring depths) with and without them:
    the launch records of a GEMM and of one fused cross-attention block step (forward + backward) are the same in both runs."""
    from test_hip_modules import build_block
    from detgen import det, xattn_params
    A, B = dev(rnd((1000, 1280), 71, 0.5), BF16), dev(rnd((5120, 1280), 72, 0.05), BF16)
    gemm = lambda: F().gemm(A, B, act="gelu", want_aux_out=True)          # noqa: E731
    plain = _profile_tiles(gemm)
    with guarded_allocations():
        guarded = _profile_tiles(gemm)
    assert plain and plain == guarded
    b, L, nv, dim, dv = 2, 20, 64, 1024, 256
    m = build_block(xattn_params(dim, dv, 8, 64, 2, tag="disp"), dim, dv, 8, 64, nv, 2, "gelu", BF16)
    ml = torch.zeros(b, L, dtype=torch.int64, device="cuda")
    ml[:, 0] = 1
    y = dev(det((b, L, dim), "disp-y"), BF16).requires_grad_(True)
    vf = dev(det((b, 1, nv, dv), "disp-vf"), BF16)
    dy = dev(det((b, L, dim), "disp-dy"), BF16)

    def step():
        out, _ = m(y, vf, ml)
        out.backward(dy)
    plain = _profile_tiles(step)
    with guarded_allocations():
        guarded = _profile_tiles(step)
    assert any(t[0] <= -4 for t in plain) and plain == guarded


# ---------------------------------------------------------------------------------------------------------------------------------------
# LayerNorm, rows_reduce, gate_grad: every dispatch branch of ff_rowwise.hip
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("rows,cols", [(1, 64), (3, 1280), (1023, 256), (1025, 512), (2049, 1024), (37, 2048), (5, 36), (64, 4096),
                                       (257, 2560)],
                         ids=["r1", "r3", "r1023", "r1025", "r2049", "nch-wide", "non-vector-c36", "c4096-col-reduce", "r257-c2560"])
def test_layernorm_branches_guarded(dtype, rows, cols):
    """Forward + backward (with the residual gradient added) per row against float64: rows-per-block 4 / 8 / 12 (1, 3, 1023, 1025, 2049
    rows), the fused backward's column chunks (widths 256 ... 4096), the element-wise path (36 columns) and the column-reduce of the fp32
    gamma / beta gradients (4096 columns)."""
    x, g, b = dev(rnd((rows, cols), 1, 2.0), dtype), dev(1 + 0.2 * rnd((cols,), 2), dtype), dev(0.1 * rnd((cols,), 3), dtype)
    dy, res = dev(rnd((rows, cols), 4), dtype), dev(rnd((rows, cols), 5), dtype)
    with guarded_allocations() as guard:
        y, mean, rstd = F().layernorm_fwd(x, g, b)
        dx, dg, db = F().layernorm_bwd(dy, x, g, mean, rstd, dx_residual=res)
        guard.check()
    yr, cache = O.layernorm_fwd(as64(x), as64(g), as64(b))
    dxr, dgr, dbr = O.layernorm_bwd(as64(dy), cache, as64(g))
    t = TOL[dtype]
    assert rel(y, yr) < t["out"] and rel(dx, dxr + as64(res)) < t["grad"]
    _rows(y, yr, (0,), dtype, "out", "y")
    _rows(dx, dxr + as64(res), (0,), dtype, "grad", "dx")
    assert np.allclose(as64(mean), as64(x).mean(-1), rtol=1e-5, atol=1e-5) and np.allclose(as64(rstd), cache[1][:, 0], rtol=1e-4)
    assert rel(dg, dgr) < t["grad"] and rel(db, dbr) < t["grad"]
    _rows(dg.reshape(1, -1), dgr.reshape(1, -1), (0,), dtype, "grad", "dgamma")       # one row: but no NaN anywhere
    assert torch.isfinite(dg).all() and torch.isfinite(db).all()


@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
def test_layernorm_time_embedding_addend_guarded(dtype):
    """The time-embedding addend (x + tpe[t] per segment): forward and backward per row."""
    b, T, v, D = 3, 2, 5, 64
    x, tpe = dev(rnd((b * T * v, D), 1), dtype), dev(rnd((4, D), 2), dtype)
    g, be = dev(1 + 0.2 * rnd((D,), 3), dtype), dev(0.1 * rnd((D,), 4), dtype)
    dy = dev(rnd((b * T * v, D), 5), dtype)
    with guarded_allocations() as guard:
        y, mean, rstd = F().layernorm_fwd(x, g, be, add=tpe, add_rows_per_seg=T * v, add_div=v)
        dx, dg, db = F().layernorm_bwd(dy, x, g, mean, rstd, add=tpe, add_rows_per_seg=T * v, add_div=v)
        guard.check()
    xx = as64(x).reshape(b, T, v, D) + as64(tpe)[:T][None, :, None, :]
    yr, cache = O.layernorm_fwd(xx.reshape(-1, D), as64(g), as64(be))
    dxr, dgr, dbr = O.layernorm_bwd(as64(dy), cache, as64(g))
    _rows(y, yr, (0,), dtype, "out", "y")
    _rows(dx, dxr, (0,), dtype, "grad", "dx")
    assert rel(dg, dgr) < TOL[dtype]["grad"] and rel(db, dbr) < TOL[dtype]["grad"]


@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("b,T,v,D", [(4, 3, 7, 128), (1, 1, 1, 36), (2, 4, 257, 1024), (32, 1, 64, 1280)])
def test_rows_reduce_and_gate_grad_guarded(dtype, b, T, v, D):
    x = dev(rnd((b * T * v, D), 1), dtype)
    with guarded_allocations() as guard:
        out_t = F().rows_reduce(x, T * v, v)                  # d time_pos_emb pattern
        out_l = F().rows_reduce(x, T * v, 1)                  # d latents pattern
        a, c, alpha = dev(rnd((b * T * v, D), 2), dtype), dev(rnd((b * T * v, D), 3), dtype), dev(np.array([0.3]), dtype)
        ga = F().gate_grad(a, c, alpha)
        guard.check()
    _rows(out_t, as64(x).reshape(b, T, v, D).sum((0, 2)), (0,), dtype, "grad", "d tpe rows")
    _rows(out_l, as64(x).reshape(b, T * v, D).sum(0), (0,), dtype, "grad", "d latents rows")
    prod = as64(a) * as64(c)
    ref = prod.sum() * (1 - np.tanh(as64(alpha)[0]) ** 2)
    scale = np.linalg.norm(prod) * (1 - np.tanh(as64(alpha)[0]) ** 2)
    assert abs(float(ga.float().cpu()) - ref) <= TOL[dtype]["grad"] * (scale + abs(ref))


# ---------------------------------------------------------------------------------------------------------------------------------------
# attention core
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,dh", [(F32, 64), (BF16, 64), (BF16, 128)], ids=["f32-64", "bf16-64", "bf16-128"])
@pytest.mark.parametrize("nq", [1, 64, 65])
@pytest.mark.parametrize("nkv", [1, 63, 65, 321])
def test_attention_rows_guarded(dtype, dh, nq, nkv):
    from test_hip_primitives import _attn_ref
    b, h = 2, 3
    q, k, v = (dev(rnd((b, n, h, dh), s, sc), dtype) for n, s, sc in ((nq, 1, dh ** -0.5), (nkv, 2, 1.0), (nkv, 3, 1.0)))
    do = dev(rnd((b, nq, h, dh), 4), dtype)
    with guarded_allocations() as g:
        o, lse = F().attention_fwd(q, k, v)
        dq, dk, dv = F().attention_bwd(q, k, v, o, do, lse)
        g.check()
    oref, bwd = _attn_ref(as64(q), as64(k), as64(v), None, 0)
    assert rel(o, oref) < TOL[dtype]["out"]
    _rows(o, oref, (0, 2, 1), dtype, "out", "o (b, h, q)")
    assert torch.isfinite(lse).all()
    for got, ref, name in zip((dq, dk, dv), bwd(as64(do)), "qkv"):
        if name in "qk" and nkv == 1:
            # one key: every weight is exactly 1, so ds = p (dp - D) and with it the exact d q and d k are exactly 0; the kernel's
            # D = rowsum(dO . O) starts from the ROUNDED O, so dp - D leaves a rounding residue (measured on an MI355X: L2 norm over the
            # whole tensor <= 2.2e-5 for d q, <= 2.9e-5 for d k): held absolutely
            assert float(got.abs().max()) < 1e-3, name
            # ... and by the element bounds of util.attn_bound_ok, whose u_T term is that residue: in fp32 (2^-24 sum |dO . o| |k|, about 5e-7) far
            # tighter than the line above, in bf16 (2^-8 of it: o = v is exact here, the bound cannot know) looser, so both stay
            ok, worst, idx = attn_bound_ok("d" + name, got, attention_ref(q, k, v, do), dtype)
            assert ok, f"d{name} element {idx} is {worst:.4g} x its bound"
            continue
        assert rel(got, ref) < TOL[dtype]["grad"], name
        if name == "k" and nq == 1:
            continue        # one query: d k_j = p_j (dp_j - D) q is a single cancelling term per row - its row error says nothing about tiles
        _rows(got, ref, (0, 2, 1), dtype, "grad", f"d{name} (b, h, row)")


@pytest.mark.parametrize("dtype,dh,nv", [(F32, 16, 8), (F32, 64, 64), (BF16, 64, 64)], ids=["f32-toy", "f32", "bf16"])
def test_attention_media_mask_rows_guarded(dtype, dh, nv):
    """Media-masked attention per (b, h, q) row: rows before any image are exactly zero (o and dq), uniform rows get no q gradient."""
    from test_hip_primitives import _attn_ref
    b, h, L, N = 3, 2, 70, 2
    ml = np.zeros((b, L), np.int64)
    ml[0, [0, 33]] = 1
    ml[1, [5, 40, 66]] = 1
    tt = O.text_time_of(ml)
    q, k, v = (dev(rnd((b, n, h, dh), s, sc), dtype) for n, s, sc in ((L, 1, dh ** -0.5), (N * nv, 2, 1.0), (N * nv, 3, 1.0)))
    do = dev(rnd((b, L, h, dh), 4), dtype)
    ttd = torch.as_tensor(tt, dtype=torch.int32).cuda()
    with guarded_allocations() as g:
        o, lse = F().attention_fwd(q, k, v, tt=ttd, n_visual=nv)
        dq, dk, dv = F().attention_bwd(q, k, v, o, do, lse, tt=ttd, n_visual=nv)
        g.check()
    oref, bwd = _attn_ref(as64(q), as64(k), as64(v), tt, nv)
    _rows(o, oref, (0, 2, 1), dtype, "out", "o")             # exact-zero reference rows must be exactly zero
    for got, ref, name in zip((dq, dk, dv), bwd(as64(do)), "qkv"):
        _rows(got, ref, (0, 2, 1), dtype, "grad", f"d{name}")


# ---------------------------------------------------------------------------------------------------------------------------------------
# the fused cross-attention block: every branch of xa_qattn_fwd / xa_dattn_bwd, batch >= 2
# ---------------------------------------------------------------------------------------------------------------------------------------
XA_CASES = [
    # (dtype, dim_head, b, L, nv, dim, heads): resident kernels (bf16, dh 64, <= 32 tokens, <= 64 keys), ring depth 6 / 4, with and
    # without the in-launch exchange (phase 2/3 at dim <= 1280, a multiple of 256); the generic BM = 32 kernel, the BM = 64 single-tile
    # kernel and the multi-tile kernel (n_q > 64) with two and three samples; bf16 at dim_head 64 / 128; fp32 at 16 / 32 / 64 / 128
    (BF16, 64, 3, 20, 64, 1280, 8), (BF16, 64, 2, 32, 40, 768, 8), (BF16, 64, 5, 7, 64, 1536, 8),
    (BF16, 64, 2, 48, 64, 512, 8), (BF16, 64, 2, 64, 64, 512, 8), (BF16, 64, 3, 150, 64, 512, 8), (BF16, 128, 2, 100, 64, 512, 4),
    (BF16, 128, 2, 24, 64, 512, 4),
    (F32, 16, 2, 70, 16, 128, 4), (F32, 32, 3, 40, 32, 256, 4), (F32, 64, 2, 130, 64, 256, 4), (F32, 128, 2, 66, 64, 256, 2),
]


@pytest.mark.parametrize("dtype,dh,b,L,nv,dim,heads", XA_CASES,
                         ids=[f"{'bf16' if c[0] == BF16 else 'f32'}-dh{c[1]}-b{c[2]}-L{c[3]}-nv{c[4]}-d{c[5]}" for c in XA_CASES])
def test_fused_xattn_block_rows_guarded(dtype, dh, b, L, nv, dim, heads):
    """Forward and backward of the gated cross-attention block per (sample, token) row against the oracle, with per-sample media tags that
    leave leading tokens without an image (their attention contribution must be exactly zero) and a second sample with its own offsets."""
    from test_hip_modules import build_block
    from detgen import det, xattn_params
    dv, ffm = 128, 2
    p = xattn_params(dim, dv, heads, dh, ffm, tag=f"bounds{dim}{dh}")
    m = build_block(p, dim, dv, heads, dh, nv, ffm, "gelu", dtype)
    ml = np.zeros((b, L), np.int64)
    ml[0, 0] = 1
    ml[1, min(3, L - 1)] = 1                                    # tokens 0..2 of sample 1 see nothing
    if b > 2:
        ml[2, [1, L - 2]] = 1
    y = dev(det((b, L, dim), "bounds-y"), dtype).requires_grad_(True)
    vf = dev(det((b, 1, nv, dv), "bounds-vf"), dtype).requires_grad_(True)
    dy = dev(det((b, L, dim), "bounds-dy"), dtype)
    mlt = torch.as_tensor(ml).cuda()
    with guarded_allocations() as g:
        out, _ = m(y, vf, mlt)
        out.backward(dy)
        g.check()
    p64 = {k: as64(v) for k, v in m.state_dict().items()}
    outr, _, cache = O.gated_xattn_block_fwd(as64(y), as64(vf), ml, p64, heads=heads, dim_head=dh, n_visual=nv)
    dyr, dvfr, gr = O.gated_xattn_block_bwd(as64(dy), cache, p64, heads=heads, dim_head=dh)
    t = TOL[dtype]
    assert rel(out - y, outr - as64(y)) < t["out"]
    assert rel(y.grad, dyr) < t["grad"] and rel(vf.grad, dvfr) < t["grad"]
    _rows(out - y, outr - as64(y), (0, 1), dtype, "grad", "out - y (sample, token)")
    _rows(y.grad, dyr, (0, 1), dtype, "grad", "dy (sample, token)")
    _rows(vf.grad, dvfr, (0, 1, 2), dtype, "grad", "dvf (sample, media, key)")
    for k in ("attn.to_q.weight", "attn.to_kv.weight", "attn.to_out.weight", "ffw.1.weight"):
        assert rel(dict(m.named_parameters())[k].grad, gr[k]) < t["grad"], k


# ---------------------------------------------------------------------------------------------------------------------------------------
# whole-module parity tests, rerun once inside the guards
# ---------------------------------------------------------------------------------------------------------------------------------------
def _rerun(fn, *args):
    with guarded_allocations() as g:
        fn(*args)
        g.check()


@pytest.mark.parametrize("case", [(3, 20, 64, 1280), (2, 32, 40, 768), (5, 7, 64, 1536), (4, 32, 64, 1024)], ids=str)
def test_resident_fused_kernels_guarded(case):
    from test_hip_modules import test_resident_fused_kernels_bf16_vs_oracle
    _rerun(test_resident_fused_kernels_bf16_vs_oracle, *case)


@pytest.mark.parametrize("case", [(32, 1, 1280, 4, "gelu"), (3, 5, 256, 1, "sqrelu")], ids=["gpt2-large-decode-b32", "tiny-M15"])
def test_decode_feedforward_guarded(case):
    """The decode kernels' workspace (partial slabs and the down-projection's tickets) starts as 0xA5 bytes: the tickets must really be
    zeroed by the up-projection launch (csrc/ff_decode.hip), or the combine goes wrong."""
    from test_hip_modules import test_decode_shaped_feedforward_bf16_vs_oracle
    _rerun(test_decode_shaped_feedforward_bf16_vs_oracle, *case)


def test_resampler_vit_l_guarded():
    from test_hip_modules import test_resampler_vs_oracle_vit_l_shape
    _rerun(test_resampler_vs_oracle_vit_l_shape, BF16)


def test_config_c_block_guarded():
    from test_hip_configs import test_config_C_opt_1p3b_block
    _rerun(test_config_C_opt_1p3b_block, BF16)


@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
def test_shifted_cross_entropy_guarded(dtype):
    from test_hip_loss import test_shifted_cross_entropy_matches_torch
    for reduction in ("none", "mean"):
        _rerun(test_shifted_cross_entropy_matches_torch, dtype, reduction)


@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
def test_fused_adamw_guarded(dtype):
    """test_hip_optim's shapes include lengths that are not a multiple of the vector width (3, 513 x 7, 1): the moments are guarded
    allocations (zero bodies), so a vector tail that ran past a tensor's end lands in a guard."""
    from test_hip_optim import test_fused_adamw_matches_oracle_and_torch
    _rerun(test_fused_adamw_matches_oracle_and_torch, dtype)


# ---------------------------------------------------------------------------------------------------------------------------------------
# time_pos_emb gradient rows of frames the batch does not have: exactly zero on every training path
# ---------------------------------------------------------------------------------------------------------------------------------------
def _tpe_rows_zero(model, what):
    tpe = model.flamingo.resampler.time_pos_emb
    T = 1                                                       # still images: one frame
    assert tpe.shape[0] > T and tpe.grad is not None, what
    torch.cuda.synchronize()
    rest = tpe.grad[T:]
    assert int((rest != 0).sum()) == 0, f"{what}: time_pos_emb.grad rows {T}.. hold {rest.abs().max().item():.3g}"
    assert float(tpe.grad[:T].abs().sum()) > 0, what


@pytest.mark.parametrize("mode", ["eager-stack", "eager-layerwise", "graphed", "piecewise"])
def test_unused_time_embedding_gradient_rows_are_zero(mode):
    """The h64 fixture model (num_time_embeds 4, still images: T = 1) after a training step on each path: the gradient rows of frames the batch
    does not have are exactly zero, as the reference's time_pos_emb[:T] slicing gives - also after replays of captured steps (whose gradient
    buffers are reused, not re-created) and with the moments and gradients under the guards' poison (eager paths)."""
    from test_model_plumbing import H64, build_h64
    from flamingo_mini_amd import FusedAdamW, GraphedTrainStep
    from flamingo_mini_amd.graphs import PiecewiseGraphedTrainStep
    model, _, batch = build_h64(BF16, "cuda")
    model.flamingo.resampler.layerwise = mode == "eager-layerwise"
    params = list(model.parameters_trainable())
    if mode.startswith("eager"):
        opt = FusedAdamW(params, **H64["adamw"])
        with guarded_allocations() as g:
            for _ in range(2):
                model.zero_grad(set_to_none=True)
                model(**batch).loss.backward()
                _tpe_rows_zero(model, mode)
                opt.step()
                _tpe_rows_zero(model, mode + " after the optimizer")
            g.check()
        return
    opt = FusedAdamW(params, capturable=True, **H64["adamw"])
    if mode == "graphed":
        step = GraphedTrainStep(model, opt, batch, warmup=1)
    else:
        step = PiecewiseGraphedTrainStep(model, opt, batch, warmup=1, segment_layers=1)
    try:
        for i in range(3):
            step()
            _tpe_rows_zero(model, f"{mode} replay {i}")
    finally:
        if hasattr(step, "close"):
            step.close()
