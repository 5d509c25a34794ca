"""Every LayerNorm implementation held to per-element bounds on designed rows, on the MI355X.

The parity tests compare LayerNorm outputs with rel() / rel_rows() at 5e-6 / 8e-3 on N(0, 2^2) rows and never look at the statistics the
block kernels save for backward.  Here every output is held element by element to float64 from what the kernel saw (ln_cases.ln_ref,
util.ln_bound_ok) on the row families of tests/ln_cases.py - offsets of 100 / 1000, a 2000-sigma channel in the head, the body and the
tail of a row, a raised head, constant, zero, tiny-variance, 1e4 and 1e-3 rows, family r mod 13 in row r.
Part A, the C ABI (ff_layernorm_fwd / bwd, ff_rows_reduce, ff_gate_grad) in bf16 and fp32 at the smallest shapes that reach each branch
(ln_cases.ABI_SHAPES), with the time-embedding addend, y == NULL followed by stats_given, dgamma == NULL, and dx_residual aliasing dx.
Part B, the statistics inside the block kernels: ff_xattn_block_fwd on designed rows, mean_a / rstd_a / yn and mean_f / rstd_f / xn_f read
from `saved` through ff_xattn_saved_view, one case per kernel path (ln_cases.BLOCK_CASES), each asserting its path from the launch log;
once with alpha_attn = 0 (y1 = y exactly: the designed rows reach LN(y1)) and once with the usual gate; the reference reads the stored y1.
Every buffer lies between guard bytes; outputs and `saved` are NaN (all bytes 0xFF) before the call."""
import ctypes as C

import numpy as np
import pytest
import torch

import ln_cases as lc
from util import TOL, ln_bound_ok

pytestmark = pytest.mark.gpu
BF16, F32 = lc.BF16, lc.F32
BITS = {F32: torch.int32, BF16: torch.int16}
DTYPES = pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
PADB = 256
WORST, FAMILY_RSTD = {}, {}


class Buf:
    """`nbytes` of device memory, every byte 0xFF (a NaN in bf16 and in fp32), between two guards of PADB bytes"""

    def __init__(self, nbytes):
        self.n = int(nbytes)
        self.flat = torch.full((self.n + 2 * PADB,), 0xFF, dtype=torch.uint8, device="cuda")
        self.body = self.flat[PADB:PADB + self.n]
        assert self.body.data_ptr() % 16 == 0

    def view(self, dtype, shape):
        return self.body.view(dtype).view(shape)

    def guards_intact(self):
        return bool((self.flat[:PADB] == 0xFF).all()) and bool((self.flat[PADB + self.n:] == 0xFF).all())


def put(t):
    buf = Buf(t.numel() * t.element_size())
    v = buf.view(t.dtype, t.shape)
    v.copy_(t)
    return buf, v


def out(dtype, shape):
    buf = Buf(int(np.prod(shape)) * torch.empty((), dtype=dtype).element_size())
    return buf, buf.view(dtype, shape)


def bits(t):
    return t.contiguous().view(BITS.get(t.dtype, torch.int32))


def note(key, worst, name):
    WORST[key] = max(WORST.get(key, (0.0, "")), (worst, name))


def held(name, dtype, checks):
    """checks: (what, got, ref, decode) - every figure is printed and collected before the first assertion"""
    res = [(what, ln_bound_ok(what, got, ref, dtype, decode=dec)) for what, got, ref, dec in checks]
    print(f"{name}: " + " ".join(f"{what} {w:.3f}" for what, (ok, w, idx) in res))
    for what, (ok, w, idx) in res:
        note((lc.name_of(dtype), what), w, name)
    for what, (ok, w, idx) in res:
        assert ok, f"{name}: {what} element {idx} is {w:.4g} x its bound"


# ---- Part A: the C ABI ------------------------------------------------------------------------------------------------------------------
def abi_run(case, want_params=True, residual=True, alias=False, split_stats=False):
    """ff_layernorm_fwd and ff_layernorm_bwd on the case; asserts that no guard byte and no input changed; the outputs on the CPU"""
    from flamingo_mini_amd import ffi
    lib, dt, rows, cols = ffi.lib(), case.dtype, case.rows, case.cols
    ins = {k: put(getattr(case, k)) for k in ("x", "gamma", "beta", "dy", "res") + (("add",) if case.add is not None else ())}
    outs = dict(y=out(dt, (rows, cols)), dx=out(dt, (rows, cols)), dgamma=out(dt, (cols,)), dbeta=out(dt, (cols,)),
                mean=out(F32, (rows,)), rstd=out(F32, (rows,)))
    P = {k: v.data_ptr() for k, (_, v) in {**ins, **outs}.items()}
    m = ffi.rowmap(cols)
    d = ffi.LnDesc(ffi.dtype_code(dt), rows, cols, m, m, m, case.add_rows_per_seg, case.add_div, lc.EPS, 0)
    stream = ffi.stream_handle(torch.device("cuda"))
    if split_stats:          # the statistics alone, then the normalisation from them
        ffi.check(lib.ff_layernorm_fwd(d, P["x"], P.get("add"), None, None, None, P["mean"], P["rstd"], stream), "ff_layernorm_fwd(stats)")
        torch.cuda.synchronize()
        assert bool(torch.isnan(outs["y"][1].float()).all()), "y == NULL wrote y"
        d.stats_given = 1
    ffi.check(lib.ff_layernorm_fwd(d, P["x"], P.get("add"), P["gamma"], P["beta"], P["y"], P["mean"], P["rstd"], stream), "ff_layernorm_fwd")
    d.stats_given = 0
    need = int(lib.ff_layernorm_bwd_workspace_bytes(d))
    ws = Buf(need)
    res_ptr = None
    if residual:
        res_ptr = P["res"]
        if alias:
            outs["dx"][1].copy_(ins["res"][1])
            res_ptr = P["dx"]
    ffi.check(lib.ff_layernorm_bwd(d, P["dy"], P["x"], P.get("add"), P["gamma"], P["mean"], P["rstd"], P["dx"], res_ptr,
                                   P["dgamma"] if want_params else None, P["dbeta"] if want_params else None, ws.body.data_ptr(), need, stream),
              "ff_layernorm_bwd")
    torch.cuda.synchronize()
    for k, (buf, v) in {**ins, **outs, "ws": (ws, None)}.items():
        assert buf.guards_intact(), f"{case.name}: a byte outside {k} was written"
    for k, (buf, v) in ins.items():
        assert torch.equal(bits(v.cpu()), bits(getattr(case, k))), f"{case.name}: {k} was written"
    got = {k: v.cpu() for k, (_, v) in outs.items()}
    if not want_params:
        assert bool(torch.isnan(got["dgamma"].float()).all() and torch.isnan(got["dbeta"].float()).all()), "dgamma == NULL wrote a parameter gradient"
    return got


def abi_held(case, got, residual=True, params=True):
    ref = lc.ln_ref(case.v, case.gamma, case.beta, case.dy, stats=(got["mean"], got["rstd"]), residual=case.res if residual else None)
    checks = [(w, got[w], ref, False) for w in ("mean", "rstd", "y", "dx") + (("dgamma", "dbeta") if params else ())]
    held(case.name, case.dtype, checks)
    return ref


ABI_IDS = [f"{r}x{c}" for r, c in lc.ABI_SHAPES]


@pytest.mark.parametrize("rows,cols", lc.ABI_SHAPES, ids=ABI_IDS)
@DTYPES
def test_abi_layernorm_within_the_element_bounds(dtype, rows, cols):
    """mean, rstd, y, dx (+ residual), dgamma, dbeta of the forward and the backward call, element by element.  At the variant shapes also:
    the same with the time-embedding addend; y == NULL then stats_given (the same bits as the one call); dgamma == NULL without residual
    (ln_bwd_dx_kernel alone: an all-zero dy row gives exact zeros); dx_residual aliasing dx (the same bits as the separate residual)."""
    case = lc.AbiCase(dtype, rows, cols)
    base = abi_run(case)
    abi_held(case, base)
    if (rows, cols) not in lc.ABI_VARIANT_SHAPES:
        return
    with_add = lc.AbiCase(dtype, rows, cols, add=True)
    abi_held(with_add, abi_run(with_add))
    split = abi_run(case, split_stats=True)
    for k in ("mean", "rstd", "y"):
        assert torch.equal(bits(split[k]), bits(base[k])), f"stats_given: {k} differs from the one-call forward"
    alone = abi_run(case, want_params=False, residual=False)
    ref = abi_held(case, alone, residual=False, params=False)
    zero_rows = np.nonzero(ref["t_dx"].max(-1) == 0)[0]
    assert len(zero_rows) >= 1 and int((alone["dx"][torch.from_numpy(zero_rows)] != 0).sum()) == 0, "an all-zero dy row is not exactly zero"
    aliased = abi_run(case, alias=True)
    for k in ("dx", "dgamma", "dbeta"):
        assert torch.equal(bits(aliased[k]), bits(base[k])), f"dx_residual == dx: {k} differs from the separate residual"


@pytest.mark.parametrize("rows,cols,rpb,rpg", lc.REDUCE_CASES, ids=[f"{r}x{c}-{g}" for r, c, _, g in lc.REDUCE_CASES])
@DTYPES
def test_rows_reduce_within_the_element_bounds(dtype, rows, cols, rpb, rpg):
    from flamingo_mini_amd import ffi
    lib = ffi.lib()
    x = lc.reduce_input(dtype, rows, cols)
    xb, xv = put(x)
    ob, ov = out(dtype, (rpb // rpg, cols))
    d = ffi.ReduceDesc(ffi.dtype_code(dtype), rows, cols, ffi.rowmap(cols), rpb, rpg)
    need = int(lib.ff_rows_reduce_workspace_bytes(d))
    ws = Buf(need)
    ffi.check(lib.ff_rows_reduce(d, xv.data_ptr(), ov.data_ptr(), ws.body.data_ptr(), need, ffi.stream_handle(xv.device)), "ff_rows_reduce")
    torch.cuda.synchronize()
    assert xb.guards_intact() and ob.guards_intact() and ws.guards_intact() and torch.equal(bits(xv.cpu()), bits(x))
    held(f"rows_reduce-{lc.name_of(dtype)}-{rows}x{cols}", dtype, [("rows_reduce", ov.cpu(), lc.rows_reduce_ref(x, rpb, rpg), False)])


@pytest.mark.parametrize("rows,cols", lc.GATE_CASES, ids=[f"{r}x{c}" for r, c in lc.GATE_CASES])
@DTYPES
def test_gate_grad_within_the_bound(dtype, rows, cols):
    from flamingo_mini_amd import ffi
    lib = ffi.lib()
    a, b, alpha = lc.gate_inputs(dtype, rows, cols)
    (ab, av), (bb, bv), (lb, lv) = put(a), put(b), put(alpha)
    ob, ov = out(dtype, (1,))
    need = int(lib.ff_gate_grad_workspace_bytes(rows, cols))
    ws = Buf(need)
    ffi.check(lib.ff_gate_grad(ffi.dtype_code(dtype), rows, cols, av.data_ptr(), bv.data_ptr(), lv.data_ptr(), ov.data_ptr(), ws.body.data_ptr(), need,
                               ffi.stream_handle(av.device)), "ff_gate_grad")
    torch.cuda.synchronize()
    assert all(x.guards_intact() for x in (ab, bb, lb, ob, ws))
    held(f"gate_grad-{lc.name_of(dtype)}-{rows}x{cols}", dtype, [("gate_grad", ov.cpu(), lc.gate_grad_ref(a, b, alpha), False)])


# ---- Part B: the statistics inside the block kernels ------------------------------------------------------------------------------------
def block_run(case, alpha_attn):
    """ff_xattn_block_fwd on the case; returns the seven saved regions on the CPU (through ff_xattn_saved_view) and the fused forward
    launch's (tile, ring depth) from the launch log.  Asserts from the same log what normalised y1: the decode feed-forward's two launches
    (tiles -10 and -11, once each) for ffw == "decode" and neither of them otherwise; "phase3" is the fused launch's tile -8, "separate" its
    tile -4 or -6 without the decode launches (ff_layernorm_fwd leaves no record of its own)."""
    from flamingo_mini_amd import ffi
    from flamingo_mini_amd import functional as Fn
    lib, dt = ffi.lib(), case.dtype
    dev = torch.device("cuda")
    params = case.params(alpha_attn)
    pb = [put(p) for p in params]
    (yb, yv), (vb, vv) = put(case.y), put(case.vf)
    tt = torch.from_numpy(case.tt).cuda()
    sync = Fn.ensure_sync_buffer(dev) if case.sync else None
    desc = ffi.XattnDesc(ffi.dtype_code(dt), case.b, case.L, case.dim, case.dv, 1, case.nv, case.heads, case.dh, lc.BLOCK_FF_MULT, ffi.ACT_GELU,
                         case.L, 0)
    desc.sync = None if sync is None else sync.data_ptr()
    saved, scratch = Buf(lib.ff_xattn_saved_bytes(desc)), Buf(lib.ff_xattn_scratch_bytes(desc))
    ob, ov = out(dt, (case.b, case.L, case.dim))
    lib.ff_gemm_profile_enable(64)
    try:
        ffi.check(lib.ff_xattn_block_fwd(desc, yv.data_ptr(), vv.data_ptr(), tt.data_ptr(), ffi.ptr_array([v for _, v in pb]), None, None,
                                         ov.data_ptr(), saved.body.data_ptr(), saved.n, scratch.body.data_ptr(), scratch.n, ffi.stream_handle(dev)),
                  "ff_xattn_block_fwd")
        torch.cuda.synchronize()
        recs = (ffi.GemmProfileRecord * 64)()
        n = lib.ff_gemm_profile_read(recs, 64)
    finally:
        lib.ff_gemm_profile_enable(0)
    log = [(recs[i].tile, recs[i].b_layout) for i in range(n)]
    fused = [r for r in log if r[0] in (-4, -6, -8)]
    assert len(fused) == 1, log
    decode = sorted(r[0] for r in log if r[0] in (-10, -11))          # the decode feed-forward's two launches (csrc/ff_decode.hip)
    assert decode == ([-11, -10] if case.ffw == "decode" else []), f"{case.name}: LN(y1) was to run on the {case.ffw} path, launch log {log}"
    for name, buf in [("saved", saved), ("scratch", scratch), ("y_out", ob), ("y", yb), ("vf", vb)] + [(f"param {i}", b) for i, (b, _) in enumerate(pb)]:
        assert buf.guards_intact(), f"{case.name}: a byte outside {name} was written"
    assert torch.equal(bits(yv.cpu()), bits(case.y)), "y was written"
    for (b, v), p in zip(pb, params):
        assert torch.equal(bits(v.cpu()), bits(p)), "a parameter was written"
    assert not bool(torch.isnan(ov.float()).any()), "y_out holds an element nobody wrote"
    if case.sync:
        assert Fn.sync_exchange_status() == 0
    got, off, nb = {}, C.c_size_t(), C.c_size_t()
    for what, code in ffi.XA_SAVED.items():
        ffi.check(lib.ff_xattn_saved_view(desc, code, C.byref(off), C.byref(nb)), "ff_xattn_saved_view")
        region = saved.body[off.value:off.value + nb.value]
        stat = what.startswith(("mean", "rstd"))
        got[what] = region.view(F32 if stat else dt).view((case.rows,) if stat else (case.rows, case.dim)).cpu()
    return got, fused[0]


def block_held(case, got, tag):
    """LN(y): mean_a, rstd_a, yn from the designed rows; LN(y1): mean_f, rstd_f, xn_f from the STORED y1"""
    y = case.y.reshape(case.rows, case.dim)
    ra = lc.ln_ref(y, case.gamma_a, case.beta_a, P=case.P, P_var=case.P_var, stats=(got["mean_a"], got["rstd_a"]))
    dec = case.ffw == "decode"
    rf = lc.ln_ref(got["y1"], case.gamma_f, case.beta_f, P=16 if dec else 0, stats=(got["mean_f"], got["rstd_f"]))
    for ref, got_r, which in ((ra, got["rstd_a"], "rstd_a"), (rf, got["rstd_f"], "rstd_f")):
        rel = np.abs(got_r.double().numpy() - ref["rstd"]) / ref["rstd"]
        for r, e in enumerate(rel):
            key = (lc.name_of(case.dtype), lc.family_of(r))
            FAMILY_RSTD[key] = max(FAMILY_RSTD.get(key, (0.0, "")), (float(e), f"{which} of {case.name}{tag}"))
        print(f"{case.name}{tag}: worst |{which} - rstd*| / rstd* = {rel.max():.3e} (row {int(rel.argmax())}, {lc.family_of(int(rel.argmax()))}; kappa <= {ref['kappa'].max():.1f})")
    held(case.name + tag, case.dtype, [("mean", got["mean_a"], ra, False), ("rstd", got["rstd_a"], ra, False), ("y", got["yn"], ra, False),
                                       ("mean", got["mean_f"], rf, False), ("rstd", got["rstd_f"], rf, False), ("y", got["xn_f"], rf, dec)])
    if case.dtype == F32:      # the fp32 ceiling: whatever kappa is, a row scaled wrongly by more than the fp32 tolerance breaks the parity tests' promise
        for ref, got_r, which in ((ra, got["rstd_a"], "rstd_a"), (rf, got["rstd_f"], "rstd_f")):
            rel = np.abs(got_r.double().numpy() - ref["rstd"]) / ref["rstd"]
            assert rel.max() <= TOL[F32]["out"], f"{case.name}{tag}: {which} of row {int(rel.argmax())} ({lc.family_of(int(rel.argmax()))}) is off by {rel.max():.3e} relative"


@pytest.mark.parametrize("row", lc.BLOCK_CASES, ids=[r[0] for r in lc.BLOCK_CASES])
def test_block_kernels_save_statistics_within_the_element_bounds(row):
    """Every path writes all seven by-products (a region left unwritten is NaN and fails its bound).  `saved` has no rows past b * L: with
    L < 32 a kernel that stored the rows of its 32-row tile past a sample's text would overwrite the next sample's rows (held by the
    bounds) or, for the last sample, the bytes behind the region - the next region, or the guard behind `saved`."""
    case = lc.BlockCase(row)
    got, (tile, ring) = block_run(case, 0.0)
    assert (tile, ring) == (case.tile, case.ring), f"{case.name}: launch log says tile {tile}, ring depth {ring}"
    assert torch.equal(bits(got["y1"]), bits(case.y.reshape(case.rows, case.dim))), "alpha_attn = 0: y1 is not y"
    block_held(case, got, "")
    gated, path = block_run(case, 0.55)
    assert path == (tile, ring)
    assert not torch.equal(bits(gated["y1"]), bits(got["y1"]))
    for k in ("mean_a", "rstd_a", "yn"):
        assert torch.equal(bits(gated[k]), bits(got[k])), f"{k} depends on the gate"
    block_held(case, gated, " [gated]")
    print({k: v for k, v in WORST.items()})
    print({k: v for k, v in FAMILY_RSTD.items() if k[0] == lc.name_of(case.dtype)})
