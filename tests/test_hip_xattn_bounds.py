"""The fused cross-attention block held stage by stage to per-element bounds, on the MI355X.

The parity tests hold the block by rel() / rel_rows() of its 1280-wide output rows behind two residual adds, on scores of about N(0, 1)
and one image per sample.  Here one test per (case, pattern) of tests/xattn_cases.py - one case per kernel path of csrc/ff_xattn_fused.hip
(general kernels at 32- and 64-row tiles, single and multi-tile backward, the resident kernels at ring depth 4 and 6 with and without the
in-launch exchange) and the decode feed-forward of csrc/ff_decode.hip, each asserted from the launch log - runs ff_xattn_block_fwd,
ff_xattn_block_bwd_kv_data and ff_xattn_wgrad_grouped on designed K / V with several images inside a key tile, zero, image and uniform
rows in every wave, and judges every stage from what the kernel stored for the stage before (xattn_cases.stage_checks): Qs, lse, O,
attn_out, y1, Hpre, Aact, ffw_out, y_out, d H, d Qs, d K, d V, read through ff_xattn_saved_view and ff_xattn_wgrad_stash_view.
Every buffer lies between guard bytes; outputs, `saved`, the stash and the scratch are NaN (all bytes 0xFF) before the calls."""
import ctypes as C

import numpy as np
import pytest
import torch

import xattn_cases as xc
from test_hip_layernorm_bounds import Buf, bits, out, put

pytestmark = pytest.mark.gpu
F32 = xc.F32
DIM_VISUAL = 32           # of the descriptor only: K / V come from outside, to_kv is never applied


def block_run(case):
    """forward, data backward (with a stash) and the grouped weight gradients of one block; returns (what the block stored: xattn_cases'
    FWD_KEYS and BWD_KEYS on the CPU, the launch log as (tile, b_layout) pairs).  Asserts that no guard byte, no input and no parameter
    changed, that every output element was written and that no arrival wait of the in-launch exchange timed out."""
    from flamingo_mini_amd import ffi
    from flamingo_mini_amd import functional as Fn
    lib, dt = ffi.lib(), case.dtype
    dev = torch.device("cuda")
    b, L, d = case.b, case.L, case.dim
    pb = [put(p) for p in case.params]
    ins = dict(y=put(case.y), kv=put(case.kv), dyo=put(case.dyo), tt=put(torch.from_numpy(case.tt_buf)))
    src = dict(y=case.y, kv=case.kv, dyo=case.dyo, tt=torch.from_numpy(case.tt_buf))
    sync = Fn.ensure_sync_buffer(dev) if case.sync else None
    desc = ffi.XattnDesc(ffi.dtype_code(dt), b, L, d, DIM_VISUAL, case.n_media, case.nv, case.heads, case.dh, xc.FF_MULT, ffi.ACT_GELU,
                         case.tt_stride, case.tt_offset)
    desc.cached_k = desc.cached_v = ffi.Strides(case.n_kv * 2 * case.inner, 2 * case.inner, case.dh)
    desc.sync = None if sync is None else sync.data_ptr()
    saved, scratch = Buf(lib.ff_xattn_saved_bytes(desc)), Buf(lib.ff_xattn_scratch_bytes(desc))
    stash, ws = Buf(lib.ff_xattn_wgrad_stash_bytes(desc)), Buf(max(int(lib.ff_xattn_wgrad_workspace_bytes(desc)), 16))
    outs = dict(y_out=out(dt, (b, L, d)), dy=out(dt, (b, L, d)), dkv=out(dt, tuple(case.kv.shape)))
    grads = [None if i == 5 else out(dt, tuple(p.shape)) for i, p in enumerate(case.params)]
    gptr = ffi.ptr_array([None if g is None else g[1] for g in grads])
    pptr = ffi.ptr_array([v for _, v in pb])
    P = {k: v.data_ptr() for k, (_, v) in {**ins, **outs}.items()}
    kptr, vptr = P["kv"], P["kv"] + case.inner * case.kv.element_size()
    stream = ffi.stream_handle(dev)
    lib.ff_gemm_profile_enable(64)
    try:
        ffi.check(lib.ff_xattn_block_fwd(desc, P["y"], None, P["tt"], pptr, kptr, vptr, P["y_out"], saved.body.data_ptr(), saved.n,
                                         scratch.body.data_ptr(), scratch.n, stream), "ff_xattn_block_fwd")
        ffi.check(lib.ff_xattn_block_bwd_kv_data(desc, P["y"], kptr, vptr, P["tt"], pptr, P["dyo"], saved.body.data_ptr(), saved.n, gptr, P["dy"],
                                                 P["dkv"], stash.body.data_ptr(), stash.n, scratch.body.data_ptr(), scratch.n, stream),
                  "ff_xattn_block_bwd_kv_data")
        ffi.check(lib.ff_xattn_wgrad_grouped(desc, 1, ffi.ptr_array([ins["dyo"][1]]), ffi.ptr_array([saved.body]), saved.n, ffi.ptr_array([stash.body]),
                                             stash.n, pptr, gptr, ws.body.data_ptr(), ws.n, stream), "ff_xattn_wgrad_grouped")
        torch.cuda.synchronize()
        recs = (ffi.GemmProfileRecord * 64)()
        n = lib.ff_gemm_profile_read(recs, 64)
    finally:
        lib.ff_gemm_profile_enable(0)
    log = [(recs[i].tile, recs[i].b_layout) for i in range(n)]
    named = [("saved", saved), ("scratch", scratch), ("stash", stash), ("workspace", ws)] + [(k, buf) for k, (buf, _) in {**ins, **outs}.items()] + \
            [(f"param {i}", buf) for i, (buf, _) in enumerate(pb)] + [(f"grad {i}", g[0]) for i, g in enumerate(grads) if g is not None]
    for name, buf in named:
        assert buf.guards_intact(), f"{case.name}: a byte outside {name} was written"
    for k, (_, v) in ins.items():
        assert torch.equal(bits(v.cpu()), bits(src[k])), f"{case.name}: {k} was written"
    for (_, v), p in zip(pb, case.params):
        assert torch.equal(bits(v.cpu()), bits(p)), f"{case.name}: a parameter was written"
    for k, (_, v) in outs.items():
        assert not bool(torch.isnan(v.float()).any()), f"{case.name}: {k} holds an element nobody wrote"
    for i, g in enumerate(grads):
        assert g is None or not bool(torch.isnan(g[1].float()).any()), f"{case.name}: gradient {i} holds an element nobody wrote"
    if case.sync:
        assert Fn.sync_exchange_status() == 0, f"{case.name}: an arrival wait of the in-launch exchange timed out"
    st, off, nb = {}, C.c_size_t(), C.c_size_t()
    shape = dict(yn=(b, L, d), Qs=(b, L, case.inner), lse=(b, case.heads, L), O=(b, L, case.inner), attn_out=(b, L, d), y1=(b, L, d), xn_f=(b, L, d),
                 Hpre=(b, L, case.ffi), Aact=(b, L, case.ffi), ffw_out=(b, L, d), dy1=(b, L, d), dH=(b, L, case.ffi), dQs=(b, L, case.inner))
    for view, buf, codes in ((lib.ff_xattn_saved_view, saved, {**ffi.XA_SAVED, **ffi.XA_SAVED_STAGES}), (lib.ff_xattn_wgrad_stash_view, stash, ffi.XA_STASH)):
        for what, code in codes.items():
            if what in shape:
                ffi.check(view(desc, code, C.byref(off), C.byref(nb)), "saved / stash view")
                st[what] = buf.body[off.value:off.value + nb.value].view(F32 if what == "lse" else dt).view(shape[what]).cpu()
    st["y_out"], st["dkv"] = outs["y_out"][1].cpu(), outs["dkv"][1].cpu()
    assert set(st) == set(xc.FWD_KEYS + xc.BWD_KEYS)
    return st, log


def assert_path(case, log):
    """the kernels the case is there for, from the launch log: the fused forward's tile code and ring depth, the fused backward's tile code,
    the decode feed-forward's two launches exactly where they are to run, and attention_bwd_dkv (tile -3) exactly where the queries of a
    sample span several tiles"""
    fwd = [r for r in log if r[0] in (-4, -6, -8)]
    bwd = [r for r in log if r[0] in (-5, -7, -9)]
    assert len(fwd) == 1 and len(bwd) == 1, f"{case.name}: launch log {log}"
    assert fwd[0] == (case.tile, case.ring), f"{case.name}: the forward ran tile {fwd[0][0]} at ring depth {fwd[0][1]}, launch log {log}"
    assert bwd[0][0] == case.bwd_tile, f"{case.name}: the backward ran tile {bwd[0][0]}, launch log {log}"
    decode = sorted(r[0] for r in log if r[0] in (-10, -11))
    assert decode == ([-11, -10] if case.ffw == "decode" else []), f"{case.name}: the feed-forward was to run on the {case.ffw} path, launch log {log}"
    assert sum(r[0] == -3 for r in log) == (1 if case.L > 64 else 0), f"{case.name}: attention_bwd_dkv, launch log {log}"
    assert not any(r[0] in (-1, -2) for r in log), f"{case.name}: a stand-alone attention kernel ran, launch log {log}"


@pytest.mark.parametrize("pattern", xc.PATTERNS)
@pytest.mark.parametrize("row", xc.CASES, ids=xc.CASE_IDS)
def test_fused_block_stages_within_the_element_bounds(row, pattern):
    case = xc.Case(row, pattern)
    st, log = block_run(case)
    assert_path(case, log)
    xc.check_conditions(case, xc.f64(st["Qs"]).reshape(case.b, case.L, case.heads, case.dh), xc.f64(case.K4()), "stored Qs")
    res = xc.stage_checks(case, st)
    print(f"{case.name}: " + " ".join(f"{what.replace(' ', '_')} {worst:.3f}" for _, what, _, worst, _ in res))      # every figure before the first assertion
    bad = xc.failures(case, res)
    assert not bad, "\n".join(bad)
