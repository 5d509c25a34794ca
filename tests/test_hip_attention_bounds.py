"""The three attention kernels of csrc/ff_attention.hip held to per-element bounds on every layout, on the MI355X.

test_hip_primitives.py and test_hip_bounds.py compare o and the gradients with rel() / rel_rows() at 5e-6 / 8e-3 on one kind of input
(scores about N(0, 1)), never look at lse and only ever pass contiguous tensors with tt_offset = 0.  Here lse, o, dq, dk and dv are held
element by element to float64 from what the kernel saw (attn_cases.attention_ref, util.attn_bound_ok) at the inputs of
tests/attn_cases.py: every instantiation (bf16 32 / 64 / 128, fp32 16 / 32 / 64 / 128) at (n_q, n_kv) = (1, 1), (65, 63), (64, 130),
(130, 200) under flat scores, one dominant key per row (first key, a middle tile, last key, another key for every row of a wave), two
near-tied keys in different tiles, all scores near +200 / -200, and row scales from 0 to 25 inside one wave; media mode with hand-written
text_time (zero rows, every image, two kinds of uniform rows in every wave of one workgroup, a workgroup of zero rows, a ragged one on
the last image) over 5 x 8, 4 x 40 and 3 x 72 keys (216 keys: what three images of 72 take); and, through the C ABI, K / V and dK / dV as
halves of one (b, n_kv, 2, h, d) buffer, head-major storage, rows wider than dim_head, gradients laid out differently from their forward
tensors and text_time read at an offset inside wider rows - each bit for bit equal to the contiguous call, with every element outside a
strided view still holding its sentinel.  Every buffer is carved from a sentinel-filled arena (Buf); outputs are NaN before the call."""
import numpy as np
import pytest
import torch

import attn_cases as ac
from guarded import SENTINEL
from util import attn_bound_ok

pytestmark = pytest.mark.gpu
BF16, F32 = ac.BF16, ac.F32
BITS = {F32: torch.int32, BF16: torch.int16}
VEC = {F32: 4, BF16: 8}                          # elements per 16 bytes: what every stride must be a multiple of
PAD = 64
OUTPUTS = ("lse", "o", "dq", "dk", "dv")
FF_ERR_SHAPE, FF_ERR_UNSUPPORTED, FF_ERR_WORKSPACE = -1, -2, -3          # include/flamingo_fusion.h
TT_EXTRA, TT_OFFSET = 24, 7
WORST = {}


class Buf:
    """A flat device buffer holding the sentinel everywhere, PAD elements before and after its body; tensors are strided views of the
    body, and `inside` remembers which elements belong to one."""

    def __init__(self, n, dtype):
        self.flat = torch.empty(n + 2 * PAD, dtype=dtype, device="cuda")
        self.bits = self.flat.view(BITS[dtype])
        self.bits.fill_(SENTINEL[dtype])
        self.body = self.flat[PAD:PAD + n]
        self.inside = torch.zeros(n + 2 * PAD, dtype=torch.bool, device="cuda")
        assert self.body.data_ptr() % 16 == 0

    def claim(self, view):
        assert view.untyped_storage().data_ptr() == self.flat.untyped_storage().data_ptr()
        self.inside.as_strided(view.shape, view.stride(), view.storage_offset()).fill_(True)
        return view

    def outside_intact(self):
        return bool((self.bits[~self.inside] == SENTINEL[self.flat.dtype]).all())


def place(kind, n, dh, dtype):
    """(buffer, (B, n, H, dh) view): c contiguous, h head-major storage (b, h, n, d), w the leading dh elements of rows of dh + 16 bytes x 2"""
    b, h = ac.B, ac.H
    dw = dh + 2 * VEC[dtype] if kind == "w" else dh
    buf = Buf(b * n * h * dw, dtype)
    view = {"c": lambda: buf.body.view(b, n, h, dh), "h": lambda: buf.body.view(b, h, n, dh).permute(0, 2, 1, 3),
            "w": lambda: buf.body.view(b, n, h, dw)[..., :dh]}[kind]()
    return buf, buf.claim(view)


def place_halves(n, dh, dtype):
    """K and V (dK and dV) as the two halves of one (b, n, 2, h, d) buffer, the product's own K / V layout"""
    buf = Buf(ac.B * n * 2 * ac.H * dh, dtype)
    body = buf.body.view(ac.B, n, 2, ac.H, dh)
    return buf, buf.claim(body[:, :, 0]), buf.claim(body[:, :, 1])


# layout -> how q, k, v, o, do, dq, dk, dv are stored ("2": k with v, dk with dv as halves of one buffer)
LAYOUTS = {
    "contiguous": dict(q="c", k="c", v="c", o="c", do="c", dq="c", dk="c", dv="c"),
    "kv-halves": dict(q="c", k="2", v="2", o="c", do="c", dq="c", dk="2", dv="2"),
    "head-major": dict(q="h", k="h", v="h", o="h", do="h", dq="h", dk="h", dv="h"),
    "wide-rows": dict(q="w", k="c", v="c", o="w", do="w", dq="w", dk="c", dv="c"),
    "grads-elsewhere": dict(q="c", k="c", v="h", o="w", do="h", dq="h", dk="w", dv="c"),
}


def strides_of(view, dtype):
    from flamingo_mini_amd import ffi
    sb, sr, sh, one = view.stride()
    assert one == 1 and view.data_ptr() % 16 == 0 and all(s % VEC[dtype] == 0 for s in (sb, sr, sh)), (view.stride(), view.data_ptr() % 16)
    return ffi.Strides(sb, sr, sh)


def run(case, layout="contiguous"):
    """ff_attention_fwd and ff_attention_bwd on the case's values in the given layout.  Asserts that nothing outside an output's view, no
    input and nothing around any buffer was written; returns the five outputs on the CPU, contiguous."""
    from flamingo_mini_amd import ffi
    lib, dt, dh, n_q, n_kv = ffi.lib(), case.dtype, case.dh, case.n_q, case.n_kv
    kinds, T, bufs = LAYOUTS[layout], {}, []
    for pair, n in ((("k", "v"), n_kv), (("dk", "dv"), n_kv)):
        if kinds[pair[0]] == "2":
            buf, T[pair[0]], T[pair[1]] = place_halves(n, dh, dt)
            bufs.append(buf)
    for name, n in (("q", n_q), ("k", n_kv), ("v", n_kv), ("o", n_q), ("do", n_q), ("dq", n_q), ("dk", n_kv), ("dv", n_kv)):
        if name not in T:
            buf, T[name] = place(kinds[name], n, dh, dt)
            bufs.append(buf)
    for name in ("q", "k", "v", "do"):
        T[name].copy_(getattr(case, name))
    for name in ("o", "dq", "dk", "dv"):
        T[name].fill_(float("nan"))
    lse_buf = Buf(ac.B * ac.H * n_q, F32)
    lse = lse_buf.claim(lse_buf.body.view(ac.B, ac.H, n_q))
    lse.fill_(float("nan"))
    bufs.append(lse_buf)
    tt, tt_stride, tt_offset = None, 0, 0
    if case.tt is not None:
        wide = layout != "contiguous"                # rows wider than n_q, read at an offset, garbage outside the window
        tt_stride, tt_offset = (n_q + TT_EXTRA, TT_OFFSET) if wide else (n_q, 0)
        tt = torch.empty((ac.B, tt_stride), dtype=torch.int32)
        tt[:, 0::2], tt[:, 1::2] = -5, 2 ** 30
        tt[:, tt_offset:tt_offset + n_q] = torch.from_numpy(case.tt)
        tt = tt.cuda()
    d = ffi.AttnDesc(ffi.dtype_code(dt), ac.B, ac.H, dh, n_q, n_kv, ffi.ATTN_DENSE if tt is None else ffi.ATTN_MEDIA, case.n_visual, tt_stride, tt_offset)
    d.q, d.k, d.v, d.o = (strides_of(T[n], dt) for n in ("q", "k", "v", "o"))
    d.dq, d.dk, d.dv, d.dout = (strides_of(T[n], dt) for n in ("dq", "dk", "dv", "do"))
    need = int(lib.ff_attention_bwd_workspace_bytes(d))
    assert need == ac.B * ac.H * n_q * 4
    ws = Buf(need // 4, F32)
    ws.claim(ws.body)
    bufs.append(ws)
    before = [b.bits.clone() for b in bufs]
    tt_before = None if tt is None else tt.clone()
    stream = ffi.stream_handle(T["q"].device)
    ffi.check(lib.ff_attention_fwd(d, T["q"].data_ptr(), T["k"].data_ptr(), T["v"].data_ptr(), ffi.ptr(tt), T["o"].data_ptr(), lse.data_ptr(),
                                   stream), "ff_attention_fwd")
    torch.cuda.synchronize()
    o_bits, lse_bits = T["o"].contiguous().view(BITS[dt]).clone(), lse.view(torch.int32).clone()
    ffi.check(lib.ff_attention_bwd(d, T["q"].data_ptr(), T["k"].data_ptr(), T["v"].data_ptr(), ffi.ptr(tt), T["o"].data_ptr(), T["do"].data_ptr(),
                                   lse.data_ptr(), T["dq"].data_ptr(), T["dk"].data_ptr(), T["dv"].data_ptr(), ws.body.data_ptr(), need, stream),
              "ff_attention_bwd")
    torch.cuda.synchronize()
    for buf, was in zip(bufs, before):
        assert buf.outside_intact(), f"{case.name} [{layout}]: an element outside every view was written"
        same = (buf.bits == was) | buf.inside
        assert bool(same.all())
    for name in ("q", "k", "v", "do"):
        assert torch.equal(T[name].cpu().view(BITS[dt]), getattr(case, name).view(BITS[dt])), f"{case.name} [{layout}]: {name} was written"
    assert torch.equal(T["o"].contiguous().view(BITS[dt]), o_bits) and torch.equal(lse.view(torch.int32), lse_bits), "the backward wrote o or lse"
    assert tt is None or torch.equal(tt, tt_before)
    out = {name: T[name].contiguous().cpu() for name in ("o", "dq", "dk", "dv")}
    out["lse"] = lse.cpu()
    return out


def held(case, got, ref=None):
    """every output against the float64 reference by util.attn_bound_ok; prints and collects every figure, then asserts"""
    ref = case.ref() if ref is None else ref
    res = {what: attn_bound_ok(what, got[what], ref, case.dtype) for what in OUTPUTS}
    print(f"{case.name}: " + " ".join(f"{what} {w:.3f}" for what, (ok, w, idx) in res.items()))
    for what, (ok, w, idx) in res.items():
        key = (ac.name_of(case.dtype), what)
        WORST[key] = max(WORST.get(key, (0.0, "")), (w, case.name))
    for what, (ok, w, idx) in res.items():
        assert ok, f"{case.name}: {what} element {idx} is {w:.4g} x its bound"
    return ref


def bits(t):
    return t.view(BITS.get(t.dtype, torch.int32))


INST_IDS = [f"{ac.name_of(t)}-{d}" for t, d in ac.DENSE_INST]


@pytest.mark.parametrize("n_q,n_kv", ac.DENSE_SHAPES, ids=[f"{a}x{b}" for a, b in ac.DENSE_SHAPES])
@pytest.mark.parametrize("dtype,dh", ac.DENSE_INST, ids=INST_IDS)
def test_dense_every_instantiation_within_the_element_bounds(dtype, dh, n_q, n_kv):
    """lse, o, dq, dk, dv element by element under all nine input patterns; (1, 1) and n_q = 1 are cases like any other: with one key
    d q and d k are exactly 0 in float64, and what the kernel leaves (D comes from the rounded O) is inside the u_T term of their bounds"""
    for case in ac.dense_cases(dtype, dh, [(n_q, n_kv)]):
        held(case, run(case))
    print({k: v for k, v in WORST.items() if k[0] == ac.name_of(dtype)})


@pytest.mark.parametrize("nv,n_media", ac.MEDIA_KEYS, ids=[f"nv{a}x{b}" for a, b in ac.MEDIA_KEYS])
@pytest.mark.parametrize("dtype,dh", ac.MEDIA_INST, ids=[f"{ac.name_of(t)}-{d}" for t, d in ac.MEDIA_INST])
def test_media_mixed_blocks_within_the_element_bounds(dtype, dh, nv, n_media):
    """One workgroup with zero rows, rows on every image and uniform rows in each of its waves, one of zero rows only, a ragged one on the
    last image; key ranges inside a 16-key sub-block (8), across 64-key tiles (40) and longer than a tile (72); flat and sharp scores."""
    for case in ac.media_cases(dtype, dh, [(nv, n_media)]):
        got = run(case)
        ref = held(case, got)
        zero, uni = torch.from_numpy(ref["kinds"] == 0), torch.from_numpy(ref["kinds"] == 2)
        assert int(zero[:, 64:128].sum()) == 2 * 64 and int(zero[:, :64].sum()) >= 8 and int(uni[:, :64].sum()) >= 16
        assert int((got["o"][zero] != 0).sum()) == 0 and int((got["dq"][zero] != 0).sum()) == 0, "a text_time = 0 row is not exactly zero"
        assert int((got["dq"][uni] != 0).sum()) == 0, "a uniform row got a q gradient"
        assert bool((got["lse"].permute(0, 2, 1)[zero] == float(ac.POS_BIG)).all())
        mean_v = case.v.double().mean(dim=1, keepdim=True).expand(-1, case.n_q, -1, -1)          # what o* of a uniform row is
        assert torch.allclose(torch.from_numpy(ref["o"])[uni], mean_v[uni], rtol=1e-12, atol=1e-14)
        # d k, d v of the reference take nothing from zero rows and d k nothing from uniform rows: the bounds above hold the kernel's to that
        assert float(np.abs(ref["p"][np.broadcast_to((ref["kinds"] == 0)[:, None], ref["p"].shape[:3])]).max()) == 0.0


LAYOUT_INST = [(BF16, 64), (F32, 32)]
_TWIN = {}


def layout_case(dtype, dh, mode):
    if mode == "dense":
        return ac.make_case(dtype, dh, 130, 200, "scales")
    return ac.make_case(dtype, dh, ac.MEDIA_NQ, 160, "flat", ac.media_text_time(ac.MEDIA_NQ, 4), 40)


def contiguous_twin(dtype, dh, mode):
    """the contiguous call on the same values, held by the bounds: computed once, shared by the layouts and left unchanged"""
    key = (dtype, dh, mode)
    if key not in _TWIN:
        case = layout_case(dtype, dh, mode)
        got = run(case)
        held(case, got)
        _TWIN[key] = got
    return _TWIN[key]


@pytest.mark.parametrize("layout", [k for k in LAYOUTS if k != "contiguous"])
@pytest.mark.parametrize("mode", ["dense", "media"])
@pytest.mark.parametrize("dtype,dh", LAYOUT_INST, ids=[f"{ac.name_of(t)}-{d}" for t, d in LAYOUT_INST])
def test_layouts_are_bit_equal_to_the_contiguous_call(dtype, dh, mode, layout):
    """The eight ff_strides and tt_stride / tt_offset: the layout does not enter the arithmetic, so every output is bit for bit that of
    the contiguous call; run() itself asserts that nothing outside a view and no input was written."""
    twin = contiguous_twin(dtype, dh, mode)
    got = run(layout_case(dtype, dh, mode), layout)
    for what in OUTPUTS:
        assert torch.equal(bits(got[what]), bits(twin[what])), f"{layout}: {what} differs from the contiguous call"


@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
def test_rejected_descriptors_launch_nothing(dtype):
    """Host checks: each returns its error code (include/flamingo_fusion.h) and leaves every output as it was."""
    from flamingo_mini_amd import ffi
    lib, dh, n_q, n_kv, nv = ffi.lib(), 64, 70, 80, 40
    T, bufs = {}, []
    for name, n in (("q", n_q), ("k", n_kv), ("v", n_kv), ("o", n_q), ("do", n_q), ("dq", n_q), ("dk", n_kv), ("dv", n_kv)):
        buf, T[name] = place("c", n, dh, dtype)
        T[name].fill_(float("nan") if name in ("o", "dq", "dk", "dv") else 0.5)
        bufs.append(buf)
    lse_buf = Buf(ac.B * ac.H * n_q, F32)
    lse = lse_buf.claim(lse_buf.body.view(ac.B, ac.H, n_q))
    lse.fill_(float("nan"))
    ws = Buf(ac.B * ac.H * n_q, F32)
    bufs += [lse_buf, ws]
    tt = torch.ones((ac.B, n_q), dtype=torch.int32, device="cuda")
    stream = ffi.stream_handle(tt.device)
    before = [b.bits.clone() for b in bufs]

    def desc(dim_head=dh, n_keys=n_kv, mode=ffi.ATTN_MEDIA):
        d = ffi.AttnDesc(ffi.dtype_code(dtype), ac.B, ac.H, dim_head, n_q, n_keys, mode, nv, n_q, 0)
        d.q, d.k, d.v, d.o = (strides_of(T[n], dtype) for n in ("q", "k", "v", "o"))
        d.dq, d.dk, d.dv, d.dout = (strides_of(T[n], dtype) for n in ("dq", "dk", "dv", "do"))
        return d

    def fwd(d, tt_=tt):
        return lib.ff_attention_fwd(d, T["q"].data_ptr(), T["k"].data_ptr(), T["v"].data_ptr(), ffi.ptr(tt_), T["o"].data_ptr(), lse.data_ptr(), stream)

    def bwd(d, tt_=tt, ws_ptr=ws.body.data_ptr(), ws_bytes=ac.B * ac.H * n_q * 4):
        return lib.ff_attention_bwd(d, T["q"].data_ptr(), T["k"].data_ptr(), T["v"].data_ptr(), ffi.ptr(tt_), T["o"].data_ptr(), T["do"].data_ptr(),
                                    lse.data_ptr(), T["dq"].data_ptr(), T["dk"].data_ptr(), T["dv"].data_ptr(), ws_ptr, ws_bytes, stream)

    odd = desc()
    odd.k.sr += 1                                    # a stride that is no multiple of 16 bytes
    assert fwd(odd) == FF_ERR_UNSUPPORTED and bwd(odd) == FF_ERR_UNSUPPORTED
    odd = desc()
    odd.dv.sh += VEC[dtype] // 2                     # ... on a gradient tensor: the backward only
    assert bwd(odd) == FF_ERR_UNSUPPORTED
    assert fwd(desc(dim_head=48)) == FF_ERR_UNSUPPORTED and bwd(desc(dim_head=48)) == FF_ERR_UNSUPPORTED
    assert fwd(desc(n_keys=n_kv - 8)) == FF_ERR_SHAPE and bwd(desc(n_keys=n_kv - 8)) == FF_ERR_SHAPE      # 72 keys, 40 per image
    assert fwd(desc(), None) == FF_ERR_SHAPE and bwd(desc(), None) == FF_ERR_SHAPE                          # media mode without text_time
    assert bwd(desc(), ws_bytes=ac.B * ac.H * n_q * 4 - 4) == FF_ERR_WORKSPACE and bwd(desc(), ws_ptr=None) == FF_ERR_WORKSPACE
    assert int(lib.ff_attention_bwd_workspace_bytes(desc())) == ac.B * ac.H * n_q * 4
    torch.cuda.synchronize()
    for buf, was in zip(bufs, before):
        assert torch.equal(buf.bits, was), "a rejected call wrote something"
    assert b"workspace" in lib.ff_last_error()
