"""Inputs, stage references and restatement of the per-element tests of the fused cross-attention block (a helper module, not a conftest):
shared by tests/test_hip_xattn_bounds.py (the kernels), tests/test_xattn_cases.py (the checkers, on the CPU) and tools/xattn_c.py (the
checkers' constants).

ff_xattn_block_fwd stores every stage's result in `saved`, ff_xattn_block_bwd_kv_data leaves d y1, d H and d Qs in the stash and d K / d V
in `dkv`.  Each stage is therefore judged from what the kernel STORED for the stage before (stage_checks), with the bounds the project
already has (util.gemm_bound_ok, util.attn_bound_ok): tight per-element bounds through the composed block without a bound for the
composition.

  F1  Qs                        scale . yn . Wq^T from the stored yn
  F2  lse, O                    attn_cases.attention_ref(Qs, K, V, tt) from the stored Qs
  F3  attn_out, y1              O . Wo^T and y + tanh(alpha_attn) . attn_out from the stored O
  F4  Hpre, Aact, ffw_out, y_out   from the stored xn_f, Aact and y1
  B1  d H                       from d y_out, W3, the stored Hpre and the gate
  B2  d Qs, d K, d V            attention_ref(Qs, K, V, dO*, tt), dO* = tanh(alpha_attn) . d y1 . Wo in float64 from the stored d y1; the
                                kernels form d O themselves and never store it, so the bound gains the terms attention_ref(e_do=) gives

One case per kernel path of csrc/ff_xattn_fused.hip (and the decode feed-forward of csrc/ff_decode.hip) at the smallest shape that takes it
(CASES); K and V come from outside the block (cached_k / cached_v strides, as after ff_kv_project_fwd), so they can be designed."""
import zlib

import numpy as np
import torch

import attn_cases as ac
from oracle import flamingo_oracle as O
from util import attn_bound_ok, gemm_bound_ok

BF16, F32 = torch.bfloat16, torch.float32
FF_MULT = 2
EPS = float(np.float32(1e-5))
GAP = ac.GAP
PATTERNS = ["flat", "sharp-rows", "offset", "scales"]
K_SCALES, DO_SCALES = [0.0, 1e-3, 1.0, 6.0, 25.0], [1.0, 1e-3, 40.0]
KIND = {0: "zero row", 1: "image row", 2: "uniform row"}
ALPHA_ATTN, ALPHA_FFW = 0.55, 0.4

# (name, dtype, heads, dim_head, b, L, n_visual, n_media, dim, sync, forward tile, ring depth, backward tile, ffw, tt_stride, tt_offset)
#   forward tile: ff_gemm_profile_record.tile of the fused forward launch (-4 alone, -6 with to_out, -8 with to_out and LN(y1)), ring depth
#   its b_layout (0 = the general kernel); backward tile: -5 alone, -7 with d LN(y), -9 with the LayerNorm backward behind it; ffw: "decode"
#   = the two launches of csrc/ff_decode.hip (tiles -10 and -11), which also keep to_out out of the fused launch at <= 32 rows.
#   res-*: the resident-operand kernels (bf16, 8 heads x 64, <= 32 tokens and <= 64 keys per sample): ring 6 needs dim >= 384, dim 256 has
#   only four k-steps, at dim 1536 six stages no longer fit the LDS; 4 x 16 and 2 x 32 keys put several images into the one key tile
#   (ranges with lo > 0), 3 x 20 = 60 keys leave the tile ragged.  phase3-*: with a sync buffer, to_out / LN(y1) forward and d LN(y) / the
#   LayerNorm backward run inside the launch.  decode: one token per sample, text_time rows of stride 24 read at offset 23.
#   general-*: dim_head 128 (two key tiles of 2 x 40 keys), 64-row query tiles, several query tiles (the backward then leaves d K / d V to
#   attention_bwd_dkv), and the four fp32 head sizes over 5 x 8 and 4 x 40 keys.
CASES = [
    ("res-ring6", BF16, 8, 64, 3, 20, 16, 4, 384, False, -4, 6, -5, "separate", 20, 0),
    ("res-ring4-ragged", BF16, 8, 64, 3, 32, 20, 3, 256, False, -4, 4, -5, "separate", 32, 0),
    ("res-ring4-lds", BF16, 8, 64, 5, 7, 64, 1, 1536, False, -4, 4, -5, "separate", 7, 0),
    ("phase3-dim256", BF16, 8, 64, 3, 20, 32, 2, 256, True, -8, 4, -9, "phase3", 20, 0),
    ("phase3-dim1280", BF16, 8, 64, 3, 32, 32, 2, 1280, True, -8, 6, -9, "phase3", 32, 0),
    ("decode", BF16, 8, 64, 5, 1, 32, 2, 1280, True, -4, 6, -7, "decode", 24, 23),
    ("general-bf16-dh128", BF16, 2, 128, 2, 24, 40, 2, 256, False, -4, 0, -5, "separate", 24, 0),
    ("general-bf16-bm64", BF16, 2, 64, 2, 48, 72, 3, 128, False, -4, 0, -5, "separate", 48, 0),
    ("general-bf16-multitile", BF16, 2, 64, 2, 130, 72, 3, 128, False, -4, 0, -5, "separate", 130, 0),
    ("general-f32-dh16", F32, 4, 16, 2, 70, 8, 5, 128, False, -4, 0, -5, "separate", 70, 0),
    ("general-f32-dh32", F32, 4, 32, 3, 40, 40, 4, 256, False, -4, 0, -5, "separate", 40, 0),
    ("general-f32-dh64", F32, 2, 64, 2, 20, 8, 5, 128, False, -4, 0, -5, "separate", 20, 0),
    ("general-f32-dh128", F32, 2, 128, 2, 33, 40, 4, 256, False, -4, 0, -5, "separate", 33, 0),
]
CASE_IDS = [row[0] for row in CASES]


def name_of(dtype):
    return "bf16" if dtype == BF16 else "f32"


def _rng(*key):
    return np.random.default_rng(zlib.crc32(repr(key).encode()))


def to_dtype(a, dtype):
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(dtype)


def f64(t):
    return t.detach().double().cpu().numpy()


def text_time(b, L, n_media):
    """(b, L) int32, after attn_cases.media_text_time: t cycles through 0 (zero row), 1..n_media (one image each), n_media + 1 and
    n_media + 3 (uniform rows) - the cycle has at most 8 entries, so every 16-row wave holds all kinds -, each sample starting the cycle
    elsewhere; where b >= 3 sample 1 has zero rows only; with L = 1 the samples differ in kind."""
    cyc = [0] + list(range(1, n_media + 1)) + [n_media + 1, n_media + 3]
    tt = np.zeros((b, L), np.int32)
    for s in range(b):
        tt[s] = [cyc[(i + (2 * s if L > 1 else s)) % len(cyc)] for i in range(L)]
    if b >= 3 and L > 1:
        tt[1] = 0
    return tt


def ln64(x, gamma, beta):
    mu = x.mean(-1, keepdims=True)
    var = ((x - mu) ** 2).mean(-1, keepdims=True)
    return (x - mu) / np.sqrt(var + EPS) * gamma + beta


class Case:
    """One (case, pattern): CPU tensors in the case's dtype - y (b, L, dim), the block's eleven parameters in the order of
    include/flamingo_fusion.h, kv (b, n_kv, 2 * inner) with K in the first half of a row, dyo (b, L, dim) - and text_time: tt_buf
    (b, tt_stride) as the kernel receives it, tt (b, L) the window at tt_offset it is to read.  qt (b, L, heads, dim_head) float64: the q
    the kernel will form, round_T(scale . LN(y) . Wq^T) with LN(y) rounded to T first, which K is designed from."""

    def __init__(self, row, pattern="flat"):
        (self.name, self.dtype, self.heads, self.dh, self.b, self.L, self.nv, self.n_media, self.dim, self.sync, self.tile, self.ring,
         self.bwd_tile, self.ffw, self.tt_stride, self.tt_offset) = row
        self.pattern, self.case = pattern, row[0]
        self.name = f"{row[0]}-{pattern}"
        dt, b, L, d, H, dh = self.dtype, self.b, self.L, self.dim, self.heads, self.dh
        self.rows, self.inner, self.ffi, self.n_kv = b * L, H * dh, FF_MULT * d, self.nv * self.n_media
        self.scale = float(np.float32(1.0) / np.sqrt(np.float32(dh)))
        self.resident = self.ring != 0
        self.bm = 32 if L <= 32 else 64                      # queries per workgroup of the fused kernels
        g = _rng("xattn", row[0], pattern)
        # text_time: the window, inside rows of tt_stride entries whose other entries would give other kinds
        self.tt = text_time(b, L, self.n_media)
        self.tt_buf = g.integers(0, self.n_media + 4, size=(b, self.tt_stride)).astype(np.int32)
        if self.tt_offset:
            self.tt_buf[:, 0] = np.where(self.tt[:, 0] == 0, 1, 0)          # read without the offset, every sample changes its kind
        self.tt_buf[:, self.tt_offset:self.tt_offset + L] = self.tt
        self.lo, self.hi, sm, un = ac.row_ranges(self.tt, L, self.n_kv, self.nv)
        self.kinds = np.where(sm == 1, 1, np.where(un == 1, 2, 0))
        # y: N(0, 1) with a few constant rows (their LN output is exactly beta: they share one q)
        y = g.standard_normal((b * L, d))
        self.const_rows = [r for r in range(b * L) if r % 11 == 5] if b * L >= 6 else [b * L - 1]
        for r in self.const_rows:
            y[r] = (0.5, -1.5, 2.0)[r % 3]
        self.y = to_dtype(y.reshape(b, L, d), dt)
        beta_scale = 3.0 if pattern == "offset" else 0.5                    # offset: the common part of every q dominates its scores
        w = lambda o, i: to_dtype(g.standard_normal((o, i)) * i ** -0.5, dt)
        a = lambda v: to_dtype(np.array([v]), dt)
        self.params = [a(ALPHA_ATTN), a(ALPHA_FFW), to_dtype(1.0 + 0.1 * g.standard_normal(d), dt), to_dtype(beta_scale * g.standard_normal(d), dt),
                       w(self.inner, d), to_dtype(np.zeros((8, 8)), dt), w(d, self.inner), to_dtype(1.0 + 0.1 * g.standard_normal(d), dt),
                       to_dtype(0.2 * g.standard_normal(d), dt), w(self.ffi, d), w(d, self.ffi)]
        gamma, beta, Wq = f64(self.params[2]), f64(self.params[3]), f64(self.params[4])
        yn = f64(to_dtype(ln64(f64(self.y).reshape(b * L, d), gamma, beta), dt))
        for r in self.const_rows:
            assert np.array_equal(yn[r], beta), "a constant row's LN output is beta"
        self.qt = f64(to_dtype(self.scale * (yn @ Wq.T), dt)).reshape(b, L, H, dh)
        # K, V, d y_out
        k, v = g.standard_normal((b, self.n_kv, H, dh)), g.standard_normal((b, self.n_kv, H, dh))
        dyo = g.standard_normal((b, L, d))
        self.S = 0.0
        if pattern == "sharp-rows":
            k = self._sharp(k)
        elif pattern == "offset":           # every key gets t c_h / |c_h|^2 added, t = +200 / -200 alternating by head: all scores near +-200
            c = self.scale * (Wq @ beta).reshape(H, dh)                      # the common part of every q
            t = 200.0 * np.where(np.arange(H) % 2 == 0, 1.0, -1.0)
            k = k + (t[:, None] * c / (c * c).sum(-1, keepdims=True))[None, None]
        elif pattern == "scales":
            k = k * np.asarray(K_SCALES)[np.arange(self.n_kv) % 5][None, :, None, None]
            dyo = dyo * np.asarray(DO_SCALES)[np.arange(L) % 3][None, :, None]
        else:
            assert pattern == "flat", pattern
        self.kv = to_dtype(np.concatenate([k.reshape(b, self.n_kv, self.inner), v.reshape(b, self.n_kv, self.inner)], -1), dt)
        self.dyo = to_dtype(dyo, dt)

    def _sharp(self, k):
        """row i's dominant key is lo + (37 i + 11) mod n inside its own range, k_j = S q_i / |q_i|^2; a row whose key is already taken
        keeps it.  S: the smallest of a few candidates that puts the best score of at least 60 % of the softmax (row, head) pairs 1.1 GAP
        above the next one (the keys are rounded to T afterwards, and the kernel's own q may differ from qt in the last place)."""
        b, L, H = self.b, self.L, self.heads
        owner = -np.ones((b, self.n_kv), np.int64)
        dom = np.zeros((b, L), np.int64)
        for s in range(b):
            for i in range(L):
                if self.kinds[s, i] == 1:
                    j = int(self.lo[s, i] + (37 * i + 11) % self.nv)
                    dom[s, i] = j
                    if owner[s, j] < 0 and (self.qt[s, i] ** 2).sum(-1).min() > 0:
                        owner[s, j] = i
        self.dom = dom
        unit = np.zeros_like(k)
        for s in range(b):
            for j in range(self.n_kv):
                if owner[s, j] >= 0:
                    q = self.qt[s, owner[s, j]]
                    unit[s, j] = q / (q * q).sum(-1, keepdims=True)
        designed = (owner >= 0)[:, :, None, None]
        for S in (150.0, 250.0, 400.0, 700.0, 1200.0, 2000.0):
            kk = np.where(designed, S * unit, k)
            frac = sharp_fraction(self, self.qt, f64(to_dtype(kk, self.dtype)), 1.1 * GAP)
            if frac >= 0.6:
                break
        self.S = S
        return kk

    # what the tests and the restatement take apart
    def K4(self):
        return self.kv[..., :self.inner].reshape(self.b, self.n_kv, self.heads, self.dh)

    def V4(self):
        return self.kv[..., self.inner:].reshape(self.b, self.n_kv, self.heads, self.dh)

    def kind_of(self, s, i):
        return f"{KIND[int(self.kinds[s, i])]}, text_time {int(self.tt[s, i])}"


def all_cases(patterns=PATTERNS):
    for row in CASES:
        for p in patterns:
            yield Case(row, p)


# ---- the conditions on the inputs (on the CPU from qt, on the device from the stored Qs) --------------------------------------------------
def _scores(case, q4, k4):
    """(s (b, h, L, n_kv) float64, seen (b, 1, L, n_kv)) for the softmax rows' own ranges"""
    key = np.arange(case.n_kv)[None, None, :]
    seen = (key >= case.lo[:, :, None]) & (key < case.hi[:, :, None]) & (case.kinds == 1)[:, :, None]
    s = np.einsum("bihd,bjhd->bhij", np.asarray(q4, np.float64), np.asarray(k4, np.float64))
    return s, seen[:, None]


def sharp_fraction(case, q4, k4, gap=GAP):
    """fraction of the softmax (row, head) pairs whose best score is at least `gap` above the next one of the row's range"""
    s, seen = _scores(case, q4, k4)
    sm = np.sort(np.where(seen, s, -np.inf), axis=-1)
    rows = np.broadcast_to((case.kinds == 1)[:, None, :], sm.shape[:3])
    with np.errstate(invalid="ignore"):
        ok = (sm[..., -1] - sm[..., -2] >= gap) & rows
    return float(ok.sum()) / max(int(rows.sum()), 1)


def min_abs_score(case, q4, k4):
    s, seen = _scores(case, q4, k4)
    return float(np.abs(s)[np.broadcast_to(seen, s.shape)].min())


def kinds_present(case):
    """text_time kinds among the rows: zero, every image, n_media + 1 and n_media + 3"""
    return set(int(t) for t in case.tt.reshape(-1)) >= set([0, case.n_media + 1, case.n_media + 3] + list(range(1, case.n_media + 1)))


def check_conditions(case, q4, k4, where):
    assert kinds_present(case), f"{case.name}: a text_time kind is missing"
    if case.pattern == "sharp-rows":
        frac = sharp_fraction(case, q4, k4)
        assert frac >= 0.5, f"{case.name} ({where}): only {frac:.2f} of the softmax rows have their best score {GAP} above the next (S = {case.S})"
    if case.pattern == "offset":
        m = min_abs_score(case, q4, k4)
        assert m >= 100.0, f"{case.name} ({where}): a score of a softmax row has magnitude {m:.1f} < 100"


# ---- the stage checks ---------------------------------------------------------------------------------------------------------------------
FWD_KEYS = ("yn", "Qs", "lse", "O", "attn_out", "y1", "xn_f", "Hpre", "Aact", "ffw_out", "y_out")
BWD_KEYS = ("dy1", "dH", "dQs", "dkv")


def _act_epi(acc):
    return O.act_fwd(acc, "gelu"), np.abs(O.act_bwd(np.ones_like(acc), acc, "gelu"))


def attention_refs(case, st, backward=True):
    """attention_ref for F2 (and B2) from the stored Qs (and d y1); with the backward: dO* = tanh(alpha_attn) d y1 Wo in float64 and e_do,
    gemm_bound_ok's own bound for that product (its output rounding included), which attention_ref turns into e_dq / e_dk / e_dv"""
    b, L, H, dh = case.b, case.L, case.heads, case.dh
    Q4 = st["Qs"].reshape(b, L, H, dh)
    if not backward:
        return ac.attention_ref(Q4, case.K4(), case.V4(), None, case.tt, case.nv)
    g1 = float(np.tanh(f64(case.params[0])[0]))
    dy1, Wo = f64(st["dy1"]).reshape(case.rows, case.dim), f64(case.params[6])
    dO = g1 * (dy1 @ Wo)
    u_out = 2.0 ** -7 if case.dtype == BF16 else 2.0 ** -22
    e = u_out * np.abs(dO) + 2.0 * case.dim * 2.0 ** -24 * abs(g1) * (np.abs(dy1) @ np.abs(Wo))
    return ac.attention_ref(Q4, case.K4(), case.V4(), dO.reshape(b, L, H, dh), case.tt, case.nv, e_do=e.reshape(b, L, H, dh))


def stage_checks(case, st, backward=True, ref=None):
    """st: what the block stored (FWD_KEYS, and BWD_KEYS with the backward), CPU tensors.  Every stage of the table from the stored result
    of the stage before.  Returns a list of (stage, what, ok, worst error / bound, where): `where` names the element - sample, token or key,
    head or column, and the row's text_time kind.  Nothing is excluded, NaN counts as inf; conditions that are not bounds (a zero row's lse
    is the sentinel, its attn_out is 0 and its y1 is y bit for bit) appear as entries of their own with worst = inf when they fail."""
    dt, b, L, H, dh, d = case.dtype, case.b, case.L, case.heads, case.dh, case.dim
    rows, P = case.rows, case.params
    res = []
    g1, g2 = float(np.tanh(f64(P[0])[0])), float(np.tanh(f64(P[1])[0]))
    u_act = 2.0 ** -8 if dt == BF16 else 2.0 ** -19          # as tests/test_hip_bounds.py::test_gemm_epilogues_guarded
    u_out_act = None if dt == BF16 else u_act

    def row_where(idx, per_head):
        r, c = idx
        s, i = divmod(int(r), L)
        col = f"head {c // dh}, column {c % dh}" if per_head else f"column {c}"
        return f"sample {s}, token {i}, {col} ({case.kind_of(s, i)})"

    def gemm(stage, what, C, A, B, per_head=False, **kw):
        ok, worst, idx = gemm_bound_ok(C, A, B, **kw)
        res.append((stage, what, ok, worst, row_where(idx, per_head)))

    def exact(stage, what, ok, where):
        res.append((stage, what, bool(ok), 0.0 if ok else float("inf"), where))

    y2 = case.y.reshape(rows, d)
    zero_rows = np.nonzero(case.kinds.reshape(-1) == 0)[0]
    zr = torch.from_numpy(zero_rows)
    bits = lambda t: t.contiguous().view(torch.int16 if t.dtype == BF16 else torch.int32)
    # F1
    gemm("F1", "Qs", st["Qs"].reshape(rows, case.inner), st["yn"].reshape(rows, d), P[4], per_head=True, scale=case.scale)
    # F2 (and the reference of B2)
    if ref is None:
        ref = attention_refs(case, st, backward)
    lse, O4 = st["lse"].reshape(b, H, L), st["O"].reshape(b, L, H, dh)
    ok, worst, (s, h, i) = attn_bound_ok("lse", lse, ref, dt)
    res.append(("F2", "lse", ok, worst, f"sample {s}, token {i}, head {h} ({case.kind_of(s, i)})"))
    ok, worst, (s, i, h, c) = attn_bound_ok("o", O4, ref, dt)
    res.append(("F2", "O", ok, worst, f"sample {s}, token {i}, head {h}, column {c} ({case.kind_of(s, i)})"))
    zl = lse.float().permute(0, 2, 1).reshape(rows, H)[zr]
    exact("F2", "lse of zero rows", bool((zl == float(ac.POS_BIG)).all()), "a text_time = 0 row's lse is not the sentinel 1e30")
    # F3
    O2 = st["O"].reshape(rows, case.inner)
    gemm("F3", "attn_out", st["attn_out"].reshape(rows, d), O2, P[6])
    gemm("F3", "y1", st["y1"].reshape(rows, d), O2, P[6], epilogue=lambda a: (f64(y2) + g1 * a, np.full_like(a, g1)))
    exact("F3", "attn_out of zero rows", int((st["attn_out"].reshape(rows, d)[zr].float() != 0).sum()) == 0 or
          int((O2[zr].float() != 0).sum()) != 0, "a text_time = 0 row's attn_out is not exactly 0")
    exact("F3", "y1 of zero rows", torch.equal(bits(st["y1"].reshape(rows, d)[zr]), bits(y2[zr])) or int((O2[zr].float() != 0).sum()) != 0,
          "a text_time = 0 row's y1 is not y bit for bit")
    # F4
    xn, A2, y1 = st["xn_f"].reshape(rows, d), st["Aact"].reshape(rows, case.ffi), st["y1"].reshape(rows, d)
    gemm("F4", "Hpre", st["Hpre"].reshape(rows, case.ffi), xn, P[9])
    gemm("F4", "Aact", A2, xn, P[9], epilogue=_act_epi, u_mid=u_act, u_out=u_out_act)
    gemm("F4", "ffw_out", st["ffw_out"].reshape(rows, d), A2, P[10])
    gemm("F4", "y_out", st["y_out"].reshape(rows, d), A2, P[10], epilogue=lambda a: (f64(y1) + g2 * a, np.full_like(a, g2)))
    if not backward:
        return res
    # B1
    hp = f64(st["Hpre"]).reshape(rows, case.ffi)
    dgate = g2 * O.act_bwd(np.ones((rows, case.ffi)), hp, "gelu")
    # fp32: the factor is cdf(h) + h pdf(h), two terms of opposite sign for h < 0 that cancel at h = -0.75; a float32 evaluation (erff,
    # __expf) is off in proportion to the size of the two terms, not to their difference (as util.quick_gelu_ref has it for QuickGELU), so
    # what the bound scales is |cdf| + |h pdf|.  bf16 keeps |factor|: there the factor's own error is 2^-14 of the output's rounding.
    pdf = np.exp(-0.5 * hp * hp) / np.sqrt(2.0 * np.pi)
    size = np.abs(dgate) if dt == BF16 else abs(g2) * (O.act_bwd(np.ones_like(hp), hp, "gelu") + (np.abs(hp) - hp) * pdf)      # cdf + |h| pdf
    gemm("B1", "dH", st["dH"].reshape(rows, case.ffi), case.dyo.reshape(rows, d), P[10], b_layout=1,
         epilogue=lambda a: (a * dgate, size), u_mid=u_act, u_out=u_out_act)
    # B2
    dkv = st["dkv"].reshape(b, case.n_kv, 2, H, dh)
    ok, worst, (s, i, h, c) = attn_bound_ok("dq", st["dQs"].reshape(b, L, H, dh), ref, dt, extra=True)
    res.append(("B2", "dQs", ok, worst, f"sample {s}, token {i}, head {h}, column {c} ({case.kind_of(s, i)})"))
    for what, part in (("dk", dkv[:, :, 0]), ("dv", dkv[:, :, 1])):
        ok, worst, (s, j, h, c) = attn_bound_ok(what, part, ref, dt, extra=True)
        res.append(("B2", "dK" if what == "dk" else "dV", ok, worst, f"sample {s}, key {j} (image {j // case.nv + 1}), head {h}, column {c}"))
    return res


def failures(case, res):
    return [f"{case.name}: stage {stage}, {what}: {where} is {worst:.4g} x its bound" for stage, what, ok, worst, where in res if not ok]


# ---- the block restated in float32 --------------------------------------------------------------------------------------------------------
MUTATIONS = {      # defect -> (the case it is injected into, the stage whose checker it belongs to)
    "range-shift": ("res-ring6", "F2"),              # a row's key range shifted by one key
    "drop-last-key": ("res-ring4-ragged", "F2"),     # the ragged last key of the key tile dropped
    "lse-log2": ("phase3-dim256", "F2"),             # lse off by log 2
    "zero-1e-30": ("general-f32-dh64", "F2"),        # a zero row's o = 1e-30
    "uniform-as-image": ("res-ring6", "F2"),         # a uniform row treated as an image row
    "swap-heads": ("phase3-dim1280", "F3"),          # two heads' slices of O swapped before to_out
    "no-gate": ("phase3-dim256", "F3"),              # the gate left out of y1
    "no-tt-offset": ("decode", "F2"),                # text_time read without tt_offset
    "D-drop-col": ("general-f32-dh32", "B2"),        # D taken from the unrounded O with a dropped d O column (in bf16 one column of 64
                                                     # is about what the rounding of O and of d O may do to D: not a defect the bound can see)
    "dk-neighbour": ("general-bf16-dh128", "B2"),    # d K accumulated over the rows of the neighbouring sample
    "no-scale": ("general-f32-dh32", "F1"),          # q without the 1 / sqrt(dim_head)
    "gelu-from-rounded": ("general-f32-dh16", "F4"), # fp32: the activation taken from a pre-activation cut to eight bits
    "dH-no-gate": ("general-bf16-bm64", "B1"),       # d H without tanh(alpha_ffw)
}
ATTN_MUT = ("range-shift", "drop-last-key", "lse-log2", "zero-1e-30", "uniform-as-image")


def _ln32(x, gamma, beta):
    f = np.float32
    mu = x.mean(-1, keepdims=True, dtype=f)
    var = ((x - mu) ** 2).mean(-1, keepdims=True, dtype=f)
    return ((x - mu) * (f(1) / np.sqrt(var + f(EPS))) * gamma + beta).astype(f)


def _gelu_cdf32(h, mutate=None):
    """gelu_cdf of csrc/ff_common.h on a float32 tensor: erfc(-h / sqrt 2) / 2; "erf-cdf": (1 + erf(h / sqrt 2)) / 2, what the fp32 kernels
    had until these tests measured its negative tail"""
    c = np.float32(0.70710678118654752440)
    return 0.5 * (1.0 + torch.erf(h * c)) if mutate == "erf-cdf" else 0.5 * torch.special.erfc(-c * h)


def block_f32(case, mutate=None, backward=True):
    """The block in float32 numpy, every stored tensor rounded to the case's dtype where the kernels round it: LN(y) (two passes; the
    LayerNorm kernels have their own restatements in tests/ln_cases.py), Qs = round(scale . acc), the attention by attn_cases.attn_fwd_f32 /
    attn_bwd_f32 with the fused kernels' tiling (`bm` queries per workgroup; the resident kernels see one key tile, so nothing is
    rescaled), attn_out = round(acc) and y1 = round(y + tanh(alpha) acc) from the SAME fp32 accumulator, the feed-forward likewise, and for
    the backward d O = round(tanh(alpha) . (d y1 . Wo)) - the product in float32, rounded to T before D = rowsum(dO . O) and the two
    passes use it (xa_dattn_bwd_kernel and xa_dattn_bwd_res_kernel park it as T in LDS).  d y1 itself comes from a float64 LayerNorm
    backward: it is an input of B2, not a result any stage here judges.  `mutate`: MUTATIONS.  Returns the dict stage_checks takes."""
    f, dt = np.float32, case.dtype
    b, L, H, dh, d, rows = case.b, case.L, case.heads, case.dh, case.dim, case.rows
    P = [p.float().numpy() for p in case.params]
    r = lambda a: ac._round(np.ascontiguousarray(a, f), dt)
    T = lambda a, shape: torch.from_numpy(np.ascontiguousarray(a, f)).to(dt).reshape(shape)
    g1, g2 = f(np.tanh(P[0][0])), f(np.tanh(P[1][0]))
    y = case.y.float().numpy().reshape(rows, d)
    st = {}
    yn = r(_ln32(y, P[2], P[3]))
    q = r(f(1.0 if mutate == "no-scale" else case.scale) * (yn @ P[4].T))
    st["yn"], st["Qs"] = T(yn, (b, L, d)), T(q, (b, L, case.inner))
    tt = case.tt_buf[:, :L] if mutate == "no-tt-offset" else case.tt
    amut = mutate if mutate in ATTN_MUT else None
    at = tuple(int(x) for x in np.argwhere(case.kinds == 1)[0])
    at = (at[0], H - 1, at[1])
    Q4, K4, V4 = st["Qs"].reshape(b, L, H, dh), case.K4(), case.V4()
    o, lse = ac.attn_fwd_f32(Q4, K4, V4, tt, case.nv, mutate=amut, at=at, bm=case.bm)
    st["O"], st["lse"] = o.reshape(b, L, case.inner), lse
    O2 = o.float().numpy().reshape(rows, case.inner)
    if mutate == "swap-heads":
        O2 = O2.copy()
        O2[:, :dh], O2[:, dh:2 * dh] = O2[:, dh:2 * dh].copy(), O2[:, :dh].copy()
    acc = O2 @ P[6].T
    y1 = r(y + (f(1) if mutate == "no-gate" else g1) * acc)
    st["attn_out"], st["y1"] = T(acc, (b, L, d)), T(y1, (b, L, d))
    xn = r(_ln32(y1, P[7], P[8]))
    acc1 = xn @ P[9].T
    hpre = r(acc1)
    src = torch.from_numpy(acc1 if mutate != "gelu-from-rounded" else torch.from_numpy(acc1).to(BF16).float().numpy())
    aact = r((src * _gelu_cdf32(src, mutate)).numpy())       # act_fwd of csrc/ff_common.h in float32
    acc3 = aact @ P[10].T
    st.update(xn_f=T(xn, (b, L, d)), Hpre=T(hpre, (b, L, case.ffi)), Aact=T(aact, (b, L, case.ffi)), ffw_out=T(acc3, (b, L, d)),
              y_out=T(y1 + g2 * acc3, (b, L, d)))
    if not backward:
        return st
    dyo = case.dyo.float().numpy().reshape(rows, d)
    ht = torch.from_numpy(hpre)                              # act_grad of csrc/ff_common.h in float32: cdf + h * pdf
    dact = (_gelu_cdf32(ht, mutate) + ht * (f(0.39894228040143267794) * torch.exp(-0.5 * ht * ht))).numpy()
    assert dact.dtype == f
    dH = r((dyo @ P[10]) * (f(1) if mutate == "dH-no-gate" else g2) * dact)
    dxn = (dH @ P[9]).astype(np.float64)
    x64, gam = y1.astype(np.float64), P[7].astype(np.float64)
    mu, var = x64.mean(-1, keepdims=True), x64.var(-1, keepdims=True)
    xh, gdy = (x64 - mu) / np.sqrt(var + EPS), dxn * gam
    dy1 = r((gdy - gdy.mean(-1, keepdims=True) - xh * (gdy * xh).mean(-1, keepdims=True)) / np.sqrt(var + EPS) + dyo)
    dO = T(g1 * (dy1 @ P[6]), (b, L, H, dh))
    kw = dict(tt=tt, n_visual=case.nv, mutate=amut, bm=case.bm)
    if mutate == "D-drop-col":
        o32, _ = ac.attn_fwd_f32(Q4, K4, V4, tt, case.nv, bm=case.bm, keep_f32=True)
        kw["D"] = (dO.float().numpy()[..., 1:] * o32.numpy()[..., 1:]).sum(-1, dtype=f).transpose(0, 2, 1)
    dq, dk, dv = ac.attn_bwd_f32(Q4, K4, V4, o, dO, lse, **kw)
    if mutate == "dk-neighbour":
        roll = lambda t: torch.roll(t, 1, 0)
        _, dk, _ = ac.attn_bwd_f32(roll(Q4), K4, V4, roll(o), roll(dO), roll(lse), tt=np.roll(tt, 1, 0), n_visual=case.nv, bm=case.bm)
    st.update(dy1=T(dy1, (b, L, d)), dH=T(dH, (b, L, case.ffi)), dQs=dq.reshape(b, L, case.inner),
              dkv=torch.cat([dk.reshape(b, case.n_kv, case.inner), dv.reshape(b, case.n_kv, case.inner)], -1))
    return st
