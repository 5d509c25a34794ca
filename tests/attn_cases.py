"""Inputs of the per-element attention tests (a helper module, not a conftest): the case table shared by
tests/test_hip_attention_bounds.py (the kernels), tests/test_attn_cases.py (the checkers, on the CPU) and tools/attn_c.py (the checkers'
constants); the float64 reference with the terms of util.attn_bound_ok; and restatements of attn_fwd_kernel, attn_bwd_dq_kernel and
attn_bwd_dkv_kernel (csrc/ff_attention.hip, csrc/ff_attention_core.h) in float32 numpy, in the kernels' operation order - what the
constants are measured with and what the CPU tests inject defects into.

All tensors are (b, n, h, d) with b = 2, h = 3.  Dense cases: the seven instantiations x four shapes x nine input patterns.  Media cases:
n_q = 170 text positions whose text_time is written by hand (media_text_time) over 5 x 8, 4 x 40 and 3 x 72 keys."""
import zlib

import numpy as np
import torch

from oracle import flamingo_oracle as O

BF16, F32 = torch.bfloat16, torch.float32
B, H, TILE = 2, 3, 64
NEG_BIG, POS_BIG = np.float32(-1.0e30), np.float32(1.0e30)          # kNegBig, kPosBig of csrc/ff_attention_core.h
TINY = np.float32(2.0 ** -126)
DENSE_INST = [(BF16, 32), (BF16, 64), (BF16, 128), (F32, 16), (F32, 32), (F32, 64), (F32, 128)]
DENSE_SHAPES = [(1, 1), (65, 63), (64, 130), (130, 200)]
SHARP = ["sharp-first", "sharp-mid", "sharp-last", "sharp-rows"]
PATTERNS = ["flat"] + SHARP + ["tied", "offset+", "offset-", "scales"]
MEDIA_INST = [(F32, 16), (F32, 64), (BF16, 64), (BF16, 128)]
MEDIA_KEYS = [(8, 5), (40, 4), (72, 3)]          # (n_visual, images): ranges inside a 16-key sub-block, straddling 64-key tiles, longer than a tile
MEDIA_NQ = 170                                    # block 0 mixed, block 1 all zero rows, block 2 (ragged) all on the last image
MEDIA_PATTERNS = ["flat", "sharp-rows"]
GAP = 95.0                                        # dominant score - the next one: exp(-95) = 5.5e-42 is below 2^-126 (the device's exp returns 0) and
                                                  # above 2^-149 (float32 still holds it, so the exact gradient of a key no row favours is not 0)
Q_SCALES, DO_SCALES = [0.0, 1e-3, 1.0, 6.0, 25.0], [1.0, 1e-3, 40.0]


def name_of(dtype):
    return "bf16" if dtype == BF16 else "f32"


def _rng(*key):
    return np.random.default_rng(zlib.crc32(repr(key).encode()))


def _stored(a, dtype):
    """float32 array -> what a tensor of `dtype` holds of it, as float64 numpy"""
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(dtype).double().numpy()


def dominant_keys(pattern, n_q, lo, hi):
    """(b, n_q): the key each row's score mass is put on; lo / hi (b, n_q): the row's key range"""
    i = np.arange(n_q)[None, :]
    n = np.maximum(hi - lo, 1)
    off = {"sharp-first": 0 * i, "sharp-mid": n // 2 + 0 * i, "sharp-last": n - 1 + 0 * i, "sharp-rows": (37 * i + 11) % n}[pattern]
    return lo + off % n


def media_text_time(n_q, n_media):
    """(B, n_q) int32.  Rows 0..63: t cycles through 0 (zero row), 1..n_media (one image each), n_media + 1 and n_media + 3 (uniform
    rows), so every 16-row wave of the first workgroup holds all four kinds, each sample starting the cycle elsewhere; rows 64..127: all 0;
    rows 128..: all on the last image."""
    cyc = [0] + list(range(1, n_media + 1)) + [n_media + 1, n_media + 3]
    tt = np.zeros((B, n_q), np.int32)
    for s in range(B):
        tt[s, :TILE] = [cyc[(i + 2 * s) % len(cyc)] for i in range(TILE)]
    tt[:, 2 * TILE:] = n_media
    return tt


def row_ranges(tt, n_q, n_kv, n_visual):
    """row_range of csrc/ff_attention_core.h: (lo, hi, softmax, uniform), each (B, n_q)"""
    if tt is None:
        z = np.zeros((B, n_q), np.int64)
        return z, z + n_kv, z + 1, z
    t = np.asarray(tt, np.int64)
    n_media = n_kv // n_visual
    zero, img = t <= 0, (t > 0) & (t <= n_media)
    lo = np.where(img, (t - 1) * n_visual, 0)
    hi = np.where(img, t * n_visual, np.where(zero, 0, n_kv))
    return lo, hi, img.astype(np.int64), (~zero & ~img).astype(np.int64)


class Case:
    """q, k, v, do: CPU tensors (b, n, h, d) in `dtype`; tt (B, n_q) int32 numpy or None (dense); n_visual"""

    def __init__(self, name, dtype, dh, q, k, v, do, tt=None, n_visual=0, pattern="flat"):
        self.name, self.dtype, self.dh, self.tt, self.n_visual, self.pattern = name, dtype, dh, tt, n_visual, pattern
        self.q, self.k, self.v, self.do = (torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(dtype) for a in (q, k, v, do))
        self.n_q, self.n_kv = q.shape[1], k.shape[1]

    def ref(self):
        return attention_ref(self.q, self.k, self.v, self.do, self.tt, self.n_visual)


def make_case(dtype, dh, n_q, n_kv, pattern, tt=None, n_visual=0):
    """One input set.  flat: q ~ N(0, 1/dh), k, v, dO ~ N(0, 1) - scores about N(0, 1).
    sharp-*: q_i = S k_j / |k_j|^2 for the row's dominant key j (key 0 of its range, the middle one, the last one, or (37 i + 11) mod n:
        another place for every row of a wave), S chosen from the stored keys so that the dominant score is S and every other one GAP below.
    tied: key n_kv - 2 is key 3 plus a twentieth of noise; q_i in the span of the two with scores S + (i mod 7 - 3) / 4 and S, every other
        key GAP below.  (The keys of the sharp and tied patterns are scaled to one norm, sqrt(dh).)
    offset+ / offset-: k_j[0:4] = 2 and q_i[0:4] = +-25: all scores of a row are +-200 + N(0, 1).
    scales: rows of q times (0, 1e-3, 1, 6, 25)[i mod 5], rows of dO times (1, 1e-3, 40)[i mod 3]: flat, exactly uniform, and sharp rows
        beside each other in every wave."""
    key = (name_of(dtype), dh, n_q, n_kv, pattern, n_visual)
    g = _rng(*key)
    q = g.standard_normal((B, n_q, H, dh)) * dh ** -0.5
    k, v, do = (g.standard_normal((B, n, H, dh)) for n in (n_kv, n_kv, n_q))
    lo, hi, sm, un = row_ranges(tt, n_q, n_kv, n_visual)
    seen = (np.arange(n_kv)[None, None, :] >= lo[:, :, None]) & (np.arange(n_kv)[None, None, :] < hi[:, :, None])       # (b, n_q, n_kv)
    bi = np.arange(B)[:, None]
    if pattern in SHARP or pattern == "tied":
        if pattern == "tied" and n_kv > 1:               # the second key close to the first: q near both and far from every other key
            k[:, max(n_kv - 2, 0)] = k[:, min(3, n_kv - 1)] + 0.05 * k[:, max(n_kv - 2, 0)]
        k = k / np.linalg.norm(k, axis=-1, keepdims=True) * dh ** 0.5      # equal norms: a longer key in the same direction would score higher
        ks = _stored(k, dtype)
        if pattern == "tied":
            j1, j2 = np.minimum(lo + 3, hi - 1), np.maximum(hi - 2, lo)
            j1, j2 = np.where(hi > lo, j1, 0), np.where(hi > lo, j2, 0)
            k1, k2 = ks[bi, j1], ks[bi, j2]                                                 # (b, n_q, h, d)
            g11, g12, g22 = (k1 * k1).sum(-1), (k1 * k2).sum(-1), (k2 * k2).sum(-1)
            det = g11 * g22 - g12 * g12
            same = (j1 == j2)[:, :, None] | (det < 1e-9 * g11 * g22)
            det = np.where(same, 1.0, det)
            al, be = (g22 - g12) / det, (g11 - g12) / det                                   # unit scores on both first: S scales them
            unit = np.where(same[..., None], k1 / g11[..., None], al[..., None] * k1 + be[..., None] * k2)
            dom = [j1, j2]
        else:
            j1 = dominant_keys(pattern, n_q, lo, hi)
            j1 = np.where(hi > lo, j1, 0)
            k1 = ks[bi, j1]
            unit = k1 / (k1 * k1).sum(-1, keepdims=True)
            dom = [j1]
        coef = np.einsum("bihd,bjhd->bhij", unit, ks)
        other = np.broadcast_to(seen[:, None], coef.shape).copy()
        for j in dom:
            np.put_along_axis(other, np.broadcast_to(j[:, None, :, None], coef.shape[:3] + (1,)), False, axis=3)
        cmax = float(coef[other].max()) if other.any() else 0.0
        S = GAP / max(1.0 - cmax, 1e-3)
        q = S * unit
        if pattern == "tied":                                                               # S + delta_i on the first key, S on the second
            delta = 0.25 * (np.arange(n_q) % 7 - 3)[None, :, None]
            q = q + np.where(same[..., None], 0.0, (delta * g22 / det)[..., None] * k1 - (delta * g12 / det)[..., None] * k2)
    elif pattern in ("offset+", "offset-"):
        k[..., :4] = 2.0
        q[..., :4] = 25.0 if pattern == "offset+" else -25.0
    elif pattern == "scales":
        q = q * np.asarray(Q_SCALES)[np.arange(n_q) % 5][None, :, None, None]
        do = do * np.asarray(DO_SCALES)[np.arange(n_q) % 3][None, :, None, None]
    else:
        assert pattern == "flat", pattern
    where = f"{n_q}x{n_kv}" if tt is None else f"media-nv{n_visual}x{n_kv // n_visual}"
    return Case(f"{name_of(dtype)}-dh{dh}-{where}-{pattern}", dtype, dh, q, k, v, do, tt, n_visual, pattern)


def dense_cases(dtype, dh, shapes=DENSE_SHAPES, patterns=PATTERNS):
    for n_q, n_kv in shapes:
        for pattern in patterns:
            yield make_case(dtype, dh, n_q, n_kv, pattern)


def media_cases(dtype, dh, keys=MEDIA_KEYS, patterns=MEDIA_PATTERNS):
    for nv, n_media in keys:
        for pattern in patterns:
            yield make_case(dtype, dh, MEDIA_NQ, nv * n_media, pattern, media_text_time(MEDIA_NQ, n_media), nv)


def all_cases(dtype):
    """every input set of tests/test_hip_attention_bounds.py in `dtype` (what tools/attn_c.py measures the constants on)"""
    for dt, dh in DENSE_INST:
        if dt == dtype:
            yield from dense_cases(dt, dh)
    for dt, dh in MEDIA_INST:
        if dt == dtype:
            yield from media_cases(dt, dh)


# ---- the float64 reference and the terms of the bounds ----------------------------------------------------------------------------------
def _bhnd(t):
    return (t.detach().double().cpu().numpy() if torch.is_tensor(t) else np.asarray(t, np.float64)).transpose(0, 2, 1, 3)


def attention_ref(q, k, v, do=None, tt=None, n_visual=0, e_do=None):
    """Everything util.attn_bound_ok needs, in float64 from the tensors as stored ((b, n, h, d); tt (b, n_q) or None = dense), with the
    allowed key set of each row from oracle.attention_masks.  A dict of float64 numpy arrays:
      lse (b, h, n_q), o (b, n_q, h, d) and, with dO, dq, dk, dv; per output x: t_x (the terms one float32 rounding is proportional to),
      pu_x (what the bf16 rounding of P / dS scales), ut_x (dq, dk: what the rounding of the stored O scales through D), fl_x (what a
      probability below 2^-126, lost by the device's exp, scales); kinds (b, n_q): 0 zero row, 1 softmax row, 2 uniform row; p (b, h, n_q,
      n_kv) and s, for the case table's own tests.  A zero row: p = 0, o = 0, lse = 1e30 (the kernel's sentinel), no gradient; a uniform
      row: all scores 0 over all keys, no gradient to the scores.
      With e_do (the fused block kernels, which form dO themselves and never store it: tests/xattn_cases.py) also e_dv, e_dq, e_dk, the
      fixed terms util.attn_bound_ok adds when asked (extra=True)."""
    Q, K, V = _bhnd(q), _bhnd(k), _bhnd(v)
    b, h, n_q, dh = Q.shape
    n_kv = K.shape[2]
    if tt is None:
        seen = np.ones((b, 1, n_q, n_kv), bool)
        zero = uni = np.zeros((b, 1, n_q, 1), bool)
    else:
        allow, zero = O.attention_masks(np.asarray(tt), n_kv // n_visual, n_visual)
        uni = ~allow.any(-1, keepdims=True) & ~zero
        seen = (allow | uni) & ~zero
    soft = seen & ~uni
    s = np.where(uni, 0.0, Q @ K.transpose(0, 1, 3, 2))
    a = np.where(uni, 0.0, np.abs(Q) @ np.abs(K).transpose(0, 1, 3, 2))
    with np.errstate(all="ignore"):
        sm = np.where(seen, s, -np.inf)
        mx = np.where(zero, 0.0, sm.max(-1, keepdims=True))
        lse = mx + np.log(np.where(zero, 1.0, np.exp(sm - mx).sum(-1, keepdims=True)))
        p = np.where(seen, np.exp(sm - lse), 0.0)
    w = p * (1.0 + a + np.where(seen, np.abs(s - lse), 0.0))
    o = p @ V
    back = lambda x: x.transpose(0, 2, 1, 3)
    kinds = np.where(zero, 0, np.where(uni, 2, 1))[:, 0, :, 0]
    out = dict(p=p, s=s, kinds=kinds, seen=np.broadcast_to(seen, p.shape),
               lse=np.where(zero, float(POS_BIG), lse)[..., 0], t_lse=np.where(zero, 0.0, 1.0 + np.abs(lse) + (p * a).sum(-1, keepdims=True))[..., 0],
               o=back(o), t_o=back(w @ np.abs(V) + np.abs(o) * w.sum(-1, keepdims=True)), pu_o=back(p @ np.abs(V)),
               fl_o=back(np.broadcast_to(seen, p.shape).astype(np.float64) @ np.abs(V)))
    if do is None:
        return out
    dO = _bhnd(do)
    VT = V.transpose(0, 1, 3, 2)
    dp, bb = dO @ VT, np.abs(dO) @ np.abs(VT)
    D, Dabs = (dO * o).sum(-1, keepdims=True), np.abs(dO * o).sum(-1, keepdims=True)
    ds = np.where(soft, p * (dp - D), 0.0)
    g = np.where(soft, p * (np.abs(dp) + np.abs(D)) * (1.0 + a + np.abs(np.where(seen, s - lse, 0.0))) + p * (bb + Dabs), 0.0)
    fl = np.where(soft, 1.0 + np.abs(dp) + np.abs(D), 0.0)
    ps = np.where(soft, p, 0.0)
    T = lambda x: x.transpose(0, 1, 3, 2)
    seen_f = np.broadcast_to(seen, p.shape).astype(np.float64)
    out.update(dv=back(T(p) @ dO), t_dv=back(T(w) @ np.abs(dO)), pu_dv=back(T(p) @ np.abs(dO)), fl_dv=back(T(seen_f) @ np.abs(dO)),
               dq=back(ds @ K), t_dq=back(g @ np.abs(K)), pu_dq=back(np.abs(ds) @ np.abs(K)), ut_dq=back(Dabs * (ps @ np.abs(K))),
               fl_dq=back(fl @ np.abs(K)),
               dk=back(T(ds) @ Q), t_dk=back(T(g) @ np.abs(Q)), pu_dk=back(T(np.abs(ds)) @ np.abs(Q)), ut_dk=back(T(Dabs * ps) @ np.abs(Q)),
               fl_dk=back(T(fl) @ np.abs(Q)))
    if e_do is not None:      # dO is itself a result with the element-wise error bound e_do (b, n_q, h, d): what that adds, to first order
        E = _bhnd(e_do)
        hh = np.where(soft, E @ np.abs(VT) + (E * np.abs(o)).sum(-1, keepdims=True), 0.0)      # h_ij = sum_d e_id (|v_jd| + |o_id|): dp_ij - D_i
        out.update(e_dv=back(T(p) @ E), e_dq=back((ps * hh) @ np.abs(K)), e_dk=back(T(ps * hh) @ np.abs(Q)))
    return out


# ---- the kernels restated ---------------------------------------------------------------------------------------------------------------
def _f32(t):
    return np.ascontiguousarray(t.detach().float().cpu().numpy().transpose(0, 2, 1, 3))


def _round(a, dtype):
    """float32 array rounded to `dtype`, as float32"""
    return a if dtype == F32 else torch.from_numpy(np.ascontiguousarray(a)).to(dtype).float().numpy()


def _store(a, dtype):
    return torch.from_numpy(np.ascontiguousarray(a.transpose(0, 2, 1, 3))).to(dtype)


def _exp(x):
    """the device's __expf: float32, results below 2^-126 are returned as 0"""
    e = np.exp(x.astype(np.float32))
    return np.where(e < TINY, np.float32(0), e).astype(np.float32)


def _tile(X, r0):
    """rows r0 .. r0 + 63 of (h, n, d), zero filled past n"""
    t = np.zeros((X.shape[0], TILE, X.shape[2]), np.float32)
    n = max(0, min(TILE, X.shape[1] - r0))
    t[:, :n] = X[:, r0:r0 + n]
    return t


def _block_range(lo, hi):
    ne = hi > lo
    return (int(lo[ne].min()), int(hi[ne].max())) if ne.any() else (0x7FFFFFFF, 0)


def _ranges(case_tt, n_q, n_kv, n_visual, mutate):
    lo, hi, sm, un = row_ranges(case_tt, n_q, n_kv, n_visual)
    if mutate == "range-shift":                     # the image's keys taken one key late
        lo, hi = np.where(sm == 1, lo + 1, lo), np.where(sm == 1, hi + 1, hi)
    if mutate == "drop-last-key":                   # the last key of the last image (the ragged end of the key tile) is never seen
        hi = np.where((sm == 1) & (hi == n_kv), hi - 1, hi)
    if mutate == "uniform-as-image":                # a text_time past the last image is taken for the first image
        lo, hi, sm, un = np.where(un == 1, 0, lo), np.where(un == 1, n_visual, hi), np.where(un == 1, 1, sm), 0 * un
    return lo, hi, sm, un


def attn_fwd_f32(q, k, v, tt=None, n_visual=0, mutate=None, at=(0, 0, 0), tile=0, bm=TILE, keep_f32=False):
    """attn_fwd_kernel + attn_fwd_loop: per workgroup of 64 queries the key tiles [blo, bhi) of block_range, per tile S^T = K Q^T, the
    masked scores at -1e30, the group maximum, alpha = exp(m - m_new), p = exp(s - m_new) (0 where masked), each lane's partial lsum
    (its 16 of the tile's 64 keys) rescaled and summed over the four lanes at the end, acc * alpha + P V with P rounded to bf16 in bf16,
    o = acc * (1 / lsum) rounded to storage, lse = m + log(lsum), 1e30 where lsum = 0.  Returns (o (b, n_q, h, d) in q's dtype, lse
    (b, h, n_q) float32).  `mutate` with at = (sample, head, query) and `tile` (index of a 64-key tile): skip-tile (that row does not see
    that tile), no-rescale (acc is not multiplied by alpha), lse-log2 (that row's lse + log 2), range-shift (every image's range one key
    late), zero-1e-30 (the first zero row of sample `at[0]` holds 1e-30), drop-last-key, uniform-as-image (_ranges).  `bm`: queries per
    workgroup (the fused kernels of csrc/ff_xattn_fused.hip run 32 or 64); keep_f32: o is returned as accumulated, not rounded to storage."""
    dtype, f = q.dtype, np.float32
    Q, K, V = _f32(q), _f32(k), _f32(v)
    b, h, n_q, dh = Q.shape
    n_kv = K.shape[2]
    lo, hi, sm, un = _ranges(tt, n_q, n_kv, n_visual, mutate)
    o, lse = np.zeros_like(Q), np.zeros((b, h, n_q), np.float32)
    with np.errstate(all="ignore"):
        for s in range(b):
            for q0 in range(0, n_q, bm):
                rows = slice(q0, min(q0 + bm, n_q))
                l, u, uni = lo[s, rows, None], hi[s, rows, None], un[s, rows, None] == 1
                blo, bhi = _block_range(l, u)
                R = l.shape[0]
                m, lsum, acc = np.full((h, R), NEG_BIG, f), np.zeros((h, R, 4), f), np.zeros((h, R, dh), f)
                for k0 in range(blo // TILE * TILE, bhi, TILE):
                    kt, vt = _tile(K[s], k0), _tile(V[s], k0)
                    z = Q[s, :, rows] @ kt.transpose(0, 2, 1)
                    key = k0 + np.arange(TILE)[None, :]
                    z = np.where((key >= l) & (key < u), np.where(uni, f(0), z), NEG_BIG).astype(f)
                    if mutate == "skip-tile" and s == at[0] and k0 == tile * TILE and q0 <= at[2] < q0 + bm:
                        z[at[1], at[2] - q0] = NEG_BIG
                    m_new = np.maximum(m, z.max(-1))
                    alpha = _exp(m - m_new)
                    p = np.where(z > f(0.5) * NEG_BIG, _exp(z - m_new[..., None]), f(0)).astype(f)
                    lsum = lsum * alpha[..., None] + p.reshape(h, R, 4, 4, 4).sum(axis=(2, 4), dtype=f)     # key = sub * 16 + lane * 4 + r
                    m = m_new
                    if mutate != "no-rescale":
                        acc = acc * alpha[..., None]
                    acc = acc + _round(p, dtype) @ vt
                ls = (lsum[..., 0] + lsum[..., 1]) + (lsum[..., 2] + lsum[..., 3])
                inv = np.where(ls > 0, f(1) / ls, f(0)).astype(f)
                o[s, :, rows] = acc * inv[..., None]
                lse[s, :, rows] = np.where(ls > 0, m + np.log(ls), POS_BIG)
    assert o.dtype == np.float32 and lse.dtype == np.float32
    if mutate == "lse-log2":
        lse[at] += np.float32(np.log(2.0))
    if mutate == "zero-1e-30":
        o[at[0], :, int(np.nonzero((hi - lo)[at[0]] == 0)[0][0])] = np.float32(1e-30)
    return _store(o, F32 if keep_f32 else dtype), torch.from_numpy(lse)


def attn_bwd_f32(q, k, v, o, do, lse, tt=None, n_visual=0, mutate=None, at=(0, 0, 0), tile=0, bm=TILE, D=None):
    """attn_bwd_dq_kernel and attn_bwd_dkv_kernel: D = rowsum(dO . O) from the STORED o; p = exp(s - L) with the stored lse (0 outside the
    row's range); dS = p (dP - D), 0 for zero and uniform rows; dQ += dS K over the key tiles of block_range (zero and uniform rows have an
    empty range there); per 64 keys, over all 64-query tiles, dV += P^T dO and dK += dS^T Q, P and dS rounded to bf16 in bf16.  Returns
    (dq, dk, dv) in q's dtype.  `mutate`: D-zero (D of query `at` is 0), dk-miss-qtile (dK skips query tile `tile`), uniform-dq (uniform
    rows are treated as softmax rows by the dQ kernel), range-shift, drop-last-key, uniform-as-image.  `bm`: queries per workgroup of the
    dQ pass; D (b, h, n_q) float32: taken in place of rowsum(dO . O)."""
    dtype, f = q.dtype, np.float32
    Q, K, V, Om, dO = _f32(q), _f32(k), _f32(v), _f32(o), _f32(do)
    L = lse.detach().float().cpu().numpy()
    b, h, n_q, dh = Q.shape
    n_kv = K.shape[2]
    lo, hi, sm, un = _ranges(tt, n_q, n_kv, n_visual, mutate)
    D = (dO * Om).sum(-1, dtype=f) if D is None else np.ascontiguousarray(D, f)
    if mutate == "D-zero":
        D[at] = 0
    dq, dk, dv = np.zeros_like(Q), np.zeros_like(K), np.zeros_like(V)
    with np.errstate(all="ignore"):
        for s in range(b):
            keep = (sm[s] == 1) | ((un[s] == 1) if mutate == "uniform-dq" else False)
            lq, uq = np.where(keep, lo[s], 0), np.where(keep, hi[s], 0)
            for q0 in range(0, n_q, bm):
                rows = slice(q0, min(q0 + bm, n_q))
                l, u = lq[rows, None], uq[rows, None]
                blo, bhi = _block_range(l, u)
                acc = np.zeros((h, l.shape[0], dh), f)
                for k0 in range(blo // TILE * TILE, bhi, TILE):
                    kt, vt = _tile(K[s], k0), _tile(V[s], k0)
                    z, dp = Q[s, :, rows] @ kt.transpose(0, 2, 1), dO[s, :, rows] @ vt.transpose(0, 2, 1)
                    key = k0 + np.arange(TILE)[None, :]
                    p = np.where((key >= l) & (key < u), _exp(z - L[s, :, rows, None]), f(0)).astype(f)
                    acc = acc + _round(p * (dp - D[s, :, rows, None]), dtype) @ kt
                dq[s, :, rows] = acc
            for k0 in range(0, n_kv, TILE):
                keys = slice(k0, min(k0 + TILE, n_kv))
                key = np.arange(k0, min(k0 + TILE, n_kv))[None, :]
                acc_k, acc_v = np.zeros((h, key.shape[1], dh), f), np.zeros((h, key.shape[1], dh), f)
                for q0 in range(0, n_q, TILE):
                    rows = slice(q0, min(q0 + TILE, n_q))
                    Qt, dOt = Q[s, :, rows], dO[s, :, rows]
                    z, dp = Qt @ K[s, :, keys].transpose(0, 2, 1), dOt @ V[s, :, keys].transpose(0, 2, 1)
                    ok = (key >= lo[s, rows, None]) & (key < hi[s, rows, None])
                    sc = np.where(un[s, rows, None] == 1, f(0), z).astype(f)
                    p = np.where(ok, _exp(sc - L[s, :, rows, None]), f(0)).astype(f)
                    ds = np.where(sm[s, rows, None] == 1, p * (dp - D[s, :, rows, None]), f(0)).astype(f)
                    acc_v = acc_v + _round(p, dtype).transpose(0, 2, 1) @ dOt
                    if not (mutate == "dk-miss-qtile" and q0 == tile * TILE):
                        acc_k = acc_k + _round(ds, dtype).transpose(0, 2, 1) @ Qt
                dk[s, :, keys], dv[s, :, keys] = acc_k, acc_v
    assert dq.dtype == dk.dtype == dv.dtype == np.float32
    return _store(dq, dtype), _store(dk, dtype), _store(dv, dtype)
