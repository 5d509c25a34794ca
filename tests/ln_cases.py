"""Inputs of the per-element LayerNorm tests (a helper module, not a conftest): the designed rows and case tables shared by
tests/test_hip_layernorm_bounds.py (the kernels), tests/test_ln_cases.py (the checkers, on the CPU) and tools/ln_c.py (the checkers'
constants); the float64 reference with the terms of util.ln_bound_ok; and restatements in float32 numpy, in the kernels' operation
order, of the five LayerNorm implementations - what the constants are measured with and what the CPU tests inject defects into:
  ln_fwd_f32 / ln_bwd_f32   csrc/ff_rowwise.hip: one wave per row, two passes (the register path and the re-reading path of ln_fwd_kernel
                            add in the same order, so one restatement stands for both); ln_bwd_fused_kernel with its rows-per-block
                            serial sums and ln_final_body; ln_bwd_dx_kernel with col_reduce_kernel's row split and col_reduce_final_kernel
  onepass_f32               the shifted one-pass sums of the general fused kernel (4 or 8 threads per row, shift = mean of the first 4 fp32
                            / 8 bf16 elements), of the resident kernel and of the decode feed-forward kernel (16 threads per row, eight
                            accumulators, shift = mean of the first 16 elements), with each kernel's normalising step
  chan_f32                  phase 3 of the resident kernel: two passes per head slice, the eight (mean, M2) pairs combined
  rows_reduce_f32, gate_grad_f32   col_reduce_kernel MODE 0 and dot_partial_kernel + gate_grad_final_kernel
A test tensor takes family r mod F for row r: every wave and workgroup holds a mix of families, and swapped rows show."""
import zlib

import numpy as np
import torch

BF16, F32 = torch.bfloat16, torch.float32
EPS = float(np.float32(1e-5))                    # what the kernels receive as `float eps`
U = 2.0 ** -24
VEC = {F32: 4, BF16: 8}                          # elements per 16-byte piece
f32 = np.float32
FAMILIES = ["plain", "offset+", "offset-", "massive-head", "massive-head-", "massive-body", "massive-tail", "head-off", "const", "zero",
            "tiny-var", "big", "small"]
F = len(FAMILIES)
QUIET = ("massive-body", "massive-tail", "const", "zero", "small")      # families whose condition is <= 2 under every shift (test_ln_cases)

# ---- the case tables ----------------------------------------------------------------------------------------------------------------------
# Part A, the C ABI: rows 1 / 5 / 1025 / 2049 give the fused backward 4 / 8 / 12 rows per block and a partial last block; columns 36 (bf16:
# the element-wise VEC = 1 path; fp32 still has whole 16-byte pieces there, so 35 is added for it), 256, 1024 | 1536, 2048 (fp32: register
# path | re-reading path, bf16: 2048 | 4096), 4096 (bf16: the fused backward at NCH 8, fp32: ln_bwd_dx + column reduce).  NCH of the fused
# backward: bf16 256, 1024 -> 2; 1536, 2048 -> 4; 4096 -> 8;  fp32 256 -> 2; 1024 -> 4; 1536, 2048 -> 8.
ABI_SHAPES = [(1, 36), (5, 35), (5, 36), (2049, 36), (1, 256), (5, 256), (1025, 256), (5, 1024), (2049, 1024), (5, 1536), (1025, 1536),
              (5, 2048), (1025, 2048), (1, 4096), (5, 4096), (1025, 4096)]
ABI_VARIANT_SHAPES = [(5, 36), (1025, 256), (1025, 1536), (1025, 4096)]
REDUCE_CASES = [(26, 36, 13, 13), (2049 * 2, 256, 2049, 2049), (1040, 1536, 104, 13), (1025, 4096, 1025, 1025)]      # rows, cols, per batch, per group
GATE_CASES = [(5, 36), (1025, 256), (2049, 1536)]
# Part B, the block kernels: (name, dtype, heads, dim_head, b, L, n_visual, dim, sync, tile, ring, P, ffw)
#   tile: the code ff_gemm_profile_record.tile of the fused forward launch (-4 alone, -6 with to_out, -8 with to_out and LN(y1)); ring: that
#   record's b_layout, the resident kernel's ring depth, 0 = the general kernel; P: elements of the one-pass shift of LN(y) (4 fp32 / 8 bf16
#   general kernel, 16 resident kernel); ffw: what normalises y1 - "decode" (one pass, P = 16), "phase3" (per-head two-pass inside the launch)
#   or "separate" (ff_layernorm_fwd behind the block's to_out product).
#   general-f32-widest is dim 1536: the widest model width of the project (the resident kernels' limit too), 48 pieces per thread, twice
#   what a thread keeps in registers, so the re-loading branch of the statistics runs.  The fp32 kernel itself is limited only by the LDS
#   its gamma / beta rows take (beyond 7000 columns), where the block's feed-forward weights alone would be gigabytes.
#   general-f32-bm64-reload: 64-row tiles (4 threads per row) at dim 512, 32 pieces per thread: the re-loading branch at TPR = 4 as well.
#   resident-L32-40keys: a full 32-row tile over fewer than 64 keys; text_time is all ones (the attention's row kinds do not enter the
#   LayerNorm statistics; tests/test_hip_modules.py has them at this shape).
#   Every fp32 case has the separate ff_layernorm_fwd behind the block (phase 3 and the decode kernel are bf16 only).
BLOCK_CASES = [
    ("general-f32-multitile", F32, 4, 16, 2, 70, 8, 128, False, -4, 0, 4, "separate"),
    ("general-f32-bm64", F32, 4, 32, 3, 40, 8, 256, False, -4, 0, 4, "separate"),
    ("general-bf16", BF16, 2, 128, 2, 24, 8, 512, False, -4, 0, 8, "separate"),
    ("general-f32-widest", F32, 4, 16, 2, 20, 8, 1536, False, -4, 0, 4, "separate"),
    ("general-f32-bm64-reload", F32, 4, 32, 2, 40, 8, 512, False, -4, 0, 4, "separate"),
    ("resident-ring6", BF16, 8, 64, 3, 20, 64, 1280, False, -4, 6, 16, "separate"),
    ("resident-ring4", BF16, 8, 64, 5, 7, 64, 1536, False, -4, 4, 16, "separate"),
    ("resident-L32-40keys", BF16, 8, 64, 2, 32, 40, 768, False, -4, 6, 16, "separate"),
    ("phase3-dim256", BF16, 8, 64, 3, 20, 64, 256, True, -8, 4, 16, "phase3"),
    ("phase3-dim1280", BF16, 8, 64, 3, 20, 64, 1280, True, -8, 6, 16, "phase3"),
    ("phase3-dim1280-L1", BF16, 8, 64, 39, 1, 64, 1280, True, -8, 6, 16, "phase3"),
    ("decode-dim128", BF16, 8, 64, 2, 14, 64, 128, True, -4, 0, 8, "decode"),
    ("decode-dim384", BF16, 8, 64, 2, 16, 64, 384, True, -4, 6, 16, "decode"),
    ("decode-dim1280", BF16, 8, 64, 13, 1, 64, 1280, True, -4, 6, 16, "decode"),
    ("separate-ln-dim1536", BF16, 8, 64, 3, 20, 64, 1536, True, -4, 4, 16, "separate"),
]
BLOCK_FF_MULT, BLOCK_DIM_VISUAL = 2, 32
# History, not a configuration: the fp32 general kernel took its variance from the one-pass sums until this suite measured the result
# (util.py: the LayerNorm block); it now takes a second pass, and the library has no switch back.  The flag names which restatement stands
# for the kernel; the one-pass fp32 kinds of onepass_f32 (general4, general4-bm32) are kept only so that tests/test_ln_cases.py can show
# the old form missing the fp32 ceiling and inject defects into one-pass sums in fp32.
GENERAL_F32_TWO_PASS = True


def name_of(dtype):
    return "bf16" if dtype == BF16 else "f32"


def _rng(*key):
    return np.random.default_rng(zlib.crc32(repr(key).encode()))


def to_dtype(a, dtype):
    """float array -> CPU tensor of `dtype`"""
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(dtype)


def stored(t):
    """what a tensor holds, as float64 numpy"""
    return t.detach().double().cpu().numpy()


def family_of(r):
    return FAMILIES[r % F]


def designed_rows(rows, cols, dtype, key=()):
    """(rows, cols) CPU tensor in `dtype`; row r is of family r mod F.  z ~ N(0, 1) per element.
    plain z; offset+- z +- 100 (bf16) / 1000 (fp32); massive-head 2000 in column 0; massive-head- -2000 in the last column of the first
    16-byte piece; massive-body 2000 in column 17; massive-tail 2000 in the last column; head-off the first 16 columns raised by 50; const
    3.25 everywhere; zero; tiny-var 1 + 0.004 z (variance near eps); big 1e4 z; small 1e-3 z."""
    z = _rng("rows", name_of(dtype), rows, cols, *key).standard_normal((rows, cols))
    off = 100.0 if dtype == BF16 else 1000.0
    x = np.empty_like(z)
    for r in range(rows):
        fam, v = family_of(r), z[r].copy()
        if fam == "offset+":
            v += off
        elif fam == "offset-":
            v -= off
        elif fam == "massive-head":
            v[0] = 2000.0
        elif fam == "massive-head-":
            v[min(VEC[dtype], cols) - 1] = -2000.0
        elif fam == "massive-body":
            v[min(17, cols - 1)] = 2000.0
        elif fam == "massive-tail":
            v[-1] = 2000.0
        elif fam == "head-off":
            v[:16] += 50.0
        elif fam == "const":
            v[:] = 3.25
        elif fam == "zero":
            v[:] = 0.0
        elif fam == "tiny-var":
            v = 1.0 + 0.004 * v
        elif fam == "big":
            v *= 1e4
        elif fam == "small":
            v *= 1e-3
        x[r] = v
    return to_dtype(x, dtype)


def operands(rows, cols, dtype, key=()):
    """gamma = 1 + 0.2 z with one entry exactly 0 and one negative, beta = 0.1 z, dy = z with every seventh row all zero, a residual z"""
    g = _rng("operands", name_of(dtype), rows, cols, *key)
    gamma, beta = 1.0 + 0.2 * g.standard_normal(cols), 0.1 * g.standard_normal(cols)
    gamma[cols // 3], gamma[(2 * cols) // 3] = 0.0, -0.75
    dy, res = g.standard_normal((rows, cols)), g.standard_normal((rows, cols))
    dy[::7] = 0.0
    return tuple(to_dtype(a, dtype) for a in (gamma, beta, dy, res))


def seen(x, add=None, add_rows_per_seg=0, add_div=1):
    """what the kernels normalise, as a float32 tensor: x, or fl32(x + add[(row % add_rows_per_seg) / add_div]) - ONE float32 addition,
    the same on every machine"""
    v = x.float()
    if add is not None:
        idx = (torch.arange(x.shape[0]) % add_rows_per_seg) // add_div
        v = v + add.float()[idx]
    return v


# ---- the float64 reference and the terms of the bounds ------------------------------------------------------------------------------------
def ln_ref(x, gamma=None, beta=None, dy=None, P=0, eps=EPS, stats=None, residual=None, P_var=None):
    """Everything util.ln_bound_ok needs, in float64 from the tensors as stored.  x (rows, cols): what the kernel normalises (ln_cases.seen);
    P: elements of the kernel's one-pass shift (4, 8, 16), 0 = a two-pass kernel (P_var: the same for the variance alone, where a kernel takes
    the mean from shifted sums and the variance by a second pass; default P); stats = (mean, rstd) as the kernel STORED them (None: the
    exact ones): y, dx, dgamma, dbeta are computed from those, so the normalising step is judged apart from the statistics.
    A dict of float64 numpy arrays: mean, var, rstd, s (the shift: mean of the first P elements; = mean for P = 0), kappa = (var + 2 (mean -
    s)^2) / (var + eps), t_mean = |s0| + mean_c |x_c - s0| with s0 = s (P > 0) or 0; and, as far as the operands are given,
      y = (x - mean) rstd g + b,             t_y = |x - mean| rstd |g| + |b|,  t_y_dec = |mean rstd| |g| (the decode kernel's x rs - mean rs)
      dx = rstd (dy g - mean(dy g) - xh mean(dy g xh)) [+ residual],   t_dx = rstd (|dy g| + mean|dy g| + |xh| mean|dy g xh|),  xh = (x - mean) rstd
      dgamma = sum_r dy xh, t_dgamma = sum_r |dy xh|;  dbeta = sum_r dy, t_dbeta = sum_r |dy|;  residual (or None)."""
    X = stored(x) if torch.is_tensor(x) else np.asarray(x, np.float64)
    mean = X.mean(-1)
    var = ((X - mean[:, None]) ** 2).mean(-1)
    rstd = 1.0 / np.sqrt(var + eps)
    s = X[:, :P].mean(-1) if P else mean
    s0 = s if P else np.zeros_like(mean)
    P_var = P if P_var is None else P_var
    sv = X[:, :P_var].mean(-1) if P_var else mean
    out = dict(mean=mean, var=var, rstd=rstd, s=s, kappa=(var + 2.0 * (mean - sv) ** 2) / (var + eps),
               t_mean=np.abs(s0) + np.abs(X - s0[:, None]).mean(-1), residual=None)
    mk, rk = (mean, rstd) if stats is None else (np.asarray(stored(a) if torch.is_tensor(a) else a, np.float64).reshape(-1) for a in stats)
    xh = (X - mk[:, None]) * rk[:, None]
    if gamma is not None:
        g = stored(gamma)
        if beta is not None:
            b = stored(beta)
            out.update(y=xh * g + b, t_y=np.abs(xh) * np.abs(g) + np.abs(b), t_y_dec=np.abs(mk * rk)[:, None] * np.abs(g)[None, :])
        if dy is not None:
            D = stored(dy)
            dyh = D * g
            m1, m2 = dyh.mean(-1, keepdims=True), (dyh * xh).mean(-1, keepdims=True)
            dx = rk[:, None] * (dyh - m1 - xh * m2)
            t_dx = rk[:, None] * (np.abs(dyh) + np.abs(dyh).mean(-1, keepdims=True) + np.abs(xh) * np.abs(dyh * xh).mean(-1, keepdims=True))
            if residual is not None:
                out["residual"] = stored(residual)
                dx = dx + out["residual"]
            out.update(dx=dx, t_dx=t_dx, dgamma=(D * xh).sum(0), t_dgamma=np.abs(D * xh).sum(0), dbeta=D.sum(0), t_dbeta=np.abs(D).sum(0))
    return out


def rows_reduce_ref(x, rows_per_batch, rows_per_group):
    """out[g][c] = sum over the batches of the rows of group g; (value, sum of |x|) in float64"""
    X = stored(x)
    rows, cols = X.shape
    X = X.reshape(rows // rows_per_batch, rows_per_batch // rows_per_group, rows_per_group, cols)
    return dict(rows_reduce=X.sum(axis=(0, 2)), t_rows_reduce=np.abs(X).sum(axis=(0, 2)))


def gate_grad_ref(a, b, alpha):
    A, B = stored(a), stored(b)
    k = 1.0 - np.tanh(float(stored(alpha).reshape(-1)[0])) ** 2
    return dict(gate_grad=np.array([k * (A * B).sum()]), t_gate_grad=np.array([k * np.abs(A * B).sum()]))


# ---- the kernels restated -----------------------------------------------------------------------------------------------------------------
def _round(a, dtype):
    return np.asarray(a, np.float32) if dtype == F32 else to_dtype(a, dtype).float().numpy()


def _fma(a, b, c):
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)


def _xor_sum(v, first):
    """v (..., n) float32: the xor-shuffle sum over the last axis with offsets first, first / 2, ..., 1 (every lane ends with the same bits)"""
    n, o = v.shape[-1], first
    while o > 0:
        v = v + v[..., np.arange(n) ^ o]
        o >>= 1
    return v[..., 0]


def _vec_of(cols, dtype):
    return VEC[dtype] if cols % VEC[dtype] == 0 else 1


def _lanes(a, vec):
    """(rows, cols) -> ((rows, U, 64, vec) zero padded, (U, 64) mask): lane l of the row's wave owns the pieces l + 64 u"""
    rows, cols = a.shape
    nchunk = cols // vec
    nu = -(-nchunk // 64)
    pad = np.zeros((rows, nu * 64 * vec), np.float32)
    pad[:, :cols] = a
    return pad.reshape(rows, nu, 64, vec), (np.arange(nu * 64) < nchunk).reshape(nu, 64)


def _lane_serial(terms, mask):
    """each lane's serial sum over its pieces and their elements, then wave_sum: (rows,)"""
    s = np.zeros(terms.shape[:1] + (64,), np.float32)
    for u in range(terms.shape[1]):
        for i in range(terms.shape[3]):
            s = s + np.where(mask[u], terms[:, u, :, i], f32(0))
    return _xor_sum(s, 32)


def ln_fwd_f32(v, gamma, beta, dtype, eps=EPS, stats=None, mutate=None):
    """ln_fwd_kernel on v (rows, cols) float32 (ln_cases.seen): (mean, rstd float32 arrays, y as a tensor of `dtype`).
    mutate: n-1 (the variance divided by cols - 1), eps-outside (1 / (sqrt(var) + eps)), swap (mean / rstd of rows 2 k and 2 k + 1
    exchanged before normalising and storing), gamma-xor8 (gamma read from column c ^ 8)."""
    v = np.asarray(v, np.float32)
    rows, cols = v.shape
    vec = _vec_of(cols, dtype)
    n = f32(cols)
    if stats is None:
        V, mask = _lanes(v, vec)
        mu = _lane_serial(V, mask) / n
        d = V - mu[:, None, None, None]
        var = _lane_serial(d * d, mask) / (f32(cols - 1) if mutate == "n-1" else n)
        rs = f32(1) / (np.sqrt(var) + f32(eps)) if mutate == "eps-outside" else f32(1) / np.sqrt(var + f32(eps))
        if mutate == "swap":
            k = np.arange(rows) ^ 1
            k[k >= rows] = rows - 1
            mu, rs = mu[k], rs[k]
    else:
        mu, rs = (np.asarray(a, np.float32) for a in stats)
    g, b = gamma.float().numpy(), beta.float().numpy()
    if mutate == "gamma-xor8":
        g = g[np.minimum(np.arange(cols) ^ 8, cols - 1)]
    y = (v - mu[:, None]) * rs[:, None] * g + b
    assert y.dtype == np.float32 and mu.dtype == np.float32 and rs.dtype == np.float32
    return mu, rs, to_dtype(y, dtype)


def fused_rows_per_block(rows):
    return max(4, (-(-rows // 256) + 3) // 4 * 4)


def fused_backward_taken(rows, cols, dtype, want_params=True):
    vec = _vec_of(cols, dtype)
    return want_params and vec > 1 and -(-(cols // vec) // 64) <= 8 and 8 * cols * 4 <= 150 * 1024


def _final_body(partial):
    """ln_final_body: partial (nblk, n) float32 -> (n,): 16 block-lanes with eight accumulators each, a tree, then 16 serial additions"""
    nblk, n = partial.shape
    red = []
    for ty in range(16):
        v = [np.zeros(n, np.float32) for _ in range(8)]
        b = ty
        while b + 7 * 16 < nblk:
            for u in range(8):
                v[u] = v[u] + partial[b + 16 * u]
            b += 8 * 16
        while b < nblk:
            v[0] = v[0] + partial[b]
            b += 16
        red.append(((v[0] + v[1]) + (v[2] + v[3])) + ((v[4] + v[5]) + (v[6] + v[7])))
    s = np.zeros(n, np.float32)
    for ty in range(16):
        s = s + red[ty]
    return s


def split_plan(n_rows, col_blocks, ngroups=1):
    target = max(1, 512 // max(1, col_blocks * ngroups))
    nsplit = max(1, min(min(target, 32), -(-n_rows // 32)))
    rps = -(-n_rows // nsplit)
    return rps, -(-n_rows // rps)


def _col_reduce(T, vec, ngroups=1):
    """col_reduce_kernel + col_reduce_final_kernel over the rows of ONE group, T (rows, cols) float32: row lane ty adds rows ty, ty + 4, ...
    of its split, the four lanes are added left to right, the splits by four chains (ngroups: how many groups share the launch - it enters
    the split plan only)"""
    rows, cols = T.shape
    rps, nsplit = split_plan(rows, -(-cols // (64 * vec)), ngroups)
    parts = []
    for sp in range(nsplit):
        lane = []
        for ty in range(4):
            acc = np.zeros(cols, np.float32)
            for i in range(sp * rps + ty, min(rows, (sp + 1) * rps), 4):
                acc = acc + T[i]
            lane.append(acc)
        parts.append(((lane[0] + lane[1]) + lane[2]) + lane[3])
    v = [np.zeros(cols, np.float32) for _ in range(4)]
    s = 0
    while s + 4 <= nsplit:
        for k in range(4):
            v[k] = v[k] + parts[s + k]
        s += 4
    while s < nsplit:
        v[0] = v[0] + parts[s]
        s += 1
    return (v[0] + v[1]) + (v[2] + v[3])


def ln_bwd_f32(dy, v, gamma, mean, rstd, dtype, residual=None, want_params=True, mutate=None):
    """ff_layernorm_bwd on v (rows, cols) float32 with the given float32 statistics: (dx, dgamma, dbeta) as tensors of `dtype` (the last two
    None without want_params).  The fused kernel where layernorm_bwd takes it, else ln_bwd_dx_kernel + the column reduce.
    mutate: no-xhat-term (dx without xh mean(dy g xh)), dgamma-miss-block (the second row block left out of dgamma), dbeta-dyg (dbeta summed
    from dy g)."""
    v, mu, rs = np.asarray(v, np.float32), np.asarray(mean, np.float32)[:, None], np.asarray(rstd, np.float32)[:, None]
    rows, cols = v.shape
    vec = _vec_of(cols, dtype)
    d, g = dy.float().numpy(), gamma.float().numpy()
    fused = fused_backward_taken(rows, cols, dtype, want_params)
    dyh, xh = d * g, (v - mu) * rs
    t2 = dyh * xh if fused else dyh * (v - mu) * rs
    D1, mask = _lanes(dyh, vec)
    D2, _ = _lanes(t2, vec)
    s1 = np.zeros((rows, 64), np.float32)
    s2 = np.zeros((rows, 64), np.float32)
    for u in range(D1.shape[1]):
        for i in range(vec):
            s1 = s1 + np.where(mask[u], D1[:, u, :, i], f32(0))
            s2 = s2 + np.where(mask[u], D2[:, u, :, i], f32(0))
    m1, m2 = (_xor_sum(s1, 32) / f32(cols))[:, None], (_xor_sum(s2, 32) / f32(cols))[:, None]
    o = rs * (dyh - m1 - (f32(0) if mutate == "no-xhat-term" else xh * m2))
    if residual is not None:
        o = o + residual.float().numpy()
    assert o.dtype == np.float32
    dx = to_dtype(o, dtype)
    if not want_params:
        return dx, None, None
    tg, tb = (d * xh if fused else d * (v - mu) * rs), (dyh if mutate == "dbeta-dyg" else d)
    if fused:
        rpb = fused_rows_per_block(rows)
        nblk = -(-rows // rpb)

        def blocks(T):
            pad = np.zeros((nblk * rpb, cols), np.float32)
            pad[:rows] = T
            pad = pad.reshape(nblk, rpb // 4, 4, cols)
            acc = np.zeros((nblk, 4, cols), np.float32)
            for k in range(rpb // 4):
                acc = acc + pad[:, k]
            return (acc[:, 0] + acc[:, 1]) + (acc[:, 2] + acc[:, 3])
        pg, pb = blocks(tg), blocks(tb)
        if mutate == "dgamma-miss-block":
            pg[min(1, nblk - 1)] = 0
        dg, db = _final_body(pg), _final_body(pb)
    else:
        if mutate == "dgamma-miss-block":
            tg = tg.copy()
            tg[4:8] = 0
        dg, db = _col_reduce(tg, vec), _col_reduce(tb, vec)
    assert dg.dtype == np.float32 and db.dtype == np.float32
    return dx, to_dtype(dg, dtype), to_dtype(db, dtype)


def rows_reduce_f32(x, rows_per_batch, rows_per_group, dtype):
    """ff_rows_reduce: col_reduce_kernel MODE 0 per group (row i of the group's list = batch i / rows_per_group, row i % rows_per_group)"""
    X = x.float().numpy()
    rows, cols = X.shape
    nb, ng = rows // rows_per_batch, rows_per_batch // rows_per_group
    X = X.reshape(nb, ng, rows_per_group, cols)
    vec = _vec_of(cols, dtype)
    out = np.zeros((ng, cols), np.float32)
    for gi in range(ng):
        out[gi] = _col_reduce(np.ascontiguousarray(X[:, gi]).reshape(nb * rows_per_group, cols), vec, ng)
    return to_dtype(out, dtype)


def gate_grad_f32(a, b, alpha, dtype):
    """dot_partial_kernel (thread t of block k adds the pieces k * 256 + t, + blocks * 256, ...; block_sum) + gate_grad_final_kernel"""
    A, B = a.float().numpy().reshape(-1), b.float().numpy().reshape(-1)
    n = A.size
    vec = _vec_of(a.shape[1], dtype)
    nblk = int(max(1, min(512, n // 4096)))
    nchunk, T = n // vec, nblk * 256
    steps = -(-nchunk // T)
    pad = np.zeros(steps * T * vec, np.float32)
    pad[:nchunk * vec] = (A * B)[:nchunk * vec]
    pad = pad.reshape(steps, nblk, 4, 64, vec)
    s = np.zeros((nblk, 4, 64), np.float32)
    for k in range(steps):
        for i in range(vec):
            s = s + pad[k, :, :, :, i]
    w = _xor_sum(s, 32)
    part = ((w[:, 0] + w[:, 1]) + w[:, 2]) + w[:, 3]
    s = np.zeros(256, np.float32)
    for k in range(-(-nblk // 256)):
        chunk = part[k * 256:(k + 1) * 256]
        s[:chunk.size] = s[:chunk.size] + chunk
    w = _xor_sum(s.reshape(4, 64), 32)
    tot = ((w[0] + w[1]) + w[2]) + w[3]
    t = np.tanh(alpha.float().numpy().reshape(-1)[0]).astype(np.float32)
    return to_dtype(np.array([tot * (f32(1) - t * t)], np.float32), dtype)


ONEPASS = {"general4": (4, 4), "general8": (8, 4), "general4-bm32": (4, 8), "general8-bm32": (8, 8), "resident": (16, 16), "decode": (16, 16),
           "general4-2p": (4, 4), "general4-bm32-2p": (4, 8)}


def onepass_kind(dtype, L, P):
    """the restatement that stands for a Part B case's fused kernel: by the shift's width and the general kernel's row tile (64 rows: 4 threads
    per row, 32 rows: 8)"""
    if P == 16:
        return "resident"
    return f"general{P}" + ("-bm32" if L <= 32 else "") + ("-2p" if dtype == F32 and GENERAL_F32_TWO_PASS else "")


def onepass_f32(x, gamma, beta, kind, eps=EPS, mutate=None):
    """The shifted one-pass statistics and the normalising step of the fused kernels on x (rows, cols) as stored (bf16 or fp32 tensor):
    (mean, rstd float32, y tensor in x's dtype).  kind: general4 / general8 (xa_qattn_fwd_kernel, fp32 / bf16: TPR = 4 threads per row at a
    64-row tile - 8 with the suffix -bm32 -, thread `sub` adds the pieces sub, sub + TPR, ... one element after the other, shift = mean of
    the first piece), resident (xa_qattn_fwd_res_kernel: 16 threads per row, eight accumulators s1[e], s2[e] = fma(d, d, s2[e]), a tree,
    shift = mean of the first 16 elements), decode (ff_decode.hip: as resident with two pieces per step, mean - shift = sum * (1 / n), y =
    fma(fma(x, rs, -mu rs), g, b)).  The suffix -2p: the fp32 general kernel as it is now - the mean from the shifted sum, the variance
    by a second pass around it in the same thread order (without the suffix: the one-pass form it had before, kept for the defect tests).
    mutate: unshifted (E[x^2] - mean^2 around 0), shift-x0 (the shift is the first element), n-1, eps-outside, miss-piece (the second 8
    elements left out of both sums), no-fmax (the variance not clamped at 0); a tuple applies several."""
    mutate = set(mutate) if isinstance(mutate, (tuple, list, set)) else {mutate}
    dtype = x.dtype
    X = x.float().numpy()
    rows, cols = X.shape
    P, tpr = ONEPASS[kind]
    vn = VEC[dtype]
    nchunk = cols // vn
    first = X[:, :P]
    if kind.startswith("general"):
        fs = np.zeros(rows, np.float32)
        for e in range(P):
            fs = fs + first[:, e]
        shift = fs * f32(1.0 / P)
    else:
        hs = np.zeros(rows, np.float32)
        for e in range(8):
            hs = hs + (first[:, e] + first[:, 8 + e])
        shift = hs * f32(1.0 / 16.0)
    if "unshifted" in mutate:
        shift = np.zeros(rows, np.float32)
    elif "shift-x0" in mutate:
        shift = X[:, 0].copy()
    Xc = X.reshape(rows, nchunk, vn).copy()
    keep = np.ones(nchunk * vn, bool)
    if "miss-piece" in mutate:
        keep[8:16] = False
    keep = keep.reshape(nchunk, vn)
    d = Xc - shift[:, None, None]
    if kind.startswith("general"):
        ppt = nchunk // tpr
        s1, s2 = np.zeros((rows, tpr), np.float32), np.zeros((rows, tpr), np.float32)
        for u in range(ppt):
            ch = slice(u * tpr, (u + 1) * tpr)
            for e in range(vn):
                k = keep[ch, e]
                s1 = s1 + np.where(k, d[:, ch, e], f32(0))
                s2 = s2 + np.where(k, d[:, ch, e] * d[:, ch, e], f32(0))
        sum_, sq = _xor_sum(s1, tpr // 2), _xor_sum(s2, tpr // 2)
    else:
        per = -(-nchunk // 16)
        pad = np.zeros((rows, per * 16, vn), np.float32)
        pad[:, :nchunk] = np.where(keep[None], d, f32(0))
        pad = pad.reshape(rows, per, 16, vn)
        s1, s2 = np.zeros((rows, 16, vn), np.float32), np.zeros((rows, 16, vn), np.float32)
        if kind == "resident":
            for u in range(per):
                s1 = s1 + pad[:, u]
                s2 = _fma(pad[:, u], pad[:, u], s2)
        else:
            for u in range(0, per, 2):
                d0, d1 = pad[:, u], (pad[:, u + 1] if u + 1 < per else np.zeros_like(pad[:, u]))
                s1 = s1 + (d0 + d1)
                s2 = _fma(d1, d1, _fma(d0, d0, s2))
        tree = lambda a: ((a[..., 0] + a[..., 1]) + (a[..., 2] + a[..., 3])) + ((a[..., 4] + a[..., 5]) + (a[..., 6] + a[..., 7]))
        sum_, sq = _xor_sum(tree(s1), 8), _xor_sum(tree(s2), 8)
    n = f32(cols)
    nv = f32(cols - 1) if "n-1" in mutate else n
    if kind == "decode":
        inv = f32(1) / n
        dm = sum_ * inv
        var = sq * (f32(1) / nv) - dm * dm
    else:
        dm = sum_ / n
        var = sq / nv - dm * dm
    mu = shift + dm
    if kind.endswith("-2p"):
        dd = Xc - mu[:, None, None]
        q = np.zeros((rows, tpr), np.float32)
        for u in range(ppt):
            ch = slice(u * tpr, (u + 1) * tpr)
            for e in range(vn):
                q = q + np.where(keep[ch, e], dd[:, ch, e] * dd[:, ch, e], f32(0))
        var = _xor_sum(q, tpr // 2) / nv
    if "no-fmax" not in mutate:
        var = np.maximum(var, f32(0))
    with np.errstate(invalid="ignore", divide="ignore"):
        rs = f32(1) / (np.sqrt(var) + f32(eps)) if "eps-outside" in mutate else f32(1) / np.sqrt(var + f32(eps))
    g, b = gamma.float().numpy(), beta.float().numpy()
    if kind == "decode":
        nmr = -mu * rs
        y = _fma(_fma(X, np.broadcast_to(rs[:, None], X.shape), np.broadcast_to(nmr[:, None], X.shape)), np.broadcast_to(g, X.shape),
                 np.broadcast_to(b, X.shape))
    else:
        y = (X - mu[:, None]) * rs[:, None] * g + b
    assert mu.dtype == np.float32 and rs.dtype == np.float32 and y.dtype == np.float32
    return mu, rs, to_dtype(y, dtype)


def chan_f32(y1, gamma, beta, heads=8, eps=EPS, mutate=None):
    """Phase 3 of the resident kernel on y1 (rows, dim) bf16 as stored: per head slice of cs = dim / heads columns the sum of every 8-element
    item, the slice mean, M2 by a second pass (fma per element inside an item, the items added serially), and the heads' pairs combined as
    equal-sized groups (Chan et al.): mean = avg(mean_h), M2 = sum(M2_h + cs (mean_h - mean)^2).  mutate: miss-head (head 5's pair left
    out of the combine).  Returns (mean, rstd, xn)."""
    X = y1.float().numpy()
    rows, dim = X.shape
    cs = dim // heads
    cpr = cs // 8
    it = X.reshape(rows, heads, cpr, 8)
    sx = np.zeros((rows, heads, cpr), np.float32)
    for e in range(8):
        sx = sx + it[..., e]
    pa = np.zeros((rows, heads), np.float32)
    for q in range(cpr):
        pa = pa + sx[:, :, q]
    mw = pa / f32(cs)
    m2i = np.zeros((rows, heads, cpr), np.float32)
    for e in range(8):
        dlt = it[..., e] - mw[:, :, None]
        m2i = _fma(dlt, dlt, m2i)
    pb = np.zeros((rows, heads), np.float32)
    for q in range(cpr):
        pb = pb + m2i[:, :, q]
    use = [h for h in range(heads) if not (mutate == "miss-head" and h == 5)]
    mean = np.zeros(rows, np.float32)
    for h in use:
        mean = mean + mw[:, h]
    mean = mean / f32(heads)
    m2 = np.zeros(rows, np.float32)
    for h in use:
        dm = mw[:, h] - mean
        m2 = m2 + (pb[:, h] + f32(cs) * dm * dm)
    rs = f32(1) / np.sqrt(m2 / f32(dim) + f32(eps))
    y = (X - mean[:, None]) * rs[:, None] * gamma.float().numpy() + beta.float().numpy()
    assert mean.dtype == np.float32 and rs.dtype == np.float32 and y.dtype == np.float32
    return mean, rs, to_dtype(y, BF16)


# ---- the inputs of the GPU tests, by case ---------------------------------------------------------------------------------------------
class AbiCase:
    """Part A: x (rows, cols) designed rows, gamma, beta, dy, residual; with `add` a (3, cols) addend read as add[(row % 6) // 2]"""

    def __init__(self, dtype, rows, cols, add=False):
        self.name, self.dtype, self.rows, self.cols = f"{name_of(dtype)}-{rows}x{cols}" + ("-add" if add else ""), dtype, rows, cols
        self.x = designed_rows(rows, cols, dtype)
        self.gamma, self.beta, self.dy, self.res = operands(rows, cols, dtype)
        self.add, self.add_rows_per_seg, self.add_div = None, 0, 1
        if add:
            self.add = to_dtype(0.5 * _rng("add", name_of(dtype), cols).standard_normal((3, cols)), dtype)
            self.add_rows_per_seg, self.add_div = 6, 2
        self.v = seen(self.x, self.add, self.add_rows_per_seg, self.add_div)


def abi_cases(dtype):
    for rows, cols in ABI_SHAPES:
        yield AbiCase(dtype, rows, cols)
    for rows, cols in ABI_VARIANT_SHAPES:
        yield AbiCase(dtype, rows, cols, add=True)


def reduce_input(dtype, rows, cols):
    return designed_rows(rows, cols, dtype, key=("reduce",))


def gate_inputs(dtype, rows, cols):
    a = designed_rows(rows, cols, dtype, key=("gate-a",))
    b = to_dtype(_rng("gate-b", name_of(dtype), rows, cols).standard_normal((rows, cols)), dtype)
    return a, b, to_dtype(np.array([0.55]), dtype)


class BlockCase:
    """Part B: y (b, L, dim) designed rows (row r = sample * L + token), the block's eleven parameters in the order of
    include/flamingo_fusion.h (alpha_attn = 0 or 0.55), visual features and text_time (every token on the one image)."""

    def __init__(self, row):
        (self.name, self.dtype, self.heads, self.dh, self.b, self.L, self.nv, self.dim, self.sync, self.tile, self.ring, self.P, self.ffw) = row
        self.rows, self.inner, self.ffi, self.dv = self.b * self.L, self.heads * self.dh, BLOCK_FF_MULT * self.dim, BLOCK_DIM_VISUAL
        self.kind = onepass_kind(self.dtype, self.L, self.P)
        self.P_var = 0 if self.dtype == F32 and GENERAL_F32_TWO_PASS else self.P
        dt, d = self.dtype, self.dim
        self.y = designed_rows(self.rows, d, dt, key=("block",)).reshape(self.b, self.L, d)
        g = _rng("block", self.name)
        self.gamma_a, self.beta_a, _, _ = operands(1, d, dt, key=("norm-a",))
        self.gamma_f, self.beta_f, _, _ = operands(1, d, dt, key=("norm-f",))
        w = lambda o, i: to_dtype(g.standard_normal((o, i)) * i ** -0.5, dt)
        self.weights = dict(to_q=w(self.inner, d), to_kv=w(2 * self.inner, self.dv), to_out=w(d, self.inner), ffw1=w(self.ffi, d), ffw3=w(d, self.ffi))
        self.vf = to_dtype(g.standard_normal((self.b, 1, self.nv, self.dv)), dt)
        self.tt = np.ones((self.b, self.L), np.int32)

    def params(self, alpha_attn):
        a = lambda v: to_dtype(np.array([v]), self.dtype)
        W = self.weights
        return [a(alpha_attn), a(0.4), self.gamma_a, self.beta_a, W["to_q"], W["to_kv"], W["to_out"], self.gamma_f, self.beta_f, W["ffw1"], W["ffw3"]]


def block_cases():
    return [BlockCase(row) for row in BLOCK_CASES]
