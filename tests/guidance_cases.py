"""Inputs of the classifier-free-guidance tests (a helper module, not a conftest): the float64 statement of rules G1 - G3 of
ff_guided_logits (include/flamingo_fusion.h), the bound the kernel is held to, a float32 restatement of guided_logits_kernel
(csrc/ff_guidance.hip) in numpy, and the designed row pairs.  Shared by tests/test_guidance_cases.py (the restatement and the torch form,
on the CPU) and tests/test_hip_guidance.py (the kernel).

A case is a pair of (rows, V) tensors, cond and uncond, each laid out with its OWN row stride and its own offset from the 16-byte grid
(ld == V, ld == 2 V - the [:, -1] view of a (rows, 2, V) tensor -, an odd ld > V; logprob_cases' helpers), a float32 output with a stride
and an offset of its own, and the scales to run it at.  With an odd stride nine rows run through every start phase of either dtype.

The bound (B(.) is the project's log-probability bound, tests/util.py CE_C_F: CE_C_F 2^-24 (|lse*| + |x| + 1)):
    |out - out*| <= |1 - g| B(lu) + g B(lc) + 4 2^-24 (g |lc* - lu*| + |lu*| + |out*|)
out = fmaf(g, lc - lu, lu) is lu (1 - g) + g lc, so the errors of lu and lc enter with |1 - g| and g; the last term covers the roundings
of G2 as the kernel orders them: d = lc - lu rounds once (2^-24 |lc* - lu*|, times g), the fma rounds once (2^-24 |out*|), and lu's own
subtraction is inside B(lu).  The constant 4 leaves room for the second-order terms.  An entry that is -inf in either input must be
exactly -inf; a NaN anywhere it is not due is a miss."""
import numpy as np
import torch

import logprob_cases as LP
import loss_cases as lc

BF16, F32 = lc.BF16, lc.F32
VOCABS = [1, 7, 9, 320, 50257, 50258]
SCALES = [0.0, 0.5, 1.0, 1.5, 3.0, 7.5]                  # all exact in float32
HUGE = {F32: 3.0e4, BF16: 2.0 ** 120}                   # bf16: the top of its exponent range at which 7.5 (lc - lu) (at most 4 |x|) stays finite in float32
NINF = float("-inf")


def rows_for(V):
    return 9 if V < 5000 else 3


def layouts(V):
    """(ld, off) of an input: contiguous, the [:, -1] view of (rows, 2, V), an odd stride off the grid"""
    return [(V, 0), (2 * V, 1), (LP.odd_ld(V), 1)]


def pair(V, dtype, kind="normal", seed=1, rows=None):
    """(cond, uncond), (rows, V) in `dtype` on the CPU.  normal: std 3, the uncond row a noisy copy of the cond row (as the two branches of
    one model are) plus rows that are unrelated; sharp: one logit 80 above the rest, at different columns in the two; flat: a constant row
    against a normal one and a nearly constant one; huge: +-HUGE[dtype]."""
    rows = rows_for(V) if rows is None else rows
    rng = np.random.default_rng(1000 * seed + V)
    c = (rng.standard_normal((rows, V)) * 3.0).astype(np.float32)
    u = (c + rng.standard_normal((rows, V)).astype(np.float32)).astype(np.float32)
    u[rows // 2:] = (rng.standard_normal((rows - rows // 2, V)) * 3.0).astype(np.float32)
    if kind == "sharp":
        c[:, V - 1 - (V > 9) * 8] = c.max(-1) + 80.0
        u[:, V // 2] = u.max(-1) + 80.0
    elif kind == "flat":
        c[::2] = 1.25
        u[1::2] = (rng.standard_normal((len(u[1::2]), V)) * 1e-3).astype(np.float32)
        u[0] = -7.0
    elif kind == "huge":
        h = np.float32(HUGE[dtype])
        c = np.where(c > 0, h, -h).astype(np.float32) + (c if dtype == F32 else 0)
        u = np.where(u > 1, h, -h).astype(np.float32) + (u if dtype == F32 else 0)
        c[:, 0], u[:, V - 1] = h, h                                                       # (no row is all -HUGE)
    else:
        assert kind == "normal", kind
    return torch.from_numpy(c.astype(np.float32)).to(dtype), torch.from_numpy(u.astype(np.float32)).to(dtype)


def neg_inf_masks(where, rows, V, dtype, ld, off):
    """(rows, V) bool: logprob_cases' placements without a token to spare; never a whole row"""
    mask = LP.neg_inf_mask(where, V, dtype, torch.zeros(rows, dtype=torch.long), ld, off)
    mask[:, 0] = where in ("col0", "first300") and V > 1                                # (LP spares the token's column: 0 here)
    if V <= 300 and where == "first300":
        mask[:, V - 1] = False
    if V == 1:
        mask[:] = False
    return mask


def cases(dtype, vocabs=VOCABS):
    """dicts: name, cond, uncond (CPU tensors), ld_c, off_c, ld_u, off_u, ld_o, off_o, scales"""
    k = 0
    for V in vocabs:
        lay = layouts(V)
        c, u = pair(V, dtype)
        for i, (ld_c, off_c) in enumerate(lay):                      # every pair of input layouts, the output's layout and the scale cycling
            for j, (ld_u, off_u) in enumerate(lay):
                ld_o, off_o = [(V, 0), (LP.odd_ld(V), 3), (V + 4, 2), (V, 1)][k % 4]
                yield dict(name=f"V={V} cond ld={ld_c} off={off_c} uncond ld={ld_u} off={off_u} out ld={ld_o} off={off_o}", cond=c, uncond=u, ld_c=ld_c, off_c=off_c,
                           ld_u=ld_u, off_u=off_u, ld_o=ld_o, off_o=off_o, scales=[SCALES[k % 6], SCALES[(k + 3) % 6]] if V < 5000 else [SCALES[k % 6]])
                k += 1
        ld, off = lay[2]
        yield dict(name=f"V={V} every scale", cond=c, uncond=u, ld_c=ld, off_c=off, ld_u=V, off_u=0, ld_o=LP.odd_ld(V), off_o=1, scales=SCALES)
        for kind in ("sharp", "flat", "huge"):
            c2, u2 = pair(V, dtype, kind, seed=2)
            yield dict(name=f"V={V} {kind}", cond=c2, uncond=u2, ld_c=ld, off_c=off, ld_u=ld, off_u=0, ld_o=V, off_o=0, scales=[0.0, 1.5, 7.5] if V < 5000 else [1.5])
    for V in [v for v in vocabs if v in (9, 320, 50258)]:            # -inf: in cond only, in uncond only, in both (the same and different columns)
        ld, off = layouts(V)[2]
        rows = rows_for(V)
        for where in lc.NEG_INF:
            other = lc.NEG_INF[(lc.NEG_INF.index(where) + 1) % len(lc.NEG_INF)]
            for side in ("cond", "uncond", "both", "both-apart"):
                c, u = (t.clone() for t in pair(V, dtype, seed=3))
                if side in ("cond", "both", "both-apart"):
                    c[neg_inf_masks(where, rows, V, dtype, ld, off)] = NINF
                if side in ("uncond", "both"):
                    u[neg_inf_masks(where, rows, V, dtype, V, 0)] = NINF
                if side == "both-apart":
                    u[neg_inf_masks(other, rows, V, dtype, V, 0)] = NINF
                yield dict(name=f"V={V} -inf {where} in {side}", cond=c, uncond=u, ld_c=ld, off_c=off, ld_u=V, off_u=0, ld_o=V, off_o=0,
                           scales=[0.0, 0.5, 1.0, 3.0] if V < 5000 else [0.0, 3.0])


def reference(cond, uncond, g):
    """float64 from the values as stored: dict(out, lc, lu, lse_c, lse_u, ninf) - rules G1 - G3"""
    c, u = cond.double(), uncond.double()
    lse_c, lse_u = torch.logsumexp(c, -1, keepdim=True), torch.logsumexp(u, -1, keepdim=True)
    lc_, lu_ = c - lse_c, u - lse_u
    ninf = (c == NINF) | (u == NINF)
    d = torch.where(ninf, torch.zeros_like(lc_), lc_ - lu_)
    out = torch.where(ninf, torch.full_like(lc_, NINF), lu_ + float(g) * d)
    bad = lambda x: (x.isnan() | (x == float("inf"))).any(-1, keepdim=True)
    out = torch.where(bad(c) | bad(u), torch.full_like(out, float("nan")), out)
    return dict(out=out, lc=lc_, lu=lu_, d=d, lse_c=lse_c, lse_u=lse_u, ninf=ninf, c=c, u=u)


def bound(ref, g, c_f):
    """the stated bound per element (inf where the entry is -inf: those are compared exactly)"""
    e = 2.0 ** -24
    B = lambda lse, x: c_f * e * (lse.abs() + x.abs() + 1.0)
    lu_abs = torch.where(ref["ninf"], torch.zeros_like(ref["lu"]), ref["lu"].abs())
    out_abs = torch.where(ref["ninf"], torch.zeros_like(ref["out"]), ref["out"].abs())
    b = abs(1.0 - g) * B(ref["lse_u"], ref["u"]) + g * B(ref["lse_c"], ref["c"]) + 4.0 * e * (g * ref["d"].abs() + lu_abs + out_abs)
    return torch.where(ref["ninf"], torch.full_like(b, float("inf")), b)


def within_bound(out, cond, uncond, g, c_f):
    """(ok, worst ratio): every finite entry inside the bound, every -inf entry exactly -inf, NaN = a miss"""
    ref = reference(cond, uncond, g)
    got = out.double()
    exact = bool((got[ref["ninf"]] == NINF).all())
    keep = ~ref["ninf"]
    ratio = torch.nan_to_num((got[keep] - ref["out"][keep]).abs() / bound(ref, g, c_f)[keep], nan=float("inf"), posinf=float("inf"))
    worst = float(ratio.max()) if ratio.numel() else 0.0
    return exact and worst <= 1.0, worst


def row_lse_f32(x, ld, off):
    """every row's lse as guided_logits_kernel forms it: the row pass of the loss forward (loss_cases.ce_fwd_f32) at the row's own start"""
    return LP.token_logprob_f32(x, torch.zeros(x.shape[0], dtype=torch.long), ld, off)[1].numpy()


def guided_f32(cond, uncond, g, ld_c=None, off_c=0, ld_u=None, off_u=0):
    """guided_logits_kernel in float32 numpy: (rows, V) float32.  lse per row and input as above; lc = x_c - lse_c, lu = x_u - lse_u,
    d = lc - lu, each rounded to float32; out = fma(g, d, lu) - the product of two float32 is exact in float64, so the fma is the float64
    sum rounded once more; G3's selects."""
    f = np.float32
    C, U = cond.float().numpy(), uncond.float().numpy()
    with np.errstate(all="ignore"):
        lse_c = row_lse_f32(cond, ld_c, off_c)[:, None]
        lse_u = row_lse_f32(uncond, ld_u, off_u)[:, None]
        lc_, lu_ = (C - lse_c).astype(f), (U - lse_u).astype(f)
        d = (lc_ - lu_).astype(f)
        out = (np.float64(f(g)) * d.astype(np.float64) + lu_.astype(np.float64)).astype(f)
        out = np.where((C == -np.inf) | (U == -np.inf), f(-np.inf), out)
        out = np.where(np.isnan(lse_c) | np.isnan(lse_u), f(np.nan), out)
    return torch.from_numpy(out.astype(f))
