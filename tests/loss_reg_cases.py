"""Label smoothing and z-loss in the shifted cross-entropy (a helper module, not a conftest), shared by tests/test_loss_reg_cases.py (CPU),
tests/test_hip_loss_reg.py (the kernels) and tools/loss_reg_c.py (the constants): the (eps, zeta) grid, the float64 reference with its
error-term arrays - util.shifted_ce_ref extended -, and float32 numpy restatements of the two regularised kernels of csrc/ff_loss.hip in
their operation order, with defects to inject.  The inputs are loss_cases.ce_cases, unchanged.

Per scored row with target t, V columns:   loss = lse - (1 - eps) x_t - eps mean(x) + zeta lse^2,
                                           d_c  = g (p_c (1 + 2 zeta lse) - (1 - eps) [c = t] - eps / V),   p_c = exp(x_c - lse)."""
import numpy as np
import torch

import loss_cases as lc
from util import CE_C_B, CE_C_F, _t64, ce_bound_ok, ce_excess, shifted_ce_ref

GRID = [(0.1, 0.0), (0.0, 1e-4), (0.1, 1e-4), (1.0, 0.5)]          # (label_smoothing, z_loss)
MUTATIONS = ["no-mean-term", "mean-over-V-1", "onehot-unscaled", "eps-over-V-missing", "z-term-missing", "z-grad-without-factor-2"]

# The constants of the bounds, by the method behind util.CE_C_F / CE_C_B (tools/loss_reg_c.py, on the CPU): the worst excess of the float32
# restatements below over the float64 reference at exactly the inputs of tests/test_hip_loss_reg.py - every case of loss_cases.ce_cases at
# every (eps, zeta) of GRID, both dtypes - times 4.
# Worst excess: lse 1.06 (bf16 V = 3: the plain kernel's figure, lse is unchanged); loss 2.37 (bf16 V = 2047 off the grid, eps 1, zeta 0.5;
# fp32 2.15; with zeta = 0: 1.59) - the lse error enters zeta lse^2 twice over, 2 zeta lse dlse, so the term's share is about twice that of
# lse itself; d 1.78 (fp32 V = 50257, eps 0.1, zeta 0: where p is close to eps / V the difference, the quotient eps / V and the product
# with g each round; with eps = 0: 1.02; in bf16 half a storage ulp covers nearly everything: <= 0.40).
# util.CE_C_F = 5.0 and CE_C_B = 3.8 (4 x 1.24 and 4 x 0.95 of the plain kernels) do not cover these, so the regularised kernels get
# constants of their own, by the same rule: c_f = 4 x 2.37, c_b = 4 x 1.78.
# On the MI355X (worst error / bound over the four groups of tests/test_hip_loss_reg.py, 2026-10-20): lse 0.12 (fp32) / 0.11 (bf16), loss
# 0.21 / 0.22; d logits 0.34 in fp32 apart from the two one-dominant-logit patterns, 0.9999: there every other p is below 2^-126, the
# exponential returns 0 and the error is p |g| against the 2^-126 |g| of the bound's last term, as in the plain kernel - which is why the
# backward carries 1 + 2 zeta lse inside the exponent: formed as a product after it, a flushed p whose p (1 + 2 zeta lse) is a normal number
# was 1.018 x the bound at zeta = 1e-4; 0.9998 in bf16: exact results next to a rounding tie, where half a storage ulp is nearly all of
# the bound.  No device figure is above 1.
assert (CE_C_F, CE_C_B) == (5.0, 3.8)
CE_REG_C_F = 9.5
CE_REG_C_B = 7.1


def as_launched(eps, zeta):
    """the two values as the entry points receive them: rounded to float32 (0.1 and 1e-4 are not float32 numbers)"""
    return float(np.float32(eps)), float(np.float32(zeta))


def shifted_ce_reg_ref(logits, labels, g, eps, zeta, ignore_index=-100):
    """util.shifted_ce_ref with label smoothing eps and z-loss zeta (both rounded to float32 first, as the kernels get them), float64 from
    the logits as stored.  The same dict: lse, t_lse and flush unchanged;
      loss = lse - (1 - eps) x_t - eps mean(x) + zeta lse^2, 0 for an ignored label; +inf where eps > 0 and the row holds a -inf logit;
      d = g (p (1 + 2 zeta lse) - (1 - eps) onehot - eps / V), exactly 0 for the last position and for ignored rows;
      t_loss = |lse| + (1 - eps) |x_t| + eps mean|x| + zeta lse^2 + 1 (0 for an ignored label),
      t_d = |g| (p (1 + 2 zeta |lse|) (1 + |x - lse| + |lse|) + (1 - eps) onehot + eps / V)."""
    eps, zeta = as_launched(eps, zeta)
    ref = shifted_ce_ref(logits, labels, g, ignore_index)
    x, g = _t64(logits), _t64(g).reshape(-1)
    lab = labels.detach().cpu().long()
    b, L, V = x.shape
    xs, tgt = x[:, :-1], lab[:, 1:]
    valid = tgt != ignore_index
    lse = ref["lse"].reshape(b, L - 1)
    xt = xs.gather(-1, tgt.clamp(0, V - 1).unsqueeze(-1)).squeeze(-1)
    zero = torch.zeros_like(lse)
    smooth = eps * xs.mean(dim=-1) if eps > 0 else zero                     # (0 x -inf has no place in the definition)
    smooth_abs = eps * xs.abs().mean(dim=-1) if eps > 0 else zero
    loss = torch.where(valid, lse - (1.0 - eps) * xt - smooth + zeta * lse * lse, zero)
    t_loss = torch.where(valid, lse.abs() + (1.0 - eps) * xt.abs() + smooth_abs + zeta * lse * lse + 1.0, zero)
    lse_, zero_ = lse.unsqueeze(-1), torch.zeros_like(xs)
    p = (xs - lse_).exp()
    onehot = torch.zeros_like(xs).scatter_(-1, tgt.clamp(0, V - 1).unsqueeze(-1), 1.0) * valid.unsqueeze(-1)
    gr = (g.reshape(b, L - 1) * valid).unsqueeze(-1)
    d, t_d = torch.zeros_like(x), torch.zeros_like(x)
    d[:, :-1] = torch.where(valid.unsqueeze(-1), (p * (1.0 + 2.0 * zeta * lse_) - (1.0 - eps) * onehot - eps / V) * gr, zero_)
    size = torch.where(p == 0, zero_, p * (1.0 + 2.0 * zeta * lse_.abs()) * (1.0 + (xs - lse_).abs() + lse_.abs()))      # p = 0 at a -inf logit
    t_d[:, :-1] = torch.where(valid.unsqueeze(-1), gr.abs() * (size + (1.0 - eps) * onehot + eps / V), zero_)
    ref.update(loss=loss.reshape(-1), t_loss=t_loss.reshape(-1), d=d, t_d=t_d)
    return ref


def reg_bound_ok(what, got, ref, storage_dtype=torch.float32):
    """util.ce_bound_ok (the same three bounds, on shifted_ce_reg_ref's terms) with the constants of this module"""
    return ce_bound_ok(what, got, ref, storage_dtype, c=CE_REG_C_B if what == "d" else CE_REG_C_F)


def reg_excess(what, got, ref, storage_dtype=torch.float32):
    """util.ce_excess; an element that equals its reference (a +inf loss that is +inf) counts as 0, as in ce_bound_ok - inf - inf is NaN"""
    got = _t64(got).reshape(ref[what].shape)
    same = got == ref[what]
    if bool(same.any()):
        ref = dict(ref)
        got = torch.where(same, torch.zeros_like(got), got)
        ref[what] = torch.where(same, torch.zeros_like(got), ref[what])
        ref["t_" + what] = torch.where(same & torch.isinf(ref["t_" + what]), torch.ones_like(got), ref["t_" + what])
    return ce_excess(what, got, ref, storage_dtype)


# ---- the regularised kernels restated --------------------------------------------------------------------------------------------------------
def row_sums_f32(x, base_off=0):
    """The row sums of x as shifted_ce_fwd_kernel<T, float, float> forms them, float32 (b * (L - 1),): every thread adds its columns in its
    order (lc.thread_columns), the xor-shuffle adds of a wave, then ((w0 + w1) + w2) + w3 over the four waves."""
    dtype = x.dtype
    b, L_, V = x.shape
    X = x.float().numpy()
    starts = lc.row_starts(b, L_, V, dtype, base_off)
    rows = [(s, i) for s in range(b) for i in range(L_ - 1)]
    out = np.empty(len(rows), np.float32)
    with np.errstate(all="ignore"):
        for head in sorted({lc.row_layout(V, dtype, starts[s * L_ + i])[0] for s, i in rows}):
            sel = [k for k, (s, i) in enumerate(rows) if lc.row_layout(V, dtype, starts[s * L_ + i])[0] == head]
            cols = lc.thread_columns(V, dtype, head)
            G = np.stack([X[rows[k][0], rows[k][1]] for k in sel])[:, np.maximum(cols, 0)]          # (R, 256, steps)
            sx = np.zeros(G.shape[:2], np.float32)
            for j in range(cols.shape[1]):
                sx = np.where((cols[:, j] >= 0)[None, :], sx + G[:, :, j], sx)
            sx = sx.reshape(-1, 4, 64)
            for o in (32, 16, 8, 4, 2, 1):
                sx = sx + sx[..., np.arange(64) ^ o]
            w = sx[:, :, 0]
            out[sel] = ((w[:, 0] + w[:, 1]) + w[:, 2]) + w[:, 3]
            assert sx.dtype == np.float32
    return out


def ce_reg_fwd_f32(x, lab, eps, zeta, base_off=0, lse=None, sums=None, mutate=None):
    """The regularised forward in float32 numpy: lse as lc.ce_fwd_f32 gives it (the kernel's (m, s) part is the plain kernel's),
    mean = sum / V, v = lse - (1 - eps) x_t, v -= eps mean (eps > 0 only), loss = v + (zeta lse) lse.  Returns (loss, lse), float32.
    lse / sums: results of lc.ce_fwd_f32 / row_sums_f32 on the same input, to save their recomputation."""
    f = np.float32
    eps, zeta = f(eps), f(zeta)
    b, L_, V = x.shape
    if lse is None:
        lse = lc.ce_fwd_f32(x, lab, base_off)[1]
    l = lse.numpy()
    sx = row_sums_f32(x, base_off) if sums is None else sums
    X, labn = x.float().numpy(), lab.numpy()
    loss = np.empty_like(l)
    with np.errstate(all="ignore"):
        for k, (s, i) in enumerate((s, i) for s in range(b) for i in range(L_ - 1)):
            t = int(labn[s, i + 1])
            if t == lc.IGNORE:
                loss[k] = 0
                continue
            mean = sx[k] / f(V - 1 if mutate == "mean-over-V-1" else V)
            v = l[k] - (f(1) - eps) * X[s, i, t]
            if eps > 0 and mutate != "no-mean-term":
                v = v - eps * mean
            loss[k] = v if mutate == "z-term-missing" else v + (zeta * l[k]) * l[k]
    assert loss.dtype == np.float32
    return torch.from_numpy(loss), lse


def ce_reg_bwd_f32(x, lab, lse, g, eps, zeta, mutate=None):
    """The regularised backward in float32 numpy: per row pk = 1 + (2 zeta) lse, lk = lse - log |pk|, hot = 1 - eps, eov = eps / V, then per
    element d = ((sign(pk) exp(x - lk) - [c = t] hot) - eov) g, rounded to the logits' type; last position and ignored rows exactly 0.
    (pk sits in the exponent: the device's exponential flushes a p below 2^-126 to 0, and p pk may be a normal number.)"""
    f = np.float32
    eps, zeta = f(eps), f(zeta)
    dtype = x.dtype
    b, L_, V = x.shape
    X, labn, l, gn = x.float().numpy(), lab.numpy(), lse.numpy(), g.numpy()
    d = np.zeros((b, L_, V), np.float32)
    with np.errstate(all="ignore"):
        for s in range(b):
            for i in range(L_ - 1):
                t, r = int(labn[s, i + 1]), s * (L_ - 1) + i
                if t == lc.IGNORE or gn[r] == 0:
                    continue
                pk = f(1) if mutate == "z-term-missing" else f(1) + (f(1 if mutate == "z-grad-without-factor-2" else 2) * zeta) * l[r]
                hot = f(1) if mutate == "onehot-unscaled" else f(1) - eps
                eov = f(0) if mutate == "eps-over-V-missing" else eps / f(V)
                onehot = np.zeros(V, np.float32)
                onehot[t] = hot
                lk = l[r] - np.log(np.abs(pk))
                d[s, i] = ((np.exp(X[s, i] - lk) * (f(-1) if pk < 0 else f(1)) - onehot) - eov) * gn[r]
    assert d.dtype == np.float32
    return torch.from_numpy(d).to(dtype)
