"""Inputs of the per-element AdamW tests (a helper module, not a conftest): ONE tensor list, the hyper-parameter sets and the storage modes
shared by tests/test_hip_optim_bounds.py (the kernels) and tests/test_guarded_checks.py (the checker itself, on the CPU), and a float32
restatement of the kernel's update in torch CPU ops, in the operation order of `update` in csrc/ff_optim.hip - what the checker's
constant is measured with and what its CPU tests mutate.

The list (one chunk = 32768 elements = one workgroup; the vector loop takes two 2048-element pieces per pass, then one piece):
sizes around one piece, two pieces, one chunk and two chunks, ragged tails (1, 3, 513 x 7, 32769), a tensor with a partial last chunk on the
vector path (98304 + 2048 + 8), a zero-element tensor, and two views that start one element off the 16-byte grid with n % 8 == 0 (the
element-wise path at vector-eligible sizes).  The list is laid out twice: 36 non-empty tensors refill the 32-entry pointer table, and the
33rd - the first of the second launch - spans two chunks, so every later tensor's first workgroup is not its index."""
import numpy as np
import torch

BF16, F32 = torch.bfloat16, torch.float32
#                size, elements off the 16-byte grid
ONE_LIST = [(1, 0), (3, 0), (8, 0), (2040, 0), (2048, 0), (2056, 0), (4096, 0), (4104, 0), (3591, 0), (0, 0), (2056, 1), (32760, 0), (32768, 0),
            (32769, 0), (32776, 0), (40968, 1), (65536, 0), (65544, 0), (98304 + 2048 + 8, 0)]
TENSORS = ONE_LIST * 2
GAP = 64                                        # elements between two tensors (a multiple of 16 bytes for both dtypes), all sentinel
SENTINEL = {F32: 0x7EFFA5A5, BF16: 0x7EFF}      # tests/guarded.py's: finite and huge
#   storage of: parameter, moments, fp32 master copy
MODES = {"f32": (F32, F32, False), "bf16": (BF16, BF16, False), "bf16-f32state": (BF16, F32, False), "bf16-master": (BF16, F32, True)}
# Parameters (p_values): 0.125 <= |p| < 0.5.  Below 0.5 half a bf16 ulp is at most 2^-10, less than both learning rates, so an update changes
# the stored value (the non-vacuity condition).  Away from zero because m_new = b1 m + (1 - b1) g' may cancel: its rounding error,
# proportional to |b1 m| + |(1 - b1) g'|, reaches the update amplified by that sum / |m_new|, which |p| + |update| does not know of -
# for |p| >= 0.125 >> lr that error stays far below one fp32 rounding of p, and the constant of adamw_bound_ok stays small and sharp.
# g_scale: set B's scaled gradients (0.08 / 8 = 0.01) are within a factor of ten of its eps, so eps - and through it grad_scale - shows.
# max_grad_norm: far below the norm of the scaled gradients of the list (about 470 / 9.5), asserted where it is used.
HP = {"A": dict(lr=3e-3, betas=(0.9, 0.95), eps=1e-8, weight_decay=0.05, grad_scale=1.0, max_grad_norm=100.0, g_scale=0.5),
      "B": dict(lr=1e-2, betas=(0.8, 0.999), eps=1e-3, weight_decay=0.0, grad_scale=0.125, max_grad_norm=2.0, g_scale=0.08)}


def layout(tensors=TENSORS):
    """([(first element, size)] of every tensor in one flat arena, arena size): each tensor starts GAP or GAP + 1 elements after a
    multiple of 64 elements, so the tensors with offset 0 are 16-byte aligned in both dtypes and the views are one element off."""
    at, out = 0, []
    for n, off in tensors:
        at = (at + GAP + 63) // 64 * 64
        out.append((at + off, n))
        at += off + n
    return out, (at + GAP + 63) // 64 * 64 + 4096


def owned(tensors=TENSORS):
    """flat indices of the arena elements that belong to a tensor, in list order (int64)"""
    lay, _ = layout(tensors)
    return torch.cat([torch.arange(o, o + n) for o, n in lay])


def segments(tensors=TENSORS):
    """[(first, end)] of every tensor in the concatenation of the list"""
    out, at = [], 0
    for n, _ in tensors:
        out.append((at, at + n))
        at += n
    return out


def values(seed, scale, tensors=TENSORS):
    """float32 normal values for a whole arena (the tests overwrite the gaps with the sentinel)"""
    _, total = layout(tensors)
    return (np.random.default_rng(seed).standard_normal(total) * scale).astype(np.float32)


def p_values(seed, tensors=TENSORS):
    """float32 parameter values for a whole arena: random sign, 0.125 <= |p| < 0.5 (see HP)"""
    _, total = layout(tensors)
    rng = np.random.default_rng(seed)
    return (np.where(rng.random(total) < 0.5, -1.0, 1.0) * (0.125 + 0.375 * rng.random(total))).astype(np.float32)


def injected_state(hp, n, seed=77):
    """a state to load before step 1000, (m, v) as float32 numpy of n elements: the update it gives is of the order of lr, and v is so far
    below the squared gradients - the clipped ones too - that one more step changes it by more than a bf16 ulp although (1 - beta2) is
    only 1e-3 in set B (the non-vacuity condition)"""
    rng = np.random.default_rng(seed)
    gs = hp["g_scale"] * hp["grad_scale"]
    m = rng.standard_normal(n) * 0.3 * gs
    v = (0.5 + rng.random(n)) * 0.002 * gs * gs
    return m.astype(np.float32), v.astype(np.float32)


def clip_coef64(g64, hp):
    """(norm, coefficient) of torch.nn.utils.clip_grad_norm_ in float64 from the scaled gradients"""
    norm = float(np.sqrt(float(((g64.double() * float(np.float32(hp["grad_scale"]))) ** 2).sum())))
    return norm, min(1.0, float(np.float32(hp["max_grad_norm"])) / (norm + 1e-6))


def adamw_f32_step(p, g, m, v, w, step, hp, mode, clipped=False, mutate=None):
    """The kernel's formula restated in float32 torch CPU ops, one operation per kernel operation and in its order (no contraction into
    FMAs, host powf for the bias corrections).  p, g: parameter storage; m, v: moment storage; w: the fp32 master copy or None.  Returns
    the new (p, m, v, w) in their storage types.  `mutate` names one defect for the checker's tests:
    keep-p, no-decay, no-bias-correction, eps-in-sqrt, linear-v, no-grad-scale, no-clip."""
    T, ST, master = MODES[mode]
    f = np.float32
    lr, b1, b2, eps, wd, gs = (f(x) for x in (hp["lr"], hp["betas"][0], hp["betas"][1], hp["eps"], hp["weight_decay"], hp["grad_scale"]))
    if mutate == "no-decay":
        wd = f(0)
    if mutate == "no-grad-scale":
        gs = f(1)
    bc1 = f(1) - np.power(b1, f(step))
    bc2_sqrt = np.sqrt(f(1) - np.power(b2, f(step)))
    if mutate == "no-bias-correction":
        bc1, bc2_sqrt = f(1), f(1)
    if clipped:                                     # grad_sumsq (fp32 squares), the fp64 reduction, grad_clip_coef_kernel
        s = (g.float() * float(hp["grad_scale"])).square().sum(dtype=torch.float64)
        nrm = f(np.sqrt(float(s)))
        c = f(hp["max_grad_norm"]) / (nrm + f(1e-6))
        gs = gs * (f(1) if (c > 1 or mutate == "no-clip") else c)
    step_size, keep = lr / bc1, f(1) - lr * wd
    assert all(isinstance(x, np.float32) for x in (step_size, keep, gs, bc2_sqrt))
    pf = (w if master else p).float()
    gr = g.float() * float(gs)
    mf, vf = m.float(), v.float()
    pf = pf * float(keep)
    mf = float(b1) * mf + float(f(1) - b1) * gr
    vf = float(b2) * vf + (float(f(1) - b2) * gr * gr if mutate != "linear-v" else float(f(1) - b2) * gr)
    den = (vf + float(eps)).sqrt() / float(bc2_sqrt) if mutate == "eps-in-sqrt" else vf.sqrt() / float(bc2_sqrt) + float(eps)
    pf = pf - float(step_size) * mf / den
    if mutate == "keep-p":
        pf = (w if master else p).float()
    return pf.to(T), mf.to(ST), vf.to(ST), (pf if master else None)
