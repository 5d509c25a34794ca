"""The weight average of FusedAdamW(ema_decay=...) restated in numpy (a helper module, not a conftest), shared by tests/test_ema_cases.py (the
restatement itself, on the CPU) and tests/test_hip_ema.py (ema_update_kernel of csrc/ff_optim.hip, on the MI355X).

The rule, as in include/flamingo_fusion.h and DESIGN.md - in fp32, each operation rounded once, the same code whether the step count comes
from the host or from the device:

    t    = step_dev ? *step_dev : (float)step                 // number of the step just taken, >= 1
    if (skip && *skip != 0) return;                           // wave-uniform, before any tensor access (as GUARD)
    if (every > 1 && fmodf(t, (float)every) != 0) return;     // wave-uniform
    d_t  = warmup ? fminf(decay, (1.0f + t) / (10.0f + t)) : decay
    a    = 1.0f - d_t
    th   = master ? master[i][e] : (float)params[i][e]        // bf16 widened exactly
    ema[i][e] = fmaf(a, th - ema[i][e], ema[i][e])

`coefficient` computes a in np.float32 exactly as the kernel does: add, divide, min and subtract are correctly rounded in both, so a is
bit-identical.  `ref_step` applies the update in float64.  `bound` is the per-element tolerance of the kernel's result against it,
    |got - ref| <= 0.5 ulp32(max(|got|, |ref|)) + 2 * 2^-24 * a * |th - ema|
derived, not measured: the subtraction is rounded once (relative 2^-24, scaled by a), the fused multiply-add is rounded once (half an ulp
of the result), and the factor 2 on the second term is slack for the binade edge.

The GPU tests preload the shadows with `shadow_values()`, values independent of the parameters (oc.values, not copies of the weights): a
shadow that starts as the weight is one AdamW step of order lr away from it, and at decay 0.9999 the increment 1e-4 * lr * |update| falls
below half an fp32 ulp of the shadow - the step would be vacuous."""
import numpy as np

import optim_cases as oc

DECAYS = (0.9999, 0.9)
SHADOW_SEED, SHADOW_SCALE = 4242, 0.5


def averages(every, t):
    """the `every` rule: is step t one that averages"""
    return every <= 1 or float(np.fmod(np.float32(t), np.float32(every))) == 0.0


def coefficient(decay, warmup, t):
    """a = 1 - d_t as an np.float32, every operation a float32 one"""
    f = np.float32
    d = f(decay)
    if warmup:
        d = min(d, (f(1.0) + f(t)) / (f(10.0) + f(t)))
    a = f(1.0) - d
    assert isinstance(a, np.float32)
    return a


def ref_step(ema, theta, decay, warmup, every, t):
    """float64 shadow after step t from the stored shadow and the weights that step left (any float arrays); a step the `every` rule leaves
    out returns the shadow as it is"""
    e = np.asarray(ema, np.float64)
    if not averages(every, t):
        return e.copy()
    return e + float(coefficient(decay, warmup, t)) * (np.asarray(theta, np.float64) - e)


def ulp32(x):
    """the spacing of float32 at |x| (float64 array), 2^-149 at and below the smallest normal"""
    x = np.abs(np.asarray(x, np.float64))
    _, e = np.frexp(x)
    return np.ldexp(1.0, np.where(x == 0, -149, np.maximum(e - 24, -149)))


def bound(got, ref, ema, theta, a):
    """the per-element tolerance (float64 array); got: the kernel's float32 results, ref: ref_step's, ema / theta: what the step started from"""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    return 0.5 * ulp32(np.maximum(np.abs(got), np.abs(ref))) + 2.0 * 2.0 ** -24 * float(a) * np.abs(np.asarray(theta, np.float64) - np.asarray(ema, np.float64))


def shadow_values(seed=SHADOW_SEED):
    """float32 shadow values for the tensors of oc.TENSORS, concatenated in list order: oc.values, independent of the parameters"""
    return oc.values(seed, SHADOW_SCALE)[oc.owned().numpy()]


def moved_fraction(ref, ema):
    """per tensor of 64 elements or more: the fraction of reference results that, rounded to float32, differ from the stored old shadow"""
    changed = np.asarray(ref, np.float64).astype(np.float32) != np.asarray(ema, np.float32)
    return [(k, b - a, float(changed[a:b].mean())) for k, (a, b) in enumerate(oc.segments()) if b - a >= 64]
