"""tests/ema_cases.py checked on the CPU: the numpy restatement of the weight average against the closed form for a constant weight, the
warmup schedule's values, the `every` rule and its own tolerance; and the inputs the GPU tests (tests/test_hip_ema.py) use are not vacuous."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ema_cases as ec  # noqa: E402
import optim_cases as oc  # noqa: E402


@pytest.mark.parametrize("warmup", [False, True], ids=["plain", "warmup"])
@pytest.mark.parametrize("decay", ec.DECAYS)
def test_constant_weight_follows_the_closed_form(decay, warmup):
    """ema_n = theta + (ema_0 - theta) * prod(1 - a_t)"""
    rng = np.random.default_rng(3)
    theta, ema0 = rng.standard_normal(257), rng.standard_normal(257)
    ema, keep = ema0.copy(), 1.0
    for t in range(1, 41):
        ema = ec.ref_step(ema, theta, decay, warmup, 1, t)
        keep *= 1.0 - float(ec.coefficient(decay, warmup, t))
        want = theta + (ema0 - theta) * keep
        assert np.max(np.abs(ema - want)) <= 1e-13 * max(1.0, np.max(np.abs(want))), t
    assert keep < 1.0 and not np.array_equal(ema, ema0)


def test_warmup_schedule_values():
    """d_t = min(decay, (1 + t) / (10 + t)): 2 / 11, 11 / 20 and 1001 / 1010 at t = 1, 10, 1000, capped by the decay; a = 1 - d_t in float32"""
    for t, d in ((1, 2 / 11), (10, 11 / 20), (1000, 1001 / 1010)):
        a = ec.coefficient(0.9999, True, t)
        assert a.dtype == np.float32 and abs(float(a) - (1 - d)) <= 2.0 ** -23, (t, float(a))
        assert a == np.float32(1) - np.float32(np.float32(1 + t) / np.float32(10 + t))
    assert ec.coefficient(0.9, True, 1000) == np.float32(1) - np.float32(0.9)            # the decay caps the schedule ...
    assert ec.coefficient(0.9, True, 10) == np.float32(1) - np.float32(11) / np.float32(20)  # ... only where the schedule is above it
    for t in (1, 10, 1000):
        assert ec.coefficient(0.9999, False, t) == np.float32(1) - np.float32(0.9999)
    assert float(ec.coefficient(0.9999, False, 1)) != 1 - 0.9999                         # (float32 arithmetic, not float64)


def test_every_rule():
    assert [t for t in range(1, 10) if ec.averages(3, t)] == [3, 6, 9]
    assert all(ec.averages(1, t) for t in range(1, 10))
    ema, theta = np.float32([1.0, -2.0]), np.float32([0.5, 0.25])
    assert np.array_equal(ec.ref_step(ema, theta, 0.9, False, 3, 4), ema.astype(np.float64))
    assert not np.array_equal(ec.ref_step(ema, theta, 0.9, False, 3, 6), ema.astype(np.float64))
    assert np.array_equal(ec.ref_step(ema, theta, 0.9, False, 3, 6), ec.ref_step(ema, theta, 0.9, False, 1, 6))


def test_the_bound_passes_the_float32_rule_and_catches_a_wrong_coefficient():
    """One float32 subtraction and one fused multiply-add (emulated: the exact float64 product and sum, rounded once) stay within the bound;
    the update with d_t instead of 1 - d_t, and a stale shadow, do not."""
    rng = np.random.default_rng(5)
    theta = oc.p_values(1)[:4096]
    ema = (rng.standard_normal(4096) * 0.5).astype(np.float32)
    for decay in ec.DECAYS:
        a = ec.coefficient(decay, False, 1)
        ref = ec.ref_step(ema, theta, decay, False, 1, 1)
        diff = (theta - ema).astype(np.float32)
        got = (float(a) * diff.astype(np.float64) + ema.astype(np.float64)).astype(np.float32)
        tol = ec.bound(got, ref, ema, theta, a)
        assert np.all(np.abs(got.astype(np.float64) - ref) <= tol)
        wrong = (float(np.float32(decay)) * diff.astype(np.float64) + ema.astype(np.float64)).astype(np.float32)
        assert np.mean(np.abs(wrong.astype(np.float64) - ref) > ec.bound(wrong, ref, ema, theta, a)) > 0.9
        assert np.mean(np.abs(ema.astype(np.float64) - ref) > ec.bound(ema, ref, ema, theta, a)) > 0.9
    assert ec.ulp32(np.array([1.0, 1.5, 0.75, 2.0 ** -130, 0.0])).tolist() == [2.0 ** -23, 2.0 ** -23, 2.0 ** -24, 2.0 ** -149, 2.0 ** -149]


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("warmup,t", [(False, 2), (True, 1000)], ids=["plain", "warmup-1000"])
@pytest.mark.parametrize("decay", ec.DECAYS)
def test_the_gpu_inputs_are_not_vacuous(decay, warmup, t, dtype):
    """The preloaded shadows against the list's parameter values in both storage types: in every tensor of 64 elements or more at least a
    quarter of the reference results differ from the stored old shadow - on the reference alone."""
    theta = torch.from_numpy(oc.p_values(1)).to(dtype).float().numpy()[oc.owned().numpy()]
    ema = ec.shadow_values()
    assert ema.dtype == np.float32 and ema.shape == theta.shape == (oc.segments()[-1][1],)
    rows = ec.moved_fraction(ec.ref_step(ema, theta, decay, warmup, 1, t), ema)
    assert len(rows) >= 30
    for k, n, frac in rows:
        assert frac >= 0.25, (k, n, frac)
