"""Stochastic rounding on the MI355X: ff_stochastic_round_bf16 and the SR instantiations of adamw_kernel held to the numpy restatement
(tests/sr_cases.py) bit for bit, what the feature is for (updates below half a bf16 ulp accumulate), and determinism.

The optimizer check, per stored bf16 array of one step from the state the kernel itself stored: ref, terms = util.adamw_ref_step's
(float64), E = ADAMW_C 2^-24 terms - the project's bound on the fp32 arithmetic in front of the store - and r = the helper's 16 bits of
the element (seed, the parameter's ordinal, the step, the slot, the element index).  The kernel's fp32 result x lies in [ref - E, ref + E],
and for a fixed r the rule is monotone in x, so
  (a) the stored value lies between the least value any r can make of ref - E and the greatest any r can make of ref + E.  For
      non-negative x these are sr_bf16(ref - E, 0) and sr_bf16(ref + E, 0xFFFF); the rule works on the magnitude, so for negative x
      r = 0xFFFF gives the lower value and r = 0 the higher one, and the check takes whichever applies;
  (b) where sr_bf16(ref - E, r) == sr_bf16(ref + E, r) the stored value equals it EXACTLY; elsewhere it lies between the two, which
      means it is one of the two wherever they are neighbours - everywhere but at the few elements of exp_avg whose two terms cancel
      to less than E, where ref - E and ref + E have opposite signs and many bf16 values lie between them.  The share of elements
      not determined exactly comes from the reference alone and must stay within 1 % of every array (0.04 - 0.29 % in a CPU run
      with numpy random bits in place of Philox), so at least 99 % of every array pins the rule, the slot, the stream id, the step
      and the element index, on the vector and on the element-wise path.
fp32 moments are held to util.adamw_bound_ok as in tests/test_hip_optim_bounds.py, whose arenas and state helpers this file uses."""
import numpy as np
import pytest
import torch

import optim_cases as oc
import sr_cases as sr
import test_hip_optim_bounds as tb
from guarded import guarded_allocations
from util import ADAMW_C, adamw_bound_ok, adamw_ref_step

pytestmark = pytest.mark.gpu
BF16, F32 = oc.BF16, oc.F32
SEED = 0x9E3779B97F4A7C15                        # (above 2^63: the seed crosses the C boundary as a long long)
SPECIALS = np.array([0x00000000, 0x80000000, 0x00000001, 0x807FFFFF, 0x00012345, 0x80654321, 0x7F800000, 0xFF800000, 0x7FC00000, 0xFFC12345,
                     0x7F800001, 0x7F7F0000, 0x7F7F0001, 0xFF7FFFFF, 0x7F7E8000, 0x3F400000, 0xBE9A0000, 0x3F3FFFFF, 0x3F800001, 0x00800000],
                    dtype=np.uint32)           # +-0, denormals, inf, NaNs (quiet, payload, signalling), around the largest finite, representable, ...


def _u16(t):
    return t.contiguous().view(torch.int16).cpu().numpy().view(np.uint16)


# ---- 1. the rule and the bits, on their own ----------------------------------------------------------------------------------------------
def _round_inputs(n, shift):
    """n fp32 bit patterns: normal values over many binades with the special values at the front and at the very end (the ragged tail)"""
    rng = np.random.default_rng(n)
    x = (rng.standard_normal(n) * np.exp2(rng.integers(-20, 20, n))).astype(np.float32).view(np.uint32)
    k = min(n, len(SPECIALS))
    x[:k] = np.roll(SPECIALS, shift)[:k]
    if n > 2 * len(SPECIALS):
        x[-5:] = SPECIALS[[1, 4, 9, 13, 6]]
    return x


def _round(lib, src, dst, n, seed, sid, step, slot):
    from flamingo_mini_amd import ffi
    ffi.check(lib.ff_stochastic_round_bf16(src.data_ptr(), dst.data_ptr(), n, seed - (seed >> 63 << 64), sid, step, slot,
                                           ffi.stream_handle(src.device)), "ff_stochastic_round_bf16")


@pytest.mark.parametrize("n, off", [(1, 0), (7, 0), (8, 0), (2056, 1), (32768 + 8 + 3, 0)], ids=["1", "7", "8", "2056-off-grid", "chunk+8+3"])
def test_round_kernel_equals_the_restatement_bit_for_bit(n, off):
    """Source and destination are guarded allocations (the off-grid case: views one element into them, so the whole tensor takes the
    element-wise path); what the kernel does not own - the guards, the poisoned elements around an off-grid view - keeps every bit."""
    from flamingo_mini_amd import ffi, functional as F
    lib = ffi.lib()
    bits = _round_inputs(n, n % 7)
    args = dict(seed=SEED, sid=12345, step=1000, slot=1)
    with guarded_allocations() as g:
        src_buf, dst_buf = F._new(n + 8, F32, "cuda"), F._new(n + 8, BF16, "cuda")
        src, dst = src_buf[off:off + n], dst_buf[off:off + n]
        assert src.data_ptr() % 16 == 4 * off and dst.data_ptr() % 16 == 2 * off
        src.copy_(torch.from_numpy(bits.view(np.float32)))
        around = _u16(dst_buf).copy()
        outs = {}
        for name, change in [("base", {}), ("seed", dict(seed=SEED ^ 1)), ("seed-high", dict(seed=SEED ^ (1 << 40))), ("stream_id", dict(sid=12346)),
                             ("step", dict(step=1001)), ("slot", dict(slot=2))]:
            a = dict(args, **change)
            _round(lib, src, dst, n, a["seed"], a["sid"], a["step"], a["slot"])
            torch.cuda.synchronize()
            got = _u16(dst_buf)
            want = sr.sr_bf16(bits, sr.sr_bits(n, a["seed"], a["sid"], a["step"], a["slot"]))
            bad = np.nonzero(got[off:off + n] != want)[0]
            assert bad.size == 0, f"{name}: {bad.size} of {n} differ, first element {bad[0]}: x {bits[bad[0]]:#010x} got {got[off + bad[0]]:#06x} want {want[bad[0]]:#06x}"
            assert (got[:off] == around[:off]).all() and (got[off + n:] == around[off + n:]).all(), f"{name}: wrote outside its {n} elements"
            outs[name] = got[off:off + n].copy()
        g.check()
        assert torch.equal(src.view(torch.int32).cpu(), torch.from_numpy(bits.view(np.int32))), "the source was written"
    if n >= 2056:                                  # each of the five inputs of the counter and the key selects other bits
        for name, out in outs.items():
            assert name == "base" or (out != outs["base"]).mean() > 0.2, name
    # the public wrapper is the same call (an aligned output of its own)
    if off == 0:
        y = F.stochastic_round_bf16(torch.from_numpy(bits.view(np.float32)).cuda(), seed=SEED, stream_id=12345, step=1000, slot=1)
        assert y.dtype == BF16 and (_u16(y) == outs["base"]).all()


# ---- 2. one AdamW step, every element ----------------------------------------------------------------------------------------------------
def _bits(step, slot):
    """the helper's 16 bits for every element of the list, concatenated: tensor k is stream k"""
    return np.concatenate([sr.sr_bits(n, SEED, k, step, slot) if n else np.zeros(0, np.uint32) for k, (n, _) in enumerate(oc.TENSORS)])


def _f32_outward(x, up):
    """float64 -> float32 rounded towards +inf (up) or -inf, so that the interval [ref - E, ref + E] never shrinks"""
    y = x.astype(np.float32)
    wrong = (y.astype(np.float64) < x) if up else (y.astype(np.float64) > x)
    return np.where(wrong, np.nextafter(y, np.float32(np.inf if up else -np.inf)), y).astype(np.float32)


def _check_sr_array(what, got, ref, terms, r):
    """(a), (b) and the cap of the module docstring for one stored bf16 array; prints the figures before it asserts"""
    got_bits = _u16(got)
    ref, terms = ref.numpy(), terms.numpy()
    e = ADAMW_C * 2.0 ** -24 * terms
    lo, hi = sr.f32_bits(_f32_outward(ref - e, False)), sr.f32_bits(_f32_outward(ref + e, True))
    neg_lo, neg_hi = (lo >> 31).astype(bool), (hi >> 31).astype(bool)
    least = sr.bf16_to_f64(sr.sr_bf16(lo, np.where(neg_lo, 0xFFFF, 0).astype(np.uint32)))
    most = sr.bf16_to_f64(sr.sr_bf16(hi, np.where(neg_hi, 0, 0xFFFF).astype(np.uint32)))
    a, b = sr.sr_bf16(lo, r), sr.sr_bf16(hi, r)
    open_ = a != b
    share = float(open_.mean()) if open_.size else 0.0
    val = sr.bf16_to_f64(got_bits)
    outside = ~((least <= val) & (val <= most))
    exact_bad = ~open_ & (got_bits != a)
    va, vb = sr.bf16_to_f64(a), sr.bf16_to_f64(b)
    either_bad = open_ & ~((va <= val) & (val <= vb))
    print(f"{what}: {share * 100:.3f} % of {got_bits.size} elements left to one of two values; outside the interval {int(outside.sum())}, "
          f"not the determined value {int(exact_bad.sum())}, not between the two {int(either_bad.sum())}")
    assert share <= 0.01, f"{what}: {share * 100:.2f} % of the elements are not determined by the reference"
    for name, bad in (("outside [least, most]", outside), ("not the value the reference determines", exact_bad), ("not between the two values", either_bad)):
        if bad.any():
            i = int(np.nonzero(bad)[0][0])
            raise AssertionError(f"{what}: {int(bad.sum())} elements {name}; first: element {tb._where(i)}: got {got_bits[i]:#06x}, reference {ref[i]!r} "
                                 f"-> {a[i]:#06x} / {b[i]:#06x} with r = {int(r[i]):#06x}, interval [{least[i]!r}, {most[i]!r}]")


def _make(mode, hpn, variant, capturable, seed=SEED):
    from flamingo_mini_amd import FusedAdamW
    T, ST, _ = oc.MODES[mode]
    hp = oc.HP[hpn]
    pa, ga = tb.Arena(oc.p_values(1), T), tb.Arena(oc.values(100, hp["g_scale"]), T)
    params = [torch.nn.Parameter(v) for v in pa.views()]
    opt = FusedAdamW(params, lr=hp["lr"], betas=hp["betas"], eps=hp["eps"], weight_decay=hp["weight_decay"], grad_scale=hp["grad_scale"],
                     capturable=capturable or variant == "guarded", state_dtype=F32 if ST == F32 else None,
                     max_grad_norm=hp["max_grad_norm"] if variant == "clipped" else None, skip_nonfinite=variant == "guarded",
                     stochastic_rounding=True, sr_seed=seed)
    return pa, ga, params, opt


def _set_grads(params, ga):
    for p, g in zip(params, ga.views()):
        p.grad = g


def _step_and_check(what, opt, params, pa, ga, mode, hpn, variant, step, fill):
    """One step from the stored state with gradient values `fill` (a seed of oc.values), checked as the module docstring says"""
    T, ST, _ = oc.MODES[mode]
    hp = oc.HP[hpn]
    what = f"{what} step {step}"
    old = tb._stored(opt, params, pa, mode)
    if variant == "acc":                           # two folds of 0.5: the accumulators hold fp32 values that bf16 cannot
        for k in (0, 1):
            ga.fill(oc.values(fill + 5000 * k, hp["g_scale"]))
            _set_grads(params, ga)
            opt.accumulate(0.5)
        g = torch.cat([opt.accumulated_grad(p).reshape(-1) for p in params]).clone()
        assert g.dtype == F32 and not torch.equal(g, g.to(BF16).float())
    else:
        ga.fill(oc.values(fill, hp["g_scale"]))
        _set_grads(params, ga)
        g = ga.flat()
    opt.step()
    torch.cuda.synchronize()
    new = tb._stored(opt, params, pa, mode)
    assert pa.gaps_intact(), f"{what}: a parameter's neighbours were overwritten"
    coef = 1.0
    if variant == "clipped":
        norm, coef = oc.clip_coef64(g, hp)
        assert coef < 0.5, (norm, hp["max_grad_norm"])
    if variant == "guarded":
        assert float(opt.step_skipped) == 0.0
    refs, terms = adamw_ref_step(old[0], g, old[1], old[2], step, hp["lr"], *hp["betas"], hp["eps"], hp["weight_decay"], hp["grad_scale"], coef)
    _check_sr_array(f"{what} p", new[0], refs[0], terms[0], _bits(step, sr.SLOT_P))
    for name, got, ref, t, slot in (("exp_avg", new[1], refs[1], terms[1], sr.SLOT_M), ("exp_avg_sq", new[2], refs[2], terms[2], sr.SLOT_V)):
        assert got.dtype == ST
        if ST == BF16:
            _check_sr_array(f"{what} {name}", got, ref, t, _bits(step, slot))
        else:
            ok, worst, idx = adamw_bound_ok(got, ref, t, F32)
            print(f"{what} {name}: worst element at {worst:.3f} of its bound")
            assert ok, f"{what}: {name} element {tb._where(idx)} is {worst:.4g} x its bound"


def _skipped_step_leaves_every_byte(what, opt, params, pa, ga, mode):
    """a non-finite gradient: the guarded SR launch returns before it touches a tensor, and the step number is not used up"""
    hit = int(oc.owned()[12345])
    keep = ga.t[hit].clone()
    ga.t[hit] = float("inf")
    _set_grads(params, ga)
    before_p, before = pa.bits.clone(), [x.clone() for x in tb._stored(opt, params, pa, mode)[1:3]]
    opt.step()
    torch.cuda.synchronize()
    assert float(opt.step_skipped) == 1.0, what
    after = tb._stored(opt, params, pa, mode)[1:3]
    assert torch.equal(pa.bits, before_p) and all(torch.equal(_bytes(a), _bytes(b)) for a, b in zip(after, before)), f"{what}: a skipped step wrote"
    ga.t[hit] = keep


def _bytes(t):
    return t.contiguous().view(torch.uint8)


@pytest.mark.parametrize("variant", ["plain", "clipped", "guarded", "acc"])
@pytest.mark.parametrize("hpn", ["A", "B"])
@pytest.mark.parametrize("mode", ["bf16", "bf16-f32state"])
def test_sr_adamw_every_element_of_every_step(mode, hpn, variant):
    """Steps 1 to 3 from zero state (the step count on the host, except guarded, which needs it on the device; guarded also skips once
    between steps 1 and 2), then step 1000 from a loaded state with the count on the device: the kernel converts *step_dev itself."""
    what = f"{mode} {hpn} {variant}"
    with guarded_allocations() as g:
        pa, ga, params, opt = _make(mode, hpn, variant, capturable=False)
        for step in (1, 2, 3):
            _step_and_check(what, opt, params, pa, ga, mode, hpn, variant, step, 100 + step)
            if variant == "guarded" and step == 1:
                _skipped_step_leaves_every_byte(what, opt, params, pa, ga, mode)
            g.check()
        assert float(opt.state_dict()["state"][0]["step"]) == 3.0
    with guarded_allocations() as g:
        pa, ga, params, opt = _make(mode, hpn, variant, capturable=True)
        tb._load_injected(opt, params, mode, hpn, 999)
        _step_and_check(what + " capturable", opt, params, pa, ga, mode, hpn, variant, 1000, 1100)
        g.check()
        assert float(opt.state_dict()["state"][0]["step"]) == 1000.0


# ---- 3. what it is for -------------------------------------------------------------------------------------------------------------------
N_PURPOSE = 32768
PURPOSE = dict(lr=1e-4, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, capturable=True)


def _f32_restatement(steps):
    """`update`'s formula on one fp32 element (p = 0.75, gradient 1), one operation per kernel operation: (p, exp_avg, exp_avg_sq)"""
    f = np.float32
    p, m, v, lr, b1, b2, eps = f(0.75), f(0), f(0), f(1e-4), f(0.9), f(0.999), f(1e-8)
    for t in range(1, steps + 1):
        m = b1 * m + (f(1) - b1) * f(1)
        v = b2 * v + (f(1) - b2) * f(1) * f(1)
        bc1, bc2_sqrt = f(1) - np.power(b1, f(t)), np.sqrt(f(1) - np.power(b2, f(t)))
        p = p - (lr / bc1) * m / (np.sqrt(v) / bc2_sqrt + eps)
    return float(p), float(m), float(v)


def _constant_run(steps, **kw):
    from flamingo_mini_amd import FusedAdamW
    p = torch.nn.Parameter(torch.full((N_PURPOSE,), 0.75, dtype=BF16, device="cuda"))
    p.grad = torch.ones_like(p)
    opt = FusedAdamW([p], **PURPOSE, **kw)
    for _ in range(steps):
        opt.step()
    torch.cuda.synchronize()
    return p.detach().double().cpu(), opt.state[p]["exp_avg"].double().cpu(), opt.state[p]["exp_avg_sq"].double().cpu()


def test_parameters_move_where_round_to_nearest_loses_every_update():
    """400 steps of lr 1e-4 on p = 0.75 with fp32 moments: 1e-4 is below half a bf16 ulp (2^-9), so round-to-nearest never moves the
    parameter; with SR the mean follows the fp32 run.  Bound: 6 sigma, sigma <= sqrt(400 q (1 - q)) 2^-8 / sqrt(32768), q = lr / 2^-8."""
    want = _f32_restatement(400)[0]
    assert abs(want - 0.709993) < 2e-6, want
    rne, _, _ = _constant_run(400, state_dtype=F32)
    assert bool((rne == 0.75).all()), "the control moved: the premise of this test is gone"
    got, _, _ = _constant_run(400, state_dtype=F32, stochastic_rounding=True, sr_seed=3)
    print(f"mean {float(got.mean()):.6f} (fp32 {want:.6f}), {got.unique().numel()} distinct values")
    assert abs(float(got.mean()) - want) <= 4.2e-4, (float(got.mean()), want)
    assert got.unique().numel() >= 8


def test_bf16_moments_keep_moving_where_round_to_nearest_stalls():
    """2000 steps with bf16 moments: round-to-nearest stalls exp_avg_sq at 0.25 (a third of its value, so the step is 1.86 x too large);
    with SR its mean is 1 - 0.999^2000 and exp_avg's is 1, within 6 sigma of the 0.0194 per-element spread of a CPU run."""
    _, m, v = _constant_run(2000)
    assert bool((v == 0.25).all()) and bool((m == 0.984375).all()), "the control moved: the premise of this test is gone"
    _, m, v = _constant_run(2000, stochastic_rounding=True, sr_seed=3)
    want = 1.0 - 0.999 ** 2000
    print(f"exp_avg_sq mean {float(v.mean()):.6f} (exact {want:.6f}), exp_avg mean {float(m.mean()):.6f}")
    assert abs(float(v.mean()) - want) <= 6.4e-4, (float(v.mean()), want)
    assert abs(float(m.mean()) - 1.0) <= 6.4e-4, float(m.mean())


# ---- 4. determinism ----------------------------------------------------------------------------------------------------------------------
class _Tiny(torch.nn.Module):
    """element-wise only (no GEMM library inside the capture), parameter sizes on and off the vector path"""

    def __init__(self):
        super().__init__()
        gen = torch.Generator().manual_seed(5)
        self.a = torch.nn.Parameter((0.5 + torch.rand(40, 2056, generator=gen)).to(BF16))
        self.b = torch.nn.Parameter((0.5 + torch.rand(2056, generator=gen)).to(BF16))
        self.c = torch.nn.Parameter((0.5 + torch.rand(40, 1, generator=gen)).to(BF16))
        self.d = torch.nn.Parameter((0.5 + torch.rand(3, generator=gen)).to(BF16))

    def forward(self, x):
        h = torch.tanh(x.unsqueeze(1) * self.a + self.b) * self.c
        return (h.float().square().mean() + self.d.float().square().sum()) * 10.0


def _state_bits(model, opt):
    out = []
    for p in model.parameters():
        out += [_u16(p.detach()), _u16(opt.state[p]["exp_avg"]), _u16(opt.state[p]["exp_avg_sq"])]
    return out


def _same(a, b):
    return all((x == y).all() for x, y in zip(a, b))


def _eager_steps(model, opt, x, steps, partition=None):
    for _ in range(steps):
        model.zero_grad(set_to_none=True)
        model(x).backward()
        if partition is None:
            opt.step()
        else:
            for k, only in enumerate(partition(model)):
                opt.step(only=only, advance=k == 0)
    torch.cuda.synchronize()


def test_two_optimizers_built_alike_round_alike_in_every_way_of_stepping():
    """Cloned parameters, 3 steps each: a twin optimizer, GraphedTrainStep replays (step 1 is its eager warm-up, steps 2 and 3 are
    replays of the captured step) and two step(only=...) calls per step in place of one step() all store the same bits; another
    sr_seed does not."""
    from flamingo_mini_amd import FusedAdamW
    from flamingo_mini_amd.graphs import GraphedTrainStep
    x = torch.linspace(-1, 1, 6 * 2056).reshape(6, 2056).to(BF16).cuda()
    kw = dict(lr=1e-3, betas=(0.9, 0.99), weight_decay=0.01, capturable=True, stochastic_rounding=True)

    def fresh(seed=21):
        model = _Tiny().cuda()
        return model, FusedAdamW(list(model.parameters()), sr_seed=seed, **kw)

    model, opt = fresh()
    start = [_u16(p.detach()).copy() for p in model.parameters()]
    _eager_steps(model, opt, x, 3)
    base = _state_bits(model, opt)
    assert not _same(start, base[0::3]), "nothing moved"

    model, opt = fresh()
    _eager_steps(model, opt, x, 3)
    assert _same(_state_bits(model, opt), base), "a twin optimizer rounded differently"

    model, opt = fresh()
    step = GraphedTrainStep(model, opt, dict(x=x), warmup=1, loss_fn=lambda out: out)
    step()
    step()
    torch.cuda.synchronize()
    step.close()
    assert float(opt.state_dict()["state"][0]["step"]) == 3.0
    assert _same(_state_bits(model, opt), base), "graph replays rounded differently from eager steps"

    model, opt = fresh()
    _eager_steps(model, opt, x, 3, partition=lambda m: ({id(m.d), id(m.a)}, {id(m.c), id(m.b)}))
    assert _same(_state_bits(model, opt), base), "step(only=...) in two parts rounded differently from one step()"

    model, opt = fresh(seed=22)
    _eager_steps(model, opt, x, 3)
    other = _state_bits(model, opt)
    assert not _same(other[0::3], base[0::3]) and not _same(other[1::3], base[1::3])
