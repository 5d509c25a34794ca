"""Every AdamW kernel of csrc/ff_optim.hip held to a per-element bound on EACH step, on the MI355X.

The parity tests (test_hip_optim.py, test_hip_grad_clip.py) compare the parameters after four steps with one whole-tensor rel() at 1e-2 in
bf16 - more than AdamW moves a weight in four steps, so the parameter rule itself went unchecked there.  Here every step is checked on its own:
p, m, v (and the fp32 master copy) are read as the kernel stored them, one step runs, and each stored element is held to
util.adamw_ref_step from exactly that state with util.adamw_bound_ok,
        |got - ref| <= 0.5 ulp_storage(ref) + c 2^-24 terms,
so a rounding tie never grows into a divergence between kernel and reference.  All eight instantiations - {fp32, bf16 with bf16 moments,
bf16 with fp32 moments, bf16 with fp32 master copies} x {unclipped, clipped} - run over ONE tensor list (tests/optim_cases.py: sizes around
the vector loop's pieces and the workgroup chunk, ragged tails, a zero-element tensor, views off the 16-byte grid, 36 tensors = two launch
tables), with two hyper-parameter sets, at steps 1 to 3 from zero state, at step 1000 from a loaded state in host-step and in capturable
mode, and in replays of a captured step.  Parameters and gradients live in arenas whose gaps hold a finite sentinel that must survive every
step bit for bit; the moments are guarded allocations (tests/guarded.py).  A step only counts if it is not vacuous: in every tensor of 64
elements or more, at least a quarter of the reference results round to something else than the stored old value.  ff_scale_grads and
ff_grad_sumsq (scale != 1) run over the same list."""
import ctypes as C

import numpy as np
import pytest
import torch

import optim_cases as oc
from guarded import guarded_allocations
from util import adamw_bound_ok, adamw_ref_step

pytestmark = pytest.mark.gpu
BF16, F32 = oc.BF16, oc.F32
LAYOUT, TOTAL = oc.layout()
SEG = oc.segments()
BITS = {F32: torch.int32, BF16: torch.int16}
MODE_IDS = list(oc.MODES)


class Arena:
    """One flat device buffer holding every tensor of the list (oc.layout) with oc.GAP or more sentinel elements around each."""

    def __init__(self, vals, dtype):
        self.dtype = dtype
        self.own = oc.owned().cuda()
        self.gap = torch.ones(TOTAL, dtype=torch.bool, device="cuda")
        self.gap[self.own] = False
        self.t = torch.from_numpy(vals).to(dtype).cuda()
        self.bits = self.t.view(BITS[dtype])
        self.bits[self.gap] = oc.SENTINEL[dtype]
        es = self.t.element_size()
        for (o, n), (_, off) in zip(LAYOUT, oc.TENSORS):             # the aligned tensors are aligned, the views one element off
            assert (self.t.data_ptr() + o * es) % 16 == off * es

    def views(self):
        return [self.t[o:o + n] for o, n in LAYOUT]

    def fill(self, vals):
        """new values into the same storage (the gaps keep their sentinel)"""
        self.t[self.own] = torch.from_numpy(vals).to(self.dtype).cuda()[self.own]

    def flat(self):
        """a copy of the tensors' elements, concatenated in list order"""
        return self.t[self.own]

    def gaps_intact(self):
        return bool((self.bits[self.gap] == oc.SENTINEL[self.dtype]).all())


def _where(idx):
    k = next(i for i, (a, b) in enumerate(SEG) if a <= idx < b)
    return f"{idx - SEG[k][0]} of tensor {k} ({oc.TENSORS[k][0]} elements{', off the 16-byte grid' if oc.TENSORS[k][1] else ''})"


def _make(mode, hpn, clipped, capturable=False):
    from flamingo_mini_amd import FusedAdamW
    T, ST, master = oc.MODES[mode]
    hp = oc.HP[hpn]
    pa, ga = Arena(oc.p_values(1), T), Arena(oc.values(100, hp["g_scale"]), T)
    params = [torch.nn.Parameter(v) for v in pa.views()]
    for p, g in zip(params, ga.views()):
        p.grad = g
        assert p.data_ptr() % 16 == g.data_ptr() % 16
    opt = FusedAdamW(params, lr=hp["lr"], betas=hp["betas"], eps=hp["eps"], weight_decay=hp["weight_decay"], grad_scale=hp["grad_scale"],
                     capturable=capturable, master_dtype=F32 if master else None, state_dtype=F32 if (T, ST, master) == (BF16, F32, False) else None,
                     max_grad_norm=hp["max_grad_norm"] if clipped else None)
    return pa, ga, params, opt


def _stored(opt, params, pa, mode):
    """(p, m, v, w) as they are stored now: flat copies in list order (before the first step: zero moments, the master copy = p)"""
    T, ST, master = oc.MODES[mode]
    p = pa.flat()
    if "exp_avg" not in opt.state.get(params[0], {}):
        z = torch.zeros(p.numel(), dtype=ST, device="cuda")
        return p, z, z.clone(), (p.float() if master else None)
    cat = lambda k: torch.cat([opt.state[q][k].reshape(-1) for q in params])
    m, v = cat("exp_avg"), cat("exp_avg_sq")
    assert m.dtype == ST and v.dtype == ST
    return p, m, v, (cat("master") if master else None)


def _step_and_check(what, opt, params, pa, ga, mode, hpn, clipped, step, lr=None, run=None):
    """One step (opt.step, or `run`) from the stored state: arenas intact, gradients unchanged, every stored element within its bound of the
    float64 step from the old state, the bf16 parameter equal to the rounded master copy, and the step not vacuous."""
    T, ST, master = oc.MODES[mode]
    hp = oc.HP[hpn]
    torch.cuda.synchronize()
    old = _stored(opt, params, pa, mode)
    g = ga.flat()
    g_bits = ga.bits.clone()
    (run or opt.step)()
    torch.cuda.synchronize()
    new = _stored(opt, params, pa, mode)
    assert pa.gaps_intact(), f"{what} step {step}: a parameter's neighbours were overwritten"
    assert torch.equal(ga.bits, g_bits), f"{what} step {step}: the gradients (or their neighbours) were written"
    coef = 1.0
    if clipped:
        norm, coef = oc.clip_coef64(g, hp)
        assert coef < 0.5, (norm, hp["max_grad_norm"])                     # a norm that really clips
        assert abs(float(opt.grad_norm) - norm) <= 1e-5 * norm, (float(opt.grad_norm), norm)
    refs, terms = adamw_ref_step(old[3] if master else old[0], g, old[1], old[2], step, hp["lr"] if lr is None else lr, *hp["betas"], hp["eps"],
                                 hp["weight_decay"], hp["grad_scale"], coef)
    checks = (("master" if master else "p", new[3] if master else new[0], old[3] if master else old[0], F32 if master else T),
              ("exp_avg", new[1], old[1], ST), ("exp_avg_sq", new[2], old[2], ST))
    for (name, got, before, sd), ref, t in zip(checks, refs, terms):
        ok, worst, idx = adamw_bound_ok(got, ref, t, sd)
        print(f"{what} step {step} {name}: worst element at {worst:.3f} of its bound")
        assert ok, f"{what} step {step}: {name} element {_where(idx)} is {worst:.4g} x its bound (got {float(got[idx])!r}, reference {float(ref[idx])!r})"
        changed = ref.to(sd).double() != before.double().cpu()                 # from the reference alone: the step is not vacuous
        for k, (a, b) in enumerate(SEG):
            if b - a >= 64:
                frac = float(changed[a:b].double().mean())
                assert frac >= 0.25, f"{what} step {step}: only {frac:.2f} of {name} in tensor {k} ({b - a} elements) changes"
    if master:
        assert torch.equal(new[0].view(torch.int16), new[3].to(BF16).view(torch.int16)), f"{what} step {step}: p is not the rounded master copy"


def _load_injected(opt, params, mode, hpn, step):
    """load_state_dict of a state `step` steps old: oc.injected_state's moments in the moments' storage type, the master copy = p"""
    T, ST, master = oc.MODES[mode]
    m, v = oc.injected_state(oc.HP[hpn], SEG[-1][1])
    sd = opt.state_dict()
    sd["state"] = {}
    for i, ((a, b), q) in enumerate(zip(SEG, params)):
        st = dict(step=torch.tensor(float(step)), exp_avg=torch.from_numpy(m[a:b]).to(ST).cuda(), exp_avg_sq=torch.from_numpy(v[a:b]).to(ST).cuda())
        if master:
            st["master"] = q.detach().float()
        sd["state"][i] = st
    opt.load_state_dict(sd)
    assert all(opt.state[q]["exp_avg"].dtype == ST and ("master" in opt.state[q]) == master for q in params)


@pytest.mark.parametrize("clipped", [False, True], ids=["unclipped", "clipped"])
@pytest.mark.parametrize("hpn", ["A", "B"])
@pytest.mark.parametrize("mode", MODE_IDS)
def test_adamw_every_step_within_the_element_bound(mode, hpn, clipped):
    """Steps 1 to 3 from zero state, then step 1000 from a loaded state with the step count on the host and on the device (capturable:
    the bias corrections come from the device's powf).  Moments allocated by the optimizer are guarded allocations."""
    what = f"{mode} {hpn} {'clipped' if clipped else 'unclipped'}"
    hp = oc.HP[hpn]
    with guarded_allocations() as g:
        pa, ga, params, opt = _make(mode, hpn, clipped)
        for step in (1, 2, 3):
            ga.fill(oc.values(100 + step, hp["g_scale"]))
            _step_and_check(what, opt, params, pa, ga, mode, hpn, clipped, step)
            g.check()
        assert float(opt.state_dict()["state"][0]["step"]) == 3.0
    for capturable in (False, True):
        with guarded_allocations() as g:
            pa, ga, params, opt = _make(mode, hpn, clipped, capturable)
            _load_injected(opt, params, mode, hpn, 999)
            ga.fill(oc.values(1100, hp["g_scale"]))
            _step_and_check(what + (" capturable" if capturable else " host-step"), opt, params, pa, ga, mode, hpn, clipped, 1000)
            g.check()
            assert float(opt.state_dict()["state"][0]["step"]) == 1000.0


@pytest.mark.parametrize("clipped", [False, True], ids=["unclipped", "clipped"])
@pytest.mark.parametrize("mode", MODE_IDS)
def test_adamw_graph_replays_within_the_element_bound(mode, clipped):
    """One captured capturable step replayed three times, new gradient values in the same storage and a new learning rate before each
    (sync_device_hyperparams): every replay is a step of its own, checked like an eager one."""
    what = f"{mode} {'clipped' if clipped else 'unclipped'} graph"
    hp = oc.HP["A"]
    lrs = [hp["lr"], 2e-3, 6e-3, 4e-3]
    with guarded_allocations() as g:
        pa, ga, params, opt = _make(mode, "A", clipped, capturable=True)
        side = torch.cuda.Stream()

        def eager_on_side_stream():                   # step 1 eagerly: allocates the state, the device counters, the clipping buffers
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):
                opt.step()
            torch.cuda.current_stream().wait_stream(side)

        ga.fill(oc.values(101, hp["g_scale"]))
        _step_and_check(what, opt, params, pa, ga, mode, "A", clipped, 1, run=eager_on_side_stream)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            opt.step()                                # capture does not execute
        for step in (2, 3, 4):
            ga.fill(oc.values(100 + step, hp["g_scale"]))
            opt.param_groups[0]["lr"] = lrs[step - 1]
            opt.sync_device_hyperparams()
            _step_and_check(what, opt, params, pa, ga, mode, "A", clipped, step, lr=lrs[step - 1], run=graph.replay)
        g.check()
        assert float(opt.state_dict()["state"][0]["step"]) == 4.0


def _tables(arena):
    from flamingo_mini_amd import ffi
    views = arena.views()
    return ffi.lib(), ffi.dtype_code(arena.dtype), len(views), ffi.ptr_array(views), (C.c_longlong * len(views))(*[v.numel() for v in views]), \
        ffi.stream_handle(arena.t.device)


@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
def test_scale_grads_is_one_multiply_and_one_rounding(dtype):
    """ff_scale_grads over the list: every element equals (g.float() * coef).to(dtype) bit for bit (one fp32 multiply, one round to nearest
    even), a coefficient of 1 leaves every bit alone, and nothing around a tensor - the views' direct neighbours included - is touched."""
    from flamingo_mini_amd import ffi
    ga = Arena(oc.values(7, 0.5), dtype)
    lib, code, n, ptrs, numels, stream = _tables(ga)
    for c in (1.0, 0.37123):
        coef = torch.tensor(c, dtype=F32, device="cuda")
        before = ga.t.clone()
        want = before.clone()
        want[ga.own] = (before[ga.own].float() * coef).to(dtype)
        ffi.check(lib.ff_scale_grads(code, n, ptrs, numels, coef.data_ptr(), stream), "ff_scale_grads")
        torch.cuda.synchronize()
        assert ga.gaps_intact(), c
        bad = (ga.bits != want.view(BITS[dtype])).nonzero()
        assert bad.numel() == 0, f"coef {c}: {bad.numel()} elements differ, first at arena element {int(bad[0])}"
        if c == 1.0:
            assert torch.equal(ga.bits, before.view(BITS[dtype]))
        else:
            assert not torch.equal(ga.bits, before.view(BITS[dtype]))


@pytest.mark.parametrize("scale", [0.125, 3.0])
@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
def test_sumsq_with_a_scale_matches_float64(dtype, scale):
    """ff_grad_sumsq(scale != 1) over the list (two launch tables, slots continuing) against float64, by test_sumsq_kernel_matches_float64's
    1e-5 rule; one slot per workgroup and none beyond, the gradients untouched."""
    from flamingo_mini_amd import ffi
    ga = Arena(oc.values(8, 0.5), dtype)
    lib, code, n, ptrs, numels, stream = _tables(ga)
    slots = int(lib.ff_grad_sumsq_partials(n, numels))
    assert slots == sum((k + 32767) // 32768 for k, _ in oc.TENSORS)
    before = ga.bits.clone()
    sums = []
    for _ in range(2):
        partials = torch.full((slots + 1,), float("nan"), device="cuda")
        s = torch.empty((), dtype=torch.float64, device="cuda")
        ffi.check(lib.ff_grad_sumsq(code, n, ptrs, numels, scale, partials.data_ptr(), slots, stream), "ff_grad_sumsq")
        ffi.check(lib.ff_grad_sumsq_reduce(partials.data_ptr(), slots, s.data_ptr(), 0, stream), "ff_grad_sumsq_reduce")
        torch.cuda.synchronize()
        assert torch.isnan(partials[slots]) and not torch.isnan(partials[:slots]).any()
        sums.append(float(s))
    ref = float(((ga.flat().double().cpu() * float(np.float32(scale))) ** 2).sum())
    assert abs(sums[0] - ref) <= 1e-5 * ref, (sums[0], ref)
    assert sums[0] == sums[1]                             # fixed slots, fixed order: bit for bit
    assert torch.equal(ga.bits, before)
