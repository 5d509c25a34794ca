"""fp32 gradient accumulation over micro-batches on the MI355X: ff_grad_accumulate, ff_adamw_step_acc, FusedAdamW.accumulate() and
GraphedTrainStep(micro_batches=...).

The kernels run over the tensor list of tests/optim_cases.py (sizes around the vector pieces and the 32768-element chunk, ragged tails, a
zero-element tensor, views one element off the 16-byte grid, 36 tensors = two launch tables).  Gradients, accumulators, parameters, moments
and master copies all live in sentinel-gapped arenas (test_hip_optim_bounds.Arena); every gap must survive every call bit for bit.

The AdamW bound is util.adamw_bound_ok with the project's ADAMW_C, not re-tuned.  Its CPU measurement (the method of tools/adamw_c.py)
repeated for THESE inputs - the float32 restatement of the kernel's formula (optim_cases.adamw_f32_step) reading fp32 gradients
oc.values(300 + step, g_scale) in the three bf16 storage modes, both hyper-parameter sets, unclipped and clipped, steps 1 to 4 from zero
state - gives a worst excess of 4.43 (exp_avg_sq, fp32 moments, clipped, set A; p <= 4.10, exp_avg <= 2.15), below the 5.13 that ADAMW_C =
4 x 5.13 was built from; the least fraction of elements a step changes is 0.65 (the non-vacuity rule asks for 0.25)."""
import ctypes as C

import numpy as np
import pytest
import torch

import optim_cases as oc
import test_hip_optim_bounds as ob
from guarded import guarded_allocations
from util import adamw_bound_ok, adamw_ref_step, rel

pytestmark = pytest.mark.gpu
BF16, F32 = oc.BF16, oc.F32
SEG = ob.SEG
N = len(oc.TENSORS)
NUMELS = (C.c_longlong * N)(*[n for n, _ in oc.TENSORS])
ACC_MODES = ["bf16", "bf16-f32state", "bf16-master"]


def _ffi():
    from flamingo_mini_amd import ffi
    return ffi, ffi.lib()


def _ptrs(arena):
    from flamingo_mini_amd import ffi
    return ffi.ptr_array(arena.views())


def _bits(t):
    return t.view(ob.BITS[t.dtype])


# ---- the accumulate kernel ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("s", [1.0, 0.25, 1.0 / 3.0], ids=["s1", "s0.25", "s1over3"])
@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
def test_accumulate_kernel_is_one_multiply_add_per_element(dtype, s):
    """overwrite=1 onto NaN-filled accumulators: every element is the rounded product (g.float() * s) bit for bit (the accumulator was never
    read).  Then three overwrite=0 calls with fresh gradients, each checked from the accumulator as stored before it: for s = 1 and 0.25 the
    product is exact, so the result must equal torch's fp32 acc_old + g.float() * s bit for bit; for s = 1/3 one rounding (FMA) or two
    (multiply, add) are allowed: |got - (acc_old + s32 g)| <= 2^-24 (|s32 g| + |acc_old + s32 g|) in float64 (s32 g is exact there).
    After every call: gradient bits unchanged, both arenas' gaps intact (the views' direct neighbours included), no NaN."""
    ffi, lib = _ffi()
    ga = ob.Arena(oc.values(200, 0.5), dtype)
    aa = ob.Arena(oc.values(299, 1.0), F32)
    aa.t[aa.own] = float("nan")
    gp, ap, code, stream = _ptrs(ga), _ptrs(aa), ffi.dtype_code(dtype), ffi.stream_handle(ga.t.device)
    s32 = float(np.float32(s))
    for call in range(4):
        if call:
            ga.fill(oc.values(200 + call, 0.5))
        g, g_bits, acc_old = ga.flat(), ga.bits.clone(), aa.flat()
        ffi.check(lib.ff_grad_accumulate(code, N, gp, ap, NUMELS, s, int(call == 0), stream), "ff_grad_accumulate")
        torch.cuda.synchronize()
        got = aa.flat()
        assert torch.equal(ga.bits, g_bits), f"call {call}: the gradients (or their neighbours) were written"
        assert ga.gaps_intact() and aa.gaps_intact(), f"call {call}: an accumulator's neighbours were overwritten"
        assert not torch.isnan(got).any(), f"call {call}: {int(torch.isnan(got).sum())} NaN elements"
        if call == 0:
            want = (g.float() * s).to(F32)
        elif s in (1.0, 0.25):
            want = acc_old + g.float() * s
        else:
            want = None
            e = g.double() * s32
            ref = acc_old.double() + e
            ratio = (got.double() - ref).abs() / (2.0 ** -24 * (e.abs() + ref.abs()) + 1e-300)
            i = int(torch.argmax(ratio))
            print(f"{dtype} s=1/3 call {call}: worst element at {float(ratio[i]):.3f} of its bound")
            assert float(ratio[i]) <= 1.0, f"call {call}: element {ob._where(i)} is {float(ratio[i]):.4g} x its bound"
        if want is not None:
            bad = (_bits(got) != _bits(want)).nonzero()
            assert bad.numel() == 0, f"call {call}: {bad.numel()} elements differ, first {ob._where(int(bad[0]))}: " \
                                     f"got {float(got[int(bad[0])])!r}, want {float(want[int(bad[0])])!r}"
        if call:
            assert float((got != acc_old).float().mean()) > 0.9            # (not vacuous: the fold changed what was stored)


# ---- AdamW reading the accumulators ------------------------------------------------------------------------------------------------------
class _AccState:
    """Parameters, fp32 gradients (the accumulators), moments and master copies of one storage mode in arenas; one step = the library calls
    FusedAdamW.step() makes with a cycle open (ff_grad_sumsq / _reduce / ff_grad_clip_coef over the accumulators when clipped, then
    ff_adamw_step_acc or - `entry` - the call it must equal)."""

    def __init__(self, mode, hpn, clipped):
        self.ffi, self.lib = _ffi()
        self.mode, self.hp, self.clipped = mode, oc.HP[hpn], clipped
        T, ST, master = oc.MODES[mode]
        zeros = np.zeros(ob.TOTAL, np.float32)
        self.pa, self.ga = ob.Arena(oc.p_values(1), T), ob.Arena(oc.values(300, self.hp["g_scale"]), F32)
        self.ma, self.va = ob.Arena(zeros, ST), ob.Arena(zeros, ST)
        self.wa = ob.Arena(self.pa.t.float().cpu().numpy(), F32) if master else None
        self.arenas = [a for a in (self.pa, self.ga, self.ma, self.va, self.wa) if a is not None]
        self.ptrs = [_ptrs(a) for a in (self.pa, self.ga, self.ma, self.va)] + [_ptrs(self.wa) if master else None]
        slots = int(self.lib.ff_grad_sumsq_partials(N, NUMELS))
        self.partials = torch.zeros(slots, device="cuda")
        self.sum = torch.zeros((), dtype=torch.float64, device="cuda")
        self.norm, self.coef = torch.zeros((), device="cuda"), torch.ones((), device="cuda")
        self.step_dev, self.lr_dev = torch.zeros((), device="cuda"), torch.full((), self.hp["lr"], device="cuda")

    def stored(self):
        return self.pa.flat(), self.ma.flat(), self.va.flat(), (self.wa.flat() if self.wa is not None else None)

    def launch(self, step, on_device=False, entry="acc"):
        ffi, lib, hp = self.ffi, self.lib, self.hp
        T, ST, master = oc.MODES[self.mode]
        stream = ffi.stream_handle(self.pa.t.device)
        p, g, m, v, w = self.ptrs
        coef = None
        if self.clipped:
            ffi.check(lib.ff_grad_sumsq(ffi.DTYPE_F32, N, g, NUMELS, hp["grad_scale"], self.partials.data_ptr(), self.partials.numel(), stream), "ff_grad_sumsq")
            ffi.check(lib.ff_grad_sumsq_reduce(self.partials.data_ptr(), self.partials.numel(), self.sum.data_ptr(), 0, stream), "ff_grad_sumsq_reduce")
            ffi.check(lib.ff_grad_clip_coef(self.sum.data_ptr(), hp["max_grad_norm"], self.norm.data_ptr(), self.coef.data_ptr(), stream), "ff_grad_clip_coef")
            coef = self.coef.data_ptr()
        desc = ffi.AdamWDesc(ffi.dtype_code(T), N, 0 if on_device else step, hp["lr"], hp["betas"][0], hp["betas"][1], hp["eps"], hp["weight_decay"],
                             hp["grad_scale"], self.step_dev.data_ptr() if on_device else None)
        lr_dev = self.lr_dev.data_ptr() if on_device else None
        if entry == "acc":
            rc = lib.ff_adamw_step_acc(desc, ffi.dtype_code(ST), p, g, m, v, w, lr_dev, coef, NUMELS, stream)
        elif coef is None:
            rc = lib.ff_adamw_step_mixed(desc, ffi.dtype_code(ST), p, g, m, v, w, lr_dev, NUMELS, stream)
        else:
            rc = lib.ff_adamw_step_clipped(desc, ffi.dtype_code(ST), p, g, m, v, w, lr_dev, coef, NUMELS, stream)
        ffi.check(rc, f"ff_adamw_step_{entry}")

    def step_and_check(self, what, step, run):
        """test_hip_optim_bounds._step_and_check with the fp32 accumulator as the gradient."""
        T, ST, master = oc.MODES[self.mode]
        hp = self.hp
        torch.cuda.synchronize()
        old, g, g_bits = self.stored(), self.ga.flat(), self.ga.bits.clone()
        run()
        torch.cuda.synchronize()
        new = self.stored()
        assert all(a.gaps_intact() for a in self.arenas), f"{what} step {step}: a tensor's neighbours were overwritten"
        assert torch.equal(self.ga.bits, g_bits), f"{what} step {step}: the accumulators were written"
        coef = 1.0
        if self.clipped:
            norm, coef = oc.clip_coef64(g, hp)
            assert coef < 0.5, (norm, hp["max_grad_norm"])                     # a norm that really clips
            assert abs(float(self.norm) - norm) <= 1e-5 * norm, (float(self.norm), norm)
        refs, terms = adamw_ref_step(old[3] if master else old[0], g, old[1], old[2], step, hp["lr"], *hp["betas"], hp["eps"], hp["weight_decay"],
                                     hp["grad_scale"], coef)
        checks = (("master" if master else "p", new[3] if master else new[0], old[3] if master else old[0], F32 if master else T),
                  ("exp_avg", new[1], old[1], ST), ("exp_avg_sq", new[2], old[2], ST))
        for (name, got, before, sd), ref, t in zip(checks, refs, terms):
            ok, worst, idx = adamw_bound_ok(got, ref, t, sd)
            print(f"{what} step {step} {name}: worst element at {worst:.3f} of its bound")
            assert ok, f"{what} step {step}: {name} element {ob._where(idx)} is {worst:.4g} x its bound (got {float(got[idx])!r}, reference {float(ref[idx])!r})"
            changed = ref.to(sd).double() != before.double().cpu()             # from the reference alone: the step is not vacuous
            for k, (a, b) in enumerate(SEG):
                if b - a >= 64:
                    frac = float(changed[a:b].double().mean())
                    assert frac >= 0.25, f"{what} step {step}: only {frac:.2f} of {name} in tensor {k} ({b - a} elements) changes"
        if master:
            assert torch.equal(new[0].view(torch.int16), new[3].to(BF16).view(torch.int16)), f"{what} step {step}: p is not the rounded master copy"


@pytest.mark.parametrize("clipped", [False, True], ids=["unclipped", "clipped"])
@pytest.mark.parametrize("hpn", ["A", "B"])
@pytest.mark.parametrize("mode", ACC_MODES)
def test_adamw_on_accumulators_within_the_element_bound(mode, hpn, clipped):
    """bf16 parameters, fp32 gradients that are NOT bf16-representable (a kernel that read them as bf16 would be off by 2^-9 relative, far
    outside the bound): steps 1 to 3 from zero state with the step count on the host, then step 4 captured with the count and the learning
    rate on the device and replayed once."""
    what = f"acc {mode} {hpn} {'clipped' if clipped else 'unclipped'}"
    st = _AccState(mode, hpn, clipped)
    g0 = st.ga.flat()
    assert float((g0.to(BF16).float() != g0).float().mean()) > 0.9
    for step in (1, 2, 3):
        st.ga.fill(oc.values(300 + step, st.hp["g_scale"]))
        st.step_and_check(what, step, lambda: st.launch(step))
    st.step_dev.fill_(4.0)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        st.launch(4, on_device=True)                  # capture does not execute
    st.ga.fill(oc.values(304, st.hp["g_scale"]))
    st.step_and_check(what + " graph", 4, graph.replay)


@pytest.mark.parametrize("clipped", [False, True], ids=["unclipped", "clipped"])
def test_adamw_acc_on_fp32_parameters_is_the_fp32_kernel(clipped):
    """fp32 parameters: ff_adamw_step_acc dispatches to the existing fp32 kernels - bit for bit ff_adamw_step_mixed / _clipped on the same
    gradients, over three steps."""
    a, b = _AccState("f32", "A", clipped), _AccState("f32", "A", clipped)
    for step in (1, 2, 3):
        for st, entry in ((a, "acc"), (b, "mixed")):
            st.ga.fill(oc.values(300 + step, st.hp["g_scale"]))
            st.launch(step, entry=entry)
        torch.cuda.synchronize()
        for x, y, name in zip(a.stored()[:3], b.stored()[:3], ("p", "exp_avg", "exp_avg_sq")):
            assert torch.equal(_bits(x), _bits(y)), (step, name)
        assert all(ar.gaps_intact() for ar in a.arenas)
    assert not torch.equal(a.pa.flat(), torch.from_numpy(oc.p_values(1))[oc.owned()].cuda())


# ---- the optimizer -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("clipped", [False, True], ids=["unclipped", "clipped"])
@pytest.mark.parametrize("mode", ["bf16", "bf16-master"])
def test_optimizer_accumulates_four_micro_batches_in_fp32_and_steps_on_the_sum(mode, clipped):
    """Four accumulate(0.25) folds of bf16 gradients, then step().  The accumulator against the float64 sum: 0.25 g is exact, the first fold
    stores it unrounded, each of the three later folds rounds one partial sum, |partial sum| <= sum_k |0.25 g_k|, so
            |acc - sum_k 0.25 g_k| <= 3 x 2^-24 x (1 + 2^-20) x sum_k |0.25 g_k|
    (autograd's bf16 `grad += g` has 2^-9 in place of 2^-24).  The step is held to adamw_ref_step on the accumulator as stored, and with
    max_grad_norm the reported norm is the accumulators' (1e-5 relative to float64, the rule of the clip tests)."""
    from flamingo_mini_amd import FusedAdamW
    T, ST, master = oc.MODES[mode]
    hp = oc.HP["A"]
    with guarded_allocations() as guards:
        pa, ga = ob.Arena(oc.p_values(1), T), ob.Arena(oc.values(400, hp["g_scale"]), T)
        params = [torch.nn.Parameter(v) for v in pa.views()]
        opt = FusedAdamW(params, lr=hp["lr"], betas=hp["betas"], eps=hp["eps"], weight_decay=hp["weight_decay"], grad_scale=hp["grad_scale"],
                         master_dtype=F32 if master else None, max_grad_norm=hp["max_grad_norm"] if clipped else None)
        total, size = torch.zeros(SEG[-1][1], dtype=torch.float64), torch.zeros(SEG[-1][1], dtype=torch.float64)
        for k in range(4):
            ga.fill(oc.values(400 + k, hp["g_scale"]))
            g64 = ga.flat().double().cpu() * 0.25
            total, size = total + g64, size + g64.abs()
            for p, g in zip(params, ga.views()):
                p.grad = g
            g_bits = ga.bits.clone()
            opt.accumulate(0.25)
            torch.cuda.synchronize()
            assert all(p.grad is None for p in params)
            assert torch.equal(ga.bits, g_bits) and pa.gaps_intact()
            guards.check()
        acc = torch.cat([opt.accumulated_grad(p).reshape(-1) for p in params])
        assert acc.dtype == F32 and all(opt.accumulated_grad(p).shape == p.shape for p in params)
        ratio = (acc.double().cpu() - total).abs() / (3 * 2.0 ** -24 * (1 + 2.0 ** -20) * size + 1e-300)
        i = int(torch.argmax(ratio))
        print(f"{mode}: worst accumulator element at {float(ratio[i]):.3f} of its bound")
        assert float(ratio[i]) <= 1.0, f"accumulator element {ob._where(i)} is {float(ratio[i]):.4g} x its bound"
        assert float((acc.to(BF16).float() != acc).float().mean()) > 0.5       # the sum has left the bf16 grid: fp32 storage matters
        old = ob._stored(opt, params, pa, mode)
        opt.step()
        torch.cuda.synchronize()
        new = ob._stored(opt, params, pa, mode)
        guards.check()
        assert pa.gaps_intact() and all(opt.accumulated_grad(p) is None for p in params)
        coef = 1.0
        if clipped:
            norm, coef = oc.clip_coef64(acc, hp)
            assert coef < 0.5, (norm, hp["max_grad_norm"])
            assert abs(float(opt.grad_norm) - norm) <= 1e-5 * norm, (float(opt.grad_norm), norm)
        refs, terms = adamw_ref_step(old[3] if master else old[0], acc, old[1], old[2], 1, hp["lr"], *hp["betas"], hp["eps"], hp["weight_decay"],
                                     hp["grad_scale"], coef)
        for name, got, sd, ref, t in (("master" if master else "p", new[3] if master else new[0], F32 if master else T, refs[0], terms[0]),
                                      ("exp_avg", new[1], ST, refs[1], terms[1]), ("exp_avg_sq", new[2], ST, refs[2], terms[2])):
            ok, worst, idx = adamw_bound_ok(got, ref, t, sd)
            print(f"{mode} {name}: worst element at {worst:.3f} of its bound")
            assert ok, f"{name} element {ob._where(idx)} is {worst:.4g} x its bound"
        if master:
            assert torch.equal(new[0].view(torch.int16), new[3].to(BF16).view(torch.int16))
        assert float(opt.state_dict()["state"][0]["step"]) == 1.0 and set(opt.state_dict()["state"][0]) == {"step", "exp_avg", "exp_avg_sq"} | ({"master"} if master else set())


# ---- the whole model: two micro-batches in one graph ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_micro_batched_graph_step_equals_the_full_batch_step_and_the_eager_loop(dtype):
    """h64 fixture (batch 4, labels = ids: both halves hold the same number of targets, so the mean of the two micro-batch losses is the
    full batch's loss).  Three arms from the same state, three training steps each: GraphedTrainStep(micro_batches=2) (warm-up + two
    replays), an ordinary GraphedTrainStep on the full batch, and an eager loop of backward, accumulate(0.5), backward, accumulate(0.5),
    step().  Same parameters to the project's graph-versus-eager tolerance."""
    import copy
    from test_model_plumbing import H64, build_h64
    from flamingo_mini_amd import FusedAdamW, GraphedTrainStep
    base, z, batch = build_h64(dtype, "cuda")
    assert batch["input_ids"].shape[0] == 4
    arms = {"micro": base, "full": copy.deepcopy(base), "eager": copy.deepcopy(base)}
    halves = [{k: v[i * 2:(i + 1) * 2] for k, v in batch.items()} for i in range(2)]
    losses, finals = {}, {}
    for name, model in arms.items():
        opt = FusedAdamW(list(model.parameters_trainable()), capturable=name != "eager", **H64["adamw"])
        if name == "eager":
            out = []
            for _ in range(3):
                model.zero_grad(set_to_none=True)
                parts = []
                for half in halves:
                    loss = model(**half).loss
                    loss.backward()
                    opt.accumulate(0.5)
                    parts.append(float(loss.detach()))
                assert all(p.grad is None for p in model.parameters())
                opt.step()
                out.append(sum(parts) / 2)
        else:
            with GraphedTrainStep(model, opt, batch, warmup=1, micro_batches=2 if name == "micro" else 1) as step:
                out = [None] + [float(step()) for _ in range(2)]
        torch.cuda.synchronize()
        assert {float(s["step"]) for s in opt.state_dict()["state"].values()} == {3.0}
        losses[name] = out
        finals[name] = {k: p.detach().float().clone() for k, p in model.named_parameters() if p.requires_grad}
    tol = 2e-5 if dtype == torch.float32 else 3e-2
    for name in ("full", "eager"):
        for a, b in zip(losses["micro"][1:], losses[name][1:]):
            assert abs(a - b) <= tol * max(1.0, abs(a)), (name, losses)
        for k, v in finals["micro"].items():
            assert rel(v, finals[name][k]) < (1e-4 if dtype == torch.float32 else 3e-2), (name, k)
    model = arms["eager"]
    opt = FusedAdamW(list(model.parameters_trainable()), capturable=True, **H64["adamw"])
    with pytest.raises(ValueError, match="equal chunks"):
        GraphedTrainStep(model, opt, batch, micro_batches=3)
    with pytest.raises(ValueError, match="reducer"):
        GraphedTrainStep(model, opt, batch, micro_batches=2, reducer=object())
