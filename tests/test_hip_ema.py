"""The weight average of FusedAdamW(ema_decay=...) on the MI355X: ema_update_kernel of csrc/ff_optim.hip held to a per-element bound on
every checked step, and the optimizer's plumbing around it.

Every step is checked on its own: the weights theta (the fp32 master copy where there is one, else the parameter) and the shadow are read
as stored, one step runs, and each shadow element is held to tests/ema_cases.py's float64 reference computed from that shadow and the
theta the step produced,
        |got - ref| <= 0.5 ulp32(max(|got|, |ref|)) + 2 * 2^-24 * a * |theta - ema|
(derived there, not measured).  All cases run over the tensor list of tests/optim_cases.py: sizes around the vector pieces and the chunk,
ragged tails, a zero-element tensor, views off the 16-byte grid, 36 non-empty tensors = two launch tables.  Parameters and gradients live
in arenas whose gaps hold a sentinel that must survive; the shadows are guarded allocations (tests/guarded.py).  After the first step -
whose shadow starts as the pre-step weight - the shadows are preloaded with values independent of the parameters, so that a checked step is
not vacuous (tests/test_ema_cases.py): in every tensor of 64 elements or more at least a quarter of the reference results differ from the
stored old shadow."""
import copy

import numpy as np
import pytest
import torch

import ema_cases as ec
import optim_cases as oc
from guarded import guarded_allocations
from test_hip_optim_bounds import Arena, SEG

pytestmark = pytest.mark.gpu
BF16, F32 = oc.BF16, oc.F32
HP = oc.HP["A"]
MODES = ("f32", "bf16", "bf16-master")              # theta = the parameter, the parameter, the master copy
POISONED = 13                                       # the tensor (32769 elements) that gets the inf


def _make(mode, capturable=False, **kw):
    from flamingo_mini_amd import FusedAdamW
    T, _, master = oc.MODES[mode]
    pa, ga = Arena(oc.p_values(1), T), Arena(oc.values(100, HP["g_scale"]), T)
    params = [torch.nn.Parameter(v) for v in pa.views()]
    for p, g in zip(params, ga.views()):
        p.grad = g
    opt = FusedAdamW(params, lr=HP["lr"], betas=HP["betas"], eps=HP["eps"], weight_decay=HP["weight_decay"], capturable=capturable,
                     master_dtype=F32 if master else None, **kw)
    return pa, ga, params, opt


def _grads(ga, seed):
    ga.fill(oc.values(seed, HP["g_scale"]))


def _theta(opt, params, pa):
    """the weights as stored, float64 numpy in list order: the master copies where the state has them, else the parameters"""
    if "master" in opt.state.get(params[0], {}):
        return torch.cat([opt.state[q]["master"].reshape(-1) for q in params]).double().cpu().numpy()
    return pa.flat().double().cpu().numpy()


def _shadows(opt, params):
    out = [opt.state[q]["ema"] for q in params]
    assert all(s.dtype == F32 and s.shape == q.shape and s.is_contiguous() for s, q in zip(out, params))
    return torch.cat([s.reshape(-1) for s in out])


def _state_bits(opt, params, pa):
    """everything a step may write, as bits: parameter arena, moments, master copies, shadows"""
    out = {"p": pa.bits.clone()}
    for k in ("exp_avg", "exp_avg_sq", "master", "ema"):
        if k in opt.state.get(params[0], {}):
            t = torch.cat([opt.state[q][k].reshape(-1) for q in params])
            out[k] = t.view(torch.int32 if t.dtype == F32 else torch.int16).clone()
    return out


def _preload(opt, params):
    vals = torch.from_numpy(ec.shadow_values()).cuda()
    for q, (a, b) in zip(params, SEG):
        opt.state[q]["ema"].copy_(vals[a:b])


def _steps_taken(opt):
    return float(opt.state_dict()["state"][0]["step"])


def _held(what, got, ema_old, theta, decay, warmup, every, t, vacuity):
    """every element of `got` (float32 numpy) within its bound of the float64 step t from (ema_old, theta)"""
    ref = ec.ref_step(ema_old, theta, decay, warmup, every, t)
    a = ec.coefficient(decay, warmup, t)
    ratio = np.abs(got.astype(np.float64) - ref) / ec.bound(got, ref, ema_old, theta, a)
    assert not np.isnan(ratio).any(), f"{what} step {t}: NaN in the shadows"
    worst = int(np.argmax(ratio)) if ratio.size else 0
    print(f"{what} step {t}: a = {float(a):.6g}, worst element at {float(ratio[worst]) if ratio.size else 0.0:.3f} of its bound")
    assert not ratio.size or ratio[worst] <= 1.0, \
        f"{what} step {t}: element {worst} is {ratio[worst]:.4g} x its bound (got {got[worst]!r}, reference {ref[worst]!r}, old {ema_old[worst]!r})"
    if vacuity:
        for k, n, frac in ec.moved_fraction(ref, ema_old):
            assert frac >= 0.25, f"{what} step {t}: only {frac:.2f} of the shadow of tensor {k} ({n} elements) changes"


def _step_and_check(what, opt, params, pa, ga, t, run=None, vacuity=True):
    """One step (opt.step, or `run`) from the stored state: arenas intact, gradients unchanged, every shadow element within its bound.  A
    step from fresh state is checked against the reference started from the pre-step weight."""
    torch.cuda.synchronize()
    theta_old = _theta(opt, params, pa)
    fresh = "ema" not in opt.state.get(params[0], {})
    ema_old = theta_old.astype(np.float32) if fresh else _shadows(opt, params).cpu().numpy()
    g_bits = ga.bits.clone()
    (run or opt.step)()
    torch.cuda.synchronize()
    assert pa.gaps_intact(), f"{what} step {t}: a parameter's neighbours were overwritten"
    assert torch.equal(ga.bits, g_bits), f"{what} step {t}: the gradients (or their neighbours) were written"
    theta = _theta(opt, params, pa)
    assert not np.array_equal(theta, theta_old)
    _held(what, _shadows(opt, params).cpu().numpy(), ema_old, theta, opt.ema_decay, opt.ema_warmup, opt.ema_every, t, vacuity and not fresh)


def _load(opt, params, mode, step):
    """load_state_dict of a state `step` steps old (oc.injected_state's moments, the master copy = p, ec.shadow_values' shadows); the loaded
    shadows then move into guarded allocations"""
    from flamingo_mini_amd import functional as F
    T, ST, master = oc.MODES[mode]
    m, v = oc.injected_state(HP, SEG[-1][1])
    ema = ec.shadow_values()
    sd = opt.state_dict()
    sd["state"] = {}
    for i, ((a, b), q) in enumerate(zip(SEG, params)):
        st = dict(step=torch.tensor(float(step)), exp_avg=torch.from_numpy(m[a:b]).to(ST).cuda(), exp_avg_sq=torch.from_numpy(v[a:b]).to(ST).cuda(),
                  ema=torch.from_numpy(ema[a:b]).cuda())
        if master:
            st["master"] = q.detach().float()
        sd["state"][i] = st
    opt.load_state_dict(sd)
    for q, (a, b) in zip(params, SEG):
        loaded = opt.state[q]["ema"]
        assert loaded.dtype == F32 and np.array_equal(loaded.cpu().numpy(), ema[a:b])
        opt.state[q]["ema"] = F._new_like(q.detach(), dtype=F32)
        opt.state[q]["ema"].copy_(loaded)


# ---------------------------------------------------------------------------------------------------------------- 1. the per-element bound
@pytest.mark.parametrize("decay", ec.DECAYS)
@pytest.mark.parametrize("warmup", [False, True], ids=["plain", "warmup"])
@pytest.mark.parametrize("capturable", [False, True], ids=["host-step", "capturable"])
@pytest.mark.parametrize("mode", MODES)
def test_every_checked_step_within_the_element_bound(mode, capturable, warmup, decay):
    """Steps 1 to 3 from fresh state (the shadows preloaded after step 1), then step 1000 from a loaded state."""
    what = f"{mode} {'capturable' if capturable else 'host-step'} {'warmup' if warmup else 'plain'} {decay}"
    kw = dict(ema_decay=decay, ema_warmup=warmup)
    with guarded_allocations() as g:
        pa, ga, params, opt = _make(mode, capturable, **kw)
        for t in (1, 2, 3):
            _grads(ga, 100 + t)
            _step_and_check(what, opt, params, pa, ga, t)
            if t == 1:
                assert [id(p) for p, _ in opt.ema_parameters()] == [id(p) for p in params]
                _preload(opt, params)
            g.check()
        assert _steps_taken(opt) == 3.0
    with guarded_allocations() as g:
        pa, ga, params, opt = _make(mode, capturable, **kw)
        _load(opt, params, mode, 999)
        _grads(ga, 1100)
        _step_and_check(what + " loaded", opt, params, pa, ga, 1000)
        g.check()
        assert _steps_taken(opt) == 1000.0


# ---------------------------------------------------------------------------------------------------------------- 2. off means off
def test_without_the_arguments_nothing_is_kept_and_the_weights_are_the_same():
    pa, ga, params, plain = _make("bf16-master")
    pb, gb, others, averaging = _make("bf16-master", ema_decay=0.9)
    for t in (1, 2):
        for arena in (ga, gb):
            _grads(arena, 100 + t)
        plain.step()
        averaging.step()
    torch.cuda.synchronize()
    assert all("ema" not in plain.state[q] for q in params) and list(plain.ema_parameters()) == []
    sd = plain.state_dict()
    assert set(sd) == {"state", "param_groups"} and all(set(st) == {"step", "exp_avg", "exp_avg_sq", "master"} for st in sd["state"].values())
    group = set(sd["param_groups"][0])
    assert {"lr", "betas", "eps", "weight_decay", "grad_scale", "capturable", "params"} <= group and not any("ema" in k for k in group)
    assert set(averaging.state_dict()["param_groups"][0]) == group       # the settings are optimizer-wide: in no group
    assert all(set(st) == {"step", "exp_avg", "exp_avg_sq", "master", "ema"} for st in averaging.state_dict()["state"].values())
    a, b = _state_bits(plain, params, pa), _state_bits(averaging, others, pb)
    assert set(b) - set(a) == {"ema"}
    for k in a:                                      # the average only reads the weights
        assert torch.equal(a[k], b[k]), k


# ---------------------------------------------------------------------------------------------------------------- 3. skipped steps
@pytest.mark.parametrize("mode", ["f32", "bf16-master"])
def test_a_step_skipped_on_the_device_leaves_the_shadows_and_the_warmup_alone(mode):
    """skip_nonfinite with one inf in a gradient: shadows, moments, weights and the step counter stay bit for bit, skipped_steps counts, and
    the next taken step averages with the un-advanced t (warmup on: t shows in the coefficient)."""
    what = f"{mode} guarded"
    with guarded_allocations() as g:
        pa, ga, params, opt = _make(mode, True, skip_nonfinite=True, ema_decay=0.9999, ema_warmup=True)
        _grads(ga, 101)
        _step_and_check(what, opt, params, pa, ga, 1)
        _preload(opt, params)
        _grads(ga, 102)
        _step_and_check(what, opt, params, pa, ga, 2)
        _grads(ga, 103)
        ga.views()[POISONED][5] = float("inf")
        torch.cuda.synchronize()
        before = _state_bits(opt, params, pa)
        opt.step()
        torch.cuda.synchronize()
        assert float(opt.step_skipped) == 1.0 and int(opt.skipped_steps) == 1 and _steps_taken(opt) == 2.0
        after = _state_bits(opt, params, pa)
        for k in before:
            assert torch.equal(before[k], after[k]), f"{what}: {k} changed in a skipped step"
        _grads(ga, 104)
        _step_and_check(what + " after the skip", opt, params, pa, ga, 3)
        assert float(opt.step_skipped) == 0.0 and int(opt.skipped_steps) == 1 and _steps_taken(opt) == 3.0
        g.check()


def test_a_step_skipped_by_a_grad_scaler_leaves_the_shadows_and_the_warmup_alone():
    """torch.amp.GradScaler.step(opt) hands found_inf over on the device: the same, without skip_nonfinite."""
    what = "f32 GradScaler"
    pa, ga, params, opt = _make("f32", True, ema_decay=0.9999, ema_warmup=True)
    scaler = torch.amp.GradScaler("cuda", init_scale=8.0)

    def scaled_step(seed, poison=False):
        xs = Arena(oc.values(seed, HP["g_scale"]), F32).views()
        if poison:
            xs[POISONED][5] = float("inf")

        def run():
            opt.zero_grad(set_to_none=True)
            scaler.scale(sum((p * x).sum() for p, x in zip(params, xs))).backward()
            scaler.step(opt)
            scaler.update()
        return run

    _step_and_check(what, opt, params, pa, ga, 1, run=scaled_step(201))
    _preload(opt, params)
    torch.cuda.synchronize()
    before = _state_bits(opt, params, pa)
    scaled_step(202, poison=True)()
    torch.cuda.synchronize()
    assert float(opt.step_skipped) == 1.0 and _steps_taken(opt) == 1.0
    after = _state_bits(opt, params, pa)
    for k in before:
        assert torch.equal(before[k], after[k]), f"{what}: {k} changed in a skipped step"
    _step_and_check(what + " after the skip", opt, params, pa, ga, 2, run=scaled_step(203))
    assert float(opt.step_skipped) == 0.0 and _steps_taken(opt) == 2.0


# ---------------------------------------------------------------------------------------------------------------- 4. ema_every
@pytest.mark.parametrize("how", ["host-step", "capturable", "graph"])
def test_ema_every_3_averages_on_steps_3_and_6_only(how):
    """Host mode does not issue the launch on the other steps, capturable mode and the replays of one captured step() decide on the device:
    the shadows change on steps 3 and 6 - within the bound - and are bit-identical after every other step."""
    with guarded_allocations() as g:
        pa, ga, params, opt = _make("bf16", how != "host-step", ema_decay=0.9, ema_every=3)
        side, graph = torch.cuda.Stream(), None

        def eager_on_side_stream():
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):
                opt.step()
            torch.cuda.current_stream().wait_stream(side)

        for t in range(1, 7):
            _grads(ga, 100 + t)
            run = opt.step if how != "graph" else (eager_on_side_stream if t == 1 else graph.replay)
            if t in (3, 6):
                old = _shadows(opt, params).clone()
                _step_and_check(f"every-3 {how}", opt, params, pa, ga, t, run=run, vacuity=False)
                moved = (_shadows(opt, params).view(torch.int32) != old.view(torch.int32)).double().mean()
                assert float(moved) > 0.5, (t, float(moved))
            else:
                torch.cuda.synchronize()
                old = _theta(opt, params, pa).astype(np.float32) if t == 1 else _shadows(opt, params).cpu().numpy()
                run()
                torch.cuda.synchronize()
                assert np.array_equal(_shadows(opt, params).cpu().numpy().view(np.int32), old.view(np.int32)), f"{how}: the shadows moved in step {t}"
            if how == "graph" and t == 1:
                graph = torch.cuda.CUDAGraph()
                with torch.cuda.graph(graph):
                    opt.step()
        g.check()
        assert _steps_taken(opt) == 6.0


# ---------------------------------------------------------------------------------------------------------------- 5. capture
@pytest.mark.parametrize("mode", ["bf16", "bf16-master"])
def test_replays_of_a_captured_step_equal_eager_steps_bit_for_bit(mode):
    kw = dict(ema_decay=0.9999, ema_warmup=True)
    pa, ga, params, opt = _make(mode, True, **kw)
    pb, gb, others, eager = _make(mode, True, **kw)
    side = torch.cuda.Stream()
    _grads(ga, 101)
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        opt.step()                                    # step 1 eagerly: allocates the state, the shadows, the device counters
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        opt.step()
    _grads(gb, 101)
    eager.step()
    for t in (2, 3, 4):
        _grads(ga, 100 + t)
        _grads(gb, 100 + t)
        graph.replay()
        eager.step()
    torch.cuda.synchronize()
    assert _steps_taken(opt) == _steps_taken(eager) == 4.0
    a, b = _state_bits(opt, params, pa), _state_bits(eager, others, pb)
    assert "ema" in a and set(a) == set(b)
    for k in a:
        assert torch.equal(a[k], b[k]), k
    assert not torch.equal(_shadows(opt, params), torch.from_numpy(oc.p_values(1)[oc.owned().numpy()]).to(oc.MODES[mode][0]).float().cuda())


@pytest.mark.parametrize("kind,dtype", [("graphed", F32), ("graphed", BF16), ("micro", BF16)], ids=["graphed-f32", "graphed-bf16-master", "micro-bf16-master"])
def test_graphed_train_step_averages_inside_the_graph(kind, dtype):
    """GraphedTrainStep at the h64 fixture model (micro: micro_batches=2), graphs.py as it is: after each of two replays every shadow is within
    the bound of the reference applied to the weights that replay left - the second one after the LR scheduler changed group["lr"]."""
    from flamingo_mini_amd import FusedAdamW, GraphedTrainStep
    from test_model_plumbing import H64, build_h64
    model, _, batch = build_h64(dtype, "cuda")
    opt = FusedAdamW(list(model.parameters_trainable()), capturable=True, master_dtype=F32 if dtype == BF16 else None, ema_decay=0.9,
                     ema_warmup=True, **H64["adamw"])
    step = GraphedTrainStep(model, opt, batch, warmup=1, micro_batches=2 if kind == "micro" else 1)      # (the warm-up is training step 1)
    pairs = list(opt.ema_parameters())
    assert len(pairs) >= 30 and all(s.dtype == F32 and s.shape == p.shape for p, s in pairs)
    weight = lambda p: opt.state[p]["master"] if dtype == BF16 else p.detach()
    flat = lambda ts: torch.cat([t.reshape(-1) for t in ts]).double().cpu().numpy()
    for t in (2, 3):
        if t == 3:
            opt.param_groups[0]["lr"] = 3 * H64["adamw"]["lr"]
        torch.cuda.synchronize()
        old, theta_old = flat([s for _, s in pairs]).astype(np.float32), flat([weight(p) for p, _ in pairs])
        step()
        torch.cuda.synchronize()
        theta = flat([weight(p) for p, _ in pairs])
        got = flat([s for _, s in pairs]).astype(np.float32)
        _held(f"{kind} {dtype}", got, old, theta, 0.9, True, 1, t, vacuity=False)
        assert float(np.mean(theta != theta_old)) > 0.5 and float(np.mean(got != old)) > 0.5
    step.close()
    assert _steps_taken(opt) == 3.0


# ---------------------------------------------------------------------------------------------------------------- 6. partition, resume
def test_partial_steps_average_exactly_what_they_update():
    kw = dict(ema_decay=0.9999, ema_warmup=True)
    pa, ga, params, opt = _make("bf16-master", True, **kw)
    pb, gb, others, whole = _make("bf16-master", True, **kw)
    first, second = {id(p) for p in params[0::2]}, {id(p) for p in params[1::2]}
    for t in (1, 2):
        _grads(ga, 100 + t)
        _grads(gb, 100 + t)
        opt.step(only=first, advance=True)
        if t == 1:
            assert [id(p) for p, _ in opt.ema_parameters()] == [id(p) for p in params[0::2]]
        opt.step(only=second, advance=False)
        whole.step()
    torch.cuda.synchronize()
    assert _steps_taken(opt) == _steps_taken(whole) == 2.0
    a, b = _state_bits(opt, params, pa), _state_bits(whole, others, pb)
    for k in ("p", "master", "ema"):
        assert torch.equal(a[k], b[k]), k
    assert pa.gaps_intact()


@pytest.mark.parametrize("mode", ["bf16", "bf16-master"])
def test_resuming_from_a_state_dict_continues_the_same_shadows(mode):
    kw = dict(ema_decay=0.9999, ema_warmup=True)
    pa, ga, params, straight = _make(mode, **kw)
    pb, gb, others, first = _make(mode, **kw)
    for t in (1, 2, 3):
        _grads(ga, 100 + t)
        straight.step()
    for t in (1, 2):
        _grads(gb, 100 + t)
        first.step()
    torch.cuda.synchronize()
    sd = copy.deepcopy(first.state_dict())
    assert all(st["ema"].dtype == F32 for st in sd["state"].values())
    pc, gc, resumed_params, resumed = _make(mode, **kw)
    pc.t.copy_(pb.t)
    resumed.load_state_dict(sd)
    assert all(resumed.state[q]["ema"].dtype == F32 and (q.numel() == 0 or resumed.state[q]["ema"].data_ptr() != first.state[p]["ema"].data_ptr())
               for q, p in zip(resumed_params, others))
    _grads(gc, 103)
    resumed.step()
    torch.cuda.synchronize()
    a, c = _state_bits(straight, params, pa), _state_bits(resumed, resumed_params, pc)
    assert set(a) == set(c)
    for k in a:
        assert torch.equal(a[k], c[k]), k


# ---------------------------------------------------------------------------------------------------------------- 7. swap_ema
@pytest.mark.parametrize("mode", MODES)
def test_swap_ema_is_in_place_and_restores_every_bit(mode):
    pa, ga, params, opt = _make(mode, ema_decay=0.9)
    for t in (1, 2):
        _grads(ga, 100 + t)
        opt.step()
    torch.cuda.synchronize()
    before = _state_bits(opt, params, pa)
    ptrs = [p.data_ptr() for p in params]
    bits = torch.int32 if params[0].dtype == F32 else torch.int16

    def swapped_and_guarded():
        assert [p.data_ptr() for p in params] == ptrs and pa.gaps_intact()
        pairs = list(opt.ema_parameters())
        assert [id(p) for p, _ in pairs] == [id(p) for p in params]
        for p, s in pairs:
            assert torch.equal(p.detach().view(bits), s.to(p.dtype).view(bits))
        inside = _state_bits(opt, params, pa)
        assert not torch.equal(inside["p"], before["p"])
        for k in before:
            if k != "p":
                assert torch.equal(inside[k], before[k]), k
        for call in (opt.step, opt.accumulate, lambda: opt.swap_ema().__enter__()):
            with pytest.raises(RuntimeError, match="swap_ema"):
                call()

    with opt.swap_ema() as inner:
        assert inner is opt
        swapped_and_guarded()
    torch.cuda.synchronize()
    after = _state_bits(opt, params, pa)
    for k in before:
        assert torch.equal(after[k], before[k]), k
    with pytest.raises(KeyError):
        with opt.swap_ema():
            swapped_and_guarded()
            raise KeyError("left by an exception")
    torch.cuda.synchronize()
    after = _state_bits(opt, params, pa)
    for k in before:
        assert torch.equal(after[k], before[k]), k
    scratch = torch.zeros(8, device="cuda")
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        scratch.add_(1.0)
        with pytest.raises(RuntimeError, match="capturing"):
            opt.swap_ema().__enter__()
    _grads(ga, 103)
    _step_and_check(f"{mode} after swap_ema", opt, params, pa, ga, 3, vacuity=False)      # the optimizer goes on as if nothing had happened


def test_decode_sessions_stay_valid_and_decode_with_the_averaged_weights():
    """The tiny GPT-2-backed fixture model: a greedy static-decode session created before the block is not stale inside it, and the tokens
    generate(static_decode=True) returns inside equal, token for token, those of a second model instance loaded with the
    state_dict_trainable() taken inside the block."""
    from flamingo_mini_amd import FusedAdamW
    from test_model_plumbing import build
    model, z = build(torch.float32, "cuda", "gpt2")
    model.eval()
    ids, ml = torch.from_numpy(z["ids"])[:, :4].cuda(), torch.from_numpy(z["ml"])[:, :4].cuda()
    kw = dict(media_locations=ml, attention_mask=torch.ones_like(ids), pixel_values=torch.from_numpy(z["px"]).float().cuda(), max_length=10,
              static_decode=True)
    try:
        params = list(model.parameters_trainable())
        opt = FusedAdamW(params, lr=0.3, weight_decay=0.0, ema_decay=0.5)
        gen = torch.Generator(device="cuda").manual_seed(11)
        for _ in range(4):                            # four huge steps (about +-lr per element each) along random gradients: the average is a different model from the last iterate
            for p in params:
                p.grad = torch.randn(p.shape, generator=gen, device="cuda")
            opt.step()
        outside = model.generate(ids, **kw)
        (sess,) = model._decode_sessions.values()
        ptrs = [p.data_ptr() for p in params]
        with opt.swap_ema():
            assert not sess.stale() and [p.data_ptr() for p in params] == ptrs
            inside = model.generate(ids, **kw)
            assert list(model._decode_sessions.values()) == [sess]
            averaged = {k: v.detach().clone() for k, v in model.state_dict_trainable().items()}
        again = model.generate(ids, **kw)
        twin, _ = build(torch.float32, "cuda", "gpt2")
        twin.eval()
        missing, unexpected = twin.flamingo.load_state_dict(averaged, strict=False)
        assert not unexpected and averaged and not set(missing) & set(averaged)
        want = twin.generate(ids, **kw)
        twin.reset_decode_sessions()
        assert inside.shape == want.shape and torch.equal(inside, want), (inside.tolist(), want.tolist())
        assert torch.equal(again, outside) and not sess.stale()
        assert not torch.equal(inside, outside), "the averaged weights decode the same tokens as the last iterate: the comparison shows nothing"
    finally:
        model.reset_decode_sessions()
