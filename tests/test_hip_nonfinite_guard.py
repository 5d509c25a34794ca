"""Skipping non-finite steps on the device (FusedAdamW(skip_nonfinite=True); ff_grad_guard, ff_adamw_step_guarded): the guard kernel against
its formula, a skipped step as a bit-for-bit no-op in every storage mode and through both gradient paths, captured replays, whole-model
graphed steps through a poisoned batch, two ranks skipping together, and torch.amp.GradScaler handing found_inf / the scale over on the
device."""
import math
import os
import socket
import sys

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from util import ADAMW_C_PARITY, adamw_state, adamw_step_ok, as64, dev, rel, rnd

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# the scalar path (1, 3), a ragged tail (513 x 7, 8191), more than two 32768-element chunks (70001); the one-element tensor is not the first,
# so that "element 0 of the first tensor" and "the only element of (1,)" are two places
SHAPES = [(3,), (1,), (513, 7), (8191,), (70001,)]
MANY = [(37 * i + 5,) for i in range(45)]               # 45 tensors: the 32-entry pointer table is refilled
HP = dict(lr=3e-3, betas=(0.9, 0.95), eps=1e-8, weight_decay=0.05)
C_CLIP = 50.0                                           # below the norm of every gradient set here (>= 90): the clipped arms really clip
POISONS = {"nan": float("nan"), "+inf": float("inf"), "-inf": float("-inf")}
# place: (tensor list, tensor index, flat element index)
PLACES = {"first-0": (SHAPES, 0, 0), "70001-last": (SHAPES, 4, 70000), "70001-chunk2": (SHAPES, 4, 40000), "single": (SHAPES, 1, 0),
          "many-40": (MANY, 40, 7)}


# ---------------------------------------------------------------------------------------------------------------- 1. the guard kernel
def _guard_formula(s, max_norm, found, scale):
    """ff_grad_guard's formula in numpy float32, every operation rounded once: (norm, coef, bad)"""
    f = np.float32
    with np.errstate(all="ignore"):
        inv = f(1) / f(scale) if scale is not None else f(1)
        nrm = f(np.sqrt(np.float64(s))) * inv if s is not None else f(0) * inv
        bad = (s is not None and not np.isfinite(s)) or bool(found) or not np.isfinite(inv)
        c = min(f(1), f(max_norm) / (nrm + f(1e-6))) if max_norm > 0 else f(1)
        coef = f(0) if bad else inv * c
    return f(nrm), f(coef), bad


def _same(a, b):
    return np.array_equal(np.float32(a), np.float32(b), equal_nan=True)


@pytest.mark.parametrize("s", [4.0, 1e-30, 4.0 * 1024.0 ** 2, float("inf"), float("nan"), None], ids=["4", "1e-30", "2048^2", "inf", "nan", "no-sum"])
def test_guard_kernel_follows_its_formula(s):
    from flamingo_mini_amd import ffi
    lib = ffi.lib()
    stream = ffi.stream_handle(torch.device("cuda", 0))
    total = torch.zeros((), dtype=torch.int64, device="cuda")
    expected_total = 0
    sum_t = None if s is None else torch.full((), s, dtype=torch.float64, device="cuda")
    for max_norm in (0.0, 1.0):
        for found in (None, 0.0, 1.0):
            if s is None and found is None:
                continue                                # (refused before a launch: tests/test_nonfinite_guard_args.py)
            for scale in (None, 1024.0, 0.0):
                out = torch.full((4,), -7.0, device="cuda")                     # norm, coef, skip, take
                found_t = None if found is None else torch.full((1,), found, device="cuda")
                scale_t = None if scale is None else torch.full((), scale, device="cuda")
                ffi.check(lib.ff_grad_guard(ffi.ptr(sum_t), max_norm, ffi.ptr(found_t), ffi.ptr(scale_t), out[0:].data_ptr(), out[1:].data_ptr(),
                                            out[2:].data_ptr(), out[3:].data_ptr(), total.data_ptr(), stream), "ff_grad_guard")
                norm, coef, skip, take = out.cpu().numpy()
                e_norm, e_coef, bad = _guard_formula(s, max_norm, found, scale)
                what = (s, max_norm, found, scale)
                expected_total += int(bad)
                assert skip == (1.0 if bad else 0.0) and take == 1.0 - skip, what
                assert _same(norm, e_norm) and _same(coef, e_coef), (what, norm, e_norm, coef, e_coef)
                if s is not None and not math.isfinite(s):
                    assert skip == 1.0 and coef == 0.0 and take == 0.0 and not math.isfinite(norm), what
                    if scale is None:
                        assert _same(norm, np.float32(np.sqrt(np.float64(s)))), what            # the non-finite value as it is
                if scale == 0.0:
                    assert skip == 1.0, what
                if s is not None and math.isfinite(s) and found is None and scale is None:
                    ref = torch.full((2,), -7.0, device="cuda")                 # ff_grad_clip_coef: bit for bit
                    ffi.check(lib.ff_grad_clip_coef(sum_t.data_ptr(), max_norm or 1.0, ref[0:].data_ptr(), ref[1:].data_ptr(), stream), "coef")
                    assert torch.equal(out[0].view(torch.int32), ref[0].view(torch.int32)), what
                    if max_norm > 0:
                        assert torch.equal(out[1].view(torch.int32), ref[1].view(torch.int32)), what
                    else:
                        assert coef == 1.0, what
                # the optional outputs may be left out
                few = torch.full((2,), -7.0, device="cuda")
                ffi.check(lib.ff_grad_guard(ffi.ptr(sum_t), max_norm, ffi.ptr(found_t), ffi.ptr(scale_t), None, few[0:].data_ptr(), few[1:].data_ptr(),
                                            None, None, stream), "ff_grad_guard")
                assert torch.equal(few.view(torch.int32), out[1:3].view(torch.int32)), what
    assert int(total) == expected_total > 0           # the running total accumulates over the calls


# ---------------------------------------------------------------------------------------------------------------- 2. a skipped step is a no-op
MODES = {"f32": (torch.float32, {}), "bf16": (torch.bfloat16, {}), "bf16-state32": (torch.bfloat16, dict(state_dtype=torch.float32)),
         "bf16-master": (torch.bfloat16, dict(master_dtype=torch.float32))}


def _grads(shapes, k, dtype):
    return [dev(rnd(s, 100 * k + i, 0.5), dtype) for i, s in enumerate(shapes)]


def _feed(opt, params, gs, path, poisoned=None):
    """Hand the gradients `gs` to the optimizer: as `.grad`, or as two accumulate(0.5) folds of the same tensors (0.5 g + 0.5 g = g exactly
    in fp32, so both paths step on the same values).  poisoned: the tensors of the SECOND fold (the poison arrives in a later micro-batch)."""
    if path == "grad":
        for p, g in zip(params, poisoned or gs):
            p.grad = g
        return
    for fold in (gs, poisoned or gs):
        for p, g in zip(params, fold):
            p.grad = g
        opt.accumulate(0.5)


def _snapshot(opt, params):
    out = []
    for p in params:
        st = opt.state[p]
        out.append({k: t.clone() for k, t in (("p", p.detach()), ("exp_avg", st["exp_avg"]), ("exp_avg_sq", st["exp_avg_sq"]),
                                              ("master", st.get("master"))) if t is not None})
    return out


def _step_counter(opt):
    (counter,) = opt.param_groups[0]["_step_dev"].values()
    return counter


@pytest.mark.parametrize("place", list(PLACES))
@pytest.mark.parametrize("poison", list(POISONS))
@pytest.mark.parametrize("path", ["grad", "accumulate"])
@pytest.mark.parametrize("clip", [None, C_CLIP], ids=["unclipped", "clipped"])
@pytest.mark.parametrize("mode", list(MODES))
def test_skipped_step_is_a_noop_and_training_continues_as_if_it_had_not_happened(mode, clip, path, poison, place):
    from flamingo_mini_amd import FusedAdamW
    dtype, kw = MODES[mode]
    shapes, ti, ei = PLACES[place]
    kw = dict(capturable=True, max_grad_norm=clip, **kw, **HP)

    def make(**extra):
        ps = [torch.nn.Parameter(dev(rnd(s, 10 + i), dtype)) for i, s in enumerate(shapes)]
        return ps, FusedAdamW(ps, **kw, **extra)

    ours, opt = make(skip_nonfinite=True)
    twin, opt_t = make(skip_nonfinite=True)
    clean = [_grads(shapes, 1, dtype), _grads(shapes, 2, dtype)]
    bad = [g.clone() for g in _grads(shapes, 3, dtype)]
    bad[ti].view(-1)[ei] = POISONS[poison]
    bad_bits = [g.clone() for g in bad]

    def clean_step(t):
        gs = clean[t - 1]
        norm = float(np.sqrt(sum(float(np.sum(as64(g) ** 2)) for g in gs)))
        coef = min(1.0, clip / (norm + 1e-6)) if clip else 1.0
        assert not clip or coef < 1.0
        before = [adamw_state(opt, p) for p in ours]
        _feed(opt, ours, gs, path)
        opt.step()
        for i, p in enumerate(ours):                    # this step alone, element by element, with the bias corrections of step t
            new, storages = adamw_state(opt, p)
            ok, what = adamw_step_ok(before[i][0], new, gs[i], storages, t, HP["lr"], 0.9, 0.95, 1e-8, 0.05, coef=coef, c=ADAMW_C_PARITY)
            assert ok, (t, shapes[i], what)
            if "master" in opt.state[p]:
                assert torch.equal(p.detach(), opt.state[p]["master"].to(torch.bfloat16)), (t, shapes[i])
        assert float(opt.step_skipped) == 0.0 and float(_step_counter(opt)) == t
        assert abs(float(opt.grad_norm) - norm) <= 1e-5 * norm, (float(opt.grad_norm), norm)

    clean_step(1)
    snap, counter = _snapshot(opt, ours), _step_counter(opt).clone()
    _feed(opt, ours, _grads(shapes, 3, dtype), path, poisoned=bad)
    opt.step()
    assert float(opt.step_skipped) == 1.0 and not math.isfinite(float(opt.grad_norm))
    assert torch.equal(_step_counter(opt), counter)
    for i, (p, old) in enumerate(zip(ours, _snapshot(opt, ours))):
        for k, t in snap[i].items():
            assert torch.equal(old[k].view(torch.uint8), t.view(torch.uint8)), (shapes[i], k)
    for g, bits in zip(bad, bad_bits):                  # the poisoned gradients are as they were
        assert torch.equal(g.view(torch.uint8), bits.view(torch.uint8))
    if path == "grad":
        assert all(p.grad is g for p, g in zip(ours, bad))
    else:
        assert all(p.grad is None and opt.accumulated_grad(p) is None for p in ours)       # the cycle is closed after a skipped step too
    clean_step(2)

    for t in (1, 2):                                    # the twin never saw the poisoned step
        _feed(opt_t, twin, clean[t - 1], path)
        opt_t.step()
    for i, (a, b) in enumerate(zip(_snapshot(opt, ours), _snapshot(opt_t, twin))):
        assert a.keys() == b.keys()
        for k in a:
            assert torch.equal(a[k].view(torch.uint8), b[k].view(torch.uint8)), (shapes[i], k)
    assert torch.equal(_step_counter(opt), _step_counter(opt_t))
    sd = opt.state_dict()["state"]
    assert len(sd) == len(shapes) and all(float(sd[i]["step"]) == 2.0 for i in range(len(shapes)))
    assert int(opt.skipped_steps) == 1 and int(opt_t.skipped_steps) == 0

    # control: without the guard the same poisoned step reaches the parameters
    ctrl, opt_c = make()
    _feed(opt_c, ctrl, clean[0], path)
    opt_c.step()
    _feed(opt_c, ctrl, _grads(shapes, 3, dtype), path, poisoned=bad)
    opt_c.step()
    assert opt_c.step_skipped is None
    assert not all(bool(torch.isfinite(p).all()) for p in ctrl)


# ---------------------------------------------------------------------------------------------------------------- 3. graph replay
def test_guarded_step_graph_replay_equals_eager_steps():
    """capturable: a captured guarded, clipped step replayed over clean and poisoned gradients (new values copied into the same .grad storage,
    a new learning rate every step) equals the same sequence run eagerly, bit for bit, and the reported scalars keep their storage."""
    from flamingo_mini_amd import FusedAdamW
    shapes = [(130,), (33, 40), (8191,)]
    poisoned = [None, float("nan"), None, float("inf"), float("-inf"), None]
    lrs = [1e-2, 5e-3, 2e-2, 1e-3, 7e-3, 3e-3]

    def grads(k):
        gs = [dev(rnd(s, 70 * k + i, 0.3)) for i, s in enumerate(shapes)]
        if poisoned[k] is not None:
            gs[k % 3].view(-1)[11 * k] = poisoned[k]
        return gs

    def make():
        ps = [torch.nn.Parameter(dev(rnd(s, 10 + i))) for i, s in enumerate(shapes)]
        for p, g in zip(ps, grads(0)):
            p.grad = g
        return ps

    p_e, p_g = make(), make()
    o_e = FusedAdamW(p_e, lr=lrs[0], capturable=True, max_grad_norm=2.0, skip_nonfinite=True)
    o_g = FusedAdamW(p_g, lr=lrs[0], capturable=True, max_grad_norm=2.0, skip_nonfinite=True)
    norms_e, skips_e = [], []
    for k, lr in enumerate(lrs):
        for p, g in zip(p_e, grads(k)):
            p.grad.copy_(g)
        o_e.param_groups[0]["lr"] = lr
        o_e.step()
        norms_e.append(o_e.grad_norm.clone())
        skips_e.append(float(o_e.step_skipped))
    assert skips_e == [0.0 if v is None else 1.0 for v in poisoned]
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        o_g.step()                                    # step 1 eagerly (allocates the guard's buffers)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    storage = [t.data_ptr() for t in (o_g.skipped_steps, o_g.step_skipped, o_g.grad_norm)]
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        o_g.step()
    for k, lr in enumerate(lrs[1:], start=1):
        for p, g in zip(p_g, grads(k)):
            p.grad.copy_(g)
        o_g.param_groups[0]["lr"] = lr
        o_g.sync_device_hyperparams()
        graph.replay()
        assert torch.equal(o_g.grad_norm.view(torch.int32), norms_e[k].view(torch.int32)), k
        assert float(o_g.step_skipped) == skips_e[k], k
        assert [t.data_ptr() for t in (o_g.skipped_steps, o_g.step_skipped, o_g.grad_norm)] == storage
    torch.cuda.synchronize()
    assert int(o_g.skipped_steps) == 3 and int(o_e.skipped_steps) == 3
    assert float(norms_e[0]) > 2.0                    # the coefficient is < 1 in the clean steps
    for a, b in zip(p_e, p_g):
        assert torch.equal(a, b) and bool(torch.isfinite(a).all())
        assert torch.equal(o_e.state[a]["exp_avg"], o_g.state[b]["exp_avg"])
        assert torch.equal(o_e.state[a]["exp_avg_sq"], o_g.state[b]["exp_avg_sq"])
    assert torch.equal(_step_counter(o_e), _step_counter(o_g)) and float(_step_counter(o_g)) == 3.0


# ---------------------------------------------------------------------------------------------------------------- 4. whole model
def _paths():
    for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tests", "golden")):
        if p not in sys.path:
            sys.path.insert(0, p)


def _h64(dtype):
    _paths()
    from test_model_plumbing import H64, build_h64
    model, _, batch = build_h64(dtype, "cuda")
    return model, batch, dict(H64["adamw"])


_NORMS = {}


def _first_norm(dtype):
    """float64 norm of the h64 fixture's first-step gradients (computed once per dtype): max_grad_norm is set below it, so every step clips"""
    if dtype not in _NORMS:
        model, batch, _ = _h64(dtype)
        model(**batch).loss.backward()
        _NORMS[dtype] = float(np.sqrt(sum(float(np.sum(as64(p.grad) ** 2)) for p in model.parameters_trainable() if p.grad is not None)))
    return _NORMS[dtype]


def _poisoned(batch, sample):
    out = dict(batch)
    px = batch["pixel_values"].clone()
    px[sample].view(-1)[1234] = float("inf")
    out["pixel_values"] = px
    return out


@pytest.mark.parametrize("kind,dtype", [("graphed", torch.float32), ("graphed", torch.bfloat16), ("piecewise", torch.float32), ("micro", torch.float32)],
                         ids=["graphed-f32", "graphed-bf16", "piecewise-f32", "micro2-f32"])
def test_graphed_training_steps_through_a_poisoned_batch(kind, dtype):
    """Run A: warm-up step on the clean batch, a replay on a batch with one +inf pixel (sample 0; micro: sample 2, so that only the second
    micro-batch is poisoned), a replay on the clean batch.  Run B: the same without the poisoned replay.  A skipped it and is where B is."""
    from flamingo_mini_amd import FusedAdamW, GraphedTrainStep
    from flamingo_mini_amd import functional as F
    from flamingo_mini_amd.graphs import PiecewiseGraphedTrainStep
    c = 0.25 * _first_norm(dtype)

    def run(poison):
        model, batch, adamw = _h64(dtype)
        opt = FusedAdamW(list(model.parameters_trainable()), capturable=True, skip_nonfinite=True, max_grad_norm=c, **adamw)
        if kind == "piecewise":
            step = PiecewiseGraphedTrainStep(model, opt, batch, warmup=1, segment_layers=1, overlap_optimizer=False)
        else:
            step = GraphedTrainStep(model, opt, batch, warmup=1, micro_batches=2 if kind == "micro" else 1)      # (the warm-up is training step 1)
        assert float(opt.grad_norm) > c and int(opt.skipped_steps) == 0
        bad_loss = None
        if poison:
            assert batch["pixel_values"].shape[0] == 4
            bad_loss = float(step(_poisoned(batch, 2 if kind == "micro" else 0)))
            assert float(opt.step_skipped) == 1.0 and not math.isfinite(float(opt.grad_norm))
        step(batch)
        torch.cuda.synchronize()
        step.close()
        assert float(opt.step_skipped) == 0.0
        assert {float(s["step"]) for s in opt.state_dict()["state"].values()} == {2.0}
        return model, opt, bad_loss

    model_a, opt_a, bad_loss = run(True)
    model_b, opt_b, _ = run(False)
    assert not math.isfinite(bad_loss)                  # the replay returns the loss of the step it skipped
    assert int(opt_a.skipped_steps) == 1 and int(opt_b.skipped_steps) == 0
    tol = 1e-4 if dtype == torch.float32 else 3e-2
    for (k, p), (_, q) in zip(model_a.named_parameters(), model_b.named_parameters()):
        if p.requires_grad:
            assert bool(torch.isfinite(p).all()), k
            assert rel(p, q) < tol, k
    assert F.sync_exchange_status() == 0


# ---------------------------------------------------------------------------------------------------------------- 5. two ranks
def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _worker(rank, world, port, out_dir, c):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from flamingo_mini_amd import FusedAdamW
    from flamingo_mini_amd.data_parallel import GradientAllReducer
    model, batch, adamw = _h64(torch.float32)
    per = batch["input_ids"].shape[0] // world
    mine = {k: v[rank * per:(rank + 1) * per].contiguous() for k, v in batch.items()}
    reducer = GradientAllReducer(model)
    opt = FusedAdamW(list(model.parameters_trainable()), capturable=True, skip_nonfinite=True, max_grad_norm=c, **adamw)
    skipped = []
    for step in range(3):
        feed = _poisoned(mine, 0) if (step == 1 and rank == 1) else mine          # step 2: only rank 1's half is poisoned
        model.zero_grad(set_to_none=True)
        model(**feed).loss.backward()
        reducer.finish()
        opt.step()
        skipped.append(float(opt.step_skipped))
    torch.cuda.synchronize()
    reducer.close()
    np.savez(os.path.join(out_dir, f"rank{rank}.npz"), skipped=np.array(skipped), skipped_steps=np.array([int(opt.skipped_steps)]),
             **{k: p.detach().float().cpu().numpy() for k, p in model.named_parameters() if p.requires_grad})
    dist.barrier()
    dist.destroy_process_group()


def test_two_ranks_skip_together():
    """Two processes sharing the GPU through gloo, each on half of the batch; in step 2 only rank 1's half is poisoned.  The averaged
    gradients are non-finite on both ranks, so both skip that step with no extra exchange, and both end where one process ends that took
    the two clean steps on the whole batch."""
    import tempfile
    from flamingo_mini_amd import FusedAdamW
    c = 0.25 * _first_norm(torch.float32)
    with tempfile.TemporaryDirectory() as tmp:
        mp.start_processes(_worker, args=(2, _free_port(), tmp, c), nprocs=2, join=True, start_method="spawn")
        r0, r1 = dict(np.load(os.path.join(tmp, "rank0.npz"))), dict(np.load(os.path.join(tmp, "rank1.npz")))
    assert list(r0["skipped"]) == [0.0, 1.0, 0.0] and list(r1["skipped"]) == [0.0, 1.0, 0.0]
    assert int(r0["skipped_steps"][0]) == 1 and int(r1["skipped_steps"][0]) == 1
    model, batch, adamw = _h64(torch.float32)
    opt = FusedAdamW(list(model.parameters_trainable()), capturable=True, skip_nonfinite=True, max_grad_norm=c, **adamw)
    for _ in range(2):
        model.zero_grad(set_to_none=True)
        model(**batch).loss.backward()
        opt.step()
    torch.cuda.synchronize()
    assert float(opt.grad_norm) > c and int(opt.skipped_steps) == 0
    for k, p in model.named_parameters():
        if p.requires_grad:
            assert np.array_equal(r0[k], r1[k]), k
            assert rel(torch.from_numpy(r0[k]), p.detach().float().cpu()) < 1e-4, k


# ---------------------------------------------------------------------------------------------------------------- 6. torch.amp.GradScaler
@pytest.mark.parametrize("clip", [None, C_CLIP], ids=["unclipped", "clipped"])
def test_grad_scaler_hands_found_inf_and_scale_over_on_the_device(clip):
    """scaler.step(FusedAdamW(capturable=True)) against scaler.step(torch.optim.AdamW(fused=True)) (clipped: scaler.unscale_ +
    torch.nn.utils.clip_grad_norm_ there, max_grad_norm here): five steps, the data of step 3 holds an inf.  Same scale after every
    update(), same parameters, step 3 changes nothing on either side, and our .grad still holds the SCALED gradients after the step."""
    from flamingo_mini_amd import FusedAdamW
    ours = [torch.nn.Parameter(dev(rnd(s, 10 + i))) for i, s in enumerate(SHAPES)]
    theirs = [torch.nn.Parameter(p.detach().clone()) for p in ours]
    opt_a = FusedAdamW(ours, capturable=True, max_grad_norm=clip, **HP)
    opt_b = torch.optim.AdamW(theirs, fused=True, **HP)
    assert opt_a._step_supports_amp_scaling is True
    sc_a = torch.amp.GradScaler("cuda", init_scale=1024.0, growth_interval=2)
    sc_b = torch.amp.GradScaler("cuda", init_scale=1024.0, growth_interval=2)
    scales = []
    for step in range(1, 6):
        xs = [dev(rnd(s, 100 * step + i, 0.5)) for i, s in enumerate(SHAPES)]
        if step == 3:
            xs[4].view(-1)[40000] = float("inf")
        before_a, before_b = [p.detach().clone() for p in ours], [p.detach().clone() for p in theirs]
        for params, opt, sc in ((ours, opt_a, sc_a), (theirs, opt_b, sc_b)):
            opt.zero_grad(set_to_none=True)
            loss = sum((p * x).sum() for p, x in zip(params, xs))
            sc.scale(loss).backward()
        scale = sc_a.get_scale()
        scaled = [p.grad.clone() for p in ours]
        sc_a.step(opt_a)
        if clip:
            sc_b.unscale_(opt_b)
            torch.nn.utils.clip_grad_norm_(theirs, clip)
        sc_b.step(opt_b)
        sc_a.update()
        sc_b.update()
        scales.append(sc_a.get_scale())
        assert sc_a.get_scale() == sc_b.get_scale(), step
        assert not hasattr(opt_a, "found_inf") and not hasattr(opt_a, "grad_scale")        # GradScaler took its attributes back
        for p, g, x in zip(ours, scaled, xs):           # no in-place unscale pass ran over our gradients
            assert torch.equal(p.grad.view(torch.int32), g.view(torch.int32)), step
            assert torch.equal(g.view(torch.int32), (x * scale).view(torch.int32)), step
        assert float(opt_a.step_skipped) == (1.0 if step == 3 else 0.0)
        if clip and step != 3:                          # the norm of the UNSCALED gradients
            norm = float(np.sqrt(sum(float(np.sum(as64(x) ** 2)) for x in xs)))
            assert norm > clip and abs(float(opt_a.grad_norm) - norm) <= 1e-5 * norm, (float(opt_a.grad_norm), norm)
        for i, (a, b) in enumerate(zip(ours, theirs)):
            if step == 3:
                assert torch.equal(a, before_a[i]) and torch.equal(b, before_b[i]), SHAPES[i]
            else:
                assert not torch.equal(a, before_a[i])
            assert rel(a, b) < 1e-6, (step, SHAPES[i])
    assert scales == [1024.0, 2048.0, 1024.0, 1024.0, 2048.0]
    assert int(opt_a.skipped_steps) == 1 and float(_step_counter(opt_a)) == 4.0
    assert clip or opt_a.grad_norm is None            # no sweep ran: there is no norm to report
    # an open accumulate() cycle cannot be combined with a scaler's attributes
    for p in ours:
        p.grad = torch.zeros_like(p)
    opt_a.accumulate(1.0)
    opt_a.found_inf, opt_a.grad_scale = torch.zeros(1, device="cuda"), torch.ones((), device="cuda")
    with pytest.raises(ValueError, match="accumulate"):
        opt_a.step()
