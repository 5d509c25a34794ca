"""Gradient clipping by global L2 norm (max_grad_norm; the reference's HF Trainer clips to 1.0 before every step) on the HIP kernels:
the sum-of-squares kernels against float64, FusedAdamW(max_grad_norm) against the float64 AdamW oracle and against torch's
clip_grad_norm_ + AdamW, captured replays, whole-model training steps (graphed, piecewise), the functional clip_grad_norm_, and
ShardedAdamW(max_grad_norm) / GradientAllReducer + FusedAdamW(max_grad_norm) on one and on two ranks."""
import ctypes as C
import os
import socket
import sys

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from oracle import flamingo_oracle as O
from util import ADAMW_C_PARITY, adamw_state, adamw_step_ok, as64, dev, rel, rnd

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(1,), (3,), (513, 7), (8191,), (5120, 1280)]
HP = dict(lr=3e-3, betas=(0.9, 0.95), eps=1e-8, weight_decay=0.05)


def _norm_on_device(grads):
    """ff_grad_sumsq over the list (one launch table per dtype, slots continuing), ff_grad_sumsq_reduce, ff_grad_clip_coef."""
    from flamingo_mini_amd import ffi
    lib = ffi.lib()
    stream = ffi.stream_handle(grads[0].device)
    tables = []
    for dt in (torch.float32, torch.bfloat16):
        gs = [g for g in grads if g.dtype == dt]
        if gs:
            n = (C.c_longlong * len(gs))(*[g.numel() for g in gs])
            tables.append((ffi.dtype_code(dt), gs, n, lib.ff_grad_sumsq_partials(len(gs), n)))
    total = sum(t[3] for t in tables)
    partials = torch.full((total + 1,), float("nan"), device="cuda")      # one slot beyond the last must stay untouched
    s = torch.empty((), dtype=torch.float64, device="cuda")
    norm, coef = torch.empty((), device="cuda"), torch.empty((), device="cuda")
    off = 0
    for code, gs, n, k in tables:
        ffi.check(lib.ff_grad_sumsq(code, len(gs), ffi.ptr_array(gs), n, 1.0, partials.data_ptr() + 4 * off, total - off, stream), "sumsq")
        off += k
    ffi.check(lib.ff_grad_sumsq_reduce(partials.data_ptr(), total, s.data_ptr(), 0, stream), "reduce")
    ffi.check(lib.ff_grad_clip_coef(s.data_ptr(), 1.0, norm.data_ptr(), coef.data_ptr(), stream), "coef")
    torch.cuda.synchronize()
    assert torch.isnan(partials[total]) and not torch.isnan(partials[:total]).any()
    return float(s), float(norm), float(coef)


def _ref_sumsq(grads):
    return sum(float(np.sum(as64(g) ** 2)) for g in grads)


@pytest.mark.parametrize("kind", ["f32", "bf16", "mixed", "many", "unaligned"])
def test_sumsq_kernel_matches_float64(kind):
    if kind == "many":          # > 32 tensors: the pointer table is refilled, the slots continue
        grads = [dev(rnd((37 * i + 5,), 300 + i), torch.bfloat16 if i % 3 else torch.float32) for i in range(45)]
    elif kind == "unaligned":   # views off the 16-byte grid and odd sizes: the element-wise path
        base = dev(rnd((70001,), 7))
        grads = [base[1:], base[3:40003], dev(rnd((9001,), 8), torch.bfloat16)[1:]]
    else:
        dts = {"f32": [torch.float32], "bf16": [torch.bfloat16], "mixed": [torch.float32, torch.bfloat16]}[kind]
        grads = [dev(rnd(s, 10 + i), dts[i % len(dts)]) for i, s in enumerate(SHAPES)]
    ref = _ref_sumsq(grads)
    s1, norm, coef = _norm_on_device(grads)
    s2, _, _ = _norm_on_device(grads)
    assert abs(s1 - ref) <= 1e-5 * ref, (s1, ref)
    assert abs(norm - np.sqrt(ref)) <= 1e-5 * np.sqrt(ref)
    assert abs(coef - min(1.0, 1.0 / (norm + 1e-6))) <= 1e-6
    assert s1 == s2                                      # fixed slots, fixed order: bit for bit


def test_sumsq_kernel_on_an_embedding_sized_tensor():
    """64 M bf16 elements (the token embedding at config B, 128 MiB): one launch of 2048 workgroups, every slot covered; exact values, exact
    sum.  (Tensors of more than 2^31 elements take the same 64-bit element offsets; their slot count is checked on the host.)"""
    n = 64 * 1024 * 1024
    g = ((torch.arange(n, device="cuda") % 7) - 3).to(torch.bfloat16) * 0.25
    per = np.array([((k % 7) - 3) * 0.25 for k in range(7)]) ** 2
    counts = np.bincount(np.arange(7), minlength=7) * (n // 7) + (np.arange(7) < n % 7)
    ref = float(np.dot(per, counts))
    s, _, _ = _norm_on_device([g])
    assert s == ref, (s, ref)


def _clip64(grads, c):
    norm = np.sqrt(sum(float(np.sum(g ** 2)) for g in grads))
    return [g * min(1.0, c / (norm + 1e-6)) for g in grads], norm


@pytest.mark.parametrize("c", [100.0, 1e5], ids=["clips", "above"])
@pytest.mark.parametrize("mode", ["f32", "bf16", "bf16-master"])
def test_fused_adamw_clipped_matches_oracle_and_torch(mode, c):
    from flamingo_mini_amd import FusedAdamW
    dtype = torch.float32 if mode == "f32" else torch.bfloat16
    master = mode == "bf16-master"
    ours = [torch.nn.Parameter(dev(rnd(s, 10 + i), dtype)) for i, s in enumerate(SHAPES)]
    theirs = [torch.nn.Parameter(p.detach().clone()) for p in ours]
    ref = [(as64(p), np.zeros(p.shape), np.zeros(p.shape)) for p in ours]
    opt_a = FusedAdamW(ours, max_grad_norm=c, master_dtype=torch.float32 if master else None, **HP)
    opt_b = torch.optim.AdamW(theirs, fused=True, **HP)
    norms = []
    for step in range(1, 5):
        gs = [dev(rnd(a.shape, 100 * step + i, 0.5), dtype) for i, a in enumerate(ours)]
        g64, norm = _clip64([as64(g) for g in gs], c)
        norms.append(norm)
        for i, (a, b) in enumerate(zip(ours, theirs)):
            a.grad, b.grad = gs[i], gs[i].clone()
            p64, m64, v64 = ref[i]
            ref[i] = O.adamw_step(p64, g64[i], m64, v64, step, lr=HP["lr"], beta1=0.9, beta2=0.95, eps=1e-8, weight_decay=0.05)
            if master:            # fp32 master copy and fp32 moments
                ref[i] = tuple(as64(torch.as_tensor(t).to(torch.float32)) for t in ref[i])
            elif dtype == torch.bfloat16:
                ref[i] = tuple(as64(torch.as_tensor(t).to(torch.bfloat16)) for t in ref[i])
        before = [adamw_state(opt_a, a) for a in ours]
        opt_a.step()
        torch.nn.utils.clip_grad_norm_(theirs, c)
        opt_b.step()
        for i, a in enumerate(ours):        # this step alone, element by element, from the state the kernel had stored (util.adamw_bound_ok)
            new, storages = adamw_state(opt_a, a)       # (the fp32 master copy and fp32 moments exist from the first step on)
            ok, bad = adamw_step_ok(before[i][0], new, gs[i], storages, step, HP["lr"], 0.9, 0.95, 1e-8, 0.05, coef=min(1.0, c / (norm + 1e-6)),
                                    c=ADAMW_C_PARITY)
            assert ok, (step, SHAPES[i], bad)
            if master:
                assert torch.equal(a.detach(), new[0].to(torch.bfloat16)), (step, SHAPES[i])
        assert abs(float(opt_a.grad_norm) - norm) <= 1e-5 * norm, (float(opt_a.grad_norm), norm)
    assert c < min(norms) or c > max(norms)
    tol = 1e-6 if mode == "f32" else 1e-2
    for i, (a, b) in enumerate(zip(ours, theirs)):
        st = opt_a.state[a]
        assert rel(st["master"] if master else a, ref[i][0]) < (1e-6 if master else tol), SHAPES[i]
        assert rel(st["exp_avg"], ref[i][1]) < (1e-6 if master else tol) and rel(st["exp_avg_sq"], ref[i][2]) < (1e-6 if master else tol)
        if master:
            assert rel(a, ref[i][0]) < 1e-2
        assert rel(a, b) < 1e-2, SHAPES[i]                    # torch's clip_grad_norm_ + AdamW
    assert torch.equal(ours[-1].grad, dev(rnd(SHAPES[-1], 404, 0.5), dtype))      # .grad is left unscaled


@pytest.mark.parametrize("mode", ["f32", "bf16", "bf16-master"])
def test_huge_max_grad_norm_is_the_unclipped_step(mode):
    from flamingo_mini_amd import FusedAdamW
    dtype = torch.float32 if mode == "f32" else torch.bfloat16
    kw = dict(master_dtype=torch.float32 if mode == "bf16-master" else None, **HP)
    a = [torch.nn.Parameter(dev(rnd(s, 10 + i), dtype)) for i, s in enumerate(SHAPES)]
    b = [torch.nn.Parameter(p.detach().clone()) for p in a]
    oa, ob = FusedAdamW(a, max_grad_norm=1e9, **kw), FusedAdamW(b, **kw)
    for step in range(3):
        for i, (x, y) in enumerate(zip(a, b)):
            x.grad = dev(rnd(x.shape, 50 * step + i, 0.5), dtype)
            y.grad = x.grad.clone()
        oa.step()
        ob.step()
    for x, y in zip(a, b):
        assert torch.equal(x, y)
        for k in oa.state[x]:
            if mode == "f32":
                assert torch.equal(oa.state[x][k], ob.state[y][k]), k
            else:     # (the bf16 kernels with the coefficient contract the moments' multiply-adds differently: last-bit differences,
                      # which bf16 moments round to an occasional one-ulp flip, 2^-8)
                assert rel(oa.state[x][k], ob.state[y][k]) < (1e-5 if oa.state[x][k].dtype == torch.float32 else 2.0 ** -8), k


def test_clipped_step_graph_replay_equals_eager_steps():
    """capturable: a captured clipped step replayed n times equals n eager steps bit for bit, grad_norm follows every replay (new gradient
    values copied into the same .grad storage), and a learning-rate schedule stays effective."""
    from flamingo_mini_amd import FusedAdamW
    shapes = [(130,), (33, 40), (8191,)]
    lrs = [1e-2, 5e-3, 2e-2, 1e-3]

    def grads(k):
        return [dev(rnd(s, 70 * k + i, 0.3)) for i, s in enumerate(shapes)]

    def make():
        ps = [torch.nn.Parameter(dev(rnd(s, 10 + i))) for i, s in enumerate(shapes)]
        for p, g in zip(ps, grads(0)):
            p.grad = g
        return ps

    p_e, p_g = make(), make()
    o_e = FusedAdamW(p_e, lr=lrs[0], capturable=True, max_grad_norm=2.0)
    o_g = FusedAdamW(p_g, lr=lrs[0], capturable=True, max_grad_norm=2.0)
    norms_e = []
    for k, lr in enumerate(lrs):
        for p, g in zip(p_e, grads(k)):
            p.grad.copy_(g)
        o_e.param_groups[0]["lr"] = lr
        o_e.step()
        norms_e.append(o_e.grad_norm.clone())
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        o_g.step()                                    # step 1 eagerly (allocates the clipping buffers)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    norm_storage = o_g.grad_norm.data_ptr()
    assert torch.equal(o_g.grad_norm, norms_e[0])
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        o_g.step()
    for k, lr in enumerate(lrs[1:], start=1):
        for p, g in zip(p_g, grads(k)):
            p.grad.copy_(g)
        o_g.param_groups[0]["lr"] = lr
        o_g.sync_device_hyperparams()
        graph.replay()
        assert torch.equal(o_g.grad_norm, norms_e[k]), k
    torch.cuda.synchronize()
    assert o_g.grad_norm.data_ptr() == norm_storage
    assert float(norms_e[0]) > 2.0                    # the coefficient is < 1 in these steps
    for a, b in zip(p_e, p_g):
        assert torch.equal(a, b)
        assert torch.equal(o_e.state[a]["exp_avg"], o_g.state[b]["exp_avg"])


# ---------------------------------------------------------------------------------------------------------------- whole model
def _paths():
    for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tests", "golden")):
        if p not in sys.path:
            sys.path.insert(0, p)


def _h64(dtype):
    _paths()
    from test_model_plumbing import H64, build_h64
    model, _, batch = build_h64(dtype, "cuda")
    return model, batch, dict(H64["adamw"])


def _first_norm(dtype):
    """float64 norm of the h64 fixture's first-step gradients: max_grad_norm is set below it, so every step clips."""
    model, batch, _ = _h64(dtype)
    model(**batch).loss.backward()
    return float(np.sqrt(sum(float(np.sum(as64(p.grad) ** 2)) for p in model.parameters_trainable() if p.grad is not None)))


def _eager_torch_clip(model, batch, adamw, c, steps=3):
    """the reference recipe: backward, torch.nn.utils.clip_grad_norm_, then the (unclipped) fused AdamW"""
    from flamingo_mini_amd import FusedAdamW
    params = list(model.parameters_trainable())
    opt = FusedAdamW(params, **adamw)
    for _ in range(steps):
        model.zero_grad(set_to_none=True)
        model(**batch).loss.backward()
        torch.nn.utils.clip_grad_norm_([p for p in params if p.grad is not None], c)
        opt.step()
    torch.cuda.synchronize()


@pytest.mark.parametrize("kind,dtype", [("graphed", torch.float32), ("graphed", torch.bfloat16), ("piecewise", torch.float32)],
                         ids=["graphed-f32", "graphed-bf16", "piecewise-f32"])
def test_graphed_training_with_max_grad_norm_equals_eager_torch_clipping(kind, dtype):
    from flamingo_mini_amd import FusedAdamW, GraphedTrainStep
    from flamingo_mini_amd.graphs import PiecewiseGraphedTrainStep
    c = 0.25 * _first_norm(dtype)
    ref, batch, adamw = _h64(dtype)
    _eager_torch_clip(ref, batch, adamw, c)
    model, batch, _ = _h64(dtype)
    opt = FusedAdamW(list(model.parameters_trainable()), capturable=True, max_grad_norm=c, **adamw)
    if kind == "graphed":
        step = GraphedTrainStep(model, opt, batch, warmup=1)                     # (the constructor's warm-up is training step 1)
    else:
        step = PiecewiseGraphedTrainStep(model, opt, batch, warmup=1, segment_layers=1, overlap_optimizer=False)
    norms = [float(opt.grad_norm)]
    for _ in range(2):
        step()
        norms.append(float(opt.grad_norm))
    torch.cuda.synchronize()
    step.close()
    assert min(norms) > c, (norms, c)
    tol = 1e-4 if dtype == torch.float32 else 3e-2
    for (k, p), (_, q) in zip(model.named_parameters(), ref.named_parameters()):
        if p.requires_grad:
            assert rel(p, q) < tol, k


def test_functional_clip_grad_norm_matches_torch():
    from flamingo_mini_amd import clip_grad_norm_
    for dts in ([torch.float32], [torch.bfloat16], [torch.float32, torch.bfloat16]):
        for c in (10.0, 1e6):
            ours = [torch.nn.Parameter(dev(rnd(s, 10 + i), dts[i % len(dts)])) for i, s in enumerate(SHAPES)]
            theirs = [torch.nn.Parameter(p.detach().clone()) for p in ours]
            for i, (a, b) in enumerate(zip(ours, theirs)):
                a.grad = dev(rnd(a.shape, 60 + i, 0.5), a.dtype)
                b.grad = a.grad.clone()
            before = [p.grad.clone() for p in ours]
            ref = np.sqrt(_ref_sumsq(before))
            n_ours = clip_grad_norm_(ours, c)
            n_theirs = torch.nn.utils.clip_grad_norm_(theirs, c)
            assert n_ours.dtype == torch.float32 and n_ours.dim() == 0 and n_ours.is_cuda
            assert abs(float(n_ours) - ref) <= 1e-5 * ref
            f32 = dts == [torch.float32]
            assert abs(float(n_ours) - float(n_theirs)) <= (1e-6 if f32 else 1e-2) * ref
            for a, b, g in zip(ours, theirs, before):
                if c > ref:
                    assert torch.equal(a.grad, g)
                assert rel(a.grad, b.grad) < (1e-5 if a.dtype == torch.float32 else 1e-2)
    g = [torch.nn.Parameter(dev(rnd((100,), 1)))]
    g[0].grad = dev(rnd((100,), 2))
    g[0].grad[5] = float("inf")
    with pytest.raises(RuntimeError, match="non-finite"):
        clip_grad_norm_(g, 1.0, error_if_nonfinite=True)
    t = [torch.nn.Parameter(g[0].detach().clone())]
    t[0].grad = g[0].grad.clone()
    assert torch.isinf(clip_grad_norm_(g, 1.0)) and torch.isinf(torch.nn.utils.clip_grad_norm_(t, 1.0))
    assert torch.equal(torch.isnan(g[0].grad), torch.isnan(t[0].grad)) and torch.equal(g[0].grad.nan_to_num(), t[0].grad.nan_to_num())


# ---------------------------------------------------------------------------------------------------------------- data parallel
def _train_eager(model, batch, opt, steps=3, micro=1):
    for _ in range(steps):
        opt.zero_grad(set_to_none=True)
        for k in range(micro):
            part = {n: v[k::micro].contiguous() for n, v in batch.items()} if micro > 1 else batch
            ctx = opt.no_sync() if (hasattr(opt, "no_sync") and k < micro - 1) else _nullctx()
            with ctx:
                loss = model(**part).loss
                (loss / micro).backward()
        opt.step()
    torch.cuda.synchronize()


class _nullctx:
    def __enter__(self):
        return self

    def __exit__(self, *a):
        return False


@pytest.mark.parametrize("mode", ["eager", "capturable", "no_sync"])
def test_sharded_adamw_one_rank_equals_fused_adamw(mode):
    """World size 1 without collectives: eager steps, a captured step (GraphedTrainStep), and two accumulated micro-batches (no_sync: the
    buckets' pipelines run in step()) equal FusedAdamW(max_grad_norm) on the same model."""
    from flamingo_mini_amd import FusedAdamW, GraphedTrainStep
    from flamingo_mini_amd.data_parallel import ShardedAdamW
    c = 0.25 * _first_norm(torch.float32)
    ref, batch, adamw = _h64(torch.float32)
    o_ref = FusedAdamW(list(ref.parameters_trainable()), max_grad_norm=c, **adamw)
    _train_eager(ref, batch, o_ref, micro=2 if mode == "no_sync" else 1)
    model, _, _ = _h64(torch.float32)
    opt = ShardedAdamW(model, max_grad_norm=c, capturable=mode == "capturable", **adamw)
    try:
        assert not opt.collectives
        if mode == "capturable":
            step = GraphedTrainStep(model, opt, batch, warmup=1)
            for _ in range(2):
                step()
            torch.cuda.synchronize()
            step.close()
        else:
            _train_eager(model, batch, opt, micro=2 if mode == "no_sync" else 1)
    finally:
        opt.close()
    assert float(o_ref.grad_norm) > c
    assert abs(float(opt.grad_norm) - float(o_ref.grad_norm)) <= 1e-5 * float(o_ref.grad_norm), (float(opt.grad_norm), float(o_ref.grad_norm))
    for (k, p), (_, q) in zip(model.named_parameters(), ref.named_parameters()):
        if p.requires_grad:
            assert rel(p, q) < 1e-4, k


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _worker(rank, world, port, out_dir, kind, dtype_name, c):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from flamingo_mini_amd import FusedAdamW
    from flamingo_mini_amd.data_parallel import GradientAllReducer, ShardedAdamW
    model, batch, adamw = _h64(getattr(torch, dtype_name))
    per = batch["input_ids"].shape[0] // world
    mine = {k: v[rank * per:(rank + 1) * per].contiguous() for k, v in batch.items()}
    if kind == "sharded":
        opt = ShardedAdamW(model, max_grad_norm=c, **adamw)
        assert opt.collectives and not opt.cuda
        _train_eager(model, mine, opt)
        norm = opt.grad_norm
        opt.close()
    else:
        reducer = GradientAllReducer(model)
        opt = FusedAdamW(list(model.parameters_trainable()), max_grad_norm=c, **adamw)
        for _ in range(3):
            model.zero_grad(set_to_none=True)
            model(**mine).loss.backward()
            reducer.finish()
            opt.step()
        torch.cuda.synchronize()
        norm = opt.grad_norm
        reducer.close()
    np.savez(os.path.join(out_dir, f"rank{rank}.npz"), grad_norm=np.array([float(norm)], np.float32),
             **{k: p.detach().float().cpu().numpy() for k, p in model.named_parameters() if p.requires_grad})
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.parametrize("kind,dtype_name", [("sharded", "float32"), ("sharded", "bfloat16"), ("allreduce", "float32"), ("allreduce", "bfloat16")])
def test_two_ranks_with_max_grad_norm_equal_one_process_on_the_whole_batch(tmp_path, kind, dtype_name):
    """Two processes sharing the GPU through gloo, each on half of the batch, equal one process on the whole batch with FusedAdamW(max_grad_norm),
    and both ranks hold the same norm bit for bit.  sharded: ShardedAdamW(max_grad_norm) (shard sums, one all-reduce of the sum, replicated
    un-fused parameters counted once); allreduce: GradientAllReducer + FusedAdamW(max_grad_norm) (finish() averages before step())."""
    from flamingo_mini_amd import FusedAdamW
    dtype = getattr(torch, dtype_name)
    c = 0.25 * _first_norm(dtype)
    mp.start_processes(_worker, args=(2, _free_port(), str(tmp_path), kind, dtype_name, c), nprocs=2, join=True, start_method="spawn")
    r0, r1 = np.load(tmp_path / "rank0.npz"), np.load(tmp_path / "rank1.npz")
    assert np.array_equal(r0["grad_norm"], r1["grad_norm"])         # the same coefficient on both ranks, bit for bit
    model, batch, adamw = _h64(dtype)
    opt = FusedAdamW(list(model.parameters_trainable()), max_grad_norm=c, **adamw)
    _train_eager(model, batch, opt)
    f32 = dtype == torch.float32
    assert float(opt.grad_norm) > c
    assert abs(float(r0["grad_norm"][0]) - float(opt.grad_norm)) <= (1e-4 if f32 else 3e-2) * float(opt.grad_norm)
    for k, p in model.named_parameters():
        if p.requires_grad:
            assert np.array_equal(r0[k], r1[k]), k
            assert rel(torch.from_numpy(r0[k]), p.detach().float().cpu()) < (1e-4 if f32 else 3e-2), k
