"""Two data-parallel ranks on the REAL kernels: two processes share the one GPU of the test box (RCCL refuses two ranks on a device, so
the exchange goes through gloo, which accepts device tensors), each trains on its half of the h64 fixture's batch, and the result must
equal one process training on the whole batch - DDP's mean semantics (/root/reference/training/train.sh:26,36) on the
fused bf16 / fp32 kernels with hoisted K / V, deferred grouped weight gradients and the reducer's buckets, for eager steps and for the
piecewise replay (captured sub-graphs, collectives issued between them, AdamW as per-segment sub-graphs), and for fp32 parameters under
torch.autocast (the fused modules run on casts of the parameters: no gradient bucket of theirs reaches the reducer).  In every case each
rank also checks which gradient storage its reducer exchanged: every trainable parameter's gradient exactly once per step."""
import os
import socket
import sys

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_STEPS = 3


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _paths():
    for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tests", "golden")):
        if p not in sys.path:
            sys.path.insert(0, p)


def _train(model, batch, kind, reducer, adamw, autocast=None):
    """kind: eager | piecewise | overlapped; autocast: None (the parameters' own dtype) or the dtype of torch.autocast around the forward."""
    from flamingo_mini_amd import FusedAdamW
    from flamingo_mini_amd.graphs import PiecewiseGraphedTrainStep
    opt = FusedAdamW([p for p in model.parameters_trainable()], capturable=kind != "eager", **adamw)
    losses = []
    if kind == "eager":
        for _ in range(N_STEPS):
            model.zero_grad(set_to_none=True)
            with torch.autocast("cuda", dtype=autocast or torch.bfloat16, enabled=autocast is not None):
                loss = model(**batch).loss
            loss.backward()
            if reducer is not None:
                reducer.finish()
            opt.step()
            losses.append(float(loss.detach()))
    else:
        step = PiecewiseGraphedTrainStep(model, opt, batch, warmup=1, reducer=reducer, segment_layers=1, pace="host" if kind == "overlapped" else "stream",
                                         overlap_optimizer=kind == "overlapped", autocast=autocast)       # (the constructor's warm-up is training step 1)
        losses = [float("nan")] + [float(step()) for _ in range(N_STEPS - 1)]
    torch.cuda.synchronize()
    return losses


def _record_exchanges(reducer, model):
    """The exchange-coverage invariant, independent of tolerances.  Every exchange of the reducer goes through `_mean_in_place` (early buckets,
    accumulated and deferred gradients, the fused parameters' gradients under autocast); the wrapper records the byte range of each tensor it
    all-reduces, and the wrapped finish() - once per training step, after the step's last exchange - counts per trainable parameter how many
    of the step's ranges hold its gradient storage (-1: no gradient).  1 everywhere = nothing missed, nothing exchanged twice; a range that
    is a merged arena bucket holds many gradients, but each gradient lies in one range."""
    params = [p for _, p in model.named_parameters() if p.requires_grad]
    ranges, counts, exchanges = [], [], []
    mean_in_place, finish = reducer._mean_in_place, reducer.finish

    def recorded_mean_in_place(t):
        ranges.append((t.data_ptr(), t.numel() * t.element_size()))
        mean_in_place(t)

    def recorded_finish():
        finish()
        row = []
        for p in params:
            if p.grad is None:
                row.append(-1)
                continue
            lo = p.grad.data_ptr()
            hi = lo + p.grad.numel() * p.grad.element_size()
            row.append(sum(a <= lo and hi <= a + n for a, n in ranges))
        counts.append(row)
        exchanges.append(len(ranges))
        ranges.clear()

    reducer._mean_in_place, reducer.finish = recorded_mean_in_place, recorded_finish
    return counts, exchanges


def _worker(rank, world, port, out_dir, kind, dtype_name, amp):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    _paths()
    from test_model_plumbing import H64, build_h64
    from flamingo_mini_amd.data_parallel import GradientAllReducer
    model, z, batch = build_h64(getattr(torch, dtype_name), "cuda")
    per = batch["input_ids"].shape[0] // world
    mine = {k: v[rank * per:(rank + 1) * per].contiguous() for k, v in batch.items()}
    reducer = GradientAllReducer(model)
    assert reducer.active and not reducer.cuda
    counts, exchanges = _record_exchanges(reducer, model)
    losses = _train(model, mine, kind, reducer, H64["adamw"], AMP.get(amp))
    reducer.close()
    np.savez(os.path.join(out_dir, f"rank{rank}.npz"), losses=np.array(losses), coverage=np.array(counts), exchanges=np.array(exchanges),
             coverage_names=np.array([k for k, p in model.named_parameters() if p.requires_grad]),
             **{k: p.detach().float().cpu().numpy() for k, p in model.named_parameters() if p.requires_grad})
    dist.barrier()
    dist.destroy_process_group()


AMP = {"bf16": torch.bfloat16, "fp16": torch.float16}
CASES = [(k, d, None) for d in ("float32", "bfloat16") for k in ("eager", "piecewise", "overlapped")] + \
    [("eager", "float32", "bf16"), ("eager", "float32", "fp16"), ("piecewise", "float32", "bf16"), ("overlapped", "float32", "bf16")]


def _case_id(kind, dtype_name, amp):
    return f"{kind}-{dtype_name}" if amp is None else f"{kind}-autocast{'' if amp == 'bf16' else '-' + amp}-{dtype_name}"


@pytest.mark.parametrize("kind,dtype_name,amp", [pytest.param(*c, id=_case_id(*c)) for c in CASES])
def test_two_ranks_on_the_real_kernels_equal_one_process_on_the_whole_batch(tmp_path, kind, dtype_name, amp):
    """(*-autocast: fp32 parameters under torch.autocast - bf16, or fp16, where the fused modules keep their fp32 kernels.  Under bf16 they run on
    casts of the parameters, no gradient bucket of theirs arrives, and the reducer exchanges those parameters' gradients in finish() - or, in
    the piecewise replay, as buckets of their own after the segment that made them final, before that segment's optimizer piece.  The
    reference is one process under the same autocast dtype.)"""
    _paths()
    from test_model_plumbing import H64, build_h64
    from util import rel
    mp.start_processes(_worker, args=(2, _free_port(), str(tmp_path), kind, dtype_name, amp), nprocs=2, join=True, start_method="spawn")
    r0, r1 = np.load(tmp_path / "rank0.npz"), np.load(tmp_path / "rank1.npz")
    for r in (r0, r1):          # every trainable gradient inside exactly one exchanged range, in every step (the constructor's warm-up included)
        assert r["coverage"].shape == (N_STEPS, len(r["coverage_names"])), r["coverage"].shape
        for i, row in enumerate(r["coverage"]):
            bad = {str(n): int(c) for n, c in zip(r["coverage_names"], row) if c != 1}
            assert not bad, (i, bad, r["exchanges"].tolist())
    assert np.array_equal(r0["exchanges"], r1["exchanges"]), (r0["exchanges"], r1["exchanges"])
    model, z, batch = build_h64(getattr(torch, dtype_name), "cuda")
    ref_losses = _train(model, batch, "eager", None, H64["adamw"], AMP.get(amp))
    f32 = dtype_name == "float32" and amp is None
    for i in range(1 if kind != "eager" else 0, N_STEPS):      # the whole-batch loss is the mean of the two ranks' losses (equal token counts)
        both = 0.5 * (float(r0["losses"][i]) + float(r1["losses"][i]))
        assert abs(both - ref_losses[i]) <= (2e-5 if f32 else 3e-2) * max(1.0, abs(ref_losses[i])), (i, both, ref_losses)
    for k, p in model.named_parameters():
        if not p.requires_grad:
            continue
        assert np.array_equal(r0[k], r1[k]), k                  # the ranks hold the same parameters after every exchange
        assert rel(torch.from_numpy(r0[k]), p.detach().float().cpu()) < (1e-4 if f32 else 3e-2), k
