#!/usr/bin/env python
"""Label smoothing and z-loss in the fused shifted cross-entropy at the benchmark's loss shape (config B: bf16 logits, batch 32, 33
positions, vocabulary 50258).  One JSON line, microseconds per forward + backward pair:

    plain_pair_us    ff_shifted_ce_fwd + ff_shifted_ce_bwd (what label_smoothing = z_loss = 0 launches)
    reg_pair_us      ff_shifted_ce_fwd_reg + ff_shifted_ce_bwd_reg at label_smoothing 0.1, z_loss 1e-4: the same bytes, one more sum in the
                     forward and one more fma per element in the backward
    torch_chain_us   what a Trainer user with --label_smoothing_factor 0.1 runs today: transformers' LabelSmoother(epsilon=0.1) on the
                     model's logits with shifted labels, and its backward to d logits, on the same GPU and the same inputs
    bytes_per_pair   the bytes the two kernels have to move (logits read twice, d logits written once, the row vectors), and with it
    plain_tb_s / reg_tb_s   bytes_per_pair over the pair's time

Method: every path is warmed up, then timed with device events around --launches back-to-back pairs, in --rounds rounds with the paths
ALTERNATING inside a round; the median over the rounds is reported with min .. max, the spread that a difference has to exceed.
Needs the GPU: there is no fallback.

    python tools/loss_reg_bench.py [--rounds 7] [--launches 50]
"""
import argparse
import json
import statistics

import torch

import benchlib


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--seq", type=int, default=33)
    ap.add_argument("--vocab", type=int, default=50258)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--launches", type=int, default=50)
    ap.add_argument("--label-smoothing", type=float, default=0.1)
    ap.add_argument("--z-loss", type=float, default=1e-4)
    a = ap.parse_args()
    benchlib.need_gpu(__file__)
    from transformers.trainer_pt_utils import LabelSmoother
    from flamingo_mini_amd import ffi
    lib, dev, dt = ffi.lib(), torch.device("cuda"), torch.bfloat16
    b, L, V = a.batch, a.seq, a.vocab
    gen = torch.Generator(device="cuda").manual_seed(0)
    logits = (torch.randn((b, L, V), generator=gen, device=dev) * 3).to(dt)
    labels = torch.randint(0, V, (b, L), generator=gen, device=dev)
    labels[:, 1] = -100
    n = b * (L - 1)
    rows, lse = torch.empty(n, device=dev), torch.empty(n, device=dev)
    g = torch.full((n,), 1.0 / int((labels[:, 1:] != -100).sum()), device=dev)
    d = torch.empty_like(logits)
    code, stream = ffi.dtype_code(dt), ffi.stream_handle(dev)
    head = (code, b, L, V, logits.data_ptr(), labels.data_ptr(), -100)

    def plain():
        ffi.check(lib.ff_shifted_ce_fwd(*head, rows.data_ptr(), lse.data_ptr(), stream), "ff_shifted_ce_fwd")
        ffi.check(lib.ff_shifted_ce_bwd(*head, lse.data_ptr(), g.data_ptr(), d.data_ptr(), stream), "ff_shifted_ce_bwd")

    def reg():
        ffi.check(lib.ff_shifted_ce_fwd_reg(*head, rows.data_ptr(), lse.data_ptr(), a.label_smoothing, a.z_loss, stream), "ff_shifted_ce_fwd_reg")
        ffi.check(lib.ff_shifted_ce_bwd_reg(*head, lse.data_ptr(), g.data_ptr(), d.data_ptr(), a.label_smoothing, a.z_loss, stream), "ff_shifted_ce_bwd_reg")

    leaf = logits.clone().requires_grad_(True)
    smoother = LabelSmoother(epsilon=a.label_smoothing)

    def chain():
        leaf.grad = None
        smoother({"logits": leaf}, labels, shift_labels=True).backward()

    paths = {"plain_pair_us": plain, "reg_pair_us": reg, "torch_chain_us": chain}
    times = {k: [] for k in paths}
    for fn in paths.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    for _ in range(a.rounds):
        for name, fn in paths.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.launches):
                fn()
            e1.record()
            torch.cuda.synchronize()
            times[name].append(e0.elapsed_time(e1) / a.launches * 1e3)
    moved = (2 * b * L - b) * V * 2 + b * L * V * 2 + n * 4 * 4            # forward reads b (L - 1) rows, backward reads and writes b L; loss, lse (x 2), g
    res = {"geometry": f"bf16 logits ({b}, {L}, {V}), label_smoothing {a.label_smoothing}, z_loss {a.z_loss}", "rounds": a.rounds, "launches": a.launches,
           "device": torch.cuda.get_device_name(0), "bytes_per_pair": moved}
    for name, ts in times.items():
        res[name] = {"median": round(statistics.median(ts), 1), "min": round(min(ts), 1), "max": round(max(ts), 1)}
    for k in ("plain", "reg"):
        res[f"{k}_tb_s"] = round(moved / (res[f"{k}_pair_us"]["median"] * 1e-6) / 1e12, 2)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
