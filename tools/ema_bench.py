"""Cost of the weight average (FusedAdamW(ema_decay=...)) in the optimizer step alone, over the trainable parameter shapes of a bench.py
workload (default: config B).

    python tools/ema_bench.py [--config B] [--rounds 7] [--steps 24] [--out FILE]

Four FusedAdamW(capturable=True) optimizers over their own bf16 copies of the same parameter shapes, bf16 moments, one shared set of bf16
gradients:
    plain      no average                                        (the code path as it was)
    plain2     the same again                                    (A/A: what two identical arms differ by)
    ema        ema_decay=0.9999                                  (one ff_ema_update after each bucket's AdamW launch)
    ema8       ema_decay=0.9999, ema_every=8                     (the launch is there every step and returns at once on 7 steps of 8)
Each step() is captured into a HIP graph after an eager warm-up step; the graphs are replayed alternately (`--rounds` rounds of `--steps`
back-to-back replays each - a multiple of 8, so that every block of ema8 holds the same number of averaging steps - device events around
each block), so that clock and thermal drift fall on all arms alike.  Prints the table and one JSON line: median ms per step of each arm,
the bytes a step moves per parameter (computed from the shapes: reads + writes of parameters, gradients, moments and shadows; ema8's is the
average over 8 steps), the rate that gives, the per-round differences against plain next to the A/A spread, and the rate of the averaging
pass alone (10 bytes per parameter over ema - plain).  The model is only built for its shapes and dropped before anything is timed."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ADAMW_BYTES = 2 * 2 + 2 + 2 * 2 * 2      # parameter read + write, gradient read, two moments read + write (all bf16)
EMA_BYTES = 2 + 2 * 4                    # parameter read, fp32 shadow read + write
ARMS = {   # name: (FusedAdamW arguments, bytes moved per parameter and step, bytes of optimizer state per parameter)
    "plain": (dict(), ADAMW_BYTES, 4),
    "plain2": (dict(), ADAMW_BYTES, 4),
    "ema": (dict(ema_decay=0.9999), ADAMW_BYTES + EMA_BYTES, 8),
    "ema8": (dict(ema_decay=0.9999, ema_every=8), ADAMW_BYTES + EMA_BYTES / 8, 8),
}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="B")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--steps", type=int, default=24)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if a.steps % 8:
        ap.error("--steps must be a multiple of 8 (ema8 averages on every 8th step)")
    saved, sys.argv = sys.argv, [sys.argv[0], "--config", a.config]
    import bench
    args = bench.parse()
    sys.argv = saved
    from flamingo_mini_amd import FusedAdamW, ffi
    ffi.lib()
    device = torch.device("cuda", 0)
    model, _ = bench.build_model(args, device, torch.bfloat16)
    shapes = [tuple(p.shape) for p in model.parameters_trainable()]
    del model
    torch.cuda.empty_cache()
    n_params = sum(torch.Size(s).numel() for s in shapes)
    gen = torch.Generator(device=device).manual_seed(1)
    grads = [(torch.randn(s, generator=gen, device=device) * 1e-3).to(torch.bfloat16) for s in shapes]
    graphs, opts = {}, {}
    for name, (kw, _, _) in ARMS.items():
        params = [torch.nn.Parameter((torch.randn(s, generator=gen, device=device) * 0.02).to(torch.bfloat16)) for s in shapes]
        for p, g in zip(params, grads):
            p.grad = g
        opt = opts[name] = FusedAdamW(params, lr=1e-4, capturable=True, **kw)
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):                          # the eager step allocates the state, the shadows and the device counters
            opt.step()
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        graphs[name] = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graphs[name]):
            opt.step()
    times = {k: [] for k in ARMS}
    for _ in range(a.rounds):
        for name, graph in graphs.items():
            graph.replay()                                     # (one untimed replay after switching)
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            for _ in range(a.steps):
                graph.replay()
            t1.record()
            t1.synchronize()
            times[name].append(t0.elapsed_time(t1) / a.steps)
    out = dict(config=a.config, tensors=len(shapes), trainable_params=n_params, rounds=a.rounds, steps_per_round=a.steps)
    for name, (_, per_param, state) in ARMS.items():
        ms = statistics.median(times[name])
        out[name] = dict(ms_median=round(ms, 4), ms_all=[round(t, 4) for t in times[name]], bytes_per_param=per_param,
                         tb_per_s=round(per_param * n_params / (ms * 1e-3) / 1e12, 3), state_bytes_per_param=state,
                         steps_taken=int(float(opts[name].state_dict()["state"][0]["step"])))
    diffs = {name: [x - y for x, y in zip(times[name], times["plain"])] for name in ("plain2", "ema", "ema8")}
    for name, d in diffs.items():
        out[f"{name}_minus_plain_ms"] = dict(median=round(statistics.median(d), 4), all=[round(x, 4) for x in d])
    out["aa_spread_ms"] = round(max(abs(x) for x in diffs["plain2"]), 4)
    ema_ms = statistics.median(diffs["ema"])
    out["ema_pass"] = dict(ms=round(ema_ms, 4), bytes_per_param=EMA_BYTES, tb_per_s=round(EMA_BYTES * n_params / (ema_ms * 1e-3) / 1e12, 3))
    lines = [f"{'arm':8s}{'ms / step':>11s}{'bytes / parameter':>20s}{'TB/s':>8s}{'state bytes / parameter':>26s}    per-round difference against plain, ms"]
    for name in ARMS:
        r = out[name]
        d = "" if name == "plain" else " ".join(f"{x:+.4f}" for x in diffs[name])
        lines.append(f"{name:8s}{r['ms_median']:11.4f}{r['bytes_per_param']:20.2f}{r['tb_per_s']:8.2f}{r['state_bytes_per_param']:26d}    {d}")
    lines.append(f"A/A spread (largest |plain2 - plain| of a round): {out['aa_spread_ms']:.4f} ms")
    lines.append(f"the averaging pass alone (ema - plain, median of the rounds): {ema_ms:.4f} ms for {EMA_BYTES} bytes per parameter = "
                 f"{out['ema_pass']['tb_per_s']:.2f} TB/s; the plain AdamW arm of this run: {out['plain']['tb_per_s']:.2f} TB/s")
    text = "\n".join(lines) + "\n" + json.dumps(out)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
