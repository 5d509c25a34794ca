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
import statistics

import torch

import benchlib

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
    device = torch.device("cuda", 0)
    shapes = benchlib.trainable_shapes(a.config, device)
    n_params = sum(torch.Size(s).numel() for s in shapes)
    graphs, opts = benchlib.capture_arms(shapes, {name: kw for name, (kw, _, _) in ARMS.items()}, device)
    times = benchlib.replay_rounds({name: graph.replay for name, graph in graphs.items()}, a.rounds, a.steps)
    out = dict(config=a.config, tensors=len(shapes), trainable_params=n_params, rounds=a.rounds, steps_per_round=a.steps)
    for name, (_, per_param, state) in ARMS.items():
        ms = statistics.median(times[name])
        ms_median, ms_all = benchlib.ms_summary(times[name])
        out[name] = dict(ms_median=ms_median, ms_all=ms_all, bytes_per_param=per_param,
                         tb_per_s=round(per_param * n_params / (ms * 1e-3) / 1e12, 3), state_bytes_per_param=state,
                         steps_taken=int(float(opts[name].state_dict()["state"][0]["step"])))
    diffs = {name: benchlib.round_diffs(times, name, "plain") for name in ("plain2", "ema", "ema8")}
    for name, d in diffs.items():
        median, every = benchlib.ms_summary(d)
        out[f"{name}_minus_plain_ms"] = dict(median=median, all=every)
    out["aa_spread_ms"] = round(benchlib.aa_spread(diffs["plain2"]), 4)
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
    benchlib.emit("\n".join(lines) + "\n" + json.dumps(out), a.out)


if __name__ == "__main__":
    main()
