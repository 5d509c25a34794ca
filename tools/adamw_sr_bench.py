"""Cost of stochastic rounding in the optimizer step alone, over the trainable parameter shapes of a bench.py workload (default: config B).

    python tools/adamw_sr_bench.py [--config B] [--rounds 7] [--steps 20] [--out FILE]

Four FusedAdamW(capturable=True) optimizers over their own bf16 copies of the same parameter shapes (one shared set of bf16 gradients):
    rne        bf16 moments, round to nearest                    (the default configuration)
    sr         bf16 moments, stochastic rounding                 (three Philox calls per 8-element vector)
    sr_f32     fp32 moments, stochastic rounding                 (one call per vector)
    master     fp32 master copies and fp32 moments               (the remedy before stochastic rounding)
Each step() is captured into a HIP graph after an eager warm-up step; the graphs are replayed alternately (`--rounds` rounds of `--steps`
back-to-back replays each, device events around each block), so that clock and thermal drift fall on all arms alike.  Prints one JSON
line: median ms per step of each arm, the bytes a step of each arm moves (computed from the shapes: reads + writes of parameters,
gradients, moments, master copies), the rate that gives, the median per-round differences against rne and master, and the optimizer
state each arm keeps per parameter.  The model is only built for its shapes and dropped before anything is timed."""
import argparse
import json
import statistics

import torch

import benchlib

ARMS = {   # name: (FusedAdamW arguments, bytes moved per parameter and step, bytes of optimizer state per parameter)
    "rne": (dict(), 2 * 2 + 2 + 2 * 2 * 2, 4),
    "sr": (dict(stochastic_rounding=True, sr_seed=1), 2 * 2 + 2 + 2 * 2 * 2, 4),
    "sr_f32": (dict(stochastic_rounding=True, sr_seed=1, state_dtype=torch.float32), 2 * 2 + 2 + 2 * 2 * 4, 8),
    "master": (dict(master_dtype=torch.float32), 2 + 2 + 2 * 4 + 2 * 2 * 4, 12),
}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="B")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    device = torch.device("cuda", 0)
    shapes = benchlib.trainable_shapes(a.config, device)
    n_params = sum(torch.Size(s).numel() for s in shapes)
    graphs, opts = benchlib.capture_arms(shapes, {name: kw for name, (kw, _, _) in ARMS.items()}, device)
    times = benchlib.replay_rounds({name: graph.replay for name, graph in graphs.items()}, a.rounds, a.steps)
    out = dict(config=a.config, tensors=len(shapes), trainable_params=n_params, rounds=a.rounds, steps_per_round=a.steps)
    for name, (_, per_param, state) in ARMS.items():
        ms = statistics.median(times[name])
        ms_median, ms_all = benchlib.ms_summary(times[name])
        out[name] = dict(ms_median=ms_median, ms_all=ms_all, bytes_per_step=per_param * n_params,
                         tb_per_s=round(per_param * n_params / (ms * 1e-3) / 1e12, 3), state_bytes_per_param=state,
                         steps_taken=int(float(opts[name].state_dict()["state"][0]["step"])))
    for name in ("sr", "sr_f32", "master"):
        out[f"{name}_minus_rne_ms_median"] = benchlib.median_diff(times, name, "rne")
    for name in ("sr", "sr_f32"):
        out[f"{name}_minus_master_ms_median"] = benchlib.median_diff(times, name, "master")
    benchlib.emit(json.dumps(out), a.out)


if __name__ == "__main__":
    main()
