"""Cost of gradient clipping (max_grad_norm) in the captured training step at a bench.py workload (default: config B, the headline).

    python tools/grad_clip_bench.py [--config B] [--rounds 7] [--steps 10] [--max-grad-norm 1.0] [--only clipped] [--skip-nonfinite]

Builds the model through bench.build_model, captures two GraphedTrainSteps on it - FusedAdamW(capturable=True) without and with
max_grad_norm - and replays them alternately (`--rounds` rounds of `--steps` replays each, HIP events around each block), so that
clock and thermal drift fall on both alike.  Prints one JSON line: median ms per step of each, their difference, and the trainable
gradient bytes one sum-of-squares sweep reads.  `--only clipped` replays just the clipped step (for a rocprofv3 --kernel-trace --stats
run that isolates the clipping kernels).

`--skip-nonfinite` measures the non-finite gradient guard (FusedAdamW(skip_nonfinite=True)) the same way: four steps on the same model -
plain, clipped, clipped+guard, guard (no clipping) - plus a second clipped step (A/A: the noise of the method), all replayed alternately in
the same rounds.  Adds to the JSON line the medians of the per-round differences clipped+guard - clipped (expected about 0: ff_grad_guard
takes the place of ff_grad_clip_coef, no extra pass), guard - plain (expected: one sum-of-squares sweep, as clipped - plain) and
clipped - clipped, the largest per-round |A/A| difference, and the two acceptance checks against it."""
import argparse
import json
import statistics

import benchlib


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="B")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--max-grad-norm", type=float, default=1.0)
    ap.add_argument("--only", default="", choices=["", "clipped"])
    ap.add_argument("--skip-nonfinite", action="store_true")
    a = ap.parse_args()
    model, batch, params = benchlib.train_setup(a.config)
    from flamingo_mini_amd import FusedAdamW, GraphedTrainStep
    grad_bytes = sum(p.numel() * p.element_size() for p in params)
    kinds = ["clipped"] if a.only else ["plain", "clipped"]
    if a.skip_nonfinite:
        if a.only:
            ap.error("--skip-nonfinite measures all its arms: not with --only")
        kinds += ["clipped+guard", "guard", "clipped_aa"]
    steps, opts = {}, {}
    for kind in kinds:
        opts[kind] = FusedAdamW(params, lr=1e-4, capturable=True, max_grad_norm=a.max_grad_norm if kind.startswith("clipped") else None,
                                skip_nonfinite=kind.endswith("guard"))
        steps[kind] = GraphedTrainStep(model, opts[kind], batch, warmup=2)
    times = benchlib.replay_rounds(steps, a.rounds, a.steps)
    for s in steps.values():
        s.close()
    out = dict(config=a.config, trainable_params=sum(p.numel() for p in params), grad_bytes=grad_bytes, max_grad_norm=a.max_grad_norm,
               rounds=a.rounds, steps_per_round=a.steps, grad_norm=float(opts["clipped"].grad_norm))
    for kind in kinds:
        out[f"{kind}_ms_median"], out[f"{kind}_ms_all"] = benchlib.ms_summary(times[kind])
    if not a.only:
        out["delta_ms_median"] = benchlib.median_diff(times, "clipped", "plain")
    if a.skip_nonfinite:
        def diffs(x, y):
            return benchlib.round_diffs(times, x, y)

        aa = diffs("clipped_aa", "clipped")
        aa_bound = benchlib.aa_spread(aa)
        guard_on_clip = statistics.median(diffs("clipped+guard", "clipped"))
        guard_alone = statistics.median(diffs("guard", "plain"))
        out.update(skipped_steps={k: int(opts[k].skipped_steps) for k in ("clipped+guard", "guard")},
                   clipped_guard_minus_clipped_ms_median=round(guard_on_clip, 4), guard_minus_plain_ms_median=round(guard_alone, 4),
                   aa_ms_median=round(statistics.median(aa), 4), aa_abs_max_ms=round(aa_bound, 4),
                   accept_guard_on_clip=abs(guard_on_clip) <= aa_bound,
                   accept_guard_alone=guard_alone <= statistics.median(diffs("clipped", "plain")) + aa_bound)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
