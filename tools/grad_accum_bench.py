"""Step time of gradient accumulation in the captured training step at a bench.py workload (default: config B, the headline).

    python tools/grad_accum_bench.py [--config B] [--micro-batches 2] [--rounds 7] [--steps 10] [--max-grad-norm 0] [--only accumulate]

Builds the model through bench.build_model and captures three steps on it, each one whole graph over the same batch:
  full        GraphedTrainStep on the whole batch (no accumulation: the reference point)
  autograd    k x (forward, backward of loss / k) with autograd adding into the existing `.grad`, then FusedAdamW.step() - what accumulation
              was before FusedAdamW.accumulate(): from the second micro-batch on the gated blocks leave the deferred, grouped weight-gradient
              launches, and bf16 gradients are summed in bf16
  accumulate  GraphedTrainStep(micro_batches=k): k x (forward, backward, accumulate(1 / k)) + step() on the fp32 accumulators
and replays them alternately (`--rounds` rounds of `--steps` replays each, HIP events around each block), so that clock and thermal
drift fall on all alike.  Prints one JSON line: median ms per step of each, the paired differences, and the bytes one accumulate sweep and
one AdamW sweep over the trainable list move.  `--only NAME` replays just one of them (for a rocprofv3 --kernel-trace --stats run)."""
import argparse
import json

import torch

import benchlib

KINDS = ["full", "autograd", "accumulate"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="B")
    ap.add_argument("--micro-batches", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--max-grad-norm", type=float, default=0.0)
    ap.add_argument("--only", default="", choices=[""] + KINDS)
    a = ap.parse_args()
    model, batch, params = benchlib.train_setup(a.config)
    from flamingo_mini_amd import FusedAdamW, GraphedTrainStep
    k = a.micro_batches

    class AutogradAccumulation(GraphedTrainStep):
        """The same capture with autograd's own accumulation: every micro-batch's backward adds into `.grad`."""

        def _eager(self):
            self.model.zero_grad(set_to_none=True)
            total = None
            for i in range(k):
                micro = {n: (v[i * (v.shape[0] // k):(i + 1) * (v.shape[0] // k)] if torch.is_tensor(v) else v) for n, v in self.static.items()}
                loss = self._loss_fn(self.model(**micro))
                (loss / k).backward()
                total = loss.detach() if total is None else total + loss.detach()
            self.optimizer.step()
            return total / k

    kinds = [a.only] if a.only else KINDS
    steps, opts = {}, {}
    for kind in kinds:
        opts[kind] = FusedAdamW(params, lr=1e-4, capturable=True, max_grad_norm=a.max_grad_norm or None)
        cls = AutogradAccumulation if kind == "autograd" else GraphedTrainStep
        steps[kind] = cls(model, opts[kind], batch, warmup=2, **({"micro_batches": k} if kind == "accumulate" else {}))
    times = benchlib.replay_rounds(steps, a.rounds, a.steps)
    losses = {kind: float(steps[kind].loss) for kind in kinds}
    for s in steps.values():
        s.close()
    n = sum(p.numel() for p in params)
    grad_bytes = sum(p.numel() * p.element_size() for p in params)
    out = dict(config=a.config, micro_batches=k, trainable_params=n, rounds=a.rounds, steps_per_round=a.steps, max_grad_norm=a.max_grad_norm or None,
               accumulator_bytes=4 * n,
               accumulate_sweep_bytes=dict(first=grad_bytes + 4 * n, later=grad_bytes + 8 * n),       # read g (+ read acc) + write acc
               last_loss=losses)
    for kind in kinds:
        out[f"{kind}_ms_median"], out[f"{kind}_ms_all"] = benchlib.ms_summary(times[kind])
    if not a.only:
        out["accumulate_minus_autograd_ms_median"] = benchlib.median_diff(times, "accumulate", "autograd")
        out["accumulate_minus_full_ms_median"] = benchlib.median_diff(times, "accumulate", "full")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
