#!/usr/bin/env python
"""Token log-probabilities (generate(output_logprobs=True)) at the benchmark's caption geometry (config B: gpt2-large + CLIP ViT-L/14,
random-init backbones, batch 32, bf16, a 4-token prompt with the media tag first - bench.py's caption leg).  One JSON line:

    token_logprob_us    ff_token_logprob alone on 32 rows x 50 258 columns, bf16 and fp32, next to torch's log_softmax + gather on the same
                        inputs, the chain the kernel replaces: --launches calls are captured into one HIP graph, which is replayed
                        --replays times between two device events (the device paces the launches, not the host's enqueue rate; the
                        default window is 20 000 launches, a few tenths of a second)
    greedy_off / greedy_on   generate() on the static path without and with return_dict_in_generate=True, output_logprobs=True: tokens/s
                        and ms per replayed decode step

Method (benchlib.host_rounds): every path is warmed up with one full call (sessions built, graphs captured), then timed with a
host clock around `--rounds` calls that each end in a device synchronise, ALTERNATING inside a round; the median is reported with the
spread.  The default path against the commit before the feature: run `--only off` (it needs nothing of the feature) on both trees.
`--only kernel` times the launches alone, without building the model - also the program for a kernel trace in a run of its own:
    rocprofv3 --kernel-trace --stats --output-format csv -d <out> -- python tools/token_logprob_bench.py --only kernel --eager
(--eager: plain launches, which the trace lists by kernel name; its AverageNs of token_logprob_kernel is the kernel's own time).
Needs the GPU: there is no fallback.

    python tools/token_logprob_bench.py [--tokens 32] [--rounds 5] [--only off | kernel]
"""
import argparse
import json

import torch

import benchlib


def main():
    ap = argparse.ArgumentParser()
    benchlib.caption_arguments(ap)
    ap.add_argument("--launches", type=int, default=200, help="calls captured into the timed graph")
    ap.add_argument("--replays", type=int, default=100, help="replays of that graph inside the timed window")
    ap.add_argument("--eager", action="store_true", help="time plain launches instead of a replayed graph (for a kernel trace)")
    ap.add_argument("--only", choices=["off", "kernel"], default=None,
                    help="off: the default decode leg alone (runs on a tree without the feature); kernel: the launch timings alone, no model")
    a = ap.parse_args()
    benchlib.need_gpu(__file__)
    dev, dt = torch.device("cuda"), torch.bfloat16
    res = {"device": torch.cuda.get_device_name(0)}
    times = {}
    if a.only != "kernel":
        model, ids, kw = benchlib.caption_setup(a, dev, dt)
        paths = {"greedy_off": lambda: model.generate(ids, **kw)}
        if a.only is None:
            paths["greedy_on"] = lambda: model.generate(ids, return_dict_in_generate=True, output_logprobs=True, **kw)
        res.update(geometry=f"{a.lm}, batch {a.batch}, prompt 4 + {a.tokens} new tokens, bf16, random-init backbones", rounds=a.rounds)
        with torch.no_grad():
            times, _ = benchlib.host_rounds(paths, a.rounds)
        res["decode_step_hip_graph"] = all(benchlib.graphed(s) for s in model._decode_sessions.values())
    if a.only != "off":
        from flamingo_mini_amd import functional as F
        V = 50258
        g = torch.Generator(device="cuda").manual_seed(0)
        x32 = torch.randn((a.batch, V), generator=g, device=dev) * 4
        tok = torch.randint(0, V, (a.batch,), generator=g, device=dev)
        out = torch.zeros(a.batch, device=dev)

        def timed(fn):
            """microseconds per call: --launches calls in one graph, replayed --replays times between two device events"""
            return benchlib.launch_us(fn, a.launches, a.replays, eager=a.eager, digits=2)

        res.update(window=f"{'eager launches' if a.eager else 'graph replay'}, {a.launches if a.eager else a.launches * a.replays} calls per figure",
                   token_logprob_us={}, torch_chain_us={})
        with torch.no_grad():
            for name, x in (("bf16", x32.to(dt)), ("fp32", x32)):
                res["token_logprob_us"][name] = timed(lambda: F.token_logprobs(x, tok, out=out))
                res["torch_chain_us"][name] = timed(lambda: x.float().log_softmax(-1).gather(1, tok[:, None]))
    for name, ts in times.items():
        res[name] = benchlib.tokens_report(ts, a.batch, a.tokens)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
