#!/usr/bin/env python
"""Classifier-free guidance (generate(guidance_scale=)) at the benchmark's caption geometry (config B: gpt2-large + CLIP ViT-L/14,
random-init backbones, batch 32, bf16, a 4-token prompt with the media tag first - bench.py's caption leg).  One JSON line:

    guided_logits_us    ff_guided_logits alone on 32 + 32 rows x 50 258 columns (the two halves of one (64, V) buffer), bf16 and fp32, next to
                        ff_token_logprob on the same 32 rows (the yardstick of the other selection tools) and to decoding.guided_logits_torch
                        on the GPU, the chain the kernel replaces: --launches calls are captured into one HIP graph, which is replayed
                        --replays times between two device events (benchlib.launch_us)
    greedy_off          generate() on the static path, unguided, batch 32: tokens/s and ms per replayed decode step
    greedy_guided       the same call with guidance_scale=1.5: 64 rows run through the LM
    greedy_off_b64      unguided at batch 64, the yardstick of the guided step: beyond 32 rows the decode feed-forward kernels give way to
                        the GEMM path, guided or not

Method (benchlib.host_rounds): every path is warmed up with one full call (sessions built, graphs captured), then timed with a host clock
around `--rounds` calls that each end in a device synchronise, ALTERNATING inside a round; the median is reported with the spread.  The
default path against the commit before the feature: run `--only off` (it needs nothing of the feature) on both trees.  `--only kernel`
times the launches alone, without building the model.  Needs the GPU: there is no fallback.

    python tools/guidance_bench.py [--tokens 32] [--rounds 5] [--only off | kernel]
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
    ap.add_argument("--scale", type=float, default=1.5)
    ap.add_argument("--only", choices=["off", "kernel"], default=None,
                    help="off: the default decode leg alone (runs on a tree without the feature); kernel: the launch timings alone, no model")
    a = ap.parse_args()
    benchlib.need_gpu(__file__)
    dev, dt = torch.device("cuda"), torch.bfloat16
    res = {"device": torch.cuda.get_device_name(0)}
    times, batches = {}, {}
    if a.only != "kernel":
        model, ids, kw = benchlib.caption_setup(a, dev, dt)
        paths = {"greedy_off": lambda: model.generate(ids, **kw)}
        batches["greedy_off"] = a.batch
        if a.only is None:
            twice = lambda t: torch.cat([t, t], dim=0)
            ids2, kw2 = twice(ids), dict(kw, **{k: twice(kw[k]) for k in ("media_locations", "attention_mask", "pixel_values")})
            paths["greedy_guided"] = lambda: model.generate(ids, guidance_scale=a.scale, **kw)
            paths["greedy_off_b64"] = lambda: model.generate(ids2, **kw2)
            batches.update(greedy_guided=a.batch, greedy_off_b64=2 * a.batch)
        res.update(geometry=f"{a.lm}, batch {a.batch}, prompt 4 + {a.tokens} new tokens, bf16, random-init backbones", rounds=a.rounds)
        with torch.no_grad():
            times, _ = benchlib.host_rounds(paths, a.rounds)
        res["decode_step_hip_graph"] = all(benchlib.graphed(s) for s in model._decode_sessions.values())
    if a.only != "off":
        from flamingo_mini_amd import decoding, functional as F
        V = 50258
        g = torch.Generator(device="cuda").manual_seed(0)
        x32 = torch.randn((2 * a.batch, V), generator=g, device=dev) * 4
        tok = torch.randint(0, V, (a.batch,), generator=g, device=dev)
        scale = torch.tensor([a.scale], device=dev)
        out, lp = torch.zeros((a.batch, V), device=dev), torch.zeros(a.batch, device=dev)
        timed = lambda fn: benchlib.launch_us(fn, a.launches, a.replays, digits=2)
        res.update(window=f"graph replay, {a.launches * a.replays} calls per figure", guided_logits_us={}, token_logprob_us={}, torch_chain_us={})
        with torch.no_grad():
            for name, x in (("bf16", x32.to(dt)), ("fp32", x32)):
                c, u = x[:a.batch], x[a.batch:]
                res["guided_logits_us"][name] = timed(lambda: F.guided_logits(c, u, scale, out=out))
                res["token_logprob_us"][name] = timed(lambda: F.token_logprobs(c, tok, out=lp))
                res["torch_chain_us"][name] = timed(lambda: decoding.guided_logits_torch(c, u, scale))
        res["torch_over_kernel"] = {k: round(res["torch_chain_us"][k] / res["guided_logits_us"][k], 1) for k in res["guided_logits_us"]}
    for name, ts in times.items():
        res[name] = benchlib.tokens_report(ts, batches[name], a.tokens)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
