#!/usr/bin/env python
"""The truncation samplers (generate(min_p=, typical_p=, epsilon_cutoff=, eta_cutoff=)) at the benchmark's caption geometry (config B:
gpt2-large + CLIP ViT-L/14, random-init backbones, batch 32, bf16, a 4-token prompt with the media tag first - bench.py's caption leg),
temperature 0.8, top_k 50, top_p 0.9.  One JSON line:

    launch_us           on 32 x 50 258 bf16 rows (randn x 4): ff_sample_token (the yardstick: the parent commit's launch, untouched), then
                        ff_sample_token_truncated with each rule alone and with all four, under the same temperature / top_k / top_p, and
                        "rules_only": each rule alone and all four with top_k / top_p off (the rule's own passes beside the bare draw);
                        --launches calls are captured into one HIP graph, which is replayed --replays times between two device events
                        (benchlib.launch_us)
    torch_chain_us      decoding.filter_logits + truncate_logits_torch + softmax + multinomial on the same rows on the GPU, all four rules:
                        the chain the launch replaces (eager, events around --launches calls: it synchronises inside)
    sampled_off         generate(do_sample=True, static_decode=True): tokens/s and ms per replayed decode step without the rules
    sampled_truncated   the same call with all four rules

Method (benchlib.host_rounds): every path is warmed up with one full call (sessions built, graphs captured), then timed with a host clock
around `--rounds` calls that each end in a device synchronise, ALTERNATING inside a round; the median is reported with the spread.  The
default sampled call against the commit before the feature: run `--only off` (it needs nothing of the feature) on both trees.  `--only
kernel` times the launches alone, without building the model.  Needs the GPU: there is no fallback.

    python tools/truncation_bench.py [--tokens 32] [--rounds 5] [--only off | kernel]
"""
import argparse
import json

import torch

import benchlib

RULES = dict(min_p=0.05, typical_p=0.9, epsilon_cutoff=3e-4, eta_cutoff=2e-3)


def main():
    ap = argparse.ArgumentParser()
    benchlib.caption_arguments(ap)
    ap.add_argument("--launches", type=int, default=50, help="calls captured into the timed graph")
    ap.add_argument("--replays", type=int, default=40, help="replays of that graph inside the timed window")
    ap.add_argument("--temperature", type=float, default=0.8)
    ap.add_argument("--top-k", type=int, default=50)
    ap.add_argument("--top-p", type=float, default=0.9)
    ap.add_argument("--only", choices=["off", "kernel"], default=None,
                    help="off: the default sampled decode leg alone (runs on a tree without the feature); kernel: the launch timings alone, no model")
    a = ap.parse_args()
    benchlib.need_gpu(__file__)
    dev, dt = torch.device("cuda"), torch.bfloat16
    sk = dict(do_sample=True, temperature=a.temperature, top_k=a.top_k, top_p=a.top_p)
    res = {"device": torch.cuda.get_device_name(0), "sampling": {k: v for k, v in sk.items() if k != "do_sample"}, "rules": RULES}
    times = {}
    if a.only != "kernel":
        model, ids, kw = benchlib.caption_setup(a, dev, dt)
        gen = torch.Generator(device="cuda")
        paths = {"sampled_off": lambda: model.generate(ids, generator=gen.manual_seed(1), static_decode=True, **kw, **sk)}
        if a.only is None:
            paths["sampled_truncated"] = lambda: model.generate(ids, generator=gen.manual_seed(1), static_decode=True, **kw, **sk, **RULES)
        res.update(geometry=f"{a.lm}, batch {a.batch}, prompt 4 + {a.tokens} new tokens, bf16, random-init backbones", rounds=a.rounds)
        with torch.no_grad():
            times, _ = benchlib.host_rounds(paths, a.rounds)
        res["decode_step_hip_graph"] = all(benchlib.graphed(s) for s in model._decode_sessions.values())
    if a.only != "off":
        from flamingo_mini_amd import decoding, functional as F
        V = 50258
        g = torch.Generator(device="cuda").manual_seed(0)
        x = (torch.randn((a.batch, V), generator=g, device=dev) * 4).to(dt)
        u = torch.rand(a.batch, generator=g, device=dev)
        tok = torch.empty(a.batch, dtype=torch.long, device=dev)
        timed = lambda fn: benchlib.launch_us(fn, a.launches, a.replays, digits=1)
        arms = {"ff_sample_token": {}, **{name: {name: v} for name, v in RULES.items()}, "all_four": RULES}
        res.update(window=f"graph replay, {a.launches * a.replays} calls per figure", launch_us={}, rules_only_launch_us={})
        with torch.no_grad():
            for name, tr in arms.items():
                res["launch_us"][name] = timed(lambda: F.sample_tokens(x, u, a.temperature, a.top_k, a.top_p, out=tok, **tr))
                res["rules_only_launch_us"][name] = timed(lambda: F.sample_tokens(x, u, a.temperature, 0, 1.0, out=tok, **tr))

            def chain():
                kept = decoding.truncate_logits_torch(decoding.filter_logits(x.float(), a.temperature, a.top_k, a.top_p), **RULES)
                return torch.multinomial(kept.softmax(-1), 1)[:, 0]
            res["torch_chain_us"] = benchlib.launch_us(chain, a.launches, eager=True, digits=1)
        res["torch_over_kernel"] = round(res["torch_chain_us"] / res["launch_us"]["all_four"], 1)
    for name, ts in times.items():
        res[name] = benchlib.tokens_report(ts, a.batch, a.tokens)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
