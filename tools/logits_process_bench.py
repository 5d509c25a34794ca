#!/usr/bin/env python
"""Logits processors (repetition penalty 1.3, no-repeat bigrams, min_length) at the benchmark's caption geometry (config B: gpt2-large + CLIP
ViT-L/14, random-init backbones, batch 32, bf16, a 4-token prompt with the media tag first - bench.py's caption leg).  One JSON line:

    process_logits_us   ff_logits_process alone on 32 rows x 50 258 columns bf16 with histories of 32, 150 and 1024 tokens (device events
                        around --launches back-to-back calls; the logits are not restored between calls: a later call penalises the
                        penalised values again, with the same loads and stores)
    torch_chain_us      FlamingoModel._process_logits (decoding.process_logits), the torch restatement the dynamic loops use, on the same GPU and inputs: the op chain
                        the kernel replaces (cat, gather, where, scatter, unfold, compare, all, scatter)
    greedy_off / greedy_on   generate() on the static path without and with the processors: tokens/s and ms per replayed decode step

Method (benchlib.host_rounds): every path is warmed up with one full call (sessions built, graphs captured), then timed with a host clock
around `--rounds` calls that each end in a device synchronise, ALTERNATING inside a round; the median is reported with the spread.  The
greedy_off figure is what the commit before the processors measured with the same command: run this file's greedy_off leg there
(`--only off` needs nothing of the feature) to compare.  Needs the GPU: there is no fallback.

    python tools/logits_process_bench.py [--tokens 32] [--rounds 5] [--only off]
"""
import argparse
import json

import torch

import benchlib


def main():
    ap = argparse.ArgumentParser()
    benchlib.caption_arguments(ap)
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--only", choices=["off"], default=None, help="off: the processors-off decode leg alone (runs on a tree without the feature)")
    a = ap.parse_args()
    benchlib.need_gpu(__file__)
    dev, dt = torch.device("cuda"), torch.bfloat16
    model, ids, kw = benchlib.caption_setup(a, dev, dt)
    proc = dict(repetition_penalty=1.3, no_repeat_ngram_size=2, min_length=kw["max_length"] // 2, eos_token_id=50256, pad_token_id=50256)
    paths = {"greedy_off": lambda: model.generate(ids, **kw)}
    if a.only is None:
        paths["greedy_on"] = lambda: model.generate(ids, **proc, **kw)
    res = {"geometry": f"{a.lm}, batch {a.batch}, prompt 4 + {a.tokens} new tokens, bf16, random-init backbones", "rounds": a.rounds,
           "device": torch.cuda.get_device_name(0)}
    with torch.no_grad():
        times, _ = benchlib.host_rounds(paths, a.rounds)
        res["decode_step_hip_graph"] = all(benchlib.graphed(s) for s in model._decode_sessions.values())
        if a.only is None:
            from flamingo_mini_amd import functional as F
            from flamingo_mini_amd.modeling_flamingo import FlamingoModel
            V = 50258
            g = torch.Generator(device="cuda").manual_seed(0)
            logits = (torch.randn((a.batch, V), generator=g, device=dev) * 4).to(dt)
            hist = torch.randint(0, V, (a.batch, 1024), generator=g, device=dev)
            min_len = torch.full((1,), 2048, dtype=torch.long, device=dev)

            res["process_logits_us"], res["torch_chain_us"] = {}, {}
            for n in (32, 150, 1024):
                n_dev = torch.full((1,), n, dtype=torch.long, device=dev)
                h = hist[:, :n].contiguous()
                x32 = logits.float()
                res["process_logits_us"][n] = benchlib.launch_us(lambda: F.process_logits(logits, h, n_dev, 1.3, 2, 50256, min_len), a.launches)
                res["torch_chain_us"][n] = benchlib.launch_us(lambda: FlamingoModel._process_logits(x32, h, 1.3, 2, 50256, 2048), a.launches)
    for name, ts in times.items():
        res[name] = benchlib.tokens_report(ts, a.batch, a.tokens)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
