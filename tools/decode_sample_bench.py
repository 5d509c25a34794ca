#!/usr/bin/env python
"""Sampled caption decoding at the benchmark's geometry (config B: gpt2-large + CLIP ViT-L/14, random-init backbones, batch 32, bf16, a
4-token prompt with the media tag first - bench.py's caption leg), temperature 0.8, top_k 50, top_p 0.9.  Four numbers, one JSON line:

    dynamic_sampling   tokens/s of generate(do_sample=True): the growing-cache loop (decoding.dynamic_decode; filter_logits: topk + sort + 2 softmax + cumsum + scatter,
                       torch.multinomial, torch.cat of ids / masks, a host synchronisation per token)
    static_sampling    tokens/s of generate(do_sample=True, static_decode=True): the fixed-shape session, one decode step replayed from a
                       HIP graph with ff_sample_token inside it
    static_greedy      tokens/s of greedy_generate on the same session machinery (argmax in place of the sampling launch)
    sample_launch_us   the sampling launch alone on the model's own prompt-step logits (batch x vocab, bf16)

Method: every path is warmed up with one full call (sessions built, graphs captured, code objects loaded) and then timed with a host clock
around `--rounds` calls that each end in a device synchronise, the three paths ALTERNATING inside a round; the median per path is reported
with the spread (min .. max).  The launch is timed with device events around `--launches` back-to-back launches (each runs for tens of
microseconds: longer than a host launch, so the stream never drains).  Needs the GPU: there is no fallback.

    python tools/decode_sample_bench.py [--tokens 32] [--rounds 5]
"""
import argparse
import json

import torch

import benchlib


def main():
    ap = argparse.ArgumentParser()
    benchlib.caption_arguments(ap)
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--temperature", type=float, default=0.8)
    ap.add_argument("--top-k", type=int, default=50)
    ap.add_argument("--top-p", type=float, default=0.9)
    a = ap.parse_args()
    benchlib.need_gpu(__file__)
    from flamingo_mini_amd import functional as F
    dev, dt = torch.device("cuda"), torch.bfloat16
    model, ids, kw = benchlib.caption_setup(a, dev, dt)
    ml, am, px, L = kw["media_locations"], kw["attention_mask"], kw["pixel_values"], kw["max_length"]
    sk = dict(do_sample=True, temperature=a.temperature, top_k=a.top_k, top_p=a.top_p)
    gen = torch.Generator(device="cuda")

    def dynamic():
        return model.generate(ids, generator=gen.manual_seed(1), **kw, **sk)

    def static():
        return model.generate(ids, generator=gen.manual_seed(1), static_decode=True, **kw, **sk)

    def greedy():
        return model.greedy_generate(ids, ml, am, pixel_values=px, max_length=L)

    paths = {"dynamic_sampling": dynamic, "static_sampling": static, "static_greedy": greedy}
    with torch.no_grad():
        times, outs = benchlib.host_rounds(paths, a.rounds)
        for out in outs.values():
            assert out.shape == (a.batch, L), out.shape
        sessions = list(model._decode_sessions.values())
        graphed = {("sampling" if s.sampling is not None else "greedy"): benchlib.graphed(s) for s in sessions}

        # the launch alone, on the logits the model really produces for this prompt
        logits = model.flamingo(input_ids=ids, attention_mask=am, media_locations=ml, pixel_values=px).logits[:, -1]
        u = torch.rand(a.batch, device=dev)
        tok = torch.empty(a.batch, dtype=torch.long, device=dev)
        launch_us = benchlib.launch_us(lambda: F.sample_tokens(logits, u, a.temperature, a.top_k, a.top_p, out=tok), a.launches, warmup=10)

    res = {"geometry": f"{a.lm}, batch {a.batch}, prompt 4 + {a.tokens} new tokens, bf16, random-init backbones",
           "sampling": {"temperature": a.temperature, "top_k": a.top_k, "top_p": a.top_p}, "rounds": a.rounds,
           "decode_step_hip_graph": graphed, "vocab": int(logits.shape[-1]), "logits_row_stride": int(logits.stride(0)),
           "sample_launch_us": launch_us, "device": torch.cuda.get_device_name(0)}
    for name, ts in times.items():
        res[name] = benchlib.tokens_report(ts, a.batch, a.tokens, per="ms_per_new_token")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
