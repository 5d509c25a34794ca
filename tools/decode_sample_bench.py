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
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lm", default="gpt2-large")
    ap.add_argument("--clip", default="openai/clip-vit-large-patch14")
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--tokens", type=int, default=32, help="new tokens per image")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--temperature", type=float, default=0.8)
    ap.add_argument("--top-k", type=int, default=50)
    ap.add_argument("--top-p", type=float, default=0.9)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("decode_sample_bench.py measures on the GPU; none is visible")
    import bench
    from flamingo_mini_amd import functional as F
    dev, dt = torch.device("cuda"), torch.bfloat16
    margs = argparse.Namespace(lm=a.lm, clip=a.clip, xattn_every=1, lm_dropout=None, backbone_tweaks="off", batch=a.batch, seq_len=32, images=1, frames=0)
    model, cfg = bench.build_model(margs, dev, dt)
    model.eval()
    batch = bench.synthetic_batch(margs, cfg, dev, dt, 0)
    ids, ml, am = batch["input_ids"][:, :4], batch["media_locations"][:, :4], batch["attention_mask"][:, :4]
    px = batch["pixel_values"]
    L = 4 + a.tokens
    sk = dict(do_sample=True, temperature=a.temperature, top_k=a.top_k, top_p=a.top_p)
    gen = torch.Generator(device="cuda")

    def dynamic():
        return model.generate(ids, media_locations=ml, attention_mask=am, pixel_values=px, max_length=L, generator=gen.manual_seed(1), **sk)

    def static():
        return model.generate(ids, media_locations=ml, attention_mask=am, pixel_values=px, max_length=L, generator=gen.manual_seed(1),
                              static_decode=True, **sk)

    def greedy():
        return model.greedy_generate(ids, ml, am, pixel_values=px, max_length=L)

    paths = {"dynamic_sampling": dynamic, "static_sampling": static, "static_greedy": greedy}
    times = {k: [] for k in paths}
    with torch.no_grad():
        for fn in paths.values():
            out = fn()
            assert out.shape == (a.batch, L), out.shape
        torch.cuda.synchronize()
        for _ in range(a.rounds):
            for name, fn in paths.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                times[name].append(time.perf_counter() - t0)
        sessions = list(model._decode_sessions.values())
        graphed = {("sampling" if s.sampling is not None else "greedy"): s.replay is not None and not s.capture_failed for s in sessions}

        # the launch alone, on the logits the model really produces for this prompt
        logits = model.flamingo(input_ids=ids, attention_mask=am, media_locations=ml, pixel_values=px).logits[:, -1]
        u = torch.rand(a.batch, device=dev)
        tok = torch.empty(a.batch, dtype=torch.long, device=dev)
        for _ in range(10):
            F.sample_tokens(logits, u, a.temperature, a.top_k, a.top_p, out=tok)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(a.launches):
            F.sample_tokens(logits, u, a.temperature, a.top_k, a.top_p, out=tok)
        e1.record()
        torch.cuda.synchronize()
        launch_us = e0.elapsed_time(e1) / a.launches * 1e3

    res = {"geometry": f"{a.lm}, batch {a.batch}, prompt 4 + {a.tokens} new tokens, bf16, random-init backbones",
           "sampling": {"temperature": a.temperature, "top_k": a.top_k, "top_p": a.top_p}, "rounds": a.rounds,
           "decode_step_hip_graph": graphed, "vocab": int(logits.shape[-1]), "logits_row_stride": int(logits.stride(0)),
           "sample_launch_us": round(launch_us, 1), "device": torch.cuda.get_device_name(0)}
    for name, ts in times.items():
        n = a.batch * a.tokens
        res[name] = {"tokens_per_s": round(n / statistics.median(ts), 1), "min": round(n / max(ts), 1), "max": round(n / min(ts), 1),
                     "ms_per_new_token": round(statistics.median(ts) / a.tokens * 1e3, 3)}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
