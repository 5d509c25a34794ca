#!/usr/bin/env python
"""Logits processors (repetition penalty 1.3, no-repeat bigrams, min_length) at the benchmark's caption geometry (config B: gpt2-large + CLIP
ViT-L/14, random-init backbones, batch 32, bf16, a 4-token prompt with the media tag first - bench.py's caption leg).  One JSON line:

    process_logits_us   ff_logits_process alone on 32 rows x 50 258 columns bf16 with histories of 32, 150 and 1024 tokens (device events
                        around --launches back-to-back calls; the logits are not restored between calls: a later call penalises the
                        penalised values again, with the same loads and stores)
    torch_chain_us      FlamingoModel._process_logits (decoding.process_logits), the torch restatement the dynamic loops use, on the same GPU and inputs: the op chain
                        the kernel replaces (cat, gather, where, scatter, unfold, compare, all, scatter)
    greedy_off / greedy_on   generate() on the static path without and with the processors: tokens/s and ms per replayed decode step

Method: as tools/beam_bench.py - every path is warmed up with one full call (sessions built, graphs captured), then timed with a host clock
around `--rounds` calls that each end in a device synchronise, ALTERNATING inside a round; the median is reported with the spread.  The
greedy_off figure is what the commit before the processors measured with the same command: run this file's greedy_off leg there
(`--only off` needs nothing of the feature) to compare.  Needs the GPU: there is no fallback.

    python tools/logits_process_bench.py [--tokens 32] [--rounds 5] [--only off]
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
    ap.add_argument("--only", choices=["off"], default=None, help="off: the processors-off decode leg alone (runs on a tree without the feature)")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("logits_process_bench.py measures on the GPU; none is visible")
    import bench
    dev, dt = torch.device("cuda"), torch.bfloat16
    margs = argparse.Namespace(lm=a.lm, clip=a.clip, xattn_every=1, lm_dropout=None, backbone_tweaks="off", batch=a.batch, seq_len=32, images=1, frames=0)
    model, cfg = bench.build_model(margs, dev, dt)
    model.eval()
    batch = bench.synthetic_batch(margs, cfg, dev, dt, 0)
    ids, ml, am = batch["input_ids"][:, :4], batch["media_locations"][:, :4], batch["attention_mask"][:, :4]
    L = 4 + a.tokens
    kw = dict(media_locations=ml, attention_mask=am, pixel_values=batch["pixel_values"], max_length=L)
    proc = dict(repetition_penalty=1.3, no_repeat_ngram_size=2, min_length=L // 2, eos_token_id=50256, pad_token_id=50256)
    paths = {"greedy_off": lambda: model.generate(ids, **kw)}
    if a.only is None:
        paths["greedy_on"] = lambda: model.generate(ids, **proc, **kw)
    res = {"geometry": f"{a.lm}, batch {a.batch}, prompt 4 + {a.tokens} new tokens, bf16, random-init backbones", "rounds": a.rounds,
           "device": torch.cuda.get_device_name(0)}
    times = {k: [] for k in paths}
    with torch.no_grad():
        for fn in paths.values():
            fn()
        torch.cuda.synchronize()
        for _ in range(a.rounds):
            for name, fn in paths.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                times[name].append(time.perf_counter() - t0)
        res["decode_step_hip_graph"] = all(s.replay is not None and not s.capture_failed for s in model._decode_sessions.values())
        if a.only is None:
            from flamingo_mini_amd import functional as F
            from flamingo_mini_amd.modeling_flamingo import FlamingoModel
            V = 50258
            g = torch.Generator(device="cuda").manual_seed(0)
            logits = (torch.randn((a.batch, V), generator=g, device=dev) * 4).to(dt)
            hist = torch.randint(0, V, (a.batch, 1024), generator=g, device=dev)
            min_len = torch.full((1,), 2048, dtype=torch.long, device=dev)

            def timed(fn):
                for _ in range(5):
                    fn()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize()
                e0.record()
                for _ in range(a.launches):
                    fn()
                e1.record()
                torch.cuda.synchronize()
                return round(e0.elapsed_time(e1) / a.launches * 1e3, 1)

            res["process_logits_us"], res["torch_chain_us"] = {}, {}
            for n in (32, 150, 1024):
                n_dev = torch.full((1,), n, dtype=torch.long, device=dev)
                h = hist[:, :n].contiguous()
                x32 = logits.float()
                res["process_logits_us"][n] = timed(lambda: F.process_logits(logits, h, n_dev, 1.3, 2, 50256, min_len))
                res["torch_chain_us"][n] = timed(lambda: FlamingoModel._process_logits(x32, h, 1.3, 2, 50256, 2048))
    for name, ts in times.items():
        n = a.batch * a.tokens
        res[name] = {"tokens_per_s": round(n / statistics.median(ts), 1), "min": round(n / max(ts), 1), "max": round(n / min(ts), 1),
                     "ms_per_decode_step": round(statistics.median(ts) / a.tokens * 1e3, 3)}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
