#!/usr/bin/env python
"""Contrastive search (generate(penalty_alpha=, top_k=)) beside 4-beam search and greedy decoding, with the method of
tools/beam_sample_bench.py.  One JSON line:

    step_us        what a contrastive decode step adds to the LM, each launch alone, back to back (device events around --launches calls):
                   32 sequences x 4 candidates, dim 1024, bf16, at n = 32 and n = 150 positions of history: `contrastive_step`
                   (ff_contrastive_step), `topk_logprobs` (ff_topk_logprob on 32 rows of 50 258 bf16 columns), `index_select` (the chosen
                   rows' logits out of 128), and `torch` = decoding.contrastive_select_torch + topk_logprobs_torch on the same data (what
                   the dynamic loop runs per step)
    contrastive /  the static caption decode at the benchmark's geometry (tools/benchlib.caption_setup: config B, batch 32, bf16, a
    beams / greedy 4-token prompt): contrastive search with k = 4, alpha = 0.6; 4-beam search; greedy decoding - the call the code before the
    / dynamic      feature served, which issues the launches it always did -; and the dynamic contrastive loop (growing caches)

Method of the caption arms: every path is warmed up with one full call (sessions built, graphs captured) and then timed with a host clock
around `--rounds` calls that each end in a device synchronise, ALTERNATING inside a round; the median per path with the spread (min .. max).
Needs the GPU: there is no fallback.

    python tools/contrastive_bench.py [--tokens 32] [--rounds 5] [--skip-caption] [--skip-dynamic]
"""
import argparse
import json
import statistics

import torch

import benchlib


def step_table(launches, dev):
    from flamingo_mini_amd import decoding as D
    from flamingo_mini_amd import functional as F
    b, k, dim, V, max_len = 32, 4, 1024, 50258, 160
    gen = torch.Generator(device=dev).manual_seed(3)
    bf = torch.bfloat16
    hidden = torch.randn((b * k, dim), generator=gen, device=dev).to(bf)
    hist = torch.randn((b, max_len, dim), generator=gen, device=dev).to(bf)
    mask = torch.ones((b, max_len), dtype=torch.bool, device=dev)
    logits = (torch.randn((b * k, V), generator=gen, device=dev) * 2).to(bf)
    next_logits = torch.empty((b, V), dtype=bf, device=dev)
    tok, lp = torch.zeros((b, k), dtype=torch.long, device=dev), torch.zeros((b, k), device=dev)
    F.topk_logprobs(logits[::k], k, out=(tok, lp))
    fin = torch.zeros(b, dtype=torch.bool, device=dev)
    alpha, n_pos = torch.full((1,), 0.6, device=dev), torch.zeros(1, dtype=torch.long, device=dev)
    out = (torch.zeros(b, dtype=torch.long, device=dev), torch.zeros(b, device=dev), torch.zeros(b, dtype=torch.long, device=dev),
           torch.zeros(b * k, dtype=torch.long, device=dev))
    next_logits.copy_(logits[::k])
    rows = {"topk_logprobs": benchlib.launch_us(lambda: F.topk_logprobs(next_logits, k, out=(tok, lp)), launches)}
    rows["index_select"] = benchlib.launch_us(lambda: torch.index_select(logits, 0, out[2], out=next_logits), launches)
    rows["topk_torch"] = benchlib.launch_us(lambda: D.topk_logprobs_torch(next_logits, k), max(launches // 10, 5))
    for n in (32, 150):
        n_pos.fill_(n)
        entry = {"contrastive_step": benchlib.launch_us(lambda: F.contrastive_step(hidden, hist, mask, tok, lp, fin, alpha, n_pos, out=out), launches),
                 "torch": benchlib.launch_us(lambda: D.contrastive_select_torch(hidden, hist[:, :n], mask[:, :n], tok, lp, fin, 0.6), max(launches // 10, 5))}
        entry["torch_over_kernel"] = round(entry["torch"] / entry["contrastive_step"], 1)
        rows[f"n{n}"] = entry
    return rows


def main():
    ap = argparse.ArgumentParser()
    benchlib.caption_arguments(ap, "lm", "clip", "batch", "tokens", "rounds")
    ap.add_argument("--k", type=int, default=4)
    ap.add_argument("--alpha", type=float, default=0.6)
    ap.add_argument("--launches", type=int, default=100)
    ap.add_argument("--skip-caption", action="store_true")
    ap.add_argument("--skip-dynamic", action="store_true")
    a = ap.parse_args()
    benchlib.need_gpu(__file__)
    dev, dt = torch.device("cuda"), torch.bfloat16
    res = {"device": torch.cuda.get_device_name(0), "launches": a.launches, "step_us": step_table(a.launches, dev)}
    if not a.skip_caption:
        model, ids, kw = benchlib.caption_setup(a, dev, dt)
        paths = {"contrastive": lambda: model.generate(ids, penalty_alpha=a.alpha, top_k=a.k, static_decode=True, **kw),
                 "beams": lambda: model.generate(ids, num_beams=a.k, static_decode=True, **kw),
                 "greedy": lambda: model.generate(ids, **kw)}
        if not a.skip_dynamic:
            paths["dynamic"] = lambda: model.generate(ids, penalty_alpha=a.alpha, top_k=a.k, static_decode=False, **kw)
        res["geometry"] = f"{a.lm}, batch {a.batch} x {a.k} candidates / beams, prompt 4 + {a.tokens} new tokens, bf16, random-init backbones"
        res["rounds"] = a.rounds
        with torch.no_grad():
            times, outs = benchlib.host_rounds(paths, a.rounds)
        assert all(outs[name].shape == (a.batch, kw["max_length"]) for name in outs if name != "beams")
        assert len(model._decode_sessions) == 3
        res["decode_step_hip_graph"] = all(benchlib.graphed(s) for s in model._decode_sessions.values())
        res["static_equals_dynamic"] = bool(torch.equal(outs["contrastive"], outs["dynamic"])) if "dynamic" in outs else None
        for name, ts in times.items():
            res[name] = benchlib.tokens_report(ts, a.batch, a.tokens)
        res["contrastive_over_beams"] = round(statistics.median(times["contrastive"]) / statistics.median(times["beams"]), 3)
        res["contrastive_minus_beams_ms_per_step"] = round(statistics.median(benchlib.round_diffs(times, "contrastive", "beams")) / a.tokens * 1e3, 3)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
