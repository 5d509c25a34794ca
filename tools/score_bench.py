#!/usr/bin/env python
"""Exact closed-set scoring (FlamingoModel.score_candidates, ff_logprob_gather).  One JSON line:

    kernel              functional.logprob_gather (out= given, base given) on 1024 x 50 258 bf16 rows (randn x 4) with 1, 8 and 300 queries per
                        row: microseconds per launch and the rate at which the logits are read (rows x vocab x 2 bytes over the launch
                        time).  The call rotates over --buffers logits tensors (4 x 103 MB: more than the 256 MiB last-level cache holds),
                        so the figure is a read from HBM and not from that cache; "one_buffer" is the same launch on one tensor.
                        --launches calls are captured into one HIP graph, replayed --replays times between two device events
                        (benchlib.launch_us).  Beside it "torch_chain": logits.float().log_softmax(-1).gather(1, tok) + base[:, None] on
                        the same logits, the chain the launch replaces (eager, events around --launches calls), and the peak allocation
                        of one call of each.
    score_candidates    gpt2-large + ViT-L/14 geometry, random-init backbones, bf16, a 4-token prompt: --candidates synthetic candidates of
                        1 - 5 tokens with shared first tokens (seeded), batch 1 and batch 8, max_rows 256 / 1024 / 4096: seconds per call
                        (benchlib.host_rounds: one warm-up call per path, then --rounds rounds with the paths alternating, host clock
                        around calls that end in a synchronise; median, min .. max), torch.cuda.max_memory_allocated over one call minus
                        what was allocated before it, the number of groups, LM steps and gather launches, the widest level.
    score_sequences     the reference's method on the same candidates (padded with the LM's eos to 5 tokens: it sums padded positions), ONE
                        image per call - its only form -, same rounds; its peak allocation the same way.
    levels              one score_candidates call (batch 8, max_rows 4096) with a synchronise around every LM step and every gather: rows,
                        milliseconds in the LM step, milliseconds in the gather, what the gather allocated at its peak beside the size of
                        a float32 (rows, vocab) tensor - the temporary the path does not make -, and the path the gated blocks' feed-forward takes at that
                        row count (the library's dispatch rule, csrc/ff_decode.hip decode_ffw_supported: at most 32 rows take the two
                        decode launches, more take the GEMM tiles).
    greedy_decode       generate(static_decode=True), batch 32, 4 + 32 tokens: the default greedy call, which needs nothing of the feature -
                        `--only decode` runs on the commit before it as well, for the comparison against the parent.

Needs the GPU: there is no fallback.

    python tools/score_bench.py [--rounds 5] [--only kernel | decode]
"""
import argparse
import json
import statistics
import time

import numpy as np
import torch

import benchlib

V = 50258
DEV = torch.device("cuda")


def synthetic_candidates(n, vocab, seed=0, firsts=40, pool=30):
    """n distinct candidates of 1 - 5 tokens: the first token one of `firsts`, every later token one of `pool` (so prefixes are shared the
    way class names share first tokens); ids below vocab - 8 (clear of eos and the tags)"""
    rng = np.random.default_rng(seed)
    first = rng.choice(vocab - 8, firsts, replace=False)
    later = rng.choice(vocab - 8, pool, replace=False)
    out = set()
    while len(out) < n:
        length = int(rng.integers(1, 6))
        out.add((int(rng.choice(first)),) + tuple(int(t) for t in rng.choice(later, length - 1)))
    return [list(c) for c in sorted(out)]


def peak_of(fn):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    out = fn()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - before
    del out
    return round(peak / 2 ** 20, 1)


def kernel_leg(a, res):
    from flamingo_mini_amd import functional as F
    dev, rows = DEV, a.rows
    g = torch.Generator(device="cuda").manual_seed(0)
    bufs = [(torch.randn((rows, V), generator=g, device=dev) * 4).to(torch.bfloat16) for _ in range(a.buffers)]
    base = torch.randn(rows, generator=g, device=dev)
    res["kernel"] = {"rows": rows, "vocab": V, "dtype": "bf16", "buffers": a.buffers, "window": f"graph replay, {a.launches * a.replays} calls per figure"}
    mb = rows * V * 2 / 1e6
    for q in (1, 8, 300):
        tok = torch.randint(0, V, (rows, q), generator=g, device=dev)
        tok32 = tok.to(torch.int32).reshape(-1).contiguous()
        row_first = (torch.arange(rows + 1, device=dev) * q).to(torch.int32)
        out = torch.empty(rows * q, device=dev)
        turn = [0]

        def rotating():
            turn[0] = (turn[0] + 1) % len(bufs)
            F.logprob_gather(bufs[turn[0]], row_first, tok32, base=base, out=out)

        launches = a.launches - a.launches % len(bufs)                        # (the captured graph holds whole rotations)
        us = benchlib.launch_us(rotating, launches, a.replays)
        one = benchlib.launch_us(lambda: F.logprob_gather(bufs[0], row_first, tok32, base=base, out=out), launches, a.replays)
        chain = lambda: bufs[0].float().log_softmax(-1).gather(1, tok) + base[:, None]
        same = torch.allclose(chain().reshape(-1), F.logprob_gather(bufs[0], row_first, tok32, base=base), rtol=0, atol=1e-4)
        chain_us = benchlib.launch_us(chain, 20, eager=True)
        res["kernel"][f"q{q}"] = {"launch_us": us, "read_TB_per_s": round(mb / us, 2), "one_buffer_us": one, "torch_chain_us": chain_us,
                                  "torch_over_kernel": round(chain_us / us, 1), "agrees_with_torch_to_1e-4": bool(same),
                                  "peak_MiB": {"kernel": peak_of(lambda: F.logprob_gather(bufs[0], row_first, tok32, base=base)), "torch_chain": peak_of(chain)}}
        del tok, tok32, out


def summary(ts):
    return {"s": round(statistics.median(ts), 4), "min": round(min(ts), 4), "max": round(max(ts), 4)}


def model_leg(a, res):
    from flamingo_mini_amd import functional as F
    dev, dt = DEV, torch.bfloat16
    a.batch = 8
    model, ids, kw = benchlib.caption_setup(a, dev, dt)
    ml, am, px = kw["media_locations"], kw["attention_mask"], kw["pixel_values"]
    vocab, eos = model.flamingo.lm.config.vocab_size, model.flamingo.lm.config.eos_token_id
    cands = synthetic_candidates(a.candidates, vocab)
    lengths = [len(c) for c in cands]
    res["candidates"] = {"n": len(cands), "tokens": sum(lengths), "distinct_prefixes": len({tuple(c[:i]) for c in cands for i in range(1, len(c) + 1)}),
                         "first_tokens": len({c[0] for c in cands}), "by_length": [lengths.count(n) for n in range(1, 6)]}
    res["geometry"] = f"{a.lm}, prompt 4 tokens, bf16, random-init backbones, vocabulary {vocab}"
    counts = {}

    def counted(b, max_rows):
        calls = {"lm_steps": 0, "gathers": 0, "widest": 0, "groups": 0}
        step, gather = model._score_step, F.logprob_gather

        def _step(step_ids, *rest):
            calls["lm_steps"] += 1
            calls["groups"] += step_ids.shape[1] > 1
            calls["widest"] = max(calls["widest"], step_ids.shape[0])
            return step(step_ids, *rest)

        def _gather(*args, **kws):
            calls["gathers"] += 1
            return gather(*args, **kws)

        model._score_step, F.logprob_gather = _step, _gather
        try:
            model.score_candidates(ids[:b], ml[:b], am[:b], pixel_values=px[:b], candidate_ids=cands, max_rows=max_rows)
        finally:
            del model._score_step
            F.logprob_gather = gather
        return calls

    paths = {}
    for b in (1, 8):
        for max_rows in (256, 1024, 4096):
            name = f"b{b}_max_rows{max_rows}"
            paths[name] = (lambda b=b, m=max_rows: model.score_candidates(ids[:b], ml[:b], am[:b], pixel_values=px[:b], candidate_ids=cands, max_rows=m))
            counts[name] = counted(b, max_rows)
    longest = max(lengths)
    seq_ids = torch.tensor([ids[0].tolist() + c + [eos] * (longest - len(c)) for c in cands], device=dev)
    seq_ml = torch.cat([ml[:1].expand(len(cands), -1), torch.zeros((len(cands), longest), dtype=ml.dtype, device=dev)], dim=1)
    seq_am = torch.ones_like(seq_ids)
    paths["score_sequences_one_image"] = lambda: model.score_sequences(seq_ids, seq_ml, seq_am, pixel_values=px[0])
    with torch.no_grad():
        times, _ = benchlib.host_rounds(paths, a.rounds)
        res["rounds"] = a.rounds
        res["score_candidates"] = {name: dict(summary(ts), peak_MiB=peak_of(paths[name]), **counts[name]) for name, ts in times.items() if name in counts}
        res["score_sequences"] = dict(summary(times["score_sequences_one_image"]), peak_MiB=peak_of(paths["score_sequences_one_image"]), images_per_call=1)
        res["rows_x_vocab_x_4_MiB"] = {name: round(c["widest"] * vocab * 4 / 2 ** 20, 1) for name, c in counts.items()}
        # one call with a synchronise around every LM step and every gather
        levels, step, gather = [], model._score_step, F.logprob_gather

        def clocked(fn, key):
            def run(*args, **kws):
                torch.cuda.synchronize()
                torch.cuda.reset_peak_memory_stats()
                before = torch.cuda.memory_allocated()
                t0 = time.perf_counter()
                out = fn(*args, **kws)
                torch.cuda.synchronize()
                took = time.perf_counter() - t0
                if key == "lm_ms":
                    path = "prompt step (uncached blocks)" if args[3] is None else "decode launches (<= 32 rows)" if args[0].numel() <= 32 else "GEMM tiles"
                    levels.append({"rows": args[0].shape[0], "ffw_path": path})
                else:                                                      # what the gather allocated at its peak, beside a float32 (rows, V)
                    levels[-1]["gather_peak_MiB"] = round((torch.cuda.max_memory_allocated() - before) / 2 ** 20, 2)
                    levels[-1]["rows_x_vocab_x_4_MiB"] = round(args[0].shape[0] * args[0].shape[1] * 4 / 2 ** 20, 1)
                levels[-1][key] = round(took * 1e3, 3)
                return out
            return run

        model._score_step, F.logprob_gather = clocked(step, "lm_ms"), clocked(gather, "gather_ms")
        try:
            model.score_candidates(ids, ml, am, pixel_values=px, candidate_ids=cands, max_rows=4096)
        finally:
            del model._score_step
            F.logprob_gather = gather
        res["levels_b8_max_rows4096"] = levels


def decode_leg(a, res):
    dev, dt = DEV, torch.bfloat16
    a.batch = 32
    model, ids, kw = benchlib.caption_setup(a, dev, dt)
    with torch.no_grad():
        times, _ = benchlib.host_rounds({"greedy_decode": lambda: model.generate(ids, static_decode=True, **kw)}, a.rounds)
    res["greedy_decode"] = dict(benchlib.tokens_report(times["greedy_decode"], a.batch, a.tokens),
                                decode_step_hip_graph=all(benchlib.graphed(s) for s in model._decode_sessions.values()))


def main():
    ap = argparse.ArgumentParser()
    benchlib.caption_arguments(ap, "lm", "clip", "tokens", "rounds")
    ap.add_argument("--candidates", type=int, default=1000)
    ap.add_argument("--rows", type=int, default=1024, help="rows of the kernel leg")
    ap.add_argument("--buffers", type=int, default=4, help="logits tensors the kernel leg rotates over")
    ap.add_argument("--launches", type=int, default=40, help="calls captured into the timed graph")
    ap.add_argument("--replays", type=int, default=10, help="replays of that graph inside the timed window")
    ap.add_argument("--only", choices=["kernel", "decode"], default=None,
                    help="kernel: the launch timings alone, no model; decode: the default greedy decode leg alone (runs on a tree without the feature)")
    ap.add_argument("--out", default=None, help="also write the line to this file")
    a = ap.parse_args()
    benchlib.need_gpu(__file__)
    res = {"device": torch.cuda.get_device_name(0)}
    if a.only in (None, "kernel"):
        with torch.no_grad():
            kernel_leg(a, res)
    if a.only is None:
        model_leg(a, res)
        torch.cuda.empty_cache()
    if a.only in (None, "decode"):
        decode_leg(a, res)
    benchlib.emit(json.dumps(res), a.out)


if __name__ == "__main__":
    main()
