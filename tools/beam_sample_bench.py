#!/usr/bin/env python
"""Beam sampling (generate(num_beams > 1, do_sample=True)) beside plain beam search, with the method of tools/beam_bench.py.  One JSON line:

    step_us        ff_beam_sample_step and ff_beam_step alone, back to back on the same logits: 32 x 4 and 32 x 8 rows of 50 258 bf16 columns
                   (device events around --launches back-to-back calls, every beam alive, no eos).  `sample` = warpers off, `sample_warped`
                   = temperature 0.9, top_k 50, top_p 0.95 (both thresholds: 16 counting and up to 17 mass passes over the key image
                   before the two noise passes), `torch` = decoding.beam_sample_select_torch + order_by_score with
                   decoding.gumbel_noise_torch on the same rows (what the dynamic loop runs per step, without its host walk)
    sample / plain the static caption decode at the benchmark's geometry (tools/benchlib.caption_setup: config B, batch 32, bf16, a
                   4-token prompt) with 4 beams, with do_sample=True (temperature 0.9, top_k 50) and without: the call the code before
                   the feature served, which issues the launches it always did

Method of the caption arms: every path is warmed up with one full call (sessions built, graphs captured) and then timed with a host clock
around `--rounds` calls that each end in a device synchronise, ALTERNATING inside a round; the median per path with the spread (min .. max).
Needs the GPU: there is no fallback.

    python tools/beam_sample_bench.py [--tokens 32] [--rounds 5] [--skip-caption]
"""
import argparse
import json
import statistics

import torch

import benchlib


def step_table(launches, dev):
    from flamingo_mini_amd import decoding as D
    from flamingo_mini_amd import functional as F
    rows = {}
    gen = torch.Generator(device=dev).manual_seed(3)
    for nb in (4, 8):
        V = 50258
        logits = (torch.randn((32 * nb, V), generator=gen, device=dev) * 2).to(torch.bfloat16)
        cur = torch.full((1,), 5, dtype=torch.long, device=dev)
        seed = torch.full((1,), 1234, dtype=torch.long, device=dev)
        st = F.BeamState(32, nb, 40, dev)

        def one(call):
            st.score.zero_()                                                 # (every beam alive, as in the middle of a search)
            call()

        def restated():
            st.score.zero_()
            D.order_by_score(*D.beam_sample_select_torch(logits, st.score, D.gumbel_noise_torch((32 * nb, V), gen, dev), nb, 0.9, 50, 0.95), V)

        entry = {"beam_step": benchlib.launch_us(lambda: one(lambda: F.beam_step(logits, st, cur)), launches),
                 "sample": benchlib.launch_us(lambda: one(lambda: F.beam_sample_step(logits, st, cur, seed)), launches),
                 "sample_warped": benchlib.launch_us(lambda: one(lambda: F.beam_sample_step(logits, st, cur, seed, 0.9, 50, 0.95)), launches),
                 "torch": benchlib.launch_us(restated, max(launches // 10, 5)),
                 "beam_step_again": benchlib.launch_us(lambda: one(lambda: F.beam_step(logits, st, cur)), launches)}
        entry["sample_over_beam_step"] = round(entry["sample"] / entry["beam_step"], 2)
        entry["torch_over_sample_warped"] = round(entry["torch"] / entry["sample_warped"], 1)
        rows[f"32x{nb}"] = entry
    return rows


def main():
    ap = argparse.ArgumentParser()
    benchlib.caption_arguments(ap, "lm", "clip", "batch", "tokens", "rounds")
    ap.add_argument("--beams", type=int, default=4)
    ap.add_argument("--launches", type=int, default=100)
    ap.add_argument("--skip-caption", action="store_true")
    a = ap.parse_args()
    benchlib.need_gpu(__file__)
    dev, dt = torch.device("cuda"), torch.bfloat16
    res = {"device": torch.cuda.get_device_name(0), "launches": a.launches, "step_us": step_table(a.launches, dev)}
    if not a.skip_caption:
        model, ids, kw = benchlib.caption_setup(a, dev, dt)
        kw.update(num_beams=a.beams, static_decode=True)
        gen = torch.Generator(device=dev).manual_seed(0)
        paths = {"sample": lambda: model.generate(ids, do_sample=True, temperature=0.9, top_k=50, generator=gen, **kw),
                 "plain": lambda: model.generate(ids, **kw)}
        res["geometry"] = f"{a.lm}, batch {a.batch} x {a.beams} beams, prompt 4 + {a.tokens} new tokens, bf16, random-init backbones"
        res["rounds"] = a.rounds
        with torch.no_grad():
            times, outs = benchlib.host_rounds(paths, a.rounds)
        assert all(out.shape == (a.batch, kw["max_length"]) for out in outs.values())
        assert len(model._decode_sessions) == 2
        res["decode_step_hip_graph"] = all(benchlib.graphed(s) for s in model._decode_sessions.values())
        for name, ts in times.items():
            res[name] = benchlib.tokens_report(ts, a.batch, a.tokens)
        res["sample_minus_plain_ms_per_step"] = round(statistics.median(benchlib.round_diffs(times, "sample", "plain")) / a.tokens * 1e3, 3)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
