#!/usr/bin/env python
"""Diverse beam search (generate(num_beam_groups=G)) beside plain beam search, with the method of tools/beam_bench.py.  One JSON line:

    step_us        ff_group_beam_step and ff_beam_step alone, back to back on the same logits: 32 x 4 and 32 x 8 rows of 50 258 bf16 columns,
                   G in {2, 4, 8} where it divides the beams (device events around --launches back-to-back calls, every beam alive, no eos).
                   Both run the same row pass (beam_rows_kernel, K = 2 nb); the difference is the merge: one ranking of nb x 2 nb
                   candidates and one walk (beam_merge_kernel) against G rankings of gs x 2 nb and G walks in sequence (group_merge_kernel)
    groups / one_group / plain   the static caption decode at the benchmark's geometry (tools/benchlib.caption_setup: config B, batch 32,
                   bf16, a 4-token prompt) with 4 beams: num_beam_groups=4 with diversity_penalty=1, num_beam_groups=1 passed explicitly,
                   and the call without group arguments - the call the code before the feature served.  The last two take one and the
                   same path (decoding.check_group_args returns None): their difference is the box's noise, and `plain_spread` reports it

Method of the caption arms: every path is warmed up with one full call (sessions built, graphs captured) and then timed with a host clock
around `--rounds` calls that each end in a device synchronise, ALTERNATING inside a round; the median per path with the spread (min .. max).
Needs the GPU: there is no fallback.

    python tools/group_beam_bench.py [--tokens 32] [--rounds 5] [--skip-caption]
"""
import argparse
import json
import statistics

import torch

import benchlib


def step_table(launches, dev):
    from flamingo_mini_amd import functional as F
    rows = {}
    gen = torch.Generator(device=dev).manual_seed(3)
    for nb in (4, 8):
        logits = (torch.randn((32 * nb, 50258), generator=gen, device=dev) * 2).to(torch.bfloat16)
        cur = torch.full((1,), 5, dtype=torch.long, device=dev)
        plain = F.BeamState(32, nb, 40, dev)

        def one(state=plain, call=lambda s: F.beam_step(logits, s, cur)):
            state.score.zero_()                                              # (every beam alive, as in the middle of a search)
            call(state)

        entry = {"beam_step": benchlib.launch_us(one, launches)}
        for G in (2, 4, 8):
            if nb % G == 0:
                st = F.BeamState(32, nb, 40, dev, n_groups=G)
                entry[f"group_beam_step_G{G}"] = benchlib.launch_us(lambda: one(st, lambda s: F.group_beam_step(logits, s, cur, 1.0)), launches)
        entry["beam_step_again"] = benchlib.launch_us(one, launches)         # (the yardstick once more: what two runs of one call differ by)
        rows[f"32x{nb}"] = entry
    return rows


def main():
    ap = argparse.ArgumentParser()
    benchlib.caption_arguments(ap, "lm", "clip", "batch", "tokens", "rounds")
    ap.add_argument("--beams", type=int, default=4)
    ap.add_argument("--groups", type=int, default=4)
    ap.add_argument("--launches", type=int, default=100)
    ap.add_argument("--skip-caption", action="store_true")
    a = ap.parse_args()
    benchlib.need_gpu(__file__)
    dev, dt = torch.device("cuda"), torch.bfloat16
    res = {"device": torch.cuda.get_device_name(0), "launches": a.launches, "step_us": step_table(a.launches, dev)}
    if not a.skip_caption:
        model, ids, kw = benchlib.caption_setup(a, dev, dt)
        kw.update(num_beams=a.beams, static_decode=True)
        paths = {"groups": lambda: model.generate(ids, num_beam_groups=a.groups, diversity_penalty=1.0, **kw),
                 "one_group": lambda: model.generate(ids, num_beam_groups=1, **kw),
                 "plain": lambda: model.generate(ids, **kw)}
        res["geometry"] = f"{a.lm}, batch {a.batch} x {a.beams} beams ({a.groups} groups), prompt 4 + {a.tokens} new tokens, bf16, random-init backbones"
        res["rounds"] = a.rounds
        with torch.no_grad():
            times, outs = benchlib.host_rounds(paths, a.rounds)
        assert all(out.shape == (a.batch, kw["max_length"]) for out in outs.values())
        assert torch.equal(outs["one_group"], outs["plain"])
        keys = list(model._decode_sessions)
        assert len(keys) == 2 and sum(k[-1] == (a.groups, 1.0) for k in keys) == 1, keys          # one_group and plain share a session
        res["decode_step_hip_graph"] = all(benchlib.graphed(s) for s in model._decode_sessions.values())
        res["rows_groups_equal_plain"] = int((outs["groups"] == outs["plain"]).all(1).sum())
        for name, ts in times.items():
            res[name] = benchlib.tokens_report(ts, a.batch, a.tokens)
        res["plain_spread_ms_per_step"] = round(benchlib.aa_spread(benchlib.round_diffs(times, "one_group", "plain")) / a.tokens * 1e3, 3)
        res["one_group_minus_plain_ms_per_step"] = round(statistics.median(benchlib.round_diffs(times, "one_group", "plain")) / a.tokens * 1e3, 3)
        res["groups_minus_plain_ms_per_step"] =round(statistics.median(benchlib.round_diffs(times, "groups", "plain")) / a.tokens * 1e3, 3)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
