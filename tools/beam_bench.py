#!/usr/bin/env python
"""Beam-search caption decoding at the benchmark's geometry (config B: gpt2-large + CLIP ViT-L/14, random-init backbones, batch 32, bf16,
a 4-token prompt with the media tag first - bench.py's caption leg), 3 beams, no eos (every call runs to the length limit).  One JSON line:

    dynamic_beam   generate(num_beams=3): the growing-cache loop (decoding.beam_search: log_softmax + topk, a host copy and a Python walk per step,
                   torch.cat, index_select of every cache tensor)
    static_beam    generate(num_beams=3, static_decode=True): the fixed-shape session, one decode step replayed from a HIP graph with
                   ff_beam_step and ff_beam_gather inside it
    beam_step_us / beam_gather_us   the two calls alone, on the model's own prompt-step logits and on the session's own static cache at its
                   full length (device events around --launches back-to-back calls)

Method: both paths are warmed up with one full call (sessions built, graphs captured, code objects loaded) and then timed with a host clock
around `--rounds` calls that each end in a device synchronise, ALTERNATING inside a round; the median per path is reported with the spread
(min .. max).  `--only static` runs the static path alone (for a kernel trace).  Needs the GPU: there is no fallback.

    python tools/beam_bench.py [--tokens 32] [--rounds 5] [--only static]
"""
import argparse
import json

import torch

import benchlib


def main():
    ap = argparse.ArgumentParser()
    benchlib.caption_arguments(ap, "lm", "clip", "batch")
    ap.add_argument("--beams", type=int, default=3)
    benchlib.caption_arguments(ap, "tokens", "rounds")
    ap.add_argument("--launches", type=int, default=100)
    ap.add_argument("--only", choices=["static", "dynamic"], default=None)
    a = ap.parse_args()
    benchlib.need_gpu(__file__)
    from flamingo_mini_amd import functional as F
    dev, dt = torch.device("cuda"), torch.bfloat16
    model, ids, kw = benchlib.caption_setup(a, dev, dt)
    L = kw["max_length"]
    prompt = {"input_ids": ids, **{k: kw[k] for k in ("attention_mask", "media_locations", "pixel_values")}}
    kw["num_beams"] = a.beams
    paths = {"dynamic_beam": lambda: model.generate(ids, **kw), "static_beam": lambda: model.generate(ids, static_decode=True, **kw)}
    if a.only:
        paths = {k: v for k, v in paths.items() if k.startswith(a.only)}
    res = {"geometry": f"{a.lm}, batch {a.batch} x {a.beams} beams, prompt 4 + {a.tokens} new tokens, bf16, random-init backbones",
           "rounds": a.rounds, "device": torch.cuda.get_device_name(0)}
    with torch.no_grad():
        times, outs = benchlib.host_rounds(paths, a.rounds)
        for out in outs.values():
            assert out.shape == (a.batch, L), out.shape
        if len(outs) == 2:
            res["rows_equal"] = int((outs["dynamic_beam"] == outs["static_beam"]).all(1).sum())
        sess = [s for s in model._decode_sessions.values() if s.beams is not None]
        if sess:
            s = sess[0]
            res["decode_step_hip_graph"] = benchlib.graphed(s)
            logits = model.flamingo(**{k: v.repeat_interleave(a.beams, 0) for k, v in prompt.items()}).logits[:, -1]
            cur = torch.full((1,), 5, dtype=torch.long, device=dev)
            n_pos = torch.full((1,), L - 1, dtype=torch.long, device=dev)
            rot = torch.arange(a.batch * a.beams, device=dev)
            rot = rot // a.beams * a.beams + (rot % a.beams + 1) % a.beams          # every row moves: the gather's most expensive case

            def step():
                s.state.score.zero_()                                                # (every beam alive, as in the middle of a search)
                F.beam_step(logits, s.state, cur)

            res["beam_step_us"] = benchlib.launch_us(step, a.launches)
            res["beam_gather_us"] = benchlib.launch_us(lambda: F.beam_gather(s.lm_tensors, rot, n_pos, a.beams), a.launches)
            res["gather_bytes_moved"] = 2 * sum(t[:, :, :L - 1].numel() * t.element_size() for t in s.lm_tensors)
            res["vocab"], res["cache_tensors"] = int(logits.shape[-1]), len(s.lm_tensors)
    for name, ts in times.items():
        res[name] = benchlib.tokens_report(ts, a.batch, a.tokens)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
