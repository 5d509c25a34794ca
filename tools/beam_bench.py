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
    ap.add_argument("--beams", type=int, default=3)
    ap.add_argument("--tokens", type=int, default=32, help="new tokens per image")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--launches", type=int, default=100)
    ap.add_argument("--only", choices=["static", "dynamic"], default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("beam_bench.py measures on the GPU; none is visible")
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
    kw = dict(media_locations=ml, attention_mask=am, pixel_values=px, max_length=L, num_beams=a.beams)
    paths = {"dynamic_beam": lambda: model.generate(ids, **kw), "static_beam": lambda: model.generate(ids, static_decode=True, **kw)}
    if a.only:
        paths = {k: v for k, v in paths.items() if k.startswith(a.only)}
    times = {k: [] for k in paths}
    res = {"geometry": f"{a.lm}, batch {a.batch} x {a.beams} beams, prompt 4 + {a.tokens} new tokens, bf16, random-init backbones",
           "rounds": a.rounds, "device": torch.cuda.get_device_name(0)}
    with torch.no_grad():
        outs = {}
        for name, fn in paths.items():
            outs[name] = fn()
            assert outs[name].shape == (a.batch, L), outs[name].shape
        if len(outs) == 2:
            res["rows_equal"] = int((outs["dynamic_beam"] == outs["static_beam"]).all(1).sum())
        torch.cuda.synchronize()
        for _ in range(a.rounds):
            for name, fn in paths.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                times[name].append(time.perf_counter() - t0)
        sess = [s for s in model._decode_sessions.values() if s.beams is not None]
        if sess:
            s = sess[0]
            res["decode_step_hip_graph"] = s.replay is not None and not s.capture_failed
            logits = model.flamingo(input_ids=ids.repeat_interleave(a.beams, 0), attention_mask=am.repeat_interleave(a.beams, 0),
                                    media_locations=ml.repeat_interleave(a.beams, 0), pixel_values=px.repeat_interleave(a.beams, 0)).logits[:, -1]
            cur = torch.full((1,), 5, dtype=torch.long, device=dev)
            n_pos = torch.full((1,), L - 1, dtype=torch.long, device=dev)
            rot = torch.arange(a.batch * a.beams, device=dev)
            rot = rot // a.beams * a.beams + (rot % a.beams + 1) % a.beams          # every row moves: the gather's most expensive case

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

            def step():
                s.state.score.zero_()                                                # (every beam alive, as in the middle of a search)
                F.beam_step(logits, s.state, cur)

            res["beam_step_us"] = timed(step)
            res["beam_gather_us"] = timed(lambda: F.beam_gather(s.lm_tensors, rot, n_pos, a.beams))
            res["gather_bytes_moved"] = 2 * sum(t[:, :, :L - 1].numel() * t.element_size() for t in s.lm_tensors)
            res["vocab"], res["cache_tensors"] = int(logits.shape[-1]), len(s.lm_tensors)
    for name, ts in times.items():
        n = a.batch * a.tokens
        res[name] = {"tokens_per_s": round(n / statistics.median(ts), 1), "min": round(n / max(ts), 1), "max": round(n / min(ts), 1),
                     "ms_per_decode_step": round(statistics.median(ts) / a.tokens * 1e3, 3)}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
