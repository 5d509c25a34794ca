"""The measuring methods the per-feature bench tools share, each stated once: two figures from two tools are comparable when both come
through the same function here.  A tool keeps what it measures: its docstring, its own arguments, its arms or paths, its byte counts and
its feature-specific figures.  The decode-feature tools (beam, group_beam, decode_sample, logits_process, token_logprob, guidance, truncation) use the caption set-up, the
host-clock rounds, the tokens report and launch_us; the optimizer-arm tools (ema, adamw_sr, grad_clip, grad_accum) use the config and
arm set-up, the replay rounds and the per-round arithmetic.
"""
import argparse
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CAPTION_ARGUMENTS = {
    "lm": dict(default="gpt2-large"),
    "clip": dict(default="openai/clip-vit-large-patch14"),
    "batch": dict(type=int, default=32),
    "tokens": dict(type=int, default=32, help="new tokens per image"),
    "rounds": dict(type=int, default=5),
}


def caption_arguments(ap, *names):
    for name in names or CAPTION_ARGUMENTS:
        ap.add_argument(f"--{name}", **CAPTION_ARGUMENTS[name])


def need_gpu(tool):
    if not torch.cuda.is_available():
        raise SystemExit(f"{os.path.basename(tool)} measures on the GPU; none is visible")


def caption_setup(a, dev, dt):
    """-> model, ids, kw: model.generate(ids, **kw) decodes a.tokens new tokens per image after the 4-token prompt"""
    import bench
    margs = argparse.Namespace(lm=a.lm, clip=a.clip, xattn_every=1, lm_dropout=None, backbone_tweaks="off", batch=a.batch, seq_len=32, images=1, frames=0)
    model, cfg = bench.build_model(margs, dev, dt)
    model.eval()
    batch = bench.synthetic_batch(margs, cfg, dev, dt, 0)
    ids, ml, am = batch["input_ids"][:, :4], batch["media_locations"][:, :4], batch["attention_mask"][:, :4]
    return model, ids, dict(media_locations=ml, attention_mask=am, pixel_values=batch["pixel_values"], max_length=4 + a.tokens)


def host_rounds(paths, rounds, sync=torch.cuda.synchronize, clock=time.perf_counter):
    """-> seconds per call {name: [one per round]}, and what each path's warm-up call returned"""
    outs = {name: fn() for name, fn in paths.items()}
    sync()
    times = {name: [] for name in paths}
    for _ in range(rounds):
        for name, fn in paths.items():
            sync()
            t0 = clock()
            fn()
            sync()
            times[name].append(clock() - t0)
    return times, outs


def tokens_report(ts, batch, tokens, per="ms_per_decode_step"):
    n = batch * tokens
    return {"tokens_per_s": round(n / statistics.median(ts), 1), "min": round(n / max(ts), 1), "max": round(n / min(ts), 1),
            per: round(statistics.median(ts) / tokens * 1e3, 3)}


def graphed(session):
    return session.replay is not None and not session.capture_failed


def us_per_call(ms, launches, replays=None, digits=1):
    return round(ms / (launches * (replays or 1)) * 1e3, digits)


def launch_us(fn, launches, replays=None, eager=False, digits=1, warmup=5):
    """microseconds per call of fn.  With `replays` (and not `eager`): `launches` calls are captured into one graph, which is replayed
    `replays` times between two device events - the device paces the launches.  Otherwise: the events around `launches` plain calls."""
    for _ in range(warmup):
        fn()
    if eager:
        replays = None
    run = fn
    if replays:
        graph = torch.cuda.CUDAGraph()
        torch.cuda.synchronize()
        with torch.cuda.graph(graph):
            for _ in range(launches):
                fn()
        graph.replay()
        run = graph.replay
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(replays or launches):
        run()
    e1.record()
    torch.cuda.synchronize()
    return us_per_call(e0.elapsed_time(e1), launches, replays, digits)


def bench_config(config):
    """-> the bench module and bench.parse() of `--config X`"""
    saved, sys.argv = sys.argv, [sys.argv[0], "--config", config]
    import bench
    try:
        return bench, bench.parse()
    finally:
        sys.argv = saved


def trainable_shapes(config, device):
    bench, args = bench_config(config)
    from flamingo_mini_amd import ffi
    ffi.lib()
    model, _ = bench.build_model(args, device, torch.bfloat16)
    shapes = [tuple(p.shape) for p in model.parameters_trainable()]
    del model
    torch.cuda.empty_cache()
    return shapes


def capture_arms(shapes, arms, device):
    """-> graphs, opts by arm name; arms: {name: FusedAdamW arguments}.  bf16 parameters and gradients from a generator seeded with 1."""
    from flamingo_mini_amd import FusedAdamW
    gen = torch.Generator(device=device).manual_seed(1)
    grads = [(torch.randn(s, generator=gen, device=device) * 1e-3).to(torch.bfloat16) for s in shapes]
    graphs, opts = {}, {}
    for name, kw in arms.items():
        params = [torch.nn.Parameter((torch.randn(s, generator=gen, device=device) * 0.02).to(torch.bfloat16)) for s in shapes]
        for p, g in zip(params, grads):
            p.grad = g
        opt = opts[name] = FusedAdamW(params, lr=1e-4, capturable=True, **kw)
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):                          # the eager step allocates the state, the shadows and the device counters
            opt.step()
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        graphs[name] = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graphs[name]):
            opt.step()
    return graphs, opts


def train_setup(config):
    """-> model, batch, trainable parameters, set up as bench.py's training leg does (dtype, stock GEMM tuning, launch structure)"""
    bench, args = bench_config(config)
    from flamingo_mini_amd import ffi
    ffi.lib()
    device = torch.device("cuda", 0)
    dtype = torch.bfloat16 if args.dtype == "bf16" else torch.float32
    if args.stock_tuning != "off" and dtype == torch.bfloat16:
        from flamingo_mini_amd.backbones import load_stock_gemm_tuning
        load_stock_gemm_tuning()
    model, cfg = bench.build_model(args, device, dtype)
    batch = bench.synthetic_batch(args, cfg, device, dtype, 0)
    model.set_launch_structure(hoist_kv=args.hoist_kv == "on")
    return model, batch, list(model.parameters_trainable())


def replay_rounds(steps, rounds, n):
    """-> ms per replay {name: [one per round]}; steps: {name: a call that replays one captured step}"""
    times = {name: [] for name in steps}
    for _ in range(rounds):
        for name, step in steps.items():
            step()                                             # (one untimed replay after switching)
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            for _ in range(n):
                step()
            t1.record()
            t1.synchronize()
            times[name].append(t0.elapsed_time(t1) / n)
    return times


def round_diffs(times, name, base):
    return [x - y for x, y in zip(times[name], times[base])]


def median_diff(times, name, base):
    return round(statistics.median(round_diffs(times, name, base)), 4)


def ms_summary(ts):
    """-> the median and every round, to 4 digits"""
    return round(statistics.median(ts), 4), [round(t, 4) for t in ts]


def aa_spread(diffs):
    """what two identical arms differ by: the largest |difference| of a round"""
    return max(abs(d) for d in diffs)


def emit(text, out):
    print(text)
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "w") as f:
            f.write(text + "\n")
