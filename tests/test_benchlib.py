"""The arithmetic of tools/benchlib.py on fake paths and fixed times (no GPU): the figures the bench tools print are the ones their inline
formulas printed before the methods moved into the library."""
import contextlib
import os
import statistics
import sys
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import benchlib  # noqa: E402


def test_host_rounds_warm_up_each_path_once_then_alternate():
    log = []
    ticks = iter(range(100))
    paths = {"A": lambda: log.append("A") or "a", "B": lambda: log.append("B") or "b"}
    times, outs = benchlib.host_rounds(paths, 3, sync=lambda: log.append("sync"), clock=lambda: next(ticks))
    calls = [x for x in log if x != "sync"]
    assert calls[:2] == ["A", "B"] and calls[2:] == ["A", "B"] * 3
    assert log == ["A", "B", "sync"] + ["sync", "A", "sync", "sync", "B", "sync"] * 3      # every timed call between two synchronisations
    assert outs == {"A": "a", "B": "b"}
    assert times == {"A": [1, 1, 1], "B": [1, 1, 1]}                                       # one clock read before, one after the call


def test_tokens_report_is_the_inline_formula():
    ts, batch, tokens = [0.52, 0.48, 0.5, 0.61, 0.49], 32, 24
    n = batch * tokens
    assert benchlib.tokens_report(ts, batch, tokens) == {
        "tokens_per_s": round(n / statistics.median(ts), 1), "min": round(n / max(ts), 1), "max": round(n / min(ts), 1),
        "ms_per_decode_step": round(statistics.median(ts) / tokens * 1e3, 3)}
    assert benchlib.tokens_report(ts, batch, tokens) == {"tokens_per_s": 1536.0, "min": 1259.0, "max": 1600.0, "ms_per_decode_step": 20.833}
    assert list(benchlib.tokens_report(ts, batch, tokens, per="ms_per_new_token")) == ["tokens_per_s", "min", "max", "ms_per_new_token"]


def test_round_differences_median_and_aa_spread():
    times = {"plain": [1.0, 1.1, 1.2, 1.0, 1.3], "plain2": [1.01, 1.08, 1.2, 1.03, 1.29], "ema": [1.5, 1.7, 1.6, 1.55, 1.9]}
    d = benchlib.round_diffs(times, "ema", "plain")
    assert [round(x, 6) for x in d] == [0.5, 0.6, 0.4, 0.55, 0.6]
    assert benchlib.median_diff(times, "ema", "plain") == 0.55
    assert benchlib.ms_summary(times["ema"]) == (1.6, [1.5, 1.7, 1.6, 1.55, 1.9])
    assert benchlib.ms_summary([0.123456, 0.2, 0.300049]) == (0.2, [0.1235, 0.2, 0.3])
    aa = benchlib.round_diffs(times, "plain2", "plain")
    assert round(benchlib.aa_spread(aa), 6) == 0.03                                        # the largest |difference|, whatever its sign
    assert round(benchlib.aa_spread([-0.04, 0.03]), 6) == 0.04


def test_launch_us_divides_by_the_calls_inside_the_window(monkeypatch):
    assert benchlib.us_per_call(3.0, 200) == 15.0                                          # eager: ms over `launches` calls
    assert benchlib.us_per_call(3.0, 200, 100, digits=2) == 0.15                           # replay: over launches x replays
    assert benchlib.us_per_call(1.23456, 100) == 12.3 and benchlib.us_per_call(1.23456, 100, digits=2) == 12.35

    log = []
    event = types.SimpleNamespace(record=lambda: log.append("event"), elapsed_time=lambda other: 3.0)      # every window lasts 3 ms
    graph = types.SimpleNamespace(replay=lambda: log.append("replay"))
    for name, fake in (("Event", lambda enable_timing: event), ("CUDAGraph", lambda: graph), ("graph", lambda g: contextlib.nullcontext()),
                       ("synchronize", lambda: None)):
        monkeypatch.setattr(benchlib.torch.cuda, name, fake)

    def fn():
        log.append("call")

    assert benchlib.launch_us(fn, 20) == 150.0
    assert log == ["call"] * 5 + ["event"] + ["call"] * 20 + ["event"]
    del log[:]
    assert benchlib.launch_us(fn, 20, 10, eager=True, digits=2, warmup=10) == 150.0        # eager wins over `replays`
    assert log == ["call"] * 10 + ["event"] + ["call"] * 20 + ["event"]
    del log[:]
    assert benchlib.launch_us(fn, 20, 10, digits=2) == 15.0
    assert log == ["call"] * 5 + ["call"] * 20 + ["replay", "event"] + ["replay"] * 10 + ["event"]
