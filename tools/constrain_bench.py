#!/usr/bin/env python
"""Constrained decoding (a candidate trie, banned words) at the benchmark's caption geometry (config B: gpt2-large + CLIP ViT-L/14, random-init
backbones, batch 32, bf16, a 4-token prompt with the media tag first - bench.py's caption leg).  One JSON line:

    constrain_us        ff_logits_constrain alone on 32 rows x 50 258 columns bf16: a trie of 10 and of 1000 candidates (3 tokens each, every
                        row at the root: the widest allowed set, the whole row streamed), the same tries two tokens deep (the walk), and 100
                        banned words (bigrams) without a trie.  Device events around --replays replays of a graph of --launches calls, the
                        method of tools/token_logprob_bench.py, whose ff_token_logprob figure (it reads the rows this launch writes) is
                        the yardstick.  The logits are not restored between calls: -inf is written over -inf, the same stores.
    torch_chain_us      decoding.constrain_logits_torch, the restatement the dynamic loops use, on the same GPU tensors (it walks the trie
                        on the host, so each call reads the history back: plain calls between device events, no graph)
    greedy_off / greedy_on / greedy_words    generate() on the static path without constraints, under a trie of 1000 candidates of
                        --tokens - 1 tokens each (prompt + candidate + eos fill max_length, so no row finishes early and every step walks
                        a row's whole generated part: the deepest walk this geometry has), and with the 100 banned words: tokens/s and ms
                        per replayed decode step

Method (benchlib.host_rounds): every path is warmed up with one full call (sessions built, graphs captured), then timed with a host clock
around `--rounds` calls that each end in a device synchronise, ALTERNATING inside a round; the median is reported with the spread.  The
greedy_off figure is what the commit before the feature measures with the same command: run this file's `--only off` leg there (it needs
nothing of the feature) to compare.  Needs the GPU: there is no fallback.

    python tools/constrain_bench.py [--tokens 32] [--rounds 5] [--only off]
"""
import argparse
import json

import numpy as np
import torch

import benchlib

V, EOS = 50258, 50256


def candidates(k, seed, length=3):
    """k distinct candidates of `length` tokens below 50 000, sharing first tokens ten to one (a trie with k / 10 children at the root)"""
    rng = np.random.default_rng(seed)
    firsts = rng.choice(50000, max(k // 10, 1), replace=False)
    out = set()
    while len(out) < k:
        out.add((int(firsts[len(out) % len(firsts)]),) + tuple(int(t) for t in rng.integers(0, 50000, length - 1)))
    return sorted(out)


def main():
    ap = argparse.ArgumentParser()
    benchlib.caption_arguments(ap)
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--replays", type=int, default=100)
    ap.add_argument("--only", choices=["off"], default=None, help="off: the constraints-off decode leg alone (runs on a tree without the feature)")
    a = ap.parse_args()
    benchlib.need_gpu(__file__)
    dev, dt = torch.device("cuda"), torch.bfloat16
    model, ids, kw = benchlib.caption_setup(a, dev, dt)
    rng = np.random.default_rng(1)
    words = [[int(t) for t in rng.integers(0, 50000, 2)] for _ in range(100)]
    paths = {"greedy_off": lambda: model.generate(ids, **kw)}
    if a.only is None:
        cands = [list(c) for c in candidates(1000, 0, a.tokens - 1)]
        paths["greedy_on"] = lambda: model.generate(ids, candidate_ids=cands, eos_token_id=EOS, pad_token_id=EOS, **kw)
        paths["greedy_words"] = lambda: model.generate(ids, bad_words_ids=words, **kw)
    res = {"geometry": f"{a.lm}, batch {a.batch}, prompt 4 + {a.tokens} new tokens, bf16, random-init backbones", "rounds": a.rounds,
           "device": torch.cuda.get_device_name(0)}
    with torch.no_grad():
        times, _ = benchlib.host_rounds(paths, a.rounds)
        res["decode_step_hip_graph"] = all(benchlib.graphed(s) for s in model._decode_sessions.values())
        if a.only is None:
            from flamingo_mini_amd import decoding as D, functional as F
            g = torch.Generator(device="cuda").manual_seed(0)
            logits = (torch.randn((a.batch, V), generator=g, device=dev) * 4).to(dt)
            hist = torch.randint(0, V, (a.batch, 64), generator=g, device=dev)
            n_dev, n0_dev = torch.full((1,), 32, dtype=torch.long, device=dev), torch.full((1,), 32, dtype=torch.long, device=dev)
            up = lambda arr: torch.from_numpy(np.atleast_1d(arr)).to(dev)
            res["constrain_us"], res["torch_chain_us"] = {}, {}
            for k in (10, 1000):
                trie = D.TokenTrie(candidates(k, k), V, EOS)
                t_dev = (up(trie.node_first), up(trie.edge_tok), up(trie.edge_child), up(trie.node_terminal), up(np.int32(trie.n_nodes)))
                for depth in (0, 2):
                    hist[:, 30:32] = torch.tensor(trie.candidates[0][:2], device=dev)
                    n0_dev.fill_(32 - depth)
                    name = f"trie_{k}" + ("_depth2" if depth else "")
                    res["constrain_us"][name] = benchlib.launch_us(lambda: F.constrain_logits(logits, hist, n_dev, n0_dev, EOS, trie=t_dev), a.launches, a.replays)
                    x32 = logits.float()
                    res["torch_chain_us"][name] = benchlib.launch_us(lambda: D.constrain_logits_torch(x32, hist[:, :32], 32 - depth, EOS, trie), 20, eager=True)
            bw = D.BadWords(words, V)
            w_dev = (up(bw.bw_off), up(bw.bw_tok), up(np.int32(bw.n)))
            logits = (torch.randn((a.batch, V), generator=g, device=dev) * 4).to(dt)
            res["constrain_us"]["words_100"] = benchlib.launch_us(lambda: F.constrain_logits(logits, hist, n_dev, n0_dev, None, bad_words=w_dev), a.launches, a.replays)
            x32 = logits.float()
            res["torch_chain_us"]["words_100"] = benchlib.launch_us(lambda: D.constrain_logits_torch(x32, hist[:, :32], 32, None, None, bw), 20, eager=True)
            tok = torch.randint(0, V, (a.batch,), generator=g, device=dev)
            lp = torch.zeros((a.batch,), dtype=torch.float32, device=dev)
            res["token_logprob_us"] = benchlib.launch_us(lambda: F.token_logprobs(logits, tok, out=lp), a.launches, a.replays)
    for name, ts in times.items():
        res[name] = benchlib.tokens_report(ts, a.batch, a.tokens)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
