"""Beam search restated in numpy from the rules of ff_beam_step (include/flamingo_fusion.h, rules 1-8; rule 9, the fixed summation order, is
the kernel's own business), and the scripted logits that drive it and FlamingoModel._beam_search alike.

`step(state, logits, cur_len, ...)` advances a state of numpy arrays with the fields of functional.BeamState; `ft` is the float type of the
arithmetic: np.float32 restates the kernel (the state's own precision), np.float64 is the reference the GPU tests judge scores against."""
import numpy as np
import torch

FIELDS = ("score", "done", "n_hyp", "hyp_score", "hyp_len", "hyp_row", "hist_tok", "hist_parent", "hist_score", "next_tok", "beam_idx", "len_norm")


def new_state(b, nb, max_len, length_penalty=1.0, pad=0):
    rows = b * nb
    st = dict(score=np.full((b, nb), -np.inf, np.float32), done=np.zeros(b, np.int32), n_hyp=np.zeros(b, np.int32),
              hyp_score=np.full((b, nb), -np.inf, np.float32), hyp_len=np.zeros((b, nb), np.int32), hyp_row=np.zeros((b, nb), np.int32),
              hist_tok=np.zeros((max_len, rows), np.int64), hist_parent=np.zeros((max_len, rows), np.int32),
              hist_score=np.zeros((max_len, rows), np.float32), next_tok=np.full(rows, pad, np.int64), beam_idx=np.arange(rows, dtype=np.int64),
              len_norm=np.asarray([0.0] + [float(t) ** length_penalty for t in range(1, max_len + 1)], np.float64).astype(np.float32))
    st["score"][:, 0] = 0.0
    return st


def candidates(score, logits, nb, ft=np.float32, extra=1):
    """Per sequence the 2 nb + extra best candidates under rules 1-5: (scores (b, n) in `ft`, beams (b, n), tokens (b, n))."""
    x = np.asarray(logits).astype(ft)
    rows, V = x.shape
    b, n = rows // nb, min(2 * nb + extra, nb * V)
    m = x.max(1, keepdims=True)
    lse = m + np.log(np.exp(x - m).sum(1, keepdims=True, dtype=ft)).astype(ft)
    cand = (np.asarray(score).reshape(-1, 1).astype(ft) + (x - lse).astype(ft)).astype(ft).reshape(b, nb * V)
    top_s, top_b, top_t = np.zeros((b, n), ft), np.zeros((b, n), np.int64), np.zeros((b, n), np.int64)
    for s in range(b):
        thr = np.partition(cand[s], nb * V - n)[nb * V - n]                 # the n-th largest value: everything at or above it, then the order of rule 4
        idx = np.flatnonzero(cand[s] >= thr)
        idx = idx[np.lexsort((idx, -cand[s][idx]))][:n]
        top_s[s], top_b[s], top_t[s] = cand[s][idx], idx // V, idx % V
    return top_s, top_b, top_t


def step(state, logits, cur_len, nb, eos=None, pad=0, early_stopping=True, ft=np.float32, events=None):
    """Rules 1-7 on `state`, in place.  Returns the 2 nb + 1 best candidate scores per sequence (b, 2 nb + 1) for margin checks.  `events`
    (a dict) counts what happened: eos at rank < nb / >= nb, sequences that became done."""
    b = state["score"].shape[0]
    top_s, top_b, top_t = candidates(state["score"], logits, nb, ft)
    norm = np.float32(state["len_norm"][cur_len])
    for s in range(b):
        ns, nt, npar = np.full(nb, -np.inf, np.float32), np.full(nb, pad, np.int64), np.arange(nb)
        if not state["done"][s]:
            nh, k = int(state["n_hyp"][s]), 0
            for rank in range(min(2 * nb, top_s.shape[1])):
                v, beam, tok = np.float32(top_s[s, rank]), int(top_b[s, rank]), int(top_t[s, rank])
                if eos is not None and tok == eos:
                    if events is not None:
                        events["eos_low" if rank < nb else "eos_high"] = events.get("eos_low" if rank < nb else "eos_high", 0) + 1
                    if rank < nb:
                        h = np.float32(v / norm)
                        p = 0
                        while p < nh and state["hyp_score"][s, p] >= h:
                            p += 1
                        if p < nb:
                            for name, val in (("hyp_score", h), ("hyp_len", cur_len), ("hyp_row", s * nb + beam)):
                                a = state[name][s]
                                a[p + 1:min(nh + 1, nb)] = a[p:min(nh + 1, nb) - 1].copy()
                                a[p] = val
                            nh = min(nh + 1, nb)
                    continue
                ns[k], nt[k], npar[k] = v, tok, beam
                k += 1
                if k == nb:
                    break
            state["n_hyp"][s] = nh
            if nh >= nb and (early_stopping or state["hyp_score"][s, nb - 1] >= np.float32(ns.max() / norm)):
                state["done"][s] = 1
                if events is not None:
                    events["done"] = events.get("done", 0) + 1
        r = slice(s * nb, (s + 1) * nb)
        state["score"][s] = ns
        state["next_tok"][r] = nt
        state["beam_idx"][r] = s * nb + npar
        state["hist_tok"][cur_len - 1, r] = nt
        state["hist_parent"][cur_len - 1, r] = s * nb + npar
        state["hist_score"][cur_len - 1, r] = ns
    return top_s


def min_margin(top_s):
    """Smallest gap between consecutive finite scores of the best 2 nb + 1 candidates, per sequence (inf where fewer than two are finite)."""
    out = np.full(top_s.shape[0], np.inf)
    for s in range(top_s.shape[0]):
        f = top_s[s][np.isfinite(top_s[s])].astype(np.float64)
        if len(f) > 1:
            out[s] = np.min(f[:-1] - f[1:])
    return out


class Script:
    """Logits as a deterministic function of a row's token history (prompt included): a table row picked by a hash of the history, plus a
    boost of the eos column that depends on the sequence (its first prompt token) and the length, so that eos shows up at low and at high
    ranks, one sequence finishes early and another runs to the length limit."""

    def __init__(self, V, seed, eos=None, eos_boost=None, rows=64):
        g = np.random.default_rng(seed)
        self.V, self.eos, self.rows = V, eos, rows
        self.table = (g.standard_normal((rows, V)) * 2.0).astype(np.float32)
        self.eos_boost = eos_boost or {}                     # first prompt token -> (from length, boost)

    def __call__(self, hist):
        """hist: (rows, L) int64 (numpy or torch) -> (rows, V) float32 numpy"""
        h = np.asarray(hist)
        w = np.arange(1, h.shape[1] + 1, dtype=np.int64)
        out = self.table[(h * w).sum(1) % self.rows].copy()
        if self.eos is not None:
            for r in range(h.shape[0]):
                start, boost = self.eos_boost.get(int(h[r, 0]), (1 << 30, 0.0))
                out[r, self.eos] = -4.0 + (boost if h.shape[1] >= start else 0.0)
        return out


def run_restatement(script, prompt, nb, max_length, eos, pad, early_stopping, length_penalty, events=None):
    """The whole search with the restatement: returns (final state with "length" and "eos", the smallest margin met)."""
    prompt = np.asarray(prompt)
    b, L0 = prompt.shape
    st = new_state(b, nb, max_length, length_penalty, pad)
    hist = np.repeat(prompt, nb, axis=0)
    worst, length = np.inf, L0
    while True:
        cur_len = hist.shape[1] + 1
        live = st["done"] == 0                                              # (a done sequence's candidates decide nothing)
        top = step(st, script(hist), cur_len, nb, eos, pad, early_stopping, events=events)
        worst = min(worst, float(min_margin(top)[live].min()))
        hist = np.concatenate([hist[st["beam_idx"]], st["next_tok"][:, None]], axis=1)
        length = cur_len
        if st["done"].all() or length >= max_length:
            break
    st["length"], st["eos"] = length, -1 if eos is None else eos
    return st, worst


class ScriptedModel:
    """What FlamingoModel._beam_search needs of `self`: _decode_step serves the script, the token history travels as the "cache" tensors, so
    _reorder_cache and _repeat_leading act on it exactly as on a real cache."""

    def __init__(self, script):
        from flamingo_mini_amd.modeling_flamingo import FlamingoModel
        self.script = script
        self._reorder_cache = FlamingoModel._reorder_cache.__get__(self)
        self.search = FlamingoModel._beam_search.__get__(self)

    def _decode_step(self, step_ids, ml, am, past, pixel_values, visual_features):
        hist = step_ids if past is None else torch.cat([past[0][0][0], step_ids], dim=1)
        logits = torch.from_numpy(self.script(hist.numpy()))
        return logits, (((hist, hist),), ((hist, hist),))
