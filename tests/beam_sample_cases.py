"""Beam sampling restated in numpy from rules S1 - S6 of ff_beam_sample_step (include/flamingo_fusion.h) - a helper module, not a conftest.
The noise is sr_cases.philox4x32 under rule S4's counter layout, the walk is beam_cases.step's.  `ft` is the float type of the arithmetic:
np.float32 restates the kernel, np.float64 is the judge the GPU tests and the torch restatement are held to.

    key     = (seed low 32, seed high 32)
    counter = (v >> 2, row, cur_len, 0x42534D50)        word v & 3 serves column v
    u       = ((w >> 9) + 0.5) 2^-23                     g = -log(-log(u))
"""
import itertools

import numpy as np

import beam_cases as BC
import sr_cases as SR

TAG = 0x42534D50


def words(rows, V, seed, cur_len):
    """The 32-bit word of every (row, column): uint32 (rows, V)."""
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    q = np.arange((V + 3) // 4, dtype=np.uint64)[None, :]
    r = np.arange(rows, dtype=np.uint64)[:, None]
    w = SR.philox4x32((q + 0 * r, r + 0 * q, int(cur_len) & 0xFFFFFFFF, TAG), (seed & 0xFFFFFFFF, seed >> 32))
    return np.stack(w, axis=-1).reshape(rows, -1)[:, :V]


def uniform(w, ft=np.float64):
    return ((np.asarray(w, np.uint32) >> np.uint32(9)).astype(ft) + ft(0.5)) * ft(2.0 ** -23)


def gumbel(w, ft=np.float64):
    return -np.log(-np.log(uniform(w, ft)))


def noise(rows, V, seed, cur_len, ft=np.float64):
    return gumbel(words(rows, V, seed, cur_len), ft)


def keep_mask(x, temperature, top_k, top_p):
    """Rule S2's kept set per row, in float64 on the values as given (membership is a function of the value), and the smallest distance
    |mass strictly above a value / Z - top_p| any nucleus decision of a row had (inf without a nucleus): (keep (rows, V) bool, margin (rows,))."""
    x = np.asarray(x, np.float64)
    rows, V = x.shape
    keep = np.ones((rows, V), bool)
    if 0 < top_k < V:
        keep = x >= np.partition(x, V - top_k, axis=1)[:, V - top_k][:, None]
    margin = np.full(rows, np.inf)
    if top_p < 1.0:
        keep &= x > -np.inf
        for r in range(rows):
            vals, counts = np.unique(x[r][keep[r]], return_counts=True)
            vals, counts = vals[::-1], counts[::-1]
            w = np.exp((vals - vals[0]) / temperature) * counts
            above = (np.cumsum(w) - w) / w.sum()
            margin[r] = float(np.abs(above - top_p).min())
            keep[r] &= np.isin(x[r], vals[above < top_p])
    return keep, margin


def select(score, logits, g, nb, temperature=1.0, top_k=0, top_p=1.0, ft=np.float32, extra=1):
    """Rules S1 - S5: per sequence the 2 nb + extra best candidates by (p descending, flat index ascending).
    Returns (p, a, beam, token), each (b, n), and the smallest nucleus margin of every sequence's rows (b,)."""
    x = np.asarray(logits).astype(ft)
    rows, V = x.shape
    b, n = rows // nb, min(2 * nb + extra, nb * V)
    keep, margin = keep_mask(logits, temperature, top_k, top_p)
    m = x.max(1, keepdims=True)
    lse = m + np.log(np.exp(x - m).sum(1, keepdims=True, dtype=ft)).astype(ft)
    logp = (x - lse).astype(ft)
    z = np.where(keep, logp if temperature == 1.0 else (logp / ft(temperature)).astype(ft), ft(-np.inf))
    a = (z + np.asarray(score).reshape(-1, 1).astype(ft)).astype(ft).reshape(b, nb * V)
    p = (a + np.asarray(g).astype(ft).reshape(b, nb * V)).astype(ft)
    out = [np.zeros((b, n), dt) for dt in (ft, ft, np.int64, np.int64)]
    for s in range(b):
        thr = np.partition(p[s], nb * V - n)[nb * V - n]
        idx = np.flatnonzero(p[s] >= thr)
        idx = idx[np.lexsort((idx, -p[s][idx]))][:n]
        out[0][s], out[1][s], out[2][s], out[3][s] = p[s][idx], a[s][idx], idx // V, idx % V
    return (*out, margin.reshape(b, nb).min(1))


def order_by_score(a, beam, tok, V):
    """Rule S6 on (b, n) arrays: a descending, then flat index ascending."""
    flat = beam * V + tok
    o = np.stack([np.lexsort((flat[s], -a[s])) for s in range(a.shape[0])])
    take = lambda t: np.take_along_axis(t, o, axis=1)
    return take(a), take(beam), take(tok)


def gaps(vals):
    """Smallest nonzero gap between consecutive finite values of a descending list (inf when there is none): an exact tie is decided by the
    flat index under every precision, anything else has to be wide."""
    f = np.sort(np.asarray(vals, np.float64)[np.isfinite(vals)])[::-1]
    d = f[:-1] - f[1:]
    d = d[d > 0]
    return float(d.min()) if d.size else np.inf


def step(state, logits, g, cur_len, nb, eos=None, pad=0, early_stopping=True, temperature=1.0, top_k=0, top_p=1.0, ft=np.float32, events=None):
    """Rules S1 - S6 on `state`, in place; the walk is beam_cases.step's, handed the drawn candidates in rule S6's order.
    Returns, per sequence (b,), the smallest margin any decision of the step had: the gaps among the best 2 nb + 1 values of p and among
    the chosen a, and the nucleus decisions of its rows (inf for a sequence that was done: its candidates decide nothing)."""
    V = np.asarray(logits).shape[1]
    p, a, beam, tok, margin = select(state["score"], logits, g, nb, temperature, top_k, top_p, ft)
    K = min(2 * nb, p.shape[1])
    ordered = order_by_score(a[:, :K], beam[:, :K], tok[:, :K], V)
    for s in range(p.shape[0]):
        margin[s] = np.inf if state["done"][s] else min(margin[s], gaps(p[s]), gaps(ordered[0][s]))
    original = BC.candidates
    BC.candidates = lambda score, x, nb_, ft_=None, extra=1: ordered          # beam_cases.step: its walk, these candidates
    try:
        BC.step(state, logits, cur_len, nb, eos, pad, early_stopping, ft=ft, events=events)
    finally:
        BC.candidates = original
    return margin


def pair_probabilities(logp):
    """Plackett-Luce: the probability of every UNORDERED pair {i, j} being the first two of a draw without replacement from softmax(logp),
    by enumeration: dict {(i, j), i < j} -> probability."""
    w = np.exp(np.asarray(logp, np.float64) - np.max(logp))
    w = w / w.sum()
    return {(i, j): w[i] * w[j] / (1 - w[i]) + w[j] * w[i] / (1 - w[j]) for i, j in itertools.combinations(range(len(w)), 2)}


def chi_square(counts, probs):
    counts, probs = np.asarray(counts, np.float64), np.asarray(probs, np.float64)
    expected = counts.sum() * probs
    return float(((counts - expected) ** 2 / expected).sum()), float(expected.min())


# the 1 - 1e-4 quantiles of the chi-square distribution (scipy.stats.chi2.ppf(1 - 1e-4, df))
CHI2_Q = {14: 42.579, 15: 44.263, 27: 63.164}
