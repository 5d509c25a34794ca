"""Contrastive search restated in numpy float64, independently of decoding.contrastive_select_torch / topk_logprobs_torch, and the designed
cases of the GPU tests (a helper module: no tests here).

The rules are T and C2 - C7 of include/flamingo_fusion.h.  `topk_logprobs` is rule T on one block of logits; `select` is C2 - C7 for one step:
it returns everything ff_contrastive_step writes, plus the scores and the margin by which the step is decided.  The `defect=` argument of
`select` injects one wrong reading of the rules at a time; tests/test_contrastive_cases.py shows that each of them fails on the designed
cases, so a kernel with that defect would fail there too.

Designed steps (`design_step`): hidden vectors of N(0, 1) entries rounded to the dtype, logits N(0, 2^2) over 320 columns, a seed per case
found on the CPU so that every sequence is DECIDABLE: the best score leads the second by at least MARGIN, or the two are an exact designed
tie (the same vector and the same logp).  Vectors that share a large common component are undecidable ten times as often and are not used."""
import numpy as np

MARGIN = 1e-3
VOCAB = 320
DEFECTS = ("masked_positions", "mean", "last_missing", "alpha_swapped", "logp_for_p", "dead_wins", "tie_to_larger", "finished_not_padded",
           "append_at_n_minus_1")


def bf16_round(x):
    """float32 values rounded to bfloat16 (round to nearest even), returned as float32"""
    u = np.ascontiguousarray(x, np.float32).view(np.uint32).astype(np.uint64)
    u = (u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000
    return u.astype(np.uint32).view(np.float32)


def topk_logprobs(logits, k):
    """rule T: (tok (rows, k) int64, logp (rows, k) float64) of `logits` (rows, V), any float dtype, evaluated in float64"""
    x = np.asarray(logits, np.float64)
    rows, V = x.shape
    tok = np.zeros((rows, k), np.int64)
    logp = np.zeros((rows, k), np.float64)
    for r in range(rows):
        order = sorted(range(V), key=lambda v: (-x[r, v], v))[:k]           # value descending, then index ascending
        m = x[r].max()
        lse = m + np.log(np.exp(x[r] - m).sum()) if np.isfinite(m) else m
        for i, v in enumerate(order):
            tok[r, i] = v
            logp[r, i] = x[r, v] - lse if x[r, v] > -np.inf else -np.inf
    return tok, logp


def select(hidden, hist, mask, n, cand_tok, cand_logp, finished, alpha, eos=-1, pad=0, defect=None):
    """rules C2 - C7 for one step, float64.  hidden (b * k, dim), hist (b, max_len, dim) - read below n -, mask (b, max_len), cand_tok /
    cand_logp (b, k), finished (b,).  Returns a dict: next_tok, logprob, sel (c*), sel_row, beam_idx, finished (after the step), score
    (b, k), hist_row (b, dim: what H[s, n] becomes), hist_pos (where it is written), margin (b,: best score minus second best; inf with one
    live candidate or none) and tie (b,: the best score is shared)."""
    hidden, hist = np.asarray(hidden, np.float64), np.asarray(hist, np.float64)
    b, k = cand_tok.shape
    out = dict(next_tok=np.zeros(b, np.int64), logprob=np.zeros(b, np.float64), sel=np.zeros(b, np.int64), sel_row=np.zeros(b, np.int64),
               beam_idx=np.zeros(b * k, np.int64), finished=np.array(finished, bool).copy(), score=np.zeros((b, k)),
               hist_row=np.zeros((b, hidden.shape[1])), hist_pos=n - 1 if defect == "append_at_n_minus_1" else n, margin=np.zeros(b), tie=np.zeros(b, bool))
    a1, a2 = (alpha, 1.0 - alpha) if defect == "alpha_swapped" else (1.0 - alpha, alpha)
    for s in range(b):
        top = n - 1 if defect == "last_missing" else n
        live = [j for j in range(top) if mask[s, j] != 0 or defect == "masked_positions"]
        for c in range(k):
            h = hidden[s * k + c]
            lp = float(cand_logp[s, c])
            if not lp > -np.inf and defect != "dead_wins":
                out["score"][s, c] = -np.inf
                continue
            cos = [float(h @ hist[s, j]) / (max(np.sqrt(h @ h), 1e-12) * max(np.sqrt(hist[s, j] @ hist[s, j]), 1e-12)) for j in live]
            pen = (float(np.mean(cos)) if defect == "mean" else max(cos)) if cos else 0.0
            conf = lp if defect == "logp_for_p" else (np.exp(lp) if lp > -np.inf else 0.0)
            out["score"][s, c] = a1 * conf - a2 * pen
        sc = out["score"][s]
        best = sc.max()
        at_best = [c for c in range(k) if sc[c] == best] if best > -np.inf else [0]
        c = at_best[-1] if defect == "tie_to_larger" else at_best[0]
        ranked = np.sort(sc[sc > -np.inf])[::-1]
        out["margin"][s] = ranked[0] - ranked[1] if len(ranked) > 1 else np.inf
        out["tie"][s] = len(at_best) > 1
        out["sel"][s], out["sel_row"][s] = c, s * k + c
        out["beam_idx"][s * k:(s + 1) * k] = s * k + c
        out["hist_row"][s] = hidden[s * k + c]
        if finished[s] and defect != "finished_not_padded":
            out["next_tok"][s], out["logprob"][s] = pad, 0.0
        else:
            out["next_tok"][s], out["logprob"][s] = cand_tok[s, c], cand_logp[s, c]
            if eos >= 0 and cand_tok[s, c] == eos:
                out["finished"][s] = True
    return out


def decidable(res):
    """per sequence: the best score leads the second by >= MARGIN, or the step is an exact designed tie (checked by the caller)"""
    return (res["margin"] >= MARGIN) | res["tie"]


def design_step(b, k, dim, n, max_len, dtype="bf16", seed=0, left_pad=(), dead=(), all_dead=(), tie=(), finished=(), eos_seq=(), alpha=0.6):
    """One designed step.  `left_pad`: sequences whose first positions are masked; `dead`: sequences whose last candidate is dead; `all_dead`:
    sequences with no live candidate; `tie`: sequences whose candidates 0 and 1 share the vector and the logp (candidate 0 must win when
    they lead); `finished`: sequences that had finished; `eos_seq`: sequences whose every candidate token is eos (whatever is chosen ends
    them).  Tries seeds from `seed` on until every sequence is decidable; returns the case as a dict of numpy arrays (hidden / hist float32
    holding dtype-representable values) with the float64 result under "ref"."""
    rnd = bf16_round if dtype == "bf16" else (lambda x: np.asarray(x, np.float32))
    eos = VOCAB - 1
    for attempt in range(200):
        g = np.random.default_rng(1000 * seed + attempt)
        hidden = rnd(g.standard_normal((b * k, dim)).astype(np.float32))
        hist = rnd(g.standard_normal((b, max_len, dim)).astype(np.float32))
        logits = rnd((2.0 * g.standard_normal((b, VOCAB))).astype(np.float32))
        logits[:, eos] = -np.inf                                          # eos is a candidate only where planted
        tok, logp = topk_logprobs(logits, k)
        logp = logp.astype(np.float32)
        mask = np.ones((b, max_len), np.uint8)
        for s in left_pad:
            mask[s, :min(3, max(n - 1, 0))] = 0
        for s in dead:
            logp[s, k - 1] = -np.inf
        for s in all_dead:
            logp[s, :] = -np.inf
        for s in tie:
            hidden[s * k + 1] = hidden[s * k]
            logp[s, 1] = logp[s, 0]
        for s in eos_seq:
            tok[s, :] = eos
        fin = np.zeros(b, bool)
        fin[list(finished)] = True
        ref = select(hidden, hist, mask, n, tok, logp, fin, alpha, eos, pad=7)
        ok = decidable(ref)
        for s in tie:                                                     # a designed tie counts only when it is the tie at the top ...
            ok[s] = ok[s] and (not ref["tie"][s] or ref["sel"][s] == 0)
        for s in range(b):                                                # ... and no accidental tie counts at all
            if ref["tie"][s] and s not in tie:
                ok[s] = False
        for s in all_dead:
            ok[s] = True
        if ok.all():
            return dict(b=b, k=k, dim=dim, n=n, max_len=max_len, dtype=dtype, hidden=hidden, hist=hist, mask=mask, cand_tok=tok, cand_logp=logp,
                        finished=fin, alpha=alpha, eos=eos, pad=7, ref=ref, seed=1000 * seed + attempt)
    raise AssertionError(f"no decidable seed for b={b} k={k} dim={dim} n={n}")


def design_rows(rows, V, k, dtype="bf16", seed=0):
    """Logits for rule T: N(0, 2^2) rounded to the dtype; row 1 holds designed ties across the k-th place (one value in many columns,
    which also overflows a short list of candidates), row 2 has fewer than k finite values, row 3 is all one value."""
    rnd = bf16_round if dtype == "bf16" else (lambda x: np.asarray(x, np.float32))
    g = np.random.default_rng(seed)
    x = rnd((2.0 * g.standard_normal((rows, V))).astype(np.float32))
    if rows > 1:
        top = np.float32(x[1].max() + 1.0)
        cols = g.permutation(V)[:min(V, max(k + 2, 300 if V > 600 else k + 2))]
        x[1, cols] = rnd(np.array([top], np.float32))[0]
    if rows > 2:
        x[2, :] = -np.inf
        x[2, g.permutation(V)[:max(k - 1, 0)]] = 1.5
    if rows > 3:
        x[3, :] = 0.25
    return x
