"""Diverse beam search restated in numpy from rules A - D of ff_group_beam_step (include/flamingo_fusion.h), in the style of beam_cases.py,
whose Script, ScriptedModel and min_margin drive and judge it.

`step(state, logits, cur_len, nb, G, lam, ...)` advances a state of numpy arrays with the fields of functional.BeamState(n_groups=G): done and
n_hyp are (b, G), the hypothesis tables (b, nb) are read as (b, G, gs).  `ft` is the float type of the arithmetic: np.float32 restates the
kernel, np.float64 is the reference the GPU tests judge scores against (lambda is the float32 value the kernel receives in both)."""
import numpy as np

import beam_cases as BC

FIELDS = BC.FIELDS


def new_state(b, nb, G, max_len, length_penalty=1.0, pad=0):
    """Rule C: beam 0 of every group has score 0, every other beam -inf."""
    st = BC.new_state(b, nb, max_len, length_penalty, pad)
    st["score"][:] = -np.inf
    st["score"][:, ::nb // G] = 0.0
    st["done"], st["n_hyp"] = np.zeros((b, G), np.int32), np.zeros((b, G), np.int32)
    return st


def row_scores(score, logits, ft=np.float32):
    """Rules 1 - 3 of ff_beam_step: (rows, V) candidate scores in `ft`, before any penalty."""
    x = np.asarray(logits).astype(ft)
    m = x.max(1, keepdims=True)
    lse = m + np.log(np.exp(x - m).sum(1, keepdims=True, dtype=ft)).astype(ft)
    return (np.asarray(score).reshape(-1, 1).astype(ft) + (x - lse).astype(ft)).astype(ft)


def penalised(cand_rows, counts, lam, ft=np.float32):
    """Rule A on a group's (gs, V) rows: fl(cand - fl(lam * c)) for the counted tokens, every other entry untouched."""
    x = cand_rows.copy()
    for tok, c in counts.items():
        x[:, tok] = (x[:, tok] - ft(ft(np.float32(lam)) * ft(c))).astype(ft)
    return x


def ranked(x, n):
    """The n best entries of a (gs, V) block under rule B's order: (scores, rows, columns)."""
    flat = x.reshape(-1)
    n = min(n, flat.size)
    thr = np.partition(flat, flat.size - n)[flat.size - n]
    idx = np.flatnonzero(flat >= thr)
    idx = idx[np.lexsort((idx, -flat[idx]))][:n]
    return flat[idx], idx // x.shape[1], idx % x.shape[1]


def step(state, logits, cur_len, nb, G, lam, eos=None, pad=0, early_stopping=True, ft=np.float32, events=None, detail=None):
    """Rules A and B on `state`, in place.  Returns the 2 gs + 1 best penalised scores per sequence and group (b, G, 2 gs + 1) for margin
    checks (-inf rows for a group that was done).  `events` (a dict) counts what happened: eos at rank < gs / >= gs, groups that became
    done, a group handled while another group of its sequence was done ("mixed"), a count c >= 2 on a candidate among a group's best 2 gs
    ("c2"), and a dead or done earlier row whose pad equals the token of such a candidate ("pad_uncounted").  `detail` (a dict) receives, per
    handled (sequence, group), the ranked candidates and the counts they were penalised with: (scores, local rows, tokens, counts)."""
    b, gs = state["score"].shape[0], nb // G
    V = np.asarray(logits).shape[1]
    cand = row_scores(state["score"], logits, ft).reshape(b, nb, V)
    norm = np.float32(state["len_norm"][cur_len])
    n_top = min(2 * gs + 1, gs * V)
    tops = np.full((b, G, n_top), -np.inf, ft)
    hyp = {n: state[n].reshape(b, G, gs) for n in ("hyp_score", "hyp_len", "hyp_row")}          # views: written in place

    def ev(name, n=1):
        if events is not None and n:
            events[name] = events.get(name, 0) + n

    for s in range(b):
        ns, nt, npar = np.full(nb, -np.inf, np.float32), np.full(nb, pad, np.int64), np.arange(nb)
        done_before = state["done"][s].copy()
        for g in range(G):
            if state["done"][s, g]:
                continue
            ev("mixed", int(done_before.any()))
            counts = {}
            for k in range(g * gs):                                                                # live next beams of the earlier groups
                if ns[k] > -np.inf:
                    counts[int(nt[k])] = counts.get(int(nt[k]), 0) + 1
            top_s, top_b, top_t = ranked(penalised(cand[s, g * gs:(g + 1) * gs], counts, lam, ft), n_top)
            tops[s, g] = top_s
            if detail is not None:
                detail[(s, g)] = (top_s, top_b, top_t, counts)
            best = [int(t) for t in top_t[:2 * gs]]
            ev("c2", int(any(counts.get(t, 0) >= 2 for t in best)))
            ev("pad_uncounted", int(any(not ns[k] > -np.inf for k in range(g * gs)) and pad in best and counts.get(pad, 0) == 0))
            nh, k = int(state["n_hyp"][s, g]), g * gs
            for rank in range(min(2 * gs, n_top)):
                v, beam, tok = np.float32(top_s[rank]), int(top_b[rank]), int(top_t[rank])
                if eos is not None and tok == eos:
                    ev("eos_low" if rank < gs else "eos_high")
                    if rank < gs:
                        h = np.float32(v / norm)
                        p = 0
                        while p < nh and hyp["hyp_score"][s, g, p] >= h:
                            p += 1
                        if p < gs:
                            for name, val in (("hyp_score", h), ("hyp_len", cur_len), ("hyp_row", s * nb + g * gs + beam)):
                                a = hyp[name][s, g]
                                a[p + 1:min(nh + 1, gs)] = a[p:min(nh + 1, gs) - 1].copy()
                                a[p] = val
                            nh = min(nh + 1, gs)
                    continue
                ns[k], nt[k], npar[k] = v, tok, g * gs + beam
                k += 1
                if k == (g + 1) * gs:
                    break
            state["n_hyp"][s, g] = nh
            if nh >= gs and (early_stopping or hyp["hyp_score"][s, g, gs - 1] >= np.float32(ns[g * gs:(g + 1) * gs].max() / norm)):
                state["done"][s, g] = 1
                ev("done")
        r = slice(s * nb, (s + 1) * nb)
        state["score"][s] = ns
        state["next_tok"][r] = nt
        state["beam_idx"][r] = s * nb + npar
        state["hist_tok"][cur_len - 1, r] = nt
        state["hist_parent"][cur_len - 1, r] = s * nb + npar
        state["hist_score"][cur_len - 1, r] = ns
    return tops


def run_restatement(script, prompt, nb, G, lam, max_length, eos, pad, early_stopping, length_penalty, events=None, ft=np.float32):
    """The whole search with the restatement: returns (final state with "length" and "eos", the smallest margin met)."""
    prompt = np.asarray(prompt)
    b, L0 = prompt.shape
    st = new_state(b, nb, G, max_length, length_penalty, pad)
    hist = np.repeat(prompt, nb, axis=0)
    worst, length = np.inf, L0
    while True:
        cur_len = hist.shape[1] + 1
        live = st["done"] == 0                                              # (a done group's candidates decide nothing)
        tops = step(st, script(hist), cur_len, nb, G, lam, eos, pad, early_stopping, ft=ft, events=events)
        m = BC.min_margin(tops.reshape(b * G, -1)).reshape(b, G)
        worst = min(worst, float(m[live].min()))
        hist = np.concatenate([hist[st["beam_idx"]], st["next_tok"][:, None]], axis=1)
        length = cur_len
        if st["done"].all() or length >= max_length:
            break
    st["length"], st["eos"] = length, -1 if eos is None else eos
    return st, worst


def group_slice(state, g, nb, G):
    """Group g's part of a state, re-indexed as the state of a plain search with nb = gs beams (rows and parents made local): what rule E
    says a group is when lambda = 0."""
    gs = nb // G
    b = state["score"].shape[0]
    rows = (np.arange(b)[:, None] * nb + g * gs + np.arange(gs)[None]).reshape(-1)
    local = lambda a: a - (a // nb) * nb - g * gs + (a // nb) * gs                                 # global row s nb + g gs + j -> s gs + j
    out = dict(score=state["score"][:, g * gs:(g + 1) * gs], done=state["done"][:, g], n_hyp=state["n_hyp"][:, g],
               hyp_score=state["hyp_score"][:, g * gs:(g + 1) * gs], hyp_len=state["hyp_len"][:, g * gs:(g + 1) * gs],
               hyp_row=state["hyp_row"][:, g * gs:(g + 1) * gs].copy(), hist_tok=state["hist_tok"][:, rows], hist_parent=local(state["hist_parent"][:, rows]),
               hist_score=state["hist_score"][:, rows], next_tok=state["next_tok"][rows], beam_idx=local(state["beam_idx"][rows]), len_norm=state["len_norm"])
    live = np.arange(gs)[None] < out["n_hyp"][:, None]                                              # unused hypothesis slots hold 0, not a row of the group
    out["hyp_row"] = np.where(live, local(out["hyp_row"]), out["hyp_row"])
    return {n: np.array(a) for n, a in out.items()}                                                 # copies: a later step of `state` does not reach them
