"""Inputs of the token log-probability tests (a helper module, not a conftest), built on tests/loss_cases.py: its vocabularies (V_SMALL,
V_BOUNDARY, 4099), its value patterns and its -inf placements, as R = 20 rows of V columns with one chosen token per row, laid out with a
row stride ld (ld == V, ld == 2 V - the logits[:, -1] view of a (rows, 2, V) tensor -, and an odd ld > V) and a base `off` elements off
the 16-byte grid, so that the rows run through every start phase; and token_logprob_f32, the float32 restatement of token_logprob_kernel
(csrc/ff_logprob.hip) - loss_cases.ce_fwd_f32, which restates the forward the kernel shares with the loss, called row by row at the row's
own start phase.  Shared by tests/test_logprob_cases.py (the restatement, on the CPU) and tests/test_hip_logprob.py (the kernel)."""
import numpy as np
import torch

import loss_cases as lc

BF16, F32 = lc.BF16, lc.F32
R = lc.B * lc.L
GROUPS = ("shapes", "strides", "patterns", "neg-inf", "gpt2")


def tokens(V, start=0, rows=R):
    """(rows,) int64: the chosen tokens cycle over columns 0..7, V-8..V-1 and V // 2 (clipped to [0, V)) - loss_cases.labels' cycle, one per
    row, nothing ignored"""
    cyc = [int(np.clip(c, 0, V - 1)) for c in list(range(8)) + list(range(V - 8, V)) + [V // 2]]
    return torch.tensor([cyc[(start + r) % len(cyc)] for r in range(rows)], dtype=torch.long)


def odd_ld(V):
    return (V + 3) | 1


def start_off(V, ld, off):
    """elements off the 16-byte grid of row 0: an ld == 2 V case is the [:, -1] view of a (rows, 2, V) tensor whose first element is `off`
    off the grid, so its rows begin V elements later - in the restatement and on the GPU alike"""
    return off + V if ld == 2 * V else off


def row_starts(rows, ld, dtype, off=0):
    """byte offset past the 16-byte grid of every row"""
    es = 16 // lc.NVEC[dtype]
    return [((off + r * ld) * es) % 16 for r in range(rows)]


def token_regions(V, dtype, tok, ld, off=0):
    """{'head', 'body', 'tail'}: where the chosen tokens fall in their rows' traversal"""
    out = set()
    for r, start in enumerate(row_starts(len(tok), ld, dtype, off)):
        head, _, tail0 = lc.row_layout(V, dtype, start)
        out.add("head" if int(tok[r]) < head else "tail" if int(tok[r]) >= tail0 else "body")
    return out


def neg_inf_mask(where, V, dtype, tok, ld, off=0):
    """(rows, V) bool: loss_cases' placements - column 0, the first body column of each row's phase, the first 300 columns, the last
    column - never at a row's own token"""
    mask = np.zeros((len(tok), V), bool)
    for r, start in enumerate(row_starts(len(tok), ld, dtype, off)):
        cols = {"col0": [0], "body0": [lc.row_layout(V, dtype, start)[0]], "first300": list(range(300)), "last": [V - 1]}[where]
        mask[r, [c for c in cols if c < V]] = True
        mask[r, int(tok[r])] = False
    return torch.from_numpy(mask)


def cases(dtype, groups=GROUPS):
    """(name, x (R, V) in `dtype` on the CPU, token (R,) int64, ld, off), by group.  shapes: every vocabulary at ld == V, the
    vector-boundary ones also one element off the grid; strides: the boundary vocabularies and 4099 at ld == 2 V and at an odd ld > V;
    patterns and neg-inf: at loss_cases.V_PATTERN; gpt2: GPT-2's own vocabulary and the one with <EOC> (loss_cases.V_GPT2), ten rows, at
    every layout - the only vocabularies at which a thread of token_logprob_kernel makes several trips through its four-vectors-at-once
    loop and then finishes in the plain one (bf16: 6282 vectors, 24 or 25 per thread; fp32: 12564, 49 or 50).
    `off` is the offset of the underlying buffer; row 0 starts start_off(V, ld, off) elements off the grid."""
    if "shapes" in groups:
        for k, V in enumerate(lc.vocabularies(dtype)):
            yield f"V={V}", lc.logits(V, dtype)[0].reshape(R, V), tokens(V, 9 * k), V, 0
        for V in lc.V_BOUNDARY[dtype]:
            yield f"V={V} off-grid", lc.logits(V, dtype, seed=2)[0].reshape(R, V), tokens(V, 3), V, 1
    if "strides" in groups:
        for k, V in enumerate(lc.V_BOUNDARY[dtype] + [lc.V_LARGE, lc.V_SMALL[-2]]):
            for ld, off in ((2 * V, k % 2), (odd_ld(V), (k + 1) % 2)):
                yield f"V={V} ld={ld} off={off}", lc.logits(V, dtype, seed=6)[0].reshape(R, V), tokens(V, 5 * k + 1), ld, off
    for V in lc.V_PATTERN[dtype]:
        for pattern in lc.PATTERNS[1:] if "patterns" in groups else []:
            x = lc.logits(V, dtype, pattern)[0].reshape(R, V)
            tok = torch.full((R,), lc.spike_column(V), dtype=torch.long) if pattern == "spike-target" else tokens(V, 4)
            yield f"V={V} {pattern}", x, tok, V, 0
        for where in lc.NEG_INF if "neg-inf" in groups else []:
            for ld, off in ((V, 0), (odd_ld(V), 1)):
                tok = tokens(V, 1)
                x = lc.logits(V, dtype, seed=3)[0].reshape(R, V).clone()
                x[neg_inf_mask(where, V, dtype, tok, ld, off)] = float("-inf")
                yield f"V={V} -inf {where} ld={ld} off={off}", x, tok, ld, off
    if "gpt2" in groups:
        yield from gpt2_cases(dtype)


def gpt2_cases(dtype):
    for k, V in enumerate(lc.V_GPT2):
        x = lc.logits(V, dtype, b=2, seed=9)[0].reshape(2 * lc.L, V)
        for j, (ld, off) in enumerate(((V, 0), (odd_ld(V), 1), (2 * V, 1), (V, 1))):
            yield f"V={V} ld={ld} off={off}", x, tokens(V, 3 * k + 5 * j, rows=2 * lc.L), ld, off


def token_logprob_f32(x, tok, ld=None, off=0):
    """token_logprob_kernel in float32 numpy: (logprob, lse), float32 tensors (rows,).  Row r starts (off + r ld) elements past the
    16-byte grid; its pass is loss_cases.ce_fwd_f32 on a one-sample, two-position tensor whose first row it is - the same head / vector /
    tail walk, (m, s) pairs and combines -, and logprob = x_tok - lse = -(lse - x_tok) exactly."""
    rows, V = x.shape
    ld = V if ld is None else ld
    lp, lse = np.empty(rows, np.float32), np.empty(rows, np.float32)
    for r in range(rows):
        pair = torch.stack([x[r], x[r]])[None]                                  # (1, 2, V): row (0, 0) is scored against label (0, 1)
        loss, l = lc.ce_fwd_f32(pair, torch.tensor([[0, int(tok[r])]]), base_off=off + r * ld)
        lp[r], lse[r] = -loss[0], l[0]
    return torch.from_numpy(lp), torch.from_numpy(lse)


def reference(x, tok):
    """float64 from the values as stored: (logprob*, lse*, x_tok)"""
    x64 = x.double()
    lse = torch.logsumexp(x64, dim=-1)
    xt = x64.gather(1, tok[:, None])[:, 0]
    return xt - lse, lse, xt


def within_bounds(lp, lse, x, tok, c):
    """the project's loss bound (tests/util.py CE_C_F = c), element by element, nothing excluded, NaN = a miss:
    |lp - lp*| <= c 2^-24 (|lse*| + |x_tok| + 1),  |lse - lse*| <= c 2^-24 (|lse*| + 1).  Returns (ok, worst lp ratio, worst lse ratio)."""
    lp_ref, lse_ref, xt = reference(x, tok)
    r_lp = (lp.double() - lp_ref).abs() / (c * 2.0 ** -24 * (lse_ref.abs() + xt.abs() + 1.0))
    r_lse = (lse.double() - lse_ref).abs() / (c * 2.0 ** -24 * (lse_ref.abs() + 1.0))
    r_lp, r_lse = torch.nan_to_num(r_lp, nan=float("inf")), torch.nan_to_num(r_lse, nan=float("inf"))
    return bool((r_lp <= 1).all()) and bool((r_lse <= 1).all()), float(r_lp.max()), float(r_lse.max())
