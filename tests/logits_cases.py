"""The rules of ff_logits_process (include/flamingo_fusion.h) restated in numpy ON BIT PATTERNS, the dtype's rounding included, and the
designed cases the kernel is held to bit for bit (tests/test_hip_logits.py) and the restatement itself to hand-written expectations and to
transformers' formulas (tests/test_logits_cases.py).

A row of logits travels as its stored bits (uint16 for bfloat16, uint32 for float32), so "keeps its bits" is checkable for NaN payloads,
signed zeros and everything else.  The product of rule 1 is one float32 multiplication (numpy's float32 scalars round once, like the
device's v_mul_f32) and one round-to-nearest-even to the dtype, done here in integer arithmetic."""
import numpy as np

DTYPES = ("bf16", "f32")
OUT_OF_RANGE = (-1, None, 1 << 40)        # None stands for V: ids that take part in the n-gram comparisons but name no logit


def bits_of(values, dtype):
    """float32 values that lie on the dtype's grid -> stored bits (exact, asserted)"""
    v = np.ascontiguousarray(values, dtype=np.float32)
    u = v.view(np.uint32)
    if dtype == "f32":
        return u.copy()
    assert not (u & 0xFFFF).any(), "values off the bfloat16 grid"
    return (u >> 16).astype(np.uint16)


def values_of(bits, dtype):
    bits = np.ascontiguousarray(bits)
    if dtype == "f32":
        return bits.view(np.float32).copy()
    return (bits.astype(np.uint32) << 16).view(np.float32)


def round_to(v, dtype):
    """one finite-or-infinite float32 -> the dtype's bits, round to nearest even (never called with a NaN)"""
    u = int(np.float32(v).view(np.uint32))
    if dtype == "f32":
        return u
    return (u + 0x7FFF + ((u >> 16) & 1)) >> 16


def neg_inf(dtype):
    return 0xFF800000 if dtype == "f32" else 0xFF80


def restate(bits, V, hist, hist_len, p=1.0, g=0, eos=-1, min_len=None, dtype="f32"):
    """bits: (rows, >= V) stored logits, hist: (rows, cap) int64 -> the bits after the call (a copy; columns >= V untouched)"""
    out = np.array(bits, copy=True)
    rows, cap = hist.shape
    n = min(max(int(hist_len), 0), cap)
    p32 = np.float32(p)
    rp = np.float32(1.0) / p32
    ninf = neg_inf(dtype)
    for r in range(rows):
        h = [int(t) for t in hist[r, :n]]
        x = values_of(bits[r, :V], dtype)
        if p32 != np.float32(1.0):
            for t in set(h):                                              # once per DISTINCT token, from the ORIGINAL value
                if 0 <= t < V and not np.isnan(x[t]):
                    with np.errstate(over="ignore"):
                        out[r, t] = round_to(x[t] * p32 if x[t] < 0 else x[t] * rp, dtype)
        if g >= 1 and n >= g:
            tail = h[n - g + 1:]
            for i in range(n - g + 1):
                if h[i:i + g - 1] == tail and 0 <= h[i + g - 1] < V:
                    out[r, h[i + g - 1]] = ninf
        if eos >= 0 and min_len is not None and n < int(min_len):
            out[r, eos] = ninf
    return out


def restate_values(x, dtype, hist, hist_len, **kw):
    """the same on float32 VALUES that lie on the dtype's grid (recorded logits): values in, values out"""
    x = np.asarray(x, np.float32)
    return values_of(restate(bits_of(x, dtype), x.shape[1], np.asarray(hist, np.int64), hist_len, dtype=dtype, **kw), dtype)


# ---------------------------------------------------------------------------------------------------------------------------------------
# designed cases
# ---------------------------------------------------------------------------------------------------------------------------------------
ROWS, VOCABS, LAYOUTS = (1, 3, 7), (7, 320, 50258, 70001), ("contiguous", "last-of-2")
N_VALUES = (0, 1, 2, 3, 63, 64, 65, 255, 256, 257, 4096)                # g - 1 and g for g = 2, 3; the 64-lane and 256-thread edges; the cap
SHAPES = [(ROWS[i % 3], V, dt, lay) for i, (V, dt, lay) in enumerate((V, dt, lay) for V in VOCABS for dt in DTYPES for lay in LAYOUTS)]
SPECIAL = {"pos": 2.5, "neg": -1.75, "zero": 0.0, "ninf": -np.inf, "nan": np.nan}       # logits of the tokens 1 .. 5 (every V >= 7 has them)
P = 1.3


def settings(n):
    """[(p, g, cap, eos, min_len)] for a history of n tokens.  g from {1, 2, 3, n, n + 1}; cap == n and > n; min_len == n + 1 (n is
    *min_len - 1: banned) and == n (not banned); eos = token 1, which the history penalises."""
    gs = sorted({1, 2, 3, n, n + 1} - {0})
    out = [(P, 0, max(n, 1), -1, None)]
    for j, g in enumerate(gs):
        cap = max(n, 1) if j % 2 else min(n + 37, 4096)
        out.append((P if j % 2 == 0 else 1.0, g, cap, 1, n + 1 if j % 2 == 0 else n))
    out.append((P, 2, min(n + 5, 4096), 1, None))                         # eos given, min_len null: rule 3 off
    out.append((1.0, 0, max(n, 1), 1, n + 1))                             # rule 3 alone
    return out


def make_case(rows, V, dtype, n, cap, g, seed, events=None):
    """(bits (rows, V), hist (rows, cap)): random logits on the dtype's grid with the SPECIAL tokens' values planted; a random history in
    which - where n allows - every special token and every out-of-range id occurs three times, the last g tokens are one token c (a match
    at i = n - g), the first g - 1 are c too (a match at i = 0) and a run of g + 1 c's sits in the middle (overlapping matches); positions
    >= n hold a TRAP token in [0, V) that the first n positions do not hold (where V leaves one): its logit must not move."""
    ev = events if events is not None else {}
    rng = np.random.default_rng(seed)
    x = (rng.standard_normal((rows, V)) * 3).astype(np.float32)
    x = (x.view(np.uint32) & 0xFFFF0000).view(np.float32) if dtype == "bf16" else x
    for t, v in enumerate(SPECIAL.values(), start=1):
        x[:, t] = v
    hist = rng.integers(0, V, (rows, cap)).astype(np.int64)
    for r in range(rows):
        h = hist[r]
        planted = list(range(1, 6)) + [V if t is None else t for t in OUT_OF_RANGE]
        if n >= 3 * len(planted):
            pos = rng.permutation(n)[:3 * len(planted)]
            h[pos] = np.repeat(planted, 3)
            ev["specials"] = ev.get("specials", 0) + 1
        elif n >= 1:
            h[rng.integers(0, n)] = planted[(r + n) % len(planted)]
        if g >= 2 and n >= g and r % 2 == 0:
            c = h[n - 1]
            h[n - g:n] = c
            ev["match_last"] = ev.get("match_last", 0) + 1
            if n >= 2 * g + 1:
                h[:g - 1] = c
                ev["match_first"] = ev.get("match_first", 0) + 1
            if n >= 4 * g + 4:
                m = n // 2 - g // 2
                h[m:m + g + 1] = c
                ev["overlap"] = ev.get("overlap", 0) + 1
        free = np.setdiff1d(np.arange(6, V), h[:n])
        h[n:] = free[0] if free.size else V - 1
        if free.size:
            ev["trap"] = ev.get("trap", 0) + 1
    return bits_of(x, dtype), hist
