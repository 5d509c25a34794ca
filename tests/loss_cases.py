"""Inputs of the per-element loss and QuickGELU tests (a helper module, not a conftest): the shapes, labels, value patterns and -inf
placements shared by tests/test_hip_loss_bounds.py (the kernels), tests/test_guarded_checks.py (the checkers, on the CPU) and
tools/loss_c.py (the checkers' constants), and float32 restatements of the kernels of csrc/ff_loss.hip and csrc/ff_elementwise.hip in
numpy, in the kernels' operation order - what the constants are measured with and what the CPU tests inject defects into.

Shifted cross-entropy: b = 4 samples of L = 5 positions, 20 rows of which 16 have a loss.  A row starts wherever the rows before it end,
so with an odd vocabulary the rows run through every start phase relative to the 16-byte grid (8 for bf16, 4 for fp32); the kernel
visits a row as a scalar head up to the grid, 16-byte vectors, and a scalar tail (row_layout)."""
import numpy as np
import torch

BF16, F32 = torch.bfloat16, torch.float32
NVEC = {F32: 4, BF16: 8}                         # elements per 16-byte vector
IGNORE = -100
B, L = 4, 5
V_SMALL = [1, 3, 7, 8, 9, 33, 255]               # below the head length, below one vector, a few vectors
V_BOUNDARY = {BF16: [2047, 2048, 2049, 2057], F32: [1023, 1024, 1025, 1029]}    # 256 vectors (one per thread) - 1, +- 0, + 1, + head and tail
V_LARGE = 4099
V_PATTERN = {BF16: [4099, 2049], F32: [4099, 1025]}
V_GPT2 = [50257, 50258]                          # b = 2 there
PATTERNS = ["normal", "ascending", "descending", "spike-target", "spike-away", "offset"]
NEG_INF = ["col0", "body0", "first300", "last"]
FLT_MAX = np.float32(3.4028234663852886e38)


def vocabularies(dtype):
    return V_SMALL + V_BOUNDARY[dtype] + [V_LARGE]


def row_layout(V, dtype, start_bytes):
    """(head, nvec, tail0) of a row that starts `start_bytes` past the 16-byte grid: columns [0, head) are scalar, then nvec vectors,
    then [tail0, V) scalar - for_row_vectors in csrc/ff_loss.hip."""
    N = NVEC[dtype]
    head = min(((16 - start_bytes % 16) & 15) // (16 // N), V)
    nvec = (V - head) // N
    return head, nvec, head + nvec * N


def row_starts(b, L_, V, dtype, base_off=0):
    """byte offset past the 16-byte grid of every row (b * L of them) of logits whose first element is base_off elements off the grid"""
    es = 16 // NVEC[dtype]
    return [((base_off + r * V) * es) % 16 for r in range(b * L_)]


def labels(V, b=B, L_=L, start=0):
    """(b, L) int64: the targets cycle over columns 0..7, V-8..V-1 and V // 2 (clipped to [0, V)), beginning at entry `start` of that
    cycle; one ignored position among the scored ones (1..L-1) of every sample, and, from three samples on, the last sample all ignored."""
    cyc = [int(np.clip(c, 0, V - 1)) for c in list(range(8)) + list(range(V - 8, V)) + [V // 2]]
    out = np.empty((b, L_), np.int64)
    k = start
    for s in range(b):
        for i in range(L_):
            out[s, i] = cyc[k % len(cyc)]
            k += i > 0                               # position 0 is never a target: do not spend a cycle entry on it
        out[s, 1 + s % (L_ - 1)] = IGNORE
    if b >= 3:
        out[b - 1] = IGNORE
    return torch.from_numpy(out)


def grad_rows(b=B, L_=L, seed=5):
    """the gradient of every loss row (the reduction='none' form), float32 normal"""
    return torch.from_numpy(np.random.default_rng(seed).standard_normal(b * (L_ - 1)).astype(np.float32))


def spike_column(V):
    return V - 9                                     # in one of the last vectors: its thread has been through its other vectors before


def logits(V, dtype, pattern="normal", b=B, L_=L, seed=1):
    """((b, L, V) logits in `dtype` on the CPU, labels or None): normal with std 3, and
    ascending / descending: every row sorted, so every element (none but the first) is a new maximum;
    spike-target / spike-away: one logit 80 above the rest, at the target (the labels to use are returned) or away from it;
    offset: all logits + 1000 (fp32) / + 64 (bf16)."""
    x = (np.random.default_rng(seed).standard_normal((b, L_, V)) * 3.0).astype(np.float32)
    lab = None
    if pattern == "ascending":
        x = np.sort(x, axis=-1)
    elif pattern == "descending":
        x = np.sort(x, axis=-1)[..., ::-1].copy()
    elif pattern in ("spike-target", "spike-away"):
        x[..., spike_column(V)] = x.max(axis=-1) + 80.0
        if pattern == "spike-target":
            lab = labels(V, b, L_)
            lab[lab != IGNORE] = spike_column(V)
    elif pattern == "offset":
        x = x + np.float32(1000.0 if dtype == F32 else 64.0)
    else:
        assert pattern == "normal", pattern
    return torch.from_numpy(x).to(dtype), lab


def neg_inf_columns(where, V, dtype, lab, base_off=0, b=B, L_=L):
    """(b, L, V) bool: where to put -inf - column 0, the first body column of each row's phase, the first 300 columns, the last column -
    never at a row's own target"""
    mask = np.zeros((b, L_, V), bool)
    starts = row_starts(b, L_, V, dtype, base_off)
    for r in range(b * L_):
        s, i = divmod(r, L_)
        cols = {"col0": [0], "body0": [row_layout(V, dtype, starts[r])[0]], "first300": list(range(300)), "last": [V - 1]}[where]
        mask[s, i, [c for c in cols if c < V]] = True
        if i < L_ - 1 and int(lab[s, i + 1]) != IGNORE:
            mask[s, i, int(lab[s, i + 1])] = False
    return torch.from_numpy(mask)


def target_regions(V, dtype, lab, base_off=0):
    """{'head', 'body', 'tail'}: where the targets of the rows that have one fall in their rows' traversal"""
    b, L_ = lab.shape
    starts, out = row_starts(b, L_, V, dtype, base_off), set()
    for s in range(b):
        for i in range(L_ - 1):
            t = int(lab[s, i + 1])
            if t != IGNORE:
                head, _, tail0 = row_layout(V, dtype, starts[s * L_ + i])
                out.add("head" if t < head else "tail" if t >= tail0 else "body")
    return out


# ---- the forward kernel restated ----------------------------------------------------------------------------------------------------------
_COLS = {}


def thread_columns(V, dtype, head):
    """(256, steps) int: the columns thread t visits, in its order (head element, its vectors, tail element), -1 where it has none"""
    key = (V, dtype, head)
    if key not in _COLS:
        N = NVEC[dtype]
        nvec = (V - head) // N
        tail0 = head + nvec * N
        t = np.arange(256)
        v = t[:, None] + 256 * np.arange((nvec + 255) // 256)[None, :]
        body = np.where((v < nvec)[:, :, None], head + v[:, :, None] * N + np.arange(N)[None, None, :], -1).reshape(256, -1)
        _COLS[key] = np.concatenate([np.where(t < head, t, -1)[:, None], body, np.where(tail0 + t < V, tail0 + t, -1)[:, None]], axis=1)
    return _COLS[key]


def ce_fwd_f32(x, lab, base_off=0, fixed=True, mutate=None):
    """shifted_ce_fwd_kernel in float32 numpy: every thread's online (m, s) over its columns, the xor-shuffle combine of a wave, the
    combine of the four waves, lse = M + log S, loss = lse - x[target].  fixed=False is the traversal before the -inf fix (m starts at -inf,
    exp(-inf - -inf) = NaN).  Returns (loss, lse), float32 (b * (L - 1),).  `mutate`: no-head, no-tail, drop-wave, no-rescale,
    unshifted-label, lse-as-loss."""
    dtype = x.dtype
    b, L_, V = x.shape
    X = x.float().numpy()
    lab = lab.numpy()
    starts = row_starts(b, L_, V, dtype, base_off)
    rows = [(s, i) for s in range(b) for i in range(L_ - 1)]
    lse = np.empty(len(rows), np.float32)
    f = np.float32
    with np.errstate(all="ignore"):
        for head in sorted({row_layout(V, dtype, starts[s * L_ + i])[0] for s, i in rows}):
            sel = [k for k, (s, i) in enumerate(rows) if row_layout(V, dtype, starts[s * L_ + i])[0] == head]
            cols = thread_columns(V, dtype, head)
            G = np.stack([X[rows[k][0], rows[k][1]] for k in sel])[:, np.maximum(cols, 0)]          # (R, 256, steps)
            m = np.full(G.shape[:2], -FLT_MAX if fixed else -np.inf, np.float32)
            s_ = np.zeros(G.shape[:2], np.float32)
            for j in range(cols.shape[1]):
                if (mutate == "no-head" and j == 0) or (mutate == "no-tail" and j == cols.shape[1] - 1):
                    continue
                valid = (cols[:, j] >= 0)[None, :]
                xj = G[:, :, j]
                gt = xj > m
                s_new = np.where(gt, (s_ if mutate == "no-rescale" else s_ * np.exp(m - xj)) + f(1), s_ + np.exp(xj - m))
                s_ = np.where(valid, s_new, s_).astype(np.float32)
                m = np.where(valid & gt, xj, m)
            m, s_ = m.reshape(-1, 4, 64), s_.reshape(-1, 4, 64)
            for o in (32, 16, 8, 4, 2, 1):
                perm = np.arange(64) ^ o
                m2, s2 = m[..., perm], s_[..., perm]
                mn = np.maximum(m, m2)
                if fixed:
                    s_ = s_ * np.exp(m - mn) + s2 * np.exp(m2 - mn)
                else:
                    s_ = np.where(m == -np.inf, f(0), s_ * np.exp(m - mn)) + np.where(m2 == -np.inf, f(0), s2 * np.exp(m2 - mn))
                m = mn
            sm, ss = m[:, :, 0], s_[:, :, 0]
            M = np.maximum(np.maximum(sm[:, 0], sm[:, 1]), np.maximum(sm[:, 2], sm[:, 3]))
            S = np.zeros_like(M)
            for k in range(4):
                if not (mutate == "drop-wave" and k == 2):
                    S = S + ss[:, k] * np.exp(sm[:, k] - M)
            assert S.dtype == np.float32 and M.dtype == np.float32
            lse[sel] = M + np.log(S)
        loss = np.empty_like(lse)
        for k, (s, i) in enumerate(rows):
            t = int(lab[s, i] if mutate == "unshifted-label" else lab[s, i + 1])
            loss[k] = lse[k] if mutate == "lse-as-loss" else f(0) if t == IGNORE else lse[k] - X[s, i, t]
    return torch.from_numpy(loss), torch.from_numpy(lse)


def ce_bwd_f32(x, lab, lse, g, base_off=0, mutate=None):
    """shifted_ce_bwd_kernel in float32 numpy: d = (exp(x - lse) - onehot) g per element, rounded to the logits' type; rows of the last
    position and ignored rows exactly 0.  `mutate`: g-misindexed (g[b L + i]), onehot-late, last-not-zero, ignored-gets-grad,
    stale-tail (the scalar tail columns keep a finite earlier content, here 0)."""
    dtype = x.dtype
    b, L_, V = x.shape
    X, lab, lse, g = x.float().numpy(), lab.numpy(), lse.numpy(), g.numpy()
    starts = row_starts(b, L_, V, dtype, base_off)
    d = np.zeros((b, L_, V), np.float32)
    f, n = np.float32, b * (L_ - 1)
    with np.errstate(all="ignore"):
        for s in range(b):
            for i in range(L_):
                last = i == L_ - 1
                r = s * (L_ - 1) + i
                t = -1 if last else int(lab[s, i + 1])
                ignored = t == IGNORE
                if (last and mutate != "last-not-zero") or (ignored and mutate != "ignored-gets-grad"):
                    continue
                gr = g[min(s * L_ + i, n - 1)] if mutate == "g-misindexed" else g[r % n]
                onehot = np.zeros(V, np.float32)
                if 0 <= t + (mutate == "onehot-late") < V and not last:
                    onehot[t + (mutate == "onehot-late")] = 1
                row = (np.exp(X[s, i] - lse[r % n]) - onehot) * f(gr)
                if mutate == "stale-tail":
                    row[row_layout(V, dtype, starts[s * L_ + i])[2]:] = 0
                d[s, i] = row
    assert d.dtype == np.float32
    return torch.from_numpy(d).to(dtype)


# ---- QuickGELU ----------------------------------------------------------------------------------------------------------------------------
GRID_PASS = {BF16: 4096 * 256 * 8, F32: 4096 * 256 * 4}          # elements one pass of the capped grid covers


def gelu_sizes(dtype):
    """0, around one vector, around one workgroup of vectors, and one with a second grid-stride pass, three more workgroups and a tail"""
    N = NVEC[dtype]
    return [0, 1, N - 1, N, N + 1, 256 * N - 1, 256 * N, 256 * N + 1, GRID_PASS[dtype] + 3 * 256 * N + N - 1]


def gelu_inputs(n, dtype, seed=11):
    """(x, dy) in `dtype` on the CPU: normal x 4, the last min(n // 2, 2001) elements a ramp from -60 to 60 (exp(-1.702 x) leaves the
    float32 range on one side and vanishes on the other; the ramp covers the ragged tail); dy normal"""
    rng = np.random.default_rng(seed)
    x = (rng.standard_normal(n) * 4.0).astype(np.float32)
    k = min(n // 2, 2001)
    if k:
        x[n - k:] = np.linspace(-60.0, 60.0, k, dtype=np.float32)
    return torch.from_numpy(x).to(dtype), torch.from_numpy(rng.standard_normal(n).astype(np.float32)).to(dtype)


def quick_gelu_f32(x, dy=None, fixed=True, mutate=None):
    """quick_gelu_kernel in float32 numpy, forward (dy None) or derivative, rounded to x's type.  fixed=False is the kernel before the
    sigmoid was scaled: exp(-1.702 x) = inf below x = -52, so x sigmoid = 0 where the value is still 1e-37.  `mutate`: skip-tail (the last
    n % N elements keep 0), skip-second-pass (elements from one grid pass on keep 0)."""
    dtype, f = x.dtype, np.float32
    v = x.float().numpy()
    with np.errstate(all="ignore"):
        if fixed:
            w = (f(-1.702) * v) * f(1.44269504)
            far = w > f(64)
            unscale = np.where(far, f(2.0 ** -64), f(1))
            s = f(1) / (unscale + np.exp2(np.where(far, w - f(64), w)))          # 2^k sigmoid(1.702 x), k = 64 where far
        else:
            unscale = np.ones_like(v)
            s = f(1) / (f(1) + np.exp(f(-1.702) * v))
        if dy is None:
            out = (v * s) * unscale
        else:
            out = (dy.float().numpy() * s * (f(1) + f(1.702) * v * (f(1) - s * unscale))) * unscale
    assert out.dtype == np.float32
    n, N = v.size, NVEC[dtype]
    if mutate == "skip-tail":
        out[n // N * N:] = 0
    if mutate == "skip-second-pass":
        out[GRID_PASS[dtype]:n // N * N] = 0
    return torch.from_numpy(out).to(dtype)


GROUPS = ("shapes", "patterns", "neg-inf", "gpt2")


def ce_cases(dtype, groups=GROUPS):
    """Every shifted cross-entropy input set of tests/test_hip_loss_bounds.py, by group: (name, logits, labels, g, elements off the
    16-byte grid).  shapes: every vocabulary, the vector-boundary ones also one element off the grid; patterns and neg-inf: at V_PATTERN;
    gpt2: GPT-2's own vocabulary and the one with <EOC>, two samples."""
    g = grad_rows()
    if "shapes" in groups:
        for k, V in enumerate(vocabularies(dtype)):
            yield f"V={V}", logits(V, dtype)[0], labels(V, start=9 * k), g, 0
        for V in V_BOUNDARY[dtype]:
            yield f"V={V} off-grid", logits(V, dtype, seed=2)[0], labels(V, start=3), g, 1
    for V in V_PATTERN[dtype]:
        for pattern in PATTERNS[1:] if "patterns" in groups else []:
            x, lab = logits(V, dtype, pattern)
            yield f"V={V} {pattern}", x, (labels(V, start=4) if lab is None else lab), g, 0
        for where in NEG_INF if "neg-inf" in groups else []:
            for off in (0, 1):
                lab = labels(V, start=1)
                x = logits(V, dtype, seed=3)[0]
                x[neg_inf_columns(where, V, dtype, lab, off)] = float("-inf")
                yield f"V={V} -inf {where}{' off-grid' if off else ''}", x, lab, g, off
    if "gpt2" in groups:
        for V in V_GPT2:
            yield f"V={V}", logits(V, dtype, b=2)[0], labels(V, b=2, start=V % 17), grad_rows(b=2), 0
