"""The rules of ff_logits_constrain (T1, T2, B1 of include/flamingo_fusion.h) restated in numpy ON BIT PATTERNS, a trie builder of its own
(breadth-first node numbers, where decoding.TokenTrie numbers in insertion order: the rules do not depend on the numbering) and the designed
cases the kernel is held to bit for bit (tests/test_hip_constraint.py) and the restatement itself to hand-written expectations, to
transformers' processors and to the torch restatement of the dynamic loops (tests/test_constraint_cases.py).

The rules only write -inf; a row travels as its stored bits (uint16 for bfloat16, uint32 for float32) so "keeps its bits" is checkable for
NaN payloads and signed zeros.  A table is what the kernel is given: arrays of CAPACITY entries plus a live size; pad_tables() doubles the
capacities and fills what lies behind the live entries with garbage the rules must never read."""
import numpy as np

from logits_cases import bits_of, neg_inf, values_of  # noqa: F401  (re-exported: the tests convert with them)

DEAD, DONE = -1, -2


def build_trie(candidates):
    """{node_first, edge_tok, edge_child, node_terminal, n_nodes} for the candidates (lists of ints), nodes numbered breadth first"""
    root = {}
    for c in candidates:
        d = root
        for t in c:
            d = d.setdefault(int(t), {})
        d[None] = True                                                        # a candidate ends here
    order, first, tok, child, term = [root], [0], [], [], []
    i = 0
    while i < len(order):
        d = order[i]
        term.append(1 if None in d else 0)
        for t in sorted(k for k in d if k is not None):
            tok.append(t)
            child.append(len(order))
            order.append(d[t])
        first.append(len(tok))
        i += 1
    return dict(node_first=np.array(first, np.int32), edge_tok=np.array(tok, np.int32), edge_child=np.array(child, np.int32),
                node_terminal=np.array(term, np.uint8), n_nodes=len(order))


def build_words(words):
    """{bw_off, bw_tok, n_bw} for the words (lists of ints, kept in the order given)"""
    return dict(bw_off=np.cumsum([0] + [len(w) for w in words]).astype(np.int32), bw_tok=np.array([t for w in words for t in w], np.int32).reshape(-1),
                n_bw=len(words))


def pad_tables(t, seed=0):
    """the same table in arrays of twice the live size (at least 4 entries), garbage behind the live entries: offsets and children that
    point far outside, terminal flags set"""
    rng = np.random.default_rng(seed)

    def grow(a, size):
        big = np.ones(size, np.uint8) if a.dtype == np.uint8 else rng.integers(0, 1 << 30, size).astype(a.dtype)
        big[:len(a)] = a
        return big
    if "edge_tok" in t:
        node_cap, edge_cap = max(2 * int(t["n_nodes"]), 4), max(2 * len(t["edge_tok"]), 4)
        return dict(node_first=grow(t["node_first"], node_cap + 1), edge_tok=grow(t["edge_tok"], edge_cap), edge_child=grow(t["edge_child"], edge_cap),
                    node_terminal=grow(t["node_terminal"], node_cap), n_nodes=t["n_nodes"])
    return dict(bw_off=grow(t["bw_off"], max(2 * int(t["n_bw"]), 4) + 1), bw_tok=grow(t["bw_tok"], max(2 * len(t["bw_tok"]), 4)), n_bw=t["n_bw"])


def walk(trie, generated, eos):
    """T1, with a linear search of the node's edges"""
    s = 0
    for t in generated:
        if s < 0:
            break
        if t == eos and trie["node_terminal"][s]:
            s = DONE
            continue
        nxt = DEAD
        for e in range(int(trie["node_first"][s]), int(trie["node_first"][s + 1])):
            if int(trie["edge_tok"][e]) == t:
                nxt = int(trie["edge_child"][e])
        s = nxt
    return s


def restate(bits, V, hist, hist_len, gen_start, eos=-1, trie=None, words=None, dtype="f32"):
    """bits: (rows, >= V) stored logits, hist: (rows, cap) int64 -> the bits after the call (a copy; columns >= V untouched)"""
    out = np.array(bits, copy=True)
    rows, cap = hist.shape
    n = min(max(int(hist_len), 0), cap)
    n0 = min(max(int(gen_start), 0), n)
    ninf = neg_inf(dtype)
    for r in range(rows):
        h = [int(t) for t in hist[r, :n]]
        if trie is not None and int(trie["n_nodes"]) > 0:
            s = walk(trie, h[n0:], eos)
            if s >= 0:
                keep = {int(t) for t in trie["edge_tok"][int(trie["node_first"][s]):int(trie["node_first"][s + 1])]}
                if trie["node_terminal"][s]:
                    keep.add(eos)
                banned = np.ones(V, bool)
                banned[[v for v in keep if 0 <= v < V]] = False
                out[r, :V][banned] = ninf
        if words is not None:
            for w in range(int(words["n_bw"])):
                word = [int(t) for t in words["bw_tok"][int(words["bw_off"][w]):int(words["bw_off"][w + 1])]]
                m = len(word)
                if m >= 1 and 0 <= word[-1] < V and n >= m - 1 and h[n - m + 1:] == word[:-1]:
                    out[r, word[-1]] = ninf
    return out


def restate_values(x, dtype, hist, gen_start, **kw):
    """the same on float32 VALUES that lie on the dtype's grid (recorded logits), against the whole of `hist`: values in, values out"""
    x = np.asarray(x, np.float32)
    hist = np.asarray(hist, np.int64)
    return values_of(restate(bits_of(x, dtype), x.shape[1], hist, hist.shape[1], gen_start, dtype=dtype, **kw), dtype)


# ---------------------------------------------------------------------------------------------------------------------------------------
# designed cases
# ---------------------------------------------------------------------------------------------------------------------------------------
SHAPES = [(3, 33, "bf16"), (4, 33, "f32"), (5, 320, "bf16"), (3, 320, "f32"), (4, 50258, "bf16"), (3, 50258, "f32")]
L0 = 3                                                                       # gen_start of the designed histories
LONG = 70                                                                    # a candidate longer than the 64 tokens the kernel's walk loads at a time
EOS = 10
# (hist_cap, *hist_len, *gen_start, rotation of the rows' tails): the root (n == n0, n0 clamped to n, cap 1), one to five generated tokens, a
# walk across the 64-token edge, histories at the cap, n0 == 0 (the prompt counts as generated), lengths outside [0, cap]
LENGTHS = [(1, 0, L0, 0), (1, 1, 0, 0), (1, 1, L0, 0), (24, L0, L0, 0), (24, L0 + 1, L0, 0), (24, L0 + 1, L0, 3), (24, L0 + 2, L0, 0), (24, L0 + 2, L0, 3),
           (24, L0 + 3, L0, 0), (24, L0 + 3, L0, 3), (24, L0 + 4, L0, 0), (24, L0 + 5, L0, 0), (24, 2, 7, 0), (24, 24, L0, 0), (24, 10, 0, 0), (24, 2, 0, 0),
           (24, 30, L0, 0), (24, -4, -2, 0), (4096, L0 + LONG, L0, 0), (4096, L0 + LONG + 1, L0, 0), (4096, 4096, L0, 0)]


def trie_for(V, eos):
    """A trie whose root has the children 0 and V - 1 among others, with a prefix pair, a leaf, and one node (under token 0) whose children
    are the WHOLE vocabulary except eos - the candidates (0, v) for every v - so the 64-ary search of the kernel runs its one-, two- and
    three-round forms at V = 33, 320 and 50258."""
    a, b, c = 2, 5, 7                                                         # tokens every V >= 33 has; eos is chosen away from them
    cands = [[V - 1], [V - 1, a], [a, b, c], [a, b], [c], [b, a, a, b, c], [9] * LONG + [c]]
    cands += [[0, v] for v in range(V) if v != eos]
    return build_trie(cands), (a, b, c)


def tails_for(V, eos, glen):
    """generated parts of exactly glen tokens for the trie of trie_for(); the first three of every list (the fewest rows a shape has) matter
    most.  glen 1: the all-vocabulary node, a leaf, a terminal inner node, inner nodes, DEAD.  glen 2: the prefix pair's shorter end (eos
    or go on), a leaf, DONE, DEAD, a leaf under the all-vocabulary node, an inner node.  Longer: leaves, inner nodes, DONE and DEAD - a
    tail shorter than glen is padded out with eos."""
    a, b, c = 2, 5, 7
    base = {1: [[0], [c], [V - 1], [a], [4], [9]],
            2: [[a, b], [V - 1, a], [c, eos], [a, a], [0, 9], [9, 9]],
            3: [[a, b, c], [b, a, a], [0, 9, 9], [a, b, eos], [9, 9, 9], [a, b, 4]]}.get(glen, [[b, a, a, b, c], [9] * LONG + [c], [a, b, c], [V - 1, a], [c], [0, 9]])
    return [(t + [eos] * glen)[:glen] for t in base]


def histories(V, eos, rows, cap, n, n0, rng, rot=0):
    """(rows, cap) histories of n tokens (n, n0 already clamped) whose generated part h[n0 .. n) is, row by row, tails_for(n - n0) rotated by
    `rot`; the prompt part is random; positions >= n hold token 0, which would move every row that read it"""
    hist = rng.integers(0, V, (rows, cap)).astype(np.int64)
    if n > n0:
        tails = tails_for(V, eos, n - n0)
        for r in range(rows):
            hist[r, n0:n] = tails[(r + rot) % len(tails)]
    hist[:, n:] = 0
    return hist


def clamped(cap, n, n0):
    n = min(max(n, 0), cap)
    return n, min(max(n0, 0), n)


def words_for(V, hist, n):
    """banned words for the histories: single tokens (0, V - 1, out of range), a bigram and a 4-gram that match row 0's tail, one that
    matches nowhere, a word longer than the history, words with out-of-range heads and last tokens"""
    words = [[0], [V - 1], [V + 5], [3, 1 << 20]]
    if n >= 1:
        words += [[int(hist[0, n - 1]), 11], [int(hist[0, n - 1]) ^ 1, 12]]
    if n >= 3:
        words += [[int(t) for t in hist[0, n - 3:n]] + [13]]
        words += [[int(t) for t in hist[-1, n - 3:n]] + [V + 1]]
    words += [[4] * (n + 1) + [14]]                                           # its head is longer than the history
    return build_words(words)


def make_logits(rows, V, dtype, seed):
    """random logits on the dtype's grid with NaN, -0.0, -inf and +inf planted at the tokens 1, 3, 4, 6 (banned in most rows, kept in some)"""
    rng = np.random.default_rng(seed)
    x = (rng.standard_normal((rows, V)) * 3).astype(np.float32)
    x = (x.view(np.uint32) & 0xFFFF0000).view(np.float32) if dtype == "bf16" else x
    x[:, 1], x[:, 3], x[:, 4], x[:, 6] = np.nan, -0.0, -np.inf, np.inf
    return bits_of(x, dtype)
