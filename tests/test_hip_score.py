"""ff_logprob_gather / functional.logprob_gather (csrc/ff_score.hip) on the MI355X, in arenas whose surroundings hold a sentinel (the arenas
of tests/test_hip_loss_bounds.py, as test_hip_logprob.run_case uses them).

Five rows with lists of 1, 0, 257, 2 and 600 queries (the last two lengths take the query loop past one trip of the 256 threads), both
dtypes, V = 33, 2049, 4099 and GPT-2's vocabularies on and off the 16-byte grid - the shapes at which the row walk makes several trips and
leaves a remainder -, at ld == V, through the wrapper on the [:, -1] view of a (rows, 2, V) tensor, and at an odd ld > V.
Without base every out[q] equals, bit for bit, functional.token_logprobs on that row (at the same address) and token - the existing kernel,
whose bounds against float64 tests/test_hip_logprob.py holds; with base it equals the float32 sum of base[r] and that value, computed on the
host.  The edge rules S2 - S4, with tables that are not monotone or exceed n_q: the arenas show that nothing outside out was written, the
logits, tok, row_first and base are unchanged, a row with an empty list writes nothing.  Graph capture: captured once, the logits and the
tables change on the device, every replay equals the eager call bit for bit."""
import numpy as np
import pytest
import torch

import logprob_cases as LP
import loss_cases as lc

pytestmark = pytest.mark.gpu
BF16, F32 = LP.BF16, LP.F32
DTYPES = pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
LENGTHS = [1, 0, 257, 2, 600]
ROWS = len(LENGTHS)


def lists_for(V, seed, lengths=LENGTHS):
    """per row: the first tokens from the cycle of logprob_cases.tokens (columns 0..7, V-8..V-1, V // 2: head, tail and body of the row's
    walk), the rest uniform over [0, V) - duplicates inside a list included"""
    rng = np.random.default_rng(seed)
    out = []
    for r, n in enumerate(lengths):
        cyc = LP.tokens(V, 5 * r + seed, rows=min(n, 17)).tolist()
        out.append(cyc + rng.integers(0, V, n - len(cyc)).tolist())
    return out


def csr(lists):
    return (torch.tensor(np.cumsum([0] + [len(l) for l in lists]), dtype=torch.int32), torch.tensor([t for l in lists for t in l], dtype=torch.int32))


def run_gather(x, row_first, tok, ld, off, base=None, wrapper=False):
    """ff_logprob_gather on x's rows laid out with row stride ld, the first `off` elements off the 16-byte grid, inside an arena; the gaps
    between the rows hold NaN.  Returns (out on the CPU - NaN where nothing was written -, the device view of the logits) after checking
    that nothing but out's body was written and every input is unchanged."""
    from flamingo_mini_amd import ffi, functional as F
    from test_hip_loss_bounds import Arena
    rows, V = x.shape
    xa = Arena((rows * ld,), x.dtype, off)
    if wrapper:
        assert ld == 2 * V
        view = xa.body.view(rows, 2, V)[:, -1]
    else:
        view = xa.body.view(rows, ld)[:, :V]
    view.copy_(x)
    n_q = tok.numel()
    oa = Arena((n_q,), F32)
    rfd, tokd = row_first.cuda(), tok.cuda()
    based = None if base is None else base.cuda()
    before = xa.bits.clone()
    if wrapper:
        assert F.logprob_gather(view, rfd, tokd, base=based, out=oa.body) is oa.body
    else:
        ffi.check(ffi.lib().ff_logprob_gather(ffi.dtype_code(x.dtype), rows, V, ld, view.data_ptr(), rfd.data_ptr(), tokd.data_ptr(), n_q, ffi.ptr(based),
                                              oa.body.data_ptr(), ffi.stream_handle(view.device)), "ff_logprob_gather")
    torch.cuda.synchronize()
    assert torch.equal(xa.bits, before), "the logits (or their surroundings, or the gaps between the rows) were written"
    assert oa.intact(), "a write outside out"
    assert torch.equal(rfd.cpu(), row_first) and torch.equal(tokd.cpu(), tok) and (base is None or torch.equal(based.cpu().view(torch.int32), base.view(torch.int32)))
    return oa.body.cpu(), view


def token_logprobs_per_query(view, lists):
    """functional.token_logprobs - the existing kernel - on the same rows at the same addresses, once per position of the longest list:
    {(row, k): value} as float32 numpy scalars"""
    from flamingo_mini_amd import functional as F
    lists = list(lists) + [[]] * (view.shape[0] - len(lists))         # (rows not named have no queries)
    rows, longest = len(lists), max(len(l) for l in lists)
    tokens = torch.tensor([[l[k] if k < len(l) else 0 for l in lists] for k in range(longest)], dtype=torch.long).cuda()
    outs = torch.full((longest, rows), float("nan"), device="cuda")
    for k in range(longest):
        F.token_logprobs(view, tokens[k], out=outs[k])
    host = outs.cpu().numpy()
    return {(r, k): host[k, r] for r, l in enumerate(lists) for k in range(len(l))}


SHAPES = [(33, "V", 0), (2049, "V", 0), (4099, "V", 0), (4099, "2V", 1), (4099, "odd", 1),
          (lc.V_GPT2[0], "V", 0), (lc.V_GPT2[0], "V", 1), (lc.V_GPT2[0], "odd", 1), (lc.V_GPT2[1], "V", 0), (lc.V_GPT2[1], "V", 1), (lc.V_GPT2[1], "2V", 1)]


@DTYPES
@pytest.mark.parametrize("V,layout,off", SHAPES, ids=lambda v: str(v))
def test_bit_equality_with_token_logprobs(dtype, V, layout, off):
    ld = {"V": V, "2V": 2 * V, "odd": LP.odd_ld(V)}[layout]
    x = lc.logits(V, dtype, b=1, L_=ROWS, seed=31)[0][0].clone()
    x[1] = float("nan")                                              # the row with the empty list: not read, so this cannot matter
    lists = lists_for(V, seed=V % 7)
    row_first, tok = csr(lists)
    assert tok.numel() == sum(LENGTHS) and bool((tok[:17] < 8).any()) and bool((tok >= V - 8).any())
    got, view = run_gather(x, row_first, tok, ld, off, wrapper=layout == "2V")
    ref = token_logprobs_per_query(view, lists)
    want = np.array([ref[(r, k)] for r, l in enumerate(lists) for k in range(len(l))], np.float32)
    assert np.isfinite(want).all()
    assert np.array_equal(got.numpy().view(np.int32), want.view(np.int32)), "out differs from token_logprobs on that row and token"
    base = torch.linspace(-7.0, 3.0, ROWS) * 1.37
    got_b, _ = run_gather(x, row_first, tok, ld, off, base=base, wrapper=layout == "2V")
    want_b = np.array([np.float32(base[r]) + ref[(r, k)] for r, l in enumerate(lists) for k in range(len(l))], np.float32)      # one float32 add
    assert np.array_equal(got_b.numpy().view(np.int32), want_b.view(np.int32)), "out differs from float32(base[r] + token_logprobs)"


@DTYPES
def test_edge_rules(dtype):
    """S2: a token outside [0, V) gives NaN and its neighbours in the list are served; -inf at the token gives -inf; a row holding NaN or
    +inf gives NaN.  S3 / S4: tables with a negative bound, a decreasing one, bounds far beyond n_q - the clamps keep every access in
    range, a query no row owns is not written, every owned one has the bits of the plain table's result."""
    V = lc.V_LARGE
    x = lc.logits(V, dtype, b=1, L_=6, seed=33)[0][0].clone()
    lists = [[5, V // 2, V - 1], [-1, 7, V, 1 << 30, -(1 << 31), 9], [11, 12], [1, 2], [3, 4], []]
    x[2, 11] = float("-inf")
    x[3, 100] = float("nan")
    x[4, 200] = float("inf")
    x[5] = float("nan")
    row_first, tok = csr(lists)
    base = torch.tensor([0.5, -1.25, 2.0, 3.0, -4.0, 9.0])
    for b_ in (None, base):
        got, view = run_gather(x, row_first, tok, LP.odd_ld(V), 1, base=b_)
        f = row_first.tolist()
        assert bool(torch.isfinite(got[f[0]:f[1]]).all())
        assert torch.isnan(got[f[1]:f[2]]).tolist() == [True, False, True, True, True, False]
        assert float(got[f[2]]) == float("-inf") and bool(torch.isfinite(got[f[2] + 1]))
        assert bool(torch.isnan(got[f[3]:f[5]]).all())
        if b_ is None:
            ref = token_logprobs_per_query(view, [[5, V // 2, V - 1], [7, 9], [12]])
            want = [ref[(0, 0)], ref[(0, 1)], ref[(0, 2)], ref[(1, 0)], ref[(1, 1)], ref[(2, 0)]]
            assert np.array_equal(got[[0, 1, 2, 4, 8, 10]].numpy().view(np.int32), np.array(want, np.float32).view(np.int32))
    # the tables of S4, on finite rows: 6 queries, rows 0 .. 4
    x = lc.logits(V, dtype, b=1, L_=ROWS, seed=34)[0][0]
    tok = torch.tensor([0, V - 1, 17, V // 2, 3, 2048], dtype=torch.int32)
    plain, _ = run_gather(x, torch.tensor([0, 2, 5, 5, 5, 6], dtype=torch.int32), tok, V, 0)
    assert bool(torch.isfinite(plain).all())
    bits = lambda t: t.view(torch.int32).tolist()
    # a negative bound, then a decrease: rows 0 and 1 own [0, 2) and [2, 5), rows 2 .. 4 own nothing ([5, 3), [3, 3), [3, 3)); query 5 has no owner
    got, _ = run_gather(x, torch.tensor([-7, 2, 5, 3, 3, 3], dtype=torch.int32), tok, V, 0)
    assert bits(got[:5]) == bits(plain[:5]) and bool(torch.isnan(got[5]))
    # bounds far beyond n_q: row 1 owns [2, 6) - query 5 now read from row 1's logits -, rows 2 .. 4 own nothing
    got, view = run_gather(x, torch.tensor([0, 2, 1 << 30, (1 << 31) - 1, 1 << 30, 7], dtype=torch.int32), tok, V, 0)
    assert bits(got[:5]) == bits(plain[:5])
    assert np.array_equal(got[5:].numpy().view(np.int32), np.array([token_logprobs_per_query(view, [[], [2048]])[(1, 0)]], np.float32).view(np.int32))
    # every bound at or below 0: nothing is written at all
    got, _ = run_gather(x, torch.tensor([0, -1, -(1 << 31), 0, -5, 0], dtype=torch.int32), tok, V, 0)
    assert bool(torch.isnan(got).all())


def test_replay_follows_device_side_logits_and_tables():
    """captured once; then the logits, the tokens, the table and base change on the device and every replay equals the eager call bit for
    bit, and each value token_logprobs' on its row and token plus base"""
    from flamingo_mini_amd import functional as F
    rows, V, n_q = 5, 2049, 300
    wide = torch.zeros((rows, 2, V), dtype=BF16, device="cuda")
    logits = wide[:, -1]
    tok = torch.zeros(n_q, dtype=torch.int32, device="cuda")
    row_first = torch.zeros(rows + 1, dtype=torch.int32, device="cuda")
    base = torch.zeros(rows, device="cuda")
    out = torch.zeros(n_q, device="cuda")
    call = lambda: F.logprob_gather(logits, row_first, tok, base=base, out=out)
    call()
    graph = torch.cuda.CUDAGraph()
    torch.cuda.synchronize()
    with torch.cuda.graph(graph):
        call()
    seen = set()
    for seed in range(4):
        lengths = [[3, 0, 280, 10, 7], [0, 299, 1, 0, 0], [60, 60, 60, 60, 60], [1, 2, 3, 4, 290]][seed]
        lists = lists_for(V, seed, lengths)
        rf, tk = csr(lists)
        logits.copy_(lc.logits(V, BF16, b=1, L_=rows, seed=40 + seed)[0][0])
        row_first.copy_(rf); tok.copy_(tk); base.copy_(torch.linspace(-2.0, 2.0, rows) * (seed + 1))
        out.fill_(float("nan"))
        graph.replay()
        got = out.clone()
        want = torch.full_like(out, float("nan"))
        F.logprob_gather(logits, row_first, tok, base=base, out=want)
        torch.cuda.synchronize()
        assert torch.equal(got.view(torch.int32), want.view(torch.int32)), seed
        ref = token_logprobs_per_query(logits, lists)
        b_host = base.cpu().numpy()
        exp = np.array([b_host[r] + ref[(r, k)] for r, l in enumerate(lists) for k in range(len(l))], np.float32)
        assert np.array_equal(got.cpu().numpy().view(np.int32), exp.view(np.int32)), seed
        seen.add(tuple(got.cpu().tolist()))
    assert len(seen) == 4
