"""Exact closed-set scoring without a GPU: ff_logprob_gather is exported and bound and rejects bad arguments with its error codes before
anything reaches a device; functional.logprob_gather has no CPU form; decoding.logprob_gather_torch, the restatement score_candidates uses
on CPU tensors, against a float64 numpy restatement of rules S1 - S3 (include/flamingo_fusion.h)."""
import ctypes as C

import numpy as np
import pytest
import torch

FF_ERR_SHAPE, FF_ERR_UNSUPPORTED = -1, -2
X = C.c_void_p(256)            # a non-null pointer that is never dereferenced: every call below fails its checks first
NAN, INF = float("nan"), float("inf")


def _call(dtype=None, rows=4, vocab=100, ld=100, logits=X, row_first=X, tok=X, n_q=7, base=X, out=X):
    from flamingo_mini_amd import ffi
    return ffi.lib().ff_logprob_gather(ffi.DTYPE_BF16 if dtype is None else dtype, rows, vocab, ld, logits, row_first, tok, n_q, base, out, None)


def test_the_entry_point_is_bound():
    import inspect
    import flamingo_mini_amd
    from flamingo_mini_amd import decoding, ffi, functional as F
    assert "ff_logprob_gather" in ffi.EXPORTED_SYMBOLS and hasattr(ffi.lib(), "ff_logprob_gather") and ffi.lib().ff_version() == 6
    assert list(inspect.signature(F.logprob_gather).parameters) == ["logits", "row_first", "tok", "base", "out"]
    assert flamingo_mini_amd.CandidateScores is decoding.CandidateScores
    assert [f.name for f in __import__("dataclasses").fields(decoding.CandidateScores)] == ["logprobs", "token_counts"]
    assert callable(decoding.score_trie) and callable(decoding.logprob_gather_torch)
    par = inspect.signature(flamingo_mini_amd.FlamingoModel.score_candidates).parameters
    for name, default in (("candidate_ids", inspect.Parameter.empty), ("eos_token_id", None), ("max_rows", 1024)):
        assert par[name].kind is inspect.Parameter.KEYWORD_ONLY and par[name].default == default


@pytest.mark.parametrize("bad", [
    dict(logits=None), dict(row_first=None), dict(tok=None), dict(out=None),
    dict(rows=0), dict(rows=-3), dict(vocab=0), dict(vocab=-1), dict(ld=99), dict(ld=0), dict(n_q=0), dict(n_q=-2),
], ids=lambda d: "-".join(f"{k}={v}" for k, v in d.items()))
def test_argument_errors_return_shape_before_any_launch(bad):
    from flamingo_mini_amd import ffi
    assert _call(**bad) == FF_ERR_SHAPE
    assert b"ff_logprob_gather" in ffi.lib().ff_last_error()


def test_other_dtypes_are_unsupported():
    from flamingo_mini_amd import ffi
    for dtype in (7, 2, -1):
        assert _call(dtype=dtype) == FF_ERR_UNSUPPORTED
        assert b"ff_logprob_gather" in ffi.lib().ff_last_error() and b"dtype" in ffi.lib().ff_last_error()


def test_logprob_gather_has_no_cpu_form():
    from flamingo_mini_amd import ffi, functional as F
    with pytest.raises(ffi.FusionLibraryError, match="no CPU fallback"):
        F.logprob_gather(torch.zeros(2, 5), torch.tensor([0, 1, 2], dtype=torch.int32), torch.zeros(2, dtype=torch.int32))


def restated(x, row_first, tok, base):
    """S1 - S3 in float64 numpy, query by query; a query no row owns stays NaN"""
    rows, V = x.shape
    n_q = len(tok)
    out = np.full(n_q, NAN)
    x = x.astype(np.float64)
    for r in range(rows):
        lo, hi = (min(max(int(v), 0), n_q) for v in (row_first[r], row_first[r + 1]))
        if hi <= lo:
            continue
        row = x[r]
        if np.isnan(row).any() or (row == INF).any():
            lse = NAN
        else:
            m = row.max()
            lse = m + np.log(np.exp(row - m).sum()) if m > -INF else -INF
        for q in range(lo, hi):
            t = int(tok[q])
            with np.errstate(invalid="ignore"):
                lp = NAN if not 0 <= t < V else row[t] - lse
            out[q] = lp if base is None else base[r] + lp
    return out


def designed(dtype):
    """7 rows, V = 37: lists of 3, 0 (empty), 4 with a duplicate token, 3 with tokens out of range, 2 with -inf at a token, 2 in a NaN
    row, 2 in a +inf row; the empty row holds NaN, which must not matter"""
    V = 37
    x = (np.random.default_rng(5).standard_normal((7, V)) * 3.0).astype(np.float32)
    x[1] = NAN
    x[4, 11] = -INF
    x[5, 20] = NAN
    x[6, 3] = INF
    lists = [[0, 36, 18], [], [7, 9, 7, 30], [-1, V, 5], [11, 12], [1, 2], [3, 4]]
    row_first = np.cumsum([0] + [len(l) for l in lists]).astype(np.int32)
    tok = np.array([t for l in lists for t in l], np.int32)
    base = np.linspace(-4.0, 2.0, 7).astype(np.float32)
    return torch.from_numpy(x).to(dtype), torch.from_numpy(row_first), torch.from_numpy(tok), torch.from_numpy(base), lists


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float64], ids=["f32", "bf16", "f64"])
@pytest.mark.parametrize("with_base", [False, True], ids=["null-base", "base"])
def test_logprob_gather_torch_follows_the_rules(dtype, with_base):
    from flamingo_mini_amd.decoding import logprob_gather_torch
    x, row_first, tok, base, lists = designed(dtype)
    b = base.to(torch.float64 if dtype == torch.float64 else torch.float32) if with_base else None
    before = x.clone()
    got = logprob_gather_torch(x, row_first, tok, b)
    assert got.dtype == (torch.float64 if dtype == torch.float64 else torch.float32) and got.shape == (len(tok),)
    assert torch.equal(torch.nan_to_num(x.float()), torch.nan_to_num(before.float()))
    want = restated(x.double().numpy(), row_first.numpy(), tok.numpy(), None if b is None else b.double().numpy())
    g = got.double().numpy()
    assert (np.isnan(g) == np.isnan(want)).all(), (g, want)
    assert (np.isinf(g) == np.isinf(want)).all() and (g[np.isinf(want)] == want[np.isinf(want)]).all()
    fin = np.isfinite(want)
    # float32 math: a few ulp of the magnitudes involved (|x| <= 15, |lse| <= 15, |base| <= 4); float64 math: the same in 2^-53
    tol = 64 * (2.0 ** -53 if dtype == torch.float64 else 2.0 ** -24) * 40.0
    assert np.abs(g[fin] - want[fin]).max() <= tol, np.abs(g[fin] - want[fin]).max()
    first = row_first.tolist()
    assert np.isnan(g[first[3]:first[3] + 2]).all() and np.isfinite(g[first[3] + 2])          # out of range: NaN; the row's third query is served
    assert g[first[4]] == -INF and np.isfinite(g[first[4] + 1])                              # -inf at the token
    assert np.isnan(g[first[5]:first[7]]).all()                                              # NaN row, +inf row
    assert g[first[2]] == g[first[2] + 2]                                                    # the duplicate token: equal values


def test_logprob_gather_torch_clamps_the_table_and_leaves_unowned_queries():
    from flamingo_mini_amd.decoding import logprob_gather_torch
    x, _, tok, base, _ = designed(torch.float32)
    tok = tok[:6].clone().clamp(0, 36)
    row_first = torch.tensor([-5, 2, 2, 1, 4, 99, 99, 3], dtype=torch.int32)      # not monotone, below 0, beyond n_q: rows 0, 3, 4 own [0,2), [1,4), [4,6)
    got = logprob_gather_torch(x, row_first, tok, base)
    want = restated(x.numpy(), row_first.numpy(), tok.numpy(), base.numpy())
    # query 1 is owned twice (rows 0 and 3 overlap): the restatement keeps the later row's value, torch's indexed store is free to keep
    # either - the caller's duty (S4) is a partition; what is checked is that every query with one owner agrees and the other is served
    for q in (0, 2, 3, 4, 5):
        assert abs(float(got[q]) - want[q]) <= 1e-4
    assert got.shape == (6,) and bool(torch.isfinite(got[1]))
