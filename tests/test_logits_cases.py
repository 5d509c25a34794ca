"""The numpy restatement of ff_logits_process's rules (tests/logits_cases.py) without a GPU: against hand-written expectations, against
transformers' own logits processors on float32 (equal up to the stated difference: x * (1.0f / p) where transformers computes x / p, at most
one float32 ulp apart), against the torch restatement the dynamic decode loops use (FlamingoModel._process_logits), and the designed cases
hold the events the GPU test relies on."""
import numpy as np
import pytest
import torch

import logits_cases as LC

INF = np.inf


def run(x, hist, n=None, dtype="f32", **kw):
    hist = np.asarray([hist], np.int64)
    return LC.restate_values(np.asarray([x], np.float32), dtype, hist, hist.shape[1] if n is None else n, **kw)[0]


def test_hand_written_expectations():
    x = [1.0, -2.0, 0.0, 4.0, -INF, np.nan, 3.0, 0.5]
    h = [0, 1, 0, 3, 0]
    # rule 1, p = 2 (exact products): token 0 occurs three times and is halved ONCE; negative values are multiplied
    np.testing.assert_array_equal(run(x, h, p=2.0), np.float32([0.5, -4.0, 0.0, 2.0, -INF, np.nan, 3.0, 0.5]))
    # zero, -inf and NaN under the penalty: signed zero kept, -inf stays, NaN keeps its bits
    got = LC.restate(LC.bits_of(np.float32([[-0.0, 0.0, -INF, np.nan]]), "f32"), 4, np.int64([[0, 1, 2, 3, 3]]), 5, p=2.0)
    assert got[0].tolist() == [0x80000000, 0, 0xFF800000, 0x7FC00000]
    # rule 2, g = 2: the last token is 0; after the 0 at i = 0 came 1, after the 0 at i = 2 came 3
    np.testing.assert_array_equal(run(x, h, g=2), np.float32([1.0, -INF, 0.0, -INF, -INF, np.nan, 3.0, 0.5]))
    # g = 1 bans every token of the history, g = n needs h[0 .. n-2] == h[1 .. n-1], g = n + 1 does nothing
    np.testing.assert_array_equal(run(x, h, g=1), np.float32([-INF, -INF, 0.0, -INF, -INF, np.nan, 3.0, 0.5]))
    np.testing.assert_array_equal(run(x, h, g=5), np.float32(x))
    np.testing.assert_array_equal(run(x, [6, 6, 6], g=3), np.float32([1.0, -2.0, 0.0, 4.0, -INF, np.nan, -INF, 0.5]))
    np.testing.assert_array_equal(run(x, h, g=6), np.float32(x))
    # rule 4: the ban wins over the penalty (token 1), the penalty holds elsewhere (tokens 0, 3 under g = 3: tail (3, 0), no earlier match)
    np.testing.assert_array_equal(run(x, h, p=2.0, g=2), np.float32([0.5, -INF, 0.0, -INF, -INF, np.nan, 3.0, 0.5]))
    np.testing.assert_array_equal(run(x, h, p=2.0, g=3), np.float32([0.5, -4.0, 0.0, 2.0, -INF, np.nan, 3.0, 0.5]))
    # rule 3: n < *min_len bans eos; n == *min_len does not; a null min_len or eos = -1 switches the rule off; a NaN is banned like any entry
    np.testing.assert_array_equal(run(x, h, eos=6, min_len=6), np.float32([1.0, -2.0, 0.0, 4.0, -INF, np.nan, -INF, 0.5]))
    np.testing.assert_array_equal(run(x, h, eos=6, min_len=5), np.float32(x))
    np.testing.assert_array_equal(run(x, h, eos=6, min_len=None), np.float32(x))
    np.testing.assert_array_equal(run(x, h, eos=-1, min_len=9), np.float32(x))
    np.testing.assert_array_equal(run(x, h, eos=5, min_len=9), np.float32([1.0, -2.0, 0.0, 4.0, -INF, -INF, 3.0, 0.5]))
    # hist_len is clamped to [0, cap]; positions >= n are not read
    np.testing.assert_array_equal(run(x, h, n=99, g=1), run(x, h, g=1))
    np.testing.assert_array_equal(run(x, h, n=-3, g=1, p=2.0), np.float32(x))
    np.testing.assert_array_equal(run(x, h, n=2, g=1), np.float32([-INF, -INF, 0.0, 4.0, -INF, np.nan, 3.0, 0.5]))
    # ids outside [0, V) take part in the comparisons and name no logit
    np.testing.assert_array_equal(run(x, [13, 2, -1, 13], g=2, p=2.0), np.float32([1.0, -2.0, -INF, 4.0, -INF, np.nan, 3.0, 0.5]))
    np.testing.assert_array_equal(run(x, [1 << 40, 7, 1 << 40, 8, 1 << 40], g=1), np.float32([1.0, -2.0, 0.0, 4.0, -INF, np.nan, 3.0, -INF]))


def test_the_product_is_rounded_once_to_the_dtype():
    """1 * float32(1 / 1.3) = 0.76923078...: between the bfloat16 neighbours 0x3F44 (0.765625) and 0x3F45 (0.76953125), nearer the latter;
    -1.75 * float32(1.3) = -2.275: between 0xC011 (-2.265625) and 0xC012 (-2.28125), nearer the latter.  float32 keeps the product."""
    bits = LC.restate(LC.bits_of(np.float32([[1.0, -1.75]]), "bf16"), 2, np.int64([[0, 1]]), 2, p=1.3, dtype="bf16")
    assert bits.dtype == np.uint16 and bits[0].tolist() == [0x3F45, 0xC012]
    got = run([1.0, -1.75], [0, 1], p=1.3)
    assert got[0] == np.float32(1.0) * (np.float32(1.0) / np.float32(1.3)) and got[1] == np.float32(-1.75) * np.float32(1.3)
    # a tie goes to the even neighbour: 1 + 2^-8 lies halfway between 0x3F80 and 0x3F81, 1 + 3 * 2^-8 halfway between 0x3F81 and 0x3F82
    assert LC.round_to(np.float32(1 + 2.0 ** -8), "bf16") == 0x3F80 and LC.round_to(np.float32(1 + 3 * 2.0 ** -8), "bf16") == 0x3F82


def _hf():
    lp = pytest.importorskip("transformers.generation.logits_process")
    return lp


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_float32_equals_transformers_up_to_one_ulp(seed):
    """transformers' RepetitionPenaltyLogitsProcessor, NoRepeatNGramLogitsProcessor and MinLengthLogitsProcessor, each alone on float32: bans
    and the eos entry agree exactly, negative logits exactly (both multiply by p), the others within one float32 ulp (x * (1.0f / p) vs x / p)."""
    lp = _hf()
    rng = np.random.default_rng(seed)
    rows, V, n = 4, 50, 40
    x = (rng.standard_normal((rows, V)) * 3).astype(np.float32)
    hist = rng.integers(0, 12, (rows, n)).astype(np.int64)                # a small alphabet: many repeats, many n-gram matches
    ids, scores = torch.from_numpy(hist), torch.from_numpy(x)
    for p in (1.3, 0.8, 2.0):
        want = lp.RepetitionPenaltyLogitsProcessor(penalty=p)(ids, scores.clone()).numpy()
        got = LC.restate_values(x, "f32", hist, n, p=p)
        neg = x < 0
        np.testing.assert_array_equal(got[neg], want[neg])
        assert (np.abs(got - want) <= np.spacing(np.maximum(np.abs(got), np.abs(want)))).all()
        assert (got != x).any(1).all()
    for g in (1, 2, 3, 5):
        want = lp.NoRepeatNGramLogitsProcessor(g)(ids, scores.clone()).numpy()
        np.testing.assert_array_equal(LC.restate_values(x, "f32", hist, n, g=g), want)
        assert np.isinf(want).any() or g == 5
    for min_len in (n, n + 1):
        try:
            proc = lp.MinLengthLogitsProcessor(min_len, 7, device="cpu")
        except TypeError:                                                 # (older transformers: no device argument)
            proc = lp.MinLengthLogitsProcessor(min_len, 7)
        np.testing.assert_array_equal(LC.restate_values(x, "f32", hist, n, eos=7, min_len=min_len), proc(ids, scores.clone()).numpy())


@pytest.mark.parametrize("n,g", [(0, 2), (1, 1), (2, 3), (3, 3), (40, 1), (40, 2), (40, 3), (40, 40), (40, 41), (40, 0)])
def test_the_torch_restatement_of_the_dynamic_loops_is_the_same_function(n, g):
    """FlamingoModel._process_logits on float32 gives the restatement's values (NaN where it has NaN), out-of-range ids included"""
    from flamingo_mini_amd.modeling_flamingo import FlamingoModel
    rows, V = 3, 320
    bits, hist = LC.make_case(rows, V, "f32", n, max(n, 1), g, seed=5 + n)
    if n == 40 and g == 40:
        hist[0, :n] = 9                                                   # one row whose whole history is one token: the single window matches
    x = LC.values_of(bits, "f32")
    for p, eos, min_len in ((LC.P, None, None), (1.0, 1, n + 1), (LC.P, 1, n), (0.7, 1, n + 3)):
        want = LC.values_of(LC.restate(bits, V, hist, n, p=p, g=g, eos=-1 if eos is None else eos, min_len=min_len), "f32")
        got = FlamingoModel._process_logits(torch.from_numpy(x.copy()), torch.from_numpy(hist[:, :n]), p, g, eos, min_len).numpy()
        np.testing.assert_array_equal(got, want)
        assert np.array_equal(LC.values_of(bits, "f32"), x, equal_nan=True)          # the input is not modified


def test_the_designed_cases_hold_their_events():
    """over the settings of every n at V = 320: the special tokens three times each, matches at i = 0 and i = n - g, overlapping matches,
    trap tokens behind the history; and the restatement moves something in every setting that has a processor on and a history"""
    ev = {}
    for n in LC.N_VALUES:
        for p, g, cap, eos, min_len in LC.settings(n):
            assert 1 <= cap <= 4096 and cap >= n
            bits, hist = LC.make_case(3, 320, "bf16", n, cap, g, seed=n, events=ev)
            out = LC.restate(bits, 320, hist, n, p=p, g=g, eos=eos, min_len=min_len, dtype="bf16")
            if n >= 3 and (p != 1.0 or 1 <= g <= 3):
                assert (out != bits).any(), (n, p, g)
            if eos >= 0 and min_len is not None and n < min_len:
                assert (out[:, eos] == LC.neg_inf("bf16")).all()
    assert all(ev.get(k, 0) > 0 for k in ("specials", "match_first", "match_last", "overlap", "trap")), ev
    gs = {g for n in LC.N_VALUES for _, g, *_ in LC.settings(n)}
    assert {0, 1, 2, 3, 4096, 4097} <= gs
