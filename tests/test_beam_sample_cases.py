"""The restatements of beam sampling against each other and against the law they claim, without a GPU: tests/beam_sample_cases.py (numpy,
rules S1 - S6 of ff_beam_sample_step) with the noise off IS beam search; decoding.beam_sample_select_torch equals it on random and
designed inputs; the Gumbel top-k over rule S4's noise has the Plackett-Luce law (chi-square at the 1 - 1e-4 quantile, fixed seeds); the
noise of an entry depends on nothing but (seed, cur_len, row, column); and the dynamic loop with the restatement's noise is the numpy search."""
import numpy as np
import pytest
import torch

import beam_cases as BC
import beam_sample_cases as BSC


def random_case(seed, b=2, nb=3, V=37, dead=False):
    g = np.random.default_rng(seed)
    x = (g.standard_normal((b * nb, V)) * 2).astype(np.float32)
    score = -(g.integers(0, 64, (b, nb)) / 8.0).astype(np.float32)
    if dead:
        score[0, nb - 1] = -np.inf
    return x, score


# ---- (a) without warpers and without noise the step is beam search's ----
@pytest.mark.parametrize("seed,eos,early", [(0, None, True), (1, 5, True), (2, 9, False), (3, 0, True)])
def test_with_the_warpers_off_and_no_noise_the_step_is_beam_search(seed, eos, early):
    """three steps from the initial state (its dead beams included): every field equals beam_cases.step's"""
    b, nb, V, max_len = 2, 3, 37, 8
    mine, plain = BC.new_state(b, nb, max_len), BC.new_state(b, nb, max_len)
    for cur_len in (3, 4, 5):
        x, _ = random_case(10 * seed + cur_len, b, nb, V)
        if eos is not None:
            x[:, eos] += 4.0
        BSC.step(mine, x, np.zeros((b * nb, V)), cur_len, nb, eos, 0, early)
        BC.step(plain, x, cur_len, nb, eos, 0, early)
        for f in BC.FIELDS:
            assert np.array_equal(mine[f], plain[f]), (cur_len, f)


# ---- (b) the torch restatement equals the numpy one ----
def torch_select(score, x, g, nb, *warp, dtype=torch.float64):
    from flamingo_mini_amd import decoding as D
    a, beam, tok = D.beam_sample_select_torch(torch.from_numpy(x).to(dtype), torch.from_numpy(score), torch.from_numpy(g), nb, *warp)
    return a.numpy(), beam.numpy(), tok.numpy()


def assert_same_selection(score, x, g, nb, warp, tol=1e-9):
    p, a, beam, tok, _ = BSC.select(score, x, g, nb, *warp, ft=np.float64, extra=0)
    ta, tb, tt = torch_select(score, x, g, nb, *warp)
    assert np.array_equal(tb, beam) and np.array_equal(tt, tok), (warp, tb.tolist(), beam.tolist(), tt.tolist(), tok.tolist())
    fin = np.isfinite(a)
    assert np.array_equal(np.isfinite(ta), fin) and np.abs(ta[fin] - a[fin]).max(initial=0) <= tol
    return a, beam, tok


WARPS = [(1.0, 0, 1.0), (0.7, 0, 1.0), (1.0, 5, 1.0), (1.3, 0, 0.8), (0.9, 12, 0.6), (1.0, 1, 1.0), (2.0, 40, 0.3)]


@pytest.mark.parametrize("warp", WARPS, ids=str)
@pytest.mark.parametrize("seed", [0, 1, 2])
def test_torch_restatement_equals_numpy_on_random_inputs(seed, warp):
    x, score = random_case(seed, dead=seed == 1)
    assert_same_selection(score, x, BSC.noise(6, 37, 100 + seed, 4), 3, warp)


def test_torch_restatement_equals_numpy_on_designed_inputs():
    """ties in x (equal a in one row: the flat index decides both orders), a dead beam, a row with all but one column filtered (-inf logits:
    fewer finite candidates than 2 nb, so -inf candidates are taken in flat-index order), and - through the walk - eos at ranks < nb and >= nb"""
    from flamingo_mini_amd import decoding as D
    b, nb, V = 2, 3, 11
    x, score = random_case(7, b, nb, V, dead=True)
    x[1, 2] = x[1, 6] = x[1].max() + 1.0                                       # a tie at the top of row 1
    x[3] = -np.inf
    x[3, 4] = 0.5                                                              # all but one filtered
    x[4] = -np.inf
    x[4, 9] = 1.0
    x[5] = -np.inf
    x[5, 0] = -0.5
    score[1] = (0.0, -0.25, -0.5)
    g = BSC.noise(b * nb, V, 5, 3)
    g0 = np.zeros_like(g)
    for warp in ((1.0, 0, 1.0), (1.0, 2, 1.0), (0.8, 0, 0.7)):
        for noise in (g, g0):
            a, beam, tok = assert_same_selection(score, x, noise, nb, warp)
            oa, ob, ot = BSC.order_by_score(a, beam, tok, V)
            ta, tflat = D.order_by_score(*[torch.from_numpy(t) for t in (a, beam, tok)], V)
            assert np.array_equal(tflat.numpy(), ob * V + ot)
    a, beam, tok = assert_same_selection(score, x, g0, nb, (1.0, 0, 1.0))
    assert np.isinf(a[1]).sum() == 2 * nb - 3 and tok[1, 3:].tolist() == [0, 1, 2] and beam[1, 3:].tolist() == [0, 0, 0]      # sequence 1: three finite candidates
    assert {(int(beam[0, i]), int(tok[0, i])) for i in range(2)} == {(1, 2), (1, 6)} and tok[0, 0] == 2                     # the tie: the lower column first
    events = {}
    for eos in range(V):                                                       # every token as eos once: met at ranks < nb and, behind skipped ones, >= nb
        st = BC.new_state(b, nb, 8)
        st["score"][:] = score
        BSC.step(st, x, g0, 4, nb, eos, 0, False, events=events)
    assert events.get("eos_low", 0) > 0 and events.get("eos_high", 0) > 0, events


# ---- (c) the law ----
def test_pairs_drawn_follow_the_plackett_luce_law():
    """V = 6, nb = 1, 20000 sequences sharing the logits, as rows of one call: the unordered pairs drawn against the exact pair probabilities,
    chi-square on 14 degrees of freedom"""
    b, V = 20000, 6
    x = np.array([0.9, 0.1, -0.4, 0.5, -0.1, 0.3], np.float32)
    _, _, beam, tok, _ = BSC.select(np.zeros((b, 1), np.float32), np.tile(x, (b, 1)), BSC.noise(b, V, 20260301, 2), 1, ft=np.float32, extra=0)
    assert (beam == 0).all() and (tok[:, 0] != tok[:, 1]).all()
    probs = BSC.pair_probabilities(x)
    lo, hi = tok.min(1), tok.max(1)
    chi, smallest = BSC.chi_square([int(((lo == i) & (hi == j)).sum()) for i, j in probs], list(probs.values()))
    print(f"pair chi-square {chi:.2f} on 14 degrees of freedom, smallest expected count {smallest:.0f}")
    assert len(probs) == 15 and smallest >= 120 and chi <= BSC.CHI2_Q[14]


@pytest.mark.parametrize("seed", [1, 2, 3, 20260301])
def test_the_entry_of_largest_p_follows_softmax_of_a(seed):
    """V = 8, nb = 2, scores (0, -0.7): each sequence's first candidate against softmax(a) over the 16 entries, 15 degrees of freedom"""
    b, nb, V = 20000, 2, 8
    x = np.stack([np.array([0.9, 0.1, -0.4, 0.5, -0.1, 0.3, 0.7, -0.6], np.float32), np.array([0.2, 0.8, -0.3, 0.0, 0.6, -0.5, 0.4, 1.0], np.float32)])
    score = np.tile(np.array([0.0, -0.7], np.float32), (b, 1))
    _, a, beam, tok, _ = BSC.select(score, np.tile(x, (b, 1)), BSC.noise(b * nb, V, seed, 3), nb, ft=np.float32, extra=0)
    a0 = (x - np.log(np.exp(x.astype(np.float64)).sum(1, keepdims=True)) + np.array([[0.0], [-0.7]])).reshape(-1)
    probs = np.exp(a0) / np.exp(a0).sum()
    chi, smallest = BSC.chi_square(np.bincount(beam[:, 0] * V + tok[:, 0], minlength=nb * V), probs)
    print(f"first-entry chi-square {chi:.2f} on 15 degrees of freedom (seed {seed}), smallest expected count {smallest:.0f}")
    assert smallest >= 120 and chi <= BSC.CHI2_Q[15]


# ---- (d) the noise layout ----
def test_an_entry_of_the_noise_depends_on_seed_length_row_and_column_only():
    base = BSC.words(7, 50, 9, 4)
    assert np.array_equal(BSC.words(3, 50, 9, 4), base[:3]) and np.array_equal(BSC.words(7, 13, 9, 4), base[:, :13])
    assert np.array_equal(BSC.words(9, 1031, 9, 4)[:7, :50], base)
    assert not np.array_equal(BSC.words(7, 50, 10, 4), base) and not np.array_equal(BSC.words(7, 50, 9, 5), base)
    assert not np.array_equal(BSC.words(7, 50, 9 + (1 << 32), 4), base)        # the seed's high word is part of the key
    assert len(np.unique(base)) == base.size
    import sr_cases as SR
    w = SR.philox4x32((3, 5, 4, BSC.TAG), (9, 0))                              # column 14 of row 5: word 2 of call 3
    assert int(base[5, 14]) == int(w[2])


def test_the_uniform_number_lies_strictly_inside_the_unit_interval():
    for ft in (np.float32, np.float64):
        u = BSC.uniform(np.array([0, 0x1FF, 0x200, 0xFFFFFFFF], np.uint32), ft)
        assert u[0] == u[1] == 2.0 ** -24 and u[2] == 3 * 2.0 ** -24 and u[3] == 1 - 2.0 ** -24 and u.dtype == ft
        g = BSC.gumbel(np.array([0, 0xFFFFFFFF], np.uint32), ft)
        assert np.isfinite(g).all() and -2.9 < g[0] < -2.8 and 16.6 < g[1] < 16.7
    from flamingo_mini_amd import decoding as D
    g = D.gumbel_noise_torch((4, 1000), torch.Generator().manual_seed(0))
    assert g.dtype == torch.float32 and bool(torch.isfinite(g).all()) and -2.9 < float(g.min()) and float(g.max()) < 16.7


# ---- the dynamic loop with the restatement's noise is the numpy search ----
@pytest.mark.parametrize("early", [True, False])
def test_dynamic_loop_with_given_noise_equals_the_numpy_search(early):
    """decoding.beam_search(sampling=, noise=) over beam_cases.ScriptedModel against the numpy restatement stepped over the same script and
    the same Philox noise, 12 steps with eos events: the ids and scores it returns are _beam_finalize of the restatement's state"""
    from flamingo_mini_amd import decoding as D
    from flamingo_mini_amd.modeling_flamingo import _beam_finalize
    V, nb, eos, pad, max_len, warp, seed = 300, 4, 7, 0, 14, (0.9, 40, 1.0), 3
    prompt = np.array([[1, 11], [2, 12], [3, 13]], np.int64)
    script = BC.Script(V, 4, eos=eos, eos_boost={1: (4, 9.0), 2: (6, 5.5)})
    st, hist, worst = BC.new_state(3, nb, max_len, 1.0, pad), np.repeat(prompt, nb, axis=0), np.inf
    for cur_len in range(3, max_len + 1):
        worst = min(worst, float(BSC.step(st, script(hist), BSC.noise(3 * nb, V, seed, cur_len), cur_len, nb, eos, pad, early, *warp, ft=np.float64).min()))
        hist = np.concatenate([hist[st["beam_idx"]], st["next_tok"][:, None]], axis=1)
        if st["done"].all():
            break
    assert worst >= 1e-3, "the script is not decidable"
    st["length"], st["eos"] = cur_len, eos
    want_ids, want_s = _beam_finalize(st, 2, prompt, nb, pad, n_return=nb)
    ids = torch.from_numpy(prompt)
    got_ids, got_s = BC.ScriptedModel(script).search(ids, torch.zeros_like(ids), torch.ones_like(ids), None, None, max_len, nb, eos, pad, early, 1.0, n_return=nb,
                                                     sampling=D.Sampling(*warp), noise=lambda rows, V_, cur: torch.from_numpy(BSC.noise(rows, V_, seed, cur)))
    assert torch.equal(got_ids, want_ids)
    torch.testing.assert_close(got_s, want_s, rtol=0, atol=1e-5)
