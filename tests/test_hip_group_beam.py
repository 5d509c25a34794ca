"""Diverse beam search on the graph-replayed decode path, on the GPU: ff_group_beam_step (functional.group_beam_step) against the numpy
restatement of rules A - D (tests/group_beam_cases.py) on designed single steps, against ff_beam_step itself where rule E says the two
coincide, over a scripted multi-step search eager and replayed, inside the beam _DecodeSession of generate(num_beam_groups=2), and on a
property that needs no restatement.

GROUP_SCORE_BOUND, the distance allowed between a score the kernel writes and the float64 value of the same candidate, is SCORE_BOUND's
derivation in tests/test_hip_beam.py - 3.1e-5 for rules 1 - 3 on rows of at most 2^17 columns with |x - max| <= 64, |lse| < 32, |logp| < 64
- plus the two roundings of rule A, under the assumption that the running (penalised) scores satisfy |score| < 64 and lambda * c <= 32, so
that every penalised candidate is below 128 in magnitude, with u = 2^-24:
  fl(lambda * c) <= 32: 32 u = 1.9e-6 (0 for the dyadic lambdas used here; counted all the same);
  fl(f - that) < 128:   128 u = 7.6e-6.
The restatement keeps its float64 results in the state's fp32 fields, which moves a score below 64 by at most 32 u = 1.9e-6.
Total 4.25e-5 <= GROUP_SCORE_BOUND = 4.5e-5, and the designed margin 1e-3 is 22 x that (>= 20 x).  The designed steps use scores in
[-16, 0], logits in [-6, 13] and lambda * c <= 33; the scripted search and the sessions stay far inside the assumed ranges (asserted where
the scores are compared).  Measured worst: the MEASURED lines."""
import contextlib

import numpy as np
import pytest
import torch

import beam_cases as BC
import group_beam_cases as GC
from test_hip_beam import FLT_FIELDS, INT_FIELDS, MARGIN, poison

BF16, F32 = torch.bfloat16, torch.float32
GROUP_SCORE_BOUND = 4.5e-5
assert MARGIN >= 20 * GROUP_SCORE_BOUND


def same_state(got, want, where=""):
    """Integers exact, scores within GROUP_SCORE_BOUND (non-finite entries at the same places with the same value).  Returns the worst error."""
    worst = 0.0
    for n in INT_FIELDS:
        assert np.array_equal(got[n], want[n]), (where, n, got[n].tolist(), want[n].tolist())
    for n in FLT_FIELDS:
        g, w = got[n].astype(np.float64), want[n].astype(np.float64)
        fin = np.isfinite(w)
        assert np.array_equal(np.isfinite(g), fin) and np.array_equal(g[~fin], w[~fin]), (where, n, g.tolist(), w.tolist())
        if fin.any():
            if n != "hist_score":                                                    # (its untouched rows hold the poison)
                assert float(np.abs(w[fin]).max()) < 64, (where, n, "outside the range the bound assumes")
            err = float(np.abs(g[fin] - w[fin]).max())
            assert err <= GROUP_SCORE_BOUND, (where, n, err)
            worst = max(worst, err)
    return worst


def copy_state(host):
    return {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in host.items()}


def group_decidable(detail, x, nb, G, b, designed_ties=False):
    """Per sequence: in every handled group, every gap between consecutive finite scores of the best 2 gs + 1 penalised candidates is >=
    MARGIN - or exactly 0 between two candidates of one row with equal logits and equal counts (equal bits in fp32 too: row, then column
    decide); designed_ties also admits any exact tie inside one row.  Returns (ok (b,), number of exact ties admitted)."""
    gs = nb // G
    ok, zero = np.ones(b, bool), 0
    for (s, g), (top_s, top_b, top_t, counts) in detail.items():
        fin = np.isfinite(top_s)
        f, rows, toks = top_s[fin].astype(np.float64), top_b[fin], top_t[fin]
        for i in range(len(f) - 1):
            gap = f[i] - f[i + 1]
            same_row = rows[i] == rows[i + 1]
            plain = same_row and counts.get(int(toks[i]), 0) == counts.get(int(toks[i + 1]), 0) and \
                x[s * nb + g * gs + rows[i], toks[i]] == x[s * nb + g * gs + rows[i + 1], toks[i + 1]]
            if gap == 0 and (plain or (designed_ties and same_row)):
                zero += 1
            elif gap < MARGIN:
                ok[s] = False
    return ok, zero


# ---------------------------------------------------------------------------------------------------------------------------------------
# 1. designed single steps
# ---------------------------------------------------------------------------------------------------------------------------------------
DESIGNED = [  # (b, nb, G, V, dtype, layout, lambda, ladder step, one variant per sequence, seed)
    (2, 2, 2, 7, F32, "contiguous", 4.125, 0.25, ("deep-eos", "dead0"), 0),
    (2, 4, 2, 257, F32, "contiguous", 0.5, 0.375, ("tie", "twin"), 0),
    (1, 8, 8, 257, F32, "contiguous", 4.125, 0.25, ("deep",), 0),
    (2, 8, 2, 50258, BF16, "last-of-2", 4.125, 0.25, ("deep-eos", "twin"), 0),
    (3, 6, 3, 70001, BF16, "contiguous", 4.125, 0.25, ("deep", "twin", "done0"), 0),
    (1, 4, 4, 65536, BF16, "contiguous", 4.125, 0.25, ("deep",), 0),
]
CASE_ID = lambda c: f"{c[0]}x{c[1]}g{c[2]}x{c[3]}-{str(c[4])[6:]}-{c[5]}"


def design(b, nb, G, V, dtype, lam, ladder, variants, seed):
    """(logits (b nb, V) float32 on the dtype's grid, pre-state overrides, eos, pad, the hot tokens per sequence).  Every row of a sequence
    carries the same ladder of planted logits 13 - ladder * j at the sequence's hot tokens h_0, h_1, ... over a unit-normal background, and
    row j of every group has the score -2 j, so row 0 of a group outranks its other rows: group g then has to take the hot tokens the
    groups before it left over, which sit at the in-row rank g gs and below.  Variants (one per sequence):
      deep      the ladder alone: the last group's winners have the unpenalised in-row rank (G - 1) gs and more;
      deep-eos  (two groups) eos = h_gs: group 1 meets it at rank 0, makes it a hypothesis and takes h_gs+1 .. h_2gs - in-row rank 2 gs;
      twin      row 1 of group 0 has the score -1/16: group 0 takes h_0 (and h_1, ...) from BOTH rows, later groups see the count 2;
      tie       a further token at 13 - lambda: in group 1 it ties with the penalised h_0 exactly, the column decides;
      done0     group 0 is done before the step and pad = h_0: its rows hold the token the next group takes, and count nothing;
      dead0     group 0's rows are dead (-inf) and h_0 = token 0, the token a dead row's -inf candidates carry: it counts nothing."""
    g = np.random.default_rng(4000 + seed)
    gs = nb // G
    n_hot = min(nb + 2 * gs + 2, V - 1)
    x = torch.from_numpy(g.standard_normal((b * nb, V)).astype(np.float32)).to(dtype).float().numpy()
    score = np.tile(np.tile(-2.0 * np.arange(gs, dtype=np.float32), G), (b, 1))
    over = dict(done=np.zeros((b, G), np.int32), n_hyp=np.zeros((b, G), np.int32), hyp_score=np.full((b, nb), -np.inf, np.float32))
    if V < 64:
        hots = [g.permutation(V)[:n_hot] for _ in range(b)]
        while hots[0][1] < 2:                                                   # (the eos of deep-eos: not a token a dead row carries)
            hots[0] = g.permutation(V)[:n_hot]
    else:
        pool = 2 * gs + g.choice(V - 2 * gs, b * (n_hot + 1), replace=False)
        hots = [pool[s * (n_hot + 1):(s + 1) * (n_hot + 1)] for s in range(b)]  # (one spare per sequence: the tie token)
    eos, pad = None, 1
    for s, variant in enumerate(variants):
        hot = [int(t) for t in hots[s]]
        if variant == "dead0":
            hot = [0] + [t for t in hot if t != 0][:n_hot - 1]
            score[s, :gs] = -np.inf
        if variant == "deep-eos":
            eos = hot[gs]
        if variant == "twin":
            score[s, 1] = -1.0 / 16
        if variant == "done0":
            pad = hot[0]
            over["done"][s, 0], over["n_hyp"][s, 0] = 1, gs
            over["hyp_score"][s, :gs] = -0.5 - 0.25 * np.arange(gs)
        for j, t in enumerate(hot[:n_hot]):
            x[s * nb:(s + 1) * nb, t] = 13.0 - ladder * j
        if variant == "tie":
            x[s * nb:(s + 1) * nb, hot[n_hot]] = 13.0 - lam
        hots[s] = hot
    assert eos is None or eos != pad
    return torch.from_numpy(x).to(dtype).float().numpy(), score, over, eos, pad, hots


def start_state(b, nb, G, max_len, score, over, pad):
    st = GC.new_state(b, nb, G, max_len, 1.0, pad)
    st["score"][:] = score
    for n, v in over.items():
        st[n][:] = v
    return st


def check_designed(case):
    """The preconditions of a designed step, in float64 (no GPU): every decision keeps the margin or ties exactly as designed, and every
    planted event really happens.  Returns what the GPU test needs."""
    b, nb, G, V, dtype, layout, lam, ladder, variants, seed = case
    gs = nb // G
    x, score, over, eos, pad, hots = design(b, nb, G, V, dtype, lam, ladder, variants, seed)
    assert np.abs(x).max() <= 13 and np.isfinite(score).any() and lam * nb <= 33 and score[np.isfinite(score)].min() >= -16
    st, detail, events = start_state(b, nb, G, 8, score, over, pad), {}, {}
    GC.step(st, x, 5, nb, G, lam, eos, pad, False, ft=np.float64, events=events, detail=detail)
    ok, zero = group_decidable(detail, x, nb, G, b, designed_ties=True)
    assert ok.all(), "planted scores closer than the margin"
    assert zero == (1 if "tie" in variants else 0), zero
    unpen = GC.row_scores(score, x, np.float64).reshape(b, nb, V)
    for s, variant in enumerate(variants):
        live = [k for k in range(nb) if st["score"][s, k] > -np.inf]
        toks = {k: int(st["next_tok"][s * nb + k]) for k in live}
        if variant in ("deep", "deep-eos"):                                     # a winner of the last group from in-row rank >= 2 gs ...
            k = nb - 1
            row = int(st["beam_idx"][s * nb + k]) - s * nb
            rank = int((unpen[s, row] > unpen[s, row, toks[k]]).sum())
            assert rank >= 2 * gs, (variant, rank)
            # ... so a kernel that keeps only the best 2 gs of every row cannot find it: the restatement fed such rows chooses otherwise
            cut = x.copy()
            for r in range(s * nb, (s + 1) * nb):
                cut[r, np.argsort(-x[r], kind="stable")[2 * gs:]] = -1e4
            alt = start_state(b, nb, G, 8, score, over, pad)
            GC.step(alt, cut, 5, nb, G, lam, eos, pad, False, ft=np.float64)
            assert not np.array_equal(alt["next_tok"][s * nb:(s + 1) * nb], st["next_tok"][s * nb:(s + 1) * nb])
            if G == 8:
                assert len(detail[(s, G - 1)][3]) == 7 and toks[k] == hots[s][7]                # the last of 8 groups: 7 penalised tokens
        if variant == "deep-eos":
            assert st["n_hyp"][s].tolist() == [0, 1] and st["hyp_row"][s, gs] == s * nb + gs and toks[nb - 1] == hots[s][2 * gs]
        if variant == "twin":
            assert toks[0] == toks[1] == hots[s][0] and max(detail[(s, 1)][3].values()) == 2
            if lam < 1:                                                         # (the small lambda: h_0 at 2 lambda is still among the ranked 2 gs)
                assert any(detail[(s, 1)][3].get(int(t), 0) == 2 for t in detail[(s, 1)][2][:2 * gs])
        if variant == "tie":
            top_s, _, top_t, counts = detail[(s, 1)]
            assert top_s[0] == top_s[1] and sorted(counts.get(int(t), 0) for t in top_t[:2]) == [0, 1] and top_t[0] < top_t[1]
        if variant == "done0":
            assert not any(k < gs for k in live) and toks[gs] == pad and (st["next_tok"][s * nb:s * nb + gs] == pad).all()
        if variant == "dead0":
            assert not any(k < gs for k in live) and st["next_tok"][s * nb] == 0 and toks[gs] == 0
    if "done0" in variants:
        assert events.get("pad_uncounted", 0) > 0 and events.get("mixed", 0) > 0
    return x, score, over, eos, pad, detail


@pytest.mark.parametrize("case", DESIGNED, ids=CASE_ID)
def test_designed_cases_are_decidable_and_hold_their_events(case):
    check_designed(case)


@pytest.mark.gpu
@pytest.mark.parametrize("case", DESIGNED, ids=CASE_ID)
def test_designed_steps_match_the_reference_exactly(case):
    """One step from a designed state: the whole state block afterwards equals the float64 restatement's, integers exactly, scores within
    GROUP_SCORE_BOUND.  State and workspace come from the guarded, poisoned seam."""
    from guarded import guarded_allocations
    from flamingo_mini_amd import functional as F
    b, nb, G, V, dtype, layout, lam, ladder, variants, seed = case
    x, score, over, eos, pad, detail = check_designed(case)
    max_len, cur = 8, 5
    xt = torch.from_numpy(x).to(dtype)
    if layout == "last-of-2":
        buf = torch.full((b * nb, 2, V), float("nan"), dtype=dtype)
        buf[:, 1] = xt
        dev = buf.cuda()[:, -1]
    else:
        dev = xt.cuda()
    with guarded_allocations() as g:
        st = F.BeamState(b, nb, max_len, "cuda", eos=eos, pad=pad, early_stopping=False, length_penalty=1.0, n_groups=G)
        assert st.done.shape == (b, G) and st.n_hyp.shape == (b, G)
        poison(st)
        st.score.copy_(torch.from_numpy(score))
        for n, v in over.items():
            getattr(st, n).copy_(torch.from_numpy(v))
        pre = st.to_host()
        nxt, idx = F.group_beam_step(dev, st, torch.tensor([cur], device="cuda"), lam)
        post = st.to_host()
        g.check()
    assert nxt.data_ptr() == st.next_tok.data_ptr() and idx.data_ptr() == st.beam_idx.data_ptr()
    ref = copy_state(pre)
    GC.step(ref, x, cur, nb, G, lam, eos, pad, False, ft=np.float64)
    worst = same_state(post, ref, where=CASE_ID(case))
    print(f"MEASURED group_beam_step score error {worst:.3e} (bound {GROUP_SCORE_BOUND:.1e}) at {case[:4]}")


@pytest.mark.gpu
def test_a_nan_row_and_an_inf_row_leave_every_index_in_range():
    """Rule F: the guards are intact and every integer the step wrote lies inside its table."""
    from guarded import guarded_allocations
    from flamingo_mini_amd import functional as F
    b, nb, G, V, max_len, cur = 2, 4, 2, 257, 8, 5
    x = torch.from_numpy(np.random.default_rng(5).standard_normal((b * nb, V)).astype(np.float32))
    x[1] = float("nan")
    x[2, 5] = float("nan")
    x[6] = float("inf")
    x[7, 9] = float("inf")
    with guarded_allocations() as g:
        st = F.BeamState(b, nb, max_len, "cuda", eos=3, pad=1, early_stopping=False, n_groups=G)
        st.score.copy_(torch.from_numpy(-np.arange(b * nb, dtype=np.float32).reshape(b, nb) / 8))
        F.group_beam_step(x.cuda(), st, torch.tensor([cur], device="cuda"), 0.5)
        post = st.to_host()
        g.check()
    rows = np.arange(b * nb)
    assert ((post["next_tok"] >= 0) & (post["next_tok"] < V)).all()
    assert (post["beam_idx"] // (nb // G) == rows // (nb // G)).all(), "a parent outside the row's group"
    assert np.array_equal(post["hist_tok"][cur - 1], post["next_tok"]) and np.array_equal(post["hist_parent"][cur - 1], post["beam_idx"])
    assert ((post["n_hyp"] >= 0) & (post["n_hyp"] <= nb // G)).all() and np.isin(post["done"], (0, 1)).all()
    assert np.isin(post["hyp_len"], (0, cur)).all() and ((post["hyp_row"] >= 0) & (post["hyp_row"] < b * nb)).all()
    assert (post["hist_tok"][np.arange(max_len) != cur - 1] == 0).all()


# ---------------------------------------------------------------------------------------------------------------------------------------
# 2. rule E on the device: lambda = 0 is ff_beam_step per group, one group is ff_beam_step
# ---------------------------------------------------------------------------------------------------------------------------------------
def random_start(b, nb, G, V, dtype, seed, eos):
    """A state in the middle of a search: scores with dead beams, a done group, groups with hypotheses; logits with the eos column high."""
    g = np.random.default_rng(seed)
    gs = nb // G
    x = torch.from_numpy((g.standard_normal((b * nb, V)) * 2).astype(np.float32)).to(dtype)
    x[:, eos] = torch.from_numpy((4 + 2 * g.random(b * nb)).astype(np.float32)).to(dtype)
    score = -(g.integers(0, 64, (b, nb)) / 8.0).astype(np.float32)
    score[g.random((b, nb)) < 0.15] = -np.inf
    n_hyp = g.integers(0, gs + 1, (b, G)).astype(np.int32)
    done = np.zeros((b, G), np.int32)
    done[0, G - 1], n_hyp[0, G - 1] = 1, gs
    hs = -np.sort(g.random((b, G, gs)) * 4, axis=-1).astype(np.float32)
    hs[np.arange(gs)[None, None] >= n_hyp[..., None]] = -np.inf
    return x, dict(score=score, n_hyp=n_hyp, done=done, hyp_score=hs.reshape(b, nb))


@pytest.mark.gpu
@pytest.mark.parametrize("b,nb,G,V,dtype", [(2, 4, 2, 257, F32), (3, 6, 3, 50258, BF16), (2, 8, 4, 1000, BF16), (1, 8, 8, 70001, BF16)],
                         ids=lambda v: str(v).replace("torch.", ""))
@pytest.mark.parametrize("early", [True, False])
def test_without_a_penalty_every_group_is_ff_beam_step_on_its_rows(b, nb, G, V, dtype, early):
    """Group g's scores, tokens, parents, histories and hypotheses after ff_group_beam_step(lambda = 0) equal ff_beam_step run with nb = gs
    on that group's rows and its slice of the state: integers exact, scores bit for bit."""
    from flamingo_mini_amd import functional as F
    gs, eos, cur_len, max_len = nb // G, 11, 5, 8
    x, start = random_start(b, nb, G, V, dtype, 100 * nb + G, eos)
    cur = torch.tensor([cur_len], device="cuda")
    st = F.BeamState(b, nb, max_len, "cuda", eos=eos, pad=2, early_stopping=early, length_penalty=0.6, n_groups=G)
    for n, v in start.items():
        getattr(st, n).copy_(torch.from_numpy(v))
    F.group_beam_step(x.cuda(), st, cur, 0.0)
    post = st.to_host()
    for g in range(G):
        rows = (np.arange(b)[:, None] * nb + g * gs + np.arange(gs)[None]).reshape(-1)
        one = F.BeamState(b, gs, max_len, "cuda", eos=eos, pad=2, early_stopping=early, length_penalty=0.6)
        one.score.copy_(torch.from_numpy(start["score"][:, g * gs:(g + 1) * gs]))
        one.hyp_score.copy_(torch.from_numpy(start["hyp_score"][:, g * gs:(g + 1) * gs]))
        one.n_hyp.copy_(torch.from_numpy(start["n_hyp"][:, g]))
        one.done.copy_(torch.from_numpy(start["done"][:, g]))
        F.beam_step(x[rows].cuda(), one, cur)
        want, got = one.to_host(), GC.group_slice(post, g, nb, G)
        fresh = np.arange(gs)[None] < want["n_hyp"][:, None]                         # hypothesis slots in use
        for n in BC.FIELDS:
            w, h = want[n], got[n]
            if n.startswith("hist_"):                                                # (this step's row; the others were never written)
                w, h = w[cur_len - 1], h[cur_len - 1]
            if n in ("hyp_len", "hyp_row"):                                          # (slots the start state filled carry no row; unused ones 0)
                made = fresh & (want["hyp_len"] == cur_len)
                w, h = w[made], h[made]
            assert np.array_equal(w.view(np.int32) if w.dtype == np.float32 else w, h.view(np.int32) if h.dtype == np.float32 else h), (g, n)


@pytest.mark.gpu
@pytest.mark.parametrize("nb,V,dtype", [(3, 257, F32), (8, 50258, BF16)], ids=lambda v: str(v).replace("torch.", ""))
def test_one_group_through_the_group_entry_point_is_ff_beam_step_bit_for_bit(nb, V, dtype):
    from flamingo_mini_amd import functional as F
    b, eos, max_len = 3, 11, 8
    x, start = random_start(b, nb, 1, V, dtype, 7 + nb, eos)
    blocks = []
    for fn in (lambda st, c: F.beam_step(x.cuda(), st, c), lambda st, c: F.group_beam_step(x.cuda(), st, c, 0.0)):
        st = F.BeamState(b, nb, max_len, "cuda", eos=eos, pad=2, early_stopping=False, length_penalty=2.0)
        assert st.n_groups == 1 and st.done.shape == (b,)
        for n, v in start.items():
            getattr(st, n).copy_(torch.from_numpy(v.reshape(getattr(st, n).shape)))
        fn(st, torch.tensor([5], device="cuda"))
        blocks.append(st.storage.cpu())
    assert torch.equal(blocks[0], blocks[1])


# ---------------------------------------------------------------------------------------------------------------------------------------
# 3. twelve scripted steps, eager and from one captured graph
# ---------------------------------------------------------------------------------------------------------------------------------------
MS_V, MS_NB, MS_G, MS_LAM, MS_EOS, MS_PAD, MS_MAXLEN = 257, 4, 2, 0.5, 7, 0, 14
MS_PROMPT = np.array([[1, 11], [2, 12], [3, 13]], np.int64)
MS_BOOST = {1: (4, 9.0), 2: (6, 5.5)}
MS_SEEDS = {True: 0, False: 0}       # a table whose runs keep every margin >= 1e-3 and hold the events (both asserted on the way)


def scripted_run(early):
    """The restatement (float32) over the script: (script, logits per step, states before every step, events); asserts the margins."""
    script = BC.Script(MS_V, MS_SEEDS[early], eos=MS_EOS, eos_boost=MS_BOOST)
    st, events, steps = GC.new_state(3, MS_NB, MS_G, MS_MAXLEN, 1.0, MS_PAD), {}, []
    hist = np.repeat(MS_PROMPT, MS_NB, axis=0)
    for cur_len in range(3, MS_MAXLEN + 1):
        logits, live = script(hist), st["done"] == 0
        tops = GC.step(st, logits, cur_len, MS_NB, MS_G, MS_LAM, MS_EOS, MS_PAD, early, events=events)
        margin = BC.min_margin(tops.reshape(3 * MS_G, -1)).reshape(3, MS_G)[live].min(initial=np.inf)
        assert margin >= MARGIN, f"step {cur_len} of the script is not decidable: {margin:.2e}"
        steps.append((cur_len, logits))
        hist = np.concatenate([hist[st["beam_idx"]], st["next_tok"][:, None]], axis=1)
    assert all(events.get(k, 0) > 0 for k in ("eos_low", "eos_high", "done", "mixed")), events
    return steps, events


@pytest.mark.parametrize("early", [True, False])
def test_the_script_keeps_every_margin_and_holds_the_events(early):
    scripted_run(early)


@pytest.mark.gpu
@pytest.mark.parametrize("early", [True, False])
def test_state_block_after_every_step_of_a_scripted_search(early):
    """12 steps, V = 257, 3 sequences x 4 beams in 2 groups, eos at low and high ranks, groups done while others run.  Before every step the
    device state is copied; the restatement (float32) advances the copy and the device state after the step must equal it as a WHOLE.  Once
    with eager calls, once replaying ONE captured graph whose logits buffer and cur_len are updated on the device; the two final blocks are
    equal bit for bit."""
    from guarded import guarded_allocations
    from flamingo_mini_amd import functional as F
    steps, _ = scripted_run(early)
    final, worst = [], 0.0
    for replayed in (False, True):
        with guarded_allocations() as g:
            st = F.BeamState(3, MS_NB, MS_MAXLEN, "cuda", eos=MS_EOS, pad=MS_PAD, early_stopping=early, length_penalty=1.0, n_groups=MS_G)
            poison(st)
            cur = torch.full((1,), MS_MAXLEN, dtype=torch.long, device="cuda")
            buf = torch.zeros((3 * MS_NB, MS_V), dtype=torch.float32, device="cuda")
            if replayed:
                scratch = F.BeamState(3, MS_NB, MS_MAXLEN, "cuda", eos=MS_EOS, pad=MS_PAD, early_stopping=early, n_groups=MS_G)
                F.group_beam_step(buf, scratch, cur, MS_LAM)                          # eager once, on a state of its own
                graph = torch.cuda.CUDAGraph()
                torch.cuda.synchronize()
                keep = st.storage.clone()
                with torch.cuda.graph(graph):
                    F.group_beam_step(buf, st, cur, MS_LAM)
                st.storage.copy_(keep)
            for cur_len, logits in steps:
                pre = st.to_host()
                buf.copy_(torch.from_numpy(logits))
                cur.fill_(cur_len)
                if replayed:
                    graph.replay()
                else:
                    F.group_beam_step(buf, st, cur, MS_LAM)
                post = st.to_host()
                ref = copy_state(pre)
                GC.step(ref, logits, cur_len, MS_NB, MS_G, MS_LAM, MS_EOS, MS_PAD, early)
                worst = max(worst, same_state(post, ref, where=f"step {cur_len} replayed {replayed}"))
            g.check()
        final.append(st.storage.cpu())
    print(f"MEASURED multi-step group score error {worst:.3e}")
    assert torch.equal(final[0], final[1]), "eager and replayed steps differ in some bit"


# ---------------------------------------------------------------------------------------------------------------------------------------
# 4. the diverse beam decode session (G1 geometry of tests/test_hip_decode.py, batch 4, 4 beams in 2 groups)
# ---------------------------------------------------------------------------------------------------------------------------------------
NB, NG, LAM = 4, 2, 0.5
TAG = "group-beam"


def group_generate(model, inputs, max_length, graph=True, rec=None, **kw):
    ids, ml, am, vf = inputs
    model.decode_graph = graph
    with (rec.installed() if rec is not None else contextlib.nullcontext()):
        out = model.generate(ids, media_locations=ml, attention_mask=am, visual_features=vf, max_length=max_length, num_beams=NB,
                             num_beam_groups=NG, diversity_penalty=LAM, static_decode=True, **kw)
    model.decode_graph = True
    return out


def replay_restatement(sess, logits, L0, length, eos, early, lp):
    """The restatement (float32) driven by the logits the session recorded: the final state, with "length" and "eos"."""
    st = GC.new_state(sess.n_seq, NB, NG, sess.max_length, lp, sess.fill)
    for pos in range(L0, length):
        GC.step(st, logits[:, pos], pos + 1, NB, NG, LAM, eos, sess.fill, early)
    st["length"], st["eos"] = length, -1 if eos is None else eos
    return st


@pytest.fixture(scope="module")
def g1():
    import test_hip_decode as D
    model, model64 = D.models("gpt2")
    inputs = D.make_inputs(4, 1, TAG)
    model.reset_decode_sessions()
    yield D, model, model64, inputs
    model.decode_graph = True
    model.reset_decode_sessions()
    D._MODELS.clear()


@pytest.fixture(scope="module")
def base_run(g1):
    """the replayed run without eos, recorder installed: (ids, recorded logits (rows, max_length, V), host state, session)"""
    from test_hip_sampling import _SampleRecorder
    D, model, _, inputs = g1
    rec = _SampleRecorder()
    out = group_generate(model, inputs, D.MAXLEN, rec=rec)
    sess = rec.session
    return out, sess._rec.clone().cpu().numpy(), sess.state.to_host(), sess


def decidable_steps(logits, host, L0, length, fill):
    """Per (sequence, position): the float64 transition from the session's own scores before the step, and whether it is decidable.
    Returns (ok (b, length - L0) bool, the float64 states after every step)."""
    b = host["score"].shape[0]
    ok, after = np.ones((b, length - L0), bool), []
    for pos in range(L0, length):
        x = logits[:, pos]
        assert np.isfinite(x).all()
        st = GC.new_state(b, NB, NG, host["hist_tok"].shape[0], 1.0, fill)
        if pos > L0:
            st["score"][:] = host["hist_score"][pos - 1].reshape(b, NB)
        detail = {}
        GC.step(st, x, pos + 1, NB, NG, LAM, None, fill, True, ft=np.float64, detail=detail)
        ok[:, pos - L0] = group_decidable(detail, x, NB, NG, b)[0]
        after.append(st)
    return ok, after


@pytest.mark.gpu
def test_session_replays_a_graph_and_every_step_follows_the_rules(g1, base_run):
    """A group session exists under its own key and its graph really runs; every step's transition - the session's own hist_score before the
    step plus the recorded logits in, the history row after the step out - equals the float64 restatement wherever that is decidable; at
    most 5 % of the (sequence, step) pairs may be undecidable; the returned ids are _beam_finalize of the restatement's final state."""
    from flamingo_mini_amd.decoding import Groups, _beam_finalize
    D, model, _, inputs = g1
    out, logits, host, sess = base_run
    keys = [k for k, s in model._decode_sessions.items() if s is sess]
    assert keys and keys[0][-1] == Groups(NG, LAM) and keys[0][8] == (NB, True, 1.0) and sess.groups == (NG, LAM) and sess.b == 4 * NB
    assert sess.replay is not None and not sess.capture_failed and sess.state.n_groups == NG and host["done"].shape == (4, NG)
    assert out.shape == (4, D.MAXLEN) and torch.equal(out[:, :D.L0], inputs[0])
    ok, after = decidable_steps(logits, host, D.L0, D.MAXLEN, sess.fill)
    bad, worst = [], 0.0
    for i, pos in enumerate(range(D.L0, D.MAXLEN)):
        for s in np.flatnonzero(ok[:, i]):
            r = slice(s * NB, (s + 1) * NB)
            got = (host["hist_tok"][pos, r].tolist(), host["hist_parent"][pos, r].tolist())
            want = (after[i]["next_tok"][r].tolist(), after[i]["beam_idx"][r].tolist())
            if got != want:
                bad.append((s, pos, got, want))
            else:
                assert np.abs(host["hist_score"][pos, r]).max() < 64
                worst = max(worst, float(np.abs(host["hist_score"][pos, r].astype(np.float64) - after[i]["score"][s].astype(np.float64)).max()))
    total = ok.size
    print(f"MEASURED group session undecidable {total - int(ok.sum())} of {total}; score error {worst:.3e}")
    assert not bad, f"(sequence, position, got, want): {bad[:4]}"
    assert worst <= GROUP_SCORE_BOUND
    assert total - int(ok.sum()) <= 0.05 * total, total - int(ok.sum())
    st = replay_restatement(sess, logits, D.L0, D.MAXLEN, None, True, 1.0)
    assert torch.equal(out.cpu(), _beam_finalize(st, D.L0, inputs[0].cpu(), NB, sess.fill, n_groups=NG))


@pytest.mark.gpu
def test_session_eager_steps_equal_the_replayed_graph(g1, base_run):
    D, model, _, inputs = g1
    eager = group_generate(model, inputs, D.MAXLEN, graph=False)
    sess = [s for s in model._decode_sessions.values() if s.groups is not None and not s.graph_wanted]
    assert sess and sess[0].replay is None
    assert torch.equal(eager, base_run[0])


@pytest.mark.gpu
def test_static_result_equals_the_dynamic_loop_on_the_same_logits(g1, base_run):
    """The dynamic loop (decoding.beam_search with groups) is driven by the logits the session recorded, looked up by a row's token history
    (rebuilt from hist_parent): for every sequence whose steps were all decidable it returns the session's ids and scores.  (The two paths
    of generate() compute their logits with different kernels in bf16, one ulp of which is 60 x the margin; on logits of its own the loop
    may rightly choose otherwise, so the rules are compared on ONE set of logits.)"""
    from flamingo_mini_amd import decoding as Dec
    D, model, _, inputs = g1
    out, logits, host, sess = base_run
    ok, _ = decidable_steps(logits, host, D.L0, D.MAXLEN, sess.fill)
    good = np.flatnonzero(ok.all(1))
    assert len(good) > 0, "no sequence with every step decidable"
    prompt = inputs[0].cpu()
    table = {}
    hist = np.repeat(prompt.numpy(), NB, axis=0)
    for pos in range(D.L0, D.MAXLEN):
        for r in range(4 * NB):
            table[tuple(hist[r])] = logits[r, pos]
        hist = np.concatenate([hist[host["hist_parent"][pos]], host["hist_tok"][pos][:, None]], axis=1)

    class Scripted(BC.ScriptedModel):
        def _decode_step(self, step_ids, ml, am, past, pixel_values, visual_features):
            h = step_ids if past is None else torch.cat([past[0][0][0], step_ids], dim=1)
            zero = np.zeros_like(logits[0, D.L0])
            x = np.stack([table.get(tuple(row), zero) for row in h.tolist()])          # (an unknown history: a sequence that left the recorded path)
            return torch.from_numpy(x), (((h, h),), ((h, h),))

    res = group_generate(model, inputs, D.MAXLEN, num_return_sequences=NB, return_dict_in_generate=True)
    ids = prompt[good]
    got_ids, got_s = Scripted(None).search(ids, torch.zeros_like(ids), torch.ones_like(ids), None, None, D.MAXLEN, NB, None, sess.fill, True, 1.0,
                                           n_return=NB, groups=Dec.Groups(NG, LAM))
    pick = (good[:, None] * NB + np.arange(NB)[None]).reshape(-1)
    assert torch.equal(got_ids, res.sequences.cpu()[pick]), (good, got_ids.tolist(), res.sequences.cpu()[pick].tolist())
    torch.testing.assert_close(got_s, res.sequences_scores.cpu()[pick], rtol=0, atol=1e-4)
    assert torch.equal(res.sequences[::NB], out)


@pytest.mark.gpu
def test_a_second_call_with_another_prompt_reuses_the_session(g1, base_run):
    D, model, _, inputs = g1
    sess = base_run[3]
    other = D.make_inputs(4, 1, TAG + "-other")
    assert not torch.equal(other[0], inputs[0])
    from test_hip_sampling import _SampleRecorder
    rec = _SampleRecorder()
    out = group_generate(model, other, D.MAXLEN, rec=rec)
    assert rec.session is sess and sess.replay is not None
    eager = group_generate(model, other, D.MAXLEN, graph=False)
    assert torch.equal(out, eager) and torch.equal(out[:, :D.L0], other[0])
    assert torch.equal(group_generate(model, inputs, D.MAXLEN), base_run[0])           # ... and the first prompt again gives what it gave


@pytest.mark.gpu
def test_num_return_sequences_returns_sorted_scores_in_rows_s_n_plus_j(g1, base_run):
    from flamingo_mini_amd.decoding import _beam_finalize
    D, model, _, inputs = g1
    out, logits, host, sess = base_run
    res = group_generate(model, inputs, D.MAXLEN, num_return_sequences=NB, return_dict_in_generate=True)
    st = replay_restatement(sess, logits, D.L0, D.MAXLEN, None, True, 1.0)
    want_ids, want_s = _beam_finalize(st, D.L0, inputs[0].cpu(), NB, sess.fill, n_return=NB, n_groups=NG)
    assert res.sequences.shape == (4 * NB, D.MAXLEN) and torch.equal(res.sequences.cpu(), want_ids) and torch.equal(res.sequences[::NB], out)
    torch.testing.assert_close(res.sequences_scores.cpu(), want_s, rtol=0, atol=GROUP_SCORE_BOUND)
    s = res.sequences_scores.reshape(4, NB)
    assert bool(torch.isfinite(s).all()) and bool((s[:, :-1] >= s[:, 1:]).all())


@pytest.mark.gpu
@pytest.mark.parametrize("early", [True, False])
def test_session_with_processors_bad_words_and_eos_together(g1, base_run, early):
    """repetition_penalty, no_repeat_ngram_size, bad_words_ids and an eos the plain run produced, in one call: the session carries all of
    them beside the groups, replayed and eager runs agree, no returned row repeats a bigram or holds the banned token, and every row is
    padding after its eos."""
    D, model, _, inputs = g1
    gen = base_run[0][:, D.L0:]
    toks = sorted((int(t) for t in gen.flatten().unique()), key=lambda t: -int((gen == t).sum()))
    eos, banned = toks[0], toks[1]
    pad = 0 if eos != 0 else 1
    kw = dict(eos_token_id=eos, pad_token_id=pad, early_stopping=early, length_penalty=0.0, repetition_penalty=1.3, no_repeat_ngram_size=2,
              bad_words_ids=[[banned]])
    from test_hip_sampling import _SampleRecorder
    rec = _SampleRecorder()
    out = group_generate(model, inputs, D.MAXLEN, rec=rec, **kw)
    sess = rec.session
    assert sess.replay is not None and sess.groups == (NG, LAM) and sess.processors is not None and sess.constraints is not None
    assert sess.seq_buf.shape == (4 * NB, D.MAXLEN)
    assert torch.equal(out, group_generate(model, inputs, D.MAXLEN, graph=False, **kw))
    host = sess.state.to_host()
    assert host["done"].shape == (4, NG)
    for row in out.cpu().tolist():
        g = row[D.L0:]
        if eos in g:
            assert all(t == pad for t in g[g.index(eos) + 1:]), (eos, pad, row)
            g = g[:g.index(eos) + 1]
        assert banned not in g, (banned, row)
        full = row[:D.L0] + g
        grams = list(zip(full[:-1], full[1:]))
        assert len(set(grams[D.L0 - 1:]) & set(grams[:D.L0 - 1])) == 0 and len(set(grams[D.L0 - 1:])) == len(grams[D.L0 - 1:]), row
    print(f"MEASURED group session with processors: hypotheses {host['n_hyp'].tolist()}, done {host['done'].tolist()}")


# ---------------------------------------------------------------------------------------------------------------------------------------
# 5. a property that needs no restatement
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("b,nb,G,V,dtype", [(3, 4, 4, 257, F32), (2, 8, 4, 50258, BF16), (2, 6, 2, 1000, BF16)], ids=lambda v: str(v).replace("torch.", ""))
def test_a_large_penalty_makes_the_groups_differ_and_no_penalty_makes_them_agree(b, nb, G, V, dtype):
    """From the initial state every group sees the same row.  With lambda above the step's largest log-probability gap a token taken by an
    earlier group falls below every free one: the first tokens of the groups' leading beams are pairwise different.  With lambda = 0 they
    are the row's argmax, all equal."""
    from flamingo_mini_amd import functional as F
    gs = nb // G
    x = torch.from_numpy((np.random.default_rng(V + nb).standard_normal((b, V)) * 2).astype(np.float32)).to(dtype)
    x = x.repeat_interleave(nb, 0).cuda()
    gap = float(x.float().max() - x.float().min())
    lead = {}
    for lam in (0.0, 2.0 * gap):
        st = F.BeamState(b, nb, 6, "cuda", eos=None, pad=0, n_groups=G)
        nxt, _ = F.group_beam_step(x, st, torch.tensor([3], device="cuda"), lam)
        lead[lam] = nxt.cpu().reshape(b, G, gs)[:, :, 0]
        assert bool(torch.isfinite(st.score).all())
    assert all(len(set(r)) == 1 for r in lead[0.0].tolist()) and torch.equal(lead[0.0][:, 0], x.float().argmax(-1).cpu()[::nb])
    assert all(len(set(r)) == G for r in lead[2.0 * gap].tolist()), lead
