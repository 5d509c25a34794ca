"""Diverse beam search without a GPU: the numpy restatement of rules A - D (tests/group_beam_cases.py) is held to three oracles that share none
of its group code - the plain restatement for G = 1, the plain restatement run per group for lambda = 0, a float64 brute force over the full
penalised matrix at tiny sizes - and the dynamic loop (FlamingoModel._beam_search with groups) is held to the restatement plus
_beam_finalize, token for token, on scripts whose every decision keeps a gap of 1e-3."""
import copy

import numpy as np
import pytest
import torch

import beam_cases as BC
import group_beam_cases as GC

V, L0, MAXLEN, EOS, PAD = 40, 2, 14, 7, 0
PROMPT = np.array([[1, 11], [2, 12], [3, 13]], np.int64)
BOOST = {1: (4, 9.0), 2: (6, 5.5)}          # as tests/test_beam_args.py: sequence "1" finishes early, "2" meets eos at high ranks, "3" never


def _same(a, b, fields=GC.FIELDS):
    for n in fields:
        x, y = np.asarray(a[n]), np.asarray(b[n])
        assert x.size == y.size and np.array_equal(x.reshape(-1), y.reshape(-1), equal_nan=x.dtype.kind == "f"), n


@pytest.mark.parametrize("early,eos,seed", [(True, EOS, 8), (False, EOS, 29), (True, None, 121)])
def test_one_group_is_the_plain_restatement_field_for_field(early, eos, seed):
    script = BC.Script(V, seed, eos=eos, eos_boost=BOOST)
    nb = 3
    a, b = BC.new_state(3, nb, MAXLEN, 1.0, PAD), GC.new_state(3, nb, 1, MAXLEN, 1.0, PAD)
    hist = np.repeat(PROMPT, nb, axis=0)
    while hist.shape[1] < MAXLEN:
        x, live = script(hist), a["done"] == 0
        top_a = BC.step(a, x, hist.shape[1] + 1, nb, eos, PAD, early)
        top_b = GC.step(b, x, hist.shape[1] + 1, nb, 1, 0.0, eos, PAD, early)
        _same(a, b)
        assert np.array_equal(top_a[live], top_b[live, 0])                # (the margins of a done group are not reported)
        hist = np.concatenate([hist[a["beam_idx"]], a["next_tok"][:, None]], axis=1)


@pytest.mark.parametrize("nb,G", [(4, 2), (6, 3), (6, 2)])
@pytest.mark.parametrize("early", [True, False])
def test_without_a_penalty_every_group_is_a_plain_search_of_its_own(nb, G, early):
    """Rule E.  The groups are first driven apart by a few penalised steps, then every step with lambda = 0 must move group g's slice of the
    state exactly as beam_cases.step moves it with nb = gs on the group's rows of the logits."""
    gs = nb // G
    script = BC.Script(V, 1000 + 10 * nb + G, eos=EOS, eos_boost={1: (5, 7.0), 2: (6, 5.5)})
    st = GC.new_state(3, nb, G, MAXLEN, 1.0, PAD)
    hist = np.repeat(PROMPT, nb, axis=0)
    for i in range(MAXLEN - L0):
        cur_len, x = hist.shape[1] + 1, script(hist)
        if i < 3:
            GC.step(st, x, cur_len, nb, G, 1.5, EOS, PAD, early)
        else:
            before = [GC.group_slice(st, g, nb, G) for g in range(G)]
            GC.step(st, x, cur_len, nb, G, 0.0, EOS, PAD, early)
            for g in range(G):
                rows = (np.arange(3)[:, None] * nb + g * gs + np.arange(gs)[None]).reshape(-1)
                BC.step(before[g], x[rows], cur_len, gs, EOS, PAD, early)
                _same(before[g], GC.group_slice(st, g, nb, G))
        hist = np.concatenate([hist[st["beam_idx"]], st["next_tok"][:, None]], axis=1)
    assert len({tuple(h) for h in hist[:nb].tolist()}) > gs, "the penalised steps did not drive the groups apart"


def _brute_force(score, logits, nb, G, lam, eos, pad, done, n_hyp, hyp_score, norm, early):
    """One step of rules A and B in float64 over the FULL penalised (gs V) matrix of every group, sorted as a list of tuples."""
    x = np.asarray(logits, np.float64)
    logp = x - np.log(np.exp(x - x.max(1, keepdims=True)).sum(1, keepdims=True)) - x.max(1, keepdims=True)
    b, gs, Vv = score.shape[0], nb // G, x.shape[1]
    out = []
    for s in range(b):
        nxt = [(-np.inf, pad, k) for k in range(nb)]
        hyps = [[(float(hyp_score[s, g * gs + j]),) for j in range(n_hyp[s, g])] for g in range(G)]
        new_done = list(done[s])
        for g in range(G):
            if done[s, g]:
                continue
            taken = [t for sc, t, _ in nxt[:g * gs] if sc > -np.inf]
            full = sorted((-(float(score[s, k]) + logp[s * nb + k, v] - float(np.float32(lam)) * taken.count(v)), k, v)
                          for k in range(g * gs, (g + 1) * gs) for v in range(Vv))[:2 * gs]
            k = g * gs
            for rank, (neg, beam, tok) in enumerate(full):
                if eos is not None and tok == eos:
                    if rank < gs:
                        hyps[g] = sorted(hyps[g] + [(-neg / norm, s * nb + beam)], key=lambda t: -t[0])[:gs]
                    continue
                if k < (g + 1) * gs:
                    nxt[k] = (-neg, tok, beam)
                    k += 1
            if len(hyps[g]) >= gs and (early or hyps[g][-1][0] >= max(t[0] for t in nxt[g * gs:(g + 1) * gs]) / norm):
                new_done[g] = 1
        out.append((nxt, hyps, new_done))
    return out


@pytest.mark.parametrize("Vv,nb,G,lam", [(5, 2, 2, 0.75), (6, 4, 2, 0.5), (7, 4, 4, 1.25), (8, 3, 3, 2.0), (9, 4, 2, 0.0), (9, 4, 1, 0.0), (8, 4, 4, 8.0)])
def test_one_step_against_a_brute_force_over_the_full_penalised_matrix(Vv, nb, G, lam):
    gs, b, eos, pad = nb // G, 3, 1, 0
    g = np.random.default_rng(100 * Vv + 10 * nb + G)
    for trial in range(40):
        st = GC.new_state(b, nb, G, 6, 1.0, pad)
        st["score"][:] = -(g.random((b, nb)) * 3).astype(np.float32)
        st["score"][g.random((b, nb)) < 0.25] = -np.inf                               # dead beams
        st["done"][:] = g.random((b, G)) < 0.2
        st["n_hyp"][:] = g.integers(0, gs + 1, (b, G))
        st["n_hyp"][st["done"] == 1] = gs
        hs = -np.sort(g.random((b, G, gs)) * 2, axis=-1).astype(np.float32)          # sorted, best first
        hs[np.arange(gs)[None, None] >= st["n_hyp"][..., None]] = -np.inf
        st["hyp_score"][:] = hs.reshape(b, nb)
        logits = (g.standard_normal((b * nb, Vv)) * 2).astype(np.float32)
        early = bool(trial % 2)
        before = copy.deepcopy(st)
        tops = GC.step(st, logits, 3, nb, G, lam, eos, pad, early, ft=np.float64)
        live = before["done"] == 0
        if BC.min_margin(tops.reshape(b * G, -1)).reshape(b, G)[live].min(initial=np.inf) < 1e-6:
            continue
        norm = float(before["len_norm"][3])
        for s, (nxt, hyps, new_done) in enumerate(_brute_force(before["score"], logits, nb, G, lam, eos, pad, before["done"], before["n_hyp"],
                                                              before["hyp_score"], norm, early)):
            assert [int(t) for t in st["next_tok"][s * nb:(s + 1) * nb]] == [t for _, t, _ in nxt]
            assert [int(r) for r in st["beam_idx"][s * nb:(s + 1) * nb]] == [s * nb + k for _, _, k in nxt]
            np.testing.assert_allclose(st["score"][s], [sc for sc, _, _ in nxt], rtol=0, atol=1e-5)
            assert [int(n) for n in st["n_hyp"][s]] == [len(h) for h in hyps]
            for gi in range(G):
                np.testing.assert_allclose(st["hyp_score"][s, gi * gs:gi * gs + len(hyps[gi])], [h[0] for h in hyps[gi]], rtol=0, atol=1e-5)
                new = [(p, h) for p, h in enumerate(hyps[gi]) if len(h) == 2]
                assert all(int(st["hyp_row"][s, gi * gs + p]) == h[1] and int(st["hyp_len"][s, gi * gs + p]) == 3 for p, h in new)
            # (the brute force judges "done" in float64; a hypothesis exactly level with the best open beam is not among these draws)
            assert [int(d) for d in st["done"][s]] == [int(d) for d in new_done]


# ---- the dynamic loop is the restatement --------------------------------------------------------------------------------------------------
NB, G, LAM = 4, 2, 0.5
CASES = [  # (early_stopping, length_penalty, eos, seed of the logits table: one whose run keeps every margin >= 1e-3)
    (True, 1.0, EOS, 2), (False, 1.0, EOS, 4), (True, 0.6, EOS, 6), (False, 0.6, EOS, 8), (True, 2.0, EOS, 10), (False, 2.0, EOS, 12),
    (True, 1.0, None, 17), (False, 2.0, None, 23),
]


def _run(early, lp, eos, seed, nb=NB, n_groups=G, lam=LAM, pad=PAD):
    script, ev = BC.Script(V, seed, eos=eos, eos_boost=BOOST), {}
    st, worst = GC.run_restatement(script, PROMPT, nb, n_groups, lam, MAXLEN, eos, pad, early, lp, events=ev)
    return script, st, worst, ev


@pytest.mark.parametrize("early,lp,eos,seed", CASES)
def test_restatement_and_finalize_equal_the_dynamic_group_beam_search(early, lp, eos, seed):
    from flamingo_mini_amd.decoding import Groups, _beam_finalize
    script, st, worst, _ = _run(early, lp, eos, seed)
    assert worst >= 1e-3, f"the script is not decidable: consecutive candidate scores {worst:.2e} apart"
    ids = torch.from_numpy(PROMPT)
    search = BC.ScriptedModel(script).search
    want = _beam_finalize(st, L0, PROMPT, NB, PAD, n_groups=G)
    got = search(ids, torch.zeros_like(ids), torch.ones_like(ids), None, None, MAXLEN, NB, eos, PAD, early, lp, groups=Groups(G, LAM))
    assert got.shape == want.shape and torch.equal(got, want), (got.tolist(), want.tolist())
    want_ids, want_s = _beam_finalize(st, L0, PROMPT, NB, PAD, n_return=NB, n_groups=G)
    got_ids, got_s = search(ids, torch.zeros_like(ids), torch.ones_like(ids), None, None, MAXLEN, NB, eos, PAD, early, lp, n_return=NB, groups=Groups(G, LAM))
    assert got_ids.shape == want_ids.shape and torch.equal(got_ids, want_ids), (got_ids.tolist(), want_ids.tolist())
    assert got_ids.shape[0] == 3 * NB and torch.equal(got_ids[::NB], want)              # rows s * n + j, the best first
    torch.testing.assert_close(got_s, want_s, rtol=1e-5, atol=1e-5)
    fin = torch.isfinite(got_s).reshape(3, NB)
    assert bool(((got_s.reshape(3, NB)[:, :-1] >= got_s.reshape(3, NB)[:, 1:]) | ~fin[:, 1:]).all())


# ... and two runs with more groups and pad = eos (what generate_captions passes): a done group's rows then hold the very token the others rank
EVENT_CASES = CASES + [(False, 1.0, EOS, 201, 6, 3, 0.25, EOS), (True, 1.0, EOS, 203, 8, 4, 0.25, EOS)]


def test_the_scripts_cover_the_events():
    """A group done while another group of its sequence still runs, eos at rank < gs and at rank >= gs, a count c >= 2 on a ranked
    candidate, and a dead beam's pad equal to a ranked candidate's token that is not counted - each at least once over the cases."""
    tot = {}
    for c in EVENT_CASES:
        for k, v in _run(*c)[3].items():
            tot[k] = tot.get(k, 0) + v
    print(tot)
    assert all(tot.get(k, 0) > 0 for k in ("mixed", "eos_low", "eos_high", "c2", "pad_uncounted", "done")), tot
