"""The numpy restatement of ff_logits_constrain's rules (tests/constraint_cases.py) without a GPU: against hand-written expectations for every
clause of T1, T2 and B1, against transformers' PrefixConstrainedLogitsProcessor and NoBadWordsLogitsProcessor, against the torch restatement
the dynamic loops use (decoding.constrain_logits_torch on decoding.TokenTrie / BadWords tables), and generate(candidate_ids=, bad_words_ids=)
end to end on the tiny CPU models of tests/test_model_plumbing.py.  Everything is an equality: the rules only write -inf."""
import numpy as np
import pytest
import torch

import constraint_cases as CC

NINF, NAN = -np.inf, np.nan
V, EOS = 12, 9
CANDS = [[3, 4], [3, 4, 5], [6], [3, 7]]                                     # (3, 4) is a prefix of (3, 4, 5); 6 and (3, 7) end in leaves
PROMPT = [3, 4, 9]                                                           # the prompt spells a candidate and eos: it must not count (n0 = 3)


def run(hists, gen_start=3, trie=True, words=None, x=None, n=None, eos=EOS):
    hist = np.array(hists, np.int64).reshape(len(hists), -1)
    x = np.tile(np.arange(V, dtype=np.float32), (len(hists), 1)) if x is None else np.array(x, np.float32)
    out = CC.restate(CC.bits_of(x, "f32"), V, hist, hist.shape[1] if n is None else n, gen_start, eos=eos, trie=CC.build_trie(CANDS) if trie else None,
                     words=CC.build_words(words) if words else None)
    return CC.values_of(out, "f32")


def kept(row):
    return sorted(int(v) for v in np.flatnonzero(row != NINF))


def test_t1_t2_by_hand():
    hists = [PROMPT, PROMPT + [3], PROMPT + [3, 4], PROMPT + [3, 4, 5], PROMPT + [6], PROMPT + [3, 7]]
    want = [[3, 6], [4, 7], [5, EOS], [EOS], [EOS], [EOS]]                    # root; inner; the prefix pair: eos or go on; leaves allow only eos
    for h, w in zip(hists, want):
        row = run([h])[0]
        assert kept(row) == w, (h, kept(row))
        assert all(row[v] == v for v in w)                                   # kept entries keep their value
    both = run([PROMPT + [3, 0], PROMPT + [6, 0]], n=4)                       # rows walk on their own
    assert kept(both[0]) == [4, 7] and kept(both[1]) == [EOS]


def test_done_and_dead_rows_are_untouched():
    for h in (PROMPT + [3, 4, 9], PROMPT + [6, 9, 0], PROMPT + [3, 4, 9, 3],      # DONE, and DONE stays
              PROMPT + [5], PROMPT + [3, 9], PROMPT + [3, 5, 4], PROMPT + [6, 6], PROMPT + [9]):    # DEAD: no child; eos at a non-terminal node, at the root
        assert kept(run([h])[0]) == list(range(V)), h


def test_gen_start_and_lengths():
    assert kept(run([PROMPT], gen_start=3)[0]) == [3, 6]                      # n == n0: the root
    assert kept(run([PROMPT], gen_start=7)[0]) == [3, 6]                      # n0 clamped to n
    assert kept(run([PROMPT], gen_start=0)[0]) == list(range(V))              # n0 == 0: the prompt is walked - (3, 4) then eos: DONE
    assert kept(run([[3, 4, 5]], gen_start=0)[0]) == [EOS]
    assert kept(run([[3, 4, 5]], gen_start=-2)[0]) == [EOS]                   # clamped to 0
    assert kept(run([PROMPT + [3, 0, 0]], n=4)[0]) == [4, 7]                  # positions >= n are not read
    assert kept(run([PROMPT + [3, 0, 0]], n=-1)[0]) == [3, 6]                 # n clamped to 0
    assert kept(run([PROMPT + [3]], n=99)[0]) == [4, 7]                       # n clamped to the cap


def test_banned_nan_becomes_ninf_and_kept_entries_keep_their_bits():
    x = np.arange(V, dtype=np.float32)[None].copy()
    x[0, 2], x[0, 3], x[0, 6] = NAN, NAN, -0.0
    bits = CC.bits_of(x, "f32")
    bits[0, 3] = 0x7FC12345                                                  # a NaN payload at a kept entry
    out = CC.restate(bits, V, np.array([PROMPT], np.int64), 3, 3, eos=EOS, trie=CC.build_trie(CANDS))
    assert out[0, 2] == 0xFF800000 and out[0, 3] == 0x7FC12345 and out[0, 6] == 0x80000000
    assert (np.delete(out[0], [3, 6]) == 0xFF800000).all()


def test_b1_by_hand():
    words = [[2], [4, 9, 1], [9, 5], [3, 4, 9, 6], [0, 0, 0, 0, 7], [8, 8]]
    row = run([PROMPT], trie=False, words=words)[0]
    # [2] always; [4, 9, 1] matches across ... the whole history (3, 4, 9): bans 1; [9, 5] bans 5; [3, 4, 9, 6] bans 6 (n == m - 1); the
    # five-token word is longer than the history allows; (8, 8): the tail is 9, not 8
    assert sorted(int(v) for v in np.flatnonzero(row == NINF)) == [1, 2, 5, 6]
    # a match spanning the prompt / generation boundary: prompt (3, 4, 9), generated (6): the word (9, 6, 0) bans 0
    row = run([PROMPT + [6]], trie=False, words=[[9, 6, 0], [4, 9, 6, 1], [4, 6, 2]])[0]
    assert sorted(int(v) for v in np.flatnonzero(row == NINF)) == [0, 1]
    # out-of-range ids: a last token outside [0, V) names no logit, an earlier one still takes part in the comparison
    hist = [[3, 1 << 40, -1]]
    row = run(hist, trie=False, words=[[1 << 20], [-1], [V], [-1, 4], [5, V]], gen_start=0)[0]
    assert sorted(int(v) for v in np.flatnonzero(row == NINF)) == [4]
    assert not (run([[3, (1 << 32) + 4]], trie=False, words=[[4, 5]], gen_start=0)[0] == NINF).any()       # int64 history ids are not truncated
    assert (run([PROMPT], trie=False, words=[[2]], n=0)[0] == NINF).sum() == 1                                # an empty history: single tokens only


def test_bans_union_and_absent_tables():
    row = run([PROMPT + [3]], words=[[7], [3, 4]])[0]                         # T2 keeps {4, 7}; B1 bans both
    assert kept(row) == []
    x = np.arange(V, dtype=np.float32)[None]
    assert np.array_equal(run([PROMPT], trie=False), x)
    empty = dict(CC.build_trie(CANDS), n_nodes=0)
    assert np.array_equal(CC.restate(CC.bits_of(x, "f32"), V, np.array([PROMPT], np.int64), 3, 3, eos=EOS, trie=empty), CC.bits_of(x, "f32"))


def test_garbage_behind_the_live_entries_is_not_read():
    trie, words = CC.build_trie(CANDS), CC.build_words([[2], [9, 5]])
    hists = np.array([PROMPT + [3, 4], PROMPT + [6, 9], PROMPT + [3, 5]], np.int64)
    x = CC.make_logits(3, V, "bf16", 1)
    a = CC.restate(x, V, hists, 5, 3, eos=EOS, trie=trie, words=words, dtype="bf16")
    b = CC.restate(x, V, hists, 5, 3, eos=EOS, trie=CC.pad_tables(trie, 1), words=CC.pad_tables(words, 2), dtype="bf16")
    assert np.array_equal(a, b) and not np.array_equal(a, x)


# ---- against transformers -------------------------------------------------------------------------------------------------------------
def test_against_transformers_prefix_constrained_processor():
    """prefix_allowed_tokens_fn written from a plain dict of the candidates; for a DONE or DEAD row it returns the whole vocabulary (this
    project leaves such rows untouched, transformers raises on an empty list).  float32, compared as values: transformers adds 0.0 to kept
    entries, which only turns -0.0 into +0.0."""
    from transformers.generation.logits_process import PrefixConstrainedLogitsProcessor
    Vt, eos, L0 = 33, CC.EOS, 3
    cands = [[32], [32, 2], [2, 5, 7], [2, 5], [7], [0, 1], [0, 31]]
    ends, inner = {tuple(c) for c in cands}, {tuple(c[:k]) for c in cands for k in range(len(c))}

    def fn(batch_id, sent):
        g = tuple(sent.tolist()[L0:])
        if g not in ends and g not in inner:
            return list(range(Vt))                                            # DONE or DEAD
        return sorted({c[len(g)] for c in cands if len(c) > len(g) and tuple(c[:len(g)]) == g} | ({eos} if g in ends else set()))

    rng = np.random.default_rng(0)
    gens = [[], [2], [2, 5], [2, 5, 7], [32], [0], [7, eos], [2, 5, eos, 4], [3], [2, eos], [0, 31]]
    for g in gens:
        hist = np.array([[4, 5, 6] + g, [9, 9, 9] + g], np.int64)
        x = rng.standard_normal((2, Vt)).astype(np.float32)
        x[:, 3], x[:, 5] = -0.0, -0.0                                        # (a banned NaN stays NaN in transformers, NaN + -inf; here it becomes -inf: by hand above)
        want = PrefixConstrainedLogitsProcessor(fn, 1)(torch.from_numpy(hist), torch.from_numpy(x.copy())).numpy()
        got = CC.restate_values(x, "f32", hist, L0, eos=eos, trie=CC.build_trie(cands))
        assert np.array_equal(got, want, equal_nan=True), g


def test_against_transformers_no_bad_words_processor():
    """in-vocabulary ids, as the processor needs.  One deliberate difference is kept out of the comparison: a word whose head is the WHOLE
    history (m == n + 1) is banned here (rule B1: n >= m - 1, checked by hand above), where transformers skips every word longer than the
    history; the words here have m <= n or do not match."""
    from transformers.generation.logits_process import NoBadWordsLogitsProcessor
    Vt = 33
    rng = np.random.default_rng(1)
    hist = rng.integers(0, Vt, (4, 9)).astype(np.int64)
    words = [[0], [32], [int(hist[0, -1]), 11], [int(t) for t in hist[1, -3:]] + [13], [int(t) for t in hist[2, 1:]] + [14], [5] * 10 + [15],
             [int(hist[3, -1]) ^ 1, 16], [int(hist[3, -2]), int(hist[3, -1]), 17]]
    for n in (9, 3, 1):
        x = rng.standard_normal((4, Vt)).astype(np.float32)
        want = NoBadWordsLogitsProcessor(words, eos_token_id=None)(torch.from_numpy(hist[:, :n].copy()), torch.from_numpy(x.copy())).numpy()
        got = CC.restate_values(x, "f32", hist[:, :n], 2, words=CC.build_words(words))
        assert np.array_equal(got, want), n
        if n == 9:
            assert sorted(np.flatnonzero(got[3] == NINF).tolist()) == [0, 17, 32] and got[0, 11] == NINF and got[1, 13] == NINF and got[2, 14] == NINF


# ---- against the torch restatement of the dynamic loops and the host-built tables ------------------------------------------------------
@pytest.mark.parametrize("Vt", [33, 320])
def test_torch_restatement_and_host_tables_equal_the_numpy_restatement(Vt):
    from flamingo_mini_amd import decoding as D
    eos = CC.EOS
    trie, _ = CC.trie_for(Vt, eos)
    cands = [[0, v] for v in range(Vt) if v != eos] + [[Vt - 1], [Vt - 1, 2], [2, 5, 7], [2, 5], [7], [5, 2, 2, 5, 7], [9] * CC.LONG + [7], [2, 5], [7]]
    host = D.TokenTrie(cands, Vt, eos)                                        # shuffled, with duplicates: the builder sorts and dedups
    assert host.n_nodes == trie["n_nodes"] and len(host.edge_tok) == len(trie["edge_tok"]) and host.longest == CC.LONG + 1
    mine = dict(node_first=host.node_first, edge_tok=host.edge_tok, edge_child=host.edge_child, node_terminal=host.node_terminal, n_nodes=host.n_nodes)
    rng = np.random.default_rng(Vt)
    moved = 0
    for cap, n, n0, rot in CC.LENGTHS:
        nn, nn0 = CC.clamped(cap, n, n0)
        hist = CC.histories(Vt, eos, 5, cap, nn, nn0, rng, rot)
        in_vocab = [w for w in _words(CC.words_for(Vt, hist, nn)) if all(0 <= t < Vt for t in w)]
        bits = CC.make_logits(5, Vt, "f32", cap + n)
        want = CC.restate(bits, Vt, hist, n, n0, eos=eos, trie=trie, words=CC.build_words(in_vocab))
        assert np.array_equal(CC.restate(bits, Vt, hist, n, n0, eos=eos, trie=mine, words=CC.build_words(in_vocab)), want)      # numbering does not matter
        bw = D.BadWords(in_vocab + in_vocab[:1], Vt)
        got = D.constrain_logits_torch(torch.from_numpy(CC.values_of(bits, "f32")), torch.from_numpy(hist[:, :nn]), n0, eos, host, bw).numpy()
        assert np.array_equal(CC.bits_of(got, "f32"), want), (cap, n, n0)
        moved += not np.array_equal(want, bits)
    assert moved == len(CC.LENGTHS)                                           # (the words alone move every case)


def _words(t):
    return [[int(v) for v in t["bw_tok"][int(t["bw_off"][w]):int(t["bw_off"][w + 1])]] for w in range(int(t["n_bw"]))]


def test_table_builders_reject_bad_input():
    from flamingo_mini_amd import decoding as D
    for bad in ([], [[]], [[1], []], [[-1]], [[40]], [[1, 39]], [[True]], [[1.0]], "ab", [3], 5):
        with pytest.raises(ValueError):
            D.TokenTrie(bad, 40, 39)
    for bad in ([], [[]], [[-1]], [[40]], [3]):
        with pytest.raises(ValueError):
            D.BadWords(bad, 40)
    assert D.BadWords([[7], [1, 2], [7]], 40).words == [(1, 2), (7,)]         # (eos may be banned); sorted, deduplicated
    c = D.Constraints(D.TokenTrie([[1], [1, 2]], 40, 39), None)
    assert c.caps() == ("constraints", 64, 64, 0, 0)
    assert D.Constraints(D.TokenTrie([[i, j] for i in range(1, 7) for j in range(20)], 40, 39), D.BadWords([[1]], 40)).caps() == ("constraints", 128, 128, 16, 64)


# ---- generate() on the tiny CPU models ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module", params=["gpt2", "opt"])
def tiny(request):
    import oracle_backend
    from test_model_plumbing import build
    oracle_backend.install()
    try:
        model, z = build(torch.float64, "cpu", request.param)
        model.eval()
        px = torch.from_numpy(z["px"]).double()
        ids, ml = torch.from_numpy(z["ids"])[:, :4], torch.from_numpy(z["ml"])[:, :4]
        yield model, ids, dict(media_locations=ml, attention_mask=torch.ones_like(ids), pixel_values=px, max_length=12)
    finally:
        oracle_backend.uninstall()


G_EOS, G_PAD = 3, 0
G_CANDS = [[5, 6, 7], [5, 6], [9], [11, 12, 13, 14], [20, 21]]


def rows_are_candidates(out, ids, cands=G_CANDS):
    assert torch.equal(out[:, :ids.shape[1]], ids[:1].expand(out.shape[0], -1)) or torch.equal(out[:, :ids.shape[1]], ids.repeat_interleave(out.shape[0] // ids.shape[0], 0))
    found = []
    for row in out[:, ids.shape[1]:].tolist():
        assert G_EOS in row, row
        k = row.index(G_EOS)
        assert row[:k] in cands and all(t == G_PAD for t in row[k + 1:]), row
        found.append(row[:k])
    return found


@pytest.mark.parametrize("mode", [dict(), dict(do_sample=True), dict(num_beams=3)], ids=["greedy", "sampling", "beams"])
def test_generate_returns_only_candidates(tiny, mode):
    """(fails on the commit before the feature with TypeError: unsupported generation arguments)"""
    model, ids, kw = tiny
    plain = model.generate(ids, eos_token_id=G_EOS, pad_token_id=G_PAD, **mode, **kw)
    out = model.generate(ids, candidate_ids=G_CANDS, eos_token_id=G_EOS, pad_token_id=G_PAD, **mode, **kw)
    rows_are_candidates(out, ids)
    assert out.shape[1] <= 4 + 5 and out.shape != plain.shape or not torch.equal(out, plain)
    assert len(model._decode_sessions) == 0                                  # CPU tensors: the dynamic loops


def test_generate_beams_return_distinct_candidates_best_first(tiny):
    model, ids, kw = tiny
    out = model.generate(ids, candidate_ids=G_CANDS, eos_token_id=G_EOS, pad_token_id=G_PAD, num_beams=3, num_return_sequences=3,
                         return_dict_in_generate=True, **kw)
    found = rows_are_candidates(out.sequences, ids)
    for s in range(ids.shape[0]):
        mine = found[3 * s:3 * s + 3]
        assert len({tuple(c) for c in mine}) == 3
        sc = out.sequences_scores[3 * s:3 * s + 3]
        assert bool((sc[:-1] >= sc[1:]).all()) and bool(torch.isfinite(sc).all())
    # two candidates, three beams: both come back; the third row's score is -inf (a row with that score is no result: all pad, or what a dead
    # beam held when torch.topk ranked its -inf eos candidate among the first three)
    out = model.generate(ids, candidate_ids=[[9], [5, 6]], eos_token_id=G_EOS, pad_token_id=G_PAD, num_beams=3, num_return_sequences=3,
                         return_dict_in_generate=True, **kw)
    for s in range(ids.shape[0]):
        rows, sc = out.sequences[3 * s:3 * s + 3, 4:].tolist(), out.sequences_scores[3 * s:3 * s + 3]
        assert sorted(r[:r.index(G_EOS)] for r in rows[:2]) == [[5, 6], [9]]
        assert bool(torch.isfinite(sc[:2]).all()) and float(sc[2]) == -np.inf


def test_generate_logprobs_are_renormalised_over_the_allowed_set(tiny):
    """greedy under a trie with output_logprobs: exp(sum of the token values) over ALL candidates' paths sums to 1 - here checked on the
    first step, whose allowed set is the root's children: the chosen token's probability is its softmax over those"""
    model, ids, kw = tiny
    out = model.generate(ids, candidate_ids=G_CANDS, eos_token_id=G_EOS, pad_token_id=G_PAD, return_dict_in_generate=True, output_logprobs=True, **kw)
    logits, _ = model._decode_step(ids, kw["media_locations"], kw["attention_mask"], None, kw["pixel_values"], None)
    roots = sorted({c[0] for c in G_CANDS})
    ref = logits[:, roots].double().log_softmax(-1)
    for r in range(ids.shape[0]):
        tok = int(out.sequences[r, 4])
        assert tok == roots[int(ref[r].argmax())]
        assert abs(float(out.token_logprobs[r, 0]) - float(ref[r].max())) < 1e-9
    assert bool((out.token_logprobs <= 0).all()) and bool(torch.isfinite(out.sequences_scores).all())


@pytest.mark.parametrize("mode", [dict(), dict(do_sample=True), dict(num_beams=3)], ids=["greedy", "sampling", "beams"])
def test_generate_never_emits_a_banned_word(tiny, mode):
    """the words are taken from the unconstrained run's own output (its first generated token, and its first bigram), so the ban changes the ids"""
    model, ids, kw = tiny
    plain = model.generate(ids, **mode, **kw)
    words = [[int(plain[0, 4])], [int(plain[1, 4]), int(plain[1, 5])], [int(ids[0, 3]), int(plain[0, 4])]]
    out = model.generate(ids, bad_words_ids=words, **mode, **kw)
    assert not torch.equal(out[:, :plain.shape[1]], plain[:, :out.shape[1]])
    for row in out.tolist():
        for w in words:
            assert not any(row[i:i + len(w)] == w for i in range(4 - len(w) + 1, len(row) - len(w) + 1)), (w, row)
    both = model.generate(ids, bad_words_ids=[[9]], candidate_ids=G_CANDS, eos_token_id=G_EOS, pad_token_id=G_PAD, **mode, **kw)
    assert [9] not in rows_are_candidates(both, ids)
