"""FlamingoModel.score_candidates / classify without a GPU: the float64 tiny models of tests/test_model_plumbing.py on the oracle backend,
both LM families.  Every score against brute force - one uncached forward per (sequence, candidate), log_softmax, gather, sum, plus the eos
term when eos is scored - under rtol 1e-5 / atol 1e-5, what test_score_sequences_and_freezing_on_the_host holds score_sequences to against
the same brute force; agreement with score_sequences per image; max_rows 1 / 3 / 1024; the number and the batch sizes of the LM forward
calls (every distinct prefix runs once); the ValueErrors; classify on a stub processor."""
import numpy as np
import pytest
import torch

L0, EOS = 6, 90
# caller order not sorted; lengths 1 - 4 with shared prefixes; (5,) is a prefix of three others and (7, 3) of none; (7, 3) appears twice
CANDS = [[7, 3], [5, 9, 11, 3], [5, 9, 2], [5], [7, 3], [12], [7, 4, 1, 8], [5, 9, 11, 6]]
TOL = dict(rtol=1e-5, atol=1e-5)


@pytest.fixture(scope="module", params=["gpt2", "opt"])
def tiny(request):
    import oracle_backend
    from test_model_plumbing import build
    oracle_backend.install()
    try:
        model, z = build(torch.float64, "cpu", request.param)
        model.eval()
        ids, ml = torch.from_numpy(z["ids"])[:, :L0].clone(), torch.from_numpy(z["ml"])[:, :L0].clone()
        px = torch.from_numpy(z["px"]).double()
        assert ids.shape[0] == 2 and not torch.equal(ids[0], ids[1]) and not torch.equal(px[0], px[1])      # different prompts and media per row
        brute = {eos: brute_force(model, ids, ml, px, CANDS, eos) for eos in (None, EOS)}                   # computed once, shared, not changed
        yield model, ids, ml, px, brute
    finally:
        oracle_backend.uninstall()


def brute_force(model, ids, ml, px, cands, eos):
    out = np.zeros((ids.shape[0], len(cands)))
    with torch.no_grad():
        for s in range(ids.shape[0]):
            for j, c in enumerate(cands):
                tgt = torch.tensor(list(c) + ([eos] if eos is not None else []))
                full = torch.cat([ids[s], tgt])[None]
                mls = torch.cat([ml[s], torch.zeros(len(tgt), dtype=ml.dtype)])[None]
                logits = model(input_ids=full, attention_mask=torch.ones_like(full), media_locations=mls, pixel_values=px[s:s + 1]).logits[0]
                logp = logits[ids.shape[1] - 1:-1].log_softmax(-1)
                out[s, j] = float(logp.gather(-1, tgt[:, None]).sum())
    return out


def score(model, ids, ml, px, cands=CANDS, **kw):
    return model.score_candidates(ids, ml, torch.ones_like(ids), pixel_values=px, candidate_ids=cands, **kw)


@pytest.mark.parametrize("eos", [None, EOS], ids=["no-eos", "eos"])
@pytest.mark.parametrize("max_rows", [1, 3, 1024])
def test_scores_equal_brute_force_for_every_max_rows(tiny, eos, max_rows):
    from flamingo_mini_amd import CandidateScores
    model, ids, ml, px, brute = tiny
    res = score(model, ids, ml, px, eos_token_id=eos, max_rows=max_rows)
    assert isinstance(res, CandidateScores) and res.logprobs.shape == (2, len(CANDS)) and res.logprobs.dtype == torch.float64
    assert res.token_counts.dtype == torch.long and res.token_counts.tolist() == [len(c) + (eos is not None) for c in CANDS]
    worst = float(np.abs(res.logprobs.numpy() - brute[eos]).max())
    print(f"MEASURED max_rows {max_rows}, eos {eos}: worst |score - brute force| {worst:.3g}")
    assert np.allclose(res.logprobs.numpy(), brute[eos], **TOL), (res.logprobs, brute[eos])
    assert torch.equal(res.logprobs[:, 0], res.logprobs[:, 4])                                 # the duplicate candidate: equal columns
    assert len(model._decode_sessions) == 0


def test_attention_mask_defaults_to_ones_and_features_may_be_given(tiny):
    model, ids, ml, px, brute = tiny
    with torch.no_grad():
        vf = model.flamingo.encode_resample_visuals(px)
    res = model.score_candidates(ids, ml, visual_features=vf, candidate_ids=CANDS)
    assert np.allclose(res.logprobs.numpy(), brute[None], **TOL)


def test_agrees_with_score_sequences_per_image(tiny):
    """equal-length candidates whose first tokens differ: score_sequences' shared prefix is the prompt, and its (float32) sums are these"""
    model, ids, ml, px, _ = tiny
    cands = [[5, 9, 11], [7, 4, 1], [12, 3, 3], [30, 9, 11]]
    got = score(model, ids, ml, px, cands).logprobs
    for s in range(2):
        rows = torch.cat([ids[s][None].repeat(4, 1), torch.tensor(cands)], dim=1)
        mls = torch.cat([ml[s][None].repeat(4, 1), torch.zeros((4, 3), dtype=ml.dtype)], dim=1)
        ref = model.score_sequences(rows, mls, torch.ones_like(rows), pixel_values=px[s])
        assert np.allclose(got[s].numpy(), ref.double().numpy(), **TOL), (s, got[s], ref)


def level_batches(cands, eos_on, b):
    """restated from the definition: the rows of the step at depth d are the distinct prefixes of length d that some longer candidate
    extends, or - with eos scored - that are a candidate themselves"""
    cands = {tuple(c) for c in cands}
    out = []
    for d in range(1, max(map(len, cands)) + 1):
        need = {c[:d] for c in cands if len(c) > d} | ({c for c in cands if len(c) == d} if eos_on else set())
        if need:
            out.append(b * len(need))
    return out


@pytest.mark.parametrize("eos", [None, EOS], ids=["no-eos", "eos"])
def test_every_distinct_prefix_runs_once(tiny, eos):
    """the calls of the model's forward: one group = the prompt step on b rows and `steps` more, steps = longest - 1 (longest with eos), each
    on b x (distinct prefixes of that length that need logits) rows; with max_rows = 1 every first token's subtree is a group of its own"""
    model, ids, ml, px, _ = tiny
    calls, orig = [], model.flamingo.forward

    def counting(*a, **kw):
        calls.append(tuple(kw["input_ids"].shape))
        return orig(*a, **kw)

    model.flamingo.forward = counting
    try:
        with torch.no_grad():
            vf = model.flamingo.encode_resample_visuals(px)
        run = lambda max_rows: (calls.clear(), model.score_candidates(ids, ml, visual_features=vf, candidate_ids=CANDS, eos_token_id=eos, max_rows=max_rows), list(calls))[2]
        steps = 4 - 1 + (eos is not None)
        one = run(1024)
        assert len(one) == 1 + steps and one == [(2, L0)] + [(n, 1) for n in level_batches(CANDS, eos is not None, 2)], one
        alone = run(1)                                                  # groups {5 ...}, {7 ...}, {12}: each from its own prompt step
        by_first = [[c for c in CANDS if c[0] == f] for f in (5, 7, 12)]
        assert alone == [call for g in by_first for call in [(2, L0)] + [(n, 1) for n in level_batches(g, eos is not None, 2)]], alone
        assert len(alone) == sum(1 + max(map(len, g)) - 1 + (eos is not None) for g in by_first)
        # max_rows = 3, b = 2: a level may hold one node.  Without eos the subtrees of 5 and of 7 have one node needing logits per level
        # and cannot share a group, the leaf 12 adds nothing to the group of 7; with eos 12 needs a row of its own at depth 1.
        three = run(3)
        assert len(three) == (8 if eos is None else 12), three
    finally:
        del model.flamingo.forward


def test_value_errors(tiny):
    model, ids, ml, px, _ = tiny
    V = model.flamingo.lm.config.vocab_size
    for bad in ([], [[]], [[5], []], [[V]], [[-1]], [[5, True]], "ab", [5, 9], [[5, 9.0]]):
        with pytest.raises(ValueError):
            score(model, ids, ml, px, bad)
    with pytest.raises(ValueError, match="eos"):
        score(model, ids, ml, px, [[5, EOS], [7]], eos_token_id=EOS)
    assert score(model, ids, ml, px, [[5, EOS], [7]]).logprobs.shape == (2, 2)                # without eos scored, 90 is a token like any
    for bad in (0, -1, 2.0, True, None, "8"):
        with pytest.raises(ValueError, match="max_rows"):
            score(model, ids, ml, px, max_rows=bad)
    with pytest.raises(ValueError, match="eos_token_id"):
        score(model, ids, ml, px, eos_token_id=V)


class StubProcessor:
    """what classify reads of a FlamingoProcessor: a verbatim tokenizer (one token per letter) and encode_text"""

    def __init__(self, ids, ml):
        self.ids, self.ml, self.seen = ids, ml, []

    def tokenizer(self, s, add_special_tokens=True):
        assert add_special_tokens is False
        self.seen.append(s)
        return {"input_ids": [3 + ord(ch) - ord("a") if ch != " " else 40 for ch in s]}

    def encode_text(self, prompt, device):
        return self.ids[:1], self.ml[:1], torch.ones_like(self.ids[:1])


def test_classify_on_a_stub_processor(tiny):
    model, ids, ml, px, _ = tiny
    proc = StubProcessor(ids, ml)
    names = [" cat", " car", " dog", " c"]
    cfg = model.flamingo.lm.config
    saved, cfg.eos_token_id = cfg.eos_token_id, EOS
    try:
        labels, probs = model.classify(proc, pixel_values=px, prompt="<image>", candidates=names)
        assert proc.seen == names and probs.shape == (2, 4) and torch.allclose(probs.sum(-1), torch.ones(2, dtype=probs.dtype))
        rep = ids[:1].expand(2, -1).contiguous()
        ref = model.score_candidates(rep, ml[:1].expand(2, -1).contiguous(), pixel_values=px, candidate_ids=[proc.tokenizer(s, add_special_tokens=False)["input_ids"] for s in names])
        assert torch.allclose(probs, ref.logprobs.softmax(-1)) and labels == [names[i] for i in ref.logprobs.argmax(-1).tolist()]
        labels_t, probs_t = model.classify(proc, pixel_values=px, candidates=names, normalize="tokens", score_eos=True)
        ref_e = model.score_candidates(rep, ml[:1].expand(2, -1).contiguous(), pixel_values=px, eos_token_id=EOS,
                                       candidate_ids=[proc.tokenizer(s, add_special_tokens=False)["input_ids"] for s in names])
        assert ref_e.token_counts.tolist() == [5, 5, 5, 3]
        want = (ref_e.logprobs / ref_e.token_counts.double()).softmax(-1)
        assert torch.allclose(probs_t, want) and torch.allclose(probs_t.sum(-1), torch.ones(2, dtype=probs_t.dtype))
        assert labels_t == [names[i] for i in want.argmax(-1).tolist()] and not torch.allclose(probs_t, probs)
        with pytest.raises(ValueError, match="normalize"):
            model.classify(proc, pixel_values=px, candidates=names, normalize="chars")
        with pytest.raises(ValueError, match="list of strings"):
            model.classify(proc, pixel_values=px, candidates=" cat")
    finally:
        cfg.eos_token_id = saved
