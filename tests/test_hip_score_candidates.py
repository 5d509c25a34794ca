"""FlamingoModel.score_candidates on the MI355X: the walk of the candidate trie over the cached decode path with ff_logprob_gather, on the G1
geometry of tests/test_hip_decode.py in bf16, b = 2.

A spy on functional.logprob_gather sees what the kernel is given - bf16 logits, the [:, -1] view of the step's output through its row
stride, never a float32 copy - and records each level's logits and tables.  Every returned score is then held to float64 computed from the
RECORDED logits (the pattern of test_hip_logprob.held_to_the_recorded_logits), the rows of a level identified by the documented order alone:
sequence-major, within a sequence the distinct prefixes of that depth that need logits, in lexicographic order.  The bound is the project's
own, CE_C_F 2^-24 (|lse*| + |x_tok| + 1) per scored token, summed along the path, plus 2^-24 of the largest partial sum for each fp32 add.
The candidates share prefixes, one is a prefix of others, one appears twice, the caller's order is not sorted; eos scored and not; max_rows 3
(several groups, each from its own prompt step) and 1024; the argmax column per row agrees with float64's, the float64 gap between the best
and the second candidate asserted to exceed twice the bound so that a tie cannot hide a failure."""
import contextlib

import pytest
import torch

from util import CE_C_F

pytestmark = pytest.mark.gpu
EOS = 310
CANDS = [[70, 30], [50, 90, 110, 30], [50, 90, 20], [50], [70, 30], [120], [70, 40, 10, 80], [50, 90, 110, 60]]


@pytest.fixture(scope="module")
def g1():
    import test_hip_decode as D
    model, _ = D.models("gpt2")
    inputs = D.make_inputs(2, 1, "candidates")
    yield D, model, inputs
    D._MODELS.clear()


@contextlib.contextmanager
def gathers_recorded(store):
    from flamingo_mini_amd import functional as F
    orig = F.logprob_gather

    def spy(logits, row_first, tok, base=None, out=None):
        res = orig(logits, row_first, tok, base, out)
        store.append(dict(dtype=logits.dtype, shape=tuple(logits.shape), stride=logits.stride(), x=logits.detach().float().cpu(), row_first=row_first.cpu(),
                          tok=tok.cpu(), base=None if base is None else base.cpu(), out=res.detach().cpu()))
        return res

    F.logprob_gather = spy
    try:
        yield store
    finally:
        F.logprob_gather = orig


def float64_from_the_records(records, cands, eos, b, L0, V):
    """({(sequence, candidate tuple): (score*, bound)}, number of groups).  A group begins with a call on b rows without base: the root.
    Its first tokens are the tokens the root is asked for; at depth d its rows are, per sequence, the sorted distinct prefixes of length d
    of the group's candidates that a longer candidate extends or - eos scored - that are a candidate themselves."""
    distinct = sorted({tuple(c) for c in cands})
    rows64, groups = {}, 0                                         # (sequence, prefix) -> (x row, float64 lse)
    i = 0
    while i < len(records):
        rec = records[i]
        assert rec["base"] is None and rec["shape"] == (b, V) and rec["stride"] == (L0 * V, 1), (rec["shape"], rec["stride"])
        per_seq = rec["tok"].numel() // b
        firsts = rec["tok"][:per_seq].tolist()
        assert firsts == sorted(set(firsts)) and rec["tok"].tolist() == firsts * b
        mine = [c for c in distinct if c[0] in firsts]
        groups += 1
        d = 0
        while True:
            need = [()] if d == 0 else sorted({c[:d] for c in mine if len(c) > d} | ({c for c in mine if len(c) == d} if eos is not None else set()))
            if not need:
                break
            rec = records[i]
            assert rec["dtype"] == torch.bfloat16 and rec["shape"] == (b * len(need), V), (d, rec["shape"], len(need))
            assert rec["stride"] == ((L0 if d == 0 else 1) * V, 1) and (rec["base"] is None) == (d == 0)
            x64 = rec["x"].double()
            lse = torch.logsumexp(x64, dim=-1)
            first = rec["row_first"].tolist()
            for s in range(b):
                for k, p in enumerate(need):
                    r = s * len(need) + k
                    rows64[(s, p)] = (x64[r], float(lse[r]))
                    asked = rec["tok"][first[r]:first[r + 1]].tolist()       # the row's queries: its edge tokens, ascending, then eos at a candidate's end
                    want = sorted({c[d] for c in mine if len(c) > d and c[:d] == p}) + ([eos] if eos is not None and p in mine else [])
                    assert asked == want, (s, p, asked, want)
            i, d = i + 1, d + 1
    out = {}
    for s in range(b):
        for c in distinct:
            toks = list(c) + ([eos] if eos is not None else [])
            total, bound, largest = 0.0, 0.0, 0.0
            for t, tok in enumerate(toks):
                x, lse = rows64[(s, c[:t])]
                xt = float(x[tok])
                total += xt - lse
                bound += CE_C_F * 2.0 ** -24 * (abs(lse) + abs(xt) + 1.0)
                largest = max(largest, abs(total))
            out[(s, c)] = (total, bound + (len(toks) - 1) * 2.0 ** -24 * largest)
    return out, groups


@pytest.mark.parametrize("eos", [None, EOS], ids=["no-eos", "eos"])
@pytest.mark.parametrize("max_rows", [1024, 3])
def test_scores_are_held_to_float64_from_the_recorded_logits(g1, eos, max_rows):
    from flamingo_mini_amd import CandidateScores
    D, model, (ids, ml, am, vf) = g1
    V = model.flamingo.lm.config.vocab_size
    records = []
    with gathers_recorded(records):
        res = model.score_candidates(ids, ml, am, visual_features=vf, candidate_ids=CANDS, eos_token_id=eos, max_rows=max_rows)
    torch.cuda.synchronize()
    assert isinstance(res, CandidateScores) and res.logprobs.shape == (2, len(CANDS)) and res.logprobs.dtype == torch.float32 and res.logprobs.is_cuda
    assert res.token_counts.tolist() == [len(c) + (eos is not None) for c in CANDS] and len(model._decode_sessions) == 0
    ref, groups = float64_from_the_records(records, CANDS, eos, 2, D.L0, V)
    # max_rows = 3 with b = 2: one node per level - the subtrees of 50 and 70 never share a group; 120 joins 70's only while it needs no row
    assert groups == (1 if max_rows == 1024 else 2 if eos is None else 3), groups
    got = res.logprobs.cpu()
    worst = 0.0
    for s in range(2):
        for j, c in enumerate(CANDS):
            want, bound = ref[(s, tuple(c))]
            ratio = abs(float(got[s, j]) - want) / bound
            worst = max(worst, ratio if ratio == ratio else float("inf"))
    print(f"MEASURED max_rows {max_rows}, eos {eos}: worst score at {worst:.3f} of its bound, {groups} group(s), {len(records)} gather launches")
    assert worst <= 1.0, f"a score at {worst:.4g} of its bound"
    assert torch.equal(got[:, 0].view(torch.int32), got[:, 4].view(torch.int32))             # the duplicate candidate: equal columns
    for s in range(2):                                                                       # the argmax, with the gap that makes it decidable
        ranked = sorted({tuple(c) for c in CANDS}, key=lambda c: -ref[(s, c)][0])
        gap = ref[(s, ranked[0])][0] - ref[(s, ranked[1])][0]
        assert gap > 2 * max(ref[(s, ranked[0])][1], ref[(s, ranked[1])][1]), (s, gap)
        assert tuple(CANDS[int(got[s].argmax())]) == ranked[0], (s, got[s].tolist(), ranked[0])


def test_prefix_sharing_keeps_the_level_batches_small(g1):
    """64 candidates of 3 tokens under 4 first tokens and 16 second-level prefixes: three gather launches, on 2, 2 x 4 and 2 x 16 rows of
    bf16 logits - every distinct prefix is one row, and 2 x 64 scores come back finite"""
    D, model, (ids, ml, am, vf) = g1
    cands = [[10 + a, 20 + b_, 100 + c] for a in range(4) for b_ in range(4) for c in range(4)]
    records = []
    with gathers_recorded(records):
        res = model.score_candidates(ids, ml, am, visual_features=vf, candidate_ids=cands)
    assert [r["shape"][0] for r in records] == [2, 2 * 4, 2 * 16] and all(r["dtype"] == torch.bfloat16 for r in records)
    assert [r["tok"].numel() for r in records] == [2 * 4, 2 * 16, 2 * 64]
    assert bool(torch.isfinite(res.logprobs).all()) and res.logprobs.shape == (2, 64)
