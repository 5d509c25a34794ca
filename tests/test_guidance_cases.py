"""Classifier-free guidance without a GPU.

The rules: the float32 restatement of guided_logits_kernel (tests/guidance_cases.py) and decoding.guided_logits_torch stay inside the bound
the kernel is held to, on every designed row pair in both dtypes, and give exactly -inf / NaN where G3 says so; the designed layouts run
the cond rows, the uncond rows and the out rows through every 16-byte start phase.

The decoding (the tiny float64 model on the oracle backend, non-zero gates): the guided dynamic loops equal, token for token, a hand-written
loop of two UNCACHED forwards per step - with the media and with media_locations zeroed - combined in float64, for greedy decoding and for
beam search; guidance_scale=0 is the ordinary decode of the same ids without media; with every gate closed every scale is the unguided
decode; bad_words_ids sees the guided scores.  Every greedy decision's float64 top-two gap is asserted to be at least 1e-3 - three orders
above the float32 rounding of the scores the loops select from (_decode_step hands them float32 logits)."""
import numpy as np
import pytest
import torch

import guidance_cases as GC
import logprob_cases as LP
import loss_cases as lc
from util import CE_C_F

BF16, F32 = GC.BF16, GC.F32
DTYPES = pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])


# ---- the rules --------------------------------------------------------------------------------------------------------------------------
@DTYPES
def test_restatement_and_torch_form_stay_inside_the_bound(dtype):
    from flamingo_mini_amd import decoding
    worst, n = [0.0, 0.0], 0
    for case in GC.cases(dtype):
        c, u, V = case["cond"], case["uncond"], case["cond"].shape[1]
        for g in case["scales"]:
            got = GC.guided_f32(c, u, g, case["ld_c"], LP.start_off(V, case["ld_c"], case["off_c"]), case["ld_u"], LP.start_off(V, case["ld_u"], case["off_u"]))
            ok, w = GC.within_bound(got, c, u, g, CE_C_F)
            assert ok, f"{case['name']} g={g}: the restatement at {w:.4g} of the bound"
            ok_t, w_t = GC.within_bound(decoding.guided_logits_torch(c, u, g), c, u, g, CE_C_F)
            assert ok_t, f"{case['name']} g={g}: guided_logits_torch at {w_t:.4g} of the bound"
            worst = [max(worst[0], w), max(worst[1], w_t)]
            n += 1
    print(f"{n} (case, scale) pairs: the restatement at most {worst[0]:.3f}, the torch form {worst[1]:.3f} of the bound")
    assert n >= 200


@DTYPES
def test_designed_layouts_cover_every_start_phase_and_every_scale(dtype):
    es, phases, scales = 16 // lc.NVEC[dtype], {"c": set(), "u": set(), "o": set()}, set()
    pairs = set()
    for case in GC.cases(dtype):
        rows, V = case["cond"].shape
        scales |= set(case["scales"])
        kind = lambda ld: "odd" if ld == LP.odd_ld(V) else ld // V
        pairs.add((kind(case["ld_c"]), kind(case["ld_u"])))
        if V >= 9:
            phases["c"] |= {s // es for s in LP.row_starts(rows, case["ld_c"], dtype, LP.start_off(V, case["ld_c"], case["off_c"]))}
            phases["u"] |= {s // es for s in LP.row_starts(rows, case["ld_u"], dtype, LP.start_off(V, case["ld_u"], case["off_u"]))}
            phases["o"] |= {s // 4 for s in LP.row_starts(rows, case["ld_o"], F32, case["off_o"])}
    assert phases["c"] == phases["u"] == set(range(lc.NVEC[dtype])) and phases["o"] == set(range(4)), phases
    assert scales == set(GC.SCALES) and pairs == {(a, b) for a in (1, 2, "odd") for b in (1, 2, "odd")}, (scales, pairs)
    assert {c["cond"].shape[1] for c in GC.cases(dtype)} == set(GC.VOCABS)


def test_edge_rules_of_the_torch_form():
    """-inf in either input is -inf for every scale (0 included: no NaN from 0 * inf, no +inf from (1 - g) * -inf); NaN or +inf in a row of
    either input gives a NaN row; float64 inputs are combined in float64, a tensor scale is read"""
    from flamingo_mini_amd import decoding
    c, u = (t.clone() for t in GC.pair(320, F32, rows=6))
    c[0, 5] = u[0, 7] = u[1, 5] = c[1, 5] = GC.NINF
    c[2, 9] = float("nan")
    u[3, 11] = float("inf")
    u[4] = GC.NINF                                                              # a row of nothing but -inf: all -inf
    for g in GC.SCALES + [100.0]:
        out = decoding.guided_logits_torch(c, u, g)
        assert out.dtype == torch.float32 and out.shape == c.shape
        assert out[0, 5] == GC.NINF and out[0, 7] == GC.NINF and out[1, 5] == GC.NINF and bool((out[4] == GC.NINF).all())
        assert bool(out[2].isnan().all()) and bool(out[3].isnan().all())
        assert bool(out[5].isfinite().all()) and int(out[0].isfinite().sum()) == 318
        assert torch.equal(out.view(torch.int32), decoding.guided_logits_torch(c, u, torch.tensor([g])).view(torch.int32))
    out64 = decoding.guided_logits_torch(c.double(), u.double(), 1.5)
    assert out64.dtype == torch.float64 and torch.allclose(out64[5], GC.reference(c, u, 1.5)["out"][5], rtol=1e-13, atol=0)


# ---- the decoding -----------------------------------------------------------------------------------------------------------------------
L0, MAXLEN, GAP = 4, 10, 1e-3


@pytest.fixture(scope="module", params=["gpt2", "opt"])
def tiny(request):
    import oracle_backend
    from test_model_plumbing import build
    oracle_backend.install()
    try:
        model, z = build(torch.float64, "cpu", request.param)
        model.eval()
        gates = [p for n, p in model.named_parameters() if "alpha_" in n]
        with torch.no_grad():                                                 # (the golden weights leave one gate closed)
            for p in gates:
                if float(p.abs()) < 1e-3:
                    p.fill_(0.3)
        assert gates and all(float(p.detach().abs()) > 1e-3 for p in gates), "the golden model's gates are open"
        px = torch.from_numpy(z["px"]).double()
        ids, ml = torch.from_numpy(z["ids"])[:, :L0].clone(), torch.from_numpy(z["ml"])[:, :L0]
        ids[1] = (ids[1] + 39) % 90
        assert int(ml.sum()) > 0
        yield model, ids, dict(media_locations=ml, attention_mask=torch.ones_like(ids), pixel_values=px, max_length=MAXLEN)
    finally:
        oracle_backend.uninstall()


def two_forwards(model, seqs, ml0, px, g):
    """float64 guided scores (rows, V) of the next token from two uncached forwards over `seqs`: with the media and without"""
    n = seqs.shape[0] // ml0.shape[0]
    ml = torch.cat([ml0.repeat_interleave(n, 0), torch.zeros(seqs.shape[0], seqs.shape[1] - L0, dtype=ml0.dtype)], 1)
    kw = dict(input_ids=seqs, attention_mask=torch.ones_like(seqs), pixel_values=px.repeat_interleave(n, 0))
    with torch.no_grad():
        c = model(media_locations=ml, **kw).logits[:, -1]
        u = model(media_locations=torch.zeros_like(ml), **kw).logits[:, -1]
    assert c.dtype == torch.float64
    return GC.reference(c, u, g)["out"]


def gap_of(scores):
    top = scores.topk(2, dim=-1).values
    return float((top[:, 0] - top[:, 1]).min())


@pytest.mark.parametrize("g", [0.0, 0.5, 1.5, 3.0])
def test_guided_greedy_equals_two_uncached_forwards_per_step(tiny, g):
    model, ids, kw = tiny
    cur, gaps = ids, []
    while cur.shape[1] < MAXLEN:
        s = two_forwards(model, cur, kw["media_locations"], kw["pixel_values"], g)
        gaps.append(gap_of(s))
        cur = torch.cat([cur, s.argmax(-1, keepdim=True)], 1)
    print(f"g={g}: smallest float64 top-two gap {min(gaps):.3e}")
    assert min(gaps) >= GAP, gaps
    got = model.generate(ids, guidance_scale=g, **kw)
    assert torch.equal(got, cur), (got.tolist(), cur.tolist())
    assert torch.equal(model.generate(ids, guidance_scale=g, static_decode=False, **kw), cur) and len(model._decode_sessions) == 0
    if g == 0.0:                                                              # the prior alone: the ordinary decode of the same ids without media
        plain = model.generate(ids, **dict(kw, media_locations=torch.zeros_like(kw["media_locations"])))
        assert torch.equal(plain, cur)
    else:
        assert not torch.equal(model.generate(ids, **kw), model.generate(ids, **dict(kw, media_locations=torch.zeros_like(kw["media_locations"])))), \
            "the media change nothing here: the test would show nothing"


@pytest.mark.parametrize("groups", [{}, dict(num_beam_groups=3, diversity_penalty=0.5)], ids=["beams", "groups"])
def test_guided_beam_search_equals_the_search_over_two_uncached_forwards(tiny, groups):
    """the project's own search (decoding.beam_search) over a hand-written step that keeps the sequences as its cache and runs two uncached
    forwards per step, combined in float64; all nb hypotheses and their scores are compared, and the scores that the final ranking
    separates differ by at least GAP"""
    from flamingo_mini_amd import decoding as D
    model, ids, kw = tiny
    nb, g = 3, 1.5
    ml0, px = kw["media_locations"], kw["pixel_values"]

    def step(step_ids, ml, am, past, pixel_values, visual_features):
        seqs = step_ids if past is None else torch.cat([past[1][0][0], step_ids], 1)
        return two_forwards(model, seqs, ml0, px, g), ((), ((seqs,),))

    reorder = lambda past, idx: ((), ((past[1][0][0].index_select(0, idx),),))
    gr = D.Groups(3, 0.5) if groups else None
    want, want_s = D.beam_search(step, reorder, ids, ml0, kw["attention_mask"], None, None, MAXLEN, nb, None, 0, True, 1.0, n_return=nb, **({"groups": gr} if gr else {}))
    out = model.generate(ids, num_beams=nb, num_return_sequences=nb, return_dict_in_generate=True, guidance_scale=g, **groups, **kw)
    assert torch.equal(out.sequences, want), (out.sequences.tolist(), want.tolist())
    assert torch.allclose(out.sequences_scores, want_s, rtol=0, atol=1e-5)
    s = want_s.view(-1, nb).double() * MAXLEN
    ranked = (s[:, :-1] - s[:, 1:])[s[:, 1:] > -1e30]
    print(f"smallest gap between ranked hypotheses: {float(ranked.min()):.3e}")
    assert not groups and float(ranked.min()) >= GAP or groups and float(ranked[ranked > 0].min()) >= GAP       # (two groups may return one sequence: the penalty is soft)
    plain = model.generate(ids, num_beams=nb, **groups, **kw)
    assert torch.equal(model.generate(ids, num_beams=nb, guidance_scale=g, **groups, **kw), want[::nb]) and plain.shape == want[::nb].shape


def test_closed_gates_make_every_scale_the_unguided_decode(tiny):
    import copy
    model, ids, kw = tiny
    shut = copy.deepcopy(model)
    with torch.no_grad():
        for n, p in shut.named_parameters():
            if "alpha_" in n:
                p.zero_()
    plain = shut.generate(ids, **kw)
    assert not torch.equal(plain, model.generate(ids, **kw))
    for g in (0.0, 0.5, 1.5, 7.5):
        assert torch.equal(shut.generate(ids, guidance_scale=g, **kw), plain), g
    assert torch.equal(shut.generate(ids, guidance_scale=3.0, num_beams=3, **kw), shut.generate(ids, num_beams=3, **kw))


def test_bad_words_see_the_guided_scores(tiny):
    """the token guidance ranks first at the first step - and the unguided model does not - is banned: it is not produced, the runner-up of
    the GUIDED scores is"""
    model, ids, kw = tiny
    for g in (3.0, 7.5, 0.0):
        s = two_forwards(model, ids, kw["media_locations"], kw["pixel_values"], g)
        plain_first = model.generate(ids, **kw)[:, L0]
        first = s.argmax(-1)
        if not bool((first != plain_first).any()):
            continue
        r = int((first != plain_first).nonzero()[0, 0])
        banned = int(first[r])
        masked = s.clone()
        masked[:, banned] = GC.NINF
        assert gap_of(masked) >= GAP
        out = model.generate(ids, guidance_scale=g, bad_words_ids=[[banned]], **kw)
        assert banned not in out[:, L0:].tolist()[r] and torch.equal(out[:, L0], masked.argmax(-1))
        assert int(model.generate(ids, guidance_scale=g, **kw)[r, L0]) == banned
        return
    pytest.fail("no scale at which guidance changes the first token: the test would show nothing")
