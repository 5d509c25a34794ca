"""Token log-probabilities, scores and num_return_sequences without a GPU: ff_token_logprob is bound and rejects bad arguments with its error
codes before anything reaches a device, functional.token_logprobs has no CPU form, and generate() on the host (the tiny model on the oracle
backend, as tests/test_logits_args.py): the dynamic greedy and sampling loops return the plain call's sequences plus token_logprobs that
equal a float64 teacher-forced log-softmax of those sequences, 0 after eos, and sequences_scores by the stated formula; every argument
error is a ValueError that builds no session; a default static call keeps its ten-element key and never calls token_logprobs; and beam
search on scripted logits (the set-up of tests/test_beam_args.py) returns its n best, best first, from both _beam_finalize and the dynamic
search."""
import ctypes as C

import numpy as np
import pytest
import torch

import beam_cases as BC

FF_ERR_SHAPE, FF_ERR_UNSUPPORTED = -1, -2
X = C.c_void_p(256)            # a non-null pointer that is never dereferenced: every call below returns before any launch


def _call(dtype=None, rows=4, vocab=100, ld=100, logits=X, token=X, skip=X, logprob=X, lse=X):
    from flamingo_mini_amd import ffi
    return ffi.lib().ff_token_logprob(ffi.DTYPE_BF16 if dtype is None else dtype, rows, vocab, ld, logits, token, skip, logprob, lse, None)


def test_the_entry_point_is_bound():
    import flamingo_mini_amd
    from flamingo_mini_amd import decoding, ffi, functional as F
    assert "ff_token_logprob" in ffi.EXPORTED_SYMBOLS and ffi.lib().ff_version() == 6
    assert callable(F.token_logprobs) and flamingo_mini_amd.GenerateOutput is decoding.GenerateOutput
    assert [f.name for f in __import__("dataclasses").fields(decoding.GenerateOutput)] == ["sequences", "sequences_scores", "token_logprobs"]


@pytest.mark.parametrize("bad", [
    dict(logits=None), dict(token=None), dict(logprob=None), dict(rows=0), dict(rows=-3), dict(vocab=0), dict(vocab=-1), dict(ld=99),
    dict(ld=99, skip=None, lse=None),
], ids=lambda d: "-".join(f"{k}={v}" for k, v in d.items()))
def test_argument_errors_return_shape_before_any_launch(bad):
    from flamingo_mini_amd import ffi
    assert _call(**bad) == FF_ERR_SHAPE
    assert b"ff_token_logprob" in ffi.lib().ff_last_error()


def test_other_dtypes_are_unsupported():
    from flamingo_mini_amd import ffi
    for dtype in (2, 7, -1):
        assert _call(dtype=dtype) == FF_ERR_UNSUPPORTED
        assert b"ff_token_logprob" in ffi.lib().ff_last_error() and b"dtype" in ffi.lib().ff_last_error()
    assert _call(dtype=7, rows=0) == FF_ERR_SHAPE                               # the shape checks come first


def test_token_logprobs_has_no_cpu_form():
    from flamingo_mini_amd import ffi, functional as F
    with pytest.raises(ffi.FusionLibraryError, match="no CPU fallback"):
        F.token_logprobs(torch.zeros(2, 5), torch.zeros(2, dtype=torch.long))


# ---- generate() on the host -----------------------------------------------------------------------------------------------------------
L0, MAXLEN = 4, 10


@pytest.fixture(scope="module", params=["gpt2", "opt"])
def tiny(request):
    import oracle_backend
    from test_model_plumbing import build
    oracle_backend.install()
    try:
        model, z = build(torch.float64, "cpu", request.param)
        model.eval()
        px = torch.from_numpy(z["px"]).double()
        ids, ml = torch.from_numpy(z["ids"])[:, :L0].clone(), torch.from_numpy(z["ml"])[:, :L0]
        ids[1] = (ids[1] + 39) % 90          # (greedy decoding of the tiny GPT-2 repeats one token; with this prompt the two rows repeat different ones)
        yield model, ids, dict(media_locations=ml, attention_mask=torch.ones_like(ids), pixel_values=px, max_length=MAXLEN)
    finally:
        oracle_backend.uninstall()


def teacher_forced(model, seqs, kw, eos):
    """float64 log-softmax, at the generated tokens, of the logits as the selection sees them (_decode_step hands the loops float32 logits)
    from ONE uncached forward over the finished sequences; 0 at the positions after a row's eos"""
    n = seqs.shape[0] // kw["media_locations"].shape[0]
    ml = kw["media_locations"].repeat_interleave(n, 0)
    mlf = torch.cat([ml, torch.zeros(seqs.shape[0], seqs.shape[1] - L0, dtype=ml.dtype)], 1)
    with torch.no_grad():
        lg = model(input_ids=seqs, attention_mask=torch.ones_like(seqs), media_locations=mlf, pixel_values=kw["pixel_values"].repeat_interleave(n, 0)).logits
    lp = lg.float().double().log_softmax(-1)[:, L0 - 1:-1].gather(-1, seqs[:, L0:, None])[..., 0]
    if eos is not None:
        after = ((seqs[:, L0:] == eos).long().cumsum(1) - (seqs[:, L0:] == eos).long()) > 0
        lp = torch.where(after, torch.zeros_like(lp), lp)
    return lp


def stated_scores(seqs, lps, eos, length_penalty):
    out = []
    for row, lp in zip(seqs[:, L0:].tolist(), lps):
        n_gen = row.index(eos) + 1 if eos is not None and eos in row else len(row)
        out.append(lp.sum() / float(np.float32(float(L0 + n_gen) ** length_penalty)))
    return torch.stack(out)


@pytest.mark.parametrize("mode", [dict(), dict(do_sample=True, temperature=0.7, top_p=0.9), dict(do_sample=True, num_return_sequences=3)],
                         ids=["greedy", "sampling", "sampling-n3"])
@pytest.mark.parametrize("with_eos", [False, True], ids=["no-eos", "eos"])
def test_dynamic_token_logprobs_equal_the_teacher_forced_log_softmax(tiny, mode, with_eos):
    from flamingo_mini_amd import GenerateOutput
    model, ids, kw = tiny
    gen = lambda: dict(generator=torch.Generator().manual_seed(5)) if mode else {}
    eos_kw = {}
    if with_eos:                                                              # an eos that one row reaches at least two steps before another
        first = model.generate(ids, **mode, **gen(), **kw)[:, L0:]
        eos = next((int(first[r, j]) for j in range(first.shape[1] - 2) for r in range(first.shape[0])
                    if int(first[r, j]) != 0 and any(int(first[r, j]) not in first[q, :j + 2].tolist() for q in range(first.shape[0]) if q != r)), None)
        assert eos is not None, first.tolist()
        eos_kw = dict(eos_token_id=eos, pad_token_id=0, length_penalty=0.7)
    plain = model.generate(ids, **mode, **eos_kw, **gen(), **kw)
    out = model.generate(ids, **mode, **eos_kw, **gen(), return_dict_in_generate=True, output_logprobs=True, **kw)
    assert isinstance(out, GenerateOutput) and torch.equal(out.sequences, plain)
    n = mode.get("num_return_sequences", 1)
    assert plain.shape[0] == ids.shape[0] * n and all(torch.equal(plain[r, :L0], ids[r // n]) for r in range(plain.shape[0]))
    assert out.token_logprobs.shape == (plain.shape[0], plain.shape[1] - L0)
    eos = eos_kw.get("eos_token_id")
    want = teacher_forced(model, plain, kw, eos)
    err = float((out.token_logprobs.double() - want).abs().max())
    print(f"largest |token_logprobs - teacher forced|: {err:.3e}")
    assert err <= 1e-12
    if with_eos:
        gen_part = plain[:, L0:]
        after = ((gen_part == eos).long().cumsum(1) - (gen_part == eos).long()) > 0
        assert int(after.sum()) > 0 and bool((out.token_logprobs[after] == 0).all()) and bool((gen_part[after] == 0).all())
        assert bool((out.token_logprobs[gen_part == eos][:1] != 0).all())     # the eos token itself carries its log-probability
    lpen = eos_kw.get("length_penalty", 1.0)
    assert torch.allclose(out.sequences_scores.double(), stated_scores(plain, out.token_logprobs.double(), eos, lpen), rtol=1e-12, atol=0)
    assert len(model._decode_sessions) == 0
    only = model.generate(ids, **mode, **eos_kw, **gen(), return_dict_in_generate=True, **kw)
    assert torch.equal(only.sequences, plain) and only.token_logprobs is None and only.sequences_scores is None


@pytest.mark.parametrize("bad", [
    dict(output_logprobs=True), dict(output_logprobs=True, return_dict_in_generate=True, num_beams=3),
    dict(num_return_sequences=0), dict(num_return_sequences=-1), dict(num_return_sequences=2.0), dict(num_return_sequences=True),
    dict(num_return_sequences=2), dict(num_return_sequences=4, num_beams=3), dict(num_return_sequences=2, return_dict_in_generate=True),
], ids=lambda d: "-".join(f"{k}={v}" for k, v in d.items()))
def test_generate_rejects_bad_output_arguments(tiny, bad):
    model, ids, kw = tiny
    for static in (None, True, False):
        with pytest.raises(ValueError):
            model.generate(ids, static_decode=static, **bad, **kw)
    assert len(model._decode_sessions) == 0


def test_routing_of_logprobs_on_cpu_tensors(tiny):
    """a static session that records log-probabilities needs GPU tensors: static_decode=True raises what ffi.require_cuda raises and builds no
    session; with static_decode=None (and False) the dynamic loop runs"""
    from flamingo_mini_amd import decoding, ffi
    model, ids, kw = tiny
    with pytest.raises(ffi.FusionLibraryError, match="no CPU fallback"):
        model.generate(ids, static_decode=True, return_dict_in_generate=True, output_logprobs=True, **kw)
    assert len(model._decode_sessions) == 0
    a = model.generate(ids, return_dict_in_generate=True, output_logprobs=True, **kw)
    b = model.generate(ids, static_decode=False, return_dict_in_generate=True, output_logprobs=True, **kw)
    assert len(model._decode_sessions) == 0 and torch.equal(a.sequences, b.sequences) and torch.equal(a.token_logprobs, b.token_logprobs)
    base = dict(num_beams=1, do_sample=False, model_default=True, lm_family="gpt2", L0=4, max_length=10, ids_is_int64=True, procs_on=False)
    assert decoding.route(is_cuda=True, static_decode=None, **base, logprobs_on=True) == "static"
    assert decoding.route(is_cuda=False, static_decode=None, **base, logprobs_on=True) == "dynamic"
    assert decoding.route(is_cuda=False, static_decode=True, **base) == "static"          # greedy without the option still runs on the host
    with pytest.raises(ffi.FusionLibraryError, match="no CPU fallback"):
        decoding.route(is_cuda=False, static_decode=True, **base, logprobs_on=True)


def test_a_default_session_keeps_its_key_and_never_calls_token_logprobs(tiny, monkeypatch):
    from flamingo_mini_amd import functional as F
    model, ids, kw = tiny
    calls = []
    monkeypatch.setattr(F, "token_logprobs", lambda *a, **k: calls.append(a))
    try:
        out = model.generate(ids, static_decode=True, eos_token_id=5, pad_token_id=7, **kw)
        assert torch.equal(out, model.generate(ids, static_decode=False, eos_token_id=5, pad_token_id=7, **kw))
        (key, sess), = model._decode_sessions.items()
        assert key == (ids.shape[0], MAXLEN, kw["pixel_values"].shape[1], "cpu", 5, 7, False, None, None, None)
        assert sess.logprobs is False and not hasattr(sess, "lp_buf") and not hasattr(sess, "lp_step")
        assert calls == []
        boxed = model.generate(ids, static_decode=True, eos_token_id=5, pad_token_id=7, return_dict_in_generate=True, **kw)
        assert torch.equal(boxed.sequences, out) and boxed.token_logprobs is None and len(model._decode_sessions) == 1 and calls == []
    finally:
        model.reset_decode_sessions()


def test_generate_captions_forwards_and_groups(tiny):
    """generate_captions with return_scores and num_return_sequences, against a stub processor: b lists of n captions and of n float scores"""
    model, ids, kw = tiny

    class Tok:
        def batch_decode(self, rows, skip_special_tokens=True):
            return [" ".join(str(int(t)) for t in r) for r in rows]

    class Proc:
        tokenizer = Tok()

        def encode_text(self, prompt, device):
            return ids[:1], kw["media_locations"][:1], torch.ones_like(ids[:1])

        def remove_tags(self, t):
            return t

    px = kw["pixel_values"]
    plain = model.generate_captions(Proc(), pixel_values=px, max_length=MAXLEN, static_decode=False)
    assert isinstance(plain, list) and len(plain) == px.shape[0] and all(isinstance(c, str) for c in plain)
    caps, scores = model.generate_captions(Proc(), pixel_values=px, max_length=MAXLEN, static_decode=False, return_scores=True)
    assert caps == plain and len(scores) == len(caps) and all(isinstance(s, float) and s < 0 for s in scores)
    caps, scores = model.generate_captions(Proc(), pixel_values=px, max_length=MAXLEN, num_beams=3, num_return_sequences=2, return_scores=True)
    assert len(caps) == px.shape[0] == len(scores) and all(len(c) == 2 for c in caps) and all(len(s) == 2 and s[0] >= s[1] for s in scores)
    assert [c[0] for c in caps] == model.generate_captions(Proc(), pixel_values=px, max_length=MAXLEN, num_beams=3)


# ---- beam search on scripted logits (the set-up of tests/test_beam_args.py) ------------------------------------------------------------------
V, NB, BL0, BMAXLEN, EOS, PAD = 40, 3, 2, 14, 7, 0
PROMPT = np.array([[1, 11], [2, 12], [3, 13]], np.int64)
BOOST = {1: (4, 9.0), 2: (6, 5.5)}
CASES = [(True, 1.0, EOS, 8), (False, 1.0, EOS, 29), (True, 0.6, EOS, 58), (False, 2.0, EOS, 102), (True, 1.0, None, 121)]     # of test_beam_args.CASES


@pytest.mark.parametrize("early,lp,eos,seed", CASES)
def test_beam_search_returns_its_n_best(early, lp, eos, seed):
    """n = num_beams: rows in non-increasing score order, row 0 and its score are today's single result, _beam_finalize(n_return=n) on the
    restatement's state agrees with the dynamic search token for token, and its scores (float32 steps there, float64 divisions here) to
    1e-5 relative - 40 times the 14 float32 roundings a running score can collect."""
    from flamingo_mini_amd.modeling_flamingo import _beam_finalize
    script = BC.Script(V, seed, eos=eos, eos_boost=BOOST)
    st, worst = BC.run_restatement(script, PROMPT, NB, BMAXLEN, eos, PAD, early, lp)
    assert worst >= 1e-3
    ids = torch.from_numpy(PROMPT)
    args = (ids, torch.zeros_like(ids), torch.ones_like(ids), None, None, BMAXLEN, NB, eos, PAD, early, lp)
    single = BC.ScriptedModel(script).search(*args)
    assert torch.equal(single, _beam_finalize(st, BL0, PROMPT, NB, PAD))
    got, got_s = BC.ScriptedModel(script).search(*args, n_return=NB)
    want, want_s = _beam_finalize(st, BL0, PROMPT, NB, PAD, n_return=NB)
    assert got.shape == want.shape == (len(PROMPT) * NB, want.shape[1]) and torch.equal(got, want), (got.tolist(), want.tolist())
    assert got_s.dtype == want_s.dtype == torch.float32 and got_s.shape == want_s.shape == (len(PROMPT) * NB,)
    finite = torch.isfinite(want_s)
    assert torch.equal(finite, torch.isfinite(got_s)) and torch.allclose(got_s[finite], want_s[finite], rtol=1e-5, atol=0)
    for scores in (got_s.view(-1, NB), want_s.view(-1, NB)):
        assert bool((scores[:, :-1] >= scores[:, 1:]).all()), scores
    first = want[::NB]
    assert torch.equal(first[:, :single.shape[1]], single) and bool((first[:, single.shape[1]:] == PAD).all())
    one, one_s = _beam_finalize(st, BL0, PROMPT, NB, PAD, n_return=1)
    assert torch.equal(one, single) and torch.equal(one_s, want_s[::NB])
    for r in range(want.shape[0]):                                             # every returned row is a distinct entry of its sequence
        assert want[r, :BL0].tolist() == PROMPT[r // NB].tolist() or not bool(finite[r])
    assert len({tuple(x) for x in want[:NB][finite[:NB]].tolist()}) == int(finite[:NB].sum())


def test_fewer_entries_than_n_pad_with_pad_and_minus_inf():
    from flamingo_mini_amd.modeling_flamingo import _beam_finalize
    script = BC.Script(V, 29, eos=EOS, eos_boost=BOOST)
    st, _ = BC.run_restatement(script, PROMPT, NB, BMAXLEN, EOS, PAD, False, 1.0)
    full, full_s = _beam_finalize(st, BL0, PROMPT, NB, PAD, n_return=NB)
    st = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in st.items()}
    s = int(np.flatnonzero(st["done"] == 0)[0])                               # a sequence that ran to the length limit: keep one open beam
    st["n_hyp"][s] = 0
    st["score"][s, 1:] = -np.inf
    ids, scores = _beam_finalize(st, BL0, PROMPT, NB, 9, n_return=NB)
    rows = ids[s * NB:(s + 1) * NB]
    assert bool(torch.isfinite(scores[s * NB])) and rows[0, :BL0].tolist() == PROMPT[s].tolist()
    assert bool((rows[1:] == 9).all()) and scores[s * NB + 1:(s + 1) * NB].tolist() == [float("-inf")] * (NB - 1)
    other = [r for r in range(len(PROMPT) * NB) if r // NB != s]
    assert torch.equal(scores[other], full_s[other])
