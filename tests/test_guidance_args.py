"""Classifier-free guidance without a GPU: ff_guided_logits is bound and rejects bad arguments with its error codes before anything reaches a
device, functional.guided_logits has no CPU form, generate() rejects bad guidance_scale values in every mode and builds no session, the
routing table for `guidance_on`, and - with monkeypatched recorders, as the other *_args tests - guidance_scale=1.0 hands _static_decode,
dynamic_decode and _beam_search exactly the arguments a call without it hands them, while any other scale hands them the guided step (the
dynamic loops) or `guidance=` (the static path); generate_captions passes the argument on."""
import ctypes as C

import pytest
import torch

FF_ERR_SHAPE, FF_ERR_UNSUPPORTED = -1, -2
X = C.c_void_p(256)            # a non-null pointer that is never dereferenced: every call below returns before any launch
L0, MAXLEN = 4, 10


def _call(dtype=None, rows=4, vocab=100, ld_cond=100, cond=X, ld_uncond=200, uncond=X, scale=X, out=X, ld_out=101):
    from flamingo_mini_amd import ffi
    return ffi.lib().ff_guided_logits(ffi.DTYPE_BF16 if dtype is None else dtype, rows, vocab, ld_cond, cond, ld_uncond, uncond, scale, out, ld_out, None)


def test_the_entry_point_is_bound():
    from flamingo_mini_amd import decoding, ffi, functional as F
    assert "ff_guided_logits" in ffi.EXPORTED_SYMBOLS and ffi.lib().ff_version() == 6
    assert callable(F.guided_logits) and callable(decoding.guided_logits_torch) and callable(decoding.check_guidance_args)


@pytest.mark.parametrize("bad", [
    dict(cond=None), dict(uncond=None), dict(scale=None), dict(out=None), dict(rows=0), dict(rows=-3), dict(vocab=0), dict(vocab=-1),
    dict(ld_cond=99), dict(ld_uncond=99), dict(ld_out=99),
], ids=lambda d: "-".join(f"{k}={v}" for k, v in d.items()))
def test_argument_errors_return_shape_before_any_launch(bad):
    from flamingo_mini_amd import ffi
    assert _call(**bad) == FF_ERR_SHAPE
    assert b"ff_guided_logits" in ffi.lib().ff_last_error()


def test_other_dtypes_are_unsupported():
    from flamingo_mini_amd import ffi
    for dtype in (2, 7, -1):
        assert _call(dtype=dtype) == FF_ERR_UNSUPPORTED
        assert b"ff_guided_logits" in ffi.lib().ff_last_error() and b"dtype" in ffi.lib().ff_last_error()
    assert _call(dtype=7, rows=0) == FF_ERR_SHAPE                               # the shape checks come first


def test_guided_logits_has_no_cpu_form():
    from flamingo_mini_amd import ffi, functional as F
    with pytest.raises(ffi.FusionLibraryError, match="no CPU fallback"):
        F.guided_logits(torch.zeros(2, 5), torch.zeros(2, 5), torch.ones(1))


def test_check_guidance_args():
    from flamingo_mini_amd.decoding import check_guidance_args
    assert check_guidance_args(1.0) is None and check_guidance_args(1) is None
    for g, want in ((0, 0.0), (0.0, 0.0), (0.5, 0.5), (1.5, 1.5), (3, 3.0), (7.5, 7.5)):
        got = check_guidance_args(g)
        assert got == want and isinstance(got, float)
    for bad in (-0.1, -1, float("inf"), float("-inf"), float("nan"), "1.5", None, True, False, [1.5], torch.tensor(1.5)):
        with pytest.raises(ValueError, match="guidance_scale"):
            check_guidance_args(bad)


@pytest.fixture(scope="module")
def tiny():
    import oracle_backend
    from test_model_plumbing import build
    oracle_backend.install()
    try:
        model, z = build(torch.float64, "cpu", "gpt2")
        model.eval()
        ids, ml = torch.from_numpy(z["ids"])[:, :L0].clone(), torch.from_numpy(z["ml"])[:, :L0]
        yield model, ids, dict(media_locations=ml, attention_mask=torch.ones_like(ids), pixel_values=torch.from_numpy(z["px"]).double(), max_length=MAXLEN)
    finally:
        oracle_backend.uninstall()


@pytest.mark.parametrize("bad", [-0.5, float("inf"), float("nan"), "2", None, True], ids=str)
@pytest.mark.parametrize("mode", [dict(), dict(do_sample=True), dict(num_beams=3)], ids=["greedy", "sampling", "beams"])
def test_generate_rejects_bad_scales(tiny, bad, mode):
    model, ids, kw = tiny
    for static in (None, True, False):
        with pytest.raises(ValueError, match="guidance_scale"):
            model.generate(ids, static_decode=static, guidance_scale=bad, **mode, **kw)
    assert len(model._decode_sessions) == 0


def test_routing_table():
    from flamingo_mini_amd import decoding, ffi
    base = dict(model_default=True, lm_family="gpt2", L0=4, max_length=10, ids_is_int64=True, procs_on=False)
    greedy, sampling, beams = dict(num_beams=1, do_sample=False), dict(num_beams=1, do_sample=True), dict(num_beams=3, do_sample=False)
    r = lambda **k: decoding.route(**base, guidance_on=True, **k)
    assert r(is_cuda=True, static_decode=None, **greedy) == "static"            # guided greedy: static by default on the GPU, as greedy
    assert r(is_cuda=True, static_decode=False, **greedy) == "dynamic"
    for mode in (sampling, beams):                                              # guided sampling and beam search: static on request
        assert r(is_cuda=True, static_decode=None, **mode) == "dynamic" and r(is_cuda=True, static_decode=True, **mode) == "static"
    for mode in (greedy, sampling, beams):                                      # CPU tensors: the dynamic loop; static_decode=True cannot be had
        assert r(is_cuda=False, static_decode=None, **mode) == "dynamic" and r(is_cuda=False, static_decode=False, **mode) == "dynamic"
        with pytest.raises(ffi.FusionLibraryError, match="no CPU fallback"):
            r(is_cuda=False, static_decode=True, **mode)
    assert decoding.route(**base, is_cuda=False, static_decode=True, **greedy) == "static"      # without guidance greedy still runs on the host
    assert r(is_cuda=True, static_decode=None, **greedy, **{}) == decoding.route(**base, is_cuda=True, static_decode=None, **greedy)
    assert decoding.route(**dict(base, lm_family=None), guidance_on=True, is_cuda=True, static_decode=True, **greedy) == "dynamic"


def test_cpu_tensors_take_the_dynamic_loop_and_static_raises(tiny):
    from flamingo_mini_amd import ffi
    model, ids, kw = tiny
    with pytest.raises(ffi.FusionLibraryError, match="no CPU fallback"):
        model.generate(ids, static_decode=True, guidance_scale=1.5, **kw)
    a = model.generate(ids, guidance_scale=1.5, **kw)
    assert torch.equal(a, model.generate(ids, static_decode=False, guidance_scale=1.5, **kw)) and a.shape == (ids.shape[0], MAXLEN)
    assert len(model._decode_sessions) == 0


def _same(a, b):
    if isinstance(a, torch.Tensor) or isinstance(b, torch.Tensor):
        return isinstance(a, torch.Tensor) and isinstance(b, torch.Tensor) and a.dtype == b.dtype and torch.equal(a, b)
    if isinstance(a, (tuple, list)) and type(a) is type(b):
        return len(a) == len(b) and all(_same(x, y) for x, y in zip(a, b))
    if isinstance(a, dict) and isinstance(b, dict):
        return list(a) == list(b) and all(_same(a[k], b[k]) for k in a)
    if isinstance(a, torch.Generator):
        return a is b
    if type(a).__name__ == "Constraints":                                      # (built anew by every call: compared by content)
        return type(a) is type(b) and a.caps() == b.caps() and a.trie is None and b.trie is None and a.bad_words.words == b.bad_words.words
    return type(a) is type(b) and a == b


MODES = [dict(), dict(do_sample=True, temperature=0.7, top_k=5), dict(num_beams=3), dict(num_beams=3, num_beam_groups=3, diversity_penalty=0.5),
         dict(eos_token_id=5, bad_words_ids=[[3]]), dict(return_dict_in_generate=True, output_logprobs=True)]


@pytest.mark.parametrize("mode", MODES, ids=lambda d: "-".join(d) or "greedy")
@pytest.mark.parametrize("static", [None, True, False])
def test_scale_one_passes_exactly_the_arguments_of_a_call_without_it(tiny, monkeypatch, mode, static):
    from flamingo_mini_amd import decoding as D, ffi
    model, ids, kw = tiny
    seen = []
    rec = lambda name: (lambda *a, **k: (seen.append((name, a, k)), (ids, torch.zeros(ids.shape[0], 0)))[1])
    monkeypatch.setattr(D, "_static_decode", rec("static"))
    monkeypatch.setattr(D, "dynamic_decode", rec("dynamic"))
    monkeypatch.setattr(type(model), "_beam_search", rec("beams"))
    monkeypatch.setattr(D, "route", (lambda orig: lambda **k: (seen.append(("route", (), k)), orig(**k))[1])(D.route))
    calls = []
    for extra in ({}, dict(guidance_scale=1.0), dict(guidance_scale=1)):
        seen.clear()
        try:
            model.generate(ids, static_decode=static, **mode, **extra, **kw)
        except ffi.FusionLibraryError:                                        # (static_decode=True on CPU tensors where a mode needs the GPU)
            seen.append(("raised", (), {}))
        calls.append(list(seen))
    assert len(calls[0]) == 2 and calls[0][0][0] == "route"
    for other in calls[1:]:
        assert [c[0] for c in other] == [c[0] for c in calls[0]]
        for (_, a0, k0), (_, a1, k1) in zip(calls[0], other):
            assert _same(a0, a1) and _same(k0, k1), (k0.keys(), k1.keys())
    for _, a, k in calls[0]:
        assert not {"guidance", "guidance_on", "guidance_scale", "step", "reorder_cache"} & set(k), k.keys()


def test_another_scale_hands_the_loops_the_guided_step_and_the_static_path_the_scale(tiny, monkeypatch):
    from flamingo_mini_amd import decoding as D
    model, ids, kw = tiny
    seen = []
    rec = lambda name: (lambda *a, **k: (seen.append((name, a, k)), ids)[1])
    monkeypatch.setattr(D, "_static_decode", rec("static"))
    monkeypatch.setattr(D, "dynamic_decode", rec("dynamic"))
    monkeypatch.setattr(type(model), "_beam_search", rec("beams"))
    monkeypatch.setattr(D, "route", lambda **k: (seen.append(("route", (), k)), "static" if k["static_decode"] else "dynamic")[1])
    model.generate(ids, guidance_scale=2.5, **kw)
    model.generate(ids, guidance_scale=2.5, num_beams=3, **kw)
    model.generate(ids, guidance_scale=2.5, static_decode=True, **kw)
    (_, _, r0), (_, a_dyn, k_dyn), (_, _, r1), (_, a_beam, k_beam), (_, _, r2), (_, a_st, k_st) = seen
    assert r0["guidance_on"] is True and r1["guidance_on"] is True and r2["guidance_on"] is True
    assert a_dyn[0] is not None and a_dyn[0] != model._decode_step and a_dyn[0].__name__ == "guided" and "guidance" not in k_dyn
    assert k_beam["step"].__name__ == "guided" and callable(k_beam["reorder_cache"]) and "guidance" not in k_beam
    assert k_st["guidance"] == 2.5 and isinstance(k_st["guidance"], float)
    for a in (a_dyn[1:6], a_beam[1:6], a_st[1:6]):                             # the visuals reach every path encoded, once
        assert a[-2] is None and a[-1] is not None and a[-1].shape[0] == ids.shape[0]


def test_a_default_session_keeps_its_key_and_never_calls_guided_logits(tiny, monkeypatch):
    from flamingo_mini_amd import functional as F
    model, ids, kw = tiny
    calls = []
    monkeypatch.setattr(F, "guided_logits", lambda *a, **k: calls.append(a))
    try:
        out = model.generate(ids, static_decode=True, eos_token_id=5, pad_token_id=7, guidance_scale=1.0, **kw)
        assert torch.equal(out, model.generate(ids, static_decode=False, eos_token_id=5, pad_token_id=7, **kw))
        (key, sess), = model._decode_sessions.items()
        assert key == (ids.shape[0], MAXLEN, kw["pixel_values"].shape[1], "cpu", 5, 7, False, None, None, None)
        assert sess.guidance is False and not any(hasattr(sess, n) for n in ("lm_tok", "scale", "guided", "lm_beam_idx"))
        assert sess.am_buf.shape[0] == sess.tt_step.shape[0] == ids.shape[0] and calls == []
    finally:
        model.reset_decode_sessions()


def test_generate_captions_passes_the_scale_on(tiny):
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
    assert model.generate_captions(Proc(), pixel_values=px, max_length=MAXLEN, static_decode=False, guidance_scale=1.0) == plain
    guided = model.generate_captions(Proc(), pixel_values=px, max_length=MAXLEN, guidance_scale=7.5)
    assert len(guided) == len(plain) and guided != plain
    with pytest.raises(ValueError, match="guidance_scale"):
        model.generate_captions(Proc(), pixel_values=px, max_length=MAXLEN, guidance_scale=-1.0)
