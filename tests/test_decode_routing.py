"""The host side of decoding (flamingo_mini_amd/decoding.py) without a GPU and - but for the last test - without a model: decoding.route,
the one place that decides between the fixed-shape sessions and the dynamic loops, against a literal restatement of the rule over the full
cross product of its inputs; the option tuples (Sampling, Beams, Processors), which must stay interchangeable with plain tuples; and the
layout of a session key."""
import itertools

import pytest
import torch


def expected(is_cuda, num_beams, do_sample, static_decode, model_default, lm_family, L0, max_length, ids_is_int64, procs_on):
    """The rule, step by step as generate() applied it: "static", "dynamic", or the exception type (CPU = ffi.FusionLibraryError)."""
    if procs_on and not is_cuda:                                              # 1. the processors have no CPU form
        return "CPU" if static_decode else TypeError
    static_ok = lm_family is not None and L0 + 1 < max_length and (not procs_on or (ids_is_int64 and max_length <= 4096))      # 2.
    if num_beams > 1:                                                         # 3. beam search: static only on request, at most 8 beams
        if do_sample:
            return ValueError
        if static_decode:
            if not is_cuda:
                return "CPU"
            return "static" if static_ok and num_beams <= 8 else "dynamic"
        return "dynamic"
    if do_sample and static_decode:                                           # 4. sampling: static only on request
        if not is_cuda:
            return "CPU"
        return "static" if static_ok else "dynamic"
    if static_decode is None:                                                 # 5. greedy: static by default on the GPU
        static_decode = is_cuda and model_default
    return "static" if static_decode and not do_sample and static_ok else "dynamic"


CASES = [dict(is_cuda=c, num_beams=nb, do_sample=s, static_decode=sd, model_default=md, lm_family=fam, L0=4, max_length=ml, ids_is_int64=i64,
              procs_on=po)
         for c, nb, s, sd, md, fam, ml, po, i64 in itertools.product(
             (False, True), (1, 3, 9), (False, True), (None, True, False), (True, False), ("gpt2", None), (10, 5, 4097), (False, True), (True, False))]


def test_route_equals_the_rule_on_every_combination():
    from flamingo_mini_amd import decoding, ffi
    assert ffi.LOGITS_HIST_MAX == 4096 and ffi.BEAM_MAX == 8                  # the literals of expected()
    given = ["repetition_penalty", "min_length"]
    seen = set()
    for kw in CASES:
        want = expected(**kw)
        seen.add(want)
        if isinstance(want, str) and want != "CPU":
            assert decoding.route(**kw, procs_given=given) == want, kw
            continue
        exc, match = (ffi.FusionLibraryError, "no CPU fallback") if want == "CPU" else \
            (want, "unsupported generation arguments .*repetition_penalty.*min_length.* on CPU tensors" if want is TypeError else "beam search with sampling")
        with pytest.raises(exc, match=match):
            decoding.route(**kw, procs_given=given)
            pytest.fail(f"route did not raise for {kw}")
    assert seen == {"static", "dynamic", "CPU", TypeError, ValueError} and len(CASES) == 2 * 3 * 2 * 3 * 2 * 2 * 3 * 2 * 2


def test_route_takes_no_tensor_and_no_model():
    import inspect
    from flamingo_mini_amd import decoding
    params = inspect.signature(decoding.route).parameters
    assert list(params)[:10] == ["is_cuda", "num_beams", "do_sample", "static_decode", "model_default", "lm_family", "L0", "max_length",
                                 "ids_is_int64", "procs_on"]
    assert decoding.route(is_cuda=True, num_beams=1, do_sample=False, static_decode=None, model_default=True, lm_family="opt", L0=4,
                          max_length=10, ids_is_int64=True, procs_on=False) == "static"


def test_option_tuples_equal_and_hash_like_plain_tuples():
    from flamingo_mini_amd.decoding import Beams, Processors, Sampling
    for cls, plain in ((Sampling, (0.8, 20, 0.9)), (Beams, (3, True, 1.0)), (Processors, (1.0, 1, 0, 0))):
        opt = cls(*plain)
        assert isinstance(opt, tuple) and hasattr(cls, "_fields") and not hasattr(opt, "__dict__")
        assert opt == plain and plain == opt and hash(opt) == hash(plain) and {plain: 1}[opt] == 1
        assert tuple(opt) == plain and len(opt) == len(plain)
    T, k, p = Sampling(0.8, 20, 0.9)
    assert (T, k, p) == (0.8, 20, 0.9)
    assert Sampling._fields == ("temperature", "top_k", "top_p") and Beams._fields == ("nb", "early_stopping", "length_penalty")
    assert Processors._fields == ("repetition_penalty", "no_repeat_ngram_size", "min_length", "min_new_tokens")
    # a key tuple holding them is the key tuple holding plain ones
    assert hash((2, 10, Sampling(0.8, 20, 0.9), None)) == hash((2, 10, (0.8, 20, 0.9), None))


@pytest.mark.parametrize("min_length,min_new,L0", [(0, 0, 4), (7, 0, 4), (0, 6, 4), (7, 6, 4), (12, 6, 4), (5, 1, 4), (0, 0, 0), (3, 2, 1)])
def test_processors_min_len(min_length, min_new, L0):
    from flamingo_mini_amd.decoding import Processors
    assert Processors(1.3, 2, min_length, min_new).min_len(L0) == max(min_length, L0 + min_new)


def test_a_session_key_keeps_its_ten_elements_and_ends_in_the_processors():
    """One greedy generate() through a session on the host (the oracle backend), as tests/test_logits_args.py does: the key is
    (batch, max_length, images per sequence, device, eos, pad, graph, sampling, beams, processors)."""
    import oracle_backend
    from flamingo_mini_amd import modeling_flamingo as MF
    from test_model_plumbing import build
    oracle_backend.install()
    try:
        model, z = build(torch.float64, "cpu", "gpt2")
        model.eval()
        px = torch.from_numpy(z["px"]).double()
        ids, ml = torch.from_numpy(z["ids"])[:, :4], torch.from_numpy(z["ml"])[:, :4]
        model.generate(ids, media_locations=ml, attention_mask=torch.ones_like(ids), pixel_values=px, max_length=10, static_decode=True,
                       eos_token_id=5, pad_token_id=7)
        (key, sess), = model._decode_sessions.items()
        assert key == (ids.shape[0], 10, px.shape[1], "cpu", 5, 7, False, None, None, None)
        assert key[-1] is sess.processors and key[-2] is sess.beams and key[-3] is sess.sampling
        assert isinstance(sess, MF._DecodeSession) and (sess.b, sess.n_seq, sess.nb, sess.max_length, sess.eos, sess.fill) == (2, 2, 1, 10, 5, 7)
    finally:
        oracle_backend.uninstall()
        model.reset_decode_sessions()
