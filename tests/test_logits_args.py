"""Logits processors without a GPU: ff_logits_process is bound and rejects bad arguments with its error codes before anything reaches a
device, the call with every processor off returns success without touching its pointers, functional.process_logits has no CPU form,
generate() rejects bad values, and the routing on the host: with CPU tensors the processor arguments stay unsupported generation
arguments (TypeError, as before the feature), static_decode=True on CPU tensors raises and builds no session, a session without processors
never calls process_logits, and the dynamic beam search applies the rules before its log-softmax (FlamingoModel._beam_search on scripted
logits against the beam restatement, token for token).  The dynamic greedy and sampling loops need GPU tensors: tests/test_hip_logits.py."""
import ctypes as C

import numpy as np
import pytest
import torch

import beam_cases as BC
import logits_cases as LC

FF_OK, FF_ERR_SHAPE, FF_ERR_UNSUPPORTED = 0, -1, -2
X = C.c_void_p(256)            # a non-null pointer that is never dereferenced: every call below returns before any launch


def _call(dtype=None, rows=4, vocab=100, ld=100, logits=X, hist=X, hist_ld=16, hist_cap=16, hist_len=X, p=1.3, g=2, eos=5, min_len=X):
    from flamingo_mini_amd import ffi
    return ffi.lib().ff_logits_process(ffi.DTYPE_BF16 if dtype is None else dtype, rows, vocab, ld, logits, hist, hist_ld, hist_cap, hist_len,
                                       p, g, eos, min_len, None)


def test_the_entry_point_is_bound():
    from flamingo_mini_amd import ffi, functional as F
    assert "ff_logits_process" in ffi.EXPORTED_SYMBOLS and ffi.lib().ff_version() == 6
    assert callable(F.process_logits) and ffi.LOGITS_HIST_MAX == 4096


@pytest.mark.parametrize("bad", [
    dict(logits=None), dict(hist=None), dict(hist_len=None),
    dict(rows=0), dict(rows=-3), dict(vocab=0), dict(vocab=-1), dict(ld=99),
    dict(hist_cap=0), dict(hist_cap=-1), dict(hist_ld=15),
    dict(p=0.0), dict(p=-1.3), dict(p=float("inf")), dict(p=float("nan")),
    dict(g=-1),
    dict(eos=-2), dict(eos=100), dict(eos=1 << 20),
], ids=lambda d: "-".join(f"{k}={v}" for k, v in d.items()))
def test_argument_errors_return_shape_before_any_launch(bad):
    from flamingo_mini_amd import ffi
    assert _call(**bad) == FF_ERR_SHAPE
    assert b"ff_logits_process" in ffi.lib().ff_last_error()


def test_other_dtypes_and_longer_histories_are_unsupported():
    from flamingo_mini_amd import ffi
    assert _call(dtype=7) == FF_ERR_UNSUPPORTED
    assert b"ff_logits_process" in ffi.lib().ff_last_error() and b"dtype" in ffi.lib().ff_last_error()
    assert _call(hist_cap=4097, hist_ld=4097) == FF_ERR_UNSUPPORTED
    assert b"ff_logits_process" in ffi.lib().ff_last_error() and b"FF_LOGITS_HIST_MAX" in ffi.lib().ff_last_error()


@pytest.mark.parametrize("off", [dict(p=1.0, g=0, eos=-1), dict(p=1.0, g=0, eos=-1, min_len=None), dict(p=1.0, g=0, eos=5, min_len=None)],
                         ids=lambda d: "-".join(f"{k}={v}" for k, v in d.items()))
def test_every_processor_off_returns_success_and_launches_nothing(off):
    """(the pointers are not memory: a launch, or any read of *hist_len, would fault or fail)"""
    assert _call(**off) == FF_OK
    assert _call(hist_cap=4096, hist_ld=4096, **off) == FF_OK
    assert _call(**dict(off, rows=0)) == FF_ERR_SHAPE                         # the checks still come first


def test_process_logits_has_no_cpu_form():
    from flamingo_mini_amd import ffi, functional as F
    with pytest.raises(ffi.FusionLibraryError, match="no CPU fallback"):
        F.process_logits(torch.zeros(2, 5), torch.zeros(2, 4, dtype=torch.long), torch.zeros(1, dtype=torch.long), repetition_penalty=1.3)


# ---- generate() on the host -----------------------------------------------------------------------------------------------------------
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
        yield model, ids, dict(media_locations=ml, attention_mask=torch.ones_like(ids), pixel_values=px, max_length=10)
    finally:
        oracle_backend.uninstall()


@pytest.mark.parametrize("bad", [
    dict(repetition_penalty=0.0), dict(repetition_penalty=-1.0), dict(repetition_penalty=float("inf")), dict(repetition_penalty=float("nan")),
    dict(repetition_penalty="1.3"), dict(no_repeat_ngram_size=-1), dict(no_repeat_ngram_size=1.5), dict(min_length=-1), dict(min_new_tokens=-2),
    dict(min_length=6), dict(min_new_tokens=2),                                # the minimum-length rule needs eos_token_id
], ids=lambda d: "-".join(f"{k}={v}" for k, v in d.items()))
def test_generate_rejects_bad_values(tiny, bad):
    model, ids, kw = tiny
    with pytest.raises(ValueError):
        model.generate(ids, **bad, **kw)
    with pytest.raises(ValueError):
        model.generate(ids, num_beams=2, **bad, **kw)
    assert len(model._decode_sessions) == 0


PROC = dict(repetition_penalty=1.3, no_repeat_ngram_size=2, min_length=8)


@pytest.mark.parametrize("mode", [dict(), dict(static_decode=False), dict(do_sample=True), dict(num_beams=3)],
                         ids=lambda d: "-".join(f"{k}={v}" for k, v in d.items()) or "default")
def test_cpu_tensors_keep_raising_type_error(tiny, mode):
    """The processors are offered for GPU tensors only (the dynamic loops on GPU tensors are held to the rules in tests/test_hip_logits.py):
    with CPU tensors every one of the arguments is what it was before, an unsupported generation argument, in every mode - named in the
    message - and nothing builds a session.  Their defaults are accepted."""
    model, ids, kw = tiny
    for args in (dict(repetition_penalty=1.3), dict(no_repeat_ngram_size=2), dict(min_length=8, eos_token_id=5), dict(min_new_tokens=2, eos_token_id=5), PROC):
        with pytest.raises(TypeError, match="unsupported generation arguments") as e:
            model.generate(ids, **dict(dict(eos_token_id=5), **args), **mode, **kw)
        assert all(name in str(e.value) for name in args if name != "eos_token_id"), str(e.value)
    assert len(model._decode_sessions) == 0
    out = model.generate(ids, repetition_penalty=1.0, no_repeat_ngram_size=0, min_length=0, min_new_tokens=0, static_decode=False, **kw)
    assert torch.equal(out, model.generate(ids, static_decode=False, **kw))


def test_static_decode_on_cpu_tensors_raises_and_builds_no_session(tiny):
    from flamingo_mini_amd import ffi
    model, ids, kw = tiny
    for mode in (dict(), dict(do_sample=True), dict(num_beams=3)):
        with pytest.raises(ffi.FusionLibraryError, match="no CPU fallback"):
            model.generate(ids, static_decode=True, eos_token_id=5, **mode, **PROC, **kw)
    assert len(model._decode_sessions) == 0


def test_a_session_without_processors_never_calls_process_logits(tiny, monkeypatch):
    """greedy static decoding runs on the host too (the oracle backend): default arguments build a session with processors None, no min_len and
    no seq_buf, and functional.process_logits is not called once"""
    from flamingo_mini_amd import functional as F
    model, ids, kw = tiny
    calls = []
    monkeypatch.setattr(F, "process_logits", lambda *a, **k: calls.append(a))
    try:
        out = model.generate(ids, static_decode=True, repetition_penalty=1.0, no_repeat_ngram_size=0, min_length=0, min_new_tokens=0, **kw)
        assert torch.equal(out, model.generate(ids, static_decode=False, **kw))
        (key, sess), = model._decode_sessions.items()
        assert sess.processors is None and key[-1] is None and not hasattr(sess, "seq_buf") and not hasattr(sess, "min_len")
        assert calls == []
    finally:
        model.reset_decode_sessions()


# ---- dynamic beam search: FlamingoModel._beam_search on scripted logits -----------------------------------------------------------------
V, NB, L0, MAXLEN, EOS, PAD = 40, 3, 2, 14, 7, 0
PROMPT = np.array([[1, 11], [2, 12], [3, 13]], np.int64)
BOOST = {1: (4, 9.0), 2: (6, 5.5)}


class Processed:
    """a script's logits after the restatement of the rules against the same history"""

    def __init__(self, script, p, g, min_len):
        self.script, self.p, self.g, self.min_len = script, p, g, min_len

    def __call__(self, hist):
        hist = np.asarray(hist)
        return LC.restate_values(self.script(hist), "f32", hist, hist.shape[1], p=self.p, g=self.g, eos=EOS, min_len=self.min_len)


@pytest.mark.parametrize("p,g,min_length,min_new", [(1.3, 2, 0, 0), (1.0, 1, 0, 0), (1.3, 0, 7, 0), (0.8, 3, 0, 6)])
def test_dynamic_beam_search_applies_the_rules_before_the_log_softmax(p, g, min_length, min_new):
    """_beam_search(processors=...) on scripted logits returns what the beam restatement (tests/beam_cases.py) plus _beam_finalize return when
    the SCRIPT is processed - i.e. the processors act on the logits and the log-softmax renormalises afterwards.  The first seed whose run is
    decidable (consecutive candidate scores >= 1e-3 apart) is used; sequence "1" is pushed to eos from length 4 on, so a minimum length of 7 or
    8 changes what finishes."""
    from flamingo_mini_amd.modeling_flamingo import _beam_finalize
    min_len = max(min_length, L0 + min_new)
    for seed in range(40):
        script = BC.Script(V, seed, eos=EOS, eos_boost=BOOST)
        st, worst = BC.run_restatement(Processed(script, p, g, min_len), PROMPT, NB, MAXLEN, EOS, PAD, True, 1.0)
        if worst >= 1e-3:
            break
    else:
        pytest.fail("no decidable script among 40 seeds")
    want = _beam_finalize(st, L0, PROMPT, NB, PAD)
    ids = torch.from_numpy(PROMPT)
    got = BC.ScriptedModel(script).search(ids, torch.zeros_like(ids), torch.ones_like(ids), None, None, MAXLEN, NB, EOS, PAD, True, 1.0,
                                          processors=(p, g, min_length, min_new))
    assert got.shape == want.shape and torch.equal(got, want), (got.tolist(), want.tolist())
    plain = BC.ScriptedModel(script).search(ids, torch.zeros_like(ids), torch.ones_like(ids), None, None, MAXLEN, NB, EOS, PAD, True, 1.0)
    assert got.shape != plain.shape or not torch.equal(got, plain)
    for row in got.tolist():
        body = row[:row.index(EOS) + 1] if EOS in row[L0:] else row
        if g >= 1:
            grams = list(zip(*[body[k:] for k in range(g)]))
            assert len(set(grams)) == len(grams), (g, row)
        if EOS in row[L0:]:
            assert row.index(EOS) >= min_len, (min_len, row)
