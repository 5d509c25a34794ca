"""Beam sampling without a GPU: the three entry points are bound, their ctypes signatures are the header's, they reject bad arguments with
their error codes before anything reaches a device; generate(num_beams > 1, do_sample=True) runs the dynamic loop on CPU tensors,
reproducibly per generator seed; the combinations the rules exclude keep their ValueErrors; and decoding.route(beam_sample_on=True) follows
beam search's rule on the cross product of tests/test_decode_routing.py's inputs."""
import ctypes as C

import pytest
import torch

FF_ERR_SHAPE, FF_ERR_UNSUPPORTED = -1, -2
X = 256                        # a non-null pointer that is never dereferenced: every call below fails its checks first
STATE = ("score", "done", "n_hyp", "hyp_score", "hyp_len", "hyp_row", "hist_tok", "hist_parent", "hist_score", "next_tok", "beam_idx", "len_norm")


def _step(logits=X, cur_len=X, ws=X, ws_bytes=1 << 20, null_desc=False, temperature=0.9, top_k=40, top_p=0.95, seed=X, **over):
    from flamingo_mini_amd import ffi
    f = dict(dtype=ffi.DTYPE_BF16, b=2, nb=4, vocab=100, ld=100, max_len=16, eos=-1, pad=0, early_stopping=1, **{n: X for n in STATE})
    f.update(over)
    d = ffi.BeamDesc(**f)
    return ffi.lib().ff_beam_sample_step(None if null_desc else C.byref(d), temperature, top_k, top_p, seed, logits, cur_len, ws, ws_bytes, None)


def test_the_entry_points_are_bound_and_the_abi_is_6():
    from flamingo_mini_amd import ffi, functional as F
    for name in ("ff_beam_sample_workspace_bytes", "ff_beam_sample_step", "ff_beam_sample_noise"):
        assert name in ffi.EXPORTED_SYMBOLS and hasattr(ffi.lib(), name)
    assert ffi.lib().ff_version() == 6 and callable(F.beam_sample_step) and callable(F.beam_sample_noise)
    ws = ffi.lib().ff_beam_sample_workspace_bytes
    assert ws(2, 4) == 2 * 4 * 8 * 12 and ws(32, 8) == 32 * 8 * 16 * 12 and ws(0, 4) == ws(2, 0) == ws(2, 9) == 0
    assert ws(2, 4) > ffi.lib().ff_beam_workspace_bytes(2, 4)                  # (p, a, column) against (score, column)


def test_ctypes_signatures_match_the_header():
    """ff_beam_step's arguments with (float temperature, int top_k, float top_p, const long long* seed) behind the descriptor"""
    from flamingo_mini_amd import ffi
    from test_cabi import _header_prototypes
    protos = _header_prototypes()
    plain = protos["ff_beam_step"][1]
    assert protos["ff_beam_sample_step"] == ("int", plain[:1] + ["float", "int", "float", "ptr"] + plain[1:])
    assert protos["ff_beam_sample_workspace_bytes"] == protos["ff_beam_workspace_bytes"]
    assert protos["ff_beam_sample_noise"] == ("int", ["int", "int", "ptr", "ptr", "ptr", "ptr"])
    want = ffi._SIGNATURES["ff_beam_step"][1]
    assert ffi._SIGNATURES["ff_beam_sample_step"] == (C.c_int, want[:1] + [C.c_float, C.c_int, C.c_float, C.c_void_p] + want[1:])
    assert ffi._SIGNATURES["ff_beam_sample_workspace_bytes"] == ffi._SIGNATURES["ff_beam_workspace_bytes"]
    assert ffi._SIGNATURES["ff_beam_sample_noise"] == (C.c_int, [C.c_int, C.c_int] + [C.c_void_p] * 4)


@pytest.mark.parametrize("bad", [
    dict(null_desc=True), dict(logits=None), dict(cur_len=None), dict(ws=None), dict(seed=None), *[{n: None} for n in STATE],
    dict(b=0), dict(b=-1), dict(nb=0), dict(nb=9), dict(vocab=7), dict(ld=99), dict(max_len=0), dict(ws_bytes=2 * 4 * 8 * 12 - 1),
    dict(temperature=0.0), dict(temperature=-1.0), dict(temperature=float("inf")), dict(temperature=float("nan")),
    dict(top_k=-1), dict(top_p=0.0), dict(top_p=1.5), dict(top_p=-0.1), dict(top_p=float("nan")),
], ids=lambda d: "-".join(f"{k}={v}" for k, v in d.items()))
def test_argument_errors_return_shape_before_any_launch(bad):
    from flamingo_mini_amd import ffi
    assert _step(**bad) == FF_ERR_SHAPE
    assert b"ff_beam_sample_step" in ffi.lib().ff_last_error()


def test_other_dtypes_are_unsupported_and_the_noise_checks_its_arguments():
    from flamingo_mini_amd import ffi
    assert _step(dtype=7) == FF_ERR_UNSUPPORTED and b"ff_beam_sample_step" in ffi.lib().ff_last_error()
    noise = ffi.lib().ff_beam_sample_noise
    for args in ((0, 8, X, X, X), (65536, 8, X, X, X), (4, 0, X, X, X), (4, 8, None, X, X), (4, 8, X, None, X), (4, 8, X, X, None)):
        assert noise(*args, None) == FF_ERR_SHAPE and b"ff_beam_sample_noise" in ffi.lib().ff_last_error()


def test_the_kernels_have_no_cpu_form():
    from flamingo_mini_amd import ffi, functional as F
    one = torch.zeros(1, dtype=torch.long)
    with pytest.raises(ffi.FusionLibraryError, match="no CPU fallback"):
        F.beam_sample_step(torch.zeros(8, 20), None, one, one)
    with pytest.raises(ffi.FusionLibraryError, match="no CPU fallback"):
        F.beam_sample_noise(4, 8, one, one)


@pytest.fixture(scope="module")
def cpu_model():
    import oracle_backend
    from test_model_plumbing import build
    oracle_backend.install()
    try:
        model, z = build(torch.float64, "cpu", "gpt2")
        model.eval()
        ids, ml = torch.from_numpy(z["ids"])[:, :4], torch.from_numpy(z["ml"])[:, :4]
        yield model, ids, dict(media_locations=ml, attention_mask=torch.ones_like(ids), pixel_values=torch.from_numpy(z["px"]).double(), max_length=8)
    finally:
        oracle_backend.uninstall()


def test_generate_on_cpu_tensors_is_reproducible_per_seed(cpu_model):
    """num_beams=3, do_sample=True runs the dynamic loop: the same generator seed gives the same sequences, another seed others; rows s * n + j
    carry sorted scores; static_decode=True raises what ffi.require_cuda raises and builds no session."""
    from flamingo_mini_amd import ffi
    model, ids, base = cpu_model
    kw = dict(base, num_beams=3, do_sample=True, temperature=1.3, top_k=50)
    gen = lambda s: torch.Generator().manual_seed(s)
    with pytest.raises(ffi.FusionLibraryError, match="no CPU fallback"):
        model.generate(ids, static_decode=True, **kw)
    assert len(model._decode_sessions) == 0
    a = model.generate(ids, generator=gen(1), **kw)
    b, L0 = ids.shape
    assert a.shape[0] == b and torch.equal(a[:, :L0], ids)
    assert torch.equal(a, model.generate(ids, generator=gen(1), **kw))
    runs = [model.generate(ids, generator=gen(s), **kw) for s in (2, 3, 4)]
    assert any(r.shape != a.shape or not torch.equal(r, a) for r in runs)
    out = model.generate(ids, generator=gen(1), num_return_sequences=3, return_dict_in_generate=True, **kw)
    assert out.sequences.shape[0] == 3 * b and torch.equal(out.sequences[:, :L0], ids.repeat_interleave(3, 0))
    s = out.sequences_scores.reshape(b, 3)
    assert bool(torch.isfinite(s).all()) and bool((s[:, :-1] >= s[:, 1:]).all())
    assert torch.equal(out.sequences[::3], a)
    assert all(len({tuple(r) for r in out.sequences[i * 3:(i + 1) * 3].tolist()}) == 3 for i in range(b)), "a draw without replacement returns distinct beams"
    assert len(model._decode_sessions) == 0


@pytest.mark.parametrize("kw,match", [
    (dict(num_beam_groups=3), "num_beam_groups > 1 cannot be combined with do_sample"),
    (dict(min_p=0.1), "not offered with beam search"), (dict(typical_p=0.9), "not offered with beam search"),
    (dict(epsilon_cutoff=0.01), "not offered with beam search"), (dict(eta_cutoff=0.01), "not offered with beam search"),
    (dict(return_dict_in_generate=True, output_logprobs=True), "output_logprobs=True is not offered with beam search"),
    (dict(temperature=0.0), "temperature"), (dict(top_p=0.0), "top_p"), (dict(top_k=-1), "top_k"), (dict(num_return_sequences=4), "exceeds num_beams"),
], ids=lambda v: "-".join(f"{k}={x}" for k, x in v.items()) if isinstance(v, dict) else None)
def test_generate_keeps_the_errors_of_what_beam_sampling_does_not_offer(cpu_model, kw, match):
    model, ids, base = cpu_model
    with pytest.raises(ValueError, match=match):
        model.generate(ids, **base, num_beams=3, do_sample=True, **kw)


def test_route_with_beam_sample_on_follows_beam_search():
    """On the cross product of tests/test_decode_routing.py's inputs with num_beams > 1: do_sample=True keeps raising, and do_sample=False
    with beam_sample_on=True returns or raises exactly what the same call without the keyword does - beam search's rule."""
    from test_decode_routing import CASES, expected
    from flamingo_mini_amd import decoding, ffi
    given = ["repetition_penalty", "min_length"]
    n = 0
    for kw in CASES:
        if kw["num_beams"] <= 1:
            continue
        if kw["do_sample"]:
            if not (kw["procs_on"] and not kw["is_cuda"]):                   # (the processors' TypeError on CPU tensors comes first)
                with pytest.raises(ValueError, match="beam search with sampling"):
                    decoding.route(**kw, procs_given=given, beam_sample_on=True)
            continue
        want = expected(**kw)
        n += 1
        if isinstance(want, str) and want != "CPU":
            assert decoding.route(**kw, procs_given=given, beam_sample_on=True) == want == decoding.route(**kw, procs_given=given), kw
            continue
        with pytest.raises(ffi.FusionLibraryError if want == "CPU" else want):
            decoding.route(**kw, procs_given=given, beam_sample_on=True)
    assert n == 2 * 2 * 3 * 2 * 2 * 3 * 2 * 2
    import inspect
    p = inspect.signature(decoding.route).parameters["beam_sample_on"]
    assert p.kind is p.KEYWORD_ONLY and p.default is False


def test_the_session_key_and_the_calls_without_sampling_are_what_they_were(monkeypatch):
    """generate(num_beams=3) without do_sample hands the dynamic loop no sampling= / generator= keyword, and with do_sample it hands both"""
    from flamingo_mini_amd import decoding
    seen = []
    monkeypatch.setattr(decoding, "beam_search", lambda *a, **kw: seen.append(kw) or torch.zeros((2, 8), dtype=torch.long))
    import oracle_backend
    from test_model_plumbing import build
    oracle_backend.install()
    try:
        model, z = build(torch.float64, "cpu", "gpt2")
        ids, ml = torch.from_numpy(z["ids"])[:, :4], torch.from_numpy(z["ml"])[:, :4]
        base = dict(media_locations=ml, attention_mask=torch.ones_like(ids), pixel_values=torch.from_numpy(z["px"]).double(), max_length=8, num_beams=3)
        model.generate(ids, **base)
        g = torch.Generator().manual_seed(0)
        model.generate(ids, **base, do_sample=True, temperature=0.7, top_k=9, top_p=0.5, generator=g)
    finally:
        oracle_backend.uninstall()
    assert "sampling" not in seen[0] and "generator" not in seen[0]
    assert seen[1]["sampling"] == decoding.Sampling(0.7, 9, 0.5) and seen[1]["generator"] is g
