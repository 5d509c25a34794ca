"""Contrastive search without a GPU: the two entry points are bound and reject bad arguments with their error codes before anything reaches
a device; the ctypes mirror of ff_contrastive_desc has the header's fields; generate() rejects what the rules exclude and builds no session;
penalty_alpha=0 hands _static_decode, dynamic_decode and _beam_search exactly the arguments a call without it hands them (monkeypatched
recorders, as the other *_args tests); the routing table for `contrastive_on`; the session-key rule; and the dynamic loop on CPU tensors
with a tiny model equals the numpy restatement (tests/contrastive_cases.py) driven by the loop's own recorded logits and hidden states, stops
at eos and pads."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import contrastive_cases as CC

FF_ERR_SHAPE, FF_ERR_UNSUPPORTED = -1, -2
X = 256                        # a non-null pointer that is never dereferenced: every call below fails its checks first
L0, MAXLEN = 4, 10
PTRS = ("hidden", "hist", "mask", "cand_tok", "cand_logp", "finished", "next_tok", "logprob", "sel_row", "beam_idx", "score")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _step(alpha=X, n_pos=X, null_desc=False, **over):
    from flamingo_mini_amd import ffi
    f = dict(dtype=ffi.DTYPE_BF16, b=2, k=4, dim=64, ld_hidden=64, max_len=16, eos=-1, pad=0, reserved=0, **{n: X for n in PTRS})
    f.update(over)
    d = ffi.ContrastiveDesc(**f)
    return ffi.lib().ff_contrastive_step(None if null_desc else C.byref(d), alpha, n_pos, None)


def _topk(dtype=None, rows=4, vocab=100, ld=100, logits=X, k=4, tok=X, logp=X):
    from flamingo_mini_amd import ffi
    return ffi.lib().ff_topk_logprob(ffi.DTYPE_BF16 if dtype is None else dtype, rows, vocab, ld, logits, k, tok, logp, None)


def test_the_entry_points_are_bound_and_the_abi_is_6():
    from flamingo_mini_amd import decoding as D, ffi, functional as F
    for name in ("ff_topk_logprob", "ff_contrastive_step"):
        assert name in ffi.EXPORTED_SYMBOLS and hasattr(ffi.lib(), name)
    assert ffi.lib().ff_version() == 6 and ffi.CONTRASTIVE_K_MAX == 8
    assert all(callable(f) for f in (F.topk_logprobs, F.contrastive_step, D.topk_logprobs_torch, D.contrastive_select_torch, D.contrastive_search,
                                     D.check_contrastive_args))


def test_the_descriptor_mirror_has_the_headers_fields():
    from flamingo_mini_amd import ffi
    text = open(os.path.join(ROOT, "include", "flamingo_fusion.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert int(re.search(r"#define FF_CONTRASTIVE_K_MAX (\d+)", text).group(1)) == ffi.CONTRASTIVE_K_MAX
    body = re.search(r"struct ff_contrastive_desc \{(.*?)\};", text, flags=re.S).group(1)
    fields, kinds = [], []
    for decl in body.split(";"):
        decl = " ".join(decl.split())
        if decl:
            names = decl.replace("*", " ").split(",")
            these = [names[0].split()[-1]] + [n.strip() for n in names[1:]]
            fields += these
            kinds += [C.c_void_p if "*" in decl else (C.c_longlong if "long long" in decl else C.c_int)] * len(these)
    assert [f[0] for f in ffi.ContrastiveDesc._fields_] == fields
    assert [f[1] for f in ffi.ContrastiveDesc._fields_] == kinds


@pytest.mark.parametrize("bad", [
    dict(null_desc=True), dict(alpha=None), dict(n_pos=None), *[{n: None} for n in PTRS if n != "score"],
    dict(b=0), dict(b=-1), dict(k=0), dict(k=9), dict(dim=0), dict(max_len=0), dict(ld_hidden=63),
], ids=lambda d: "-".join(f"{k}={v}" for k, v in d.items()))
def test_step_argument_errors_return_shape_before_any_launch(bad):
    from flamingo_mini_amd import ffi
    assert _step(**bad) == FF_ERR_SHAPE
    assert b"ff_contrastive_step" in ffi.lib().ff_last_error()


def test_step_unsupported_dtypes_and_sizes():
    from flamingo_mini_amd import ffi
    assert _step(dtype=7) == FF_ERR_UNSUPPORTED and b"ff_contrastive_step" in ffi.lib().ff_last_error()
    assert _step(dtype=ffi.DTYPE_F32, k=8, dim=4097, ld_hidden=4097) == FF_ERR_UNSUPPORTED and b"exceed" in ffi.lib().ff_last_error()
    assert _step(dtype=ffi.DTYPE_BF16, k=8, dim=8193, ld_hidden=8193) == FF_ERR_UNSUPPORTED
    assert _step(dtype=7, k=9) == FF_ERR_SHAPE                                   # the shape checks come first


@pytest.mark.parametrize("bad", [dict(logits=None), dict(tok=None), dict(logp=None), dict(rows=0), dict(vocab=0), dict(ld=99), dict(k=0), dict(k=9),
                                 dict(vocab=3, ld=3)], ids=lambda d: "-".join(f"{k}={v}" for k, v in d.items()))
def test_topk_argument_errors_return_shape_before_any_launch(bad):
    from flamingo_mini_amd import ffi
    assert _topk(**bad) == FF_ERR_SHAPE and b"ff_topk_logprob" in ffi.lib().ff_last_error()
    assert _topk(dtype=7) == FF_ERR_UNSUPPORTED


def test_the_kernels_have_no_cpu_form():
    from flamingo_mini_amd import ffi, functional as F
    with pytest.raises(ffi.FusionLibraryError, match="no CPU fallback"):
        F.topk_logprobs(torch.zeros(2, 20), 3)
    with pytest.raises(ffi.FusionLibraryError, match="no CPU fallback"):
        F.contrastive_step(torch.zeros(4, 8), torch.zeros(2, 6, 8), torch.ones(2, 6, dtype=torch.bool), torch.zeros(2, 2, dtype=torch.long), torch.zeros(2, 2),
                           torch.zeros(2, dtype=torch.bool), torch.zeros(1), torch.zeros(1, dtype=torch.long))


def test_check_contrastive_args():
    from flamingo_mini_amd.decoding import Contrastive, check_contrastive_args as chk
    assert chk(0, 0, False, 1) is None and chk(0.0, 50, True, 4) is None       # off: top_k, do_sample, num_beams are the other paths' business
    got = chk(0.6, 4, False, 1)
    assert got == Contrastive(4, 0.6) and isinstance(got.k, int) and isinstance(got.penalty_alpha, float) and chk(1, 8, False, 1) == (8, 1.0)
    for bad in (-0.1, 1.5, float("inf"), float("-inf"), float("nan"), "0.6", None, True, [0.6]):
        with pytest.raises(ValueError, match="penalty_alpha"):
            chk(bad, 4, False, 1)
    for k in (0, 1, 9, 50, 4.0, True, None):
        with pytest.raises(ValueError, match="top_k"):
            chk(0.6, k, False, 1)
    for kw, match in ((dict(do_sample=True), "do_sample"), (dict(num_beams=3), "beam search"), (dict(num_beam_groups=2), "beam search"),
                      (dict(guidance_scale=1.5), "guidance_scale"), (dict(num_return_sequences=2), "num_return_sequences")):
        args = dict(dict(penalty_alpha=0.6, top_k=4, do_sample=False, num_beams=1), **kw)
        with pytest.raises(ValueError, match=match):
            chk(**args)


@pytest.fixture(scope="module")
def tiny():
    import oracle_backend
    from test_model_plumbing import build
    oracle_backend.install()
    try:
        model, z = build(torch.float32, "cpu", "gpt2")
        model.eval()
        ids, ml = torch.from_numpy(z["ids"])[:, :L0].clone(), torch.from_numpy(z["ml"])[:, :L0]
        yield model, ids, dict(media_locations=ml, attention_mask=torch.ones_like(ids), pixel_values=torch.from_numpy(z["px"]).float(), max_length=MAXLEN)
    finally:
        oracle_backend.uninstall()


@pytest.mark.parametrize("kw,match", [
    (dict(penalty_alpha=-0.1, top_k=4), "penalty_alpha"), (dict(penalty_alpha=1.1, top_k=4), "penalty_alpha"),
    (dict(penalty_alpha=float("nan"), top_k=4), "penalty_alpha"), (dict(penalty_alpha=float("inf"), top_k=4), "penalty_alpha"),
    (dict(penalty_alpha=0.6), "top_k"), (dict(penalty_alpha=0.6, top_k=1), "top_k"), (dict(penalty_alpha=0.6, top_k=9), "top_k"),
    (dict(penalty_alpha=0.6, top_k=4, do_sample=True), "do_sample"), (dict(penalty_alpha=0.6, top_k=4, num_beams=3), "beam search"),
    (dict(penalty_alpha=0.6, top_k=4, num_beams=4, num_beam_groups=2, diversity_penalty=0.5), "beam search"),
    (dict(penalty_alpha=0.6, top_k=4, guidance_scale=1.5), "guidance_scale"),
    (dict(penalty_alpha=0.6, top_k=4, num_return_sequences=2), "num_return_sequences"),
], ids=lambda v: "-".join(f"{k}={x}" for k, x in v.items()) if isinstance(v, dict) else None)
def test_generate_rejects_what_the_rules_exclude(tiny, kw, match):
    model, ids, base = tiny
    for static in (None, True, False):
        with pytest.raises(ValueError, match=match):
            model.generate(ids, static_decode=static, **kw, **base)
    assert len(model._decode_sessions) == 0


def test_routing_table():
    from flamingo_mini_amd import decoding, ffi
    base = dict(model_default=True, lm_family="gpt2", L0=4, max_length=10, ids_is_int64=True, procs_on=False, num_beams=1, do_sample=False)
    r = lambda **k: decoding.route(**base, contrastive_on=True, **k)
    assert r(is_cuda=True, static_decode=None) == "dynamic" and r(is_cuda=True, static_decode=False) == "dynamic"       # static on request only, like beam search
    assert r(is_cuda=True, static_decode=True) == "static"
    assert r(is_cuda=False, static_decode=None) == "dynamic" and r(is_cuda=False, static_decode=False) == "dynamic"
    with pytest.raises(ffi.FusionLibraryError, match="no CPU fallback"):
        r(is_cuda=False, static_decode=True)
    assert decoding.route(**base, is_cuda=True, static_decode=None) == "static"                                         # greedy without it: as ever
    assert decoding.route(**dict(base, lm_family=None), contrastive_on=True, is_cuda=True, static_decode=True) == "dynamic"
    assert decoding.route(**dict(base, L0=9), contrastive_on=True, is_cuda=True, static_decode=True) == "dynamic"
    # the processors' and constraints' static conditions apply as for the other strategies
    assert decoding.route(**dict(base, procs_on=True, ids_is_int64=False), contrastive_on=True, is_cuda=True, static_decode=True) == "dynamic"
    assert decoding.route(**dict(base, procs_on=True), contrastive_on=True, is_cuda=True, static_decode=True) == "static"
    assert decoding.route(**base, contrastive_on=True, constraints_on=True, vocab=ffi.CONSTRAIN_VOCAB_MAX + 1, is_cuda=True, static_decode=True) == "dynamic"
    with pytest.raises(TypeError, match="unsupported generation arguments"):
        decoding.route(**dict(base, procs_on=True), procs_given=["repetition_penalty"], contrastive_on=True, is_cuda=False, static_decode=None)


def _same(a, b):
    if isinstance(a, torch.Tensor) or isinstance(b, torch.Tensor):
        return isinstance(a, torch.Tensor) and isinstance(b, torch.Tensor) and a.dtype == b.dtype and torch.equal(a, b)
    if isinstance(a, (tuple, list)) and type(a) is type(b):
        return len(a) == len(b) and all(_same(x, y) for x, y in zip(a, b))
    if isinstance(a, dict) and isinstance(b, dict):
        return list(a) == list(b) and all(_same(a[k], b[k]) for k in a)
    if type(a).__name__ == "Constraints":
        return type(a) is type(b) and a.caps() == b.caps()
    return type(a) is type(b) and a == b


MODES = [dict(), dict(top_k=5), dict(do_sample=True, temperature=0.7, top_k=5), dict(num_beams=3), dict(eos_token_id=5, bad_words_ids=[[3]]),
         dict(return_dict_in_generate=True, output_logprobs=True)]


@pytest.mark.parametrize("mode", MODES, ids=lambda d: "-".join(d) or "greedy")
@pytest.mark.parametrize("static", [None, True, False])
def test_alpha_zero_passes_exactly_the_arguments_of_a_call_without_it(tiny, monkeypatch, mode, static):
    from flamingo_mini_amd import decoding as D, ffi
    model, ids, kw = tiny
    seen = []
    rec = lambda name: (lambda *a, **k: (seen.append((name, a, k)), (ids, torch.zeros(ids.shape[0], 0)))[1])
    monkeypatch.setattr(D, "_static_decode", rec("static"))
    monkeypatch.setattr(D, "dynamic_decode", rec("dynamic"))
    monkeypatch.setattr(D, "contrastive_search", rec("contrastive"))
    monkeypatch.setattr(type(model), "_beam_search", rec("beams"))
    monkeypatch.setattr(D, "route", (lambda orig: lambda **k: (seen.append(("route", (), k)), orig(**k))[1])(D.route))
    calls = []
    for extra in ({}, dict(penalty_alpha=0.0), dict(penalty_alpha=0)):
        seen.clear()
        try:
            model.generate(ids, static_decode=static, **mode, **extra, **kw)
        except ffi.FusionLibraryError:                                        # (static_decode=True on CPU tensors where a mode needs the GPU)
            seen.append(("raised", (), {}))
        calls.append(list(seen))
    assert len(calls[0]) == 2 and calls[0][0][0] == "route" and calls[0][1][0] != "contrastive"
    for other in calls[1:]:
        assert [c[0] for c in other] == [c[0] for c in calls[0]]
        for (_, a0, k0), (_, a1, k1) in zip(calls[0], other):
            assert _same(a0, a1) and _same(k0, k1), (k0.keys(), k1.keys())
    for _, a, k in calls[0]:
        assert not {"contrastive", "contrastive_on", "penalty_alpha"} & set(k), k.keys()


def test_alpha_on_hands_the_paths_the_contrastive(tiny, monkeypatch):
    from flamingo_mini_amd import decoding as D
    model, ids, kw = tiny
    seen = []
    rec = lambda name: (lambda *a, **k: (seen.append((name, a, k)), ids)[1])
    monkeypatch.setattr(D, "_static_decode", rec("static"))
    monkeypatch.setattr(D, "contrastive_search", rec("contrastive"))
    monkeypatch.setattr(D, "dynamic_decode", rec("dynamic"))
    monkeypatch.setattr(D, "route", lambda **k: (seen.append(("route", (), k)), "static" if k["static_decode"] else "dynamic")[1])
    model.generate(ids, penalty_alpha=0.6, top_k=4, eos_token_id=5, **kw)
    model.generate(ids, penalty_alpha=0.6, top_k=4, static_decode=True, eos_token_id=5, bad_words_ids=[[3]], **kw)
    (_, _, r0), (n0, a0, k0), (_, _, r1), (n1, a1, k1) = seen
    assert r0["contrastive_on"] is True and r1["contrastive_on"] is True and r0["do_sample"] is False and r0["num_beams"] == 1
    assert n0 == "contrastive" and a0[0] == model._contrastive_step and a0[1] == model._reorder_cache and a0[8] == D.Contrastive(4, 0.6) and a0[9:11] == (5, 5)
    assert n1 == "static" and k1["contrastive"] == D.Contrastive(4, 0.6) and k1["constraints"].bad_words.words == [(3,)] and "sampling" not in k1


def test_the_session_key_ends_with_k_not_alpha(tiny, monkeypatch):
    """_static_decode builds the key it always built without a Contrastive, and one that ends with ("contrastive", k) with it - whatever alpha"""
    from flamingo_mini_amd import decoding as D
    model, ids, kw = tiny
    made = []

    class Fake:
        def __init__(self, *a, **k):
            made.append((a, k))

        def stale(self):
            return False

        def run(self, *a, **k):
            made.append(("run", k))
            return ids

    monkeypatch.setattr(D, "_ContrastiveSession", Fake)
    monkeypatch.setattr(D, "_TokenSession", Fake)
    try:
        args = (model, ids, kw["media_locations"], kw["attention_mask"], kw["pixel_values"], None, MAXLEN, 5, 7)
        D._static_decode(*args)
        D._static_decode(*args, contrastive=D.Contrastive(4, 0.6))
        D._static_decode(*args, contrastive=D.Contrastive(4, 0.3))
        D._static_decode(*args, contrastive=D.Contrastive(3, 0.6))
        keys = list(D._DECODE_SESSIONS[model])
        plain = (ids.shape[0], MAXLEN, kw["pixel_values"].shape[1], "cpu", 5, 7, False, None, None, None)
        assert keys == [plain, plain + (("contrastive", 4),), plain + (("contrastive", 3),)]
        runs = [m[1] for m in made if m[0] == "run"]
        assert "penalty_alpha" not in runs[0] and [r["penalty_alpha"] for r in runs[1:]] == [0.6, 0.3, 0.6]
        built = [m for m in made if m[0] != "run"]
        assert len(built) == 3 and "contrastive" not in built[0][1] and built[1][1]["contrastive"].k == 4 and built[2][1]["contrastive"].k == 3
    finally:
        model.reset_decode_sessions()


def _replay(trace, ids, L0_, alpha, k, eos, pad):
    """the numpy restatement driven by the loop's recorded logits and hidden states: the tokens it chooses, step by step"""
    out, und = [], 0
    for t, rec in enumerate(trace):
        n = L0_ + t
        tok, logp = CC.topk_logprobs(rec["x"].double().numpy(), k)
        assert np.array_equal(tok, rec["cand_tok"].numpy())
        assert np.abs(logp - rec["cand_logp"].double().numpy()).max() < 1e-5
        hist = rec["hist"].double().numpy()
        assert hist.shape[1] == n
        ref = CC.select(rec["hidden"].double().numpy(), hist, rec["mask"].numpy(), n, tok, rec["cand_logp"].double().numpy(), rec["finished"].numpy(), alpha,
                        -1 if eos is None else eos, pad)
        ok = ref["margin"] >= 1e-4                                              # float32 model, float64 restatement: far inside the margin
        und += int((~ok).sum())
        assert np.array_equal(rec["sel_row"].numpy()[ok], ref["sel_row"][ok]) and np.array_equal(rec["next_tok"].numpy()[ok], ref["next_tok"][ok])
        assert np.allclose(rec["logprob"].double().numpy()[ok], ref["logprob"][ok], atol=1e-5)
        if t + 1 < len(trace):                                                  # rule C7: H[s, n] <- h_c*
            nxt_hist = trace[t + 1]["hist"]
            assert torch.equal(nxt_hist[:, n], rec["hidden"][rec["sel_row"]]) and torch.equal(nxt_hist[:, :n], rec["hist"])
        out.append(rec["next_tok"])
    return torch.stack(out, 1), und


def test_the_dynamic_loop_on_cpu_tensors_equals_the_restatement(tiny):
    from flamingo_mini_amd import decoding as D
    model, ids, kw = tiny
    out = model.generate(ids, penalty_alpha=0.6, top_k=4, **kw)
    assert out.shape == (ids.shape[0], MAXLEN) and torch.equal(out[:, :L0], ids) and len(model._decode_sessions) == 0
    assert torch.equal(out, model.generate(ids, penalty_alpha=0.6, top_k=4, static_decode=False, **kw))
    trace = []
    am = kw["attention_mask"].clone()
    am[1, 0] = 0                                                                # a left-padded row: its first position never enters the penalty
    with torch.no_grad():
        res = D.contrastive_search(model._contrastive_step, model._reorder_cache, ids, kw["media_locations"], am, kw["pixel_values"], None, MAXLEN,
                                   D.Contrastive(4, 0.6), None, None, trace=trace)
    assert len(trace) == MAXLEN - L0 and not bool(trace[3]["mask"][1, 0]) and bool(trace[3]["mask"][0, 0])
    gen, und = _replay(trace, ids, L0, 0.6, 4, None, 0)
    assert torch.equal(gen, res[:, L0:]) and und <= 1
    with pytest.raises(Exception, match="no CPU fallback"):
        model.generate(ids, penalty_alpha=0.6, top_k=4, static_decode=True, **kw)


def test_the_dynamic_loop_stops_at_eos_pads_and_reports_logprobs(tiny):
    model, ids, kw = tiny
    base = model.generate(ids, penalty_alpha=0.6, top_k=4, **kw)
    eos = int(base[0, L0 + 1])                                                  # row 0 ends after two tokens
    out = model.generate(ids, penalty_alpha=0.6, top_k=4, eos_token_id=eos, pad_token_id=1, return_dict_in_generate=True, output_logprobs=True, **kw)
    seq, lps = out.sequences, out.token_logprobs
    assert lps.shape == (ids.shape[0], seq.shape[1] - L0) and lps.dtype == torch.float32 and out.sequences_scores.shape == (ids.shape[0],)
    for r in range(ids.shape[0]):
        g = seq[r, L0:].tolist()
        if eos in g:
            e = g.index(eos)
            assert g[:e + 1] == base[r, L0:L0 + e + 1].tolist() and all(t == 1 for t in g[e + 1:])
            assert bool((lps[r, e + 1:] == 0).all()) and bool((lps[r, :e + 1] < 0).all())
        else:
            assert g == base[r, L0:L0 + len(g)].tolist()
    assert eos in seq[0, L0:].tolist()
    if all(eos in seq[r, L0:].tolist() for r in range(ids.shape[0])):           # every row ended: the loop stopped there
        assert seq.shape[1] == L0 + 1 + max(seq[r, L0:].tolist().index(eos) for r in range(ids.shape[0]))
    banned = model.generate(ids, penalty_alpha=0.6, top_k=4, bad_words_ids=[[int(t)] for t in base[:, L0].tolist()], **kw)
    assert not set(banned[:, L0:].reshape(-1).tolist()) & set(base[:, L0].tolist())
