"""Constrained decoding without a GPU: ff_logits_constrain is bound and rejects bad arguments with its error codes before anything reaches a
device, the call with both tables absent returns success without touching its pointers, functional.constrain_logits has no CPU form,
generate() rejects bad values, the routing on the host (decoding.route), and a call with both arguments None never reaches
functional.constrain_logits."""
import ctypes as C

import pytest
import torch

FF_OK, FF_ERR_SHAPE, FF_ERR_UNSUPPORTED = 0, -1, -2
X = C.c_void_p(256)            # a non-null pointer that is never dereferenced: every call below returns before any launch
TRIE = dict(node_first=X, edge_tok=X, edge_child=X, node_terminal=X, n_nodes=X)
WORDS = dict(bw_off=X, bw_tok=X, n_bw=X)
NO_TRIE, NO_WORDS = dict.fromkeys(TRIE), dict.fromkeys(WORDS)


def _call(dtype=None, rows=4, vocab=100, ld=100, logits=X, hist=X, hist_ld=16, hist_cap=16, hist_len=X, gen_start=X, eos=5, node_cap=8, edge_cap=8, bw_cap=4,
          bw_tok_cap=8, **tables):
    from flamingo_mini_amd import ffi
    t = dict(TRIE, **WORDS)
    t.update(tables)
    return ffi.lib().ff_logits_constrain(ffi.DTYPE_BF16 if dtype is None else dtype, rows, vocab, ld, logits, hist, hist_ld, hist_cap, hist_len, gen_start, eos,
                                         t["node_first"], t["edge_tok"], t["edge_child"], t["node_terminal"], t["n_nodes"], node_cap, edge_cap,
                                         t["bw_off"], t["bw_tok"], t["n_bw"], bw_cap, bw_tok_cap, None)


def test_the_entry_point_is_bound():
    from flamingo_mini_amd import ffi, functional as F
    assert "ff_logits_constrain" in ffi.EXPORTED_SYMBOLS and ffi.lib().ff_version() == 6
    assert callable(F.constrain_logits) and ffi.CONSTRAIN_VOCAB_MAX == 262144


@pytest.mark.parametrize("bad", [
    dict(logits=None), dict(hist=None), dict(hist_len=None), dict(gen_start=None),
    dict(node_first=None), dict(edge_tok=None), dict(edge_child=None), dict(node_terminal=None), dict(n_nodes=None),      # half-given tables
    dict(bw_off=None), dict(bw_tok=None), dict(n_bw=None), dict(NO_TRIE, edge_child=X), dict(NO_WORDS, n_bw=X),
    dict(rows=0), dict(rows=-3), dict(vocab=0), dict(vocab=-1), dict(ld=99), dict(hist_cap=0), dict(hist_cap=-1), dict(hist_ld=15),
    dict(node_cap=0), dict(edge_cap=0), dict(edge_cap=-5), dict(bw_cap=0), dict(bw_tok_cap=-1),
    dict(eos=-1), dict(eos=-2), dict(eos=100), dict(eos=1 << 20),                     # a trie needs eos inside the vocabulary
    dict(NO_TRIE, eos=-2), dict(NO_TRIE, eos=100),                                    # without one -1 stands for none
], ids=lambda d: "-".join(f"{k}={'X' if v is X else v}" for k, v in d.items()))
def test_argument_errors_return_shape_before_any_launch(bad):
    from flamingo_mini_amd import ffi
    assert _call(**bad) == FF_ERR_SHAPE
    assert b"ff_logits_constrain" in ffi.lib().ff_last_error()


def test_other_dtypes_longer_histories_and_larger_vocabularies_are_unsupported():
    from flamingo_mini_amd import ffi
    assert _call(dtype=7) == FF_ERR_UNSUPPORTED
    assert b"ff_logits_constrain" in ffi.lib().ff_last_error() and b"dtype" in ffi.lib().ff_last_error()
    assert _call(hist_cap=4097, hist_ld=4097) == FF_ERR_UNSUPPORTED
    assert b"FF_LOGITS_HIST_MAX" in ffi.lib().ff_last_error()
    assert _call(vocab=262145, ld=262145) == FF_ERR_UNSUPPORTED
    assert b"FF_CONSTRAIN_VOCAB_MAX" in ffi.lib().ff_last_error()
    assert _call(vocab=262145, ld=262145, **NO_TRIE) == FF_ERR_UNSUPPORTED          # one cap for both tables


def test_both_tables_absent_returns_success_and_launches_nothing():
    """(the pointers are not memory: a launch, or any read of *hist_len, would fault or fail)"""
    off = dict(NO_TRIE, **NO_WORDS)
    assert _call(**off) == FF_OK
    assert _call(eos=-1, node_cap=0, edge_cap=0, bw_cap=0, bw_tok_cap=0, hist_cap=4096, hist_ld=4096, **off) == FF_OK      # the capacities of absent tables are not looked at
    assert _call(**dict(off, rows=0)) == FF_ERR_SHAPE                         # the checks still come first
    assert _call(**dict(off, gen_start=None)) == FF_ERR_SHAPE


def test_constrain_logits_has_no_cpu_form():
    from flamingo_mini_amd import ffi, functional as F
    one = torch.zeros(1, dtype=torch.long)
    i32 = lambda n: torch.zeros(n, dtype=torch.int32)
    with pytest.raises(ffi.FusionLibraryError, match="no CPU fallback"):
        F.constrain_logits(torch.zeros(2, 5), torch.zeros(2, 4, dtype=torch.long), one, one, eos=1, bad_words=(i32(3), i32(4), i32(1)))


# ---- generate() on the host -----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def tiny():
    import oracle_backend
    from test_model_plumbing import build
    oracle_backend.install()
    try:
        model, z = build(torch.float64, "cpu", "gpt2")
        model.eval()
        px = torch.from_numpy(z["px"]).double()
        ids, ml = torch.from_numpy(z["ids"])[:, :4], torch.from_numpy(z["ml"])[:, :4]
        yield model, ids, dict(media_locations=ml, attention_mask=torch.ones_like(ids), pixel_values=px, max_length=10)
    finally:
        oracle_backend.uninstall()


@pytest.mark.parametrize("bad", [
    dict(candidate_ids=[[5, 6]]),                                             # needs eos_token_id
    dict(candidate_ids=[], eos_token_id=3), dict(candidate_ids=[[]], eos_token_id=3), dict(candidate_ids=[[5], []], eos_token_id=3),
    dict(candidate_ids=[[97]], eos_token_id=3), dict(candidate_ids=[[-1]], eos_token_id=3), dict(candidate_ids=[[5, 3]], eos_token_id=3),
    dict(candidate_ids=[5, 6], eos_token_id=3), dict(candidate_ids="ab", eos_token_id=3),
    dict(candidate_ids=[[5]], eos_token_id=3, min_length=6), dict(candidate_ids=[[5]], eos_token_id=3, min_new_tokens=1),
    dict(candidate_ids=[[5], [1, 2, 4, 5, 6, 7]], eos_token_id=3),        # 4 + 6 + 1 > max_length 10
    dict(bad_words_ids=[]), dict(bad_words_ids=[[]]), dict(bad_words_ids=[[97]]), dict(bad_words_ids=[[-1, 2]]), dict(bad_words_ids=[7]),
], ids=lambda d: "-".join(f"{k}={v}" for k, v in d.items()))
def test_generate_rejects_bad_values(tiny, bad):
    model, ids, kw = tiny
    for mode in (dict(), dict(num_beams=2), dict(do_sample=True)):
        with pytest.raises(ValueError):
            model.generate(ids, **bad, **mode, **kw)
    assert len(model._decode_sessions) == 0


def test_the_longest_candidate_that_fits_is_accepted(tiny):
    model, ids, kw = tiny
    out = model.generate(ids, candidate_ids=[[5, 6, 7, 8, 9]], eos_token_id=3, pad_token_id=0, **kw)      # 4 + 5 + 1 == max_length
    assert out[:, 4:].tolist() == [[5, 6, 7, 8, 9, 3]] * 2


def test_static_decode_on_cpu_tensors_raises_and_builds_no_session(tiny):
    from flamingo_mini_amd import ffi
    model, ids, kw = tiny
    for mode in (dict(), dict(do_sample=True), dict(num_beams=3)):
        for cons in (dict(candidate_ids=[[5, 6]]), dict(bad_words_ids=[[5]])):
            with pytest.raises(ffi.FusionLibraryError, match="no CPU fallback"):
                model.generate(ids, static_decode=True, eos_token_id=3, **cons, **mode, **kw)
    assert len(model._decode_sessions) == 0


def test_a_call_without_constraints_never_reaches_constrain_logits(tiny, monkeypatch):
    """greedy static decoding runs on the host too (the oracle backend): with both arguments None the session has constraints None, its key
    is what it was (it ends with the processors), it owns no table buffer, and neither functional.constrain_logits nor the torch
    restatement is called - on the static and on the dynamic paths"""
    from flamingo_mini_amd import decoding as D, functional as F

    def boom(*a, **k):
        raise AssertionError("constrain_logits reached without constraints")
    monkeypatch.setattr(F, "constrain_logits", boom)
    monkeypatch.setattr(D, "constrain_logits_torch", boom)
    model, ids, kw = tiny
    try:
        out = model.generate(ids, static_decode=True, candidate_ids=None, bad_words_ids=None, **kw)
        assert torch.equal(out, model.generate(ids, static_decode=False, **kw))
        (key, sess), = model._decode_sessions.items()
        assert sess.constraints is None and key[-1] is None and len(key) == 10
        assert not any(hasattr(sess, a) for a in ("gen_start", "trie_bufs", "bw_bufs", "seq_buf"))
        model.generate(ids, do_sample=True, **kw)
        model.generate(ids, num_beams=3, **kw)
    finally:
        model.reset_decode_sessions()


# ---- routing ----------------------------------------------------------------------------------------------------------------------------
def test_routing():
    from flamingo_mini_amd import decoding as D, ffi
    base = dict(num_beams=1, do_sample=False, static_decode=None, model_default=True, lm_family="gpt2", L0=4, max_length=20, ids_is_int64=True, procs_on=False)
    on = dict(constraints_on=True, vocab=50258, table_entries=1024)
    assert D.route(is_cuda=True, **base) == D.route(is_cuda=True, **base, **on) == "static"
    assert D.route(is_cuda=False, **base, **on) == "dynamic"                                  # CPU tensors: the dynamic loop, no TypeError
    for mode in (dict(do_sample=True), dict(num_beams=3)):
        assert D.route(is_cuda=False, **dict(base, **mode), **on) == "dynamic"
        assert D.route(is_cuda=True, **dict(base, **mode), **on) == "dynamic"                 # sampling and beams: static on request only
        assert D.route(is_cuda=True, **dict(base, static_decode=True, **mode), **on) == "static"
    with pytest.raises(ffi.FusionLibraryError, match="no CPU fallback"):
        D.route(is_cuda=False, **dict(base, static_decode=True), **on)
    assert D.route(is_cuda=False, **dict(base, static_decode=True)) == "static"               # (what greedy decoding on the host always could)
    assert D.route(is_cuda=True, **dict(base, max_length=4097), **on) == "dynamic"            # the history cap of the kernel
    assert D.route(is_cuda=True, **dict(base, max_length=4096), **on) == "static"
    assert D.route(is_cuda=True, **dict(base, max_length=4097)) == "static"                   # ... binds only with constraints (or processors)
    assert D.route(is_cuda=True, **dict(base, ids_is_int64=False), **on) == "dynamic"
    assert D.route(is_cuda=True, **base, **dict(on, vocab=ffi.CONSTRAIN_VOCAB_MAX + 1)) == "dynamic"
    assert D.route(is_cuda=True, **base, **dict(on, vocab=ffi.CONSTRAIN_VOCAB_MAX)) == "static"
    assert D.route(is_cuda=True, **base, **dict(on, table_entries=D.CONSTRAINT_TABLE_MAX * 2)) == "dynamic"
    assert D.route(is_cuda=True, **dict(base, static_decode=False), **on) == "dynamic"


def test_generate_with_a_long_max_length_takes_the_dynamic_loop(tiny, monkeypatch):
    """max_length > 4096 with constraints: route() is asked with the constraint facts and answers "dynamic" even for GPU tensors"""
    from flamingo_mini_amd import decoding as D
    model, ids, kw = tiny
    seen = []
    real = D.route

    def spy(**k):
        seen.append((k, real(**dict(k, is_cuda=True))))
        return real(**k)
    monkeypatch.setattr(D, "route", spy)
    out = model.generate(ids, candidate_ids=[[5, 6]], eos_token_id=3, pad_token_id=0, **dict(kw, max_length=5000))
    assert out[:, 4:].tolist() == [[5, 6, 3]] * 2
    model.generate(ids, candidate_ids=[[5, 6]], eos_token_id=3, pad_token_id=0, **kw)
    model.generate(ids, **kw)
    (k0, r0), (k1, r1), (k2, r2) = seen
    assert k0["constraints_on"] and k0["vocab"] == 97 and k0["table_entries"] == 64 and k0["max_length"] == 5000 and r0 == "dynamic"
    assert k1["constraints_on"] and r1 == "static"
    assert "constraints_on" not in k2 and r2 == "static"


def test_generate_captions_tokenises_the_strings_verbatim(monkeypatch):
    from flamingo_mini_amd.modeling_flamingo import FlamingoModel

    class Tok:
        def __call__(self, s, add_special_tokens=True):
            assert add_special_tokens is False
            return {"input_ids": [ord(c) for c in s]}

        def batch_decode(self, ids, skip_special_tokens=True):
            return ["x"] * len(ids)

    class Proc:
        tokenizer = Tok()
        remove_tags = staticmethod(lambda t: t)

        def encode_text(self, prompt, device):
            one = torch.ones((1, 2), dtype=torch.long)
            return one, one.bool(), one

    class Cfg:
        bos_token_id, eos_token_id = 1, 2

    class Stub:
        device = "cpu"
        flamingo = type("F", (), {"lm": type("L", (), {"config": Cfg})})

        def generate(self, **kw):
            self.kw = kw
            return torch.zeros((3, 4), dtype=torch.long)

    stub = Stub()
    FlamingoModel.generate_captions.__wrapped__(stub, Proc(), pixel_values=torch.zeros(3, 3, 2, 2), candidates=[" a", "bc"], bad_words=["d"])
    assert stub.kw["candidate_ids"] == [[32, 97], [98, 99]] and stub.kw["bad_words_ids"] == [[100]]
    FlamingoModel.generate_captions.__wrapped__(stub, Proc(), pixel_values=torch.zeros(3, 3, 2, 2))
    assert "candidate_ids" not in stub.kw and "bad_words_ids" not in stub.kw
    with pytest.raises(ValueError):
        FlamingoModel.generate_captions.__wrapped__(stub, Proc(), pixel_values=torch.zeros(3, 3, 2, 2), candidates="cat")


def test_the_unit_is_reported_with_two_instantiations_and_no_scratch():
    """csrc/ff_constrain.hip sits inside every replayed step of a constrained session: both instantiations (bf16, fp32) are in the
    compiler's resource remarks, neither spills, both keep 8 waves per SIMD, and their names stay clear of the kernels other resource
    tests count by name"""
    import os
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
    import kernel_resources
    rows = kernel_resources.load()
    if not rows:
        pytest.skip("library not built in this tree (no csrc/_obj/*.resources.txt)")
    mine = [r for r in rows if r["unit"] == "ff_constrain"]
    assert len(mine) == 2 and len({r["mangled"] for r in mine}) == 2 and all("constrain_rows_kernel" in r["mangled"] for r in mine), [r["name"] for r in mine]
    for r in mine:
        assert r["scratch"] == 0 and r["occupancy"] >= 8, (r["name"], r["scratch"], r["vgprs"], r["occupancy"])
        for other in ("logits_process_kernel", "sample_token_kernel", "beam_rows_kernel", "adamw_kernel", "shifted_ce_", "ema_update_kernel", "token_logprob_kernel"):
            assert other not in r["mangled"], r["mangled"]
