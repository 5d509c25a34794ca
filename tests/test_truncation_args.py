"""The truncation samplers without a GPU: ff_sample_token_truncated is bound and rejects bad arguments with its error codes before anything
reaches a device; generate() checks min_p / typical_p / epsilon_cutoff / eta_cutoff; on CPU tensors the default routing is the dynamic loop
with decoding.truncate_logits_torch, draw for draw; static_decode=True on CPU tensors raises what ffi.require_cuda raises."""
import ctypes as C

import pytest
import torch

FF_ERR_SHAPE, FF_ERR_UNSUPPORTED = -1, -2
X = C.c_void_p(256)            # a non-null pointer that is never dereferenced: every call below fails its checks first
NAN, INF = float("nan"), float("inf")


def _call(dtype=None, rows=4, vocab=100, ld=100, logits=X, temperature=1.0, top_k=0, top_p=1.0, min_p=0.05, typical_p=0.9, epsilon_cutoff=1e-3,
          eta_cutoff=1e-3, u=X, token=X):
    from flamingo_mini_amd import ffi
    return ffi.lib().ff_sample_token_truncated(ffi.DTYPE_BF16 if dtype is None else dtype, rows, vocab, ld, logits, temperature, top_k, top_p,
                                               min_p, typical_p, epsilon_cutoff, eta_cutoff, u, token, None)


def test_the_entry_point_is_bound():
    import inspect
    from flamingo_mini_amd import decoding, ffi, functional as F
    assert "ff_sample_token_truncated" in ffi.EXPORTED_SYMBOLS and hasattr(ffi.lib(), "ff_sample_token_truncated") and ffi.lib().ff_version() == 6
    par = inspect.signature(F.sample_tokens).parameters
    for name, off in (("min_p", 0.0), ("typical_p", 1.0), ("epsilon_cutoff", 0.0), ("eta_cutoff", 0.0)):
        assert par[name].kind is inspect.Parameter.KEYWORD_ONLY and par[name].default == off
    assert decoding.Truncation._fields == ("min_p", "typical_p", "epsilon_cutoff", "eta_cutoff") and decoding.Sampling._fields == ("temperature", "top_k", "top_p")


@pytest.mark.parametrize("bad", [
    dict(logits=None), dict(u=None), dict(token=None),
    dict(rows=0), dict(rows=-3), dict(vocab=0), dict(vocab=-1), dict(ld=99),
    dict(temperature=0.0), dict(temperature=-1.0), dict(temperature=INF), dict(temperature=NAN),
    dict(top_k=-1),
    dict(top_p=0.0), dict(top_p=-0.5), dict(top_p=1.0000001), dict(top_p=NAN),
    dict(min_p=-0.1), dict(min_p=1.0000001), dict(min_p=NAN), dict(min_p=INF),
    dict(typical_p=0.0), dict(typical_p=-0.5), dict(typical_p=1.0000001), dict(typical_p=NAN), dict(typical_p=INF),
    dict(epsilon_cutoff=-1e-3), dict(epsilon_cutoff=1.0), dict(epsilon_cutoff=NAN), dict(epsilon_cutoff=INF),
    dict(eta_cutoff=-1e-3), dict(eta_cutoff=1.0), dict(eta_cutoff=NAN), dict(eta_cutoff=-INF),
], ids=lambda d: "-".join(f"{k}={v}" for k, v in d.items()))
def test_argument_errors_return_shape_before_any_launch(bad):
    from flamingo_mini_amd import ffi
    assert _call(**bad) == FF_ERR_SHAPE
    assert b"ff_sample_token_truncated" in ffi.lib().ff_last_error()


def test_other_dtypes_are_unsupported():
    from flamingo_mini_amd import ffi
    for dtype in (7, 2, -1):
        assert _call(dtype=dtype) == FF_ERR_UNSUPPORTED
        assert b"ff_sample_token_truncated" in ffi.lib().ff_last_error() and b"dtype" in ffi.lib().ff_last_error()


def test_sample_tokens_has_no_cpu_form_with_the_rules_either():
    from flamingo_mini_amd import ffi, functional as F
    with pytest.raises(ffi.FusionLibraryError, match="no CPU fallback"):
        F.sample_tokens(torch.zeros(2, 5), torch.zeros(2), min_p=0.1)


def test_check_truncation_args():
    from flamingo_mini_amd import decoding as D
    assert D.check_truncation_args(0.0, 1.0, 0.0, 0.0, False, 1) is None and D.check_truncation_args(0, 1, 0, 0, False, 4) is None
    t = D.check_truncation_args(0.05, 1.0, 0.0, 3e-4, True, 1)
    assert t == (0.05, 1.0, 0.0, 3e-4) and isinstance(t, D.Truncation)
    assert D.check_truncation_args(1, 0.5, 0.999, 0.999, True, 1) == (1.0, 0.5, 0.999, 0.999)
    for bad in (dict(min_p=-0.1), dict(min_p=1.1), dict(min_p=NAN), dict(min_p="0.1"), dict(min_p=True), dict(min_p=None),
                dict(typical_p=0.0), dict(typical_p=1.1), dict(typical_p=NAN), dict(typical_p=None),
                dict(epsilon_cutoff=-0.1), dict(epsilon_cutoff=1.0), dict(epsilon_cutoff=INF), dict(eta_cutoff=1.0), dict(eta_cutoff=NAN), dict(eta_cutoff=-1)):
        kw = dict(min_p=0.0, typical_p=1.0, epsilon_cutoff=0.0, eta_cutoff=0.0, do_sample=True, num_beams=1)
        with pytest.raises(ValueError, match=next(iter(bad))):
            D.check_truncation_args(**dict(kw, **bad))
    with pytest.raises(ValueError, match="do_sample"):
        D.check_truncation_args(0.1, 1.0, 0.0, 0.0, False, 1)
    with pytest.raises(ValueError, match="beam"):
        D.check_truncation_args(0.0, 0.9, 0.0, 0.0, True, 4)


@pytest.mark.parametrize("family", ["gpt2", "opt"])
def test_generate_on_the_host(family):
    """generate() raises ValueError for values out of range, for use without do_sample and for use with beams; static_decode=True with CPU
    tensors raises what ffi.require_cuda raises (and builds no session); the default routing is the dynamic loop - restated here from its
    parts (_decode_step, _filter_logits, truncate_logits_torch, torch.multinomial) - token for token, for a fixed seed."""
    import oracle_backend
    from flamingo_mini_amd import decoding, ffi
    from test_model_plumbing import build
    oracle_backend.install()
    try:
        model, z = build(torch.float64, "cpu", family)
        model.eval()
        px = torch.from_numpy(z["px"]).double()
        ids, ml = torch.from_numpy(z["ids"])[:, :4], torch.from_numpy(z["ml"])[:, :4]
        am = torch.ones_like(ids)
        kw = dict(media_locations=ml, attention_mask=am, pixel_values=px, max_length=9)
        sk = dict(do_sample=True, temperature=0.7, top_k=20, top_p=0.9)
        tk = dict(min_p=0.05, typical_p=0.9)
        for bad in (dict(min_p=1.5), dict(typical_p=0.0), dict(epsilon_cutoff=1.0), dict(eta_cutoff=-0.1), dict(min_p=NAN)):
            with pytest.raises(ValueError, match=next(iter(bad))):
                model.generate(ids, **sk, **kw, **bad)
        with pytest.raises(ValueError, match="do_sample"):
            model.generate(ids, **kw, **tk)
        with pytest.raises(ValueError, match="beam"):
            model.generate(ids, num_beams=2, **kw, **tk)
        with pytest.raises(ffi.FusionLibraryError, match="no CPU fallback"):
            model.generate(ids, static_decode=True, generator=torch.Generator().manual_seed(3), **sk, **tk, **kw)
        assert len(model._decode_sessions) == 0

        got = model.generate(ids, generator=torch.Generator().manual_seed(3), **sk, **tk, **kw)
        also = model.generate(ids, static_decode=False, generator=torch.Generator().manual_seed(3), **sk, **tk, **kw)
        plain = model.generate(ids, generator=torch.Generator().manual_seed(3), **sk, **kw)
        assert len(model._decode_sessions) == 0

        def loop(truncate):
            g = torch.Generator().manual_seed(3)
            seq, ml_, am_, past, step = ids, ml, am, None, ids
            cut = 0
            with torch.no_grad():
                while seq.shape[1] < 9:
                    logits, past = model._decode_step(step, ml_, am_, past, px, None)
                    filtered = model._filter_logits(logits, 0.7, 20, 0.9)
                    if truncate:
                        kept = decoding.truncate_logits_torch(filtered, 0.05, 0.9, 0.0, 0.0)
                        cut += int(((kept > float("-inf")).sum() < (filtered > float("-inf")).sum()))
                        filtered = kept
                    nxt = torch.multinomial(filtered.softmax(-1), 1, generator=g)[:, 0]
                    seq = torch.cat([seq, nxt[:, None]], 1)
                    ml_ = torch.cat([ml_, torch.zeros_like(ml_[:, :1])], 1)
                    am_ = torch.cat([am_, torch.ones_like(am_[:, :1])], 1)
                    step = seq[:, -1:]
            return seq, cut

        seq, cut = loop(True)
        assert cut > 0, "the rules cut nothing at these settings"
        assert got.shape == (2, 9) and torch.equal(got, seq) and torch.equal(also, seq)
        assert torch.equal(plain, loop(False)[0])                        # and without the rules the call is what it was
    finally:
        oracle_backend.uninstall()
