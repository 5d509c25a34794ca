"""Sampled decoding without a GPU: ff_sample_token rejects bad arguments with its error codes before anything reaches a device, static
sampled decoding refuses CPU tensors, and generate(do_sample=True) with the default routing is still the dynamic loop, draw for draw."""
import ctypes as C

import pytest
import torch

FF_ERR_SHAPE, FF_ERR_UNSUPPORTED = -1, -2
X = C.c_void_p(256)            # a non-null pointer that is never dereferenced: every call below fails its checks first


def _call(dtype=None, rows=4, vocab=100, ld=100, logits=X, temperature=1.0, top_k=0, top_p=1.0, u=X, token=X):
    from flamingo_mini_amd import ffi
    return ffi.lib().ff_sample_token(ffi.DTYPE_BF16 if dtype is None else dtype, rows, vocab, ld, logits, temperature, top_k, top_p, u, token, None)


def test_the_entry_point_is_bound():
    from flamingo_mini_amd import ffi, functional as F
    assert "ff_sample_token" in ffi.EXPORTED_SYMBOLS and ffi.lib().ff_version() == 6
    assert callable(F.sample_tokens)


@pytest.mark.parametrize("bad", [
    dict(logits=None), dict(u=None), dict(token=None),
    dict(rows=0), dict(rows=-3), dict(vocab=0), dict(vocab=-1), dict(ld=99),
    dict(temperature=0.0), dict(temperature=-1.0), dict(temperature=float("inf")), dict(temperature=float("nan")),
    dict(top_k=-1),
    dict(top_p=0.0), dict(top_p=-0.5), dict(top_p=1.0000001), dict(top_p=float("nan")),
], ids=lambda d: "-".join(f"{k}={v}" for k, v in d.items()))
def test_argument_errors_return_shape_before_any_launch(bad):
    from flamingo_mini_amd import ffi
    assert _call(**bad) == FF_ERR_SHAPE
    assert b"ff_sample_token" in ffi.lib().ff_last_error()


def test_other_dtypes_are_unsupported():
    from flamingo_mini_amd import ffi
    assert _call(dtype=7) == FF_ERR_UNSUPPORTED
    assert b"ff_sample_token" in ffi.lib().ff_last_error() and b"dtype" in ffi.lib().ff_last_error()


def test_sample_tokens_has_no_cpu_form():
    from flamingo_mini_amd import ffi, functional as F
    with pytest.raises(ffi.FusionLibraryError, match="no CPU fallback"):
        F.sample_tokens(torch.zeros(2, 5), torch.zeros(2))


@pytest.mark.parametrize("family", ["gpt2", "opt"])
def test_routing_on_the_host(family):
    """static_decode=True with do_sample on CPU tensors raises what ffi.require_cuda raises (and builds no session); the default routing is
    the dynamic loop - restated here from its parts (_decode_step, _filter_logits, torch.multinomial) - token for token, for a fixed seed."""
    import oracle_backend
    from flamingo_mini_amd import ffi
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
        with pytest.raises(ffi.FusionLibraryError, match="no CPU fallback"):
            model.generate(ids, static_decode=True, generator=torch.Generator().manual_seed(3), **sk, **kw)
        assert len(model._decode_sessions) == 0

        got = model.generate(ids, generator=torch.Generator().manual_seed(3), **sk, **kw)
        also = model.generate(ids, static_decode=False, generator=torch.Generator().manual_seed(3), **sk, **kw)
        assert len(model._decode_sessions) == 0

        g = torch.Generator().manual_seed(3)
        seq, ml_, am_, past, step = ids, ml, am, None, ids
        with torch.no_grad():
            while seq.shape[1] < 9:
                logits, past = model._decode_step(step, ml_, am_, past, px, None)
                probs = model._filter_logits(logits, 0.7, 20, 0.9).softmax(-1)
                nxt = torch.multinomial(probs, 1, generator=g)[:, 0]
                seq = torch.cat([seq, nxt[:, None]], 1)
                ml_ = torch.cat([ml_, torch.zeros_like(ml_[:, :1])], 1)
                am_ = torch.cat([am_, torch.ones_like(am_[:, :1])], 1)
                step = seq[:, -1:]
        assert got.shape == (2, 9) and torch.equal(got, seq) and torch.equal(also, seq)
    finally:
        oracle_backend.uninstall()
