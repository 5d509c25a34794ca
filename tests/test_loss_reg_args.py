"""label_smoothing and z_loss from the public interface down, without a GPU: argument validation in functional.shifted_cross_entropy and in
forward(), the optional config keys and their override, the stock-op branch of forward() (CPU tensors) against the definition written out
independently - all three reductions, ignored positions, loss and gradient on the logits -, bit-equality of the feature-off forms, and the
two new entry points in the header and the ctypes table."""
import numpy as np
import pytest
import torch

import oracle_backend
from test_model_plumbing import build

EPS, ZETA = 0.1, 1e-4


@pytest.fixture(scope="module")
def tiny():
    """(model in float64 on the CPU with the fused blocks on the numpy oracle, the batch with two ignored label positions, the golden)"""
    oracle_backend.install()
    try:
        model, z = build(torch.float64, "cpu", "gpt2")
        model.eval()
        ids, ml = torch.from_numpy(z["ids"]), torch.from_numpy(z["ml"])
        labels = ids.clone()
        labels[0, 3] = -100
        labels[1, -1] = -100
        batch = dict(input_ids=ids, attention_mask=torch.ones_like(ids), media_locations=ml, pixel_values=torch.from_numpy(z["px"]), labels=labels)
        yield model, batch
    finally:
        oracle_backend.uninstall()


def definition(logits, labels, eps, zeta):
    """per scored token lse - (1 - eps) x_t - eps mean(x) + zeta lse^2 and its gradient p (1 + 2 zeta lse) - (1 - eps) onehot - eps / V, in
    numpy float64, loops over the tokens: (rows (b (L - 1),), d rows / d logits (b, L, V) for unit row gradients)"""
    x, lab = logits.detach().numpy().astype(np.float64), labels.numpy()
    b, L, V = x.shape
    rows, d = np.zeros(b * (L - 1)), np.zeros_like(x)
    for s in range(b):
        for i in range(L - 1):
            t = lab[s, i + 1]
            if t == -100:
                continue
            m = x[s, i].max()
            lse = m + np.log(np.exp(x[s, i] - m).sum())
            rows[s * (L - 1) + i] = lse - (1 - eps) * x[s, i, t] - eps * x[s, i].mean() + zeta * lse * lse
            d[s, i] = np.exp(x[s, i] - lse) * (1 + 2 * zeta * lse) - eps / V
            d[s, i, t] -= 1 - eps
    return rows, d


@pytest.mark.parametrize("reduction", ["mean", "sum", "none"])
def test_forward_on_the_cpu_returns_the_regularised_loss_and_its_gradient(tiny, reduction):
    model, batch = tiny
    out = model(**batch, loss_reduction=reduction, label_smoothing=EPS, z_loss=ZETA)
    out.logits.retain_grad()
    rows, d = definition(out.logits, batch["labels"], EPS, ZETA)
    count = int((batch["labels"][:, 1:] != -100).sum())
    assert count == rows.size - 2
    g = np.random.default_rng(3).standard_normal(rows.size)
    want = {"mean": rows.sum() / count, "sum": rows.sum(), "none": rows}[reduction]
    weight = {"mean": np.full(rows.size, 1.0 / count), "sum": np.ones(rows.size), "none": g}[reduction]
    np.testing.assert_allclose(out.loss.detach().numpy(), want, rtol=1e-12, atol=0)
    (out.loss * torch.from_numpy(g)).sum().backward() if reduction == "none" else out.loss.backward()
    b, L, V = d.shape
    want_d = d.copy()
    want_d[:, :-1] *= weight.reshape(b, L - 1, 1)
    np.testing.assert_allclose(out.logits.grad.numpy(), want_d, rtol=1e-11, atol=1e-15)
    assert not out.logits.grad[:, -1].any() and not out.logits.grad[0, 2].any() and not out.logits.grad[1, -2].any()      # last position, ignored targets
    plain = model(**batch, loss_reduction=reduction).loss
    assert float((out.loss - plain).abs().max()) > 1e-5          # (logits of a random tiny model are nearly flat: the terms nearly cancel, 3e-4 here)


def test_both_off_is_bit_equal_to_a_call_without_the_arguments(tiny):
    model, batch = tiny
    base = model(**batch).loss
    for kw in (dict(label_smoothing=0.0, z_loss=0.0), dict(label_smoothing=None, z_loss=None), dict(label_smoothing=0), dict(z_loss=0.0)):
        assert torch.equal(model(**batch, **kw).loss, base), kw
        assert torch.equal(model.flamingo(**batch, **kw).loss, base), kw
    logits = model(**batch).logits
    ref = torch.nn.functional.cross_entropy(logits[:, :-1].reshape(-1, logits.shape[-1]), batch["labels"][:, 1:].reshape(-1))
    assert torch.equal(base, ref)


def test_none_takes_the_config_keys_and_an_explicit_value_overrides_them(tiny):
    model, batch = tiny
    assert not hasattr(model.config, "label_smoothing") and not hasattr(model.config, "z_loss")
    plain = model(**batch).loss
    explicit = model(**batch, label_smoothing=EPS, z_loss=ZETA).loss
    only_eps = model(**batch, label_smoothing=EPS).loss
    assert len({float(plain), float(explicit), float(only_eps)}) == 3
    try:
        model.config.label_smoothing, model.config.z_loss = EPS, ZETA
        assert model.flamingo.config is model.config
        assert torch.equal(model(**batch).loss, explicit)                                  # what a loop calling model(**batch) gets
        assert torch.equal(model(**batch, label_smoothing=None, z_loss=None).loss, explicit)
        assert torch.equal(model(**batch, label_smoothing=0.0, z_loss=0.0).loss, plain)     # the plain evaluation loss
        assert torch.equal(model(**batch, z_loss=0.0).loss, only_eps)
        model.config.label_smoothing = 1.5
        with pytest.raises(ValueError, match="label_smoothing"):
            model(**batch)
    finally:
        del model.config.label_smoothing, model.config.z_loss
    assert torch.equal(model(**batch).loss, plain)


def test_the_config_keys_are_stored_like_any_other_config_kwarg(tmp_path):
    from flamingo_mini_amd import FlamingoConfig
    cfg = FlamingoConfig(dim=64, dim_visual=48, label_smoothing=0.1, z_loss=1e-4)
    cfg.save_pretrained(tmp_path)
    back = FlamingoConfig.from_pretrained(tmp_path)
    assert (back.label_smoothing, back.z_loss) == (0.1, 1e-4)
    assert not hasattr(FlamingoConfig(dim=64, dim_visual=48), "label_smoothing")


BAD = [dict(label_smoothing=-0.01), dict(label_smoothing=1.01), dict(label_smoothing=float("nan")), dict(z_loss=-1e-9), dict(z_loss=float("inf")),
       dict(z_loss=float("nan"))]


@pytest.mark.parametrize("kw", BAD, ids=[f"{k}={v}" for d in BAD for k, v in d.items()])
def test_bad_values_raise_value_error(tiny, kw):
    from flamingo_mini_amd import functional as F
    model, batch = tiny
    with pytest.raises(ValueError, match=next(iter(kw))):
        F.shifted_cross_entropy(torch.zeros(1, 3, 5), torch.zeros(1, 3, dtype=torch.long), **kw)        # before any look at the device
    with pytest.raises(ValueError, match=next(iter(kw))):
        model(**batch, **kw)
    with pytest.raises(ValueError, match=next(iter(kw))):
        model(**{k: v for k, v in batch.items() if k != "labels"}, **kw)                                 # with no loss to compute, too


def test_the_limits_of_the_ranges_are_accepted(tiny):
    from flamingo_mini_amd import functional as F
    model, batch = tiny
    assert F.check_loss_regularisers(1, 0) == (1.0, 0.0) and F.check_loss_regularisers(0.0, 3.0e38) == (0.0, 3.0e38)
    assert torch.isfinite(model(**batch, label_smoothing=1.0, z_loss=0.5).loss)


def test_header_and_ctypes_table_agree_on_the_new_entry_points():
    import ctypes as C
    from flamingo_mini_amd import ffi
    from test_cabi import _header_prototypes
    protos = _header_prototypes()
    for name, plain in (("ff_shifted_ce_fwd_reg", "ff_shifted_ce_fwd"), ("ff_shifted_ce_bwd_reg", "ff_shifted_ce_bwd")):
        assert protos[name] == ("int", protos[plain][1][:-1] + ["float", "float", "ptr"])               # the plain arguments, the two values, the stream
        res, args = ffi._SIGNATURES[name]
        assert res is C.c_int and args == ffi._SIGNATURES[plain][1][:-1] + [C.c_float, C.c_float, C.c_void_p]
        assert hasattr(ffi.lib(), name)
    assert ffi.lib().ff_version() == 6


def test_bad_values_come_back_as_error_codes_without_a_launch():
    """(no device here: a launch would fail differently - the range check comes first, and the message names the argument)"""
    import ctypes as C
    from flamingo_mini_amd import ffi
    lib, p = ffi.lib(), C.c_void_p(16)
    for eps, zeta in ((-0.5, 0.0), (1.5, 0.0), (float("nan"), 0.0), (0.1, -1.0), (0.1, float("inf")), (0.1, float("nan"))):
        assert lib.ff_shifted_ce_fwd_reg(ffi.DTYPE_BF16, 2, 5, 9, p, p, -100, p, p, eps, zeta, None) == -2, (eps, zeta)
        assert b"label_smoothing" in lib.ff_last_error()
        assert lib.ff_shifted_ce_bwd_reg(ffi.DTYPE_BF16, 2, 5, 9, p, p, -100, p, p, p, eps, zeta, None) == -2, (eps, zeta)
        assert b"z_loss" in lib.ff_last_error()
    assert lib.ff_shifted_ce_fwd_reg(ffi.DTYPE_BF16, 2, 1, 9, p, p, -100, p, p, 0.1, 0.0, None) == -1          # seq 1: a shape error, as in the plain form
