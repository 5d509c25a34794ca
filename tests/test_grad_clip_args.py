"""Gradient clipping (max_grad_norm) without a GPU: argument validation, the modes that cannot clip refuse up front, the optimizer's
state_dict keeps torch.optim.AdamW's layout, and the library's new entry points count slots and reject bad arguments before any launch."""
import ctypes as C

import pytest
import torch


def _params(n=3, device="cpu"):
    return [torch.nn.Parameter(torch.ones(4 + i, device=device)) for i in range(n)]


@pytest.mark.parametrize("bad", [0.0, -1.0, float("nan")])
def test_max_grad_norm_must_be_positive(bad):
    from flamingo_mini_amd import FusedAdamW
    with pytest.raises(ValueError, match="max_grad_norm"):
        FusedAdamW(_params(), max_grad_norm=bad)
    from flamingo_mini_amd.data_parallel import ShardedAdamW
    with pytest.raises(ValueError, match="max_grad_norm"):
        ShardedAdamW(torch.nn.Linear(2, 2), max_grad_norm=bad)


def test_max_grad_norm_refuses_parameters_on_several_devices():
    from flamingo_mini_amd import FusedAdamW
    params = _params(2) + _params(1, device="meta")
    FusedAdamW(params)                                   # without clipping nothing spans the devices
    with pytest.raises(ValueError, match="one device"):
        FusedAdamW(params, max_grad_norm=1.0)


def test_partial_steps_cannot_clip():
    from flamingo_mini_amd import FusedAdamW
    params = _params()
    opt = FusedAdamW(params, capturable=True, max_grad_norm=1.0)
    for p in params:
        p.grad = torch.ones_like(p)
    with pytest.raises(ValueError, match="only"):
        opt.step(only={id(params[0])}, advance=True)
    with pytest.raises(ValueError, match="grad_coef"):
        opt.step(grad_coef=torch.ones(()))


def test_overlapped_piecewise_step_refuses_a_clipping_optimizer():
    """Raised in the constructor, before the model or the batch is touched (neither is usable here)."""
    from flamingo_mini_amd import FusedAdamW
    from flamingo_mini_amd.graphs import PiecewiseGraphedTrainStep
    opt = FusedAdamW(_params(), capturable=True, max_grad_norm=1.0)
    with pytest.raises(ValueError, match="overlap_optimizer.*max_grad_norm"):
        PiecewiseGraphedTrainStep(object(), opt, {}, overlap_optimizer=True)


def test_state_dict_layout_is_unchanged():
    from flamingo_mini_amd import FusedAdamW
    a, b = FusedAdamW(_params(), lr=1e-3), FusedAdamW(_params(), lr=1e-3, max_grad_norm=1.0)
    sa, sb = a.state_dict(), b.state_dict()
    assert sa["param_groups"] == sb["param_groups"]
    assert all("max_grad_norm" not in g for g in sb["param_groups"])
    b.load_state_dict(torch.optim.AdamW(_params(), lr=1e-3).state_dict())
    assert b.max_grad_norm == 1.0 and b.grad_norm is None


def test_functional_clip_refuses_other_norms():
    from flamingo_mini_amd import clip_grad_norm_
    with pytest.raises(ValueError, match="norm_type"):
        clip_grad_norm_(_params(), 1.0, norm_type=float("inf"))


def test_sumsq_slot_count_and_argument_errors():
    """One partial per 32768-element chunk of every non-empty tensor, 2048 for the token embedding (64 M elements); the launches reject
    a partial buffer that is too small, an unknown dtype and a null coefficient with error codes, before anything reaches a device."""
    from flamingo_mini_amd import ffi
    lib = ffi.lib()
    numels = [1, 32768, 32769, 0, 64 * 1024 * 1024, 3 * 2 ** 31]
    arr = (C.c_longlong * len(numels))(*numels)
    assert lib.ff_grad_sumsq_partials(len(numels), arr) == 1 + 1 + 2 + 0 + 2048 + 3 * 2 ** 16
    assert lib.ff_grad_sumsq_partials(0, None) == 0
    grads = ffi.ptr_array([None] * 3)
    small = (C.c_longlong * 3)(10, 40000, 5)
    assert lib.ff_grad_sumsq(ffi.DTYPE_F32, 3, grads, small, 1.0, None, 3, None) == -3           # needs 4 partials: FF_ERR_WORKSPACE
    assert b"partials" in lib.ff_last_error()
    assert lib.ff_grad_sumsq(7, 3, grads, small, 1.0, None, 100, None) == -2                     # FF_ERR_UNSUPPORTED
    assert lib.ff_scale_grads(ffi.DTYPE_BF16, 3, grads, small, None, None) == -1                 # no coefficient: FF_ERR_SHAPE
    assert lib.ff_grad_clip_coef(None, 1.0, None, None, None) == -1
