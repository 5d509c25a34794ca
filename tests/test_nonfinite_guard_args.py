"""Skipping non-finite steps (FusedAdamW(skip_nonfinite=True), ff_grad_guard, ff_adamw_step_guarded) without a GPU: the two entry points
are additions under ABI 6 and reject bad arguments before any launch; the optimizer refuses the modes in which the verdict cannot be
reached, keeps torch.optim.AdamW's state_dict layout, and announces torch.amp.GradScaler's device protocol only when it is capturable."""
import ctypes as C

import pytest
import torch

FF_ERR_SHAPE, FF_ERR_UNSUPPORTED = -1, -2


def _params(n=3, device="cpu"):
    return [torch.nn.Parameter(torch.ones(4 + i, device=device)) for i in range(n)]


def test_abi_version_stays_6_and_the_additions_are_bound():
    from flamingo_mini_amd import ffi
    assert ffi.ABI_VERSION == 6 and ffi.lib().ff_version() == 6
    assert {"ff_grad_guard", "ff_adamw_step_guarded"} <= set(ffi.EXPORTED_SYMBOLS)


def test_grad_guard_argument_errors():
    """coef and skip are required, and so is a source of the verdict (a sum or ext_found_inf); the addresses are never dereferenced on the
    host, so any non-null value stands for a device scalar here - every call below must return before a launch."""
    from flamingo_mini_amd import ffi
    lib = ffi.lib()
    x = 64                                                      # "a device address"
    assert lib.ff_grad_guard(x, 1.0, None, None, x, None, x, x, x, None) == FF_ERR_SHAPE          # no coef
    assert b"ff_grad_guard" in lib.ff_last_error() and b"coef" in lib.ff_last_error()
    assert lib.ff_grad_guard(x, 1.0, None, None, x, x, None, x, x, None) == FF_ERR_SHAPE          # no skip
    assert b"ff_grad_guard" in lib.ff_last_error() and b"skip" in lib.ff_last_error()
    assert lib.ff_grad_guard(None, 1.0, None, x, x, x, x, x, x, None) == FF_ERR_SHAPE             # neither a sum nor ext_found_inf
    assert b"ff_grad_guard" in lib.ff_last_error()
    assert lib.ff_grad_guard(None, 0.0, None, None, None, None, None, None, None, None) == FF_ERR_SHAPE


def test_adamw_step_guarded_argument_errors():
    from flamingo_mini_amd import ffi
    lib = ffi.lib()
    none = ffi.ptr_array([None])
    numels = (C.c_longlong * 1)(0)
    x = 64                                                      # "a device address": never dereferenced on the host

    def desc(dtype, n=0, step=1):
        return ffi.AdamWDesc(dtype, n, step, 1e-3, 0.9, 0.999, 1e-8, 0.0, 1.0, None)

    def call(d, state_dtype, grads=none, fp32=0, master=None, coef=x, skip=x, n=numels, params=none):
        return lib.ff_adamw_step_guarded(d, state_dtype, params, grads, fp32, none, none, master, None, coef, skip, n, None)

    for fp32 in (0, 1):
        assert call(desc(ffi.DTYPE_BF16), ffi.DTYPE_F32, fp32=fp32, coef=None) == FF_ERR_SHAPE
        assert b"ff_adamw_step_guarded" in lib.ff_last_error() and b"grad_coef" in lib.ff_last_error()
        assert call(desc(ffi.DTYPE_BF16), ffi.DTYPE_F32, fp32=fp32, skip=None) == FF_ERR_SHAPE
        assert b"ff_adamw_step_guarded" in lib.ff_last_error() and b"skip" in lib.ff_last_error()
        assert call(None, ffi.DTYPE_F32, fp32=fp32) == FF_ERR_SHAPE
        assert call(desc(ffi.DTYPE_BF16), ffi.DTYPE_F32, grads=None, fp32=fp32) == FF_ERR_SHAPE
        assert call(desc(ffi.DTYPE_BF16), ffi.DTYPE_F32, fp32=fp32, n=None) == FF_ERR_SHAPE
        # fp32 master copies go with bf16 parameters
        assert call(desc(ffi.DTYPE_F32), ffi.DTYPE_F32, fp32=fp32, master=none) == FF_ERR_UNSUPPORTED
        assert b"master" in lib.ff_last_error()
        assert call(desc(7), 7, fp32=fp32) == FF_ERR_UNSUPPORTED                                  # dtype 7 does not exist
        assert call(desc(ffi.DTYPE_BF16), 5, fp32=fp32) == FF_ERR_UNSUPPORTED
        assert call(desc(ffi.DTYPE_BF16, step=0), ffi.DTYPE_F32, fp32=fp32) == FF_ERR_SHAPE
        # no tensors: nothing is launched, with and without master copies
        assert call(desc(ffi.DTYPE_BF16), ffi.DTYPE_F32, fp32=fp32, master=none) == 0
        assert call(desc(ffi.DTYPE_BF16), ffi.DTYPE_BF16, fp32=fp32) == 0
        assert call(desc(ffi.DTYPE_F32), ffi.DTYPE_F32, fp32=fp32) == 0
        one = (C.c_longlong * 1)(4)                            # a non-empty tensor without pointers
        assert call(desc(ffi.DTYPE_BF16, 1), ffi.DTYPE_BF16, fp32=fp32, n=one) == FF_ERR_SHAPE


def test_skip_nonfinite_needs_capturable():
    from flamingo_mini_amd import FusedAdamW
    with pytest.raises(ValueError, match="capturable"):
        FusedAdamW(_params(), skip_nonfinite=True)
    opt = FusedAdamW(_params(), capturable=True, skip_nonfinite=True)
    assert opt.skip_nonfinite is True and FusedAdamW(_params()).skip_nonfinite is False
    assert opt.step_skipped is None and opt.skipped_steps is None and opt.grad_norm is None


def test_skip_nonfinite_refuses_parameters_on_several_devices():
    from flamingo_mini_amd import FusedAdamW
    params = _params(2) + _params(1, device="meta")
    FusedAdamW(params, capturable=True)
    with pytest.raises(ValueError, match="one device"):
        FusedAdamW(params, capturable=True, skip_nonfinite=True)


@pytest.mark.parametrize("max_grad_norm", [None, 1.0])
def test_partial_steps_and_external_coefficients_cannot_be_guarded(max_grad_norm):
    from flamingo_mini_amd import FusedAdamW
    params = _params()
    opt = FusedAdamW(params, capturable=True, skip_nonfinite=True, max_grad_norm=max_grad_norm)
    for p in params:
        p.grad = torch.ones_like(p)
    with pytest.raises(ValueError, match="only"):
        opt.step(only={id(params[0])}, advance=True)
    with pytest.raises(ValueError, match="grad_coef"):
        opt.step(grad_coef=torch.ones(()))
    assert all(torch.equal(p.detach(), torch.ones_like(p)) for p in params)


def test_overlapped_piecewise_step_refuses_a_guarding_optimizer():
    """Raised in the constructor, before the model or the batch is touched (neither is usable here)."""
    from flamingo_mini_amd import FusedAdamW
    from flamingo_mini_amd.graphs import PiecewiseGraphedTrainStep
    opt = FusedAdamW(_params(), capturable=True, skip_nonfinite=True)
    with pytest.raises(ValueError, match="overlap_optimizer.*skip_nonfinite"):
        PiecewiseGraphedTrainStep(object(), opt, {}, overlap_optimizer=True)


def test_state_dict_layout_is_unchanged():
    from flamingo_mini_amd import FusedAdamW
    a, b = FusedAdamW(_params(), lr=1e-3, capturable=True), FusedAdamW(_params(), lr=1e-3, capturable=True, skip_nonfinite=True)
    sa, sb = a.state_dict(), b.state_dict()
    assert sa["param_groups"] == sb["param_groups"] and sa["state"].keys() == sb["state"].keys()
    assert all("skip_nonfinite" not in g for g in sb["param_groups"])
    b.load_state_dict(a.state_dict())
    assert b.skip_nonfinite is True and b.skipped_steps is None


def test_amp_scaling_protocol_is_announced_by_capturable_optimizers_only():
    from flamingo_mini_amd import FusedAdamW
    assert FusedAdamW(_params())._step_supports_amp_scaling is False
    assert FusedAdamW(_params(), capturable=True)._step_supports_amp_scaling is True
    assert FusedAdamW(_params(), capturable=True, skip_nonfinite=True, max_grad_norm=1.0)._step_supports_amp_scaling is True
    mixed = FusedAdamW([dict(params=_params(1)), dict(params=_params(1), capturable=False)], capturable=True)
    assert mixed._step_supports_amp_scaling is False


def test_scaler_attributes_need_capturable_groups():
    """found_inf / grad_scale set by hand on an optimizer that did not announce the protocol: refused before any library call."""
    from flamingo_mini_amd import FusedAdamW
    params = _params()
    opt = FusedAdamW(params)
    opt.found_inf, opt.grad_scale = torch.zeros(1), torch.ones(())
    with pytest.raises(ValueError, match="capturable"):
        opt.step()
