"""The weight average (FusedAdamW(ema_decay=...), ff_ema_update) without a GPU: the constructor's ValueErrors, the library's argument
errors - returned before anything touches a device, as tests/test_cabi.py checks for the workspace queries - and the checkpoint plumbing:
load_state_dict keeps the fp32 shadows of bf16 parameters in fp32 (torch's Optimizer.load_state_dict casts floating-point state to the
parameter's dtype), an optimizer built without ema_decay drops them, and the three settings stay out of state_dict()."""
import copy
import ctypes as C

import pytest
import torch

FF_ERR_SHAPE, FF_ERR_UNSUPPORTED = -1, -2


def _params():
    return [torch.nn.Parameter(torch.randn(5, 3).bfloat16()), torch.nn.Parameter(torch.randn(4))]


@pytest.mark.parametrize("kw,match", [(dict(ema_decay=0.0), "ema_decay"), (dict(ema_decay=1.0), "ema_decay"), (dict(ema_decay=-0.5), "ema_decay"),
                                      (dict(ema_decay=1.5), "ema_decay"), (dict(ema_decay=float("nan")), "ema_decay"),
                                      (dict(ema_decay=0.99, ema_every=0), "ema_every"), (dict(ema_decay=0.99, ema_every=-2), "ema_every"),
                                      (dict(ema_decay=0.99, ema_every=2.5), "ema_every"),
                                      (dict(ema_warmup=True), "need ema_decay"), (dict(ema_every=4), "need ema_decay")])
def test_constructor_refuses(kw, match):
    from flamingo_mini_amd import FusedAdamW
    with pytest.raises(ValueError, match=match):
        FusedAdamW(_params(), **kw)


def test_constructor_accepts_and_keeps_the_settings_out_of_state_dict():
    from flamingo_mini_amd import FusedAdamW
    plain = FusedAdamW(_params())
    assert (plain.ema_decay, plain.ema_warmup, plain.ema_every) == (None, False, 1) and list(plain.ema_parameters()) == []
    opt = FusedAdamW(_params(), ema_decay=0.999, ema_warmup=True, ema_every=8)
    assert (opt.ema_decay, opt.ema_warmup, opt.ema_every) == (0.999, True, 8)
    assert list(opt.ema_parameters()) == []                                    # no state yet: the shadows come with it
    sd, ref = opt.state_dict(), plain.state_dict()
    assert sd["param_groups"] == ref["param_groups"] and not any("ema" in k for g in sd["param_groups"] for k in g)
    with opt.swap_ema():                                                       # nothing to swap, but the block is one
        for call in (opt.step, opt.accumulate, lambda: opt.swap_ema().__enter__()):
            with pytest.raises(RuntimeError, match="swap_ema"):
                call()
    with opt.swap_ema():                                                       # (left properly: it can be entered again)
        pass


def test_ema_update_argument_errors_without_a_device():
    from flamingo_mini_amd import ffi
    lib = ffi.lib()
    assert "ff_ema_update" in ffi.EXPORTED_SYMBOLS and lib.ff_version() == 6
    numels = (C.c_longlong * 2)(5, 0)
    some = ffi.ptr_array([None, None])
    call = lambda dtype=ffi.DTYPE_BF16, n=2, p=some, w=None, e=some, k=numels, decay=0.999, warmup=0, every=1, step=1, step_dev=None: \
        lib.ff_ema_update(dtype, n, p, w, e, k, decay, warmup, every, step, step_dev, None, None)
    for decay in (0.0, 1.0, -0.1, 1.5, float("nan")):
        assert call(decay=decay) == FF_ERR_SHAPE, decay
        assert b"ff_ema_update" in lib.ff_last_error() and b"decay" in lib.ff_last_error()
    assert call(every=0) == FF_ERR_SHAPE and b"every" in lib.ff_last_error()
    assert call(every=-3) == FF_ERR_SHAPE
    assert call(step=0) == FF_ERR_SHAPE and b"step" in lib.ff_last_error()
    assert call(step=-1) == FF_ERR_SHAPE
    assert call(p=None) == FF_ERR_SHAPE and b"null" in lib.ff_last_error()     # null tables with n_tensors > 0
    assert call(e=None) == FF_ERR_SHAPE
    assert call(k=None) == FF_ERR_SHAPE
    assert call(n=-1) == FF_ERR_SHAPE
    assert call(dtype=7) == FF_ERR_UNSUPPORTED                                 # dtype 7 does not exist
    assert call() == FF_ERR_SHAPE and b"tensor 0" in lib.ff_last_error()       # a non-empty tensor without pointers
    assert call(p=None, w=some) == FF_ERR_SHAPE and b"tensor 0" in lib.ff_last_error()      # (params may be null where master is given)
    # nothing to do: no tensors, with and without tables; only zero-element tensors; a device step count in the place of the host's
    assert call(n=0, p=None, e=None, k=None) == 0
    assert call(n=0) == 0 and call(dtype=ffi.DTYPE_F32, n=0, warmup=1, every=8) == 0
    assert call(k=(C.c_longlong * 2)(0, 0)) == 0
    assert call(n=0, step=0, step_dev=C.c_void_p(16)) == 0


def _filled(params, **kw):
    from flamingo_mini_amd import FusedAdamW
    opt = FusedAdamW(params, **kw)
    g = torch.Generator().manual_seed(0)
    for p in params:                       # the state FusedAdamW._buckets creates on the device, written by hand
        st = opt.state[p]
        sdt = torch.float32 if (p.dtype == torch.bfloat16 and opt.state_dtype is not None) else p.dtype
        st["step"] = torch.tensor(3.0)
        st["exp_avg"] = torch.randn(p.shape, generator=g).to(sdt)
        st["exp_avg_sq"] = torch.rand(p.shape, generator=g).to(sdt)
        if p.dtype == torch.bfloat16 and opt.master_dtype is not None:
            st["master"] = p.detach().float() + 1e-4
        if opt.ema_decay is not None:
            st["ema"] = p.detach().float() + 3e-5              # differs from the bf16 rounding: a cast through bf16 would lose it
    return opt


def test_load_state_dict_keeps_the_shadows_in_fp32_and_drops_them_without_ema_decay():
    from flamingo_mini_amd import FusedAdamW
    params = _params()
    for kw in (dict(), dict(master_dtype=torch.float32), dict(stochastic_rounding=True)):
        src = _filled(params, ema_decay=0.999, **kw)
        assert [id(p) for p, _ in src.ema_parameters()] == [id(p) for p in params]
        sd = copy.deepcopy(src.state_dict())
        assert all("ema" in st and st["ema"].dtype == torch.float32 for st in sd["state"].values())
        fresh = [torch.nn.Parameter(p.detach().clone()) for p in params]
        dst = FusedAdamW(fresh, ema_decay=0.999, **kw)
        dst.load_state_dict(sd)
        for p, q in zip(params, fresh):
            assert set(src.state[p]) == set(dst.state[q])
            a, b = src.state[p]["ema"], dst.state[q]["ema"]
            assert b.dtype == torch.float32 and torch.equal(a, b) and b.data_ptr() != a.data_ptr(), kw
            if p.dtype == torch.bfloat16:
                assert not torch.equal(b, b.bfloat16().float())                # (the check can see a cast through bf16)
        # ... into an optimizer built without ema_decay: the shadows go, as master copies do
        plain = FusedAdamW([torch.nn.Parameter(p.detach().clone()) for p in params], **kw)
        plain.load_state_dict(copy.deepcopy(sd))
        assert all("ema" not in st for st in plain.state.values()) and list(plain.ema_parameters()) == []
        assert all("ema" not in st for st in plain.state_dict()["state"].values())
    # a checkpoint without shadows into an optimizer that averages: loads, has none yet (the next step creates them)
    sd = copy.deepcopy(_filled(params).state_dict())
    late = FusedAdamW([torch.nn.Parameter(p.detach().clone()) for p in params], ema_decay=0.9)
    late.load_state_dict(sd)
    assert list(late.ema_parameters()) == [] and all("exp_avg" in st for st in late.state.values())
