"""fp32 gradient accumulation (FusedAdamW.accumulate, ABI 6) without a GPU: the library's two new entry points reject bad arguments before
any launch, and the optimizer's host-side plumbing runs on CPU tensors over tests/host_lib.py extended by numpy versions of the two calls -
accumulate() leaves `.grad is None`, so the second micro-batch's backward keeps the deferred, grouped weight-gradient launches that autograd's
own accumulation loses; the accumulators hold the weighted sum; step() refuses an unfolded `.grad`, steps like torch.optim.AdamW on the
accumulated gradients, and state_dict() keeps torch's layout."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tests", "golden")):
    if p not in sys.path:
        sys.path.insert(0, p)

import host_lib  # noqa: E402

FF_ERR_SHAPE, FF_ERR_UNSUPPORTED = -1, -2


def test_abi_version_is_6():
    from flamingo_mini_amd import ffi
    assert ffi.ABI_VERSION == 6 and ffi.lib().ff_version() == 6
    assert {"ff_grad_accumulate", "ff_adamw_step_acc"} <= set(ffi.EXPORTED_SYMBOLS)


def test_grad_accumulate_argument_errors():
    from flamingo_mini_amd import ffi
    lib = ffi.lib()
    numels = (C.c_longlong * 2)(5, 0)
    some = ffi.ptr_array([None, None])
    assert lib.ff_grad_accumulate(ffi.DTYPE_BF16, 2, None, None, None, 1.0, 1, None) == FF_ERR_SHAPE          # null tables
    assert b"ff_grad_accumulate" in lib.ff_last_error()
    assert lib.ff_grad_accumulate(ffi.DTYPE_F32, 2, some, None, numels, 1.0, 0, None) == FF_ERR_SHAPE
    assert lib.ff_grad_accumulate(ffi.DTYPE_F32, 2, some, some, numels, 1.0, 0, None) == FF_ERR_SHAPE         # a non-empty tensor without pointers
    assert b"tensor 0" in lib.ff_last_error()
    assert lib.ff_grad_accumulate(7, 2, some, some, numels, 1.0, 1, None) == FF_ERR_UNSUPPORTED              # dtype 7 does not exist
    assert lib.ff_grad_accumulate(ffi.DTYPE_BF16, 0, None, None, None, 1.0, 1, None) == 0                    # nothing to do
    assert lib.ff_grad_accumulate(ffi.DTYPE_F32, -1, some, some, numels, 1.0, 1, None) == FF_ERR_SHAPE


def test_adamw_step_acc_argument_errors():
    from flamingo_mini_amd import ffi
    lib = ffi.lib()
    none = ffi.ptr_array([None])
    numels = (C.c_longlong * 1)(0)

    def desc(dtype, n=0, step=1):
        return ffi.AdamWDesc(dtype, n, step, 1e-3, 0.9, 0.999, 1e-8, 0.0, 1.0, None)

    assert lib.ff_adamw_step_acc(None, ffi.DTYPE_F32, none, none, none, none, None, None, None, numels, None) == FF_ERR_SHAPE
    assert lib.ff_adamw_step_acc(desc(ffi.DTYPE_BF16), ffi.DTYPE_F32, none, None, none, none, None, None, None, numels, None) == FF_ERR_SHAPE
    assert lib.ff_adamw_step_acc(desc(ffi.DTYPE_BF16), ffi.DTYPE_F32, none, none, none, none, None, None, None, None, None) == FF_ERR_SHAPE
    # fp32 master copies go with bf16 parameters
    assert lib.ff_adamw_step_acc(desc(ffi.DTYPE_F32), ffi.DTYPE_F32, none, none, none, none, none, None, None, numels, None) == FF_ERR_UNSUPPORTED
    assert b"master" in lib.ff_last_error()
    assert lib.ff_adamw_step_acc(desc(7), 7, none, none, none, none, None, None, None, numels, None) == FF_ERR_UNSUPPORTED
    assert lib.ff_adamw_step_acc(desc(ffi.DTYPE_BF16), 5, none, none, none, none, None, None, None, numels, None) == FF_ERR_UNSUPPORTED
    assert lib.ff_adamw_step_acc(desc(ffi.DTYPE_BF16, step=0), ffi.DTYPE_F32, none, none, none, none, None, None, None, numels, None) == FF_ERR_SHAPE
    # no tensors: nothing is launched, with and without master copies / a clip coefficient (NULL = unclipped)
    assert lib.ff_adamw_step_acc(desc(ffi.DTYPE_BF16), ffi.DTYPE_F32, none, none, none, none, none, None, None, numels, None) == 0
    assert lib.ff_adamw_step_acc(desc(ffi.DTYPE_F32), ffi.DTYPE_F32, none, none, none, none, None, None, None, numels, None) == 0
    one = (C.c_longlong * 1)(4)                                # a non-empty tensor without pointers
    assert lib.ff_adamw_step_acc(desc(ffi.DTYPE_BF16, 1), ffi.DTYPE_BF16, none, none, none, none, None, None, None, one, None) == FF_ERR_SHAPE


# ---- the optimizer's plumbing on CPU tensors --------------------------------------------------------------------------------------------
class AccumHostLib(host_lib.HostLib):
    """tests/host_lib.HostLib plus the two ABI 6 calls in numpy (float32 parameters and gradients only, float64 arithmetic)."""

    def ff_grad_accumulate(self, dtype, n, grads, acc, numels, scale, overwrite, stream):
        self.calls.append(f"ff_grad_accumulate[{n},{'overwrite' if overwrite else 'add'}]")
        assert dtype == 0
        s = float(np.float32(scale))
        for g, a, k in zip(host_lib._ptrs(grads, n), host_lib._ptrs(acc, n), numels):
            if k:
                gv, av = host_lib._view(g, (k,)), host_lib._view(a, (k,))
                av[...] = (0.0 if overwrite else av.astype(np.float64)) + s * gv.astype(np.float64)
        return 0

    def ff_adamw_step_acc(self, d, state_dtype, params, grads32, exp_avg, exp_avg_sq, master, lr_dev, grad_coef, numels, stream):
        self.calls.append(f"ff_adamw_step_acc[{d.n_tensors}]")
        assert d.dtype == 0 and state_dtype == 0 and master is None and lr_dev is None and grad_coef is None and not d.step_dev
        f = lambda x: float(np.float32(x))
        lr, b1, b2, eps, wd, gs = f(d.lr), f(d.beta1), f(d.beta2), f(d.eps), f(d.weight_decay), f(d.grad_scale or 1.0)
        for p, g, m, v, k in zip(*(host_lib._ptrs(t, d.n_tensors) for t in (params, grads32, exp_avg, exp_avg_sq)), numels):
            if not k:
                continue
            pv, gv, mv, vv = (host_lib._view(q, (k,)) for q in (p, g, m, v))
            g64 = gv.astype(np.float64) * gs
            m64 = b1 * mv.astype(np.float64) + (1 - b1) * g64
            v64 = b2 * vv.astype(np.float64) + (1 - b2) * g64 * g64
            upd = (lr / (1 - b1 ** d.step)) * m64 / (np.sqrt(v64) / np.sqrt(1 - b2 ** d.step) + eps)
            pv[...] = pv.astype(np.float64) * (1 - lr * wd) - upd
            mv[...], vv[...] = m64, v64
        return 0


@pytest.fixture
def accum_host(monkeypatch):
    """The tiny GPT-2-backed golden model in float32 on AccumHostLib: (model, fixture arrays, host)."""
    import oracle_backend
    from flamingo_mini_amd import ffi, functional as F
    from test_model_plumbing import build
    group = F._wgrad_queue.group
    oracle_backend.uninstall()
    host_lib.install()                                      # (remembers what it replaces; uninstall() puts it back)
    host = AccumHostLib()
    ffi.lib = lambda: host
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: False)       # (raises without a device)
    model, z = build(torch.float32, "cpu", "gpt2")
    yield model.train(), z, host
    host_lib.uninstall()
    F._wgrad_queue.group = group


def _loss(model, z, rows):
    px = torch.from_numpy(z["px"])[rows].float()
    ids, ml = torch.from_numpy(z["ids"])[rows], torch.from_numpy(z["ml"])[rows]
    return model(input_ids=ids, attention_mask=torch.ones_like(ids), media_locations=ml, pixel_values=px, labels=ids).loss


def test_deferred_weight_gradients_survive_accumulation(accum_host):
    from flamingo_mini_amd import FusedAdamW
    model, z, host = accum_host
    named = {k: p for k, p in model.named_parameters() if p.requires_grad}
    params = list(named.values())
    n_hooks = len(model.flamingo.get_modified_layers())
    each = []
    for rows in ([0], [1]):                                  # the two micro-batches' own gradients (the host stand-in is deterministic)
        model.zero_grad(set_to_none=True)
        _loss(model, z, rows).backward()
        each.append({k: p.grad.detach().clone() for k, p in named.items()})

    # autograd accumulation: the second backward finds .grad in place and leaves the deferred path
    host.calls.clear()
    _loss(model, z, [0]).backward()
    assert "ff_xattn_block_bwd_kv_data" not in host.calls and host.calls.count("ff_xattn_block_bwd_kv") == n_hooks

    # accumulate(): .grad is None again, so the second backward defers and groups as the first did
    hp = dict(lr=1e-2, betas=(0.9, 0.95), eps=1e-6, weight_decay=0.05)
    opt = FusedAdamW(params, **hp)
    assert opt.accumulated_grad(params[0]) is None
    model.zero_grad(set_to_none=True)
    _loss(model, z, [0]).backward()
    opt.accumulate(0.5)
    assert all(p.grad is None for p in params)
    assert all(opt.accumulated_grad(p).dtype == torch.float32 and opt.accumulated_grad(p).shape == p.shape for p in params)
    host.calls.clear()
    _loss(model, z, [1]).backward()
    assert host.calls.count("ff_xattn_block_bwd_kv_data") == n_hooks and "ff_xattn_block_bwd_kv" not in host.calls
    grouped = [int(c.split("[")[1][:-1]) for c in host.calls if c.startswith("ff_xattn_wgrad_grouped")]
    assert grouped and sum(grouped) == n_hooks
    with pytest.raises(RuntimeError, match="not folded"):    # the second backward has not been folded yet: step() does not guess
        opt.step()
    with pytest.raises(ValueError, match="only"):
        opt.step(only={id(params[0])})
    host.calls.clear()
    opt.accumulate(0.5)
    assert host.calls == [f"ff_grad_accumulate[{len(params)},add]"]          # one call for the one (dtype, device); the first one overwrote
    assert all(p.grad is None for p in params)
    for k, p in named.items():                               # 0.5 a + 0.5 b: both products exact, one rounding
        assert torch.equal(opt.accumulated_grad(p), 0.5 * each[0][k] + 0.5 * each[1][k]), k
    before = {k: p.detach().clone() for k, p in named.items()}
    accs = {k: opt.accumulated_grad(p).clone() for k, p in named.items()}
    assert "step" not in opt.state.get(params[0], {})
    host.calls.clear()
    opt.step()
    assert [c.split("[")[0] for c in host.calls] == ["ff_adamw_step_acc"]
    assert all(opt.accumulated_grad(p) is None for p in params)             # the cycle is closed
    # ... and the update is torch.optim.AdamW's on the accumulated gradients
    twins = [torch.nn.Parameter(before[k].clone()) for k in named]
    for t, k in zip(twins, named):
        t.grad = accs[k].clone()
    ref = torch.optim.AdamW(twins, **hp)
    ref.step()
    for t, (k, p) in zip(twins, named.items()):
        assert torch.allclose(p, t, rtol=1e-5, atol=1e-7), k
    assert sum(not torch.equal(p, before[k]) for k, p in named.items()) >= len(named) // 2      # (a zero bias with a zero gradient stays)
    # state_dict: torch.optim.AdamW's keys, no accumulator in it
    sd, ref_sd = opt.state_dict(), ref.state_dict()
    assert set(sd) == set(ref_sd) == {"state", "param_groups"} and set(sd["state"]) == set(ref_sd["state"])
    for i, st in sd["state"].items():
        assert set(st) == set(ref_sd["state"][i]) == {"step", "exp_avg", "exp_avg_sq"} and float(st["step"]) == 1.0
    # a new cycle overwrites; reset_accumulation() drops it, and an ordinary step works afterwards
    _loss(model, z, [0]).backward()
    fresh = {k: p.grad.detach().clone() for k, p in named.items()}
    host.calls.clear()
    opt.accumulate(1.0)
    assert host.calls == [f"ff_grad_accumulate[{len(params)},overwrite]"]
    for k, p in named.items():
        assert torch.equal(opt.accumulated_grad(p), fresh[k]), k
    opt.reset_accumulation()
    assert all(opt.accumulated_grad(p) is None for p in params)
    opt.step()                                               # no cycle, no gradients: nothing to do, nothing raised
    assert float(opt.state_dict()["state"][0]["step"]) == 1.0


def test_graphed_step_refuses_micro_batches_it_cannot_run():
    """Raised in the constructor before the model is touched (neither model nor batch is usable here)."""
    from flamingo_mini_amd import FusedAdamW
    from flamingo_mini_amd.graphs import GraphedTrainStep
    opt = FusedAdamW([torch.nn.Parameter(torch.ones(3))], capturable=True)
    batch = dict(x=torch.zeros(4, 3), flag=True)
    with pytest.raises(ValueError, match="equal chunks"):
        GraphedTrainStep(object(), opt, batch, micro_batches=3)
    with pytest.raises(ValueError, match="reducer"):
        GraphedTrainStep(object(), opt, batch, micro_batches=2, reducer=object())
    with pytest.raises(ValueError, match="accumulate"):
        GraphedTrainStep(object(), torch.optim.AdamW([torch.nn.Parameter(torch.ones(3))]), batch, micro_batches=2)
    with pytest.raises(ValueError, match="micro_batches"):
        GraphedTrainStep(object(), opt, batch, micro_batches=0)
