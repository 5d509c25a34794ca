"""Stochastic rounding (FusedAdamW(stochastic_rounding=True)) without a GPU: argument validation, stream ids that belong to the parameter
and not to the bucket it lands in, a state_dict that keeps torch.optim.AdamW's layout, the routing of the one AdamW call site, and the
library's two new entry points rejecting bad arguments before any launch."""
import ctypes as C

import pytest
import torch

FF_ERR_SHAPE, FF_ERR_UNSUPPORTED = -1, -2


def _params(dtypes=(torch.bfloat16,) * 3):
    return [torch.nn.Parameter(torch.ones(4 + i, dtype=dt)) for i, dt in enumerate(dtypes)]


class RecordingLib:
    """Stands in for the library: every call is recorded as (name, args) and succeeds."""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def call(*args):
            self.calls.append((name, args))
            return 0
        return call


@pytest.fixture
def recorded(monkeypatch):
    from flamingo_mini_amd import ffi
    lib = RecordingLib()
    monkeypatch.setattr(ffi, "lib", lambda: lib)
    monkeypatch.setattr(ffi, "require_cuda", lambda *tensors: None)
    monkeypatch.setattr(ffi, "stream_handle", lambda device: None)
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: False)       # (raises without a device)
    return lib


def test_constructor_errors():
    from flamingo_mini_amd import FusedAdamW
    with pytest.raises(ValueError, match="master_dtype"):
        FusedAdamW(_params(), stochastic_rounding=True, master_dtype=torch.float32)
    for bad in (-1, 2 ** 64):
        with pytest.raises(ValueError, match="sr_seed"):
            FusedAdamW(_params(), stochastic_rounding=True, sr_seed=bad)
    opt = FusedAdamW(_params(), stochastic_rounding=True, sr_seed=2 ** 64 - 1, state_dtype=torch.float32)      # fp32 moments go with it
    assert opt.stochastic_rounding and opt.sr_seed == 2 ** 64 - 1
    assert not FusedAdamW(_params()).stochastic_rounding
    from flamingo_mini_amd.data_parallel import ShardedAdamW
    with pytest.raises(TypeError):
        ShardedAdamW(torch.nn.Linear(2, 2), stochastic_rounding=True)


def test_state_dict_layout_is_unchanged():
    from flamingo_mini_amd import FusedAdamW
    a, b = FusedAdamW(_params(), lr=1e-3), FusedAdamW(_params(), lr=1e-3, stochastic_rounding=True, sr_seed=7)
    sa, sb = a.state_dict(), b.state_dict()
    assert sa["param_groups"] == sb["param_groups"] and sa["state"] == sb["state"] == {}
    assert all("stochastic_rounding" not in g and "sr_seed" not in g for g in sb["param_groups"])
    b.load_state_dict(torch.optim.AdamW(_params(), lr=1e-3).state_dict())
    assert b.stochastic_rounding and b.sr_seed == 7


def _sr_calls(lib):
    """[(stream ids, parameter pointers)] of the recorded ff_adamw_step_sr calls"""
    out = []
    for name, args in lib.calls:
        if name == "ff_adamw_step_sr":
            n = args[0].n_tensors
            out.append(([int(args[11][i]) for i in range(n)], [int(args[2][i]) for i in range(n)]))
    return out


def test_stream_ids_belong_to_the_parameter_whatever_the_bucketing(recorded):
    """The id is the ordinal in param_groups order, fixed at construction: the same in a full step, when a parameter has no gradient,
    under step(only=...) in any partition, under accumulate(), and in a second optimizer built alike; fp32 parameters keep their calls."""
    from flamingo_mini_amd import FusedAdamW
    ps = _params((torch.bfloat16, torch.float32, torch.bfloat16, torch.bfloat16, torch.bfloat16))
    groups = [dict(params=ps[:2]), dict(params=ps[2:], lr=2e-3)]
    opt = FusedAdamW(groups, capturable=True, stochastic_rounding=True, sr_seed=11)
    want = {p.data_ptr(): i for i, p in enumerate(ps)}
    assert [opt._sr_ids[p] for p in ps] == list(range(5))
    assert [FusedAdamW(groups, stochastic_rounding=True)._sr_ids[p] for p in ps] == list(range(5))

    def grads(which):
        for i, p in enumerate(ps):
            p.grad = torch.ones_like(p) if i in which else None

    def seen():
        calls = _sr_calls(recorded)
        pairs = [(ptr, sid) for ids, ptrs in calls for ptr, sid in zip(ptrs, ids)]
        assert all(want[ptr] == sid for ptr, sid in pairs), pairs
        other = [name for name, _ in recorded.calls if name.startswith("ff_adamw_step") and name != "ff_adamw_step_sr"]
        recorded.calls.clear()
        return sorted(sid for _, sid in pairs), other

    grads({0, 1, 2, 3, 4})
    opt.step()
    assert seen() == ([0, 2, 3, 4], ["ff_adamw_step_mixed"])          # the fp32 parameter (ordinal 1) is updated as without the feature
    grads({2, 4})                                                      # another bucketing: the first table entry is now parameter 2
    opt.step()
    assert seen() == ([2, 4], [])
    grads({0, 2, 3, 4})
    opt.step(only={id(ps[4]), id(ps[0])}, advance=True)
    assert seen() == ([0, 4], [])
    opt.step(only={id(ps[2]), id(ps[3])}, advance=False)
    assert seen() == ([2, 3], [])
    grads({0, 3})
    opt.accumulate(1.0)
    opt.step()
    calls = [args for name, args in recorded.calls if name == "ff_adamw_step_sr"]
    assert [int(a[4]) for a in calls] == [1, 1]                        # grads_fp32: the accumulators
    assert seen() == ([0, 3], [])
    opt.add_param_group(dict(params=_params((torch.bfloat16,))))       # a later group continues the count
    assert list(opt._sr_ids.values()) == list(range(6))


def test_the_call_site_routes_to_the_sr_entry_point(recorded):
    from flamingo_mini_amd import ffi
    from flamingo_mini_amd.optim import adamw_step_call
    desc = ffi.AdamWDesc(ffi.DTYPE_BF16, 2, 1, 1e-3, 0.9, 0.999, 1e-8, 0.0, 1.0, None)
    ids = (C.c_uint * 2)(3, 9)
    ptrs = ("p", "g", "m", "v", None, "numels")
    coef, skip = torch.ones(()), torch.zeros(())
    adamw_step_call(recorded, desc, ffi.DTYPE_BF16, ptrs, "lr", None, None, False, "stream", sr=(5, ids))
    adamw_step_call(recorded, desc, ffi.DTYPE_F32, ptrs, None, coef, None, True, "stream", sr=(2 ** 64 - 2, ids))
    adamw_step_call(recorded, desc, ffi.DTYPE_BF16, ptrs, None, coef, skip, False, "stream", sr=(2 ** 63, ids))
    assert [n for n, _ in recorded.calls] == ["ff_adamw_step_sr"] * 3
    a, b, c = (args for _, args in recorded.calls)
    assert a == (desc, ffi.DTYPE_BF16, "p", "g", 0, "m", "v", "lr", None, None, 5, ids, "numels", "stream")
    assert b[1] == ffi.DTYPE_F32 and b[4] == 1 and b[8:11] == (coef.data_ptr(), None, -2)                 # the seed's 64 bits as a long long
    assert c[8:11] == (coef.data_ptr(), skip.data_ptr(), -2 ** 63)
    with pytest.raises(ffi.FusionLibraryError, match="master"):
        adamw_step_call(recorded, desc, ffi.DTYPE_F32, ("p", "g", "m", "v", "w", "numels"), None, None, None, False, "stream", sr=(5, ids))
    recorded.calls.clear()                                             # without sr the four earlier entry points, as before
    adamw_step_call(recorded, desc, ffi.DTYPE_BF16, ptrs, None, None, None, False, "stream")
    adamw_step_call(recorded, desc, ffi.DTYPE_BF16, ptrs, None, coef, None, False, "stream")
    adamw_step_call(recorded, desc, ffi.DTYPE_BF16, ptrs, None, None, None, True, "stream")
    adamw_step_call(recorded, desc, ffi.DTYPE_BF16, ptrs, None, coef, skip, False, "stream")
    assert [n for n, _ in recorded.calls] == ["ff_adamw_step_mixed", "ff_adamw_step_clipped", "ff_adamw_step_acc", "ff_adamw_step_guarded"]


def test_entry_points_reject_bad_arguments_before_any_launch():
    from flamingo_mini_amd import ffi
    lib = ffi.lib()
    none = ffi.ptr_array([None])
    numels = (C.c_longlong * 1)(0)
    ids = (C.c_uint * 1)(0)

    def desc(dtype, n=0):
        return ffi.AdamWDesc(dtype, n, 1, 1e-3, 0.9, 0.999, 1e-8, 0.0, 1.0, None)

    def sr(d, state, stream_ids, coef=None, skip=None):
        return lib.ff_adamw_step_sr(d, state, none, none, 0, none, none, None, coef, skip, 0, stream_ids, numels, None)

    assert sr(desc(ffi.DTYPE_BF16), ffi.DTYPE_BF16, ids) == 0 and sr(desc(ffi.DTYPE_BF16), ffi.DTYPE_F32, ids) == 0      # no tensors: nothing launched
    assert sr(desc(ffi.DTYPE_F32), ffi.DTYPE_F32, ids) == FF_ERR_UNSUPPORTED                   # fp32 parameters round to nothing
    assert b"bf16" in lib.ff_last_error()
    assert sr(desc(ffi.DTYPE_BF16), ffi.DTYPE_BF16, None) == FF_ERR_SHAPE                      # null stream_ids
    assert sr(desc(ffi.DTYPE_BF16, 1), ffi.DTYPE_BF16, (C.c_uint * 1)(2 ** 30)) == FF_ERR_SHAPE
    assert b"2^30" in lib.ff_last_error()
    assert sr(desc(ffi.DTYPE_BF16), ffi.DTYPE_BF16, ids, skip=C.c_void_p(16)) == FF_ERR_SHAPE  # a verdict without a coefficient
    assert sr(desc(ffi.DTYPE_BF16), 5, ids) == FF_ERR_UNSUPPORTED                              # moments in an unknown type
    one = (C.c_longlong * 1)(4)                                                                # a non-empty tensor without pointers
    assert lib.ff_adamw_step_sr(desc(ffi.DTYPE_BF16, 1), ffi.DTYPE_BF16, none, none, 0, none, none, None, None, None, 0, ids, one, None) == FF_ERR_SHAPE
    rnd = lib.ff_stochastic_round_bf16
    assert rnd(None, None, 0, 0, 0, 0, 0, None) == 0                                           # nothing to round
    assert rnd(None, None, 8, 0, 0, 0, 0, None) == FF_ERR_SHAPE
    assert rnd(C.c_void_p(16), C.c_void_p(16), 8, 0, 2 ** 30, 0, 0, None) == FF_ERR_SHAPE
    assert rnd(C.c_void_p(16), C.c_void_p(16), 8, 0, 0, 0, 4, None) == FF_ERR_SHAPE
    assert rnd(C.c_void_p(16), C.c_void_p(16), -1, 0, 0, 0, 0, None) == FF_ERR_SHAPE


def test_functional_round_validates_its_arguments():
    from flamingo_mini_amd import ffi, functional as F
    with pytest.raises(ffi.FusionLibraryError):
        F.stochastic_round_bf16(torch.ones(8))                                                # a CPU tensor: no fallback
