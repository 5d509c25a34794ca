"""Diverse beam search without a GPU: ff_group_beam_step is bound, its ctypes signature is the header's, it rejects bad arguments with their
error codes before anything reaches a device; generate() rejects the argument combinations the rules exclude; static decoding refuses CPU
tensors; and a call WITHOUT groups builds the session key and the session arguments it always built."""
import ctypes as C

import numpy as np
import pytest
import torch

FF_ERR_SHAPE, FF_ERR_UNSUPPORTED = -1, -2
X = 256                        # a non-null pointer that is never dereferenced: every call below fails its checks first
STATE = ("score", "done", "n_hyp", "hyp_score", "hyp_len", "hyp_row", "hist_tok", "hist_parent", "hist_score", "next_tok", "beam_idx", "len_norm")


def _step(logits=X, cur_len=X, ws=X, ws_bytes=1 << 20, null_desc=False, n_groups=2, lam=0.5, **over):
    from flamingo_mini_amd import ffi
    f = dict(dtype=ffi.DTYPE_BF16, b=2, nb=4, vocab=100, ld=100, max_len=16, eos=-1, pad=0, early_stopping=1, **{n: X for n in STATE})
    f.update(over)
    d = ffi.BeamDesc(**f)
    return ffi.lib().ff_group_beam_step(None if null_desc else C.byref(d), n_groups, lam, logits, cur_len, ws, ws_bytes, None)


def test_the_entry_point_is_bound_and_the_abi_is_6():
    from flamingo_mini_amd import ffi, functional as F
    assert "ff_group_beam_step" in ffi.EXPORTED_SYMBOLS and hasattr(ffi.lib(), "ff_group_beam_step") and ffi.lib().ff_version() == 6
    assert callable(F.group_beam_step)


def test_ctypes_signature_matches_the_header():
    """ff_beam_step's arguments with (int n_groups, float diversity_penalty) behind the descriptor"""
    from flamingo_mini_amd import ffi
    from test_cabi import _header_prototypes
    protos = _header_prototypes()
    plain = protos["ff_beam_step"][1]
    assert protos["ff_group_beam_step"] == ("int", plain[:1] + ["int", "float"] + plain[1:])
    res, args = ffi._SIGNATURES["ff_group_beam_step"]
    want = ffi._SIGNATURES["ff_beam_step"][1]
    assert res is C.c_int and args == want[:1] + [C.c_int, C.c_float] + want[1:]


@pytest.mark.parametrize("bad", [
    dict(null_desc=True), dict(logits=None), dict(cur_len=None), dict(ws=None), *[{n: None} for n in STATE],
    dict(b=0), dict(b=-1), dict(nb=0), dict(nb=9), dict(vocab=7), dict(ld=99), dict(max_len=0), dict(ws_bytes=2 * 4 * 8 * 8 - 1),
    dict(n_groups=0), dict(n_groups=-2), dict(n_groups=3), dict(nb=6, n_groups=4), dict(n_groups=8),
    dict(lam=-0.5), dict(lam=float("nan")), dict(lam=float("inf")), dict(lam=-float("inf")), dict(n_groups=1, lam=-1.0),
], ids=lambda d: "-".join(f"{k}={v}" for k, v in d.items()))
def test_argument_errors_return_shape_before_any_launch(bad):
    from flamingo_mini_amd import ffi
    assert _step(**bad) == FF_ERR_SHAPE
    assert b"ff_group_beam_step" in ffi.lib().ff_last_error()


def test_other_dtypes_are_unsupported():
    from flamingo_mini_amd import ffi
    assert _step(dtype=7) == FF_ERR_UNSUPPORTED and b"ff_group_beam_step" in ffi.lib().ff_last_error()


def test_the_kernels_have_no_cpu_form_and_the_state_checks_its_groups():
    from flamingo_mini_amd import ffi, functional as F
    with pytest.raises(ffi.FusionLibraryError, match="no CPU fallback"):
        F.group_beam_step(torch.zeros(8, 20), None, torch.zeros(1, dtype=torch.long), 0.5)
    with pytest.raises(ffi.FusionLibraryError, match="no CPU fallback"):
        F.BeamState(2, 4, 8, "cpu", n_groups=2)
    for bad in (0, 3, -1, 2.0, True):
        with pytest.raises(ValueError, match="n_groups"):
            F.BeamState(2, 4, 8, "cpu", n_groups=bad)
    assert F.BeamState.nbytes(3, 4, 9, 1) == F.BeamState.nbytes(3, 4, 9) and F.BeamState._layout(3, 4, 9, 1) == F.BeamState._layout(3, 4, 9)
    shapes = {n: s for n, s, *_ in F.BeamState._layout(3, 4, 9, 2)[0]}
    assert shapes["done"] == (3, 2) and shapes["n_hyp"] == (3, 2) and shapes["hyp_score"] == (3, 4)


def test_check_group_args():
    from flamingo_mini_amd import decoding as D
    assert D.check_group_args(1, 0.0, 1, False) is None and D.check_group_args(1, 0, 5, True) is None
    g = D.check_group_args(4, 1, 4, False)
    assert g == (4, 1.0) and isinstance(g, D.Groups) and isinstance(g.diversity_penalty, float)
    assert D.check_group_args(2, 0.0, 6, False) == D.Groups(2, 0.0)
    assert D.Beams._fields == ("nb", "early_stopping", "length_penalty")
    for G, lam, nb, sample in ((0, 0.0, 4, False), (-1, 0.0, 4, False), (2.0, 0.0, 4, False), (True, 0.0, 4, False), ("2", 0.0, 4, False),
                               (3, 0.5, 4, False), (2, 0.5, 1, False), (2, 0.5, 4, True), (2, -0.5, 4, False), (2, float("nan"), 4, False),
                               (2, float("inf"), 4, False), (2, "1", 4, False), (1, 0.5, 4, False), (1, 0.5, 1, False)):
        with pytest.raises(ValueError):
            D.check_group_args(G, lam, nb, sample)


@pytest.fixture(scope="module")
def cpu_model():
    import oracle_backend
    from test_model_plumbing import build
    oracle_backend.install()
    try:
        model, z = build(torch.float64, "cpu", "gpt2")
        model.eval()
        ids, ml = torch.from_numpy(z["ids"])[:, :4], torch.from_numpy(z["ml"])[:, :4]
        yield model, ids, dict(media_locations=ml, attention_mask=torch.ones_like(ids), pixel_values=torch.from_numpy(z["px"]).double(), max_length=8)
    finally:
        oracle_backend.uninstall()


@pytest.mark.parametrize("kw,match", [
    (dict(num_beams=4, num_beam_groups=0), "num_beam_groups"), (dict(num_beams=4, num_beam_groups=2.0), "num_beam_groups"),
    (dict(num_beams=4, num_beam_groups=3), "multiple"), (dict(num_beams=1, num_beam_groups=2), "multiple"),
    (dict(num_beams=4, num_beam_groups=2, do_sample=True), "do_sample"),
    (dict(num_beams=4, num_beam_groups=2, diversity_penalty=-1.0), "diversity_penalty"),
    (dict(num_beams=4, num_beam_groups=2, diversity_penalty=float("nan")), "diversity_penalty"),
    (dict(num_beams=4, num_beam_groups=2, diversity_penalty=float("inf")), "diversity_penalty"),
    (dict(num_beams=4, num_beam_groups=1, diversity_penalty=0.5), "num_beam_groups > 1"),
], ids=lambda v: "-".join(f"{k}={x}" for k, x in v.items()) if isinstance(v, dict) else None)
def test_generate_rejects_what_the_rules_exclude(cpu_model, kw, match):
    model, ids, base = cpu_model
    with pytest.raises(ValueError, match=match):
        model.generate(ids, **base, **kw)


def test_generate_on_cpu_tensors(cpu_model):
    """static_decode=True raises what ffi.require_cuda raises and builds no session; without it the dynamic loop runs diverse beam search:
    rows s * n + j with sorted scores, G = 1 is the plain call, and a large penalty makes the groups' first tokens differ."""
    from flamingo_mini_amd import ffi
    model, ids, base = cpu_model
    kw = dict(base, num_beams=4, num_beam_groups=4, diversity_penalty=50.0)
    with pytest.raises(ffi.FusionLibraryError, match="no CPU fallback"):
        model.generate(ids, static_decode=True, **kw)
    assert len(model._decode_sessions) == 0
    out = model.generate(ids, num_return_sequences=4, return_dict_in_generate=True, **kw)
    b, L0 = ids.shape
    assert out.sequences.shape[0] == 4 * b and torch.equal(out.sequences[:, :L0], ids.repeat_interleave(4, 0))
    s = out.sequences_scores.reshape(b, 4)
    assert bool(torch.isfinite(s).all()) and bool((s[:, :-1] >= s[:, 1:]).all())
    first = out.sequences[:, L0].reshape(b, 4)
    assert all(len(set(r)) == 4 for r in first.tolist()), first.tolist()
    assert torch.equal(model.generate(ids, **base, num_beams=4, num_beam_groups=1), model.generate(ids, **base, num_beams=4))
    assert len(model._decode_sessions) == 0


def test_route_and_the_session_key_without_groups_are_what_they_were(monkeypatch):
    """route() takes no group argument (routing is that of beams).  _static_decode is run with a stand-in session class: without groups the
    key is the ten elements it always was and the session is built without a `groups` argument; with groups the key gains the trailing
    Groups and the session receives them."""
    import inspect
    from flamingo_mini_amd import decoding as D
    assert "groups" not in inspect.signature(D.route).parameters and "num_beam_groups" not in inspect.signature(D.route).parameters
    common = dict(do_sample=False, model_default=True, lm_family="gpt2", L0=4, max_length=16, ids_is_int64=True, procs_on=False)
    assert D.route(is_cuda=True, num_beams=4, static_decode=True, **common) == "static"
    assert D.route(is_cuda=True, num_beams=4, static_decode=None, **common) == "dynamic"
    assert D.route(is_cuda=False, num_beams=4, static_decode=None, **common) == "dynamic"

    built = []

    class Session:
        def __init__(self, *a, **kw):
            built.append(kw)

        def stale(self):
            return False

        def run(self, *a, **kw):
            return "ran"

    class Model:
        training, decode_graph = False, True

    monkeypatch.setattr(D, "_BeamSession", Session)
    model, ids = Model(), torch.zeros((2, 4), dtype=torch.long)
    args = (model, ids, torch.zeros_like(ids), torch.ones_like(ids), None, torch.zeros(2, 3, 8), 16, 7, 0)
    beams = D.Beams(4, True, 1.0)
    assert D._static_decode(*args, beams=beams) == "ran"
    assert list(D._DECODE_SESSIONS[model]) == [(2, 16, 3, "cpu", 7, 0, False, None, (4, True, 1.0), None)]
    assert "groups" not in built[0] and built[0]["beams"] == (4, True, 1.0)
    assert D._static_decode(*args, beams=beams, groups=D.Groups(2, 0.5)) == "ran"
    keys = list(D._DECODE_SESSIONS[model])
    assert keys[1] == keys[0] + ((2, 0.5),) and isinstance(keys[1][-1], D.Groups)
    assert built[1]["groups"] == D.Groups(2, 0.5)
    assert D._static_decode(*args, beams=beams, groups=D.Groups(2, 0.5)) == "ran" and len(built) == 2           # the same key: the session is reused
    assert D._static_decode(*args, beams=beams, groups=D.Groups(2, 1.0)) == "ran" and len(built) == 3           # the penalty is a launch constant


def test_the_group_walk_is_one_kernel_without_scratch_and_the_row_pass_is_shared():
    """group_merge_kernel is the only kernel the feature adds: reported once, no scratch (its tables live in LDS), and no further
    instantiation of the row pass, which tests/test_kernel_resources.py counts by name."""
    import os
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
    import kernel_resources
    rows = kernel_resources.load()
    if not rows:
        pytest.skip("library not built in this tree (no csrc/_obj/*.resources.txt)")
    mine = [r for r in rows if "group_merge_kernel" in r["mangled"]]
    assert len(mine) == 1 and mine[0]["unit"] == "ff_beam" and mine[0]["scratch"] == 0, mine
    assert "beam_rows_kernel" not in mine[0]["mangled"] and "sample_token_kernel" not in mine[0]["mangled"]
    assert sum("beam_rows_kernel" in r["mangled"] for r in rows) == 3 and sum("beam_merge_kernel" in r["mangled"] for r in rows) == 1
