"""Beam search on the static decode path, without a GPU: the two entry points are bound and reject bad arguments with their error codes
before anything reaches a device, the ctypes mirror of ff_beam_desc matches the header, static beam search refuses CPU tensors - and the
numpy restatement of the kernel's rules (tests/beam_cases.py) plus _beam_finalize IS the old behaviour: driven by the same scripted logits as
the unmodified FlamingoModel._beam_search, it returns the same ids token for token."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

import beam_cases as BC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FF_ERR_SHAPE, FF_ERR_UNSUPPORTED = -1, -2
X = 256                        # a non-null pointer that is never dereferenced: every call below fails its checks first
STATE = ("score", "done", "n_hyp", "hyp_score", "hyp_len", "hyp_row", "hist_tok", "hist_parent", "hist_score", "next_tok", "beam_idx", "len_norm")


def _step(logits=X, cur_len=X, ws=X, ws_bytes=1 << 20, null_desc=False, **over):
    from flamingo_mini_amd import ffi
    f = dict(dtype=ffi.DTYPE_BF16, b=2, nb=3, vocab=100, ld=100, max_len=16, eos=-1, pad=0, early_stopping=1, **{n: X for n in STATE})
    f.update(over)
    d = ffi.BeamDesc(**f)
    return ffi.lib().ff_beam_step(None if null_desc else C.byref(d), logits, cur_len, ws, ws_bytes, None)


def _gather(n_tensors=2, tensors=True, elem_size=2, b=2, nb=3, outer=4, len_max=8, inner=16, beam_idx=X, n_pos=X, null_entry=False):
    from flamingo_mini_amd import ffi
    arr = (C.c_void_p * 2)(X, None if null_entry else X)
    return ffi.lib().ff_beam_gather(n_tensors, arr if tensors else None, elem_size, b, nb, outer, len_max, inner, beam_idx, n_pos, None)


def test_the_entry_points_are_bound():
    from flamingo_mini_amd import ffi, functional as F
    assert {"ff_beam_step", "ff_beam_gather", "ff_beam_workspace_bytes"} <= set(ffi.EXPORTED_SYMBOLS) and ffi.lib().ff_version() == 6
    assert callable(F.beam_step) and callable(F.beam_gather) and ffi.BEAM_MAX == 8
    assert ffi.lib().ff_beam_workspace_bytes(4, 3) == 4 * 3 * 6 * 8 and ffi.lib().ff_beam_workspace_bytes(4, 9) == 0


@pytest.mark.parametrize("bad", [
    dict(null_desc=True), dict(logits=None), dict(cur_len=None), dict(ws=None), *[{n: None} for n in STATE],
    dict(b=0), dict(b=-1), dict(nb=0), dict(nb=9), dict(vocab=5), dict(ld=99), dict(max_len=0), dict(ws_bytes=2 * 3 * 6 * 8 - 1),
], ids=lambda d: "-".join(f"{k}={v}" for k, v in d.items()))
def test_beam_step_argument_errors_return_shape_before_any_launch(bad):
    from flamingo_mini_amd import ffi
    assert _step(**bad) == FF_ERR_SHAPE
    assert b"ff_beam_step" in ffi.lib().ff_last_error()


@pytest.mark.parametrize("bad", [
    dict(tensors=False), dict(beam_idx=None), dict(n_pos=None), dict(null_entry=True), dict(n_tensors=0), dict(b=0), dict(nb=0), dict(nb=9),
    dict(outer=0), dict(len_max=0), dict(inner=0),
], ids=lambda d: "-".join(f"{k}={v}" for k, v in d.items()))
def test_beam_gather_argument_errors_return_shape_before_any_launch(bad):
    from flamingo_mini_amd import ffi
    assert _gather(**bad) == FF_ERR_SHAPE
    assert b"ff_beam_gather" in ffi.lib().ff_last_error()


def test_other_dtypes_and_element_sizes_are_unsupported():
    from flamingo_mini_amd import ffi
    assert _step(dtype=7) == FF_ERR_UNSUPPORTED and b"dtype" in ffi.lib().ff_last_error()
    for size in (1, 8):
        assert _gather(elem_size=size) == FF_ERR_UNSUPPORTED and b"ff_beam_gather" in ffi.lib().ff_last_error()


def test_beam_desc_layout_matches_the_header(tmp_path):
    """ff_beam_desc is declared struct-then-typedef in the header; its ctypes mirror is held to it here: names, order, offsets, sizes."""
    from flamingo_mini_amd import ffi
    gcc = shutil.which("gcc")
    if gcc is None:
        pytest.skip("no gcc")
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "flamingo_fusion.h")).read(), flags=re.S)
    body = re.search(r"struct\s+ff_beam_desc\s*\{(.*?)\}\s*;", text, flags=re.S).group(1)
    fields = []
    for decl in body.split(";"):
        decl = " ".join(decl.split())
        if decl:
            names = decl.replace("*", " ").split(",")
            fields += [names[0].split()[-1]] + [n.strip() for n in names[1:]]
    assert [f[0] for f in ffi.BeamDesc._fields_] == fields
    lines = ["#include <stdio.h>", "#include <stddef.h>", '#include "flamingo_fusion.h"', "int main(void) {",
             '  printf(". %zu %d\\n", sizeof(ff_beam_desc), FF_BEAM_MAX);']
    lines += [f'  printf("{f} %zu %zu\\n", offsetof(ff_beam_desc, {f}), sizeof(((ff_beam_desc*)0)->{f}));' for f in fields] + ["  return 0;", "}"]
    (tmp_path / "layout.c").write_text("\n".join(lines))
    subprocess.run([gcc, "-std=c11", "-I", os.path.join(ROOT, "include"), str(tmp_path / "layout.c"), "-o", str(tmp_path / "layout")], check=True)
    for line in subprocess.run([str(tmp_path / "layout")], check=True, capture_output=True, text=True).stdout.strip().splitlines():
        name, a, b = line.split()
        if name == ".":
            assert (C.sizeof(ffi.BeamDesc), ffi.BEAM_MAX) == (int(a), int(b))
        else:
            fld = getattr(ffi.BeamDesc, name)
            assert (fld.offset, fld.size) == (int(a), int(b)), (name, fld.offset, fld.size, a, b)


def test_beam_kernels_have_no_cpu_form():
    from flamingo_mini_amd import ffi, functional as F
    with pytest.raises(ffi.FusionLibraryError, match="no CPU fallback"):
        F.beam_step(torch.zeros(6, 20), None, torch.zeros(1, dtype=torch.long))
    with pytest.raises(ffi.FusionLibraryError, match="no CPU fallback"):
        F.beam_gather([torch.zeros(6, 2, 4, 8)], torch.arange(6), torch.zeros(1, dtype=torch.long), 3)
    with pytest.raises(ffi.FusionLibraryError, match="no CPU fallback"):
        F.BeamState(2, 3, 8, "cpu")


@pytest.mark.parametrize("family", ["gpt2", "opt"])
def test_routing_on_the_host(family):
    """num_beams=3 with static_decode=True on CPU tensors raises what ffi.require_cuda raises and builds no session (before the feature it
    silently ran the dynamic loop); without the flag, or with static_decode=False, the dynamic loop runs and returns the same ids."""
    import oracle_backend
    from flamingo_mini_amd import ffi
    from test_model_plumbing import build
    oracle_backend.install()
    try:
        model, z = build(torch.float64, "cpu", family)
        model.eval()
        px = torch.from_numpy(z["px"]).double()
        ids, ml = torch.from_numpy(z["ids"])[:, :4], torch.from_numpy(z["ml"])[:, :4]
        kw = dict(media_locations=ml, attention_mask=torch.ones_like(ids), pixel_values=px, max_length=8, num_beams=3)
        with pytest.raises(ffi.FusionLibraryError, match="no CPU fallback"):
            model.generate(ids, static_decode=True, **kw)
        assert len(model._decode_sessions) == 0
        got, also = model.generate(ids, **kw), model.generate(ids, static_decode=False, **kw)
        assert len(model._decode_sessions) == 0 and got.shape[0] == ids.shape[0] and torch.equal(got, also)
    finally:
        oracle_backend.uninstall()


# ---- the restatement is the old behaviour ----------------------------------------------------------------------------------------------
V, NB, L0, MAXLEN, EOS, PAD = 40, 3, 2, 14, 7, 0
PROMPT = np.array([[1, 11], [2, 12], [3, 13]], np.int64)
# sequence "1" is pushed to eos from length 4 on (finishes early), "2" gets a mild push from length 6 (eos shows up at high ranks), "3" none
BOOST = {1: (4, 9.0), 2: (6, 5.5)}
CASES = [  # (early_stopping, length_penalty, eos, seed of the logits table: one whose run keeps every margin >= 1e-3 and holds the events)
    (True, 1.0, EOS, 8), (False, 1.0, EOS, 29), (True, 0.6, EOS, 58), (False, 0.6, EOS, 61), (True, 2.0, EOS, 83), (False, 2.0, EOS, 102),
    (True, 1.0, None, 121), (False, 2.0, None, 142),
]


def _run(early, lp, eos, seed):
    script, ev = BC.Script(V, seed, eos=eos, eos_boost=BOOST), {}
    st, worst = BC.run_restatement(script, PROMPT, NB, MAXLEN, eos, PAD, early, lp, events=ev)
    ev["early_done"] = int(st["done"].any() and st["length"] > int(st["hyp_len"][st["done"] == 1].max(initial=0)))
    ev["ran_out"] = int((st["done"] == 0).any() and st["length"] == MAXLEN)
    return script, st, worst, ev


@pytest.mark.parametrize("early,lp,eos,seed", CASES)
def test_restatement_and_finalize_equal_the_dynamic_beam_search(early, lp, eos, seed):
    from flamingo_mini_amd.modeling_flamingo import _beam_finalize
    script, st, worst, _ = _run(early, lp, eos, seed)
    assert worst >= 1e-3, f"the script is not decidable: consecutive candidate scores {worst:.2e} apart"
    want = _beam_finalize(st, L0, PROMPT, NB, PAD)
    ids = torch.from_numpy(PROMPT)
    got = BC.ScriptedModel(script).search(ids, torch.zeros_like(ids), torch.ones_like(ids), None, None, MAXLEN, NB, eos, PAD, early, lp)
    assert got.shape == want.shape and torch.equal(got, want), (got.tolist(), want.tolist())


def test_the_scripts_cover_the_events():
    """eos at rank < nb and at rank >= nb, a sequence done early while another runs to the length limit in one and the same run, and runs
    without any eos (nothing finishes)."""
    events = {c: _run(*c)[3] for c in CASES}
    tot = {k: sum(e.get(k, 0) for e in events.values()) for k in ("eos_low", "eos_high", "done", "early_done", "ran_out")}
    print(tot)
    assert all(v > 0 for v in tot.values()), tot
    assert any(e.get("early_done") and e.get("ran_out") for e in events.values()), events
    assert all(not e.get("done") and not e.get("eos_low") and e.get("ran_out") for c, e in events.items() if c[2] is None)
