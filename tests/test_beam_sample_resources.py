"""Registers, scratch and occupancy of csrc/ff_beam_sample.hip from the compiler's own remarks (tools/kernel_resources.py; build.py keeps them
per translation unit): the unit is reported with gumbel_rows_kernel for bf16 staged, bf16 unstaged and fp32, gumbel_merge_kernel and
gumbel_noise_kernel and nothing else; none has scratch - the Philox words and the functors handed to the row walks of ff_row_keys.h live
in registers through passes that recompute the noise of every column -; and the kernels' names are clear of the names the other resource
tests count."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import kernel_resources  # noqa: E402

ROWS = kernel_resources.load()
pytestmark = pytest.mark.skipif(not ROWS, reason="library not built in this tree (no csrc/_obj/*.resources.txt)")
COUNTED = ("sample_token_kernel", "beam_rows_kernel", "truncated_draw_kernel", "logits_process_kernel", "token_logprob_kernel", "logits_constrain",
           "guided_logits_kernel", "shifted_ce_", "beam_merge_kernel", "group_merge_kernel")


def test_the_unit_has_five_kernels_without_scratch_and_names_of_their_own():
    mine = [r for r in ROWS if r["unit"] == "ff_beam_sample"]
    assert len(mine) == 5 and len({r["mangled"] for r in mine}) == 5, [r["name"] for r in mine]
    for inst in ("gumbel_rows_kernelIDF16bLb1E", "gumbel_rows_kernelIDF16bLb0E", "gumbel_rows_kernelIfLb0E", "gumbel_merge_kernel", "gumbel_noise_kernel"):
        row = [r for r in mine if inst in r["mangled"]]              # <__bf16, staged>, <__bf16, unstaged>, <float, unstaged>, the merge, the noise
        assert len(row) == 1, (inst, [r["mangled"] for r in mine])
        r = row[0]
        print(f"{r['name']}: {r['vgprs']} VGPRs, {r.get('sgprs', 0)} SGPRs, scratch {r['scratch']}, {r['occupancy']} waves/SIMD, static LDS {r.get('lds', 0)} bytes")
        assert r["scratch"] == 0, r
        assert r["vgprs"] + r.get("agprs", 0) <= 128, r                  # (one workgroup per CU runs; the figure only has to stay far from spilling)
    for other in COUNTED:
        assert not any(other in r["mangled"] for r in mine), other
    assert not any("gumbel_" in r["mangled"] for r in ROWS if r["unit"] != "ff_beam_sample")


def test_the_beam_unit_keeps_its_kernels():
    """the walk moved into ff_beam_walk.h: ff_beam still reports its row pass three times and one kernel per merge, none with scratch"""
    mine = [r for r in ROWS if r["unit"] == "ff_beam"]
    for name, n in (("beam_rows_kernel", 3), ("beam_merge_kernel", 1), ("group_merge_kernel", 1)):
        rows = [r for r in mine if name in r["mangled"]]
        assert len(rows) == n and all(r["scratch"] == 0 for r in rows), (name, [(r["name"], r["scratch"]) for r in rows])
