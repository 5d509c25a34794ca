"""Registers, scratch and occupancy of csrc/ff_contrastive.hip from the compiler's own remarks (tools/kernel_resources.py; build.py keeps them
per translation unit): the unit is reported with contrastive_topk_kernel for bf16 staged, bf16 unstaged and fp32, contrastive_step_kernel
for bf16 and fp32, each with 16-byte vectors and element by element, and nothing else; none has scratch - the functors handed to the row
walks of ff_row_keys.h and the step kernel's 2 x 8 dot-product accumulators live in registers -; and the kernels' names are clear of the
names the other resource tests count."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import kernel_resources  # noqa: E402

ROWS = kernel_resources.load()
pytestmark = pytest.mark.skipif(not ROWS, reason="library not built in this tree (no csrc/_obj/*.resources.txt)")
COUNTED = ("sample_token_kernel", "beam_rows_kernel", "truncated_draw_kernel", "logits_process_kernel", "token_logprob_kernel", "logits_constrain",
           "guided_logits_kernel", "shifted_ce_", "beam_merge_kernel", "group_merge_kernel", "gumbel_")


def test_the_unit_has_seven_kernels_without_scratch_and_names_of_their_own():
    mine = [r for r in ROWS if r["unit"] == "ff_contrastive"]
    assert len(mine) == 7 and len({r["mangled"] for r in mine}) == 7, [r["name"] for r in mine]
    for inst in ("contrastive_topk_kernelIDF16bLb1E", "contrastive_topk_kernelIDF16bLb0E", "contrastive_topk_kernelIfLb0E",
                 "contrastive_step_kernelIDF16bLb1E", "contrastive_step_kernelIDF16bLb0E", "contrastive_step_kernelIfLb1E", "contrastive_step_kernelIfLb0E"):
        row = [r for r in mine if inst in r["mangled"]]
        assert len(row) == 1, (inst, [r["mangled"] for r in mine])
        r = row[0]
        print(f"{r['name']}: {r['vgprs']} VGPRs, {r.get('sgprs', 0)} SGPRs, scratch {r['scratch']}, {r['occupancy']} waves/SIMD, static LDS {r.get('lds', 0)} bytes")
        assert r["scratch"] == 0, r
        assert r["vgprs"] + r.get("agprs", 0) <= 128, r                  # (one workgroup per CU runs; the figure only has to stay far from spilling)
    assert all(r["mangled"].startswith("_ZN2ff12contrastive_") or "contrastive_" in r["mangled"] for r in mine)
    for other in COUNTED:
        assert not any(other in r["mangled"] for r in mine), other
    assert not any("contrastive_" in r["mangled"] for r in ROWS if r["unit"] != "ff_contrastive")


def test_the_row_units_keep_their_kernels():
    """ff_row_keys.h is reused, not beam_rows_kernel: ff_beam still reports its row pass exactly three times in the whole library"""
    assert len([r for r in ROWS if "beam_rows_kernel" in r["mangled"]]) == 3
    assert len([r for r in ROWS if "gumbel_rows_kernel" in r["mangled"]]) == 3
