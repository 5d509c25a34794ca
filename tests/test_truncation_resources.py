"""Registers, scratch and occupancy of csrc/ff_truncate.hip from the compiler's own remarks (tools/kernel_resources.py; build.py keeps them
per translation unit): the unit is reported with truncated_draw_kernel for bf16 staged, bf16 unstaged and fp32 and nothing else; none has
scratch - every functor handed to the row walks of ff_row_keys.h is inlined, the sums, the thresholds and the band live in registers -;
and the kernel's name is clear of the names the other resource tests count."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import kernel_resources  # noqa: E402

ROWS = kernel_resources.load()
pytestmark = pytest.mark.skipif(not ROWS, reason="library not built in this tree (no csrc/_obj/*.resources.txt)")
COUNTED = ("sample_token_kernel", "beam_rows_kernel", "logits_process_kernel", "token_logprob_kernel", "logits_constrain", "guided_logits_kernel", "shifted_ce_")


def test_the_unit_has_three_instantiations_without_scratch_and_a_name_of_its_own():
    mine = [r for r in ROWS if r["unit"] == "ff_truncate"]
    assert len(mine) == 3 and all("truncated_draw_kernel" in r["mangled"] for r in mine), [r["name"] for r in mine]
    for inst in ("IDF16bLb1E", "IDF16bLb0E", "IfLb0E"):                  # <__bf16, staged>, <__bf16, unstaged>, <float, unstaged>
        row = [r for r in mine if f"truncated_draw_kernel{inst}" in r["mangled"]]
        assert len(row) == 1, (inst, [r["mangled"] for r in mine])
        r = row[0]
        print(f"{r['name']}: {r['vgprs']} VGPRs, {r.get('sgprs', 0)} SGPRs, scratch {r['scratch']}, {r['occupancy']} waves/SIMD, static LDS {r.get('lds', 0)} bytes")
        assert r["scratch"] == 0, r
        assert r["vgprs"] + r.get("agprs", 0) <= 128, r                  # (one workgroup per CU runs; the figure only has to stay far from spilling)
    for other in COUNTED:
        assert not any(other in r["mangled"] for r in mine), other
    assert not any("truncated_draw_kernel" in r["mangled"] for r in ROWS if r["unit"] != "ff_truncate")
