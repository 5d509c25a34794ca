"""Registers, scratch and occupancy of csrc/ff_score.hip from the compiler's own remarks (tools/kernel_resources.py; build.py keeps them
per translation unit): the unit is reported, with logprob_gather_kernel for bf16 and for fp32 and nothing else; neither instantiation has
scratch - the functor handed to the row walk is inlined, its (max, sum) pair lives in registers -; and both keep the floor of the launch
plan, 4 waves per SIMD (at most 128 registers): a level of the candidate trie launches hundreds to thousands of one-row workgroups, so
several share a CU and it is their co-residency that keeps the streaming read of the logits going.  LDS: the two 4-word pairs of the block
combine and the one word that carries lse to the workgroup."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import kernel_resources  # noqa: E402

ROWS = kernel_resources.load()
pytestmark = pytest.mark.skipif(not ROWS, reason="library not built in this tree (no csrc/_obj/*.resources.txt)")
FLOOR = 4


def test_the_unit_is_reported_without_scratch_at_the_floor_of_its_launch_plan():
    mine = [r for r in ROWS if r["unit"] == "ff_score"]
    assert len(mine) == 2 and all("logprob_gather_kernel" in r["mangled"] for r in mine), [r["name"] for r in mine]
    for dtype in ("DF16b", "f"):                                         # the Itanium codes of __bf16 and float
        row = [r for r in mine if f"logprob_gather_kernelI{dtype}E" in r["mangled"]]
        assert len(row) == 1, (dtype, [r["mangled"] for r in mine])
        r = row[0]
        print(f"{r['name']}: {r['vgprs']} VGPRs, {r.get('sgprs', 0)} SGPRs, scratch {r['scratch']}, {r['occupancy']} waves/SIMD, LDS {r.get('lds', 0)} bytes")
        assert r["scratch"] == 0 and r["occupancy"] >= FLOOR and r["vgprs"] + r.get("agprs", 0) <= 128, r
        assert r.get("lds", 0) <= 64, r
    for other in ("token_logprob_kernel", "guided_logits_kernel", "sample_token_kernel", "truncated_draw_kernel", "beam_rows_kernel", "logits_process_kernel",
                  "logits_constrain", "shifted_ce_"):
        assert not any(other in r["mangled"] for r in mine), other       # (names other resource tests count stay clear of this unit)
    assert not any("logprob_gather_kernel" in r["mangled"] for r in ROWS if r["unit"] != "ff_score")
