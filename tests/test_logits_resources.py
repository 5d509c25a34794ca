"""The compiler's resource remarks of csrc/ff_logits.hip (build.py keeps them per translation unit; tools/kernel_resources.py reads them):
the unit is reported, both instantiations of its kernel are there, and neither uses scratch memory - the kernel sits in front of every
replayed decode step's selection, a spill would put a memory round trip into a launch that does a handful of loads and stores.  Its names
stay clear of the selection kernels tests/test_kernel_resources.py counts."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import kernel_resources  # noqa: E402

ROWS = kernel_resources.load()
pytestmark = pytest.mark.skipif(not ROWS, reason="library not built in this tree (no csrc/_obj/*.resources.txt)")


def test_the_unit_is_reported_and_its_kernels_use_no_scratch():
    mine = [r for r in ROWS if r["unit"] == "ff_logits"]
    assert len(mine) == 2 and all("logits_process_kernel" in r["mangled"] for r in mine), [r["name"] for r in mine]
    for r in mine:
        assert r["scratch"] == 0 and r["occupancy"] >= 8, (r["name"], r["scratch"], r["vgprs"], r["occupancy"])
        assert "sample_token_kernel" not in r["mangled"] and "beam_rows_kernel" not in r["mangled"]
