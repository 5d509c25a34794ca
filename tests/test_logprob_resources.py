"""The compiler's resource remarks of csrc/ff_logprob.hip (build.py keeps them per translation unit; tools/kernel_resources.py reads them):
the unit is reported, both instantiations of token_logprob_kernel are there, neither uses scratch memory and both keep the occupancy of
the loss forward whose row pass they restate - the kernel sits inside every replayed decode step of a session that records
log-probabilities.  Its names stay clear of the kernels other resource tests count by name."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import kernel_resources  # noqa: E402

ROWS = kernel_resources.load()
pytestmark = pytest.mark.skipif(not ROWS, reason="library not built in this tree (no csrc/_obj/*.resources.txt)")


def test_the_unit_is_reported_and_its_kernels_use_no_scratch():
    mine = [r for r in ROWS if r["unit"] == "ff_logprob"]
    assert len(mine) == 2 and all("token_logprob_kernel" in r["mangled"] for r in mine), [r["name"] for r in mine]
    assert len({r["mangled"] for r in mine}) == 2
    for r in mine:
        assert r["scratch"] == 0 and r["occupancy"] >= 8, (r["name"], r["scratch"], r["vgprs"], r["occupancy"])
        for other in ("sample_token_kernel", "beam_rows_kernel", "logits_process_kernel", "shifted_ce_"):
            assert other not in r["mangled"], r["mangled"]
