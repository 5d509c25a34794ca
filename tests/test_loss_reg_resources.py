"""The compiler's resource remarks of csrc/ff_loss.hip (build.py keeps them per translation unit; tools/kernel_resources.py reads them): the
regularised instantiations of the two loss kernels - the ones with the trailing (float, float) pack - are there beside the plain ones, use
no scratch memory, and run at an occupancy at or above that of the plain instantiation of the same kernel and type, read from the same rows:
the two extra terms ride on passes that stream the logits, a spill or a lost wave would cost those passes their bandwidth."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import kernel_resources  # noqa: E402

ROWS = kernel_resources.load()
pytestmark = pytest.mark.skipif(not ROWS, reason="library not built in this tree (no csrc/_obj/*.resources.txt)")


def test_the_regularised_loss_kernels_are_reported_without_scratch_at_the_plain_occupancy():
    mine = [r for r in ROWS if r["unit"] == "ff_loss"]
    assert len(mine) == 8 and all("shifted_ce_" in r["mangled"] for r in mine), [r["name"] for r in mine]
    for kernel in ("shifted_ce_fwd_kernel", "shifted_ce_bwd_kernel"):
        for dtype in ("DF16b", "f"):                                     # the Itanium codes of __bf16 and float
            plain = [r for r in mine if f"{kernel}I{dtype}JEE" in r["mangled"]]
            reg = [r for r in mine if f"{kernel}I{dtype}JffEE" in r["mangled"]]
            assert len(plain) == 1 and len(reg) == 1, (kernel, dtype, [r["mangled"] for r in mine])
            for r in plain + reg:
                assert r["scratch"] == 0, (r["name"], r["scratch"])
            assert reg[0]["occupancy"] >= plain[0]["occupancy"] >= 8, (kernel, dtype, reg[0]["vgprs"], reg[0]["occupancy"], plain[0]["occupancy"])
