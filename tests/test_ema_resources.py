"""The compiler's resource remarks of csrc/ff_optim.hip (build.py keeps them per translation unit; tools/kernel_resources.py reads them):
ema_update_kernel is there for bf16 and for fp32 weights, uses no scratch memory and runs at 7 waves per SIMD or more - the floor
grad_accumulate_kernel, its nearest relative (one stream in, one fp32 read-modify-write stream), is held to - and it came as a kernel of its
own: the unit still has the 33 adamw_kernel instantiations it had before the weight average (21 round-to-nearest, 12 stochastic-rounding)."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import kernel_resources  # noqa: E402

ROWS = kernel_resources.load()
pytestmark = pytest.mark.skipif(not ROWS, reason="library not built in this tree (no csrc/_obj/*.resources.txt)")


def test_the_ema_kernel_is_reported_without_scratch_at_the_accumulate_kernels_occupancy():
    unit = [r for r in ROWS if r["unit"] == "ff_optim"]
    mine = [r for r in unit if "ema_update_kernel" in r["mangled"]]
    assert len(mine) == 2 and not any("adamw_kernel" in r["mangled"] for r in mine), [r["mangled"] for r in mine]
    for dtype in ("DF16b", "f"):                                         # the Itanium codes of __bf16 and float
        row = [r for r in mine if f"ema_update_kernelI{dtype}E" in r["mangled"]]
        assert len(row) == 1, (dtype, [r["mangled"] for r in mine])
        assert row[0]["scratch"] == 0 and row[0].get("lds", 0) == 0, row[0]
        assert row[0]["occupancy"] >= 7, (row[0]["name"], row[0]["vgprs"], row[0]["occupancy"])


def test_the_adamw_instantiations_are_the_33_there_were():
    assert sum("adamw_kernel" in r["mangled"] for r in ROWS if r["unit"] == "ff_optim") == 33
