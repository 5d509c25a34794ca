"""The constants of tests/util.py's ce_bound_ok and quick_gelu_bound_ok, measured on the CPU: the float32 restatements of the kernels
(tests/loss_cases.py: ce_fwd_f32, ce_bwd_f32, quick_gelu_f32) against the float64 references (util.shifted_ce_ref, util.quick_gelu_ref) at
the inputs of tests/test_hip_loss_bounds.py - every vocabulary, value pattern and -inf placement, aligned and one element off the grid,
every QuickGELU size, both dtypes.  Prints the worst excess (util.ce_excess / quick_gelu_excess) per case and overall.
    python tools/loss_c.py"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import torch  # noqa: E402

import loss_cases as lc  # noqa: E402
from util import ce_excess, quick_gelu_excess, quick_gelu_ref, shifted_ce_ref  # noqa: E402


def ce_case(x, lab, g, base_off=0):
    loss, lse = lc.ce_fwd_f32(x, lab, base_off)
    d = lc.ce_bwd_f32(x, lab, lse, g, base_off)
    ref = shifted_ce_ref(x, lab, g)
    return dict(lse=ce_excess("lse", lse, ref), loss=ce_excess("loss", loss, ref), d=ce_excess("d", d, ref, x.dtype))


if __name__ == "__main__":
    top = dict(lse=0.0, loss=0.0, d=0.0, gelu=0.0)
    for dtype in (lc.F32, lc.BF16):
        name = str(dtype).replace("torch.", "")
        for what, x, lab, g, off in lc.ce_cases(dtype):
            ex = ce_case(x, lab, g, off)
            for k, v in ex.items():
                top[k] = max(top[k], v)
            print(f"{name:9s} {what:34s} excess " + " ".join(f"{k} {v:6.2f}" for k, v in ex.items()))
        for n in lc.gelu_sizes(dtype):
            x, dy = lc.gelu_inputs(n, dtype)
            ex = [quick_gelu_excess(lc.quick_gelu_f32(x, w), *quick_gelu_ref(x, w), dtype) for w in (None, dy)]
            top["gelu"] = max(top["gelu"], *ex)
            print(f"{name:9s} quick_gelu n = {n:9d}: excess forward {ex[0]:6.2f} derivative {ex[1]:6.2f}")
    cf, cb, cq = max(top["lse"], top["loss"]), top["d"], top["gelu"]
    print(f"worst excess: lse {top['lse']:.2f} loss {top['loss']:.2f} -> c_f = 4 x = {4 * cf:.1f}; d {cb:.2f} -> c_b = 4 x = {4 * cb:.1f}; "
          f"quick_gelu {cq:.2f} -> c_q = 4 x = {4 * cq:.1f}")
