"""The constants of tests/loss_reg_cases.py's reg_bound_ok, measured on the CPU by the method of tools/loss_c.py: the float32 restatements
of the regularised loss kernels (loss_reg_cases.ce_reg_fwd_f32, ce_reg_bwd_f32) against the float64 reference (shifted_ce_reg_ref) at the
inputs of tests/test_hip_loss_reg.py - every case of loss_cases.ce_cases at every (eps, zeta) of loss_reg_cases.GRID, both dtypes.
Prints the worst excess per case and overall, beside util.CE_C_F / CE_C_B: where 4 x the worst excess stays below them, they are reused.
    python tools/loss_reg_c.py"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import loss_cases as lc  # noqa: E402
import loss_reg_cases as lr  # noqa: E402
from util import CE_C_B, CE_C_F  # noqa: E402


def worst_excess(dtypes=(lc.F32, lc.BF16), groups=lc.GROUPS, verbose=False):
    """{(what): (excess, where)} over the cases"""
    top = {k: (0.0, "") for k in ("lse", "loss", "d")}
    for dtype in dtypes:
        name = str(dtype).replace("torch.", "")
        for what, x, lab, g, off in lc.ce_cases(dtype, groups):
            lse, sums = lc.ce_fwd_f32(x, lab, off)[1], lr.row_sums_f32(x, off)
            for eps, zeta in lr.GRID:
                loss, _ = lr.ce_reg_fwd_f32(x, lab, eps, zeta, off, lse=lse, sums=sums)
                d = lr.ce_reg_bwd_f32(x, lab, lse, g, eps, zeta)
                ref = lr.shifted_ce_reg_ref(x, lab, g, eps, zeta)
                ex = dict(lse=lr.reg_excess("lse", lse, ref), loss=lr.reg_excess("loss", loss, ref), d=lr.reg_excess("d", d, ref, dtype))
                for k, v in ex.items():
                    if v > top[k][0]:
                        top[k] = (v, f"{name} {what} eps {eps} zeta {zeta}")
                if verbose:
                    print(f"{name:9s} {what:34s} eps {eps:<4} zeta {zeta:<6} excess " + " ".join(f"{k} {v:6.2f}" for k, v in ex.items()))
    return top


if __name__ == "__main__":
    top = worst_excess(verbose=True)
    cf, cb = max(top["lse"][0], top["loss"][0]), top["d"][0]
    print(f"worst excess: lse {top['lse'][0]:.2f} ({top['lse'][1]}), loss {top['loss'][0]:.2f} ({top['loss'][1]}) -> c_f = 4 x = {4 * cf:.1f} "
          f"(util.CE_C_F = {CE_C_F}); d {cb:.2f} ({top['d'][1]}) -> c_b = 4 x = {4 * cb:.1f} (util.CE_C_B = {CE_C_B})")
