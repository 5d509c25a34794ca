"""The constants of tests/util.py's attn_bound_ok, measured on the CPU: the float32 / bf16 restatements of the attention kernels
(tests/attn_cases.py: attn_fwd_f32, attn_bwd_f32) against the float64 reference (attn_cases.attention_ref) at exactly the inputs of
tests/test_hip_attention_bounds.py - every dense instantiation, shape and input pattern, every media case.  The backward runs on the
restated forward's stored o and lse, as the kernels' does.  Prints the worst excess (util.attn_excess) per case and overall;
c_l, c_o, c_g are 4 x the overall figures.
    python tools/attn_c.py"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import attn_cases as ac  # noqa: E402
from util import attn_excess  # noqa: E402

OUTPUTS = ("lse", "o", "dq", "dk", "dv")


def case_excess(case):
    ref = case.ref()
    o, lse = ac.attn_fwd_f32(case.q, case.k, case.v, case.tt, case.n_visual)
    dq, dk, dv = ac.attn_bwd_f32(case.q, case.k, case.v, o, case.do, lse, case.tt, case.n_visual)
    return {w: attn_excess(w, t, ref, case.dtype) for w, t in zip(OUTPUTS, (lse, o, dq, dk, dv))}


if __name__ == "__main__":
    top = {w: (0.0, "") for w in OUTPUTS}
    for dtype in (ac.F32, ac.BF16):
        for case in ac.all_cases(dtype):
            ex = case_excess(case)
            for w, v in ex.items():
                if v > top[w][0]:
                    top[w] = (v, case.name)
            print(f"{case.name:44s} excess " + " ".join(f"{w} {v:6.2f}" for w, v in ex.items()))
    for w in OUTPUTS:
        print(f"worst excess {w:3s} {top[w][0]:6.2f}  at {top[w][1]}")
    cg = max(top[w][0] for w in ("dq", "dk", "dv"))
    print(f"c_l = 4 x {top['lse'][0]:.2f} = {4 * top['lse'][0]:.1f}; c_o = 4 x {top['o'][0]:.2f} = {4 * top['o'][0]:.1f}; "
          f"c_g = 4 x {cg:.2f} = {4 * cg:.1f}")
