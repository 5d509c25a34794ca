"""The constants of tests/util.py's attn_bound_ok, measured again on the CPU at the inputs of tests/test_hip_xattn_bounds.py: the float32
/ bf16 restatement of the fused cross-attention block (tests/xattn_cases.py: block_f32 - attn_cases.attn_fwd_f32 / attn_bwd_f32 with the
fused kernels' tiling: 32 or 64 queries per workgroup, one key tile and so no rescale in the resident kernels, d O = tanh(alpha) . d y1 .
Wo taken in float32 and rounded to T before D and both passes use it) against attention_ref from the restatement's own stored Qs and
d y1, as the stage checks take it (the d O terms of the bound included: they are fixed terms, not part of the excess).
Prints the worst excess (util.attn_excess) per case and overall, next to the constants in force: a constant stays if 4 x the worst excess
is below it, otherwise it is raised to 4 x that excess.  The GEMM stages use gemm_bound_ok, which has no measured constant.
    python tools/xattn_c.py"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import util  # noqa: E402
import xattn_cases as xc  # noqa: E402

OUTPUTS = ("lse", "o", "dq", "dk", "dv")


def case_excess(case):
    st = xc.block_f32(case)
    ref = xc.attention_refs(case, st)
    b, L, H, dh = case.b, case.L, case.heads, case.dh
    dkv = st["dkv"].reshape(b, case.n_kv, 2, H, dh)
    got = dict(lse=st["lse"], o=st["O"].reshape(b, L, H, dh), dq=st["dQs"].reshape(b, L, H, dh), dk=dkv[:, :, 0], dv=dkv[:, :, 1])
    return {w: util.attn_excess(w, got[w], ref, case.dtype, extra=True) for w in OUTPUTS}


if __name__ == "__main__":
    top = {(dt, w): (0.0, "") for dt in ("f32", "bf16") for w in OUTPUTS}
    for case in xc.all_cases():
        ex = case_excess(case)
        for w, v in ex.items():
            key = (xc.name_of(case.dtype), w)
            if v > top[key][0]:
                top[key] = (v, case.name)
        print(f"{case.name:40s} excess " + " ".join(f"{w} {v:6.2f}" for w, v in ex.items()))
    for (dt, w), (v, name) in top.items():
        print(f"worst excess {dt:4s} {w:3s} {v:6.2f}  at {name}")
    worst = {w: max(top[(dt, w)][0] for dt in ("f32", "bf16")) for w in OUTPUTS}
    cg = max(worst[w] for w in ("dq", "dk", "dv"))
    for name, have, ex in (("ATTN_C_L", util.ATTN_C_L, worst["lse"]), ("ATTN_C_O", util.ATTN_C_O, worst["o"]), ("ATTN_C_G", util.ATTN_C_G, cg)):
        print(f"{name} = {have}: 4 x {ex:.2f} = {4 * ex:.1f} -> " + ("stays" if 4 * ex <= have else f"raise to {4 * ex:.1f}"))
