"""The constants of tests/util.py's ln_bound_ok, measured on the CPU: the float32 / bf16 restatements of the five LayerNorm implementations
(tests/ln_cases.py) against the float64 reference (ln_cases.ln_ref) at exactly the inputs of tests/test_hip_layernorm_bounds.py - every
C ABI shape and variant in both types, the column reduce and gate gradient cases, and the designed rows of every block case through the
restatement of that case's kernel (with alpha_attn = 0, where y1 = y exactly; the run with the usual gate normalises a y1 that only the
device produces).  The backward runs on the restated forward's statistics, as the kernels' does.  Prints the worst excess
(util.ln_excess) per case and overall, the worst relative rstd error per family on the fp32 block cases, and the LN_C_* lines of
tests/util.py: each 4 x the overall figure, rounded up to one decimal.
    python tools/ln_c.py"""
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import numpy as np  # noqa: E402

import ln_cases as lc  # noqa: E402
from util import ln_bound_ok, ln_excess as _ln_excess  # noqa: E402

RATIO = {}          # worst error / bound (util.ln_bound_ok with the constants as written in util.py) per output, filled as measure() goes


def ln_excess(what, got, ref, dtype, decode=False):
    ok, worst, idx = ln_bound_ok(what, got, ref, dtype, decode=decode)
    RATIO[what] = max(RATIO.get(what, 0.0), worst)
    return _ln_excess(what, got, ref, dtype, decode=decode)


def abi_excess(case):
    mu, rs, y = lc.ln_fwd_f32(case.v.numpy(), case.gamma, case.beta, case.dtype)
    ref = lc.ln_ref(case.v, case.gamma, case.beta, case.dy, stats=(mu, rs), residual=case.res)
    dx, dg, db = lc.ln_bwd_f32(case.dy, case.v.numpy(), case.gamma, mu, rs, case.dtype, residual=case.res)
    ref0 = lc.ln_ref(case.v, case.gamma, case.beta, case.dy, stats=(mu, rs))
    dx0, _, _ = lc.ln_bwd_f32(case.dy, case.v.numpy(), case.gamma, mu, rs, case.dtype, want_params=False)
    got = dict(mean=mu, rstd=rs, y=y, dx=dx, dgamma=dg, dbeta=db)
    ex = {w: ln_excess(w, g, ref, case.dtype) for w, g in got.items()}
    ex["dx"] = max(ex["dx"], ln_excess("dx", dx0, ref0, case.dtype))
    return ex


def block_excess(case):
    """(excess per output of LN(y), of LN(y1) at y1 = y, relative rstd error per row)"""
    y = case.y.reshape(case.rows, case.dim)
    mu, rs, yn = lc.onepass_f32(y, case.gamma_a, case.beta_a, case.kind)
    ref = lc.ln_ref(y, case.gamma_a, case.beta_a, P=case.P, P_var=case.P_var, stats=(mu, rs))
    ex = {w: ln_excess(w, g, ref, case.dtype) for w, g in dict(mean=mu, rstd=rs, y=yn).items()}
    relerr = np.abs(rs.astype(np.float64) - ref["rstd"]) / ref["rstd"]
    if case.ffw == "decode":
        mf, rf, xn = lc.onepass_f32(y, case.gamma_f, case.beta_f, "decode")
        reff = lc.ln_ref(y, case.gamma_f, case.beta_f, P=16, stats=(mf, rf))
        exf = {w: ln_excess(w, g, reff, case.dtype, decode=True) for w, g in dict(mean=mf, rstd=rf, y=xn).items()}
    elif case.ffw == "phase3":
        mf, rf, xn = lc.chan_f32(y, case.gamma_f, case.beta_f)
        reff = lc.ln_ref(y, case.gamma_f, case.beta_f, stats=(mf, rf))
        exf = {w: ln_excess(w, g, reff, case.dtype) for w, g in dict(mean=mf, rstd=rf, y=xn).items()}
    else:
        mf, rf, xn = lc.ln_fwd_f32(y.float().numpy(), case.gamma_f, case.beta_f, case.dtype)
        reff = lc.ln_ref(y, case.gamma_f, case.beta_f, stats=(mf, rf))
        exf = {w: ln_excess(w, g, reff, case.dtype) for w, g in dict(mean=mf, rstd=rf, y=xn).items()}
    return ex, exf, relerr


def measure(verbose=True):
    """{constant: (worst excess, case)} and {family: worst relative rstd error on the fp32 block cases}"""
    top = {k: (0.0, "") for k in ("m", "r", "v", "y", "x", "p")}
    say = print if verbose else (lambda *a: None)

    def note(k, v, name):
        if v > top[k][0]:
            top[k] = (v, name)

    for dtype in (lc.F32, lc.BF16):
        for case in lc.abi_cases(dtype):
            ex = abi_excess(case)
            say(f"{case.name:24s} excess " + " ".join(f"{w} {v:6.2f}" for w, v in ex.items()))
            for k, w in (("m", "mean"), ("r", "rstd"), ("y", "y"), ("x", "dx"), ("p", "dgamma"), ("p", "dbeta")):
                note(k, ex[w], f"{w} of {case.name}")
        for rows, cols, rpb, rpg in lc.REDUCE_CASES:
            x = lc.reduce_input(dtype, rows, cols)
            v = ln_excess("rows_reduce", lc.rows_reduce_f32(x, rpb, rpg, dtype), lc.rows_reduce_ref(x, rpb, rpg), dtype)
            say(f"rows_reduce {lc.name_of(dtype)} {rows}x{cols}: {v:.2f}")
            note("p", v, f"rows_reduce {lc.name_of(dtype)}-{rows}x{cols}")
        for rows, cols in lc.GATE_CASES:
            a, b, alpha = lc.gate_inputs(dtype, rows, cols)
            v = ln_excess("gate_grad", lc.gate_grad_f32(a, b, alpha, dtype), lc.gate_grad_ref(a, b, alpha), dtype)
            say(f"gate_grad {lc.name_of(dtype)} {rows}x{cols}: {v:.2f}")
            note("p", v, f"gate_grad {lc.name_of(dtype)}-{rows}x{cols}")
    fam = {}
    for case in lc.block_cases():
        ex, exf, relerr = block_excess(case)
        say(f"{case.name:24s} LN(y) [{case.kind}] " + " ".join(f"{w} {v:6.2f}" for w, v in ex.items()) + f"   LN(y1) [{case.ffw}] "
            + " ".join(f"{w} {v:6.2f}" for w, v in exf.items()))
        note("m", ex["mean"], f"mean_a of {case.name}")
        note("v", ex["rstd"], f"rstd_a of {case.name}")
        note("y", ex["y"], f"yn of {case.name}")
        note("m", exf["mean"], f"mean_f of {case.name}")
        note("v" if case.ffw == "decode" else "r", exf["rstd"], f"rstd_f of {case.name}")
        note("y", exf["y"], f"xn_f of {case.name}")
        if case.dtype == lc.F32:
            for r, e in enumerate(relerr):
                fam[lc.family_of(r)] = max(fam.get(lc.family_of(r), (0.0, "")), (float(e), case.name))
    return top, fam


def constant(v):
    return math.ceil(40.0 * v - 1e-9) / 10.0


if __name__ == "__main__":
    top, fam = measure()
    for k, (v, name) in top.items():
        print(f"worst excess c_{k} {v:6.2f}  at {name}")
    print("worst |rstd - rstd*| / rstd* per family, fp32 block cases (the ceiling is util.TOL[float32]['out'] = 5e-6):")
    for f, (e, name) in sorted(fam.items(), key=lambda kv: -kv[1][0]):
        print(f"  {f:14s} {e:.2e}  ({e / 2.0 ** -24:6.1f} u)  {name}")
    for k, (v, _) in top.items():
        print(f"LN_C_{k.upper()} = {constant(v)}")
