"""The LayerNorm checkers' own tests, on the CPU: the constants of util.ln_bound_ok are what tools/ln_c.py measures, the restatements of
the five implementations (tests/ln_cases.py) stay within the bounds at every input of tests/test_hip_layernorm_bounds.py, the designed
rows keep the two conditions the bounds rest on (the condition number kappa <= 512 on every row, <= 2 on at least four families; on
fp32 rows rstd within the project's fp32 tolerance whatever kappa is), the numpy reference agrees with the oracle and with torch in
float64, and each of twelve injected defects fails its bound - the factor by which it does is printed."""
import os
import sys

import numpy as np
import pytest
import torch

import ln_cases as lc
import util
from oracle import flamingo_oracle as O
from util import TOL, ln_bound_ok

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import ln_c  # noqa: E402

BF16, F32 = lc.BF16, lc.F32
U = 2.0 ** -24
_MEASURED = {}


def measured():
    """tools/ln_c.py's pass over every GPU input: computed once, shared by the tests of this module"""
    if not _MEASURED:
        ln_c.RATIO.clear()
        top, fam = ln_c.measure(verbose=False)
        _MEASURED.update(top=top, fam=fam, ratio=dict(ln_c.RATIO))
    return _MEASURED


def test_the_constants_are_four_times_the_measured_excess():
    """tools/ln_c.py's figures (the comment above LN_C_M in util.py)"""
    top = measured()["top"]
    got = {k: ln_c.constant(v) for k, (v, _) in top.items()}
    print({k: (round(v, 2), name) for k, (v, name) in top.items()})
    assert got == dict(m=util.LN_C_M, r=util.LN_C_R, v=util.LN_C_V, y=util.LN_C_Y, x=util.LN_C_X, p=util.LN_C_P), got
    assert (util.LN_C_M, util.LN_C_R, util.LN_C_V, util.LN_C_Y, util.LN_C_X, util.LN_C_P) == (53.3, 33.5, 21.9, 10.4, 12.9, 8.1)


def test_restatements_stay_within_the_bounds_at_every_gpu_input():
    ratio = measured()["ratio"]
    print({k: round(v, 3) for k, v in ratio.items()})
    assert set(ratio) == {"mean", "rstd", "y", "dx", "dgamma", "dbeta", "rows_reduce", "gate_grad"}
    assert all(v <= 1.0 for v in ratio.values()), ratio


def test_kappa_cap_and_fp32_ceiling():
    """The two conditions that are not measurements.  kappa <= 512 on every designed row of every block case under the shift its kernel
    uses, and <= 2 on every row of at least four families (there the bound is two-pass quality whatever the kernel does); the two-pass
    kernels have kappa <= 1 by construction.  On the fp32 cases the restated kernels keep |rstd - rstd*| / rstd* within util.TOL[fp32]."""
    worst = 0.0
    for case in lc.block_cases():
        y = case.y.reshape(case.rows, case.dim)
        for P in {case.P, case.P_var, 16 if case.ffw == "decode" else 0}:
            k = lc.ln_ref(y, P=P)["kappa"]
            worst = max(worst, float(k.max()))
            assert k.max() <= 512, (case.name, P, k.max())
            if P == 0:
                assert k.max() <= 1.0
            fams = {f for f in lc.FAMILIES if all(k[r] <= 2 for r in range(case.rows) if lc.family_of(r) == f)}
            assert case.rows < lc.F or len(fams & set(lc.QUIET)) >= 4, (case.name, P, fams)
    print(f"largest kappa {worst:.1f}")
    assert 150 < worst < 512          # the one-pass kernels do meet hard rows: the resident kernel on head-off rows at dim 1536
    fam = measured()["fam"]
    print({f: f"{e:.2e}" for f, (e, _) in fam.items()})
    assert set(fam) == set(lc.FAMILIES) and max(e for e, _ in fam.values()) <= TOL[F32]["out"]
    for rows, cols in lc.ABI_SHAPES:
        case = lc.AbiCase(F32, rows, cols)
        mu, rs, _ = lc.ln_fwd_f32(case.v.numpy(), case.gamma, case.beta, F32)
        ref = lc.ln_ref(case.v)
        assert (np.abs(rs - ref["rstd"]) / ref["rstd"]).max() <= TOL[F32]["out"], case.name


def test_the_one_pass_fp32_form_missed_the_ceiling():
    """The finding behind the fp32 general kernel's second pass: its earlier one-pass form with the 4-element shift, restated, leaves rstd of
    massive-head- and head-off rows at dim 1536 off by more than the fp32 tolerance (1.7e-5 and 1.1e-5; the device gave 1.6e-5)."""
    case = [c for c in lc.block_cases() if c.name == "general-f32-widest"][0]
    y = case.y.reshape(case.rows, case.dim)
    ref = lc.ln_ref(y, P=4)
    for kind, over in (("general4-bm32", True), ("general4-bm32-2p", False)):
        _, rs, _ = lc.onepass_f32(y, case.gamma_a, case.beta_a, kind)
        rel = np.abs(rs - ref["rstd"]) / ref["rstd"]
        print(kind, f"{rel.max():.3e}", lc.family_of(int(rel.argmax())), f"kappa {ref['kappa'].max():.1f}")
        assert (rel.max() > TOL[F32]["out"]) == over
        assert ln_bound_ok("rstd", rs, ref if over else lc.ln_ref(y, P=4, P_var=0))[0]        # ... within its kappa-scaled bound either way


@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
def test_reference_agrees_with_the_oracle_and_torch(dtype):
    case = lc.AbiCase(dtype, 27, 256)
    ref = lc.ln_ref(case.v, case.gamma, case.beta, case.dy)
    x, g, b, dy = (lc.stored(t) for t in (case.v, case.gamma, case.beta, case.dy))
    assert O.LN_EPS == pytest.approx(lc.EPS, rel=1e-6)
    ref_o = lc.ln_ref(case.v, case.gamma, case.beta, case.dy, eps=O.LN_EPS)       # (the oracle's eps is the double 1e-5, the kernels' the float)
    y, cache = O.layernorm_fwd(x, g, b)
    dx, dg, db = O.layernorm_bwd(dy, cache, g)
    scale = lambda a: np.abs(a).max() + 1e-300
    for name, a in (("y", y), ("dx", dx), ("dgamma", dg), ("dbeta", db), ("rstd", cache[1][:, 0])):
        assert np.abs(ref_o[name] - a).max() <= 1e-11 * scale(a), name
    xt = torch.from_numpy(x).requires_grad_(True)
    gt, bt = torch.from_numpy(g).requires_grad_(True), torch.from_numpy(b).requires_grad_(True)
    yt = torch.nn.functional.layer_norm(xt, (x.shape[1],), gt, bt, eps=lc.EPS)
    yt.backward(torch.from_numpy(dy))
    for name, a in (("y", yt), ("dx", xt.grad), ("dgamma", gt.grad), ("dbeta", bt.grad)):
        a = a.detach().numpy()
        assert np.abs(ref[name] - a).max() <= 1e-11 * scale(a), name
    zero = [r for r in range(27) if lc.family_of(r) == "zero"]
    assert np.all(ref["y"][zero] == b) and np.all(ref["mean"][zero] == 0) and np.all(ref["t_mean"][zero] == 0)
    assert int((ref["t_dx"].max(-1) == 0).sum()) == 4                      # every seventh dy row is all zero


# ---- injected defects -------------------------------------------------------------------------------------------------------------------
ROWS, DIM = 39, 1280


def _block_rows(dtype):
    x = lc.designed_rows(ROWS, DIM, dtype, key=("defect",))
    gamma, beta, dy, res = lc.operands(ROWS, DIM, dtype, key=("defect",))
    return x, gamma, beta, dy, res


def _onepass(mutate, dtype=BF16, kind="resident", P=16, const_value=None):
    x, gamma, beta, _, _ = _block_rows(dtype)
    if const_value is not None:      # const rows that are not 3.25: there squares and sums round (13 / 4 keeps every partial sum exact)
        x = x.clone()
        for r in range(ROWS):
            if lc.family_of(r) == "const":
                x[r] = const_value + 0.37 * r
    mu, rs, y = lc.onepass_f32(x, gamma, beta, kind, mutate=mutate)
    return dict(mean=mu, rstd=rs, y=y), lc.ln_ref(x, gamma, beta, P=P, stats=(mu, rs)), dtype


def _twopass(mutate, dtype=F32):
    x, gamma, beta, dy, res = _block_rows(dtype)
    mu, rs, y = lc.ln_fwd_f32(x.float().numpy(), gamma, beta, dtype, mutate=mutate)
    return dict(mean=mu, rstd=rs, y=y), lc.ln_ref(x, gamma, beta, stats=(mu, rs)), dtype


def _backward(mutate, dtype=F32, rows=1025, cols=256):
    case = lc.AbiCase(dtype, rows, cols)
    mu, rs, _ = lc.ln_fwd_f32(case.v.numpy(), case.gamma, case.beta, dtype)
    dx, dg, db = lc.ln_bwd_f32(case.dy, case.v.numpy(), case.gamma, mu, rs, dtype, residual=case.res, mutate=mutate)
    return dict(dx=dx, dgamma=dg, dbeta=db), lc.ln_ref(case.v, case.gamma, case.beta, case.dy, stats=(mu, rs), residual=case.res), dtype


def _chan(mutate):
    x, gamma, beta, _, _ = _block_rows(BF16)
    mu, rs, y = lc.chan_f32(x, gamma, beta, mutate=mutate)
    return dict(mean=mu, rstd=rs, y=y), lc.ln_ref(x, gamma, beta, stats=(mu, rs)), BF16


# name -> (how it is produced, the output that must fail, the families the failing element must come from (None: any row))
DEFECTS = {
    "unshifted E[x^2] - mean^2 on the offset rows": (lambda: _onepass("unshifted"), "rstd", ("offset+", "offset-")),
    "unshifted, fp32": (lambda: _onepass("unshifted", F32, "general4", 4), "rstd", ("offset+", "offset-")),
    "shift = x[0] on massive-head": (lambda: _onepass("shift-x0"), "rstd", ("massive-head",)),
    "divisor n - 1": (lambda: _onepass("n-1"), "rstd", None),
    "divisor n - 1, two-pass": (lambda: _twopass("n-1"), "rstd", None),
    "eps added outside the square root": (lambda: _onepass("eps-outside"), "rstd", ("const", "zero", "tiny-var", "small")),
    "one 8-element piece left out of both sums": (lambda: _onepass("miss-piece"), "mean", None),
    "fmaxf removed on const": (lambda: _onepass(("unshifted", "no-fmax"), F32, "general4", 4, const_value=3.3), "rstd", ("const",)),
    "mean / rstd of neighbouring rows swapped": (lambda: _twopass("swap"), "mean", None),
    "gamma read from column c ^ 8": (lambda: _twopass("gamma-xor8"), "y", None),
    "one head's pair left out of the Chan combine": (lambda: _chan("miss-head"), "mean", None),
    "dx without the xh mean(dy g xh) term": (lambda: _backward("no-xhat-term"), "dx", None),
    "dgamma missing one row-block": (lambda: _backward("dgamma-miss-block"), "dgamma", None),
    "dgamma missing one row-block, column reduce": (lambda: _backward("dgamma-miss-block", F32, 1025, 4096), "dgamma", None),
    "dbeta taken from dy g": (lambda: _backward("dbeta-dyg"), "dbeta", None),
}


def test_the_unmutated_restatements_pass_on_the_defect_inputs():
    for make in (lambda: _onepass(None), lambda: _onepass(None, F32, "general4", 4), lambda: _twopass(None), lambda: _chan(None),
                 lambda: _backward(None), lambda: _backward(None, F32, 1025, 4096)):
        got, ref, dtype = make()
        for what, g in got.items():
            ok, worst, idx = ln_bound_ok(what, g, ref, dtype)
            assert ok, (what, worst, idx)


def _rows_of(families, got, ref):
    rows = [r for r in range(len(ref["mean"])) if lc.family_of(r) in families]
    return got[rows], {k: (v[rows] if v is not None and np.ndim(v) and len(v) == len(ref["mean"]) else v) for k, v in ref.items()}


@pytest.mark.parametrize("name", list(DEFECTS), ids=[k.replace(" ", "-") for k in DEFECTS])
def test_injected_defect_is_reported(name):
    """`families`: the defect is looked for on the rows of those families alone (it may show elsewhere too, and more)"""
    make, what, families = DEFECTS[name]
    got, ref, dtype = make()
    g = got[what]
    if families is not None:
        g, ref = _rows_of(families, g, ref)
    ok, worst, idx = ln_bound_ok(what, g, ref, dtype)
    print(f"{name}: {what} element {idx} is {worst:.4g} x its bound")
    assert not ok and worst > 2.0, (name, worst)


def test_the_clamp_is_what_holds_const_rows_under_unshifted_sums():
    """fmaxf(var, 0): on the designed const rows (3.25) every sum is exact and the variance is exactly 0 with or without the clamp, shifted
    or not - the shifted kernels see d = 0 there.  It acts where E[x^2] - mean^2 rounds below zero: const rows of another value under
    unshifted sums.  With the clamp those rows give rstd = 1 / sqrt(eps) exactly; without it they are the rows that fail."""
    clamped, ref, dtype = _onepass("unshifted", F32, "general4", 4, const_value=3.3)
    bare, _, _ = _onepass(("unshifted", "no-fmax"), F32, "general4", 4, const_value=3.3)
    const = [r for r in range(ROWS) if lc.family_of(r) == "const"]
    below = [r for r in const if not bare["rstd"][r] <= clamped["rstd"][r]]          # (NaN where var + eps fell below zero too)
    assert below, "no const row's variance rounded below zero: the test does not test anything"
    assert all(clamped["rstd"][r] == np.float32(1) / np.sqrt(np.float32(lc.EPS)) for r in below)
    ok, worst, idx = ln_bound_ok("rstd", *_rows_of(("const",), bare["rstd"], ref), dtype)
    print(f"{len(below)} of {len(const)} const rows below zero; without the clamp {worst:.4g} x the bound")
    assert not ok
    same, _, _ = _onepass(("unshifted", "no-fmax"))              # the designed 3.25 rows: nothing to see
    with_clamp, _, _ = _onepass("unshifted")
    assert np.array_equal(same["rstd"][const], with_clamp["rstd"][const]) and np.array_equal(same["mean"][const], with_clamp["mean"][const])
