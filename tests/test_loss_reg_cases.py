"""The rig of the regularised loss tests, on the CPU (tests/loss_reg_cases.py): the float64 reference is torch's own definition - and HF's
LabelSmoother - on every input of loss_cases.ce_cases, -inf logits included; the float32 restatements of the two kernels stay inside the
bounds the GPU test holds the kernels to; every defect the restatements can inject leaves them; and the constants are what
tools/loss_reg_c.py measures."""
import os
import sys

import pytest
import torch

import loss_cases as lc
import loss_reg_cases as lr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DTYPES = pytest.mark.parametrize("dtype", [lc.F32, lc.BF16], ids=["f32", "bf16"])
# two float64 evaluations of one formula differ by roundings of 2^-53 each, a few per element and one per term of a sum the terms of
# which t_loss / t_d bound: 1e-11 of those terms is 1e5 such roundings
F64_SLACK = 1e-11


@pytest.fixture(scope="module")
def cases():
    """per dtype: (name, x, labels, g, off, lse and row sums of the float32 restatement) of every case - computed once, read only"""
    out = {}
    for dtype in (lc.F32, lc.BF16):
        out[dtype] = [(name, x, lab, g, off, lc.ce_fwd_f32(x, lab, off)[1], lr.row_sums_f32(x, off)) for name, x, lab, g, off in lc.ce_cases(dtype)]
    return out


def torch_definition(x, lab, g, eps, zeta):
    """(loss rows, d logits) in float64 by F.cross_entropy(label_smoothing=eps, reduction='none') + zeta logsumexp^2 and autograd"""
    eps, zeta = lr.as_launched(eps, zeta)
    b, L, V = x.shape
    xd = x.double().requires_grad_(True)
    flat, tgt = xd[:, :-1].reshape(-1, V), lab[:, 1:].reshape(-1)
    rows = torch.nn.functional.cross_entropy(flat, tgt, reduction="none", label_smoothing=eps, ignore_index=lc.IGNORE)
    rows = rows + torch.where(tgt != lc.IGNORE, zeta * torch.logsumexp(flat, dim=-1) ** 2, torch.zeros_like(rows))
    (rows * g.double()).sum().backward()
    return rows.detach(), xd.grad


def close64(got, want, terms):
    got, want, terms = got.reshape(-1), want.reshape(-1), terms.reshape(-1)
    return bool(((got == want) | ((got - want).abs() <= F64_SLACK * terms)).all())


@DTYPES
def test_the_reference_is_torch_cross_entropy_with_label_smoothing_plus_z_loss(dtype, cases):
    """loss and autograd gradient on every case group; in the -inf group the loss of every scored row is +inf where eps > 0 and finite where
    eps = 0, and the gradient is finite everywhere: -eps / V g at the -inf columns"""
    seen_inf = 0
    for name, x, lab, g, off, _, _ in cases[dtype]:
        for eps, zeta in lr.GRID:
            ref = lr.shifted_ce_reg_ref(x, lab, g, eps, zeta)
            rows, grad = torch_definition(x, lab, g, eps, zeta)
            assert close64(ref["loss"], rows, ref["t_loss"]), (name, eps, zeta)
            assert close64(ref["d"], grad, ref["t_d"] + ref["flush"]), (name, eps, zeta)
            assert bool(torch.isfinite(ref["d"]).all()) and not bool(torch.isnan(ref["loss"]).any())
            if "-inf" in name:
                scored = lab[:, 1:].reshape(-1) != lc.IGNORE
                masked = torch.isinf(x)
                holds = masked[:, :-1].any(dim=-1).reshape(-1)             # (a row whose only -inf column would be its target has none)
                assert int((holds & scored).sum()) >= 8
                assert torch.equal(torch.isposinf(ref["loss"]), holds & scored if eps > 0 else torch.zeros_like(holds)), (name, eps, zeta)
                e32 = lr.as_launched(eps, zeta)[0]
                want = (-e32 / x.shape[2] * (g.double().reshape(lc.B, lc.L - 1) * scored.reshape(lc.B, lc.L - 1))).unsqueeze(-1).expand(-1, -1, x.shape[2])
                assert torch.equal(ref["d"][:, :-1][masked[:, :-1]], want[masked[:, :-1]]), (name, eps, zeta)
                seen_inf += 1
    assert seen_inf == 2 * 2 * len(lc.NEG_INF) * len(lr.GRID)


@DTYPES
def test_the_reference_is_the_trainers_label_smoother_when_zeta_is_0(dtype, cases):
    """transformers.trainer_pt_utils.LabelSmoother(epsilon=eps) with shifted labels (what HF Trainer runs under --label_smoothing_factor):
    its mean loss and the gradient of that mean"""
    try:
        from transformers.trainer_pt_utils import LabelSmoother
    except Exception as e:  # pragma: no cover
        pytest.skip(f"transformers.trainer_pt_utils.LabelSmoother cannot be imported: {e}")
    for name, x, lab, g, off, _, _ in cases[dtype]:
        for eps, zeta in [(e, z) for e, z in lr.GRID if z == 0] + [(1.0, 0.0)]:
            e32 = lr.as_launched(eps, zeta)[0]
            count = int((lab[:, 1:] != lc.IGNORE).sum())
            ones = torch.full((lab.shape[0] * (lab.shape[1] - 1),), 1.0 / count, dtype=torch.float64)
            ref = lr.shifted_ce_reg_ref(x, lab, ones, eps, 0.0)
            xd = x.double().requires_grad_(True)
            loss = LabelSmoother(epsilon=e32, ignore_index=lc.IGNORE)({"logits": xd}, lab, shift_labels=True)
            mean, t_mean = ref["loss"].sum() / count, ref["t_loss"].sum() / count
            # the LabelSmoother sums -log p over the vocabulary in float32 whatever the logits' type (dtype=torch.float32 in its source):
            # every term rounded once, 2^-24, and a pairwise sum of V of them, 2^-24 log2 V <= 16 2^-24 at these vocabularies, of
            # eps mean(-log p) = eps (lse - mean x) per row; the gradient passes that cast once: 2^-24 of its eps / V term, below 2^-23 t_d
            V = x.shape[2]
            valid = (lab[:, 1:] != lc.IGNORE).reshape(-1)
            smooth = e32 * torch.where(valid, ref["lse"] - x.double()[:, :-1].mean(dim=-1).reshape(-1), torch.zeros_like(ref["lse"])).sum() / count
            assert V < 2 ** 16 and close64(loss.detach(), mean, t_mean + 17 * 2.0 ** -24 / F64_SLACK * smooth), (name, eps, float(loss.detach()), float(mean))
            if "-inf" not in name:          # (its masked_fill form multiplies the +inf rows' gradient by 0: NaN - the loss is what a Trainer user sees)
                loss.backward()
                assert close64(ref["d"], xd.grad, ref["t_d"] * (1 + 2.0 ** -23 / F64_SLACK) + ref["flush"]), (name, eps)


def restated(case, eps, zeta, mutate=None):
    name, x, lab, g, off, lse, sums = case
    fwd_mut = mutate if mutate in ("no-mean-term", "mean-over-V-1", "z-term-missing") else None
    loss, _ = lr.ce_reg_fwd_f32(x, lab, eps, zeta, off, lse=lse, sums=sums, mutate=fwd_mut)
    return loss, lse, lr.ce_reg_bwd_f32(x, lab, lse, g, eps, zeta, mutate=mutate)


@DTYPES
def test_the_restatements_stay_inside_the_bounds_and_set_the_constants(dtype, cases):
    """every case, every (eps, zeta): lse, loss and d of the float32 restatements within reg_bound_ok; their worst excess x 4 is the
    constant (to the one decimal the constants are written with), the larger of the two dtypes"""
    worst = {"lse": 0.0, "loss": 0.0, "d": 0.0}
    for case in cases[dtype]:
        name, x, lab, g, off = case[:5]
        for eps, zeta in lr.GRID:
            ref = lr.shifted_ce_reg_ref(x, lab, g, eps, zeta)
            for what, got in zip(("loss", "lse", "d"), restated(case, eps, zeta)):
                ok, w, idx = lr.reg_bound_ok(what, got, ref, dtype)
                assert ok, f"{name} eps {eps} zeta {zeta}: {what} element {idx} is {w:.4g} x its bound"
                worst[what] = max(worst[what], lr.reg_excess(what, got, ref, dtype))
    print(f"{dtype}: worst excess {worst}")
    assert 4 * max(worst["lse"], worst["loss"]) <= lr.CE_REG_C_F + 0.05 and 4 * worst["d"] <= lr.CE_REG_C_B + 0.05
    if dtype == lc.BF16:
        assert 4 * worst["loss"] >= lr.CE_REG_C_F - 0.05, worst          # (the figures in the comment next to the constants)
    else:
        assert 4 * worst["d"] >= lr.CE_REG_C_B - 0.05, worst


@pytest.mark.parametrize("mutate", lr.MUTATIONS)
def test_every_injected_defect_leaves_the_bounds(mutate, cases):
    """at the small and boundary vocabularies and the value patterns, both dtypes: the defect breaks a bound at one (eps, zeta) or more - and
    at every one at which it changes the formula at all"""
    what = "loss" if mutate in ("no-mean-term", "mean-over-V-1") else "d"
    caught = {}
    for dtype in (lc.F32, lc.BF16):
        for case in cases[dtype]:
            name, x, lab, g, off = case[:5]
            if x.shape[2] > lc.V_LARGE or "-inf" in name:
                continue
            for eps, zeta in lr.GRID:
                ref = lr.shifted_ce_reg_ref(x, lab, g, eps, zeta)
                loss, lse, d = restated(case, eps, zeta, mutate)
                bad = not lr.reg_bound_ok(what, loss if what == "loss" else d, ref, dtype)[0]
                if mutate == "z-term-missing":
                    bad = bad or not lr.reg_bound_ok("loss", loss, ref, dtype)[0]
                caught[(eps, zeta)] = caught.get((eps, zeta), False) or bad
    changes = {"no-mean-term": lambda e, z: e > 0, "mean-over-V-1": lambda e, z: e > 0, "onehot-unscaled": lambda e, z: e > 0,
               "eps-over-V-missing": lambda e, z: e > 0, "z-term-missing": lambda e, z: z > 0, "z-grad-without-factor-2": lambda e, z: z > 0}[mutate]
    assert caught == {(e, z): changes(e, z) for e, z in lr.GRID}, (mutate, caught)


def test_the_constants_tool_reports_what_the_test_measures():
    """tools/loss_reg_c.py on the smallest group: runs, and its figures are bounded by the constants"""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import loss_reg_c
    top = loss_reg_c.worst_excess(groups=("patterns",))
    assert 0 < 4 * max(top["lse"][0], top["loss"][0]) <= lr.CE_REG_C_F and 0 < 4 * top["d"][0] <= lr.CE_REG_C_B
