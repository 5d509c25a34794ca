"""The float32 restatement of token_logprob_kernel (tests/logprob_cases.py) without a GPU: on every designed row - loss_cases'
vocabularies, patterns and -inf placements, at ld == V, ld == 2 V and an odd ld, on and off the 16-byte grid - the kernel's operation order
in float32 stays within the project's loss bound (tests/util.py, CE_C_F) of float64 from the stored values, for the log-probability and
for lse; no row is excluded.  The edge rules of include/flamingo_fusion.h follow from the same arithmetic."""
import pytest
import torch

import logprob_cases as LP
import loss_cases as lc
from util import CE_C_F

DTYPES = pytest.mark.parametrize("dtype", [LP.F32, LP.BF16], ids=["f32", "bf16"])


@DTYPES
@pytest.mark.parametrize("group", LP.GROUPS)
def test_the_restatement_is_within_the_loss_bound_on_every_designed_row(dtype, group):
    n, worst = 0, [0.0, 0.0]
    for name, x, tok, ld, off in LP.cases(dtype, (group,)):
        assert x.shape[0] in (LP.R, 2 * lc.L) and tok.shape == x.shape[:1] and ld >= x.shape[1] and bool(((tok >= 0) & (tok < x.shape[1])).all())
        lp, lse = LP.token_logprob_f32(x, tok, ld, LP.start_off(x.shape[1], ld, off))
        ok, w_lp, w_lse = LP.within_bounds(lp, lse, x, tok, CE_C_F)
        worst = [max(worst[0], w_lp), max(worst[1], w_lse)]
        assert ok, f"{name}: logprob at {w_lp:.3f}, lse at {w_lse:.3f} of their bounds"
        n += 1
    print(f"{group}: {n} cases, worst logprob {worst[0]:.3f}, worst lse {worst[1]:.3f} of the bound")
    assert n >= 8


@DTYPES
def test_the_cases_cover_every_phase_and_every_region(dtype):
    """with an odd row stride the rows start at every phase of the 16-byte grid; the tokens fall in the scalar head, the vector body and
    the scalar tail; every -inf placement leaves the row's token alone"""
    nvec, regions = lc.NVEC[dtype], set()
    for name, x, tok, ld, off in LP.cases(dtype):
        V = x.shape[1]
        start = LP.start_off(V, ld, off)                       # where row 0 really begins: an ld == 2 V case is the [:, -1] view
        if ld % 2 == 1 and V >= 9:
            phases = {s // (16 // nvec) for s in LP.row_starts(len(tok), ld, dtype, start)}
            assert phases == set(range(nvec)), (name, phases)
        regions |= LP.token_regions(V, dtype, tok, ld, start)
        if "-inf" in name:
            assert int(torch.isinf(x).sum()) >= len(tok) // 2 and not bool(torch.isinf(x.gather(1, tok[:, None])).any()), name
    assert regions == {"head", "body", "tail"}, regions
    lds = {(ld == x.shape[1], ld == 2 * x.shape[1], ld % 2 == 1 and ld > x.shape[1]) for _, x, _, ld, _ in LP.cases(dtype)}
    assert {(False, True, False), (False, False, True)} <= lds and any(k[0] for k in lds)


def test_the_restatement_agrees_with_the_loss_restatement_on_a_contiguous_tensor():
    """rows of a contiguous (b, L, V) tensor with token[b, i] = labels[b, i + 1]: the same lse bits as loss_cases.ce_fwd_f32, logprob == -loss"""
    V = 2049
    x, _ = lc.logits(V, LP.BF16)
    lab = lc.labels(V)
    lab[lab == lc.IGNORE] = 7
    loss, lse = lc.ce_fwd_f32(x, lab)
    rows = [s * lc.L + i for s in range(lc.B) for i in range(lc.L - 1)]
    tok = torch.zeros(LP.R, dtype=torch.long)
    tok[rows] = lab[:, 1:].reshape(-1)
    lp, l2 = LP.token_logprob_f32(x.reshape(LP.R, V), tok)
    assert torch.equal(l2[rows].view(torch.int32), lse.view(torch.int32)) and torch.equal(lp[rows].view(torch.int32), (-loss).view(torch.int32))


def test_edge_rules_of_the_arithmetic():
    """x_tok = -inf gives -inf, -inf elsewhere contributes 0, a row holding NaN or +inf is NaN"""
    V = 33
    x = lc.logits(V, LP.F32)[0].reshape(LP.R, V)[:4].clone()
    tok = torch.tensor([3, 20, 32, 0])
    x[0, 3] = float("-inf")
    x[1, 5] = float("-inf")
    x[2, 9] = float("nan")
    x[3, 9] = float("inf")
    lp, lse = LP.token_logprob_f32(x, tok)
    assert float(lp[0]) == float("-inf") and bool(torch.isfinite(lse[0]))
    keep = torch.arange(V) != 5
    want = float(x[1, 20].double() - torch.logsumexp(x[1, keep].double(), 0))
    assert abs(float(lp[1]) - want) <= CE_C_F * 2.0 ** -24 * (abs(want) + abs(float(x[1, 20])) + 1)
    assert bool(torch.isnan(lp[2])) and bool(torch.isnan(lp[3]))
