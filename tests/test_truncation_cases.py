"""The truncation samplers' references against transformers' own classes, without a GPU: the float64 numpy reference
(tests/truncation_cases.py) and decoding.truncate_logits_torch each give the kept set of MinPLogitsWarper, TypicalLogitsWarper,
EpsilonLogitsWarper and EtaLogitsWarper chained in float64; with every rule off the reference is tests/test_hip_sampling.py's; and the
placement helpers' preconditions hold on the seeds the GPU tests use."""
import numpy as np
import pytest
import torch

import truncation_cases as tc

V = 3000
# float32 values: EtaLogitsWarper keeps its epsilon as a float32 tensor
VALUES = dict(min_p=tc.f32(0.05), typical_p=tc.f32(0.8), epsilon_cutoff=tc.f32(1e-3), eta_cutoff=tc.f32(5e-3))
CASES = {name: dict(tc.OFF, **{name: VALUES[name]}) for name in tc.RULES}
CASES["all-four"] = dict(VALUES)
CASES["all-four-loose"] = dict(min_p=tc.f32(1e-3), typical_p=tc.f32(0.95), epsilon_cutoff=tc.f32(3e-4), eta_cutoff=tc.f32(6e-4))
FILTERS = [(1.0, 0, 1.0), (0.7, 50, 0.9), (1.5, 0, 0.95)]


def rows():
    """random bf16-valued rows with ties (bf16 has few values near the top) and -inf entries"""
    g = torch.Generator().manual_seed(123)
    x = (torch.randn((40, V), generator=g) * 4).to(torch.bfloat16).double()
    x[torch.rand((40, V), generator=g) < 0.1] = float("-inf")
    x[::4, :7] = x[::4, :1]                                              # and ties made on purpose, wherever the row's first value lies
    return x


def hf_kept(scores, tr):
    from transformers.generation.logits_process import EpsilonLogitsWarper, EtaLogitsWarper, MinPLogitsWarper, TypicalLogitsWarper
    ids = torch.zeros((scores.shape[0], 1), dtype=torch.long)
    if tr["min_p"] > 0:
        scores = MinPLogitsWarper(tr["min_p"])(ids, scores)
    if tr["typical_p"] < 1:
        scores = TypicalLogitsWarper(tr["typical_p"])(ids, scores)
    if tr["epsilon_cutoff"] > 0:
        scores = EpsilonLogitsWarper(tr["epsilon_cutoff"])(ids, scores)
    if tr["eta_cutoff"] > 0:
        scores = EtaLogitsWarper(tr["eta_cutoff"])(ids, scores)
    return scores > float("-inf")


@pytest.mark.parametrize("filt", FILTERS, ids=lambda f: "T%g-k%d-p%g" % f)
@pytest.mark.parametrize("case", list(CASES))
def test_both_references_keep_what_transformers_keeps(case, filt):
    from flamingo_mini_amd import decoding
    tr, (T, k, p) = CASES[case], filt
    x = rows()
    scores = decoding.filter_logits(x, T, k, p)
    want = hf_kept(scores.clone(), tr)
    assert bool(want.any(-1).all()) and bool((want.sum(-1) < (x > float("-inf")).sum(-1)).any())       # never empty; something is cut
    mine = decoding.truncate_logits_torch(scores, **tr) > float("-inf")
    assert torch.equal(mine, want), [int(r) for r in (mine != want).any(-1).nonzero()[:, 0]][:8]
    # the numpy reference, on ITS rules 1 - 2 (a threshold keeps the values tied at the nucleus boundary together, filter_logits' sort may
    # split them): transformers' classes get the reference's own K1
    K1 = np.stack([tc.chain(x[r].numpy(), T, k, p).K for r in range(x.shape[0])])
    want = hf_kept(torch.where(torch.from_numpy(K1), x / T, torch.full_like(x, float("-inf"))), tr)
    ref = np.stack([tc.chain(x[r].numpy(), T, k, p, **tr).K for r in range(x.shape[0])])
    assert np.array_equal(ref, want.numpy()), np.nonzero((ref != want.numpy()).any(-1))[0][:8]


def test_equal_values_stay_or_go_together_and_the_largest_stays():
    x = rows()
    for tr in CASES.values():
        for r in range(0, x.shape[0], 4):
            c = tc.chain(x[r].numpy(), 1.0, 0, 1.0, **tr)
            xr = x[r].numpy()
            assert c.K.any() and not c.K[xr == -np.inf].any()
            assert set(xr[c.K]).isdisjoint(set(xr[~c.K]))


@pytest.mark.parametrize("setting", [(1.0, 0, 1.0), (0.7, 50, 1.0), (1.0, 0, None), (0.7, 50, None), (1.3, 1, 1.0)], ids=str)
def test_with_every_rule_off_the_reference_is_the_sampling_reference(setting):
    from test_hip_sampling import Ref, make_logits
    T, k, p_set = setting
    x = make_logits(4, 5000, torch.bfloat16, seed=31)
    x[1, ::3] = float("-inf")
    for r in range(4):
        xr = x[r].double().numpy()
        old = Ref(xr, T, k)
        p = old.place_p() if p_set is None else p_set
        new = tc.chain(xr, T, k, p, **tc.OFF)
        assert np.array_equal(new.K, old.kept(p) & (xr > -np.inf))
        assert not new.margins or abs(new.margins[0][2] - np.abs(old.above - p).min()) < 1e-12
        assert new.place_u() == old.place_u(p)
        for u in (0.0, 0.123, 0.5, 0.877, 0.999999):
            assert new.token(u) == old.token(p, u)


@pytest.mark.parametrize("shape", list(tc.SHAPES))
def test_the_placement_preconditions_hold_on_the_designed_cases(shape):
    """designed_case asserts them (every decision away from its threshold, the kept set stable under H +- DELTA_H); here also: every rule
    that is on cuts something on some row of the 50258-column shapes, so the GPU comparison is not one of untruncated rows"""
    rows_, V_, _, _ = tc.SHAPES[shape]
    x64 = tc.shape_logits(shape).double().numpy()
    for setting, (T, k, p_set, rules) in tc.SETTINGS.items():
        cases = tc.designed_case(shape, setting)
        assert len(cases) == rows_ and all(len(placed) == 3 for *_, placed in cases)
        if V_ >= 50258:
            cut = dict.fromkeys(rules, False)
            for r, p, tr, _ in cases:
                c = tc.Chain(x64[r], T, k).nucleus(p)
                for name, apply in (("min_p", c.min_p), ("typical_p", c.typical), ("epsilon_cutoff", c.epsilon), ("eta_cutoff", c.eta)):
                    before = int(c.K.sum())
                    apply(tr[name])
                    if name in rules:
                        cut[name] = cut[name] or int(c.K.sum()) < before
            assert all(cut.values()), (setting, cut)


def test_the_constants_are_eight_times_the_measured_values():
    assert tc.REL_MARGIN == 8 * 1.83e-6 and tc.DELTA_H == 8 * 1.53e-6
    assert tc.GROUP_MASS == 2e-3 and tc.TOKEN_MASS == 2e-3
