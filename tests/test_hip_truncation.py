"""The truncation samplers on the MI355X: ff_sample_token_truncated / functional.sample_tokens(min_p=, typical_p=, epsilon_cutoff=,
eta_cutoff=) (csrc/ff_truncate.hip) and the sampling _DecodeSession under a Truncation.

The reference is tests/truncation_cases.py: float64 numpy, rules 1 - 7 of include/flamingo_fusion.h on the logits exactly as stored.  No test
compares near a decision: parameters and u are placed (mass decisions >= 1e-3 away, probability decisions >= REL_MARGIN relative, the kept
set identical under H +- DELTA_H; the constants are measured, see truncation_cases) and the preconditions are asserted; then every row
must match exactly."""
import numpy as np
import pytest
import torch

import truncation_cases as tc
from test_hip_sampling import EDGE, SAMPLING, _SampleRecorder, g1, sampled  # noqa: F401  (g1: the module fixture of the G1 geometry)

BF16, F32 = tc.BF16, tc.F32


def run_kernel(x, u, T, k, p, tr, out=None):
    """x: (rows, V) device tensor (any row stride), u: rows numbers, tr: the four parameters -> tokens as a numpy array"""
    from flamingo_mini_amd import functional as F
    ut = torch.tensor(np.asarray(u, dtype=np.float32), device=x.device)
    return F.sample_tokens(x, ut, T, k, p, out=out, **tr).cpu().numpy()


# ---------------------------------------------------------------------------------------------------------------------------------------
# 1. designed rows, exact match
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("setting", list(tc.SETTINGS))
@pytest.mark.parametrize("shape", list(tc.SHAPES))
def test_designed_rows_match_the_reference_exactly(shape, setting):
    rows, V, dtype, layout = tc.SHAPES[shape]
    T, k, _, _ = tc.SETTINGS[setting]
    x = tc.shape_logits(shape)
    rep = x.repeat_interleave(3, 0)                                      # every row three times (one per placed u), in the layout under test
    if layout == "last-of-3":
        full = torch.full((3 * rows, 3, V), 99.0, dtype=dtype)           # the other positions would win every draw if they were read
        full[:, -1] = rep
        dev = full.cuda()[:, -1]
        assert dev.stride(0) == 3 * V and not dev.is_contiguous()
    else:
        dev = rep.cuda()
    bad = []
    for r, p, tr, placed in tc.designed_case(shape, setting):            # the parameters differ per row: one launch per row's three replicas
        got = run_kernel(dev[3 * r:3 * r + 3], [u for u, _ in placed], T, k, p, tr)
        bad += [(r, p, tr, int(g), t) for g, (_, t) in zip(got, placed) if int(g) != t]
    assert not bad, f"{len(bad)} (row, top_p, parameters, got, want) differ: {bad[:4]}"


# ---------------------------------------------------------------------------------------------------------------------------------------
# 2. stratified histogram
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("V,N", [(1000, 4096), (50258, 256)])
@pytest.mark.parametrize("setting", ["all-four", "all-four-T0.7-k50-p"])
def test_stratified_draws_follow_the_distribution(V, N, setting):
    """One row drawn N times with u_j = (j + 0.5) / N.  Every token lies in the reference's K5 - exactly - and every token's count is within
    3 of N r_i (stratification allows 1 per interval end, an end displaced by rounding 1 more per end)."""
    T, k, p, rules = tc.SETTINGS[setting]
    x = tc.make_logits(1, V, BF16, seed={1000: 2, 50258: 50265}[V])
    if V == 1000:
        x[0, torch.randperm(V, generator=torch.Generator().manual_seed(3))[:V // 2]] = float("-inf")
    x64 = x[0].double().numpy()
    p, tr = tc.place(x64, T, k, p, rules)                                # (it leaves a distribution, not one spike: asserted below)
    ok, ref = tc.decidable(x64, T, k, p, tr)
    assert ok, (p, tr, ref.margins)
    P, r, _ = ref.cdf()
    u = (np.arange(N) + 0.5) / N
    got = run_kernel(x.cuda().repeat(N, 1), u, T, k, p, tr)
    assert got.min() >= 0 and got.max() < V
    assert P[got].all(), f"tokens outside K5: {sorted(set(got[~P[got]].tolist()))[:8]}"
    assert np.isfinite(x64[got]).all()
    count = np.bincount(got, minlength=V)
    dev = np.abs(count - N * r)
    assert dev.max() <= 3, (int(dev.argmax()), int(count[dev.argmax()]), float(N * r[dev.argmax()]))
    assert (count > 0).sum() >= 3, int(P.sum())


# ---------------------------------------------------------------------------------------------------------------------------------------
# 3. extremes
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("V,dtype", [(50258, BF16), (1000, F32)])
@pytest.mark.parametrize("tr", [dict(min_p=1.0), dict(epsilon_cutoff=0.999)], ids=["min_p=1", "epsilon=0.999"])
def test_the_strictest_thresholds_are_greedy(V, dtype, tr):
    """min_p = 1 keeps the maximum alone, and so does epsilon_cutoff = 0.999 while no token holds that much - whatever u is, given that the
    maximum is unique, which is asserted (it is raised by 2 to make it so: bf16 maxima tie easily)."""
    x = tc.make_logits(6, V, dtype, seed=77 + V)
    top = x.float().argmax(-1)
    x[torch.arange(6), top] += 2
    top2 = x.float().topk(2, dim=-1).values
    assert bool((top2[:, 0] > top2[:, 1]).all()), "a row's maximum is not unique"
    assert float(x.double().softmax(-1).max()) < 0.999
    got = run_kernel(x.cuda(), np.linspace(0.01, 0.99, 6), 1.0, 0, 1.0, dict(tc.OFF, **tr))
    assert got.tolist() == top.tolist()


@pytest.mark.gpu
@pytest.mark.parametrize("V,dtype", [(50258, BF16), (70001, BF16), (1000, F32)])
def test_all_rules_off_through_the_new_entry_is_ff_sample_token(V, dtype):
    """typical_p = 1, epsilon_cutoff = eta_cutoff = 0 (and min_p = 0) through ff_sample_token_truncated: the tokens of ff_sample_token on the
    same rows and u, bit for bit - any u, the two kernels form the same sums in the same order."""
    from flamingo_mini_amd import ffi, functional as F
    x = tc.make_logits(16, V, dtype, seed=5 + V).cuda()
    u = torch.rand(16, generator=torch.Generator().manual_seed(9)).cuda()
    for T, k, p in ((1.0, 0, 1.0), (0.7, 50, 0.9), (1.3, 0, 0.8)):
        want = F.sample_tokens(x, u, T, k, p)
        got = torch.full((16,), -1, dtype=torch.long, device="cuda")
        ffi.check(ffi.lib().ff_sample_token_truncated(ffi.dtype_code(dtype), 16, V, V, x.data_ptr(), T, k, p, 0.0, 1.0, 0.0, 0.0, u.data_ptr(), got.data_ptr(),
                                                      ffi.stream_handle(x.device)), "ff_sample_token_truncated")
        assert torch.equal(got, want), (T, k, p)


# ---------------------------------------------------------------------------------------------------------------------------------------
# 4. rows whose token is unspecified stay in range; the output is written inside its bounds only
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("V,dtype", [(50258, BF16), (1000, F32), (70001, BF16)])
def test_unspecified_rows_stay_in_range_and_neighbours_are_unharmed(V, dtype):
    """NaN, +inf and all -inf rows beside ordinary ones in one launch under all four rules (placed on row 0): every token is inside
    [0, V), the guarded output is written inside its bounds only, row 0 equals the reference, and every ordinary row draws the token it draws
    when launched alone."""
    from guarded import guarded_allocations
    from flamingo_mini_amd import functional as F
    T, k = 0.7, 50
    x = tc.make_logits(7, V, dtype, seed=11 + V)
    x[1, V // 3] = float("nan")
    x[3, V - 1] = float("inf")
    x[5] = float("-inf")
    ordinary = [0, 2, 4, 6]
    x0 = x[0].double().numpy()
    p, tr = tc.place(x0, T, k, None, tc.RULES)
    ok, ref = tc.decidable(x0, T, k, p, tr)
    assert ok, (p, tr, ref.margins)
    u0, tok0 = ref.place_u()[1]                                          # the heaviest token
    dev = x.cuda()
    ut = torch.tensor([u0] + [0.5] * 6, dtype=torch.float32, device="cuda")
    with guarded_allocations() as g:
        tok = F.sample_tokens(dev, ut, T, k, p, **tr)                    # the output comes from the (guarded, poisoned) allocation seam
        g.check()
    tok = tok.cpu().numpy()
    assert tok.shape == (7,) and tok.min() >= 0 and tok.max() < V, tok
    assert int(tok[0]) == tok0
    for r in ordinary:
        alone = F.sample_tokens(dev[r:r + 1], ut[r:r + 1], T, k, p, **tr)
        assert int(alone[0]) == int(tok[r]) and np.isfinite(x[r, int(tok[r])].item()), r


# ---------------------------------------------------------------------------------------------------------------------------------------
# 5. the truncation decode session (G1 geometry of tests/test_hip_decode.py)
# ---------------------------------------------------------------------------------------------------------------------------------------
TRUNC = dict(min_p=0.02, typical_p=0.9, epsilon_cutoff=2e-3, eta_cutoff=5e-3)


@pytest.fixture(scope="module")
def base_run(g1):
    """the replayed run of seed 1 under TRUNC with the recorder installed: (tokens, recorded logits, u_all, the session)"""
    D, model, inputs = g1
    rec = _SampleRecorder()
    out = sampled(model, inputs, 1, rec=rec, **TRUNC)
    sess = rec.session
    return out, sess._rec.clone().cpu(), sess.u_all.clone().cpu(), sess


@pytest.mark.gpu
def test_session_truncates_under_graph_replay_and_matches_the_reference(g1, base_run):
    """(a) a truncation session exists under its own key and its graph really runs; (b) every decidable (row, step) equals the float64
    reference on the recorded logits and the session's own random numbers.  Undecidable: a mass decision (top_p, typical_p, u against the
    CDF ends) within EDGE, a probability decision within REL_MARGIN, or a kept set that changes under H +- DELTA_H; at most 5 %."""
    from flamingo_mini_amd import decoding
    D, model, inputs = g1
    out, logits, u_all, sess = base_run
    want_t = decoding.Truncation(**TRUNC)
    mine = {key: s for key, s in model._decode_sessions.items() if s.truncation is not None}
    assert sess in mine.values() and sess.truncation == want_t and sess.sampling == (0.8, 20, 0.9)
    assert all(len(key) == 11 and key[-1] == want_t for key in mine)
    assert sess.replay is not None and not sess.capture_failed
    assert out.shape == (7, D.MAXLEN) and torch.equal(out[:, :D.L0], inputs[0])
    gen = out[:, D.L0:].cpu().numpy()
    T, k, p = sess.sampling
    undecidable, bad, cut = 0, [], 0
    for r in range(7):
        for pos in range(D.L0, D.MAXLEN):
            x = logits[r, pos].double().numpy()
            assert np.isfinite(x).all()
            u = float(u_all[pos, r])
            ok, ref = tc.decidable(x, T, k, p, TRUNC, mass_edge=EDGE, u=u)
            if not ok:
                undecidable += 1
                continue
            cut += int(ref.K.sum() < tc.chain(x, T, k, p).K.sum())
            want = ref.token(u)
            if want != gen[r, pos - D.L0]:
                bad.append((r, pos, int(gen[r, pos - D.L0]), want))
    total = 7 * (D.MAXLEN - D.L0)
    print(f"MEASURED undecidable {undecidable} of {total} ({100.0 * undecidable / total:.1f} %); the four rules cut the kept set in {cut} steps")
    assert not bad, f"(row, position, got, want): {bad[:8]}"
    assert undecidable <= 0.05 * total, undecidable
    assert cut > 0, "the rules never cut anything at these settings: the comparison shows nothing"


@pytest.mark.gpu
def test_session_eager_steps_equal_the_replayed_graph_and_the_seed_decides(g1, base_run):
    """(c) the same seed with decode_graph = False: bit-identical ids; (d) the same seed again: the same ids, another seed: others"""
    D, model, inputs = g1
    rec = _SampleRecorder()
    eager = sampled(model, inputs, 1, graph=False, rec=rec, **TRUNC)
    assert rec.session.replay is None and rec.session is not base_run[3] and rec.session.truncation is not None
    assert torch.equal(eager, base_run[0])
    assert torch.equal(sampled(model, inputs, 1, **TRUNC), base_run[0])
    assert not torch.equal(sampled(model, inputs, 2, **TRUNC), base_run[0])


@pytest.mark.gpu
def test_a_plain_sampling_call_afterwards_is_what_it_was(g1, base_run):
    """(e) sampling without the rules after a truncation session: the 10-element key it always built, and ff_sample_token - never the new
    entry - is what its steps issue"""
    from flamingo_mini_amd import ffi
    D, model, inputs = g1
    lib = ffi.lib()
    calls = {"ff_sample_token": 0, "ff_sample_token_truncated": 0}
    orig = {n: getattr(lib, n) for n in calls}

    def counting(n):
        def f(*a):
            calls[n] += 1
            return orig[n](*a)
        return f

    before = set(model._decode_sessions)
    for n in calls:
        setattr(lib, n, counting(n))
    try:
        out = sampled(model, inputs, 1)
    finally:
        for n in calls:
            setattr(lib, n, orig[n])
    new = set(model._decode_sessions) - before
    plain = [key for key in model._decode_sessions if key[7] == tuple(SAMPLING.values()) and len(key) == 10]
    assert plain and all(model._decode_sessions[key].truncation is None for key in plain), (new, list(model._decode_sessions))
    assert calls["ff_sample_token"] > 0 and calls["ff_sample_token_truncated"] == 0, calls
    assert out.shape == (7, D.MAXLEN)
