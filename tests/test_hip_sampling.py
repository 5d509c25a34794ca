"""Sampled token selection on the MI355X: ff_sample_token / functional.sample_tokens (csrc/ff_sample.hip) and the sampling _DecodeSession.

The reference is a float64 numpy restatement of the four rules of include/flamingo_fusion.h, applied to the logits exactly as stored
(bf16 values are widened, never re-rounded):
  1. K = {i : x_i >= the top_k-th largest x}           (ties with it all kept; top_k = 0 or >= V: everything)
  2. q_i = exp(x_i / T - max) / sum over K
  3. P = {i in K : mass of the STRICTLY larger values of K < top_p}
  4. token = the smallest i in P whose inclusive prefix sum over P in index order exceeds u * S,  S = sum of q over P

A sampled token is a discontinuous function of its inputs, so the tests never compare near a decision: they PLACE top_p in the middle of a
distinct-value group's mass interval (group mass >= 2e-3: the nucleus boundary is >= 1e-3 away from any decision) and u in the middle of a
kept token's CDF interval (kept-normalised probability >= 2e-3), assert those preconditions, and then ask for exact equality on every row.
The 1e-3 margin is derived: an fp32 sum of V <= 70001 positive terms with 256-way partials carries a relative error of about
(V / 256 + 8) 2^-24 = 1.7e-5, plus a few ulp for exp - the margin is about 50 times that."""
import contextlib

import numpy as np
import pytest
import torch

BF16, F32 = torch.bfloat16, torch.float32
GROUP_MASS = 2e-3        # least mass of the distinct-value group top_p is placed in
TOKEN_MASS = 2e-3        # least kept-normalised probability of a token u is placed on


# ---------------------------------------------------------------------------------------------------------------------------------------
# float64 reference
# ---------------------------------------------------------------------------------------------------------------------------------------
class Ref:
    """The rules for one row x (float64, as stored) under (T, k): K, q, the distinct-value groups; then, per top_p, P."""

    def __init__(self, x, T, k):
        x = np.asarray(x, dtype=np.float64)
        V = x.size
        self.x, self.V = x, V
        if 0 < k < V:
            kth = np.sort(x)[V - k]
            self.K = x >= kth
        else:
            self.K = np.ones(V, dtype=bool)
        z = x / T
        with np.errstate(invalid="ignore", over="ignore"):
            e = np.where(self.K, np.exp(z - z[self.K].max()), 0.0)
        self.q = e / e.sum()
        # distinct values, descending; group g holds mass gm[g], the strictly larger values hold above[g]
        vals, inv = np.unique(x, return_inverse=True)
        gm = np.bincount(inv.reshape(-1), weights=self.q, minlength=vals.size)[::-1]
        self.group_of = (vals.size - 1 - inv).reshape(-1)
        self.gm = gm
        self.above = np.concatenate([[0.0], np.cumsum(gm)[:-1]])

    def kept(self, p):
        return self.K & (self.above[self.group_of] < p) if p < 1 else self.K.copy()

    def place_p(self, near=0.7):
        """top_p in the middle of the mass interval of a group of mass >= GROUP_MASS (the one whose middle is nearest `near`)"""
        mid = self.above + 0.5 * self.gm
        ok = np.nonzero(self.gm >= GROUP_MASS)[0]
        assert ok.size > 0, "no distinct-value group heavy enough to place top_p in"
        g = ok[np.argmin(np.abs(mid[ok] - near))]
        p = float(mid[g])
        assert 0 < p < 1 and self.gm[g] >= GROUP_MASS
        assert np.abs(self.above - p).min() >= 0.5 * GROUP_MASS * (1 - 1e-9)          # every decision is >= 1e-3 away
        return p

    def cdf(self, p):
        P = self.kept(p)
        w = np.where(P, self.q, 0.0)
        S = w.sum()
        return P, w / S, np.cumsum(w) / S

    def token(self, p, u):
        P, r, c = self.cdf(p)
        hit = np.nonzero(P & (c > u))[0]
        return int(hit[0]) if hit.size else int(np.nonzero(P)[0][-1])

    def place_u(self, p):
        """[(u, token)]: u in the middle of the CDF interval of the first, the heaviest and the last (in index order) kept token whose
        kept-normalised probability is >= TOKEN_MASS"""
        P, r, c = self.cdf(p)
        heavy = np.nonzero(P & (r >= TOKEN_MASS))[0]
        assert heavy.size > 0, "no kept token heavy enough to place u on"
        out = []
        for i in (heavy[0], heavy[np.argmax(r[heavy])], heavy[-1]):
            u = float(np.float32(c[i] - 0.5 * r[i]))
            assert r[i] >= TOKEN_MASS and c[i] - r[i] + 0.25 * r[i] < u < c[i] - 0.25 * r[i] and 0 <= u < 1
            assert self.token(p, u) == i
            out.append((u, int(i)))
        return out


def make_logits(rows, V, dtype, seed, scale=4.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn((rows, V), generator=g, dtype=torch.float32) * scale).to(dtype)


def run_kernel(x, u, T, k, p, out=None):
    """x: (rows, V) device tensor (any row stride), u: list / array of rows numbers -> tokens as a numpy array"""
    from flamingo_mini_amd import functional as F
    ut = torch.tensor(np.asarray(u, dtype=np.float32), device=x.device)
    return F.sample_tokens(x, ut, T, k, p, out=out).cpu().numpy()


# ---------------------------------------------------------------------------------------------------------------------------------------
# 1. designed rows, exact match
# ---------------------------------------------------------------------------------------------------------------------------------------
# (rows, V, dtype, layout).  Six basic shapes (the caption vocabulary contiguous and as the last position of a longer tensor, small and odd sizes); plus every size at which the launch takes another path: 65536 = the longest bf16 row staged
# in LDS (the largest LDS request), 70001 = a bf16 row re-read through L2, 50258 fp32 = more than one trip of the fp32 row loop.
SHAPES = {
    "b32-V50258-bf16": (32, 50258, BF16, "contiguous"),
    "b7-V50258-bf16-last-of-3": (7, 50258, BF16, "last-of-3"),
    "b5-V1000-f32": (5, 1000, F32, "contiguous"),
    "b3-V257-f32": (3, 257, F32, "contiguous"),
    "b2-V7-f32": (2, 7, F32, "contiguous"),
    "b1-V1-f32": (1, 1, F32, "contiguous"),
    "b1-V65536-bf16": (1, 65536, BF16, "contiguous"),
    "b2-V70001-bf16": (2, 70001, BF16, "contiguous"),
    "b2-V50258-f32-last-of-3": (2, 50258, F32, "last-of-3"),
}
SETTINGS = [(1.0, 0, 1.0), (0.7, 50, 1.0), (1.0, 0, None), (0.7, 50, None), (1.3, 1, 1.0)]        # None: top_p placed per row (p*)


@pytest.mark.gpu
@pytest.mark.parametrize("shape", list(SHAPES))
def test_designed_rows_match_the_reference_exactly(shape):
    rows, V, dtype, layout = SHAPES[shape]
    x = make_logits(rows, V, dtype, seed=1000 + V + rows)
    x64 = x.double().numpy()
    # every row three times (one per placed u), in the layout under test
    rep = x.repeat_interleave(3, 0)
    if layout == "last-of-3":
        full = torch.full((3 * rows, 3, V), 99.0, dtype=dtype)           # the other positions would win every draw if they were read
        full[:, -1] = rep
        dev = full.cuda()[:, -1]
        assert dev.stride(0) == 3 * V and not dev.is_contiguous()
    else:
        dev = rep.cuda()
    bad = []
    for T, k, p_set in SETTINGS:
        refs = [Ref(x64[r], T, k) for r in range(rows)]
        ps = [ref.place_p() if p_set is None else p_set for ref in refs]
        placed = [ref.place_u(p) for ref, p in zip(refs, ps)]
        if p_set is None:                                               # top_p differs per row: one launch per row's three replicas
            got = np.concatenate([run_kernel(dev[3 * r:3 * r + 3], [u for u, _ in placed[r]], T, k, ps[r]) for r in range(rows)])
        else:
            got = run_kernel(dev, [u for pl in placed for u, _ in pl], T, k, p_set)
        want = np.array([t for pl in placed for _, t in pl])
        assert got.shape == want.shape
        bad += [((T, k, ps[j // 3]), j // 3, int(got[j]), int(want[j])) for j in np.nonzero(got != want)[0]]
    assert not bad, f"{len(bad)} (setting, row, got, want) differ: {bad[:8]}"


# ---------------------------------------------------------------------------------------------------------------------------------------
# 2. stratified histogram
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("V,N", [(1000, 4096), (50258, 256)])
@pytest.mark.parametrize("setting", [(0.7, 50, None), (1.0, 0, 1.0)])
def test_stratified_draws_follow_the_distribution(V, N, setting):
    """One row drawn N times with u_j = (j + 0.5) / N.  Every token lies in the reference's kept set - exactly: no masked and no filtered
    entry is ever drawn - and every token's count is within 3 of N q_i / S: stratification allows 1 per interval end, an end displaced by
    rounding 1 more per end (N x 1e-5 < 1)."""
    T, k, p = setting
    x = make_logits(1, V, BF16, seed={1000: 2, 50258: 50265}[V])          # (seeds whose kept set holds several tokens: asserted below)
    if V == 1000:
        x[0, torch.randperm(V, generator=torch.Generator().manual_seed(3))[:V // 2]] = float("-inf")
    ref = Ref(x[0].double().numpy(), T, k)
    if p is None:
        p = ref.place_p(near=0.9)
    P, r, _ = ref.cdf(p)
    u = (np.arange(N) + 0.5) / N
    got = run_kernel(x.cuda().repeat(N, 1), u, T, k, p)
    assert got.min() >= 0 and got.max() < V
    assert P[got].all(), f"tokens outside the kept set: {sorted(set(got[~P[got]].tolist()))[:8]}"
    assert np.isfinite(ref.x[got]).all()
    count = np.bincount(got, minlength=V)
    dev = np.abs(count - N * r)
    assert dev.max() <= 3, (int(dev.argmax()), int(count[dev.argmax()]), float(N * r[dev.argmax()]))
    assert (count > 0).sum() >= 5                                        # a real distribution, not one spike


# ---------------------------------------------------------------------------------------------------------------------------------------
# 3. rows whose token is unspecified stay in range; the output is written inside its bounds only
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("V,dtype", [(50258, BF16), (1000, F32), (70001, BF16)])
def test_unspecified_rows_stay_in_range_and_neighbours_are_unharmed(V, dtype):
    from guarded import guarded_allocations
    from flamingo_mini_amd import functional as F
    T, k = 0.7, 50
    x = make_logits(7, V, dtype, seed=11 + V)
    x[1, V // 3] = float("nan")
    x[3, V - 1] = float("inf")
    x[5] = float("-inf")
    ordinary = [0, 2, 4, 6]
    refs = {r: Ref(x[r].double().numpy(), T, k) for r in ordinary}
    # one top_p for the whole launch: the middle of a heavy group of row 0 that is also >= 1e-3 clear of every other ordinary row's decisions
    clear = lambda q: all(np.abs(refs[r].above - q).min() >= 0.5 * GROUP_MASS * (1 - 1e-9) for r in ordinary)
    mids = [float(refs[0].above[g] + 0.5 * refs[0].gm[g]) for g in np.nonzero(refs[0].gm >= GROUP_MASS)[0]]
    mids = [q for q in sorted(mids, key=lambda q: abs(q - 0.7)) if 0 < q < 1 and clear(q)]
    assert mids, "no top_p is clear of every ordinary row's decisions"
    p = mids[0]
    placed = {r: refs[r].place_u(p)[1] for r in ordinary}                # the heaviest token
    u = [placed[r][0] if r in placed else 0.5 for r in range(7)]
    dev = x.cuda()
    ut = torch.tensor(u, dtype=torch.float32, device="cuda")
    for p_run in (p, 1.0):
        with guarded_allocations() as g:
            tok = F.sample_tokens(dev, ut, T, k, p_run)                  # the output comes from the (guarded, poisoned) allocation seam
            g.check()
        tok = tok.cpu().numpy()
        assert tok.shape == (7,) and tok.min() >= 0 and tok.max() < V, tok
        if p_run == p:
            assert [int(tok[r]) for r in ordinary] == [placed[r][1] for r in ordinary]
        else:
            assert [int(tok[r]) for r in ordinary] == [refs[r].token(1.0, placed[r][0]) for r in ordinary]


# ---------------------------------------------------------------------------------------------------------------------------------------
# 4. the sampling decode session (G1 geometry of tests/test_hip_decode.py)
# ---------------------------------------------------------------------------------------------------------------------------------------
SAMPLING = dict(temperature=0.8, top_k=20, top_p=0.9)
EDGE = 1e-4              # a (row, step) is decidable when u S and top_p are this far (in kept mass) from every decision


class _SampleRecorder:
    """Wraps _DecodeSession._append / .run: every _append copies the logits it draws from into `session._rec[:, pos]` on the device (so
    it is captured and runs under replay), and run() leaves the session in `self.session` (its u_all holds the call's random numbers)."""

    def __init__(self):
        self.session = None

    @contextlib.contextmanager
    def installed(self):
        from flamingo_mini_amd import modeling_flamingo as MF
        S = MF._DecodeSession
        orig_append, orig_run = S._append, S.run
        rec = self

        def _append(sess, logits):
            if getattr(sess, "_rec", None) is None:
                sess._rec = torch.full((sess.b, sess.max_length, logits.shape[-1]), float("nan"), dtype=torch.float32, device=logits.device)
            sess._rec.index_copy_(1, sess.pos, logits[:, None].float())
            orig_append(sess, logits)

        def run(sess, *a, **kw):
            rec.session = sess
            if getattr(sess, "_rec", None) is not None:
                sess._rec.fill_(float("nan"))
            return orig_run(sess, *a, **kw)

        S._append, S.run = _append, run
        try:
            yield self
        finally:
            S._append, S.run = orig_append, orig_run


@pytest.fixture(scope="module")
def g1():
    import test_hip_decode as D
    model, _ = D.models("gpt2")
    ids, ml, am, vf = D.make_inputs(7, 1, "G1-b7")
    model.reset_decode_sessions()
    yield D, model, (ids, ml, am, vf)
    model.decode_graph = True
    model.reset_decode_sessions()
    D._MODELS.clear()


def sampled(model, inputs, seed, graph=True, eos=None, rec=None, **over):
    ids, ml, am, vf = inputs
    import test_hip_decode as D
    model.decode_graph = graph
    gen = torch.Generator(device="cuda").manual_seed(seed)
    kw = dict(SAMPLING, **over)
    with (rec.installed() if rec is not None else contextlib.nullcontext()):
        out = model.generate(ids, media_locations=ml, attention_mask=am, visual_features=vf, max_length=D.MAXLEN, do_sample=True,
                             static_decode=True, eos_token_id=eos, generator=gen, **kw)
    model.decode_graph = True
    return out


@pytest.fixture(scope="module")
def base_run(g1):
    """the replayed run of seed 1 with the recorder installed: (tokens, recorded logits, u_all, the session)"""
    D, model, inputs = g1
    rec = _SampleRecorder()
    out = sampled(model, inputs, 1, rec=rec)
    sess = rec.session
    return out, sess._rec.clone().cpu(), sess.u_all.clone().cpu(), sess


@pytest.mark.gpu
def test_session_samples_under_graph_replay_and_matches_the_reference(g1, base_run):
    """(a) a sampling session exists and its graph really runs; (b) every decidable (row, step) equals the float64 reference on the recorded
    logits and the session's own random numbers; at most 5 % may be undecidable (about 21 interval ends x 2e-4 = 0.4 % is expected; at
    V = 320 the summation error is about 1e-6, far inside EDGE)."""
    D, model, inputs = g1
    out, logits, u_all, sess = base_run
    mine = [s for s in model._decode_sessions.values() if s.sampling is not None]
    assert mine and sess in mine and sess.sampling == (0.8, 20, 0.9)
    assert sess.replay is not None and not sess.capture_failed
    assert out.shape == (7, D.MAXLEN) and torch.equal(out[:, :D.L0], inputs[0])
    gen = out[:, D.L0:].cpu().numpy()
    T, k, p = sess.sampling
    undecidable, bad = 0, []
    for r in range(7):
        for pos in range(D.L0, D.MAXLEN):
            x = logits[r, pos].double().numpy()
            assert np.isfinite(x).all()
            ref = Ref(x, T, k)
            P, _, c = ref.cdf(p)
            u = float(u_all[pos, r])
            ends = np.concatenate([[0.0], c[P]])
            if np.abs(ends - u).min() < EDGE or np.abs(ref.above - p).min() < EDGE:
                undecidable += 1
                continue
            want = ref.token(p, u)
            if want != gen[r, pos - D.L0]:
                bad.append((r, pos, int(gen[r, pos - D.L0]), want))
    total = 7 * (D.MAXLEN - D.L0)
    print(f"MEASURED undecidable {undecidable} of {total}")
    assert not bad, f"(row, position, got, want): {bad[:8]}"
    assert undecidable <= 0.05 * total, undecidable


@pytest.mark.gpu
def test_session_eager_steps_equal_the_replayed_graph(g1, base_run):
    """(c) the same seed with decode_graph = False: bit-identical ids"""
    D, model, inputs = g1
    rec = _SampleRecorder()
    eager = sampled(model, inputs, 1, graph=False, rec=rec)
    assert rec.session.replay is None and rec.session is not base_run[3]
    assert torch.equal(eager, base_run[0])


@pytest.mark.gpu
def test_session_is_reproducible_per_seed_and_stops_at_eos(g1, base_run):
    """(d) the same seed twice gives the same ids, another seed others; (e) with eos = a token row 0 sampled, every row is padded after its
    first eos and the returned length follows the greedy path's n_new rule (tokens appended while some row was still alive)."""
    D, model, inputs = g1
    full = base_run[0]
    again = sampled(model, inputs, 1)
    other = sampled(model, inputs, 2)
    assert torch.equal(again, full) and not torch.equal(other, full)
    gen = full[:, D.L0:]
    eos = int(gen[0, 5])
    stop = [int((gen[i] == eos).nonzero()[0, 0]) + D.L0 if bool((gen[i] == eos).any()) else D.MAXLEN - 1 for i in range(gen.shape[0])]
    assert stop[0] <= D.L0 + 5
    want = full.clone()
    for i, s in enumerate(stop):
        want[i, s + 1:] = eos
    want = want[:, :max(stop) + 1]
    got = sampled(model, inputs, 1, eos=eos)
    assert got.shape == want.shape and torch.equal(got, want), (eos, got, want)
    assert bool((got[0, stop[0] + 1:] == eos).all())


@pytest.mark.gpu
def test_session_top_k_one_is_greedy(g1):
    """(f) top_k = 1 keeps the maximum alone, whatever u is - given that the maximum is unique at every step, which is asserted"""
    D, model, inputs = g1
    ids, ml, am, vf = inputs
    rec = _SampleRecorder()
    out = sampled(model, inputs, 5, rec=rec, top_k=1)
    lg = rec.session._rec[:, D.L0:]
    top2 = lg.topk(2, dim=-1).values
    assert bool((top2[..., 0] > top2[..., 1]).all()), "a step's maximum is not unique: top_k = 1 keeps the ties"
    greedy = model.greedy_generate(ids, ml, am, visual_features=vf, max_length=D.MAXLEN)
    assert torch.equal(out, greedy)
