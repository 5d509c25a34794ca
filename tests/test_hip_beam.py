"""Beam search on the graph-replayed decode path, on the GPU: ff_beam_step (functional.beam_step) against the numpy restatement of its
rules (tests/beam_cases.py) on designed steps and over a scripted multi-step search with eos events, ff_beam_gather (functional.beam_gather)
bitwise on guarded, poisoned cache tensors, eager and replayed, and the beam _DecodeSession of FlamingoModel.generate(num_beams=3,
static_decode=True).

SCORE_BOUND, the distance allowed between a score the kernel writes and the float64 value of the same candidate (rules 1-3 on the same
inputs), follows from the kernel's summation structure for rows of at most 2^17 columns, |x - max| <= 64, |lse| < 32, |logp| < 64,
|score| < 128, with u = 2^-24:
  sum exp(x - max): a thread adds at most V / 256 + 8 <= 282 terms one after another, then 6 butterfly and 3 wave additions: <= 291 u
  relative; expf <= 4 u relative; the rounding of x - max moves a term by <= 64 u relative.  Together <= 359 u = 2.2e-5 relative in the sum,
  the same absolute in its logarithm;
  logf (2 ulp at <= 16): 1.9e-6;  max + log: 0.95e-6;  x - lse: 1.9e-6;  score + logp: 3.8e-6.
Total 3.1e-5 <= SCORE_BOUND = 4e-5, and the designed margin 1e-3 is 25 x that (>= 20 x).  Measured worst on the designed steps: see the
MEASURED line (DESIGN.md records it)."""
import contextlib

import numpy as np
import pytest
import torch

import beam_cases as BC

BF16, F32 = torch.bfloat16, torch.float32
SCORE_BOUND = 4e-5
MARGIN = 1e-3
assert MARGIN >= 20 * SCORE_BOUND
INT_FIELDS = ("done", "n_hyp", "hyp_len", "hyp_row", "hist_tok", "hist_parent", "next_tok", "beam_idx")
FLT_FIELDS = ("score", "hyp_score", "hist_score")
POISON_F = 1.7e38


def same_state(got, want, where=""):
    """Integers exact, scores within SCORE_BOUND (non-finite entries at the same places with the same value).  Returns the worst error."""
    worst = 0.0
    for n in INT_FIELDS:
        assert np.array_equal(got[n], want[n]), (where, n, got[n].tolist(), want[n].tolist())
    for n in FLT_FIELDS:
        g, w = got[n].astype(np.float64), want[n].astype(np.float64)
        fin = np.isfinite(w)
        assert np.array_equal(np.isfinite(g), fin) and np.array_equal(g[~fin], w[~fin]), (where, n, g.tolist(), w.tolist())
        if fin.any():
            err = float(np.abs(g[fin] - w[fin]).max())
            assert err <= SCORE_BOUND, (where, n, err)
            worst = max(worst, err)
    return worst


def poison(state):
    """Everything only the library writes, after reset(): a later comparison of the WHOLE block shows any entry a step should not have touched."""
    for n in ("hist_tok", "hist_parent", "hyp_len", "hyp_row"):
        getattr(state, n).fill_(-77)
    state.hist_score.fill_(POISON_F)


def gaps_decidable(top_s, top_b, designed_ties=False):
    """per sequence: every gap between consecutive finite scores of the best 2 nb + 1 candidates is >= MARGIN - or exactly 0 inside one row
    (equal logits of one beam: equal bits in fp32 too, the flat-index rule decides); designed_ties also admits exact ties across beams"""
    ok = np.ones(top_s.shape[0], bool)
    zero = 0
    for s in range(top_s.shape[0]):
        fin = np.isfinite(top_s[s])
        f, bm = top_s[s][fin].astype(np.float64), top_b[s][fin]
        for i in range(len(f) - 1):
            gap = f[i] - f[i + 1]
            if gap == 0 and (designed_ties or bm[i] == bm[i + 1]):
                zero += 1
            elif gap < MARGIN:
                ok[s] = False
    return ok, zero


# ---------------------------------------------------------------------------------------------------------------------------------------
# 1. designed steps
# ---------------------------------------------------------------------------------------------------------------------------------------
DESIGNED = [  # (b, nb, V, dtype, layout, tie, seed): the seed is one whose planted scores are >= 1e-3 apart in float64 (asserted)
    (4, 3, 50258, BF16, "last-of-2", "beams", 0),
    (2, 3, 50258, F32, "contiguous", "row", 1),
    (3, 8, 257, F32, "contiguous", None, 0),
    (2, 2, 7, F32, "contiguous", None, 0),
    (1, 4, 65536, BF16, "contiguous", None, 0),
    (2, 2, 70001, BF16, "contiguous", None, 0),
    (1, 1, 16, F32, "contiguous", None, 0),
]


def design(b, nb, V, dtype, tie, seed):
    """(logits (b nb, V) float32 on the dtype's grid, score (b, nb) float32, eos): random rows, and per sequence 2 nb + 1 planted candidates
    well above them (12 + j / 4, j a permutation: on the bf16 grid).  tie = "row": two planted candidates of sequence 0 share a row and a
    value.  tie = "beams": beams 0 and nb - 1 of sequence 0 have equal scores and identical rows, so their candidates tie pairwise."""
    g = np.random.default_rng(1000 + seed)
    x = torch.from_numpy((g.standard_normal((b * nb, V)) * 2).astype(np.float32)).to(dtype).float().numpy()
    score = -(g.integers(0, 64, (b, nb)) / 8.0).astype(np.float32)
    n = min(2 * nb + 1, nb * V)
    eos = None
    for s in range(b):
        flat = g.choice(nb * V, n, replace=False)
        vals = 12.0 + 0.25 * g.permutation(n)
        if s == 0:
            eos = int(flat[int(np.argsort(-vals)[1])] % V)                 # the token of sequence 0's second-highest planted logit
        if s == 0 and tie == "row" and nb > 1:
            flat[1] = (flat[0] // V) * V + (flat[0] % V + 3) % V
            vals[1] = vals[0]
        for f, v in zip(flat, vals):
            if s == 0 and tie == "beams" and f // V == nb - 1:
                continue
            x[s * nb + f // V, f % V] = v
        if s == 0 and tie == "beams":
            x[nb - 1] = x[0]
            score[0, nb - 1] = score[0, 0]
    return x, score, eos


def check_designed(x, score, nb, tie):
    top_s, top_b, top_t = BC.candidates(score, x, nb, np.float64)
    ok, zero = gaps_decidable(top_s, top_b, designed_ties=True)
    assert ok.all(), "planted scores closer than the margin"
    assert (zero > 0) == (tie is not None), (zero, tie)
    return top_s, top_b, top_t


@pytest.mark.parametrize("case", DESIGNED, ids=lambda c: f"{c[0]}x{c[1]}x{c[2]}-{str(c[3])[6:]}-{c[4]}-{c[5]}")
def test_designed_cases_are_decidable(case):
    """(no GPU) the precondition of the designed steps, in float64: consecutive planted scores are >= 1e-3 apart, or tie exactly as designed"""
    b, nb, V, dtype, layout, tie, seed = case
    x, score, eos = design(b, nb, V, dtype, tie, seed)
    check_designed(x, score, nb, tie)


@pytest.mark.gpu
@pytest.mark.parametrize("case", DESIGNED, ids=lambda c: f"{c[0]}x{c[1]}x{c[2]}-{str(c[3])[6:]}-{c[4]}-{c[5]}")
def test_designed_steps_match_the_reference_exactly(case):
    """One step from a state with given scores: the whole state block afterwards - chosen (parent, token) lists, hypotheses made of the
    planted eos, histories - equals the float64 reference's, integers exactly, scores within SCORE_BOUND; ties (inside a row, across two
    beams with equal scores and rows) are decided by the flat index.  State and workspace come from the guarded, poisoned seam."""
    from guarded import guarded_allocations
    from flamingo_mini_amd import functional as F
    b, nb, V, dtype, layout, tie, seed = case
    x, score, eos = design(b, nb, V, dtype, tie, seed)
    top_s, top_b, top_t = check_designed(x, score, nb, tie)
    max_len, cur = 8, 5
    xt = torch.from_numpy(x).to(dtype)
    if layout == "last-of-2":
        buf = torch.full((b * nb, 2, V), float("nan"), dtype=dtype)
        buf[:, 1] = xt
        dev = buf.cuda()[:, -1]
    else:
        dev = xt.cuda()
    with guarded_allocations() as g:
        st = F.BeamState(b, nb, max_len, "cuda", eos=eos, pad=1, early_stopping=False, length_penalty=1.0)
        poison(st)
        st.score.copy_(torch.from_numpy(score))
        pre = st.to_host()
        nxt, idx = F.beam_step(dev, st, torch.tensor([cur], device="cuda"))
        post = st.to_host()
        g.check()
    assert nxt.data_ptr() == st.next_tok.data_ptr() and idx.data_ptr() == st.beam_idx.data_ptr()
    ref = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in pre.items()}
    BC.step(ref, x, cur, nb, eos, 1, False, ft=np.float64)
    worst = same_state(post, ref, where=str(case))
    f64 = {(s, int(top_b[s, r]), int(top_t[s, r])): float(top_s[s, r]) for s in range(b) for r in range(top_s.shape[1])}
    for s in range(b):
        for k in range(nb):
            row = s * nb + k
            if np.isfinite(post["score"][s, k]):
                want = f64[(s, int(post["beam_idx"][row]) - s * nb, int(post["next_tok"][row]))]
                worst = max(worst, abs(float(post["score"][s, k]) - want))
    print(f"MEASURED beam_step score error {worst:.3e} (bound {SCORE_BOUND:.1e}) at {case[:4]}")
    assert worst <= SCORE_BOUND


# ---------------------------------------------------------------------------------------------------------------------------------------
# 2. twelve scripted steps: the whole state after every step
# ---------------------------------------------------------------------------------------------------------------------------------------
MS_V, MS_NB, MS_EOS, MS_PAD, MS_MAXLEN = 257, 3, 7, 0, 14
MS_PROMPT = np.array([[1, 11], [2, 12], [3, 13]], np.int64)
MS_BOOST = {1: (4, 9.0), 2: (6, 5.5)}
MS_SEEDS = {True: 48, False: 48}     # a table whose runs keep every margin >= 1e-3 and hold the events (both asserted on the way)


@pytest.mark.gpu
@pytest.mark.parametrize("early", [True, False])
def test_state_block_after_every_step_of_a_scripted_search(early):
    """12 steps, V = 257, 3 sequences x 3 beams, eos at low and high ranks, one sequence done early.  Before every step the device state is
    copied; the restatement (float32) advances the copy and the device state after the step must equal it as a WHOLE (every history row,
    hypothesis and the poisoned entries no step may touch)."""
    from guarded import guarded_allocations
    from flamingo_mini_amd import functional as F
    script = BC.Script(MS_V, MS_SEEDS[early], eos=MS_EOS, eos_boost=MS_BOOST)
    events, worst = {}, 0.0
    hist = np.repeat(MS_PROMPT, MS_NB, axis=0)
    with guarded_allocations() as g:
        st = F.BeamState(3, MS_NB, MS_MAXLEN, "cuda", eos=MS_EOS, pad=MS_PAD, early_stopping=early, length_penalty=1.0)
        poison(st)
        cur = torch.zeros(1, dtype=torch.long, device="cuda")
        for cur_len in range(3, MS_MAXLEN + 1):
            pre = st.to_host()
            logits = script(hist)
            cur.fill_(cur_len)
            F.beam_step(torch.from_numpy(logits).cuda(), st, cur)
            post = st.to_host()
            ref = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in pre.items()}
            live = ref["done"] == 0
            top = BC.step(ref, logits, cur_len, MS_NB, MS_EOS, MS_PAD, early, events=events)
            assert BC.min_margin(top)[live].min(initial=np.inf) >= MARGIN, f"step {cur_len} of the script is not decidable"
            worst = max(worst, same_state(post, ref, where=f"step {cur_len}"))
            hist = np.concatenate([hist[post["beam_idx"]], post["next_tok"][:, None]], axis=1)
        g.check()
    print(f"MEASURED multi-step score error {worst:.3e}; events {events}")
    assert events.get("eos_low", 0) > 0 and events.get("eos_high", 0) > 0 and events.get("done", 0) > 0, events


# ---------------------------------------------------------------------------------------------------------------------------------------
# 3. the in-place gather
# ---------------------------------------------------------------------------------------------------------------------------------------
GATHER = [  # (shape (rows, outer, len_max, inner), dtype, nb, tensors in the table)
    ((6, 4, 23, 16), BF16, 3, 2), ((6, 4, 23, 16), BF16, 3, 72), ((6, 4, 23, 16), F32, 3, 2), ((6, 4, 23, 16), F32, 3, 72),
    ((96, 20, 24, 64), BF16, 3, 2), ((6, 4, 23, 6), BF16, 3, 2), ((6, 4, 23, 6), F32, 2, 72),
]


def beam_idx_cases(rows, nb, g):
    base = np.arange(rows) // nb * nb
    rep = base + g.integers(0, nb, rows)
    rep[:nb] = base[:nb] + min(1, nb - 1)                                   # one sequence whose rows all take one parent
    return {"identity": np.arange(rows), "repeated": rep, "rotation": base + (np.arange(rows) % nb + 1) % nb}


def bits(t):
    return t.view(torch.int16 if t.element_size() == 2 else torch.int32)


def fill_cache(t, n_pos, seed):
    """random bits at the live positions, a NaN pattern behind them"""
    gen = torch.Generator(device="cuda").manual_seed(seed)
    bits(t).copy_(torch.randint(-30000, 30000, t.shape, generator=gen, device="cuda"))
    t[:, :, n_pos:] = float("nan")


@pytest.mark.gpu
@pytest.mark.parametrize("shape,dtype,nb,n_tensors", GATHER, ids=lambda v: str(v).replace("torch.", "").replace(" ", ""))
def test_gather_moves_the_live_positions_and_nothing_else(shape, dtype, nb, n_tensors):
    """p < n_pos: bitwise before[beam_idx]; p >= n_pos: bitwise unchanged; guards intact.  Tables of 72 tensors take two launches."""
    from guarded import guarded_allocations
    from flamingo_mini_amd import functional as F
    g = np.random.default_rng(7)
    rows, outer, len_max, inner = shape
    with guarded_allocations() as guards:
        ts = [F._new(shape, dtype, "cuda") for _ in range(n_tensors)]
        n_pos_dev = torch.zeros(1, dtype=torch.long, device="cuda")
        for name, idx in beam_idx_cases(rows, nb, g).items():
            idx_dev = torch.from_numpy(idx).cuda()
            for n_pos in (0, 1, 7, len_max):
                for i, t in enumerate(ts):
                    fill_cache(t, n_pos, 31 * i + n_pos)
                check = ts if n_tensors <= 2 else [ts[0], ts[47], ts[48], ts[71]]          # (both launches of a split table, both ends)
                before = [bits(t).clone() for t in check]
                n_pos_dev.fill_(n_pos)
                F.beam_gather(ts, idx_dev, n_pos_dev, nb)
                for t, b0 in zip(check, before):
                    want = b0.clone()
                    want[:, :, :n_pos] = b0[idx_dev][:, :, :n_pos]
                    assert torch.equal(bits(t), want), (name, n_pos)
        guards.check()


@pytest.mark.gpu
def test_gather_replays_with_device_side_arguments():
    """captured once, replayed twice with n_pos and beam_idx changed on the device in between"""
    from flamingo_mini_amd import functional as F
    shape, nb = (6, 4, 23, 16), 3
    ts = [torch.empty(shape, dtype=BF16, device="cuda") for _ in range(2)]
    idx_dev = torch.arange(6, device="cuda")
    n_pos_dev = torch.zeros(1, dtype=torch.long, device="cuda")
    for t in ts:
        fill_cache(t, 23, 5)
    F.beam_gather(ts, idx_dev, n_pos_dev, nb)                               # (eager once: identity, nothing live)
    graph = torch.cuda.CUDAGraph()
    torch.cuda.synchronize()
    with torch.cuda.graph(graph):
        F.beam_gather(ts, idx_dev, n_pos_dev, nb)
    cases = beam_idx_cases(6, nb, np.random.default_rng(3))
    for n_pos, name in ((7, "rotation"), (23, "repeated")):
        before = [bits(t).clone() for t in ts]
        n_pos_dev.fill_(n_pos)
        idx_dev.copy_(torch.from_numpy(cases[name]).cuda())
        graph.replay()
        for t, b0 in zip(ts, before):
            want = b0.clone()
            want[:, :, :n_pos] = b0[idx_dev][:, :, :n_pos]
            assert torch.equal(bits(t), want), (name, n_pos)


# ---------------------------------------------------------------------------------------------------------------------------------------
# 4. the beam decode session (G1 geometry of tests/test_hip_decode.py, batch 4, 3 beams)
# ---------------------------------------------------------------------------------------------------------------------------------------
NB = 3
TAG = "beam"


def beam_generate(model, inputs, max_length, graph=True, rec=None, **kw):
    ids, ml, am, vf = inputs
    model.decode_graph = graph
    with (rec.installed() if rec is not None else contextlib.nullcontext()):
        out = model.generate(ids, media_locations=ml, attention_mask=am, visual_features=vf, max_length=max_length, num_beams=NB,
                             static_decode=True, **kw)
    model.decode_graph = True
    return out


def replay_restatement(sess, logits, L0, length, eos, early, lp):
    """The restatement (float32) driven by the logits the session recorded: the final state, with "length" and "eos"."""
    b = sess.n_seq
    st = BC.new_state(b, NB, sess.max_length, lp, sess.fill)
    for pos in range(L0, length):
        BC.step(st, logits[:, pos], pos + 1, NB, eos, sess.fill, early)
    st["length"], st["eos"] = length, -1 if eos is None else eos
    return st


@pytest.fixture(scope="module")
def g1():
    import test_hip_decode as D
    model, model64 = D.models("gpt2")
    inputs = D.make_inputs(4, 1, TAG)
    model.reset_decode_sessions()
    yield D, model, model64, inputs
    model.decode_graph = True
    model.reset_decode_sessions()
    D._MODELS.clear()


@pytest.fixture(scope="module")
def base_run(g1):
    """the replayed run without eos, recorder installed: (ids, recorded logits (rows, max_length, V), host state, session)"""
    from test_hip_sampling import _SampleRecorder
    D, model, _, inputs = g1
    rec = _SampleRecorder()
    out = beam_generate(model, inputs, D.MAXLEN, rec=rec)
    sess = rec.session
    return out, sess._rec.clone().cpu().numpy(), sess.state.to_host(), sess


@pytest.mark.gpu
def test_session_replays_a_graph_and_every_step_follows_the_rules(g1, base_run):
    """(a) a beam session exists and its graph really runs; (c) every step's transition - the session's own hist_score before the step plus
    the recorded logits in, the history row after the step out - equals the float64 reference wherever that is decidable (gaps of the best
    2 nb + 1 scores >= 1e-3, or exact ties inside one row); at most 5 % of the (sequence, step) pairs may be undecidable; (d) the returned
    ids are _beam_finalize of the restatement's final state."""
    from flamingo_mini_amd.modeling_flamingo import _beam_finalize
    D, model, _, inputs = g1
    out, logits, host, sess = base_run
    mine = [s for s in model._decode_sessions.values() if s.beams is not None]
    assert mine and sess in mine and sess.beams == (NB, True, 1.0) and sess.b == 4 * NB
    assert sess.replay is not None and not sess.capture_failed
    assert out.shape == (4, D.MAXLEN) and torch.equal(out[:, :D.L0], inputs[0])
    undecidable, bad, worst = 0, [], 0.0
    for pos in range(D.L0, D.MAXLEN):
        x = logits[:, pos]
        assert np.isfinite(x).all()
        prev = BC.new_state(4, NB, 1)["score"] if pos == D.L0 else host["hist_score"][pos - 1].reshape(4, NB)
        top_s, top_b, top_t = BC.candidates(prev, x, NB, np.float64)
        ok, _ = gaps_decidable(top_s, top_b)
        for s in range(4):
            if not ok[s]:
                undecidable += 1
                continue
            r = slice(s * NB, (s + 1) * NB)
            got = (host["hist_tok"][pos, r].tolist(), host["hist_parent"][pos, r].tolist())
            want = (top_t[s, :NB].tolist(), (s * NB + top_b[s, :NB]).tolist())
            if got != want:
                bad.append((s, pos, got, want))
            else:
                worst = max(worst, float(np.abs(host["hist_score"][pos, r].astype(np.float64) - top_s[s, :NB]).max()))
    total = 4 * (D.MAXLEN - D.L0)
    print(f"MEASURED undecidable {undecidable} of {total}; session score error {worst:.3e}")
    assert not bad, f"(sequence, position, got, want): {bad[:4]}"
    assert worst <= SCORE_BOUND
    assert undecidable <= 0.05 * total, undecidable
    st = replay_restatement(sess, logits, D.L0, D.MAXLEN, None, True, 1.0)
    assert torch.equal(out.cpu(), _beam_finalize(st, D.L0, inputs[0].cpu(), NB, sess.fill))


@pytest.mark.gpu
def test_session_eager_steps_equal_the_replayed_graph(g1, base_run):
    """(b) decode_graph = False: the same ids, bit for bit"""
    D, model, _, inputs = g1
    eager = beam_generate(model, inputs, D.MAXLEN, graph=False)
    sess = [s for s in model._decode_sessions.values() if s.beams is not None and not s.graph_wanted]
    assert sess and sess[0].replay is None
    assert torch.equal(eager, base_run[0])


@pytest.mark.gpu
def test_session_beams_are_at_least_as_likely_as_greedy(g1, base_run):
    """(e) the float64 teacher-forced log-probability of the returned sequences is at least greedy's, up to the two sequences' summed bf16
    rounding (the construction and TOL_LOGPROB of test_hip_decode.test_beam_search_on_gpu)"""
    D, model, model64, (ids, ml, am, vf) = g1
    beams = base_run[0]
    greedy = model.greedy_generate(ids, ml, am, visual_features=vf, max_length=D.MAXLEN)
    assert beams.shape == greedy.shape

    def logprobs(seq):
        lp64 = D.teacher_forced_f64(model64, seq, ml, am, vf).log_softmax(-1)[:, D.L0 - 1:-1].gather(-1, seq[:, D.L0:, None].cpu())[..., 0]
        mlf, amf = D.extend(ml, am, seq.shape[1])
        with torch.no_grad():
            lg = model(input_ids=seq, attention_mask=amf, media_locations=mlf, visual_features=vf).logits.float().log_softmax(-1)
        return lp64, lg[:, D.L0 - 1:-1].gather(-1, seq[:, D.L0:, None])[..., 0].double().cpu()

    lb64, lbg = logprobs(beams)
    lg64, lgg = logprobs(greedy)
    tok_err = max(float((lb64 - lbg).abs().max()), float((lg64 - lgg).abs().max()))
    print(f"MEASURED logprob-token {tok_err:.3e}; beam-minus-greedy(min) {float((lb64.sum(1) - lg64.sum(1)).min()):.3e}")
    assert tok_err < D.TOL_LOGPROB
    slack = (lb64 - lbg).abs().sum(1) + (lg64 - lgg).abs().sum(1)
    assert bool((lb64.sum(1) >= lg64.sum(1) - slack).all()), (lb64.sum(1), lg64.sum(1), slack)


@pytest.mark.gpu
@pytest.mark.parametrize("early,lp", [(True, 0.0), (False, 0.0)])
def test_session_stops_at_eos_and_pads(g1, base_run, early, lp):
    """(f) with an eos the run above produced (its most frequent token): replayed and eager runs agree, the ids are _beam_finalize of the restatement driven
    by the recorded logits, and every returned row is padding after its eos.  length_penalty 0: scores are not normalised, so a finished
    hypothesis beats the longer open beams of its sequence and some returned rows do end in the eos (with 1.0 this model's open beams win)."""
    from flamingo_mini_amd.modeling_flamingo import _beam_finalize
    from test_hip_sampling import _SampleRecorder
    D, model, _, inputs = g1
    gen = base_run[0][:, D.L0:]
    eos = max((int(t) for t in gen.flatten().unique()), key=lambda t: int((gen == t).sum()))       # the most frequent generated token
    pad = 0 if eos != 0 else 1
    kw = dict(eos_token_id=eos, pad_token_id=pad, early_stopping=early, length_penalty=lp)
    rec = _SampleRecorder()
    out = beam_generate(model, inputs, D.MAXLEN, rec=rec, **kw)
    sess = rec.session
    assert sess.replay is not None and sess.beams == (NB, early, lp)
    logits, host = sess._rec.clone().cpu().numpy(), sess.state.to_host()
    assert torch.equal(out, beam_generate(model, inputs, D.MAXLEN, graph=False, **kw))
    assert out.shape[1] <= D.MAXLEN and torch.equal(out[:, :D.L0], inputs[0])
    n_eos = 0
    for row in out[:, D.L0:].cpu().tolist():
        if eos in row:
            n_eos += 1
            assert all(t == pad for t in row[row.index(eos) + 1:]), (eos, pad, row)
    print(f"MEASURED eos {eos}: {n_eos} of 4 returned rows end in it, hypotheses {host['n_hyp'].tolist()}, done {host['done'].tolist()}")
    assert n_eos > 0 and int(host["n_hyp"].sum()) > 0, "the eos was never produced"
    st = replay_restatement(sess, logits, D.L0, D.MAXLEN, eos, early, lp)
    assert torch.equal(out.cpu(), _beam_finalize(st, D.L0, inputs[0].cpu(), NB, pad))


@pytest.mark.gpu
def test_session_on_an_opt_model_replays_what_it_runs_eagerly():
    """(g) OPT takes its positions from the attention mask, which the beams of a sequence share: one replayed run equals its eager run"""
    import test_hip_decode as D
    model, _ = D.models("opt")
    inputs = D.make_inputs(4, 1, TAG)
    model.reset_decode_sessions()
    try:
        replayed = beam_generate(model, inputs, D.MAXLEN)
        sess = [s for s in model._decode_sessions.values() if s.beams is not None]
        assert sess and sess[0].replay is not None and not sess[0].capture_failed
        eager = beam_generate(model, inputs, D.MAXLEN, graph=False)
        assert replayed.shape == (4, D.MAXLEN) and torch.equal(replayed, eager)
    finally:
        model.decode_graph = True
        model.reset_decode_sessions()
        D._MODELS.clear()
