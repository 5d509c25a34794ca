"""Beam sampling on the graph-replayed decode path, on the GPU: ff_beam_sample_noise and ff_beam_sample_step (functional.beam_sample_noise /
.beam_sample_step, csrc/ff_beam_sample.hip) against the numpy restatement of rules S1 - S6 (tests/beam_sample_cases.py) - the noise against
float64, designed single steps and a scripted multi-step search as whole state blocks, the law of the draw by a chi-square - and the beam
_DecodeSession of FlamingoModel.generate(num_beams=3, do_sample=True, static_decode=True).

NOISE_BOUND, the distance allowed between the kernel's g = -logf(-logf(u)) and the float64 value for the same u (u itself is exact): the inner
logarithm L = -log u lies in [6e-8, 16.7] and carries a relative error of a few ulp (2 ulp = 2.4e-7), which the outer logarithm turns into
the same ABSOLUTE error; the outer logf adds its own 2 ulp of |g| <= 16.7, 1.9e-6 at most each.  Together 4.1e-6 if both logarithms were 2 ulp off at once.
Measured on an MI355X over rows = 5, vocab = 1031: 1.36e-6 (the MEASURED line of test_noise_matches_the_float64_restatement; DESIGN.md records
it); NOISE_BOUND = 3e-6 is twice the measured maximum, rounded up.
A score the step writes is a of rule S3: test_hip_beam.SCORE_BOUND (derived there for T = 1) covers it for temperatures T >= 0.9 - the
error of logp (2.7e-5 of the 3.1e-5) is divided by T, the division and the addition of the score add 3.8e-6 each at |z|, |a| < 64:
2.7e-5 / 0.9 + 7.6e-6 = 3.8e-5 <= 4e-5.  The designed steps use T in {1, 0.9, 1.5}.  A decision is a comparison of two values of p = a + g or
of a, so the designed margin has to cover 20 x (SCORE_BOUND + NOISE_BOUND), asserted below."""
import contextlib

import numpy as np
import pytest
import torch

import beam_cases as BC
import beam_sample_cases as BSC
from test_hip_beam import MARGIN, SCORE_BOUND, poison, same_state

BF16, F32 = torch.bfloat16, torch.float32
NOISE_BOUND = 3e-6
assert MARGIN >= 20 * (SCORE_BOUND + NOISE_BOUND)


def dev_scalar(v):
    return torch.tensor([int(v)], dtype=torch.long, device="cuda")


# ---------------------------------------------------------------------------------------------------------------------------------------
# 1. the noise
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_noise_matches_the_float64_restatement():
    """rows = 5, vocab = 1031 (no multiple of 4: the last Philox call is cut): |g - g64| <= NOISE_BOUND everywhere, and the integer the
    uniform number came from is recovered: exp(-exp(-g)) 2^23 - 0.5 rounds to w >> 9.  Where u is within 1e-4 of 1 the map from g to u is
    so steep (g -> -inf like log(1 - u)) that fp32 cannot hold the integer, and a logf that is two ulp off moves u by up to u (-log u) 2.4e-7
    = 0.9 grid steps elsewhere; the entries that miss are not located but COUNTED: at most 0.1 % of the entries (the tail's mass is 1e-4)."""
    from flamingo_mini_amd import functional as F
    rows, V, seed, cur = 5, 1031, 0x1234567890ABCDEF, 7
    g = F.beam_sample_noise(rows, V, dev_scalar(seed), dev_scalar(cur)).cpu().numpy()
    w = BSC.words(rows, V, seed, cur)
    g64 = BSC.gumbel(w)
    err = float(np.abs(g.astype(np.float64) - g64).max())
    k = np.rint(np.exp(-np.exp(-g.astype(np.float64))) * 2.0 ** 23 - 0.5).astype(np.int64)
    missed = k != (w >> np.uint32(9)).astype(np.int64)
    print(f"MEASURED beam_sample_noise |g - g64| max {err:.3e} (bound {NOISE_BOUND:.1e}), g in [{g.min():.3f}, {g.max():.3f}]; "
          f"integers missed {int(missed.sum())} of {w.size}, by at most {int(np.abs(k - (w >> np.uint32(9)).astype(np.int64)).max())}")
    assert np.isfinite(g).all() and err <= NOISE_BOUND
    assert missed.sum() <= 1e-3 * w.size, int(missed.sum())


# ---------------------------------------------------------------------------------------------------------------------------------------
# 2. designed single steps
# ---------------------------------------------------------------------------------------------------------------------------------------
WARPERS = {"off": (1.0, 0, 1.0), "topk": (0.9, 5, 1.0), "nucleus": (1.5, 0, 0.9), "both": (1.0, 12, 0.8), "few-threads": (1.0, 0, 1.0)}
_MODES = ("off", "topk", "nucleus", "both")
# (b, nb, V, dtype, mode) -> the kernel seed: the first one for which the float64 restatement decides every comparison of the step by
# MARGIN or by an exact tie (found with seed_for() below on the CPU; test_designed_seeds_are_decidable asserts it for every entry)
DESIGNED = {}
_SEEDS = (0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1, 2, 0, 0, 0, 2, 0, 1)
for _i, (_nb, _V, _dt) in enumerate((nb, V, dt) for nb in (1, 3, 8) for V in (16, 300, 50258) for dt in (BF16, F32)):
    DESIGNED[(3, _nb, _V, _dt, _MODES[(_i + _i // 6) % 4])] = _SEEDS[_i]
# every logit from column 2000 on is -inf: 10 of the 256 threads hold all 2000 finite columns of a row, fewer than 2 nb = 16 thread maxima
# are finite, the bound tau is -inf and the list overflows - the row pass takes its exact fallback (the bisection on the key of p)
DESIGNED[(3, 8, 50258, BF16, "few-threads")] = 0
DESIGNED[(3, 8, 50258, F32, "few-threads")] = 1
CUR, MAX_LEN = 5, 8


def case_id(c):
    return f"{c[0]}x{c[1]}x{c[2]}-{str(c[3])[6:]}-{c[4]}"


def design(b, nb, V, dtype, mode):
    """(logits (b nb, V) float32 on the dtype's grid, score (b, nb) float32): random rows; under a nucleus every row also gets a few planted
    logits that hold nearly all of its mass, half a unit apart, so that the boundary falls into a wide gap of the cumulative mass.  One beam
    of sequence 1 is dead, and row 0 holds two equal logits among its largest (a tie in x: equal a, equal bits)."""
    g = np.random.default_rng(2000 + 7 * nb + V)
    x = torch.from_numpy((g.standard_normal((b * nb, V)) * 2).astype(np.float32)).to(dtype).float().numpy()
    score = -(g.integers(0, 64, (b, nb)) / 8.0).astype(np.float32)
    if WARPERS[mode][2] < 1.0:
        n = min(V // 2, 2 * nb + 4)
        for r in range(b * nb):
            cols = g.choice(V, n, replace=False)
            while True:                                                        # (jitter: no two rows share an lse; redrawn until the boundary's gap is wide)
                planted = (14.0 + 0.5 * g.permutation(n) + g.uniform(0, 0.25, n)).astype(np.float32)
                x[r, cols] = torch.from_numpy(planted).to(dtype).float().numpy()
                if r == 0:
                    x[0, np.argsort(-x[0])[1]] = x[0].max()                   # (the tie below, before the margin is judged)
                if BSC.keep_mask(x[r:r + 1], *WARPERS[mode])[1][0] >= 5 * MARGIN:
                    break
    if mode == "few-threads":
        x[:, 2000:] = -np.inf
    if nb > 1:
        score[1, nb - 1] = -np.inf
    top = np.argsort(-x[0])[:2]
    x[0, top[1]] = x[0, top[0]]
    return x, score


def restate(case, seed, ft=np.float64, eos=None):
    b, nb, V, dtype, mode = case
    x, score = design(b, nb, V, dtype, mode)
    st = BC.new_state(b, nb, MAX_LEN, 1.0, 1)
    st["score"][:] = score
    margin = BSC.step(st, x, BSC.noise(b * nb, V, seed, CUR), CUR, nb, eos, 1, False, *WARPERS[mode], ft=ft)
    return x, score, st, float(margin.min())


def seed_for(case, limit=64):
    """the search the table was made with (not run by the tests)"""
    return next(s for s in range(limit) if restate(case, s)[3] >= MARGIN)


@pytest.mark.parametrize("case", list(DESIGNED), ids=case_id)
def test_designed_seeds_are_decidable(case):
    """(no GPU) in float64 every gap among the best 2 nb + 1 values of p, every gap among the chosen a and every nucleus decision of the
    step is >= MARGIN, or an exact tie: what lets the GPU test below demand exact integer fields"""
    assert restate(case, DESIGNED[case])[3] >= MARGIN


@pytest.mark.gpu
@pytest.mark.parametrize("case", list(DESIGNED), ids=case_id)
def test_designed_steps_match_the_reference_exactly(case):
    """One step from a state with given scores, under the case's warpers: the whole state block afterwards equals the float64
    restatement's - integers exactly, scores within SCORE_BOUND.  The eos is the token of sequence 0's best drawn candidate, so a hypothesis
    is made.  State and workspace come from the guarded, poisoned seam."""
    from guarded import guarded_allocations
    from flamingo_mini_amd import functional as F
    b, nb, V, dtype, mode = case
    seed = DESIGNED[case]
    x, score, first, margin = restate(case, seed)
    assert margin >= MARGIN, "the designed step is not decidable"
    eos = int(first["next_tok"][0])
    with guarded_allocations() as g:
        st = F.BeamState(b, nb, MAX_LEN, "cuda", eos=eos, pad=1, early_stopping=False, length_penalty=1.0)
        poison(st)
        st.score.copy_(torch.from_numpy(score))
        pre = st.to_host()
        nxt, idx = F.beam_sample_step(torch.from_numpy(x).to(dtype).cuda(), st, dev_scalar(CUR), dev_scalar(seed), *WARPERS[mode])
        post = st.to_host()
        g.check()
    assert nxt.data_ptr() == st.next_tok.data_ptr() and idx.data_ptr() == st.beam_idx.data_ptr()
    ref = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in pre.items()}
    BSC.step(ref, x, BSC.noise(b * nb, V, seed, CUR), CUR, nb, eos, 1, False, *WARPERS[mode], ft=np.float64)
    worst = same_state(post, ref, where=case_id(case))
    print(f"MEASURED beam_sample_step score error {worst:.3e} (bound {SCORE_BOUND:.1e}) at {case_id(case)}; hypotheses {post['n_hyp'].tolist()}")
    assert int(post["n_hyp"][0]) >= 1


@pytest.mark.gpu
@pytest.mark.parametrize("nb,V,dtype", [(3, 300, BF16), (8, 50258, BF16), (4, 300, F32)], ids=lambda v: str(v).replace("torch.", ""))
def test_with_the_warpers_off_the_scores_are_those_of_beam_step_bit_for_bit(nb, V, dtype):
    """Every row holds two logits of 40 .. 44 over a background below 6, so every sequence has exactly 2 nb candidates whose a (>= 40 - 44 -
    log 2 - 2) lies more than 25 above all others (<= 6 - 40), and the noise spans less than 19.5: the draw must take those 2 nb, rule S6
    orders them by a, and the whole state block - every score bit - is what ff_beam_step leaves on the same input."""
    from flamingo_mini_amd import functional as F
    b = 3
    g = np.random.default_rng(31 + nb)
    x = torch.from_numpy(g.standard_normal((b * nb, V)).astype(np.float32)).to(dtype).float().numpy()
    assert x.max() < 6
    score = -(g.integers(0, 16, (b, nb)) / 8.0).astype(np.float32)
    for s in range(b):
        vals = 40.0 + 0.25 * g.permutation(2 * nb)
        for k in range(nb):
            x[s * nb + k, g.choice(V, 2, replace=False)] = vals[2 * k:2 * k + 2]
    blocks = []
    for sample in (False, True):
        st = F.BeamState(b, nb, MAX_LEN, "cuda", eos=int(np.argmax(x[0])), pad=1, early_stopping=False, length_penalty=1.0)
        poison(st)
        st.score.copy_(torch.from_numpy(score))
        dev = torch.from_numpy(x).to(dtype).cuda()
        if sample:
            F.beam_sample_step(dev, st, dev_scalar(CUR), dev_scalar(99))
        else:
            F.beam_step(dev, st, dev_scalar(CUR))
        blocks.append(st.storage.cpu())
    assert torch.equal(blocks[0], blocks[1])


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [BF16, F32], ids=["bf16", "f32"])
def test_a_nan_row_and_an_inf_row_leave_every_index_in_range(dtype):
    from guarded import guarded_allocations
    from flamingo_mini_amd import functional as F
    b, nb, V = 2, 3, 300
    x = torch.randn((b * nb, V), generator=torch.Generator().manual_seed(3)).to(dtype)
    x[1] = float("nan")
    x[4, 7] = float("inf")
    with guarded_allocations() as g:
        st = F.BeamState(b, nb, MAX_LEN, "cuda", eos=5, pad=1)
        st.score.zero_()
        F.beam_sample_step(x.cuda(), st, dev_scalar(CUR), dev_scalar(1), 0.9, 50, 0.9)
        host = st.to_host()
        g.check()
    assert ((host["next_tok"] >= 0) & (host["next_tok"] < V)).all()
    for s in range(b):
        r = slice(s * nb, (s + 1) * nb)
        assert ((host["beam_idx"][r] >= s * nb) & (host["beam_idx"][r] < (s + 1) * nb)).all()
        assert ((host["hist_parent"][CUR - 1, r] >= s * nb) & (host["hist_parent"][CUR - 1, r] < (s + 1) * nb)).all()


# ---------------------------------------------------------------------------------------------------------------------------------------
# 3. twelve scripted steps: the whole state after every step
# ---------------------------------------------------------------------------------------------------------------------------------------
MS_V, MS_NB, MS_EOS, MS_PAD, MS_MAXLEN = 300, 4, 7, 0, 14
MS_PROMPT = np.array([[1, 11], [2, 12], [3, 13]], np.int64)
MS_BOOST = {1: (4, 9.0), 2: (6, 5.5)}
MS_WARP = (0.9, 40, 1.0)
MS_SEEDS = {True: (4, 3), False: (4, 3)}     # (script table, kernel seed): runs that keep every margin and hold the events (both asserted on the way)


def scripted_run(early, table, seed, step_fn=None):
    """The search with the float64 restatement (or, with step_fn(pre-state, logits, cur_len) -> post-state, on the device: the restatement
    then advances a copy of every pre-state).  Returns (events, smallest margin, worst score error)."""
    script = BC.Script(MS_V, table, eos=MS_EOS, eos_boost=MS_BOOST)
    events, worst, err = {}, np.inf, 0.0
    hist = np.repeat(MS_PROMPT, MS_NB, axis=0)
    st = BC.new_state(3, MS_NB, MS_MAXLEN, 1.0, MS_PAD)
    for cur_len in range(3, MS_MAXLEN + 1):
        logits = script(hist)
        if step_fn is not None:
            st, post = step_fn(logits, cur_len)
        margin = BSC.step(st, logits, BSC.noise(3 * MS_NB, MS_V, seed, cur_len), cur_len, MS_NB, MS_EOS, MS_PAD, early, *MS_WARP, ft=np.float64, events=events)
        worst = min(worst, float(margin.min()))
        if step_fn is not None:
            assert margin.min() >= MARGIN, f"step {cur_len} of the script is not decidable"
            err = max(err, same_state(post, st, where=f"step {cur_len}"))
            st = post
        hist = np.concatenate([hist[st["beam_idx"]], st["next_tok"][:, None]], axis=1)
    return events, worst, err


def script_seeds_for(early, limit=40):
    """the search the table was made with (not run by the tests)"""
    for table in range(limit):
        for seed in range(4):
            ev, worst, _ = scripted_run(early, table, seed)
            if worst >= MARGIN and all(ev.get(k, 0) > 0 for k in ("eos_low", "eos_high", "done")):
                return table, seed


@pytest.mark.gpu
@pytest.mark.parametrize("early", [True, False])
def test_state_block_after_every_step_of_a_scripted_search(early):
    """12 steps, V = 300, 3 sequences x 4 beams, temperature 0.9 and top_k 40, eos at low and high ranks, a sequence done early.  Before every
    step the device state is copied; the float64 restatement advances the copy, and the device state after the step equals it as a WHOLE."""
    from guarded import guarded_allocations
    from flamingo_mini_amd import functional as F
    table, seed = MS_SEEDS[early]
    with guarded_allocations() as g:
        st = F.BeamState(3, MS_NB, MS_MAXLEN, "cuda", eos=MS_EOS, pad=MS_PAD, early_stopping=early, length_penalty=1.0)
        poison(st)
        cur, sd = dev_scalar(0), dev_scalar(seed)

        def on_device(logits, cur_len):
            pre = st.to_host()
            cur.fill_(cur_len)
            F.beam_sample_step(torch.from_numpy(logits).cuda(), st, cur, sd, *MS_WARP)
            return {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in pre.items()}, st.to_host()

        events, worst, err = scripted_run(early, table, seed, on_device)
        g.check()
    print(f"MEASURED multi-step beam sampling: score error {err:.3e}, smallest margin {worst:.3e}, events {events}")
    assert worst >= MARGIN
    assert events.get("eos_low", 0) > 0 and events.get("eos_high", 0) > 0 and events.get("done", 0) > 0, events


# ---------------------------------------------------------------------------------------------------------------------------------------
# 4. the law of the draw
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_the_device_draws_pairs_with_the_plackett_luce_law():
    """One launch, 8192 sequences of one beam over the same 8 logits: the unordered pair every sequence drew (the row's two candidates, which
    the step leaves in its workspace) is counted and held to the exact pair probabilities by a chi-square at the 1 - 1e-4 quantile of its
    27 degrees of freedom.  The seed is fixed."""
    from flamingo_mini_amd import functional as F
    b, V = 8192, 8
    x = np.array([1.25, 0.25, -0.5, 1.0, 0.0, 0.75, -0.75, 0.5], np.float32)  # (the rarest pair is expected 27 times)
    st = F.BeamState(b, 1, 4, "cuda")
    st.score.zero_()
    F.beam_sample_step(torch.from_numpy(np.tile(x, (b, 1))).cuda(), st, dev_scalar(2), dev_scalar(20260301))
    col = st.workspace[2 * b * 2 * 4:3 * b * 2 * 4].view(torch.int32).view(b, 2).cpu().numpy()
    assert (col[:, 0] != col[:, 1]).all() and ((col >= 0) & (col < V)).all()
    probs = BSC.pair_probabilities(x)
    pairs = list(probs)
    lo, hi = col.min(1), col.max(1)
    counts = [int(((lo == i) & (hi == j)).sum()) for i, j in pairs]
    chi, smallest = BSC.chi_square(counts, [probs[p] for p in pairs])
    print(f"MEASURED pair chi-square {chi:.2f} on 27 degrees of freedom (limit {BSC.CHI2_Q[27]}), smallest expected count {smallest:.1f}")
    assert smallest >= 20 and chi <= BSC.CHI2_Q[27]
    nxt = st.next_tok.cpu().numpy()                                           # rule S6: the next beam is the drawn candidate with the larger a
    assert np.array_equal(nxt, np.where(x[col[:, 0]] >= x[col[:, 1]], col[:, 0], col[:, 1]))


# ---------------------------------------------------------------------------------------------------------------------------------------
# 5. the beam-sampling decode session (G1 geometry of tests/test_hip_decode.py, batch 4, 3 beams)
# ---------------------------------------------------------------------------------------------------------------------------------------
NB, TAG = 3, "beam-sample"
SAMPLING = dict(temperature=0.9, top_k=40, top_p=1.0)


def gen_for(seed):
    return torch.Generator(device="cuda").manual_seed(seed)


def sample_generate(model, inputs, max_length, seed, graph=True, rec=None, **kw):
    ids, ml, am, vf = inputs
    model.decode_graph = graph
    with (rec.installed() if rec is not None else contextlib.nullcontext()):
        out = model.generate(ids, media_locations=ml, attention_mask=am, visual_features=vf, max_length=max_length, num_beams=NB, do_sample=True,
                             static_decode=True, generator=gen_for(seed), **{**SAMPLING, **kw})
    model.decode_graph = True
    return out


@pytest.fixture(scope="module")
def g1():
    import test_hip_decode as D
    model, model64 = D.models("gpt2")
    inputs = D.make_inputs(4, 1, TAG)
    model.reset_decode_sessions()
    yield D, model, inputs
    model.decode_graph = True
    model.reset_decode_sessions()
    D._MODELS.clear()


@pytest.fixture(scope="module")
def base_run(g1):
    """the replayed run, recorder installed: (GenerateOutput with NB sequences per prompt, recorded logits, host state, session, seed)"""
    from test_hip_sampling import _SampleRecorder
    D, model, inputs = g1
    rec = _SampleRecorder()
    out = sample_generate(model, inputs, D.MAXLEN, 11, rec=rec, num_return_sequences=NB, return_dict_in_generate=True)
    sess = rec.session
    return out, sess._rec.clone().cpu().numpy(), sess.state.to_host(), sess, int(sess.seed.item())


def replay(logits, seed, L0, length, fill):
    """The float64 restatement driven by the recorded logits and the session's seed: (final state, per sequence the smallest margin met)."""
    st = BC.new_state(4, NB, length, 1.0, fill)
    worst = np.full(4, np.inf)
    for pos in range(L0, length):
        worst = np.minimum(worst, BSC.step(st, logits[:, pos], BSC.noise(4 * NB, logits.shape[-1], seed, pos + 1), pos + 1, NB, None, fill, True,
                                           SAMPLING["temperature"], SAMPLING["top_k"], SAMPLING["top_p"], ft=np.float64))
    st["length"], st["eos"] = length, -1
    return st, worst


@pytest.mark.gpu
def test_session_replays_a_graph_and_every_step_follows_the_rules(g1, base_run):
    """A beam session with sampling exists and its graph runs; for every sequence whose steps were all decidable (margins >= MARGIN in the
    float64 restatement driven by the recorded logits and the session's seed) the history tables are the restatement's, and the returned
    sequences and scores are _beam_finalize of it."""
    from flamingo_mini_amd.modeling_flamingo import _beam_finalize
    D, model, inputs = g1
    out, logits, host, sess, seed = base_run
    assert sess.beams == (NB, True, 1.0) and sess.sampling == tuple(SAMPLING.values()) and sess.b == 4 * NB
    assert sess.replay is not None and not sess.capture_failed
    st, worst = replay(logits, seed, D.L0, D.MAXLEN, sess.fill)
    good = np.flatnonzero(worst >= MARGIN)
    print(f"MEASURED decidable sequences {len(good)} of 4; margins {worst.tolist()}")
    assert len(good) > 0, "no sequence with every step decidable"
    ids, scores = _beam_finalize(st, D.L0, inputs[0].cpu(), NB, sess.fill, n_return=NB)
    for s in good:
        r = slice(s * NB, (s + 1) * NB)
        for name in ("hist_tok", "hist_parent"):
            assert np.array_equal(host[name][D.L0:D.MAXLEN, r], st[name][D.L0:D.MAXLEN, r]), (s, name)
        assert np.abs(host["hist_score"][D.L0:D.MAXLEN, r].astype(np.float64) - st["hist_score"][D.L0:D.MAXLEN, r]).max() <= SCORE_BOUND
        assert torch.equal(out.sequences.cpu()[r], ids[r])
        torch.testing.assert_close(out.sequences_scores.cpu()[r], scores[r], rtol=0, atol=1e-4)
    assert bool((out.sequences_scores.view(4, NB)[:, :-1] >= out.sequences_scores.view(4, NB)[:, 1:]).all())


@pytest.mark.gpu
def test_eager_steps_equal_replayed_steps_and_the_seed_decides(g1, base_run):
    """decode_graph = False: the same ids, bit for bit; the same generator seed again and after the sessions were dropped and rebuilt: the
    same; another seed: other sequences"""
    D, model, inputs = g1
    kw = dict(num_return_sequences=NB)
    want = base_run[0].sequences
    eager = sample_generate(model, inputs, D.MAXLEN, 11, graph=False, **kw)
    sess = [s for s in model._decode_sessions.values() if s.beams is not None and s.sampling is not None and not s.graph_wanted]
    assert sess and sess[0].replay is None
    assert torch.equal(eager, want)
    assert torch.equal(sample_generate(model, inputs, D.MAXLEN, 11, **kw), want)
    other = sample_generate(model, inputs, D.MAXLEN, 12, **kw)
    assert other.shape[0] == want.shape[0] and not torch.equal(other, want)
    model.reset_decode_sessions()
    assert torch.equal(sample_generate(model, inputs, D.MAXLEN, 11, **kw), want)


@pytest.mark.gpu
def test_a_second_call_with_another_prompt_reuses_the_session(g1, base_run):
    from test_hip_sampling import _SampleRecorder
    D, model, inputs = g1
    other = D.make_inputs(4, 1, TAG + "-other")
    assert not torch.equal(other[0], inputs[0])
    rec, rec2 = _SampleRecorder(), _SampleRecorder()
    first = sample_generate(model, inputs, D.MAXLEN, 11, rec=rec, num_return_sequences=NB)
    out = sample_generate(model, other, D.MAXLEN, 11, rec=rec2)
    assert rec2.session is rec.session and rec.session.replay is not None
    assert out.shape == (4, D.MAXLEN) and torch.equal(out[:, :D.L0], other[0])
    assert torch.equal(first, base_run[0].sequences)


@pytest.mark.gpu
def test_static_result_equals_the_dynamic_loop_on_the_same_logits_and_noise(g1, base_run):
    """The dynamic loop (decoding.beam_search with sampling) is driven by the logits the session recorded, looked up by a row's token
    history, and by the KERNEL's noise (functional.beam_sample_noise under the session's seed): for every sequence whose steps were all
    decidable it returns the session's ids and scores.  (On logits and noise of its own the loop rightly chooses otherwise.)"""
    from flamingo_mini_amd import decoding as Dec
    from flamingo_mini_amd import functional as F
    D, model, inputs = g1
    out, logits, host, sess, seed = base_run
    _, worst = replay(logits, seed, D.L0, D.MAXLEN, sess.fill)
    good = np.flatnonzero(worst >= MARGIN)
    assert len(good) > 0, "no sequence with every step decidable"
    prompt = inputs[0].cpu()
    table = {}
    hist = np.repeat(prompt.numpy(), NB, axis=0)
    for pos in range(D.L0, D.MAXLEN):
        for r in range(4 * NB):
            table[tuple(hist[r])] = logits[r, pos]
        hist = np.concatenate([hist[host["hist_parent"][pos]], host["hist_tok"][pos][:, None]], axis=1)

    class Scripted(BC.ScriptedModel):
        def _decode_step(self, step_ids, ml, am, past, pixel_values, visual_features):
            h = step_ids if past is None else torch.cat([past[0][0][0], step_ids], dim=1)
            zero = np.zeros_like(logits[0, D.L0])
            x = np.stack([table.get(tuple(row), zero) for row in h.tolist()])          # (an unknown history: a sequence that left the recorded path)
            return torch.from_numpy(x), (((h, h),), ((h, h),))

    rows_of = (good[:, None] * NB + np.arange(NB)[None]).reshape(-1)

    def kernel_noise(rows, V, cur_len):                                      # the rows of the good sequences, under their own row numbers
        return F.beam_sample_noise(4 * NB, V, dev_scalar(seed), dev_scalar(cur_len)).cpu()[rows_of]

    ids = prompt[good]
    got_ids, got_s = Scripted(None).search(ids, torch.zeros_like(ids), torch.ones_like(ids), None, None, D.MAXLEN, NB, None, sess.fill, True, 1.0,
                                           n_return=NB, sampling=Dec.Sampling(*SAMPLING.values()), noise=kernel_noise)
    assert torch.equal(got_ids, out.sequences.cpu()[rows_of]), (good, got_ids.tolist(), out.sequences.cpu()[rows_of].tolist())
    torch.testing.assert_close(got_s, out.sequences_scores.cpu()[rows_of], rtol=0, atol=1e-4)


@pytest.mark.gpu
def test_beam_sampling_composes_with_processors_bad_words_a_trie_and_guidance(g1):
    """max_length 12 on a 5-token prompt: every combination runs on the static path, is reproducible per seed, and honours its rule."""
    D, model, _ = g1
    inputs = D.make_inputs(2, 1, TAG + "-mix", L0_=5)
    eos = D.VOCAB - 1
    kw = dict(eos_token_id=eos, pad_token_id=0, num_return_sequences=NB)
    run = lambda seed, **extra: sample_generate(model, inputs, 12, seed, **{**kw, **extra})
    plain = run(5)
    banned = sorted({int(t) for t in plain[:, 5:].flatten().tolist()} - {eos, 0})[:3]
    out = run(5, bad_words_ids=[[t] for t in banned], no_repeat_ngram_size=2, repetition_penalty=1.3)
    assert torch.equal(out, run(5, bad_words_ids=[[t] for t in banned], no_repeat_ngram_size=2, repetition_penalty=1.3))
    assert not any(t in banned for t in out[:, 5:].flatten().tolist())
    for row in out[:, 5:].tolist():
        live = row[:row.index(eos)] if eos in row else row                   # (a missing entry is all pad: nothing generated)
        grams = list(zip(live, live[1:])) if any(live) else []
        assert len(grams) == len(set(grams)), row
    cands = [[21, 22, 23], [21, 30], [40, 41, 42, 43], [50]]
    out = run(6, candidate_ids=cands, guidance_scale=1.5)
    assert torch.equal(out, run(6, candidate_ids=cands, guidance_scale=1.5))
    for row in out[:, 5:].tolist():
        if any(t != 0 for t in row):
            assert eos in row and row[:row.index(eos)] in cands, row
    sessions = [s for s in model._decode_sessions.values() if s.sampling is not None and s.beams is not None]
    assert sessions and all(s.replay is not None for s in sessions)
