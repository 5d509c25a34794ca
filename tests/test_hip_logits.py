"""Logits processors on the graph-replayed decode path, on the GPU: ff_logits_process (functional.process_logits, csrc/ff_logits.hip) against
the numpy restatement of its rules (tests/logits_cases.py) BIT FOR BIT over the whole rows x ld buffer on the designed cases, under graph
replay with device-side arguments, inside the greedy, sampling and beam _DecodeSession of FlamingoModel.generate(), and the dynamic loops of
generate() on GPU tensors (the torch restatement FlamingoModel._process_logits) against the same restatement, token for token.

Nothing here has a tolerance: rule 1 is one float32 product and one rounding, rules 2 and 3 write -inf, everything else keeps its bits.  In
the session tests a step is undecidable only when the two largest processed logits are exactly equal (greedy), under the EDGE rule of
tests/test_hip_sampling.py (sampling) or the margin rule of tests/test_hip_beam.py (beams); at most 5 % of the steps may be."""
import contextlib

import numpy as np
import pytest
import torch

import beam_cases as BC
import logits_cases as LC

BF16, F32 = torch.bfloat16, torch.float32
TORCH = {"bf16": (BF16, torch.int16, np.int16, np.uint16(0x7FA5)), "f32": (F32, torch.int32, np.int32, np.uint32(0x7FA5A5A5))}


def _launch(F, buf, off, V, hist, n, p, g, eos, min_len, hist_len_dev, min_len_dev, wide_hist=False):
    """one call on the view buf[:, off:off + V] with the history on the device (as a view of a wider buffer when wide_hist)"""
    hist_dev = torch.from_numpy(hist).cuda()
    if wide_hist:
        big = torch.full((hist.shape[0], hist.shape[1] + 3), 6, dtype=torch.long, device="cuda")      # (6: the trap token of most cases)
        big[:, :hist.shape[1]] = hist_dev
        hist_dev = big[:, :hist.shape[1]]
    hist_len_dev.fill_(n)
    if min_len is not None:
        min_len_dev.fill_(min_len)
    view = buf[:, off:off + V]
    out = F.process_logits(view, hist_dev, hist_len_dev, p, g, eos if eos >= 0 else None, min_len_dev if min_len is not None else None)
    assert out is view


@pytest.mark.gpu
@pytest.mark.parametrize("shape", LC.SHAPES, ids=lambda s: f"{s[0]}x{s[1]}-{s[2]}-{s[3]}")
def test_kernel_equals_the_restatement_bit_for_bit(shape):
    """Every n of N_VALUES x every setting (p, g, cap, eos, min_len) of that n: the WHOLE buffer - the view's rows, and for "last-of-2" the
    poisoned other half of every row - equals the restatement's bits.  The buffer comes from the guarded allocation seam; positions >= n of
    the history hold trap tokens; odd settings pass the history as a view with hist_ld > hist_cap."""
    from guarded import guarded_allocations
    from flamingo_mini_amd import functional as F
    rows, V, dtype, layout = shape
    tdt, idt, ndt, poison = TORCH[dtype]
    width = 2 * V if layout == "last-of-2" else V
    off = width - V
    hist_len_dev = torch.zeros(1, dtype=torch.long, device="cuda")
    min_len_dev = torch.zeros(1, dtype=torch.long, device="cuda")
    bad, launches, moved = [], 0, 0
    with guarded_allocations() as guards:
        buf = F._new((rows, width), tdt, "cuda")
        cases = [(n, k, s, n) for n in LC.N_VALUES for k, s in enumerate(LC.settings(n))]
        cases += [(64, 1, (LC.P, 2, 64, 1, 70), 64 + 5), (64, 2, (LC.P, 2, 64, 1, 70), -4)]      # *hist_len outside [0, cap]: clamped
        for n, k, (p, g, cap, eos, min_len), hist_len in cases:
            bits, hist = LC.make_case(rows, V, dtype, n, cap, g, seed=1000 * n + 10 * k + rows)
            full = np.full((rows, width), poison, bits.dtype)
            full[:, off:] = bits
            buf.view(idt).copy_(torch.from_numpy(full.view(ndt)).cuda())
            _launch(F, buf, off, V, hist, hist_len, p, g, eos, min_len, hist_len_dev, min_len_dev, wide_hist=k % 2 == 1)
            got = buf.view(idt).cpu().numpy().view(bits.dtype)
            want = full.copy()
            want[:, off:] = LC.restate(bits, V, hist, hist_len, p=p, g=g, eos=eos, min_len=min_len, dtype=dtype)
            launches += 1
            if not np.array_equal(got, want):
                r, c = np.argwhere(got != want)[0]
                bad.append((n, p, g, cap, eos, min_len, int(r), int(c) - off, hex(int(got[r, c])), hex(int(want[r, c])), int((got != want).sum())))
            moved += not np.array_equal(want, full)
        guards.check()
    assert not bad, f"{len(bad)} of {launches} (n, p, g, cap, eos, min_len, row, column, got, want, count): {bad[:6]}"
    assert moved >= launches // 2, f"only {moved} of {launches} designed calls change anything"


@pytest.mark.gpu
def test_replay_follows_device_side_history_and_lengths():
    """captured once; then the history's contents, *hist_len and *min_len change on the device and the replay follows them"""
    from flamingo_mini_amd import functional as F
    rows, V, cap, dtype = 3, 320, 96, "bf16"
    tdt, idt, ndt, _ = TORCH[dtype]
    buf = torch.zeros((rows, V), dtype=tdt, device="cuda")
    hist_dev = torch.zeros((rows, cap), dtype=torch.long, device="cuda")
    hist_len_dev = torch.zeros(1, dtype=torch.long, device="cuda")
    min_len_dev = torch.zeros(1, dtype=torch.long, device="cuda")
    call = lambda: F.process_logits(buf, hist_dev, hist_len_dev, LC.P, 2, 1, min_len_dev)
    call()
    graph = torch.cuda.CUDAGraph()
    torch.cuda.synchronize()
    with torch.cuda.graph(graph):
        call()
    for n, min_len, seed in ((65, 66, 1), (17, 17, 2), (96, 200, 3), (0, 0, 4)):
        bits, hist = LC.make_case(rows, V, dtype, n, cap, 2, seed=seed)
        buf.view(idt).copy_(torch.from_numpy(bits.view(ndt)).cuda())
        hist_dev.copy_(torch.from_numpy(hist).cuda())
        hist_len_dev.fill_(n)
        min_len_dev.fill_(min_len)
        graph.replay()
        want = LC.restate(bits, V, hist, n, p=LC.P, g=2, eos=1, min_len=min_len, dtype=dtype)
        assert np.array_equal(buf.view(idt).cpu().numpy().view(bits.dtype), want), (n, min_len)
        assert (n == 0) == np.array_equal(want, bits)


# ---------------------------------------------------------------------------------------------------------------------------------------
# the decode sessions (G1 geometry of tests/test_hip_decode.py, batch 4)
# ---------------------------------------------------------------------------------------------------------------------------------------
TAG = "logits"
PROC = dict(repetition_penalty=1.3, no_repeat_ngram_size=2)
MIN_NEW = 6                       # min_length = L0 + MIN_NEW


@pytest.fixture(scope="module")
def g1():
    import test_hip_decode as D
    model, _ = D.models("gpt2")
    inputs = D.make_inputs(4, 1, TAG)
    model.reset_decode_sessions()
    dtype = {BF16: "bf16", F32: "f32"}[next(model.parameters()).dtype]
    yield D, model, inputs, dtype
    model.decode_graph = True
    model.reset_decode_sessions()
    D._MODELS.clear()


def generate(model, inputs, max_length, graph=True, rec=None, **kw):
    ids, ml, am, vf = inputs
    model.decode_graph = graph
    with (rec.installed() if rec is not None else contextlib.nullcontext()):
        out = model.generate(ids, media_locations=ml, attention_mask=am, visual_features=vf, max_length=max_length, **kw)
    model.decode_graph = True
    return out


@pytest.fixture(scope="module")
def plain(g1):
    D, model, inputs, _ = g1
    return generate(model, inputs, D.MAXLEN)


def processed(raw, dtype, hist, **kw):
    return LC.restate_values(raw, dtype, np.asarray(hist, np.int64), np.asarray(hist).shape[1], **kw)


def repeated_bigrams(row, L0):
    """generated positions whose bigram (row[i - 1], row[i]) occurred earlier in the row"""
    return [i for i in range(L0, len(row)) if (row[i - 1], row[i]) in set(zip(row[:i - 1], row[1:i]))]


@pytest.mark.gpu
def test_greedy_session_with_unigram_ban_never_repeats_a_token(g1):
    D, model, inputs, _ = g1
    out = generate(model, inputs, D.MAXLEN, no_repeat_ngram_size=1)
    sess = [s for s in model._decode_sessions.values() if s.processors == (1.0, 1, 0, 0)]
    assert sess and sess[0].replay is not None and not sess[0].capture_failed and not hasattr(sess[0], "seq_buf")
    assert out.shape == (4, D.MAXLEN) and torch.equal(out[:, :D.L0], inputs[0])
    for row in out.cpu().tolist():
        new = row[D.L0:]
        assert len(set(new)) == len(new) and not set(new) & set(row[:D.L0]), row
    assert torch.equal(out, generate(model, inputs, D.MAXLEN, graph=False, no_repeat_ngram_size=1))


@pytest.mark.gpu
def test_greedy_session_follows_the_rules_step_for_step(g1, plain):
    """p = 1.3, g = 2, min_length = L0 + 6 with eos = the token the unconstrained run emits first in row 0: every step's token is the argmax of
    the restatement applied to the RECORDED raw logits and the row's own history (a step whose two largest processed values are exactly
    equal is undecidable); no row holds eos before index min_length; eager steps give the same ids bit for bit."""
    from test_hip_sampling import _SampleRecorder
    D, model, inputs, dtype = g1
    eos = int(plain[0, D.L0])
    pad = 0 if eos != 0 else 1
    min_len = D.L0 + MIN_NEW
    kw = dict(PROC, min_length=min_len, eos_token_id=eos, pad_token_id=pad)
    rec = _SampleRecorder()
    out = generate(model, inputs, D.MAXLEN, rec=rec, **kw)
    sess = rec.session
    assert sess.processors == (1.3, 2, min_len, 0) and sess.min_on and int(sess.min_len) == min_len
    assert sess.replay is not None and not sess.capture_failed
    assert torch.equal(out[:, :D.L0], inputs[0]) and not torch.equal(out, plain[:, :out.shape[1]])
    raw, ids = sess._rec.clone().cpu().numpy(), out.cpu().numpy()
    undecidable, bad, total = 0, [], 0
    alive = np.ones(4, bool)
    for pos in range(D.L0, ids.shape[1]):
        x = processed(raw[:, pos], dtype, ids[:, :pos], p=1.3, g=2, eos=eos, min_len=min_len)
        for r in np.flatnonzero(alive):
            total += 1
            top = np.sort(x[r])[-2:]
            if top[0] == top[1]:
                undecidable += 1
            elif int(np.argmax(x[r])) != ids[r, pos]:
                bad.append((int(r), pos, int(ids[r, pos]), int(np.argmax(x[r]))))
        alive &= ids[:, pos] != eos
    print(f"MEASURED greedy-with-processors undecidable {undecidable} of {total}")
    assert not bad, f"(row, position, got, want): {bad[:8]}"
    assert undecidable <= 0.05 * total
    assert not (ids[:, D.L0:min_len] == eos).any(), "eos generated before min_length"      # (the prompt may hold the token)
    for r in range(4):
        row = ids[r, D.L0:].tolist()
        if eos in row:
            assert all(t == pad for t in row[row.index(eos) + 1:]), row
    assert torch.equal(out, generate(model, inputs, D.MAXLEN, graph=False, **kw))
    # min_new_tokens counts from the prompt: the same bound through the other argument, another session, the same ids
    also = generate(model, inputs, D.MAXLEN, **dict(PROC, min_new_tokens=MIN_NEW, eos_token_id=eos, pad_token_id=pad))
    assert torch.equal(also, out)


@pytest.mark.gpu
def test_sampling_session_draws_from_the_processed_logits(g1):
    """the float64 reference of tests/test_hip_sampling.py on the restatement's output and the session's own random numbers, under its EDGE rule"""
    from test_hip_sampling import EDGE, SAMPLING, Ref, _SampleRecorder
    D, model, inputs, dtype = g1
    kw = dict(SAMPLING, do_sample=True, static_decode=True, **PROC)
    rec = _SampleRecorder()
    out = generate(model, inputs, D.MAXLEN, rec=rec, generator=torch.Generator(device="cuda").manual_seed(1), **kw)
    sess = rec.session
    assert sess.sampling == (0.8, 20, 0.9) and sess.processors == (1.3, 2, 0, 0) and sess.replay is not None and not sess.capture_failed
    raw, u_all, ids = sess._rec.clone().cpu().numpy(), sess.u_all.clone().cpu().numpy(), out.cpu().numpy()
    T, k, p = sess.sampling
    undecidable, bad = 0, []
    for pos in range(D.L0, D.MAXLEN):
        x = processed(raw[:, pos], dtype, ids[:, :pos], p=1.3, g=2).astype(np.float64)
        for r in range(4):
            ref = Ref(x[r], T, k)
            P, _, c = ref.cdf(p)
            u = float(u_all[pos, r])
            if np.abs(np.concatenate([[0.0], c[P]]) - u).min() < EDGE or np.abs(ref.above - p).min() < EDGE:
                undecidable += 1
            elif ref.token(p, u) != ids[r, pos]:
                bad.append((r, pos, int(ids[r, pos]), ref.token(p, u)))
    total = 4 * (D.MAXLEN - D.L0)
    print(f"MEASURED sampling-with-processors undecidable {undecidable} of {total}")
    assert not bad, f"(row, position, got, want): {bad[:8]}"
    assert undecidable <= 0.05 * total
    for row in ids.tolist():
        assert not repeated_bigrams(row, D.L0), row
    eager = generate(model, inputs, D.MAXLEN, graph=False, generator=torch.Generator(device="cuda").manual_seed(1), **kw)
    assert torch.equal(eager, out)


@pytest.mark.gpu
def test_beam_session_bans_bigrams_along_every_beam(g1):
    """3 beams, g = 2.  The histories are rebuilt from hist_parent; every decidable step's chosen (token, parent) lists equal
    beam_cases.candidates on the PROCESSED logits (float64, the margin rule of tests/test_hip_beam.py); the returned ids are _beam_finalize of
    the restatement driven by the processed logits; no bigram ending at a generated position repeats an earlier one; eager equals replayed."""
    from flamingo_mini_amd.modeling_flamingo import _beam_finalize
    from test_hip_beam import NB, SCORE_BOUND, beam_generate, gaps_decidable
    from test_hip_sampling import _SampleRecorder
    D, model, inputs, dtype = g1
    rec = _SampleRecorder()
    out = beam_generate(model, inputs, D.MAXLEN, rec=rec, no_repeat_ngram_size=2)
    sess = rec.session
    assert sess.beams == (NB, True, 1.0) and sess.processors == (1.0, 2, 0, 0) and sess.seq_buf.shape == (4 * NB, D.MAXLEN)
    assert sess.replay is not None and not sess.capture_failed
    raw, host = sess._rec.clone().cpu().numpy(), sess.state.to_host()
    hist = np.repeat(inputs[0].cpu().numpy(), NB, axis=0)
    st = BC.new_state(4, NB, sess.max_length, 1.0, sess.fill)
    undecidable, bad, worst, banned = 0, [], 0.0, 0
    for pos in range(D.L0, D.MAXLEN):
        x = processed(raw[:, pos], dtype, hist, g=2)
        assert not np.isnan(x).any()
        banned += int(np.isinf(x).sum())
        prev = BC.new_state(4, NB, 1)["score"] if pos == D.L0 else host["hist_score"][pos - 1].reshape(4, NB)
        top_s, top_b, top_t = BC.candidates(prev, x, NB, np.float64)
        ok, _ = gaps_decidable(top_s, top_b)
        for s in range(4):
            r = slice(s * NB, (s + 1) * NB)
            if not ok[s]:
                undecidable += 1
            elif (host["hist_tok"][pos, r].tolist(), host["hist_parent"][pos, r].tolist()) != (top_t[s, :NB].tolist(), (s * NB + top_b[s, :NB]).tolist()):
                bad.append((s, pos, host["hist_tok"][pos, r].tolist(), top_t[s, :NB].tolist()))
            else:
                worst = max(worst, float(np.abs(host["hist_score"][pos, r].astype(np.float64) - top_s[s, :NB]).max()))
        BC.step(st, x, pos + 1, NB, None, sess.fill, True)
        hist = np.concatenate([hist[host["hist_parent"][pos]], host["hist_tok"][pos][:, None]], axis=1)
    total = 4 * (D.MAXLEN - D.L0)
    print(f"MEASURED beams-with-processors undecidable {undecidable} of {total}; score error {worst:.3e}; entries banned {banned}")
    assert not bad, f"(sequence, position, got, want): {bad[:4]}"
    assert worst <= SCORE_BOUND and undecidable <= 0.05 * total
    assert np.array_equal(sess.seq_buf.cpu().numpy(), hist), "seq_buf did not follow the beams"
    st["length"], st["eos"] = D.MAXLEN, -1
    assert torch.equal(out.cpu(), _beam_finalize(st, D.L0, inputs[0].cpu(), NB, sess.fill))
    for row in out.cpu().tolist():
        assert not repeated_bigrams(row, D.L0), row
    assert torch.equal(out, beam_generate(model, inputs, D.MAXLEN, graph=False, no_repeat_ngram_size=2))


# ---------------------------------------------------------------------------------------------------------------------------------------
# the dynamic loops on GPU tensors (the tiny fp32 models of tests/test_model_plumbing.py): the torch restatement inside generate()
# ---------------------------------------------------------------------------------------------------------------------------------------
DYN = dict(repetition_penalty=1.3, no_repeat_ngram_size=2, min_length=8)


def restated_loop(model, ids, kw, eos, choose):
    """the dynamic loop from its parts: _decode_step, the numpy restatement on the float32 logits, `choose`, the eos bookkeeping"""
    seq, ml, am, past, step = ids, kw["media_locations"], kw["attention_mask"], None, ids
    finished = torch.zeros(ids.shape[0], dtype=torch.bool, device=ids.device)
    with torch.no_grad():
        while seq.shape[1] < kw["max_length"]:
            logits, past = model._decode_step(step, ml, am, past, kw["pixel_values"], None)
            assert logits.dtype == torch.float32
            x = LC.restate_values(logits.cpu().numpy(), "f32", seq.cpu().numpy(), seq.shape[1], p=DYN["repetition_penalty"],
                                  g=DYN["no_repeat_ngram_size"], eos=eos, min_len=DYN["min_length"])
            nxt = choose(torch.from_numpy(x).to(ids.device))
            nxt = torch.where(finished, torch.full_like(nxt, 0), nxt)
            finished = finished | (nxt == eos)
            seq = torch.cat([seq, nxt[:, None]], 1)
            ml = torch.cat([ml, torch.zeros_like(ml[:, :1])], 1)
            am = torch.cat([am, torch.ones_like(am[:, :1])], 1)
            step = seq[:, -1:]
            if bool(finished.all()):
                break
    return seq


@pytest.mark.gpu
@pytest.mark.parametrize("family", ["gpt2", "opt"])
def test_dynamic_loops_on_gpu_tensors_apply_the_rules(family):
    """static_decode=False greedy and default-routed sampling equal the loop restated from _decode_step parts with the numpy restatement,
    token for token (eos = the token the unconstrained run emits first in row 0: banned up to min_length = 8, so the run differs from the
    plain one); default-routed beam search with a unigram ban returns rows without a repeated token; int32 ids with processors take the
    dynamic loop; none of it builds a session."""
    from test_model_plumbing import build
    model, z = build(torch.float32, "cuda", family)
    model.eval()
    px = torch.from_numpy(z["px"]).float().cuda()
    ids, ml = torch.from_numpy(z["ids"]).cuda()[:, :4], torch.from_numpy(z["ml"]).cuda()[:, :4]
    kw = dict(media_locations=ml, attention_mask=torch.ones_like(ids), pixel_values=px, max_length=10)
    plain = model.generate(ids, static_decode=False, **kw)
    eos = int(plain[0, 4])
    got = model.generate(ids, eos_token_id=eos, pad_token_id=0, static_decode=False, **DYN, **kw)
    want = restated_loop(model, ids, kw, eos, lambda x: x.argmax(-1))
    assert torch.equal(got, want), (got, want)
    assert not (got[:, 4:8] == eos).any() and not torch.equal(got[:, :plain.shape[1]], plain[:, :got.shape[1]])
    sk = dict(do_sample=True, temperature=0.7, top_k=20, top_p=0.9)
    got = model.generate(ids, eos_token_id=eos, pad_token_id=0, generator=torch.Generator(device="cuda").manual_seed(3), **sk, **DYN, **kw)
    g = torch.Generator(device="cuda").manual_seed(3)
    want = restated_loop(model, ids, kw, eos, lambda x: torch.multinomial(model._filter_logits(x, 0.7, 20, 0.9).softmax(-1), 1, generator=g)[:, 0])
    assert torch.equal(got, want), (got, want)
    beams = model.generate(ids, num_beams=3, no_repeat_ngram_size=1, **kw)
    small = model.generate(ids.int(), no_repeat_ngram_size=1, **kw)
    assert beams.shape == small.shape == (2, 10)
    for row in beams.cpu().tolist() + small.cpu().tolist():
        assert len(set(row[4:])) == len(row[4:]) and not set(row[4:]) & set(row[:4]), row
    assert len(model._decode_sessions) == 0
